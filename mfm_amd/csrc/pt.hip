// Parallel tempering (replica exchange): mfm_pt_run and mfm_pt_exchange.  K temperatures x R independent ladders: chain b = r * K + k
// is slot k of ladder r and runs at betas[k] with step size step_sizes[k]; slot 0 is the one that is kept.  include/mfm.h states the
// round and the key schedule, tests/pt_ref.py restates both in float64.
//
// One round is two or three launches on the context's stream; the host only enqueues:
//   1. pt_hmc_run_kernel / pt_mala_run_kernel: hmc_run_kernel's / mala_run_kernel's lines (one wave per chain, the chain resident in
//      registers over the round's n_local steps) with beta and eps WAVE-UNIFORM, read once per wave from the two small device arrays,
//      on the shared hmc_trajectory / mala_resident_step: chain b has the bits of mfm_hmc_run / mfm_mala_run at the scalars
//      (betas[b % K], step_sizes[b % K]) on the round's key.  The tallies ADD to n_acc[b] / acc_sum[b] (per slot, i.e. per temperature).
//   2. pt_exchange_kernel: ONE WAVE PER PAIR (i, j = i + 1) of the sweep's parity.  The wave holds both rows in registers, stages x_j
//      in its own LDS row and evaluates it at beta_i, then x_i at beta_j -- row_value_grad, so each candidate carries the bits
//      mfm_mala_init gives for that position and beta -- and decides by Metropolis on the joint.  On accept it stores the two rows
//      swapped, each with the candidate log-density and gradient evaluated at its own beta.  The pairs of one parity are disjoint, a
//      wave reads and writes its own two rows and its own tally entries only: no atomics, no flags, no workgroup waits on another, and
//      a pair that straddles two workgroups of the run kernel is a pair like any other.  Slots without a partner have no wave.
//   3. pt_traj_kernel (rounds the trajectory keeps): slot 0 of every ladder to d_traj_pos / d_traj_logp.
// (Included by api.hip after chees.hip: HmcRunArgs, MalaRunArgs, HmcResident, MalaResident, hmc_trajectory, mala_resident_step,
// row_value_grad, ROW_DISPATCH and resident.hip.h's helpers.)
#pragma once

#define PT_MAX_TEMPS 64

// the ladder, in device memory: [0, K) the betas, [PT_MAX_TEMPS, PT_MAX_TEMPS + K) the step sizes
struct PtVec { double v[PT_MAX_TEMPS]; };
__global__ void pt_ladder_kernel(PtVec betas, PtVec eps, int K, double* out) {
  const int k = threadIdx.x;
  if (blockIdx.x || k >= K) return;
  out[k] = betas.v[k];
  out[PT_MAX_TEMPS + k] = eps.v[k];
}

// what the tempered run kernels take beside the run arguments (whose beta / eps they do not read)
struct PtLocal {
  const double* betas;       // [K]
  const double* eps;         // [K]
  int K;
  int32_t* n_acc;            // [B] += the round's accepted steps (may be null)
  double* acc_sum;           // [B] += the round's sum of acceptance probabilities (may be null)
};

template <int MAXIT, bool BCRT = false>
__global__ __launch_bounds__(MALA_WAVES * 64) void pt_hmc_run_kernel(HmcRunArgs r, PtLocal p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const HmcArgs& a = r.h;
  const int d = a.T.dim, lane = threadIdx.x & 63, b = resident_chain_index();      // (own scalars: resident.hip.h says why)
  if (b >= a.B) return;
  const ResidentChain c(smem, d, a.B, lane, b);
  float* const xs = c.xs; float* const gsm = c.gsm; const size_t row = c.row;
  const int k = b % p.K;
  const double beta = p.betas[k], eps = p.eps[k];         // wave-uniform: the chains of a wave's slot share them

  float x[MAXIT], g[MAXIT];                               // (in line, as hmc_run_kernel: resident.hip.h)
  double lp = a.logp[b];
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    x[it] = 0.f; g[it] = 0.f;
    if (j < d) { x[it] = a.pos[row + j]; g[it] = a.grad[row + j]; }
  }
  c.pads();
  const Key2 kc = run_chain_key(c, a, r.t);
  int n_acc = 0;
  double acc_sum = 0.0;

  for (int s = 0; s < r.t.n_steps; ++s) {
    const Key2 kb = run_step_key(c, a, r.t, kc, s);
    HmcResident<MAXIT> st{x, g, lp, false, 0.0};
    hmc_trajectory<MAXIT, BCRT, false>(a.T, beta, eps, a.num_steps, kb, d, lane, xs, gsm, nullptr, st, HmcCalled());
    n_acc += st.acc ? 1 : 0;
    acc_sum += st.pa;
    resident_step_end();
  }

#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {                    // (the final store stays in line: resident.hip.h)
    const int j = lane + 64 * it;
    if (j < d) { a.pos[row + j] = x[it]; a.grad[row + j] = g[it]; }
  }
  if (lane == 0) {
    a.logp[b] = lp;
    if (p.n_acc) p.n_acc[b] += n_acc;
    if (p.acc_sum) p.acc_sum[b] += acc_sum;
  }
}

template <int MAXIT, bool BCRT = false>
__global__ __launch_bounds__(MALA_WAVES * 64) void pt_mala_run_kernel(MalaRunArgs r, PtLocal p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const MalaArgs& a = r.m;
  const int d = a.T.dim, lane = threadIdx.x & 63, b = resident_chain_index();
  if (b >= a.B) return;
  const ResidentChain c(smem, d, a.B, lane, b);
  float* const xs = c.xs; float* const gsm = c.gsm; const size_t row = c.row;
  const int k = b % p.K;
  const double beta = p.betas[k], eps = p.eps[k];

  ResidentState<MAXIT> cs = resident_load<MAXIT>(c, a);
  float (&x)[MAXIT] = cs.x; float (&g)[MAXIT] = cs.g; double& lp = cs.lp;
  c.pads();
  float xn[MAXIT];
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) xn[it] = 0.f;
  const Key2 kc = run_chain_key(c, a, r.t);
  const double s2e = mala_s2e(eps);
  int n_acc = 0;
  double acc_sum = 0.0;

  for (int s = 0; s < r.t.n_steps; ++s) {
    const Key2 kb = run_step_key(c, a, r.t, kc, s);
    MalaResident<MAXIT> st{x, g, lp, xn, false, 0.0, 0.0, 0.0};
    mala_resident_step<MAXIT, BCRT>(a.T, beta, eps, s2e, a.textbook, kb, d, lane, xs, gsm, st);
    n_acc += st.acc ? 1 : 0;
    acc_sum += st.p;
    resident_step_end();
  }

#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    if (j < d) { a.pos[row + j] = x[it]; a.grad[row + j] = g[it]; }
  }
  if (lane == 0) {
    a.logp[b] = lp;
    if (p.n_acc) p.n_acc[b] += n_acc;
    if (p.acc_sum) p.acc_sum[b] += acc_sum;
  }
}

// ---- the exchange sweep ---------------------------------------------------------------------------------------------------------------
struct PtSwap {
  const double* betas;       // [K]
  int K, parity, pairs;      // pairs = (K - parity) / 2 per ladder: the lower slots parity, parity + 2, ...
  Key2 key;                  // the sweep's key: the pair whose lower slot is chain i draws from split(key, n_total)[chain_offset + i]
  uint32_t n_total, chain_offset;
  float* pos; double* logp; float* grad;        // state, swapped in place
  int32_t* replica;          // [B] (may be null)
  int32_t* swap_accepted;    // [R][K - 1] (may be null)
  double* swap_prob;         // [R][K - 1] (may be null)
};

// a.B is the number of PAIRS (ROW_DISPATCH sizes the grid from it); a.T the target; nothing else of `a` is read
template <int MAXIT, bool BCRT = false>
__global__ __launch_bounds__(MALA_WAVES * 64) void pt_exchange_kernel(MalaArgs a, PtSwap s) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int d = a.T.dim, lane = threadIdx.x & 63, q = resident_chain_index();
  if (q >= a.B) return;
  const ResidentChain c(smem, d, a.B, lane, q);
  float* const xs = c.xs; float* const gsm = c.gsm;
  const int ladder = q / s.pairs, k = s.parity + 2 * (q - ladder * s.pairs);
  const int i = ladder * s.K + k, j = i + 1;
  const size_t ri = (size_t)i * d, rj = (size_t)j * d;
  const double bi = s.betas[k], bj = s.betas[k + 1];

  float xi[MAXIT], xj[MAXIT], gi[MAXIT], gj[MAXIT];       // gi: the gradient of x_j at beta_i, what slot i holds after a swap
  const double lpi = s.logp[i], lpj = s.logp[j];
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int e = lane + 64 * it;
    xi[it] = 0.f; xj[it] = 0.f; gi[it] = 0.f; gj[it] = 0.f;
    if (e < d) { xi[it] = s.pos[ri + e]; xj[it] = s.pos[rj + e]; xs[e] = xj[it]; }
  }
  c.pads();
  resident_step_end();                                     // the stencil reads its neighbours' elements from this wave's row
  const double ci = __shfl(row_value_grad<MAXIT, BCRT>(a.T, bi, xs, d, lane, gi, gsm), 0, 64);      // (lane 0's: the value mfm_mala_init stores)
  resident_step_end();                                     // (the row and the mixtures' scratch are overwritten next)
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int e = lane + 64 * it;
    if (e < d) xs[e] = xi[it];
  }
  resident_step_end();
  const double cj = __shfl(row_value_grad<MAXIT, BCRT>(a.T, bj, xs, d, lane, gj, gsm), 0, 64);

  double pacc;
  {
#pragma clang fp contract(off)
    const double delta = (ci + cj) - (lpi + lpj);          // Metropolis on the joint: every operation rounded on its own
    pacc = mala_accept_p(delta);
  }
  const Key2 kp = split_at(s.key, s.n_total, s.chain_offset + (uint32_t)i);
  const bool acc = uniform01(kp, 0, 1) < pacc;
  if (acc) {
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int e = lane + 64 * it;
      if (e < d) {
        s.pos[ri + e] = xj[it]; s.grad[ri + e] = gi[it];
        s.pos[rj + e] = xi[it]; s.grad[rj + e] = gj[it];
      }
    }
  }
  if (lane == 0) {
    if (acc) {
      s.logp[i] = ci; s.logp[j] = cj;
      if (s.replica) { const int32_t t = s.replica[i]; s.replica[i] = s.replica[j]; s.replica[j] = t; }
    }
    const size_t e = (size_t)ladder * (s.K - 1) + k;       // owned by this wave alone in this sweep
    if (s.swap_accepted) s.swap_accepted[e] += acc ? 1 : 0;
    if (s.swap_prob) s.swap_prob[e] += pacc;
  }
}

// slot 0 of every ladder after a round: traj_pos[snap][r][:] / traj_logp[snap][r]
__global__ __launch_bounds__(256) void pt_traj_kernel(const float* pos, const double* logp, int K, int R, int d, float* traj_pos, double* traj_logp) {
  const int r = blockIdx.x;
  if (r >= R) return;
  const size_t src = (size_t)r * K * d, dst = (size_t)r * d;
  if (traj_pos)
    for (int e = threadIdx.x; e < d; e += 256) traj_pos[dst + e] = pos[src + e];
  if (traj_logp && threadIdx.x == 0) traj_logp[r] = logp[(size_t)r * K];
}

int launch_pt_hmc_run(const HmcRunArgs& r, const PtLocal& p, hipStream_t stream) {
  const HmcArgs& a = r.h;
  MALA_DISPATCH(pt_hmc_run_kernel, r, p);
  return 0;
}
int launch_pt_mala_run(const MalaRunArgs& r, const PtLocal& p, hipStream_t stream) {
  const MalaArgs& a = r.m;
  MALA_DISPATCH(pt_mala_run_kernel, r, p);
  return 0;
}
// one sweep; a parity without a pair (K = 2, parity 1) launches nothing
int launch_pt_exchange(const MalaArgs& a, const PtSwap& s, hipStream_t stream) {
  if (a.B <= 0) return 0;
  MALA_DISPATCH(pt_exchange_kernel, a, s);
  return 0;
}
