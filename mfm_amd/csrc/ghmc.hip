// Generalized HMC with persistent momentum over parallel chains, one wavefront per chain (mfm_ghmc_init / _step / _step_keys / _run) -- a
// BUILD-SIDE MODE beside hmc.hip: Horowitz 1991 with the non-reversible slice accept of Neal 2020, as Hoffman & Sountsov 2022 (MEADS)
// run it (blackjax.ghmc), restated in float64 in tests/ghmc_ref.py.  A chain is the MALA state (x, log p(x), g = grad log p(x) of the
// tempered density), a momentum p and a slice variable s in (-1, 1).  One transition with the chain key kb, step size eps, refresh rate
// alpha in (0, 1], slice drift delta >= 0 and the diagonal inverse mass minv:
//   1. p <- sqrt(1 - alpha) p + sqrt(alpha) n / sqrt(minv), n_j = normal64(mcmc_step_key(kb, MCMC_K_INT), j, d): hmc_trajectory's draw
//   2. s <- fmod(s + 1 + delta, 2) - 1 (deterministic)
//   3. H_0 = -logp + 1/2 sum minv p^2
//   4. ONE velocity-Verlet step, the lines of one iteration of hmc_trajectory's loop: half kick, drift x <- (float)(x + eps minv p),
//      value and gradient, half kick
//   5. H_1 likewise, dH = H_1 - H_0
//   6. accept iff |s| <= exp(-dH), a NaN dH rejecting.  Accepted: the state becomes the end point, p <- p_end, s <- s exp(dH).
//      Rejected: x, logp, g are kept, p <- -p (the REFRESHED momentum, negated), s is kept.
//   7. info: acceptance_rate = min(1, exp(-dH)) (mala_accept_p), is_accepted, energy_change = dH
// |s| <= exp(-dH) is decided as |s| <= min(1, exp(-dH)), the acceptance rate: |s| <= 1 always, so the two agree for every s and dH.
// At alpha = 1 the refresh is 0 p + 1 n: the proposal and the acceptance rate have the bits of hmc_step_kernel at num_steps = 1 on the
// same keys, unit and MASS (every product with minv is written as hmc_trajectory writes it; minv == 1 gives the unit instances' bits).
// Layout as mclmc.hip: positions / gradients float32, log-density float64, momentum float64 in registers AND in HBM ([B][d]), the slice
// variable float64 [B]; energies are float64 sums over the wave; every operation is rounded on its own.
// Targets: phi-four and the Gaussian mixtures (row_value_grad).  The inverse mass is the CALL's argument (GhmcArgs::minv, null: unit
// metric); the one installed on the context by mfm_hmc_set_inverse_mass is not read.
// (Included by api.hip after mclmc.hip: row_value_grad, ROW_DISPATCH / HMC_MASS_DISPATCH, resident.hip.h, HmcInline / HmcCalled.)
#pragma once

struct GhmcArgs {
  TargetDev T;
  Key2 key;
  const uint32_t* keys;   // non-null: one key per chain [B][2] (mfm_ghmc_step_keys; mfm_ghmc_run in key_mode 1), as HmcArgs::keys
  uint32_t n_total, chain_offset;
  int B;
  double beta, eps;
  double alpha, delta;    // (sqrt(1 - alpha) and sqrt(alpha) are taken in the transition: the same instructions whether alpha comes from the host or from memory)
  float* pos; double* logp; float* grad; double* mom; double* slice;      // state, updated in place
  float* acc_prob; uint8_t* accepted; double* energy_change;              // info [B] (may be null)
  const double* minv;     // [d] diagonal of the inverse mass matrix: read by the MASS instances only
};

// A transition's state and outcome: the kernel's registers, in the step kernel as in the run (MclmcState, mclmc.hip, says why an HBM
// sink is not used: the MAXIT 32 instances spill through it).  finish() takes the end point by select.
template <int MAXIT> struct GhmcState {
  float (&x)[MAXIT]; float (&g)[MAXIT]; double (&p)[MAXIT]; double& lp; double& s;
  bool acc; double pa, de;                               // the transition's outcome: accepted, acceptance rate, dH
  __device__ __forceinline__ void element(int it, int j, float& xo, float& go, double& po) const { xo = x[it]; go = g[it]; po = p[it]; }
  __device__ __forceinline__ double logdensity() const { return lp; }
  __device__ __forceinline__ double slice() const { return s; }
  // pe: the end momentum if accepted, the negated refreshed momentum if not; se: the slice variable after the transition
  template <int M> __device__ __forceinline__ void finish(bool acc_, double pa_, double de_, double lpe, double se, const float (&xe)[M], const float (&ge)[M],
                                                          const double (&pe)[M], int, int) {
    const double lpe0 = __shfl(lpe, 0, 64);     // the value a single-step launch stores (lane 0's) and the next one loads in every lane
#pragma unroll
    for (int it = 0; it < M; ++it) {
      x[it] = acc_ ? xe[it] : x[it];
      g[it] = acc_ ? ge[it] : g[it];
      p[it] = pe[it];
    }
    lp = acc_ ? lpe0 : lp;
    s = se;
    acc = acc_; pa = pa_; de = de_;
  }
};

// ONE transition of the chain this wave holds, with the chain key kb: the whole body of ghmc_step_kernel and of every step of
// ghmc_run_kernel, so a run equals its single steps bit for bit.  eps / alpha / delta / minv come as arguments (not through GhmcArgs)
// so that a caller can give each wave its own.  The state's elements j = lane + 64 * it come through `st` into this function's OWN arrays
// (hmc_trajectory says why).  xs: the wave's LDS row (pads written), gsm: the mixtures' gradient scratch; both are left as
// row_value_grad read them (no trailing barrier).  MASS: as hmc_trajectory -- minv in registers through MAXIT 4, read again from its
// d * 8 cache-resident bytes at every use above; !MASS never reads it.
template <int MAXIT, bool BCRT, bool MASS, class State, class Draw>
__device__ __forceinline__ void ghmc_transition(const TargetDev& T, double beta, double eps, double alpha, double delta, Key2 kb, int d, int lane,
                                                float* xs, float* gsm, const double* minv, State& st, Draw dr) {
#pragma clang fp contract(off)
  const double ca = sqrt(1.0 - alpha), sa = sqrt(alpha);
  const Key2 k_mom = mcmc_step_key(kb, MCMC_K_INT);
  float x[MAXIT], g[MAXIT];
  // the refreshed momentum (a rejection returns it negated) and the trajectory's.  Keeping the refreshed one in the caller's array
  // instead (one array fewer) was tried: ghmc_run_kernel<16> went from no scratch to 608 .. 976 bytes per lane
  double pr[MAXIT], p[MAXIT];
  constexpr bool MREG = MASS && MAXIT <= 4;            // minv in registers
  double mi[MREG ? MAXIT : 1];
  double kin = 0.0;
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    x[it] = 0.f; g[it] = 0.f; pr[it] = 0.0;
    if constexpr (MREG) mi[it] = 1.0;
    if (j < d) {
      st.element(it, j, x[it], g[it], pr[it]);
      if constexpr (MASS) {
        const double m = minv[j];
        if constexpr (MREG) mi[it] = m;
        pr[it] = ca * pr[it] + sa * dr.normal(k_mom, (uint32_t)j, (uint32_t)d) / sqrt(m);      // 1. (alpha = 1: 0 p + n / sqrt(m), hmc_trajectory's bits)
        kin += m * pr[it] * pr[it];
      } else {
        pr[it] = ca * pr[it] + sa * dr.normal(k_mom, (uint32_t)j, (uint32_t)d);
        kin += pr[it] * pr[it];
      }
    }
    p[it] = pr[it];
  }
  const double lp0 = st.logdensity();
  const double s0 = st.slice();
  const double s = fmod(s0 + 1.0 + delta, 2.0) - 1.0;                    // 2.
  const double h0 = -lp0 + 0.5 * wave_sum(kin);                          // 3.
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {                                   // 4.
    const int j = lane + 64 * it;
    if (j < d) {
      p[it] = p[it] + 0.5 * eps * (double)g[it];                         // half kick
      if constexpr (MASS) {
        const double m = MREG ? mi[MREG ? it : 0] : minv[j];
        x[it] = (float)((double)x[it] + eps * (m * p[it]));              // drift
      } else
      x[it] = (float)((double)x[it] + eps * p[it]);                      // drift
      xs[j] = x[it];
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");       // the stencil reads its neighbours' elements from this wave's row
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  const double lp = row_value_grad<MAXIT, BCRT>(T, beta, xs, d, lane, g, gsm);
  __builtin_amdgcn_wave_barrier();                             // (the next transition's drift overwrites the row)
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    if (j < d) p[it] = p[it] + 0.5 * eps * (double)g[it];               // half kick
  }
  double kin1 = 0.0;                                                     // 5.
  if constexpr (MASS) {
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int j = lane + 64 * it;
      if (j < d) kin1 += (MREG ? mi[MREG ? it : 0] : minv[j]) * p[it] * p[it];
    }
  } else
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) kin1 += (lane + 64 * it < d) ? p[it] * p[it] : 0.0;
  const double h1 = -lp + 0.5 * wave_sum(kin1);
  const double de = h1 - h0;
  const double pa = mala_accept_p(h0 - h1, dr);                          // 7. (min(1, exp(-dH)); NaN: 0)
  const bool acc = !isnan(de) && fabs(s) <= pa;                          // 6.
  const double se = acc ? s * dr(de) : s;
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) p[it] = acc ? p[it] : -pr[it];
  st.template finish<MAXIT>(acc, pa, de, lp, se, x, g, p, d, lane);
}

template <int MAXIT, bool BCRT = false, bool MASS = false>
__global__ __launch_bounds__(MALA_WAVES * 64) void ghmc_step_kernel(GhmcArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int d = a.T.dim, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rowlen = d + 2;
  const int b = blockIdx.x * MALA_WAVES + wave;
  if (b >= a.B) return;
  float* xs = smem + wave * rowlen + 1;
  float* gsm = smem + MALA_WAVES * rowlen + wave * MALA_MAXD_SMALL;
  const Key2 kb = mcmc_chain_key(a.key, a.keys, a.n_total, a.chain_offset, b);
  if (lane == 0) { xs[-1] = 0.f; xs[d] = 0.f; }
  const size_t row = (size_t)b * d;
  float x[MAXIT], g[MAXIT];                               // (the state through the kernel's own registers: GhmcState)
  double p[MAXIT];
  double lp = a.logp[b], s = a.slice[b];
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    x[it] = 0.f; g[it] = 0.f; p[it] = 0.0;
    if (j < d) { x[it] = a.pos[row + j]; g[it] = a.grad[row + j]; p[it] = a.mom[row + j]; }
  }
  GhmcState<MAXIT> st{x, g, p, lp, s, false, 0.0, 0.0};
  // MAXIT 32 calls the draws and exp, as the run does (mclmc_step_kernel: 32 unrolled draws in line do not fit beside the state)
  if constexpr (MAXIT > 16) ghmc_transition<MAXIT, BCRT, MASS>(a.T, a.beta, a.eps, a.alpha, a.delta, kb, d, lane, xs, gsm, a.minv, st, HmcCalled());
  else ghmc_transition<MAXIT, BCRT, MASS>(a.T, a.beta, a.eps, a.alpha, a.delta, kb, d, lane, xs, gsm, a.minv, st, HmcInline());
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    if (j < d) {
      if (st.acc) { a.pos[row + j] = x[it]; a.grad[row + j] = g[it]; }
      a.mom[row + j] = p[it];
    }
  }
  if (lane == 0) {
    if (st.acc) a.logp[b] = lp;
    a.slice[b] = s;
    if (a.acc_prob) a.acc_prob[b] = (float)st.pa;
    if (a.accepted) a.accepted[b] = st.acc ? 1 : 0;
    if (a.energy_change) a.energy_change[b] = st.de;
  }
}

// n_steps transitions of every chain in ONE launch (mfm_ghmc_run), on resident.hip.h: x, g, p, the log-density and s are loaded once,
// carried in registers over all the steps and stored once; keys and the thinned trajectory as hmc_run_kernel.  RunTail's n_acc / acc_sum
// are the accepted steps and the sum of the acceptance rates; de_acc_sum the sum of dH over the ACCEPTED steps, in step order.
struct GhmcRunArgs {
  GhmcArgs m;              // acc_prob / accepted / energy_change: the LAST step's info (may be null)
  RunTail t;
  double* de_acc_sum;      // [B] (may be null)
};

template <int MAXIT, bool BCRT = false, bool MASS = false>
__global__ __launch_bounds__(MALA_WAVES * 64) void ghmc_run_kernel(GhmcRunArgs r) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const GhmcArgs& a = r.m;
  const int d = a.T.dim, lane = threadIdx.x & 63, b = resident_chain_index();      // (own scalars: resident.hip.h says why)
  if (b >= a.B) return;
  const ResidentChain c(smem, d, a.B, lane, b);
  float* const xs = c.xs; float* const gsm = c.gsm; const size_t row = c.row;

  float x[MAXIT], g[MAXIT];                               // (the load in line, as hmc_run_kernel's: resident.hip.h)
  double p[MAXIT];
  double lp = a.logp[b], s = a.slice[b];
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    x[it] = 0.f; g[it] = 0.f; p[it] = 0.0;
    if (j < d) { x[it] = a.pos[row + j]; g[it] = a.grad[row + j]; p[it] = a.mom[row + j]; }
  }
  c.pads();
  const Key2 kc = run_chain_key(c, a, r.t);
  int n_acc = 0;
  double acc_sum = 0.0, de_acc = 0.0, p_last = 0.0, de_last = 0.0;
  bool acc_last = false;

  for (int k = 0; k < r.t.n_steps; ++k) {
    const Key2 kb = run_step_key(c, a, r.t, kc, k);
    GhmcState<MAXIT> st{x, g, p, lp, s, false, 0.0, 0.0};
    ghmc_transition<MAXIT, BCRT, MASS>(a.T, a.beta, a.eps, a.alpha, a.delta, kb, d, lane, xs, gsm, a.minv, st, HmcCalled());
    const bool acc = st.acc;
    n_acc += acc ? 1 : 0;
    acc_sum += st.pa;
    de_acc = acc ? de_acc + st.de : de_acc;
    if (k == r.t.n_steps - 1) { p_last = st.pa; de_last = st.de; acc_last = acc; }
    resident_snapshot(c, r.t, k, x, lp);
    resident_step_end();
  }

#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {                    // (the final store stays in line: resident.hip.h)
    const int j = lane + 64 * it;
    if (j < d) { a.pos[row + j] = x[it]; a.grad[row + j] = g[it]; a.mom[row + j] = p[it]; }
  }
  if (lane == 0) {
    a.logp[b] = lp;
    a.slice[b] = s;
    if (r.t.n_acc) r.t.n_acc[b] = n_acc;
    if (r.t.acc_sum) r.t.acc_sum[b] = acc_sum;
    if (r.de_acc_sum) r.de_acc_sum[b] = de_acc;
    if (a.acc_prob) a.acc_prob[b] = (float)p_last;
    if (a.accepted) a.accepted[b] = acc_last ? 1 : 0;
    if (a.energy_change) a.energy_change[b] = de_last;
  }
}

// mfm_ghmc_init: with kb = split(key, n_total)[chain_offset + b], p_j = normal64(mcmc_step_key(kb, MCMC_K_INT), j, d) / sqrt(minv_j) and
// s = 2 uniform01(mcmc_step_key(kb, MCMC_K_RMH)) - 1.  One wave per chain, any d; minv null: the unit metric.
__global__ __launch_bounds__(MALA_WAVES * 64) void ghmc_init_kernel(Key2 key, uint32_t n_total, uint32_t chain_offset, int B, int d, const double* minv,
                                                                    double* mom, double* slice) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, b = blockIdx.x * MALA_WAVES + (threadIdx.x >> 6);
  if (b >= B) return;
  const Key2 kb = split_at(key, n_total, chain_offset + (uint32_t)b);
  const Key2 k_mom = mcmc_step_key(kb, MCMC_K_INT);
  double* const row = mom + (size_t)b * d;
  for (int j = lane; j < d; j += 64) {
    const double n = run_normal64(k_mom, (uint32_t)j, (uint32_t)d);
    row[j] = minv ? n / sqrt(minv[j]) : n;
  }
  if (lane == 0) slice[b] = 2.0 * run_uniform01(mcmc_step_key(kb, MCMC_K_RMH)) - 1.0;
}

int launch_ghmc_step(const GhmcArgs& a, hipStream_t stream) {
  if (a.minv) HMC_MASS_DISPATCH(ghmc_step_kernel, a); else MALA_DISPATCH(ghmc_step_kernel, a);
  return 0;
}
int launch_ghmc_run(const GhmcRunArgs& r, hipStream_t stream) {
  const GhmcArgs& a = r.m;
  if (a.minv) HMC_MASS_DISPATCH(ghmc_run_kernel, r); else MALA_DISPATCH(ghmc_run_kernel, r);
  return 0;
}
void launch_ghmc_init(Key2 key, uint32_t n_total, uint32_t chain_offset, int B, int d, const double* minv, double* mom, double* slice, hipStream_t stream) {
  hipLaunchKernelGGL(ghmc_init_kernel, dim3((B + MALA_WAVES - 1) / MALA_WAVES), dim3(MALA_WAVES * 64), 0, stream, key, n_total, chain_offset, B, d, minv, mom, slice);
}

// ---- MEADS warmup (mfm_meads_warmup; include/mfm.h and tests/meads_ref.py state the algorithm) ------------------------------------------
// n_valid chains are cut into K folds of m; chain perm[f m + i] is member i of fold f (perm null: the identity).  Per iteration, all
// enqueued back to back and nothing read by the host:
//   meads_colstats_kernel   mu_f, sd_f [K][d]: column mean and population standard deviation of a fold's positions, float64, two passes,
//                           64 columns x 16 row groups per workgroup, the groups combined in a fixed order (chees_colmean_kernel's form)
//   meads_stage_kernel      Y = (x - mu_f) / sd_f and Z = g sd_f as padded float32 [2][K][m_pad][d_pad] (rows past m and columns past d
//                           zero, so the Gram tile loads unmasked), gathered through perm; the row norms S_ii of the ROUNDED values in float64
//   meads_gram_kernel       sum_{i != j} S_ij^2 of S = X X^T per fold and matrix on the exact-f32 matrix pipe: svgd.hip's sqdist tile
//                           (64 x 64, K chunks of 32, k-ascending, four independent accumulators per wave), only tiles tj >= ti, the
//                           off-diagonal entries squared in float64, counted twice for tj > ti, one partial per workgroup
//   meads_update_kernel     ONE workgroup: partials and norms summed in a fixed order, lam(Y), lam(Z), the parameters, the keep rule, the
//                           roll to fold (f + 1) mod K, the trace
//   meads_step_kernel       ghmc_step_kernel's mapping with eps / alpha / delta / minv read per wave from par[fold] (as pt.hip reads beta
//                           and eps): always the MASS instances, whose bits at minv == 1 are the unit instances'
//   meads_accmean_kernel    the fold's mean acceptance rate into the trace
// The m x m Gram form is the only one built (DESIGN.md section 4.22 says why).  No float atomics, no flags, no workgroup waits on another.
#define MEADS_PAR 8                                       // doubles ahead of a fold's minv [d]: eps, alpha, delta, 5 spare
#define MEADS_ROWGROUPS 16
constexpr int MEADS_TILE = 64, MEADS_KC = 32, MEADS_LDA = MEADS_KC + 2;      // (svgd.hip's TILE / KC / LDA: the row stride of 34 floats keeps the MFMA operand reads conflict-free)

struct MeadsBufs {
  double* par;            // [K][MEADS_PAR + d]
  int32_t* fold_of;       // [B]
  double *mu, *sd;        // [K][d]
  float* yz;              // [2][K][m_pad][d_pad]: Y, then Z
  double* norms;          // [2][K][m_pad]
  double* part;           // [2][K][n_tiles]
  double* acc;            // [B] the transition's acceptance rate
  double* result;         // [4] eps, alpha, delta of the closing pass
};

// member idx of the membership array, kept inside [0, n_valid) whatever the caller's buffer holds
__device__ __forceinline__ int meads_member(const int32_t* perm, int idx, int n_valid) {
  const int c = perm ? perm[idx] : idx;
  return min(max(c, 0), n_valid - 1);
}

__global__ __launch_bounds__(256) void meads_begin_kernel(double* par, int K, int d, double step0, double alpha0) {
  const int stride = MEADS_PAR + d;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < K * stride; e += gridDim.x * 256) {
    const int k = e % stride;
    par[e] = k == 0 ? step0 : k == 1 ? alpha0 : k == 2 ? alpha0 * 0.5 : k < MEADS_PAR ? 0.0 : 1.0;
  }
}
__global__ __launch_bounds__(256) void meads_fold_kernel(const int32_t* perm, int n_valid, int m, int B, int32_t* fold_of) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  if (i >= n_valid) { fold_of[i] = 0; return; }           // padding rows: fold 0's parameters
  const int c = perm ? perm[i] : i;
  if (c >= 0 && c < n_valid) fold_of[c] = i / m;
}

__global__ __launch_bounds__(64 * MEADS_ROWGROUPS) void meads_colstats_kernel(const float* __restrict__ x, const int32_t* __restrict__ perm, int n_valid,
                                                                              int m, int d, double* __restrict__ mu, double* __restrict__ sd) {
#pragma clang fp contract(off)
  __shared__ double part[MEADS_ROWGROUPS][64];
  __shared__ double mean[64];
  const int col = threadIdx.x & 63, grp = threadIdx.x >> 6, j = blockIdx.x * 64 + col, f = blockIdx.y;
  double s = 0.0;
  if (j < d)
    for (int i = grp; i < m; i += MEADS_ROWGROUPS) s = s + (double)x[(size_t)meads_member(perm, f * m + i, n_valid) * d + j];
  part[grp][col] = s;
  __syncthreads();
  if (grp == 0) {
    double tot = 0.0;
#pragma unroll
    for (int r = 0; r < MEADS_ROWGROUPS; ++r) tot = tot + part[r][col];
    mean[col] = tot / (double)m;
  }
  __syncthreads();
  const double mj = mean[col];
  s = 0.0;
  if (j < d)
    for (int i = grp; i < m; i += MEADS_ROWGROUPS) {
      const double v = (double)x[(size_t)meads_member(perm, f * m + i, n_valid) * d + j] - mj;
      s = s + v * v;
    }
  __syncthreads();                                        // (the first pass's partials have been read)
  part[grp][col] = s;
  __syncthreads();
  if (grp == 0 && j < d) {
    double tot = 0.0;
#pragma unroll
    for (int r = 0; r < MEADS_ROWGROUPS; ++r) tot = tot + part[r][col];
    mu[(size_t)f * d + j] = mj;
    sd[(size_t)f * d + j] = sqrt(tot / (double)m);
  }
}

// one wave per row of the padded [K][m_pad][d_pad] tiles
__global__ __launch_bounds__(256) void meads_stage_kernel(const float* __restrict__ x, const float* __restrict__ g, const int32_t* __restrict__ perm, int n_valid,
                                                          const double* __restrict__ mu, const double* __restrict__ sd, int K, int m, int m_pad, int d, int d_pad,
                                                          float* __restrict__ yz, double* __restrict__ norms) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= K * m_pad) return;
  const int f = row / m_pad, r = row - f * m_pad;
  const size_t chain = r < m ? (size_t)meads_member(perm, f * m + r, n_valid) : 0;
  float* const Y = yz + (size_t)row * d_pad;
  float* const Z = yz + ((size_t)K * m_pad + row) * d_pad;
  double ay = 0.0, az = 0.0;
  for (int c = lane; c < d_pad; c += 64) {
    float y = 0.f, z = 0.f;
    if (r < m && c < d) {
      const double s = sd[(size_t)f * d + c];
      y = (float)(((double)x[chain * d + c] - mu[(size_t)f * d + c]) / s);
      z = (float)((double)g[chain * d + c] * s);
    }
    Y[c] = y; Z[c] = z;
    ay = ay + (double)y * (double)y;
    az = az + (double)z * (double)z;
  }
  ay = wave_sum(ay); az = wave_sum(az);
  if (lane == 0) { norms[row] = ay; norms[(size_t)K * m_pad + row] = az; }
}

// blockIdx: (tile pair with tj >= ti, matrix, fold); one partial per workgroup
__global__ __launch_bounds__(256) void meads_gram_kernel(const float* __restrict__ yz, int K, int m_pad, int d_pad, int n_tiles, double* __restrict__ part) {
  __shared__ float sA[MEADS_TILE * MEADS_LDA], sB[MEADS_TILE * MEADS_LDA];
  __shared__ double red[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1;
  const int T = m_pad / MEADS_TILE;
  int ti = 0, rem = blockIdx.x;
  while (rem >= T - ti) { rem -= T - ti; ++ti; }
  const int tj = ti + rem;
  const int i0 = ti * MEADS_TILE, j0 = tj * MEADS_TILE;
  const float* X = yz + ((size_t)blockIdx.y * K + blockIdx.z) * (size_t)m_pad * d_pad;
  f32x4 acc[2][2];
  for (int a = 0; a < 2; ++a) for (int u = 0; u < 2; ++u) acc[a][u] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, fk = lane >> 4;
  for (int k0 = 0; k0 < d_pad; k0 += MEADS_KC) {
#pragma unroll
    for (int e = 0; e < MEADS_TILE * MEADS_KC / 256; ++e) {
      const int idx = t + 256 * e, r = idx >> 5, k = idx & 31;
      sA[r * MEADS_LDA + k] = X[(size_t)(i0 + r) * d_pad + k0 + k];
      sB[r * MEADS_LDA + k] = X[(size_t)(j0 + r) * d_pad + k0 + k];
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < MEADS_KC / 4; ++s) {
      float a[2], b[2];
      for (int q = 0; q < 2; ++q) a[q] = sA[(32 * wr + 16 * q + fr) * MEADS_LDA + 4 * s + fk];
      for (int u = 0; u < 2; ++u) b[u] = sB[(32 * wc + 16 * u + fr) * MEADS_LDA + 4 * s + fk];
      for (int q = 0; q < 2; ++q)
        for (int u = 0; u < 2; ++u) acc[q][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], b[u], acc[q][u], 0, 0, 0);
    }
    __syncthreads();
  }
  double sum = 0.0;
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int j = j0 + 32 * wc + 16 * u + fr;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = i0 + 32 * wr + 16 * q + 4 * fk + e;
        const double v = i == j ? 0.0 : (double)acc[q][u][e];
        sum = sum + v * v;
      }
    }
  sum = wave_sum(sum);
  if (lane == 0) red[w] = sum;
  __syncthreads();
  if (t == 0) {
    const double tot = ((red[0] + red[1]) + red[2]) + red[3];
    part[((size_t)blockIdx.y * K + blockIdx.z) * n_tiles + blockIdx.x] = tj > ti ? 2.0 * tot : tot;
  }
}

// the wave's sum of v[0 .. n) in a fixed order: lane-strided, then the butterfly
__device__ __forceinline__ double meads_wave_total(const double* v, int n, int lane) {
#pragma clang fp contract(off)
  double s = 0.0;
  for (int i = lane; i < n; i += 64) s = s + v[i];
  return wave_sum(s);
}

// ONE workgroup; wave w takes the folds w, w + 4, ...  final: the closing pass over all chains (K = 1): no roll, no keep rule, the
// parameters go to b.result and minv_out.  trace_t / mass_trace_t: this iteration's [K][6] / [K][d] (may be null).
__global__ __launch_bounds__(256) void meads_update_kernel(MeadsBufs b, int K, int m, int d, int m_pad, int n_tiles, int t, int final,
                                                           double* __restrict__ minv_out, double* __restrict__ trace_t, double* __restrict__ mass_trace_t) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int stride = MEADS_PAR + d;
  for (int f = w; f < K; f += 4) {
    double lam[2];
    for (int mat = 0; mat < 2; ++mat) {
      const double num = meads_wave_total(b.part + ((size_t)mat * K + f) * n_tiles, n_tiles, lane);
      const double tr = meads_wave_total(b.norms + ((size_t)mat * K + f) * m_pad, m, lane);
      lam[mat] = (num / ((double)m * (double)(m - 1))) / (tr / (double)m);
    }
    const double lam_y = lam[0], lam_z = lam[1];
    const double eps = isnan(lam_z) ? lam_z : fmin(1.0, 0.5 / sqrt(lam_z));
    const double gy = 1.0 / sqrt(lam_y), gt = 1.0 / ((double)t * eps);
    const double gamma = (isnan(gy) || isnan(gt)) ? NAN : fmax(gy, gt);
    const double alpha = 1.0 - exp(-2.0 * eps * gamma);
    const double delta = alpha * 0.5;
    const double* sdf = b.sd + (size_t)f * d;
    bool bad = false;
    for (int j = lane; j < d; j += 64) bad = bad || !isfinite(sdf[j] * sdf[j]);
    const bool ok = isfinite(eps) && isfinite(alpha) && isfinite(delta) && eps > 0.0 && !__any(bad);
    if (final) {
      if (lane == 0) { b.result[0] = eps; b.result[1] = alpha; b.result[2] = delta; b.result[3] = ok ? 1.0 : 0.0; }
      if (minv_out) for (int j = lane; j < d; j += 64) minv_out[j] = sdf[j] * sdf[j];
      continue;
    }
    const int r = (f + 1) % K;                            // the receiving fold: only this wave touches par[r]
    double* pr = b.par + (size_t)r * stride;
    if (lane == 0) {
      const double e_used = ok ? eps : pr[0], a_used = ok ? alpha : pr[1], d_used = ok ? delta : pr[2];
      pr[0] = e_used; pr[1] = a_used; pr[2] = d_used;
      if (trace_t) {
        trace_t[r * 6 + 0] = e_used; trace_t[r * 6 + 1] = a_used; trace_t[r * 6 + 2] = d_used;
        trace_t[f * 6 + 3] = lam_z; trace_t[f * 6 + 4] = lam_y;
      }
    }
    for (int j = lane; j < d; j += 64) {
      const double v = ok ? sdf[j] * sdf[j] : pr[MEADS_PAR + j];
      pr[MEADS_PAR + j] = v;
      if (mass_trace_t) mass_trace_t[(size_t)r * d + j] = v;
    }
  }
}

__global__ __launch_bounds__(256) void meads_accmean_kernel(const double* __restrict__ acc, const int32_t* __restrict__ perm, int n_valid, int K, int m,
                                                            double* __restrict__ trace_t) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int f = w; f < K; f += 4) {
    double s = 0.0;
    for (int i = lane; i < m; i += 64) s = s + acc[meads_member(perm, f * m + i, n_valid)];
    s = wave_sum(s);
    if (lane == 0) trace_t[f * 6 + 5] = s / (double)m;
  }
}

// iteration t (from 1) of the warmup: step t - 1 of mfm_hmc_run's key schedule at n_steps = n_iter
template <int MAXIT, bool BCRT = false>
__global__ __launch_bounds__(MALA_WAVES * 64) void meads_step_kernel(GhmcArgs a, const double* __restrict__ par, const int32_t* __restrict__ fold_of, int K,
                                                                     double* __restrict__ acc_out, int key_mode, int n_iter, int t) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int d = a.T.dim, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rowlen = d + 2;
  const int b = blockIdx.x * MALA_WAVES + wave;
  if (b >= a.B) return;
  float* xs = smem + wave * rowlen + 1;
  float* gsm = smem + MALA_WAVES * rowlen + wave * MALA_MAXD_SMALL;
  int fold = fold_of[b];
  if ((unsigned)fold >= (unsigned)K) fold = 0;
  const double* pf = par + (size_t)fold * (MEADS_PAR + d);
  const double eps = pf[0], alpha = pf[1], delta = pf[2];
  const Key2 kc = key_mode ? Key2{a.keys[2 * b], a.keys[2 * b + 1]} : Key2{0, 0};
  const Key2 kb = mcmc_run_key(key_mode, a.key, kc, (uint32_t)n_iter, (uint32_t)(t - 1), a.n_total, a.chain_offset + (uint32_t)b);
  if (lane == 0) { xs[-1] = 0.f; xs[d] = 0.f; }
  const size_t row = (size_t)b * d;
  float x[MAXIT], g[MAXIT];
  double p[MAXIT];
  double lp = a.logp[b], s = a.slice[b];
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    x[it] = 0.f; g[it] = 0.f; p[it] = 0.0;
    if (j < d) { x[it] = a.pos[row + j]; g[it] = a.grad[row + j]; p[it] = a.mom[row + j]; }
  }
  GhmcState<MAXIT> st{x, g, p, lp, s, false, 0.0, 0.0};
  if constexpr (MAXIT > 16) ghmc_transition<MAXIT, BCRT, true>(a.T, a.beta, eps, alpha, delta, kb, d, lane, xs, gsm, pf + MEADS_PAR, st, HmcCalled());
  else ghmc_transition<MAXIT, BCRT, true>(a.T, a.beta, eps, alpha, delta, kb, d, lane, xs, gsm, pf + MEADS_PAR, st, HmcInline());
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    if (j < d) {
      if (st.acc) { a.pos[row + j] = x[it]; a.grad[row + j] = g[it]; }
      a.mom[row + j] = p[it];
    }
  }
  if (lane == 0) {
    if (st.acc) a.logp[b] = lp;
    a.slice[b] = s;
    acc_out[b] = st.pa;
  }
}

// the plan of a warmup (mfm_meads_plan): fold size, the padded tile shape and the Gram launch's workgroups per iteration
struct MeadsPlan { int m, m_pad, d_pad, n_tiles, gram_workgroups; };
static MeadsPlan meads_plan(int n_valid, int K, int d) {
  MeadsPlan p;
  p.m = n_valid / K;
  p.m_pad = (p.m + MEADS_TILE - 1) / MEADS_TILE * MEADS_TILE;
  p.d_pad = (d + MEADS_KC - 1) / MEADS_KC * MEADS_KC;
  const int T = p.m_pad / MEADS_TILE;
  p.n_tiles = T * (T + 1) / 2;
  p.gram_workgroups = 2 * K * p.n_tiles;
  return p;
}

// the four statistics launches on K folds of m chains at iteration t (final: the closing pass)
static void launch_meads_stats(const MeadsBufs& b, const float* pos, const float* grad, const int32_t* perm, int n_valid, int K, int d, int t, int final,
                               double* minv_out, double* trace_t, double* mass_trace_t, hipStream_t stream) {
  const MeadsPlan p = meads_plan(n_valid, K, d);
  hipLaunchKernelGGL(meads_colstats_kernel, dim3((d + 63) / 64, K), dim3(64 * MEADS_ROWGROUPS), 0, stream, pos, perm, n_valid, p.m, d, b.mu, b.sd);
  hipLaunchKernelGGL(meads_stage_kernel, dim3((K * p.m_pad + 3) / 4), dim3(256), 0, stream, pos, grad, perm, n_valid, b.mu, b.sd, K, p.m, p.m_pad, d, p.d_pad,
                     b.yz, b.norms);
  hipLaunchKernelGGL(meads_gram_kernel, dim3(p.n_tiles, 2, K), dim3(256), 0, stream, b.yz, K, p.m_pad, p.d_pad, p.n_tiles, b.part);
  hipLaunchKernelGGL(meads_update_kernel, dim3(1), dim3(256), 0, stream, b, K, p.m, d, p.m_pad, p.n_tiles, t, final, minv_out, trace_t, mass_trace_t);
}
static int launch_meads_step(const GhmcArgs& a, const MeadsBufs& b, int K, int key_mode, int n_iter, int t, hipStream_t stream) {
  MALA_DISPATCH(meads_step_kernel, a, b.par, b.fold_of, K, b.acc, key_mode, n_iter, t);
  return 0;
}
