// ChEES-HMC (Hoffman, Radul & Sountsov 2021; blackjax's chees_adaptation): the trajectory length and the step size of HMC adapted
// ACROSS the chains (mfm_chees_warmup), and the sampler the adaptation is for, mfm_hmc_run with one leapfrog count per step
// (mfm_hmc_run_lengths).  tests/chees_ref.py is the float64 restatement and states every line's source.
//
// One iteration t = 1 .. n_iter is four launches on the context's stream; the host only enqueues, the iteration's step size eps_t,
// trajectory length T_t and leapfrog count L_t live in a CheesState in device memory that the last launch of iteration t - 1 wrote:
//   1. chees_step_kernel: hmc_step_kernel's mapping (one wave per chain, ROW_DISPATCH instances) on the shared hmc_trajectory, with
//      eps_t and L_t read from the CheesState (wave-uniform) and the key mfm_hmc_run uses for step t - 1.  Its state sink is
//      hmc_step_kernel's (HmcInHbm: accept / reject in place) and also keeps, per chain, the state before the step x, the end point x'
//      (float32, accepted or not), the end velocity v' = minv p' and alpha = min(1, exp(H_0 - H_end)) in float64, and whether the
//      trajectory diverged, !(H_end - H_0 < divergence_threshold).  The end momentum reaches the sink through hmc_trajectory's
//      st.momentum hook, which the other sinks leave empty.
//   2. chees_colmean_kernel: the column means of x and x' over the n_valid chains: a workgroup of 64 columns x 16 row groups,
//      float64, rows of a group in order, the groups combined in order.
//   3. chees_chain_kernel: one wave per valid chain: g_k / tau = (|x' - xbar'|^2 - |x - xbar|^2) <x' - xbar', v'>, float64 wave sums.
//   4. chees_update_kernel: ONE workgroup: the pooled sums over the valid, non-divergent chains in a fixed order (chain k goes to
//      thread k % 256, the threads are combined by a tree), then thread 0 writes the trace row, moves the dual averaging (DualAvg,
//      mcmc.hip.h: mfm_hmc_warmup's recursion with p := the chains' harmonic-mean acceptance) and Adam's ascent on log T, and leaves
//      eps_{t+1}, T_{t+1}, L_{t+1} in the CheesState.
// No workgroup waits on another, no atomics, no flags: the launches' order on the stream is the only synchronisation.  Padding rows
// (b >= n_valid) are stepped like any other chain and read by none of 2. - 4.
// (Included by api.hip after warmup.hip: HmcArgs, HmcInHbm, HmcInline, HmcCalled, HmcResident, hmc_trajectory, DualAvg, RunTail and
// resident.hip.h's helpers.)
#pragma once

struct CheesState {
  double eps, T;                 // of the iteration about to run
  int32_t L, t;                  // its leapfrog steps; its number, from 1
  double logT, ma;               // log T, and its moving average
  double m, v, b1t, b2t;         // Adam's moments and the running powers b1^k, b2^k of the k updates applied so far
  DualAvg da;
  double result[4];              // exp(xbar_t), exp(ma_t), eps_{t+1}, T_{t+1}: after iteration n_iter, the call's results
};
struct CheesConst {
  int32_t n_iter, n_valid, max_leapfrog;
  double target, lr, decay, div_thr;
};
// the per-chain records of the last step and the cross-chain scratch
struct CheesBufs {
  CheesState* st;
  float* x0;                     // [B][d] the state before the step
  float* prop;                   // [B][d] the end point x'
  double* vel;                   // [B][d] the end velocity minv p'
  double* alpha;                 // [B]
  uint8_t* div;                  // [B]
  double* mean;                  // [2][d] column means of x0 and of prop
  double* g;                     // [B] g_k / tau
  double* trace;                 // [n_iter][7] (may be null)
};

#define CHEES_ADAM_B1 0.9
#define CHEES_ADAM_B2 0.999
#define CHEES_ADAM_EPS 1e-8

// base-2 radical inverse of t >= 1 (1/2, 1/4, 3/4, 1/8, ...): exact in float64, never 0
__host__ __device__ inline double chees_halton(uint32_t t) {
  double h = 0.0, f = 0.5;
  for (; t; t >>= 1, f *= 0.5) if (t & 1u) h += f;
  return h;
}
__host__ __device__ inline int32_t chees_num_steps(double h, double T, double eps, int32_t max_leapfrog) {
  const double n = ceil(h * T / eps);
  return !(n >= 1.0) ? 1 : (n > (double)max_leapfrog ? max_leapfrog : (int32_t)n);
}

__global__ void chees_begin_kernel(CheesState* s, double eps, double T, int32_t max_leapfrog) {
  if (threadIdx.x || blockIdx.x) return;
  s->eps = eps; s->T = T; s->t = 1;
  s->L = chees_num_steps(chees_halton(1), T, eps, max_leapfrog);
  s->logT = log(T); s->ma = s->logT;
  s->m = 0.0; s->v = 0.0; s->b1t = 1.0; s->b2t = 1.0;
  const double x0 = log(eps);
  s->da = DualAvg{log(10.0 * eps), x0, x0, 0.0, 0.0};
  s->result[0] = eps; s->result[1] = T; s->result[2] = eps; s->result[3] = T;
}

// hmc_step_kernel's sink, which also records what the statistic reads
template <bool MASS> struct CheesInHbm {
  HmcInHbm h; const CheesBufs& c; double div_thr;
  __device__ __forceinline__ void element(int it, int j, float& x, float& g) const { h.element(it, j, x, g); c.x0[h.row + j] = x; }
  __device__ __forceinline__ double logdensity() const { return h.logdensity(); }
  template <int MAXIT> __device__ __forceinline__ void momentum(const double (&p)[MAXIT], double dh, int d, int lane) const {
#pragma clang fp contract(off)
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int j = lane + 64 * it;
      if (j < d) c.vel[h.row + j] = MASS ? h.a.minv[j] * p[it] : p[it];
    }
    if (lane == 0) c.div[h.b] = !(dh < div_thr) ? 1 : 0;
  }
  template <int MAXIT> __device__ __forceinline__ void finish(bool acc, double pa, double lp, const float (&x)[MAXIT], const float (&g)[MAXIT], int d, int lane) const {
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int j = lane + 64 * it;
      if (j < d) c.prop[h.row + j] = x[it];
    }
    if (lane == 0) c.alpha[h.b] = pa;
    h.template finish<MAXIT>(acc, pa, lp, x, g, d, lane);
  }
};

template <int MAXIT, bool BCRT = false, bool MASS = false>
__global__ __launch_bounds__(MALA_WAVES * 64) void chees_step_kernel(HmcArgs a, CheesBufs c, CheesConst k, int key_mode) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int d = a.T.dim, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rowlen = d + 2;
  const int b = blockIdx.x * MALA_WAVES + wave;
  if (b >= a.B) return;
  float* xs = smem + wave * rowlen + 1;
  float* gsm = smem + MALA_WAVES * rowlen + wave * MALA_MAXD_SMALL;
  const double eps = c.st->eps;
  const int L = c.st->L, t = c.st->t;
  const Key2 kc = key_mode ? Key2{a.keys[2 * b], a.keys[2 * b + 1]} : Key2{0, 0};
  const Key2 kb = mcmc_run_key(key_mode, a.key, kc, (uint32_t)k.n_iter, (uint32_t)(t - 1), a.n_total, a.chain_offset + (uint32_t)b);
  if (lane == 0) { xs[-1] = 0.f; xs[d] = 0.f; }
  CheesInHbm<MASS> st{HmcInHbm{a, (size_t)b * d, b}, c, k.div_thr};
  hmc_trajectory<MAXIT, BCRT, MASS>(a.T, a.beta, eps, L, kb, d, lane, xs, gsm, a.minv, st, HmcInline());
}

// column means of x0 (blockIdx.y 0) and prop (1) over the first n_valid rows
#define CHEES_ROWGROUPS 16
__global__ __launch_bounds__(64 * CHEES_ROWGROUPS) void chees_colmean_kernel(CheesBufs c, int n_valid, int d) {
#pragma clang fp contract(off)
  __shared__ double part[CHEES_ROWGROUPS][64];
  const int col = threadIdx.x & 63, grp = threadIdx.x >> 6, j = blockIdx.x * 64 + col;
  const float* src = blockIdx.y ? c.prop : c.x0;
  double s = 0.0;
  if (j < d)
    for (int b = grp; b < n_valid; b += CHEES_ROWGROUPS) s = s + (double)src[(size_t)b * d + j];
  part[grp][col] = s;
  __syncthreads();
  if (grp == 0 && j < d) {
    double tot = 0.0;
#pragma unroll
    for (int r = 0; r < CHEES_ROWGROUPS; ++r) tot = tot + part[r][col];
    c.mean[(size_t)blockIdx.y * d + j] = tot / (double)n_valid;
  }
}

// g_k / tau of chain k < n_valid: one wave per chain
__global__ __launch_bounds__(256) void chees_chain_kernel(CheesBufs c, int n_valid, int d) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= n_valid) return;
  const size_t row = (size_t)b * d;
  double na = 0.0, nb = 0.0, dot = 0.0;
  for (int j = lane; j < d; j += 64) {
    const double dx0 = (double)c.x0[row + j] - c.mean[j];
    const double dx1 = (double)c.prop[row + j] - c.mean[d + j];
    nb = nb + dx0 * dx0;
    na = na + dx1 * dx1;
    dot = dot + dx1 * c.vel[row + j];
  }
  na = wave_sum(na); nb = wave_sum(nb); dot = wave_sum(dot);
  if (lane == 0) c.g[b] = (na - nb) * dot;
}

__device__ __forceinline__ double chees_block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void chees_update_kernel(CheesBufs c, CheesConst k) {
#pragma clang fp contract(off)
  __shared__ double sh[256];
  CheesState& s = *c.st;
  const double tau = chees_halton((uint32_t)s.t) * s.T;
  double s_ag = 0.0, s_a = 0.0, s_inv = 0.0, s_all = 0.0, n_ok = 0.0;
  for (int b = threadIdx.x; b < k.n_valid; b += 256) {
    const double al = c.alpha[b];
    s_all = s_all + al;
    if (!c.div[b]) {
      s_ag = s_ag + al * (tau * c.g[b]);
      s_a = s_a + (al + 1e-20);
      s_inv = s_inv + 1.0 / al;
      n_ok = n_ok + 1.0;
    }
  }
  s_ag = chees_block_sum(s_ag, sh); s_a = chees_block_sum(s_a, sh); s_inv = chees_block_sum(s_inv, sh);
  s_all = chees_block_sum(s_all, sh); n_ok = chees_block_sum(n_ok, sh);
  if (threadIdx.x) return;
  const double ghat = n_ok > 0.0 ? s_ag / s_a : 0.0;
  const double hm = n_ok > 0.0 ? n_ok / s_inv : 0.0;
  const int t = s.t;
  if (c.trace) {
    double* row = c.trace + (size_t)(t - 1) * 7;
    row[0] = s.eps; row[1] = s.T; row[2] = (double)s.L; row[3] = hm; row[4] = ghat;
    row[5] = (double)k.n_valid - n_ok; row[6] = s_all / (double)k.n_valid;
  }
  dual_avg_update(s.da, t, hm, k.target);
  const double eps = exp(s.da.x);
  if (isfinite(ghat)) {                                   // Adam, ascending: a non-finite gradient leaves log T and the moments alone
    s.m = CHEES_ADAM_B1 * s.m + (1.0 - CHEES_ADAM_B1) * ghat;
    s.v = CHEES_ADAM_B2 * s.v + (1.0 - CHEES_ADAM_B2) * (ghat * ghat);
    s.b1t = s.b1t * CHEES_ADAM_B1; s.b2t = s.b2t * CHEES_ADAM_B2;
    const double mhat = s.m / (1.0 - s.b1t), vhat = s.v / (1.0 - s.b2t);
    s.logT = s.logT + k.lr * (mhat / (sqrt(vhat) + CHEES_ADAM_EPS));
  }
  s.logT = fmin(fmax(s.logT, s.da.x), s.da.x + log((double)k.max_leapfrog));      // T in [eps, max_leapfrog eps]
  s.ma = k.decay * s.ma + (1.0 - k.decay) * s.logT;
  s.eps = eps; s.T = exp(s.logT); s.t = t + 1;
  s.L = chees_num_steps(chees_halton((uint32_t)(t + 1)), s.T, s.eps, k.max_leapfrog);
  s.result[0] = exp(s.da.xbar); s.result[1] = exp(s.ma); s.result[2] = s.eps; s.result[3] = s.T;
}

// one iteration's four launches
int launch_chees_iteration(const HmcArgs& a, const CheesBufs& c, const CheesConst& k, int key_mode, hipStream_t stream) {
  if (a.minv) HMC_MASS_DISPATCH(chees_step_kernel, a, c, k, key_mode); else MALA_DISPATCH(chees_step_kernel, a, c, k, key_mode);
  const int d = a.T.dim;
  hipLaunchKernelGGL(chees_colmean_kernel, dim3((d + 63) / 64, 2), dim3(64 * CHEES_ROWGROUPS), 0, stream, c, k.n_valid, d);
  hipLaunchKernelGGL(chees_chain_kernel, dim3((k.n_valid + 3) / 4), dim3(256), 0, stream, c, k.n_valid, d);
  hipLaunchKernelGGL(chees_update_kernel, dim3(1), dim3(256), 0, stream, c, k);
  return 0;
}

// ---- mfm_hmc_run_lengths: hmc_run_kernel with step s making num_steps[s] leapfrog steps --------------------------------------------
// The residency load, the loop and the final store are hmc_run_kernel's lines (hmc_run.hip; resident.hip.h says why they stay in
// line in each kernel); the count is wave-uniform, so the chains of a launch stay in lock step.
template <int MAXIT, bool BCRT = false, bool MASS = false>
__global__ __launch_bounds__(MALA_WAVES * 64) void hmc_run_lengths_kernel(HmcRunArgs r, const int32_t* num_steps, int64_t* total_leapfrog) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const HmcArgs& a = r.h;
  const int d = a.T.dim, lane = threadIdx.x & 63, b = resident_chain_index();
  if (b >= a.B) return;
  const ResidentChain c(smem, d, a.B, lane, b);
  float* const xs = c.xs; float* const gsm = c.gsm; const size_t row = c.row;

  float x[MAXIT], g[MAXIT];
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
  long long n_leap = 0;
  double acc_sum = 0.0, p_last = 0.0;
  bool acc_last = false;

  for (int s = 0; s < r.t.n_steps; ++s) {
    const Key2 kb = run_step_key(c, a, r.t, kc, s);
    const int L = min(max(num_steps[s], 1), 100000);      // (the documented range; the host cannot see the array)
    HmcResident<MAXIT> st{x, g, lp, false, 0.0};
    hmc_trajectory<MAXIT, BCRT, MASS>(a.T, a.beta, a.eps, L, kb, d, lane, xs, gsm, a.minv, st, HmcCalled());
    const bool acc = st.acc;
    const double p = st.pa;
    n_acc += acc ? 1 : 0;
    n_leap += L;
    acc_sum += p;
    if (s == r.t.n_steps - 1) { p_last = p; acc_last = acc; }
    resident_snapshot(c, r.t, s, x, lp);
    resident_step_end();
  }

#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    if (j < d) { a.pos[row + j] = x[it]; a.grad[row + j] = g[it]; }
  }
  if (lane == 0) {
    a.logp[b] = lp;
    if (r.t.n_acc) r.t.n_acc[b] = n_acc;
    if (r.t.acc_sum) r.t.acc_sum[b] = acc_sum;
    if (a.acc_prob) a.acc_prob[b] = (float)p_last;
    if (a.accepted) a.accepted[b] = acc_last ? 1 : 0;
    if (total_leapfrog && b == 0) *total_leapfrog = n_leap;
  }
}

int launch_hmc_run_lengths(const HmcRunArgs& r, const int32_t* num_steps, int64_t* total_leapfrog, hipStream_t stream) {
  const HmcArgs& a = r.h;
  if (a.minv) HMC_MASS_DISPATCH(hmc_run_lengths_kernel, r, num_steps, total_leapfrog); else MALA_DISPATCH(hmc_run_lengths_kernel, r, num_steps, total_leapfrog);
  return 0;
}
