// Microcanonical Langevin Monte Carlo over parallel chains, one wavefront per chain (mfm_mclmc_init / _step / _step_keys / _run) -- a
// BUILD-SIDE MODE beside hmc.hip: the unadjusted sampler of Robnik, De Luca, Silverstein & Seljak 2023 and Robnik & Seljak 2024
// (blackjax.mclmc), restated in float64 in tests/mclmc_ref.py.  A chain is a position x, a UNIT momentum u, log p(x) and g = grad log p(x)
// of the tempered density.  One step of size eps is a palindromic schedule of
//   B(h): the exact flow of du/dt = (I - u u^T) g / (d - 1) at the gradient g -- n = g / |g|, c = u.n, delta = h |g| / (d - 1),
//         zeta = exp(-delta), u <- r / |r| with r = n (1 - zeta)(1 + zeta + c (1 - zeta)) + 2 zeta u, and the kinetic change
//         dK = (d - 1) (delta - ln 2 + ln(1 + c + (1 - c) zeta^2)); |g| = 0 leaves u and adds 0
//   A(h): x <- x + h u, then value and gradient at x
// (leapfrog: B A B, one gradient; McLachlan's minimal-norm scheme: B A B A B, two), followed by the partial refresh
// u <- (u + nu z) / |u + nu z| with z_j = normal64(mcmc_step_key(kb, MCMC_K_INT), j, d), nu = sqrt((exp(2 eps / L) - 1) / d); nu = 0
// (L = +inf) draws nothing.  There is NO accept test: every step is taken, its energy change dE = sum dK - (logp_end - logp_start) is
// the diagnostic (per chain: the sums of dE and dE^2 and the number of non-finite ones; a chain is not repaired).
// Layout as hmc.hip: positions / gradients float32, log-density float64; the momentum is float64 in registers AND in HBM ([B][d]: a
// float32 copy between launches would break run == steps); the position is rounded to float32 after every A (it is what the target is
// evaluated at); |g|^2, u.n, |r|^2 and |u + nu z|^2 are float64 sums over the wave; every operation is rounded on its own.  c is clamped
// to [-1, 1] (its rounding can leave it by an ulp, and at d = 2 the argument of the logarithm would go negative).
// Targets: phi-four and the Gaussian mixtures (row_value_grad); unit metric only.
// (Included by api.hip after hmc_run.hip: row_value_grad, MALA_DISPATCH, resident.hip.h, run_normal64 / run_exp.)
#pragma once

#define MCLMC_MAX_STAGES 2
struct MclmcArgs {
  TargetDev T;
  Key2 key;
  const uint32_t* keys;   // non-null: one key per chain [B][2] (mfm_mclmc_step_keys; mfm_mclmc_run in key_mode 1), as HmcArgs::keys
  uint32_t n_total, chain_offset;
  int B, n_stages;        // n_stages: gradients per step (1: leapfrog, 2: McLachlan)
  double beta;
  double hb[MCLMC_MAX_STAGES + 1], ha[MCLMC_MAX_STAGES];      // the schedule's times b_k eps / a_k eps (the host's products: the same in every kernel)
  double nu;              // the refresh's noise scale (0: none)
  float* pos; double* logp; float* grad; double* mom;          // state, updated in place
  double* energy_change; double* kinetic_change;               // info [B] (may be null)
};

// exp / log / sqrt and the refresh's draws as a single-step launch makes them: in line (the run kernel calls them out of line)
struct MclmcInline {
  __device__ __forceinline__ double normal(Key2 k, uint32_t idx, uint32_t size) const { return normal64(k, idx, size); }
  __device__ __forceinline__ double exp_(double v) const { return exp(v); }
  __device__ __forceinline__ double log_(double v) const { return log(v); }
  __device__ __forceinline__ double sqrt_(double v) const { return sqrt(v); }
};
// ... through mala_run.hip's out-of-line wrappers (the reason is stated there) and warmup.hip's run_log: same instructions, same bits
__device__ double run_log(double v);      // (defined in warmup.hip, which api.hip includes after this file)
struct MclmcCalled {
  __device__ __forceinline__ double normal(Key2 k, uint32_t idx, uint32_t size) const { return run_normal64(k, idx, size); }
  __device__ __forceinline__ double exp_(double v) const { return run_exp(v); }
  __device__ __forceinline__ double log_(double v) const { return run_log(v); }
  __device__ __forceinline__ double sqrt_(double v) const { return run_sqrt(v); }
};

// A step's state and outcome: the kernel's registers, in the step kernel as in the run.  An HmcInHbm-style sink (elements read from HBM
// inside mclmc_step, stored by finish) was tried for the step kernel: its MAXIT 32 instances had 5569 / 6684 VGPR spill instructions and
// 2288 / 2480 bytes of scratch per lane with the draws called (5520 / 6138 and 2164 / 2224 with them in line), and through this form they
// have none.  This is the ONLY state type.  mclmc_step still takes it as a template parameter, reads it through
// element() into its own arrays and hands the result to finish(): that shape -- hmc_trajectory's, which records that the caller's arrays
// handed in by reference cost its large instances scratch -- is the one whose resources were measured, and it is kept as measured.
template <int MAXIT> struct MclmcState {
  float (&x)[MAXIT]; float (&g)[MAXIT]; double (&u)[MAXIT]; double& lp;
  double de, dk;                                         // the step's energy change and kinetic change
  __device__ __forceinline__ void element(int it, int j, float& xo, float& go, double& uo) const { xo = x[it]; go = g[it]; uo = u[it]; }
  __device__ __forceinline__ double logdensity() const { return lp; }
  template <int M> __device__ __forceinline__ void finish(double lpe, double de_, double dk_, const float (&xe)[M], const float (&ge)[M], const double (&ue)[M], int, int) {
#pragma unroll
    for (int it = 0; it < M; ++it) { x[it] = xe[it]; g[it] = ge[it]; u[it] = ue[it]; }
    lp = lpe; de = de_; dk = dk_;
  }
};

// B(h) at the gradient g (head of this file): u in place, returns the kinetic change (wave-uniform)
template <int MAXIT, class Draw>
__device__ __forceinline__ double mclmc_momentum(double h, double dm1, const float (&g)[MAXIT], double (&u)[MAXIT], int d, int lane, Draw dr) {
#pragma clang fp contract(off)
  double g2 = 0.0;
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) g2 += (lane + 64 * it < d) ? (double)g[it] * (double)g[it] : 0.0;
  const double gn = dr.sqrt_(wave_sum(g2));
  const bool flat = gn == 0.0;                             // no branch: with n = 0 the lines below give 2 u / 2, u's own bits (a NaN gradient ends in a non-finite dE)
  const double ginv = flat ? 0.0 : 1.0 / gn;
  double e = 0.0;
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) e += (lane + 64 * it < d) ? u[it] * ((double)g[it] * ginv) : 0.0;
  const double c = fmin(fmax(wave_sum(e), -1.0), 1.0);
  const double delta = h * gn / dm1;
  const double zeta = dr.exp_(-delta);
  const double omz = 1.0 - zeta;
  const double cn = omz * (1.0 + zeta + c * omz), cu = 2.0 * zeta;
  double r2 = 0.0;
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    if (lane + 64 * it < d) {
      u[it] = ((double)g[it] * ginv) * cn + cu * u[it];
      r2 += u[it] * u[it];
    }
  }
  const double rinv = flat ? 0.5 : 1.0 / dr.sqrt_(wave_sum(r2));
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) u[it] = u[it] * rinv;
  const double dk = dm1 * (delta - 0.6931471805599453 + dr.log_(1.0 + c + (1.0 - c) * (zeta * zeta)));
  return flat ? 0.0 : dk;
}

// ONE step of the chain this wave holds, with the step's chain key kb: the whole body of mclmc_step_kernel and of every step of
// mclmc_run_kernel, so a run equals its single steps bit for bit.  The state's elements j = lane + 64 * it come through `st` into this
// function's OWN arrays (hmc_trajectory says why) and the new state goes back through st.finish with the end point's log-density (lane
// 0's value, the one a single-step launch stores and the next loads), the energy change and the kinetic change.  xs: the wave's LDS row
// (pads written), gsm: the mixtures' gradient scratch; both are left as the last row_value_grad read them (no trailing barrier).
template <int MAXIT, bool BCRT, class State, class Draw>
__device__ __forceinline__ void mclmc_step(const MclmcArgs& a, Key2 kb, int d, int lane, float* xs, float* gsm, State& st, Draw dr) {
#pragma clang fp contract(off)
  float x[MAXIT], g[MAXIT];
  double u[MAXIT];
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    x[it] = 0.f; g[it] = 0.f; u[it] = 0.0;
    if (j < d) st.element(it, j, x[it], g[it], u[it]);
  }
  const double lp0 = st.logdensity();
  const double dm1 = (double)(d - 1);
  double lp = lp0;
  double dk = mclmc_momentum<MAXIT>(a.hb[0], dm1, g, u, d, lane, dr);
  for (int k = 0; k < a.n_stages; ++k) {
    const double h = a.ha[k];
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int j = lane + 64 * it;
      if (j < d) {
        x[it] = (float)((double)x[it] + h * u[it]);                     // A
        xs[j] = x[it];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");       // the stencil reads its neighbours' elements from this wave's row
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    lp = row_value_grad<MAXIT, BCRT>(a.T, a.beta, xs, d, lane, g, gsm);
    __builtin_amdgcn_wave_barrier();                             // (the next A overwrites the row)
    dk = dk + mclmc_momentum<MAXIT>(a.hb[k + 1], dm1, g, u, d, lane, dr);
  }
  lp = __shfl(lp, 0, 64);
  const double de = dk - (lp - lp0);
  if (a.nu != 0.0) {                                             // the partial refresh
    const Key2 k_ref = mcmc_step_key(kb, MCMC_K_INT);
    double w2 = 0.0;
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int j = lane + 64 * it;
      if (j < d) {
        u[it] = u[it] + a.nu * dr.normal(k_ref, (uint32_t)j, (uint32_t)d);
        w2 += u[it] * u[it];
      }
    }
    const double winv = 1.0 / dr.sqrt_(wave_sum(w2));
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) u[it] = u[it] * winv;
  }
  st.template finish<MAXIT>(lp, de, dk, x, g, u, d, lane);
}

template <int MAXIT, bool BCRT = false>
__global__ __launch_bounds__(MALA_WAVES * 64) void mclmc_step_kernel(MclmcArgs a) {
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
  float x[MAXIT], g[MAXIT];                               // (the state through the kernel's own registers: MclmcState says why)
  double u[MAXIT];
  double lp = a.logp[b];
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    x[it] = 0.f; g[it] = 0.f; u[it] = 0.0;
    if (j < d) { x[it] = a.pos[row + j]; g[it] = a.grad[row + j]; u[it] = a.mom[row + j]; }
  }
  MclmcState<MAXIT> st{x, g, u, lp, 0.0, 0.0};
  // MAXIT 32 calls the draws and exp / log / sqrt, as the run does: 32 unrolled draws in line do not fit beside x, g and the float64 momentum
  if constexpr (MAXIT > 16) mclmc_step<MAXIT, BCRT>(a, kb, d, lane, xs, gsm, st, MclmcCalled());
  else mclmc_step<MAXIT, BCRT>(a, kb, d, lane, xs, gsm, st, MclmcInline());
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    if (j < d) { a.pos[row + j] = x[it]; a.grad[row + j] = g[it]; a.mom[row + j] = u[it]; }
  }
  if (lane == 0) {
    a.logp[b] = lp;
    if (a.energy_change) a.energy_change[b] = st.de;
    if (a.kinetic_change) a.kinetic_change[b] = st.dk;
  }
}

// n_steps steps of every chain in ONE launch (mfm_mclmc_run), on resident.hip.h: x, g, u and the log-density are loaded once, carried in
// registers over all the steps and stored once; keys and the thinned trajectory as hmc_run_kernel.  RunTail's n_acc / acc_sum stay null.
struct MclmcRunArgs {
  MclmcArgs m;
  RunTail t;
  double* de_sum; double* de_sumsq;     // [B] sums of dE and dE^2 over the steps (may be null)
  int32_t* n_nonfinite;                 // [B] steps whose dE is not finite (may be null)
  double* energy_trace;                 // [n_steps][B] every step's dE (may be null)
};

template <int MAXIT, bool BCRT = false>
__global__ __launch_bounds__(MALA_WAVES * 64) void mclmc_run_kernel(MclmcRunArgs r) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const MclmcArgs& a = r.m;
  const int d = a.T.dim, lane = threadIdx.x & 63, b = resident_chain_index();      // (own scalars: resident.hip.h says why)
  if (b >= a.B) return;
  const ResidentChain c(smem, d, a.B, lane, b);
  float* const xs = c.xs; float* const gsm = c.gsm; const size_t row = c.row;

  float x[MAXIT], g[MAXIT];                               // (the load in line, as hmc_run_kernel's: resident.hip.h)
  double u[MAXIT];
  double lp = a.logp[b];
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    x[it] = 0.f; g[it] = 0.f; u[it] = 0.0;
    if (j < d) { x[it] = a.pos[row + j]; g[it] = a.grad[row + j]; u[it] = a.mom[row + j]; }
  }
  c.pads();
  const Key2 kc = run_chain_key(c, a, r.t);
  double de_sum = 0.0, de_sumsq = 0.0;
  int n_bad = 0;

  for (int s = 0; s < r.t.n_steps; ++s) {
    const Key2 kb = run_step_key(c, a, r.t, kc, s);
    MclmcState<MAXIT> st{x, g, u, lp, 0.0, 0.0};
    mclmc_step<MAXIT, BCRT>(a, kb, d, lane, xs, gsm, st, MclmcCalled());
    const double de = st.de;
    de_sum = de_sum + de;
    de_sumsq = de_sumsq + de * de;
    n_bad += isfinite(de) ? 0 : 1;
    if (r.energy_trace && lane == 0) r.energy_trace[(size_t)s * c.B + (size_t)b] = de;
    resident_snapshot(c, r.t, s, x, lp);
    resident_step_end();
  }

#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {                    // (the final store stays in line: resident.hip.h)
    const int j = lane + 64 * it;
    if (j < d) { a.pos[row + j] = x[it]; a.grad[row + j] = g[it]; a.mom[row + j] = u[it]; }
  }
  if (lane == 0) {
    a.logp[b] = lp;
    if (r.de_sum) r.de_sum[b] = de_sum;
    if (r.de_sumsq) r.de_sumsq[b] = de_sumsq;
    if (r.n_nonfinite) r.n_nonfinite[b] = n_bad;
  }
}

// the unit momenta u_b = z / |z|, z_j = normal64(split(key, n_total)[chain_offset + b], j, d): one wave per chain, any d
__global__ __launch_bounds__(MALA_WAVES * 64) void mclmc_init_kernel(Key2 key, uint32_t n_total, uint32_t chain_offset, int B, int d, double* mom) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, b = blockIdx.x * MALA_WAVES + (threadIdx.x >> 6);
  if (b >= B) return;
  const Key2 kb = split_at(key, n_total, chain_offset + (uint32_t)b);
  double* const row = mom + (size_t)b * d;
  double z2 = 0.0;
  for (int j = lane; j < d; j += 64) {
    const double z = run_normal64(kb, (uint32_t)j, (uint32_t)d);
    row[j] = z;
    z2 += z * z;
  }
  const double zn = sqrt(wave_sum(z2));
  for (int j = lane; j < d; j += 64) row[j] = row[j] / zn;      // (each lane rescales what it wrote)
}

int launch_mclmc_step(const MclmcArgs& a, hipStream_t stream) { MALA_DISPATCH(mclmc_step_kernel, a); return 0; }
int launch_mclmc_run(const MclmcRunArgs& r, hipStream_t stream) {
  const MclmcArgs& a = r.m;
  MALA_DISPATCH(mclmc_run_kernel, r);
  return 0;
}
void launch_mclmc_init(Key2 key, uint32_t n_total, uint32_t chain_offset, int B, int d, double* mom, hipStream_t stream) {
  hipLaunchKernelGGL(mclmc_init_kernel, dim3((B + MALA_WAVES - 1) / MALA_WAVES), dim3(MALA_WAVES * 64), 0, stream, key, n_total, chain_offset, B, d, mom);
}
