// Step-size warmup: n_steps HMC or MALA steps of every chain in ONE launch, in which every chain adapts its OWN step size by dual
// averaging towards a target acceptance probability (mfm_hmc_warmup / mfm_mala_warmup; the recursion: include/mfm.h, DualAvg in mcmc.hip.h).
//
// hmc_warmup_kernel / mala_warmup_kernel are hmc_run_kernel / mala_run_kernel (the mapping, key schedule and closing fence of
// resident.hip.h; the same residency and instances) without the
// trajectory and the last step's info, and with this wave's step size eps_m in place of the launch's: step m of chain b gives the bits
// of a single-step launch (mfm_hmc_step_keys; mfm_mala_step_keys with textbook = 1) with the scalar step size eps_m[b] and the same step
// key (tests/test_gpu_warmup.py).  Every HMC chain makes the same number of leapfrog steps, so different step sizes cost no divergence.
// A chain adapts from the acceptance probability its step already holds (lane 0's float64 value, before it is rounded for any info):
// no communication between chains, no host round trip; the caller pools the per-chain results.
//
// The adaptation's state is wave-uniform.  It is read back through v_readfirstlane after every update, so it lives in scalar registers
// over the step and takes no vector register from the trajectory (DESIGN.md section 4.11 has the figures); exp and log are called out of
// line for the reason mala_run.hip states.
// (Included by api.hip after hmc_run.hip: HmcRunArgs, HmcResident, HmcCalled, MalaRunArgs, RunExp, run_normal64 / run_uniform01 / run_exp.)

struct WarmupArgs {
  double target;           // the acceptance probability steered to, inside (0, 1)
  double* step_avg;        // [B] exp(xbar_n), the result
  double* step_last;       // [B] exp(x_n) (may be null)
  double* step_traj;       // [n_steps][B] the step size USED at each step (may be null)
  double* pos_sum;         // [B][d] sum over the steps of the state after accept / reject, and
  double* pos_sumsq;       // [B][d] of its square (mfm_hmc_warmup_window: both or neither; the MASS instances of hmc_warmup_kernel only)
};

__device__ __attribute__((noinline)) double run_log(double v) { return log(v); }

// lane 0's value, in scalar registers from here on
__device__ __forceinline__ double wave_first(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ DualAvg warmup_begin(double step0) {
  const double x0 = wave_first(run_log(step0));
  return DualAvg{wave_first(run_log(10.0 * step0)), x0, x0, 0.0, 0.0};
}
// the run's two tallies, kept wave-uniform (lane 0's values, the ones that are written) so that they too ride in scalar registers over a step
__device__ __forceinline__ void warmup_tally(int& n_acc, double& acc_sum, bool acc, double p) {
  n_acc += __builtin_amdgcn_readfirstlane(acc ? 1 : 0);
  acc_sum = wave_first(acc_sum + wave_first(p));
}
// after step m (from 1) with acceptance probability p: the state moves on; returns the next step's size exp(x_m)
__device__ __forceinline__ double warmup_next(DualAvg& da, int m, double p, double target) {
  dual_avg_update(da, m, wave_first(p), target);
  da.x = wave_first(da.x); da.hbar = wave_first(da.hbar); da.xbar = wave_first(da.xbar);
  return wave_first(run_exp(da.x));
}

// both kernels' epilogue, after the state's final store: the log-density, the averaged step size, the last one, the two tallies
__device__ __forceinline__ void warmup_finish(const ResidentChain& c, const RunTail& t, const WarmupArgs& w, const DualAvg& da, double eps, int n_acc, double acc_sum, double* logp, double lp) {
  const double avg = run_exp(da.xbar);
  if (c.lane == 0) {
    logp[c.b] = lp;
    w.step_avg[c.b] = avg;
    if (w.step_last) w.step_last[c.b] = eps;
    if (t.n_acc) t.n_acc[c.b] = n_acc;
    if (t.acc_sum) t.acc_sum[c.b] = acc_sum;
  }
}

// MASS (the instances of mfm_hmc_set_inverse_mass and mfm_hmc_warmup_window): hmc_trajectory's, and the window's sums.  With w.pos_sum
// the state after every step's accept / reject, the float32 position as a double (its square is exact), is added in step order to two
// float64 sums per element, which a window of any length leaves behind in place of its trajectory.  Through MAXIT 4 the sums ride in
// registers and are stored once; above, they are kept in their own elements of the output, which only this lane touches.
template <int MAXIT, bool BCRT = false, bool MASS = false>
__global__ __launch_bounds__(MALA_WAVES * 64) void hmc_warmup_kernel(HmcRunArgs r, WarmupArgs w) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const HmcArgs& a = r.h;
  const int d = a.T.dim, lane = threadIdx.x & 63, b = resident_chain_index();      // (own scalars: resident.hip.h says why)
  if (b >= a.B) return;
  const ResidentChain c(smem, d, a.B, lane, b);
  float* const xs = c.xs; float* const gsm = c.gsm; const size_t row = c.row, B = c.B;

  float x[MAXIT], g[MAXIT];                               // (in line here: through resident_load the MAXIT 16 / 32 instances gain spill instructions, resident.hip.h)
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
  DualAvg da = warmup_begin(a.eps);
  double eps = a.eps;                                     // the first step runs at the caller's value itself
  constexpr bool SREG = MASS && MAXIT <= 4;               // the window's sums in registers
  double sx[SREG ? MAXIT : 1], sxx[SREG ? MAXIT : 1];
  if constexpr (MASS) {
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int j = lane + 64 * it;
      if constexpr (SREG) { sx[it] = 0.0; sxx[it] = 0.0; }
      else if (w.pos_sum && j < d) { w.pos_sum[row + j] = 0.0; w.pos_sumsq[row + j] = 0.0; }
    }
  }

  for (int s = 0; s < r.t.n_steps; ++s) {
    const Key2 kb = run_step_key(c, a, r.t, kc, s);
    if (w.step_traj && lane == 0) w.step_traj[(size_t)s * B + (size_t)b] = eps;
    HmcResident<MAXIT> st{x, g, lp, false, 0.0};
    hmc_trajectory<MAXIT, BCRT, MASS>(a.T, a.beta, eps, a.num_steps, kb, d, lane, xs, gsm, a.minv, st, HmcCalled());
    warmup_tally(n_acc, acc_sum, st.acc, st.pa);
    eps = warmup_next(da, s + 1, st.pa, w.target);
    if constexpr (MASS) {
#pragma clang fp contract(off)
#pragma unroll
      for (int it = 0; it < MAXIT; ++it) {
        const int j = lane + 64 * it;
        const double v = (double)x[it];
        if constexpr (SREG) { sx[it] = sx[it] + v; sxx[it] = sxx[it] + v * v; }
        else if (w.pos_sum && j < d) { w.pos_sum[row + j] = w.pos_sum[row + j] + v; w.pos_sumsq[row + j] = w.pos_sumsq[row + j] + v * v; }
      }
    }
    resident_step_end();
  }

#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {                    // (the final store stays in line: resident.hip.h)
    const int j = lane + 64 * it;
    if (j < d) { a.pos[row + j] = x[it]; a.grad[row + j] = g[it]; }
  }
  if constexpr (SREG) {
    if (w.pos_sum) {
#pragma unroll
      for (int it = 0; it < MAXIT; ++it) {
        const int j = lane + 64 * it;
        if (j < d) { w.pos_sum[row + j] = sx[it]; w.pos_sumsq[row + j] = sxx[it]; }
      }
    }
  }
  warmup_finish(c, r.t, w, da, eps, n_acc, acc_sum, a.logp, lp);
}

template <int MAXIT, bool BCRT = false>
__global__ __launch_bounds__(MALA_WAVES * 64) void mala_warmup_kernel(MalaRunArgs r, WarmupArgs w) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const MalaArgs& a = r.m;
  const int d = a.T.dim, lane = threadIdx.x & 63, b = resident_chain_index();      // (own scalars: resident.hip.h says why)
  if (b >= a.B) return;
  const ResidentChain c(smem, d, a.B, lane, b);
  float* const xs = c.xs; float* const gsm = c.gsm; const size_t row = c.row, B = c.B;

  ResidentState<MAXIT> cs = resident_load<MAXIT>(c, a);
  float (&x)[MAXIT] = cs.x; float (&g)[MAXIT] = cs.g; double& lp = cs.lp;
  c.pads();
  float xn[MAXIT];
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) xn[it] = 0.f;
  const Key2 kc = run_chain_key(c, a, r.t);
  int n_acc = 0;
  double acc_sum = 0.0;
  DualAvg da = warmup_begin(a.eps);
  double eps = a.eps;                                     // the first step runs at the caller's value itself

  for (int s = 0; s < r.t.n_steps; ++s) {
    const Key2 kb = run_step_key(c, a, r.t, kc, s);
    if (w.step_traj && lane == 0) w.step_traj[(size_t)s * B + (size_t)b] = eps;
    MalaResident<MAXIT> st{x, g, lp, xn, false, 0.0, 0.0, 0.0};
    mala_resident_step<MAXIT, BCRT>(a.T, a.beta, eps, mala_s2e(eps), a.textbook, kb, d, lane, xs, gsm, st);
    const bool acc = st.acc;
    const double p = st.p;
    warmup_tally(n_acc, acc_sum, acc, p);
    eps = warmup_next(da, s + 1, p, w.target);
    resident_step_end();
  }

#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {                    // (the final store stays in line: resident.hip.h)
    const int j = lane + 64 * it;
    if (j < d) { a.pos[row + j] = x[it]; a.grad[row + j] = g[it]; }
  }
  warmup_finish(c, r.t, w, da, eps, n_acc, acc_sum, a.logp, lp);
}

int launch_hmc_warmup(const HmcRunArgs& r, const WarmupArgs& w, hipStream_t stream) {
  const HmcArgs& a = r.h;
  if (a.minv) HMC_MASS_DISPATCH(hmc_warmup_kernel, r, w); else MALA_DISPATCH(hmc_warmup_kernel, r, w);
  return 0;
}
int launch_mala_warmup(const MalaRunArgs& r, const WarmupArgs& w, hipStream_t stream) {
  const MalaArgs& a = r.m;
  MALA_DISPATCH(mala_warmup_kernel, r, w);
  return 0;
}
