// n_steps HMC steps of every chain in ONE launch (mfm_hmc_run): what mala_run.hip is to mala.hip, for hmc.hip.  The scan of
// `inference_loop0` (mcmc_utils.py:11-25) over an HMC kernel, with the chain resident in the wave.
//
// Same mapping as hmc_step_kernel: one wave per chain, MALA_WAVES chains per workgroup, the trajectory's row staged in the wave's own
// LDS row between its two pads, the same MAXIT / BCRT instances.  What differs is residency: x[MAXIT], g[MAXIT] per lane and the
// float64 log-density are loaded ONCE, carried in registers over all the steps (an accepted end point is taken by select) and stored
// once at the end; between steps only the optional thinned trajectory goes to HBM.  A step is hmc_trajectory (hmc.hip), the very
// function hmc_step_kernel calls: n_steps launches of mfm_hmc_step / mfm_hmc_step_keys with the step keys below give the same bits
// (tests/test_gpu_hmc_run.py).
//
// Keys (mcmc_run_key), as mala_run.hip.  key_mode 0 (step-major): step j uses split(key, n_steps)[j] as mfm_hmc_step uses its key.
// key_mode 1 (chain-major): keys[b] is the chain's own key and step j uses split(keys[b], n_steps)[j].
// (Included by api.hip after hmc.hip and mala_run.hip: HmcArgs, hmc_trajectory, run_normal64 / run_uniform01 / run_exp, and
// resident.hip.h's mapping, key schedule, trajectory store and closing fence.)

struct HmcRunArgs {
  HmcArgs h;               // target, keys, beta, eps, leapfrog steps, state (in place), the LAST step's info (may be null)
  RunTail t;
};

// the draws and the exponential through mala_run.hip's out-of-line wrappers (the reason is stated there): same instructions, same bits
struct HmcCalled {
  __device__ __forceinline__ double normal(Key2 k, uint32_t idx, uint32_t size) const { return run_normal64(k, idx, size); }
  __device__ __forceinline__ double uniform(Key2 k) const { return run_uniform01(k); }
  __device__ __forceinline__ double operator()(double v) const { return run_exp(v); }
};

// a step's state and outcome: the resident chain's registers and the run's tallies
template <int MAXIT> struct HmcResident {
  float (&x)[MAXIT]; float (&g)[MAXIT]; double& lp;      // the chain: an accepted end point is taken by select
  bool acc; double pa;                                   // the step's outcome
  __device__ __forceinline__ void element(int it, int j, float& xo, float& go) const { xo = x[it]; go = g[it]; }
  __device__ __forceinline__ double logdensity() const { return lp; }
  template <int M> __device__ __forceinline__ void momentum(const double (&)[M], double, int, int) const {}
  template <int M> __device__ __forceinline__ void finish(bool acc_, double pa_, double lpe, const float (&xe)[M], const float (&ge)[M], int d, int lane) {
    const double lpe0 = __shfl(lpe, 0, 64);     // the value a single-step launch stores (lane 0's) and the next one loads in every lane
#pragma unroll
    for (int it = 0; it < M; ++it) {
      x[it] = acc_ ? xe[it] : x[it];
      g[it] = acc_ ? ge[it] : g[it];
    }
    lp = acc_ ? lpe0 : lp;
    acc = acc_; pa = pa_;
  }
};

template <int MAXIT, bool BCRT = false, bool MASS = false>
__global__ __launch_bounds__(MALA_WAVES * 64) void hmc_run_kernel(HmcRunArgs r) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const HmcArgs& a = r.h;
  const int d = a.T.dim, lane = threadIdx.x & 63, b = resident_chain_index();      // (own scalars: resident.hip.h says why)
  if (b >= a.B) return;
  const ResidentChain c(smem, d, a.B, lane, b);
  float* const xs = c.xs; float* const gsm = c.gsm; const size_t row = c.row;

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
  double acc_sum = 0.0, p_last = 0.0;
  bool acc_last = false;

  for (int s = 0; s < r.t.n_steps; ++s) {
    const Key2 kb = run_step_key(c, a, r.t, kc, s);
    HmcResident<MAXIT> st{x, g, lp, false, 0.0};
    hmc_trajectory<MAXIT, BCRT, MASS>(a.T, a.beta, a.eps, a.num_steps, kb, d, lane, xs, gsm, a.minv, st, HmcCalled());
    const bool acc = st.acc;
    const double p = st.pa;
    n_acc += acc ? 1 : 0;
    acc_sum += p;
    if (s == r.t.n_steps - 1) { p_last = p; acc_last = acc; }
    resident_snapshot(c, r.t, s, x, lp);
    resident_step_end();
  }

#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {                    // (the final store stays in line: resident.hip.h)
    const int j = lane + 64 * it;
    if (j < d) { a.pos[row + j] = x[it]; a.grad[row + j] = g[it]; }
  }
  if (lane == 0) {
    a.logp[b] = lp;
    if (r.t.n_acc) r.t.n_acc[b] = n_acc;
    if (r.t.acc_sum) r.t.acc_sum[b] = acc_sum;
    if (a.acc_prob) a.acc_prob[b] = (float)p_last;
    if (a.accepted) a.accepted[b] = acc_last ? 1 : 0;
  }
}

int launch_hmc_run(const HmcRunArgs& r, hipStream_t stream) {
  const HmcArgs& a = r.h;
  if (a.minv) HMC_MASS_DISPATCH(hmc_run_kernel, r); else MALA_DISPATCH(hmc_run_kernel, r);
  return 0;
}
