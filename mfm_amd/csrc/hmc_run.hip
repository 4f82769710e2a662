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
// (Included by api.hip after hmc.hip and mala_run.hip: HmcArgs, hmc_trajectory, run_normal64 / run_uniform01 / run_exp.)

struct HmcRunArgs {
  HmcArgs h;               // target, keys, beta, eps, leapfrog steps, state (in place), the LAST step's info (may be null)
  int key_mode;
  int n_steps, thin;       // thin >= 1: the state after step j is kept when (j + 1) % thin == 0; 0: no trajectory
  int32_t* n_acc;          // [B] accepted steps (may be null)
  double* acc_sum;         // [B] sum of the acceptance probabilities (may be null)
  float* traj_pos;         // [n_steps / thin][B][d] (may be null)
  double* traj_logp;       // [n_steps / thin][B] (may be null)
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
  const int d = a.T.dim, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rowlen = d + 2;
  const int b = blockIdx.x * MALA_WAVES + wave;
  if (b >= a.B) return;                                   // (wave-uniform; no workgroup barrier below)
  float* const xs = smem + wave * rowlen + 1;
  float* const gsm = smem + MALA_WAVES * rowlen + wave * MALA_MAXD_SMALL;
  const size_t row = (size_t)b * d;
  const size_t B = (size_t)a.B;

  float x[MAXIT], g[MAXIT];
  double lp = a.logp[b];
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    x[it] = 0.f; g[it] = 0.f;
    if (j < d) { x[it] = a.pos[row + j]; g[it] = a.grad[row + j]; }
  }
  if (lane == 0) { xs[-1] = 0.f; xs[d] = 0.f; }
  const Key2 kc = r.key_mode ? Key2{a.keys[2 * b], a.keys[2 * b + 1]} : Key2{0, 0};
  int n_acc = 0;
  double acc_sum = 0.0, p_last = 0.0;
  bool acc_last = false;

  for (int s = 0; s < r.n_steps; ++s) {
    const Key2 kb = mcmc_run_key(r.key_mode, a.key, kc, (uint32_t)r.n_steps, (uint32_t)s, a.n_total, a.chain_offset + (uint32_t)b);
    HmcResident<MAXIT> st{x, g, lp, false, 0.0};
    hmc_trajectory<MAXIT, BCRT, MASS>(a.T, a.beta, a.eps, a.num_steps, kb, d, lane, xs, gsm, a.minv, st, HmcCalled());
    const bool acc = st.acc;
    const double p = st.pa;
    n_acc += acc ? 1 : 0;
    acc_sum += p;
    if (s == r.n_steps - 1) { p_last = p; acc_last = acc; }
    if (r.thin > 0 && (s + 1) % r.thin == 0) {
      const size_t snap = (size_t)((s + 1) / r.thin - 1);
      if (r.traj_pos) {
#pragma unroll
        for (int it = 0; it < MAXIT; ++it) {
          const int j = lane + 64 * it;
          if (j < d) r.traj_pos[(snap * B + (size_t)b) * (size_t)d + j] = x[it];
        }
      }
      if (r.traj_logp && lane == 0) r.traj_logp[snap * B + (size_t)b] = lp;
    }
    // the next step's first drift overwrites the row (and the mixtures' gradient scratch) that other lanes of this wave have just read
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }

#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    if (j < d) { a.pos[row + j] = x[it]; a.grad[row + j] = g[it]; }
  }
  if (lane == 0) {
    a.logp[b] = lp;
    if (r.n_acc) r.n_acc[b] = n_acc;
    if (r.acc_sum) r.acc_sum[b] = acc_sum;
    if (a.acc_prob) a.acc_prob[b] = (float)p_last;
    if (a.accepted) a.accepted[b] = acc_last ? 1 : 0;
  }
}

int launch_hmc_run(const HmcRunArgs& r, hipStream_t stream) {
  const HmcArgs& a = r.h;
  if (a.minv) HMC_MASS_DISPATCH(hmc_run_kernel, r); else MALA_DISPATCH(hmc_run_kernel, r);
  return 0;
}
