// K1r: n_steps MALA steps of every chain in ONE launch (mfm_mala_run).  The reference's `inference_loop0` (mcmc_utils.py:11-25:
// scan the vmapped kernel over split(rng, n_iter)) and the host loop of tempered.py:126-137, with the chain resident in the wave.
//
// Same mapping as mala_step_kernel (mala.hip): one wave per chain, MALA_WAVES chains per workgroup, the proposal row staged in the
// wave's own LDS row between its two pads, the same MAXIT / BCRT instances.  What differs is residency: x[MAXIT], g[MAXIT] per lane and
// the float64 log-density are loaded ONCE, carried in registers over all the steps (an accepted proposal is taken by select) and stored
// once at the end; between steps only the optional thinned trajectory goes to HBM.  The arithmetic of a step is mala_chain_step's,
// through mcmc.hip.h (the strict form; same draws, same reductions): n_steps launches of mfm_mala_step / mfm_mala_step_keys with
// the step keys below give the same bits (tests/test_gpu_mala_run.py).
//
// Keys (mcmc_run_key).  key_mode 0 (step-major): step j uses split(key, n_steps)[j] as mfm_mala_step uses its key.  key_mode 1
// (chain-major): keys[b] is the chain's own key and step j uses split(keys[b], n_steps)[j].  Draws are always made in line.
// The mapping, the key schedule, the thinned trajectory store and the step's closing fence are resident.hip.h's, shared with
// hmc_run.hip and warmup.hip; a step is mala_resident_step below, which mala_warmup_kernel (warmup.hip) calls with eps per step.
// (Included by api.hip after mala.hip: MalaArgs, row_value_grad, MALA_DISPATCH.)

#include "resident.hip.h"

struct MalaRunArgs {
  MalaArgs m;              // target, keys, beta, eps, textbook, state (in place), the LAST step's info (may be null); pre_n / pre_u unused
  RunTail t;
};

// The float64 draws and the acceptance exponential are CALLED, not inlined.  Their double-precision polynomial coefficients cannot be
// instruction literals; inlined into the step loop they are hoisted out of it and held in registers over all the steps, which takes the
// whole 256-VGPR file plus accumulation registers (one wave per SIMD).  Out of line they live only inside the call: MAXIT = 4 compiles to
// 150 VGPRs, three waves per SIMD.  Same instructions on the same operands, so the same bits.
__device__ __attribute__((noinline)) double run_normal64(Key2 key, uint32_t idx, uint32_t size) { return normal64(key, idx, size); }
__device__ __attribute__((noinline)) double run_uniform01(Key2 key) { return uniform01(key, 0, 1); }
__device__ __attribute__((noinline)) double run_exp(double v) { return exp(v); }
__device__ __attribute__((noinline)) double run_sqrt(double v) { return sqrt(v); }      // (mclmc.hip)
struct RunExp { __device__ __forceinline__ double operator()(double v) const { return run_exp(v); } };

// The resident chain's registers and a step's outcome, as mala_resident_step sees them (HmcResident's counterpart, hmc_run.hip)
template <int MAXIT> struct MalaResident {
  float (&x)[MAXIT]; float (&g)[MAXIT]; double& lp;      // the chain: an accepted proposal is taken by select
  float (&xn)[MAXIT];                                    // the last proposal (MalaArgs::proposed)
  bool acc; double p;                                    // the step's outcome: accepted, the acceptance probability,
  double lpn, th2;                                       // the proposal's log-density in this lane and the reduced back term (mala_prop_weight)
  __device__ __forceinline__ void element(int it, float& xo, float& go) const { xo = x[it]; go = g[it]; }
  __device__ __forceinline__ double logdensity() const { return lp; }
  template <int M> __device__ __forceinline__ void finish(bool acc_, double p_, double lpn_, double th2_, const float (&xe)[M], const float (&ge)[M]) {
    const double lpn0 = __shfl(lpn_, 0, 64);    // the value a single-step launch stores (lane 0's) and the next one loads in every lane
#pragma unroll
    for (int it = 0; it < M; ++it) {
      x[it] = acc_ ? xe[it] : x[it];
      g[it] = acc_ ? ge[it] : g[it];
      xn[it] = xe[it];
    }
    lp = acc_ ? lpn0 : lp;
    acc = acc_; p = p_; lpn = lpn_; th2 = th2_;
  }
};

// ONE MALA step of the resident chain, with the step's chain key kb: every step of mala_run_kernel and of mala_warmup_kernel
// (warmup.hip).  mala_chain_step's arithmetic through mcmc.hip.h, in the strict form (same draws, same reductions).  eps and
// s2e = mala_s2e(eps) are the caller's: loop-invariant in the run, this wave's own per step in the warmup.  The shape is
// hmc_trajectory's (hmc.hip, DESIGN.md sections 4.8 / 4.10): the state comes through `st` into this function's OWN arrays and the
// outcome goes back through st.finish -- with the kernel's arrays handed in by reference the large instances lose a wave or spill.
// xs: the wave's LDS row (pads written), gsm: the mixtures' gradient scratch; the caller ends the step with resident_step_end.
template <int MAXIT, bool BCRT, class State>
__device__ __forceinline__ void mala_resident_step(const TargetDev& T, double beta, double eps, double s2e, int textbook, Key2 kb, int d, int lane,
                                                   float* xs, float* gsm, State& st) {
  const Key2 k_int = mcmc_step_key(kb, MCMC_K_INT), k_rmh = mcmc_step_key(kb, MCMC_K_RMH);
  float x[MAXIT], g[MAXIT], xn[MAXIT], gn[MAXIT];
  double th1 = 0.0;                       // |x' - x - eps g|^2 = 2 eps |noise|^2
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    st.element(it, x[it], g[it]);
    xn[it] = 0.f; gn[it] = 0.f;
    if (j < d) {
      const double n = (double)(draw_t)run_normal64(k_int, (uint32_t)j, (uint32_t)d);
      xn[it] = mala_propose<false>(x[it], g[it], n, eps, s2e, th1);
      xs[j] = xn[it];
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");       // the stencil reads its neighbours' proposal elements from this wave's row
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  const double lpn = row_value_grad<MAXIT, BCRT>(T, beta, xs, d, lane, gn, gsm);
  double th2 = 0.0;                       // |x - x' - eps g'|^2
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    if (j < d) mala_back<false>(x[it], xn[it], gn[it], eps, th2);
  }
  th1 = wave_sum(th1); th2 = wave_sum(th2);
  const double p = mala_accept_p<false>(st.logdensity(), lpn, th1, th2, eps, textbook, RunExp());
  const double u = run_uniform01(k_rmh);
  st.template finish<MAXIT>(u < p, p, lpn, th2, xn, gn);
}

template <int MAXIT, bool BCRT = false>
__global__ __launch_bounds__(MALA_WAVES * 64) void mala_run_kernel(MalaRunArgs r) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const MalaArgs& a = r.m;
  const int d = a.T.dim, lane = threadIdx.x & 63, b = resident_chain_index();      // (own scalars: resident.hip.h says why)
  if (b >= a.B) return;
  const ResidentChain c(smem, d, a.B, lane, b);
  float* const xs = c.xs; float* const gsm = c.gsm; const size_t row = c.row;

  ResidentState<MAXIT> cs = resident_load<MAXIT>(c, a);
  float (&x)[MAXIT] = cs.x; float (&g)[MAXIT] = cs.g; double& lp = cs.lp;
  c.pads();
  float xn[MAXIT];
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) xn[it] = 0.f;
  const Key2 kc = run_chain_key(c, a, r.t);
  const double s2e = mala_s2e(a.eps);
  int n_acc = 0;
  double acc_sum = 0.0, p_last = 0.0, pw_last = 0.0;
  bool acc_last = false;

  for (int s = 0; s < r.t.n_steps; ++s) {
    const Key2 kb = run_step_key(c, a, r.t, kc, s);
    MalaResident<MAXIT> st{x, g, lp, xn, false, 0.0, 0.0, 0.0};
    mala_resident_step<MAXIT, BCRT>(a.T, a.beta, a.eps, s2e, a.textbook, kb, d, lane, xs, gsm, st);
    const bool acc = st.acc;
    const double p = st.p;
    n_acc += acc ? 1 : 0;
    acc_sum += p;
    if (s == r.t.n_steps - 1) {
      p_last = p; acc_last = acc;
      if (a.prop_weight) pw_last = mala_prop_weight(st.lpn, st.th2, a.eps, RunExp());
    }
    resident_snapshot(c, r.t, s, x, lp);
    resident_step_end();
  }

#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {                    // (the final store stays in line: resident.hip.h)
    const int j = lane + 64 * it;
    if (j < d) {
      a.pos[row + j] = x[it]; a.grad[row + j] = g[it];
      if (a.proposed) a.proposed[row + j] = xn[it];
    }
  }
  if (lane == 0) {
    a.logp[b] = lp;
    if (r.t.n_acc) r.t.n_acc[b] = n_acc;
    if (r.t.acc_sum) r.t.acc_sum[b] = acc_sum;
    if (a.acc_prob) a.acc_prob[b] = (float)p_last;
    if (a.accepted) a.accepted[b] = acc_last ? 1 : 0;
    if (a.prop_weight) a.prop_weight[b] = (float)pw_last;
  }
}

int launch_mala_run(const MalaRunArgs& r, hipStream_t stream) {
  const MalaArgs& a = r.m;
  MALA_DISPATCH(mala_run_kernel, r);
  return 0;
}

// ---- the Cox process: its step is the 16-chain tile of lgcp.hip, so mfm_mala_run issues n_steps of those launches back to back; these two
// tiny kernels keep the key schedule and the per-chain tallies on the device (no host synchronisation between the steps) ----
__global__ void mala_run_keys_kernel(int key_mode, Key2 key, const uint32_t* keys, uint32_t n_steps, uint32_t s, uint32_t n_total,
                                     uint32_t chain_offset, int B, uint32_t* out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const Key2 kb = mcmc_run_key(key_mode, key, key_mode ? Key2{keys[2 * b], keys[2 * b + 1]} : Key2{0, 0}, n_steps, s, n_total, chain_offset + (uint32_t)b);
  out[2 * b] = kb.k0; out[2 * b + 1] = kb.k1;
}

__global__ void mala_run_tally_kernel(int B, const float* acc_prob, const uint8_t* accepted, int32_t* n_acc, double* acc_sum) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  if (n_acc) n_acc[b] += accepted[b] ? 1 : 0;
  if (acc_sum) acc_sum[b] += (double)acc_prob[b];
}
