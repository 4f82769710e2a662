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
// (Included by api.hip after mala.hip: MalaArgs, row_value_grad, MALA_DISPATCH.)

struct MalaRunArgs {
  MalaArgs m;              // target, keys, beta, eps, textbook, state (in place), the LAST step's info (may be null); pre_n / pre_u unused
  int key_mode;
  int n_steps, thin;       // thin >= 1: the state after step j is kept when (j + 1) % thin == 0; 0: no trajectory
  int32_t* n_acc;          // [B] accepted steps (may be null)
  double* acc_sum;         // [B] sum of the acceptance probabilities (may be null)
  float* traj_pos;         // [n_steps / thin][B][d] (may be null)
  double* traj_logp;       // [n_steps / thin][B] (may be null)
};

// The float64 draws and the acceptance exponential are CALLED, not inlined.  Their double-precision polynomial coefficients cannot be
// instruction literals; inlined into the step loop they are hoisted out of it and held in registers over all the steps, which takes the
// whole 256-VGPR file plus accumulation registers (one wave per SIMD).  Out of line they live only inside the call: MAXIT = 4 compiles to
// 150 VGPRs, three waves per SIMD.  Same instructions on the same operands, so the same bits.
__device__ __attribute__((noinline)) double run_normal64(Key2 key, uint32_t idx, uint32_t size) { return normal64(key, idx, size); }
__device__ __attribute__((noinline)) double run_uniform01(Key2 key) { return uniform01(key, 0, 1); }
__device__ __attribute__((noinline)) double run_exp(double v) { return exp(v); }
struct RunExp { __device__ __forceinline__ double operator()(double v) const { return run_exp(v); } };

template <int MAXIT, bool BCRT = false>
__global__ __launch_bounds__(MALA_WAVES * 64) void mala_run_kernel(MalaRunArgs r) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const MalaArgs& a = r.m;
  const int d = a.T.dim, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rowlen = d + 2;
  const int b = blockIdx.x * MALA_WAVES + wave;
  if (b >= a.B) return;                                   // (wave-uniform; no workgroup barrier below)
  float* const xs = smem + wave * rowlen + 1;
  float* const gsm = smem + MALA_WAVES * rowlen + wave * MALA_MAXD_SMALL;
  const size_t row = (size_t)b * d;
  const size_t B = (size_t)a.B;

  float x[MAXIT], g[MAXIT], xn[MAXIT];
  double lp = a.logp[b];
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    x[it] = 0.f; g[it] = 0.f; xn[it] = 0.f;
    if (j < d) { x[it] = a.pos[row + j]; g[it] = a.grad[row + j]; }
  }
  if (lane == 0) { xs[-1] = 0.f; xs[d] = 0.f; }
  const Key2 kc = r.key_mode ? Key2{a.keys[2 * b], a.keys[2 * b + 1]} : Key2{0, 0};
  const double s2e = mala_s2e(a.eps);
  int n_acc = 0;
  double acc_sum = 0.0, p_last = 0.0, pw_last = 0.0;
  bool acc_last = false;

  for (int s = 0; s < r.n_steps; ++s) {
    const Key2 kb = mcmc_run_key(r.key_mode, a.key, kc, (uint32_t)r.n_steps, (uint32_t)s, a.n_total, a.chain_offset + (uint32_t)b);
    const Key2 k_int = mcmc_step_key(kb, MCMC_K_INT), k_rmh = mcmc_step_key(kb, MCMC_K_RMH);
    double th1 = 0.0;                       // |x' - x - eps g|^2 = 2 eps |noise|^2
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int j = lane + 64 * it;
      if (j < d) {
        const double n = (double)(draw_t)run_normal64(k_int, (uint32_t)j, (uint32_t)d);
        xn[it] = mala_propose<false>(x[it], g[it], n, a.eps, s2e, th1);
        xs[j] = xn[it];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");       // the stencil reads its neighbours' proposal elements from this wave's row
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

    float gn[MAXIT];
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) gn[it] = 0.f;
    const double lpn = row_value_grad<MAXIT, BCRT>(a.T, a.beta, xs, d, lane, gn, gsm);
    double th2 = 0.0;                       // |x - x' - eps g'|^2
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int j = lane + 64 * it;
      if (j < d) mala_back<false>(x[it], xn[it], gn[it], a.eps, th2);
    }
    th1 = wave_sum(th1); th2 = wave_sum(th2);
    const double p = mala_accept_p<false>(lp, lpn, th1, th2, a.eps, a.textbook, RunExp());
    const double u = run_uniform01(k_rmh);
    const bool acc = u < p;
    const double lpn0 = __shfl(lpn, 0, 64);     // the value a single-step launch stores (lane 0's) and the next one loads in every lane
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      x[it] = acc ? xn[it] : x[it];
      g[it] = acc ? gn[it] : g[it];
    }
    lp = acc ? lpn0 : lp;
    n_acc += acc ? 1 : 0;
    acc_sum += p;
    if (s == r.n_steps - 1) {
      p_last = p; acc_last = acc;
      if (a.prop_weight) pw_last = mala_prop_weight(lpn, th2, a.eps, RunExp());
    }
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
    // the next step overwrites the row (and the mixtures' gradient scratch) that other lanes of this wave have just read
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }

#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    if (j < d) {
      a.pos[row + j] = x[it]; a.grad[row + j] = g[it];
      if (a.proposed) a.proposed[row + j] = xn[it];
    }
  }
  if (lane == 0) {
    a.logp[b] = lp;
    if (r.n_acc) r.n_acc[b] = n_acc;
    if (r.acc_sum) r.acc_sum[b] = acc_sum;
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
