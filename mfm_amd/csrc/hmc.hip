// Hamiltonian Monte Carlo step over parallel chains, one wavefront per chain -- a BUILD-SIDE MODE: BASELINE.json's north star names a
// "MALA/HMC log-density-and-grad step", the reference's MFM loop has MALA only and vendors no hmc.py (SURVEY.md note 7).  The kernel
// follows blackjax's HMC (the package the reference's bblackjax was cut from), restated in oracle/hmc.py: momentum ~ N(0, I) from
// split(key, 2)[0], num_steps velocity-Verlet steps (half kick, drift, value-and-gradient, half kick), H = -logp + |p|^2 / 2,
// accept with min(1, exp(H_0 - H_end)) against uniform(split(key, 2)[1]) (the accept rule's tail: mcmc.hip.h).
// Layout as the MALA kernel (mala.hip): positions / gradients float32, log-density float64; the momentum lives in float64 registers,
// the trajectory's position is rounded to float32 after every drift (it is what the target is evaluated at); energies are summed in
// float64 over the wave.  Targets: phi-four and the Gaussian mixtures (row_value_grad); the Cox process needs the K^-1 GEMM tile
// (lgcp.hip) and is not served.
// With a diagonal inverse mass matrix minv (mfm_hmc_set_inverse_mass; blackjax's inverse_mass_matrix as a vector) the MASS instances run:
// momentum p_j = n_j / sqrt(minv_j), H = -logp + sum_j minv_j p_j^2 / 2, drift x_j += eps minv_j p_j.  Every product with minv is written
// so that minv == 1 gives the unit instances' bits (1 * p and n / 1 are exact); the unit instances are compiled from the lines they
// always had.
#pragma once
// (included by api.hip after mala.hip: mcmc.hip.h, MalaArgs' helpers row_value_grad, ROW_DISPATCH / MALA_DISPATCH, mala_smem)

struct HmcArgs {
  TargetDev T;
  Key2 key;
  const uint32_t* keys;   // non-null: one key per chain [B][2] (mfm_hmc_step_keys; mfm_hmc_run in key_mode 1), as MalaArgs::keys
  uint32_t n_total, chain_offset;
  int B, num_steps;
  double beta, eps;
  float* pos; double* logp; float* grad;              // state, updated in place
  float* acc_prob; uint8_t* accepted;                 // info (may be null)
  const double* minv;                                 // [d] diagonal of the inverse mass matrix: read by the MASS instances only
};

// the float64 draws and the acceptance exponential as a single-step launch makes them: in line (hmc_run.hip calls them out of line)
struct HmcInline {
  __device__ __forceinline__ double normal(Key2 k, uint32_t idx, uint32_t size) const { return normal64(k, idx, size); }
  __device__ __forceinline__ double uniform(Key2 k) const { return uniform01(k, 0, 1); }
  __device__ __forceinline__ double operator()(double v) const { return exp(v); }
};
// where a step's state comes from and where its outcome goes: HBM for a single-step launch (hmc_run.hip: the registers of the
// resident chain)
struct HmcInHbm {
  const HmcArgs& a; size_t row; int b;
  __device__ __forceinline__ void element(int it, int j, float& x, float& g) const { x = a.pos[row + j]; g = a.grad[row + j]; }
  __device__ __forceinline__ double logdensity() const { return a.logp[b]; }
  template <int MAXIT> __device__ __forceinline__ void momentum(const double (&)[MAXIT], double, int, int) const {}      // (hmc_trajectory: for chees.hip's sink)
  // an accepted end point replaces the state; the step's info
  template <int MAXIT> __device__ __forceinline__ void finish(bool acc, double pa, double lp, const float (&x)[MAXIT], const float (&g)[MAXIT], int d, int lane) const {
    if (acc) {
#pragma unroll
      for (int it = 0; it < MAXIT; ++it) {
        const int j = lane + 64 * it;
        if (j < d) { a.pos[row + j] = x[it]; a.grad[row + j] = g[it]; }
      }
    }
    if (lane == 0) {
      if (acc) a.logp[b] = lp;
      if (a.acc_prob) a.acc_prob[b] = (float)pa;
      if (a.accepted) a.accepted[b] = acc ? 1 : 0;
    }
  }
};

// ONE HMC step of the chain this wave holds, with the step's chain key kb: the whole body of hmc_step_kernel and of every step of
// hmc_run_kernel (hmc_run.hip).  The state's elements j = lane + 64 * it come through `st` (each beside its momentum draw, the
// log-density after them: the order the step kernel has always had), and the outcome goes back through st.finish: whether the end
// point was accepted, the acceptance probability, the end point's log-density as row_value_grad returns it in this lane, and its
// x / g (0 past d).  Two things keep hmc_step_kernel<16> / <32> out of scratch memory and are not to be tidied away (DESIGN.md section
// 4.10 has the figures): the trajectory's x, g and momentum are this function's OWN arrays, not the caller's handed in by reference;
// and the state is read into x0 / g0 and copied to x / g, as the step kernel always did.  xs: the wave's LDS row (pads written), gsm: the mixtures'
// gradient scratch; both are left as the last row_value_grad read them (no trailing barrier).
// MASS: minv[j] is the diagonal of the inverse mass matrix (see the head of this file).  It stays in registers through MAXIT 4 and is
// read again from its d * 8 cache-resident bytes at every use above (DESIGN.md section 4.12 has the figures); !MASS never reads it.
template <int MAXIT, bool BCRT, bool MASS, class State, class Draw>
__device__ __forceinline__ void hmc_trajectory(const TargetDev& T, double beta, double eps, int num_steps, Key2 kb, int d, int lane,
                                               float* xs, float* gsm, const double* minv, State& st, Draw dr) {
#pragma clang fp contract(off)
  const Key2 k_mom = mcmc_step_key(kb, MCMC_K_INT), k_acc = mcmc_step_key(kb, MCMC_K_RMH);
  float x0[MAXIT], g0[MAXIT], x[MAXIT], g[MAXIT];      // (x0 / g0: the state as it comes, see above)
  double p[MAXIT];
  constexpr bool MREG = MASS && MAXIT <= 4;            // minv in registers
  double mi[MREG ? MAXIT : 1];
  double kin = 0.0;
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    x0[it] = 0.f; g0[it] = 0.f; p[it] = 0.0;
    if constexpr (MREG) mi[it] = 1.0;
    if (j < d) {
      st.element(it, j, x0[it], g0[it]);
      if constexpr (MASS) {
        const double m = minv[j];
        if constexpr (MREG) mi[it] = m;
        p[it] = dr.normal(k_mom, (uint32_t)j, (uint32_t)d) / sqrt(m);
        kin += m * p[it] * p[it];
      } else {
      p[it] = dr.normal(k_mom, (uint32_t)j, (uint32_t)d);
      kin += p[it] * p[it];
      }
    }
    x[it] = x0[it]; g[it] = g0[it];
  }
  const double lp0 = st.logdensity();
  const double h0 = -lp0 + 0.5 * wave_sum(kin);
  double lp = lp0;
  for (int s = 0; s < num_steps; ++s) {
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int j = lane + 64 * it;
      if (j < d) {
        p[it] = p[it] + 0.5 * eps * (double)g[it];                       // half kick
        if constexpr (MASS) {
          const double m = MREG ? mi[MREG ? it : 0] : minv[j];
          x[it] = (float)((double)x[it] + eps * (m * p[it]));            // drift
        } else
        x[it] = (float)((double)x[it] + eps * p[it]);                    // drift
        xs[j] = x[it];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");       // the stencil reads its neighbours' elements from this wave's row
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    lp = row_value_grad<MAXIT, BCRT>(T, beta, xs, d, lane, g, gsm);
    __builtin_amdgcn_wave_barrier();                             // (the next drift overwrites the row)
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int j = lane + 64 * it;
      if (j < d) p[it] = p[it] + 0.5 * eps * (double)g[it];             // half kick
    }
  }
  double kin1 = 0.0;
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
  const double pa = mala_accept_p(h0 - h1, dr);
  const bool acc = dr.uniform(k_acc) < pa;
  st.template momentum<MAXIT>(p, h1 - h0, d, lane);      // the end momentum and H_end - H_0, for a sink that keeps them (chees.hip); empty in the others
  st.template finish<MAXIT>(acc, pa, lp, x, g, d, lane);
}

template <int MAXIT, bool BCRT = false, bool MASS = false>      // BCRT: as mala.hip's row kernels; MASS: hmc_trajectory
__global__ __launch_bounds__(MALA_WAVES * 64) void hmc_step_kernel(HmcArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int d = a.T.dim, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rowlen = d + 2;
  const int b = blockIdx.x * MALA_WAVES + wave;
  if (b >= a.B) return;
  float* xs = smem + wave * rowlen + 1;
  float* gsm = smem + MALA_WAVES * rowlen + wave * MALA_MAXD_SMALL;
  const Key2 kb = mcmc_chain_key(a.key, a.keys, a.n_total, a.chain_offset, b);
  if (lane == 0) { xs[-1] = 0.f; xs[d] = 0.f; }
  HmcInHbm st{a, (size_t)b * d, b};
  hmc_trajectory<MAXIT, BCRT, MASS>(a.T, a.beta, a.eps, a.num_steps, kb, d, lane, xs, gsm, a.minv, st, HmcInline());
}

// ROW_DISPATCH (mala.hip) onto the MASS instances of the three HMC kernels
#define HMC_MASS() , true
#define HMC_MASS_DISPATCH(KERN, ...) ROW_DISPATCH(KERN, HMC_MASS, __VA_ARGS__)

// (a.minv non-null: the MASS instances)
int launch_hmc_step(const HmcArgs& a, hipStream_t stream) {
  if (a.minv) HMC_MASS_DISPATCH(hmc_step_kernel, a); else MALA_DISPATCH(hmc_step_kernel, a);
  return 0;
}
