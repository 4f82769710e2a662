// The resident chain: what mala_run_kernel (mala_run.hip), hmc_run_kernel (hmc_run.hip) and hmc_warmup_kernel / mala_warmup_kernel
// (warmup.hip) share.  One wave per chain, MALA_WAVES chains per workgroup, the step's row staged in the wave's own LDS row between
// its two pads (the mapping of mala_step_kernel / hmc_step_kernel); x[MAXIT], g[MAXIT] per lane and the float64 log-density are loaded
// ONCE, carried in registers over all the steps and stored once at the end.  Here: the tail of the run arguments, the wave-to-chain
// mapping with the pad stores, the key schedule, the thinned trajectory store, the fence that ends a step and the residency load.
// A: MalaArgs or HmcArgs.  The MALA step both MALA kernels call is mala_resident_step (mala_run.hip), the HMC step hmc_trajectory
// (hmc.hip).  NOT shared, on purpose: the final store of x, g, lp (all four kernels) and the residency load of the two HMC kernels --
// every helper form tried moved scratch or spills of the large instances (DESIGN.md section 4.8 has the figures per form).
// (Included by mala_run.hip, after mala.hip: MALA_WAVES, MALA_MAXD_SMALL, mcmc_run_key.)
#pragma once

// the common tail of MalaRunArgs and HmcRunArgs
struct RunTail {
  int key_mode;
  int n_steps, thin;       // thin >= 1: the state after step j is kept when (j + 1) % thin == 0; 0: no trajectory
  int32_t* n_acc;          // [B] accepted steps (may be null)
  double* acc_sum;         // [B] sum of the acceptance probabilities (may be null)
  float* traj_pos;         // [n_steps / thin][B][d] (may be null)
  double* traj_logp;       // [n_steps / thin][B] (may be null)
};

// The wave-to-chain mapping.  A kernel states d, lane and its chain b as its own scalars, straight from the launch arguments and
// threadIdx -- `const int d = a.T.dim, lane = threadIdx.x & 63, b = resident_chain_index(); if (b >= a.B) return;` (wave-uniform; no
// workgroup barrier anywhere) -- because the compiler's inter-procedural range inference runs before these helpers are inlined: with
// d / lane reaching row_value_grad through a struct it no longer proved them non-negative, and the single-step kernels that share the
// out-of-line row functions compiled to signed compares.  ResidentChain is the rest: the wave's LDS row xs between its two pads
// (pads()), the mixtures' gradient scratch gsm, and the chain's place in the [B][d] arrays.
__device__ __forceinline__ int resident_chain_index() { return blockIdx.x * MALA_WAVES + (threadIdx.x >> 6); }
struct ResidentChain {
  int d, lane, b;
  float *xs, *gsm;
  size_t row, B;           // the chain's first element in a [B][d] array; the chain count
  __device__ __forceinline__ ResidentChain(float* smem, int dim, int n_chains, int lane_, int b_) : d(dim), lane(lane_), b(b_) {
    const int wave = threadIdx.x >> 6, rowlen = dim + 2;
    xs = smem + wave * rowlen + 1;
    gsm = smem + MALA_WAVES * rowlen + wave * MALA_MAXD_SMALL;
    row = (size_t)b * dim; B = (size_t)n_chains;
  }
  // the row's two pads; a kernel writes them after its residency load, where it always did (from the constructor, ahead of the loads,
  // hmc_run_kernel<16> gained a spill instruction)
  __device__ __forceinline__ void pads() const { if (lane == 0) { xs[-1] = 0.f; xs[d] = 0.f; } }
};

// The chain's state, resident in registers: loaded once (0 past d), carried over all the steps, stored once.  The arrays are this
// struct's own and the load returns it by value; the two MALA kernels use it.  The two HMC kernels keep the load in line: through this
// helper hmc_run_kernel<16>, hmc_warmup_kernel<16, true, true> and <32, false, true> gain 1 to 4 VGPR spill instructions, and with the
// kernels' arrays handed in by reference more.  The final store stays in line in the kernels: as a helper, on the kernels' arrays by
// reference or on this struct, it moved the scratch of the MAXIT 16 HMC instances (DESIGN.md section 4.8 has the figures).
template <int MAXIT> struct ResidentState { float x[MAXIT], g[MAXIT]; double lp; };
template <int MAXIT, class A> __device__ __forceinline__ ResidentState<MAXIT> resident_load(const ResidentChain& c, const A& a) {
  ResidentState<MAXIT> s;
  s.lp = a.logp[c.b];
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = c.lane + 64 * it;
    const size_t e = c.row + j;              // (one index for both arrays: written twice, each add has one use and is split into two address computations)
    s.x[it] = 0.f; s.g[it] = 0.f;
    if (j < c.d) { s.x[it] = a.pos[e]; s.g[it] = a.grad[e]; }
  }
  return s;
}

// the chain's own key (key_mode 1), and step s's chain key in either mode (mcmc_run_key)
template <class A> __device__ __forceinline__ Key2 run_chain_key(const ResidentChain& c, const A& a, const RunTail& t) {
  return t.key_mode ? Key2{a.keys[2 * c.b], a.keys[2 * c.b + 1]} : Key2{0, 0};
}
template <class A> __device__ __forceinline__ Key2 run_step_key(const ResidentChain& c, const A& a, const RunTail& t, Key2 kc, int s) {
  return mcmc_run_key(t.key_mode, a.key, kc, (uint32_t)t.n_steps, (uint32_t)s, a.n_total, a.chain_offset + (uint32_t)c.b);
}

// the next step overwrites the row (and the mixtures' gradient scratch) that other lanes of this wave have just read
__device__ __forceinline__ void resident_step_end() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the thinned trajectory: the state after step s (from 0), where it is kept
template <int MAXIT>
__device__ __forceinline__ void resident_snapshot(const ResidentChain& c, const RunTail& t, int s, const float (&x)[MAXIT], double lp) {
  if (t.thin > 0 && (s + 1) % t.thin == 0) {
    const size_t snap = (size_t)((s + 1) / t.thin - 1);
    if (t.traj_pos) {
#pragma unroll
      for (int it = 0; it < MAXIT; ++it) {
        const int j = c.lane + 64 * it;
        if (j < c.d) t.traj_pos[(snap * c.B + (size_t)c.b) * (size_t)c.d + j] = x[it];
      }
    }
    if (t.traj_logp && c.lane == 0) t.traj_logp[snap * c.B + (size_t)c.b] = lp;
  }
}
