// The No-U-turn sampler over parallel chains, one wavefront per chain -- a BUILD-SIDE MODE like hmc.hip: the reference vendors neither.
// Multinomial NUTS in the iterative, checkpointed form (Betancourt, "A Conceptual Introduction to Hamiltonian Monte Carlo", appendix A;
// the formulation of NumPyro and blackjax), restated in tests/nuts_ref.py.  A chain's tree has its own depth, and with one wave per
// chain and no workgroup barrier anywhere that is wave-uniform control flow: no chain waits for another's tree.
//
// Per chain, with the step's chain key kb:
//   k_mom, k_tree = split(kb, 2), the halves mfm_hmc_step uses; the momentum draw is hmc_trajectory's, n / sqrt(minv) included.
//   Doubling j = 0, 1, ... draws from kd = split(k_tree, 16)[j] (16 whatever max_tree_depth is: a tree under a smaller limit is a
//   prefix of the tree under a larger one) -> k_dir, k_leaf, k_merge = split(kd, 3): forward iff uniform(k_dir) < 0.5, leaf i of the
//   doubling's subtree draws uniform(split(k_leaf, 2^j)[i]), the merge uniform(k_merge).
//   The integrator is hmc_trajectory's leapfrog (half kick, drift with the position rounded to float32, row_value_grad, half kick;
//   float64 momentum, float32 gradient), with -eps backward.  H = -logp + sum(minv p^2) / 2; a leaf has delta = H0 - H (NaN -> -inf)
//   and weight exp(delta), and is DIVERGENT when H - H0 > threshold or delta was NaN.
//   A subtree of 2^j leaves from the tree's end point in the drawn direction keeps a running p_sum and logw = logaddexp(logw, delta);
//   leaf i replaces the subtree's proposal iff i == 0 or u_i < exp(delta - logw_new) (uniform progressive sampling).  Even i stores
//   (p, p_sum) in checkpoint slot popcount(i >> 1); odd i checks the slots from popcount(i >> 1) down, one per trailing one bit of i:
//   with s = p_sum - ckpt_psum + ckpt_p the leaf is TURNING iff (minv ckpt_p) . s <= 0 or (minv p) . s <= 0.  The subtree stops at the
//   first divergent or turning leaf; that ends the transition and none of its leaves is proposed.
//   A complete subtree's proposal replaces the tree's iff u < min(1, exp(logw_sub - logw_tree)) (biased progressive sampling); then
//   the weights and p_sums are added, the end point moves, and the same U-turn test runs on the tree's (p_left, p_right, p_sum): a
//   turning tree ends the transition with the merged proposal standing.  No cross-subtree checks beyond these.
//   The proposal's (x, g, logp) becomes the state.
//
// Registers: the tree's two end points as A, the end that is being extended, and B, the other one (x float32, p float64, g float32
// each); a doubling in the other direction swaps them, the U-turn tests being symmetric in the ends.  A is integrated in place: a
// subtree that stops early ends the transition, so nothing reads the end points again.  Beside them the tree's and the subtree's
// proposals (x, g) and p_sums, and with MASS the inverse mass: 16 (18) VGPRs per element and lane.
// LDS: the checkpoints are indexed by the leaf's bits at run time, so they live in the wave's own LDS, (max_tree_depth - 1) slots of
// 2 d float64 behind the rows of mala_smem; a lane reads back only what it stored, so they need no fence.  The launch chooses the
// chains per workgroup (nuts_waves) from dim and max_tree_depth against a CU's 160 KiB.
// Served: dim <= 256 (MAXIT 1 / 2 / 4); the larger instances need the checkpoints outside LDS.
#pragma once
// (included by api.hip after hmc_run.hip: HmcArgs, HmcInline / HmcCalled, ResidentChain, RunTail, run_step_key, resident_snapshot)

struct NutsArgs {
  HmcArgs h;                      // target, keys, beta, eps, state (in place), minv; num_steps / acc_prob / accepted unused
  int max_depth, waves;           // the limit on the doublings; chains per workgroup (nuts_waves)
  double div_thr;                 // a leaf with H - H0 above this is divergent
  int32_t* depth; int32_t* n_leap; uint8_t* turning; uint8_t* divergent; double* acc_rate; double* energy;      // info [B] (may be null)
};
struct NutsRunArgs {
  NutsArgs n;                     // (info: the LAST step's)
  RunTail t;                      // key_mode, n_steps, thin, trajectory; n_acc / acc_sum unused
  int64_t* tot_leap; double* tot_acc; int32_t* tot_div; int32_t* tot_depth;      // per-chain totals [B] (may be null)
};
// what a transition reports beside the state
struct NutsOut { int depth, n_leap, turning, divergent; double acc_rate, energy; };      // (no padding: copies stay in registers)

__device__ __attribute__((noinline)) double run_log1p(double v) { return log1p(v); }
struct NutsInline : HmcInline { __device__ __forceinline__ double log1p(double v) const { return ::log1p(v); } };
struct NutsCalled : HmcCalled { __device__ __forceinline__ double log1p(double v) const { return run_log1p(v); } };

// log(exp(a) + exp(b)) = max + log1p(exp(-|a - b|)); -inf when both are
template <class Draw> __device__ __forceinline__ double nuts_logaddexp(double a, double b, Draw dr) {
  const double m = fmax(a, b);
  if (m == -INFINITY) return m;
  return m + dr.log1p(dr(-fabs(a - b)));
}
// a wave-uniform decision as a scalar (every lane holds the same value: the sums are butterflies, the draws functions of the key)
__device__ __forceinline__ bool nuts_uniform(bool v) { return __builtin_amdgcn_readfirstlane(v ? 1 : 0) != 0; }

// a step's state and outcome in HBM: a single-step launch
struct NutsInHbm {
  const NutsArgs& n; size_t row; int b;
  __device__ __forceinline__ void element(int it, int j, float& x, float& g) const { x = n.h.pos[row + j]; g = n.h.grad[row + j]; }
  __device__ __forceinline__ double logdensity() const { return n.h.logp[b]; }
  template <int MAXIT> __device__ __forceinline__ void finish(const NutsOut& o, double lp, const float (&x)[MAXIT], const float (&g)[MAXIT], int d, int lane) const {
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int j = lane + 64 * it;
      if (j < d) { n.h.pos[row + j] = x[it]; n.h.grad[row + j] = g[it]; }
    }
    if (lane == 0) {
      n.h.logp[b] = lp;
      if (n.depth) n.depth[b] = o.depth;
      if (n.n_leap) n.n_leap[b] = o.n_leap;
      if (n.turning) n.turning[b] = (uint8_t)o.turning;
      if (n.divergent) n.divergent[b] = (uint8_t)o.divergent;
      if (n.acc_rate) n.acc_rate[b] = o.acc_rate;
      if (n.energy) n.energy[b] = o.energy;
    }
  }
};
// the resident chain's registers: every step of a run
template <int MAXIT> struct NutsResident {
  float (&x)[MAXIT]; float (&g)[MAXIT]; double& lp;
  NutsOut out;
  __device__ __forceinline__ void element(int it, int j, float& xo, float& go) const { xo = x[it]; go = g[it]; }
  __device__ __forceinline__ double logdensity() const { return lp; }
  template <int M> __device__ __forceinline__ void finish(const NutsOut& o, double lpe, const float (&xe)[M], const float (&ge)[M], int d, int lane) {
#pragma unroll
    for (int it = 0; it < M; ++it) { x[it] = xe[it]; g[it] = ge[it]; }
    lp = lpe; out = o;
  }
};

// ONE NUTS transition of the chain this wave holds, with the step's chain key kb: the whole body of nuts_step_kernel and of every
// step of nuts_run_kernel.  State and Draw as hmc_trajectory's (hmc.hip): the state comes through st.element / st.logdensity into this
// function's own arrays and the outcome goes back through st.finish.  xs: the wave's LDS row (pads written), gsm: the mixtures'
// gradient scratch, ck: the wave's checkpoints, (max_depth - 1) slots of [2][d] float64.  Every log-density is lane 0's value in all
// lanes, which is what a single-step launch stores and the next one loads.
template <int MAXIT, bool BCRT, bool MASS, class State, class Draw>
__device__ __forceinline__ void nuts_trajectory(const TargetDev& T, double beta, double eps, int max_depth, double div_thr, Key2 kb, int d, int lane,
                                                float* xs, float* gsm, double* ck, const double* minv, State& st, Draw dr) {
#pragma clang fp contract(off)
  const Key2 k_mom = mcmc_step_key(kb, MCMC_K_INT), k_tree = mcmc_step_key(kb, MCMC_K_RMH);
  float ax[MAXIT], ag[MAXIT], bx[MAXIT], bg[MAXIT];      // the end points: A is extended, B is the other one
  double ap[MAXIT], bp[MAXIT];
  float px[MAXIT], pg[MAXIT], sx[MAXIT], sg[MAXIT];      // the tree's and the subtree's proposals
  double ps[MAXIT], ss[MAXIT];                           // the tree's and the subtree's p_sum
  double mi[MASS ? MAXIT : 1];
  double kin = 0.0;
#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    px[it] = 0.f; pg[it] = 0.f; ap[it] = 0.0;
    if constexpr (MASS) mi[it] = 1.0;
    if (j < d) {
      st.element(it, j, px[it], pg[it]);
      double m = 1.0;
      if constexpr (MASS) { m = minv[j]; mi[it] = m; }
      ap[it] = dr.normal(k_mom, (uint32_t)j, (uint32_t)d) / sqrt(m);
      kin += m * ap[it] * ap[it];
    }
    ax[it] = px[it]; ag[it] = pg[it]; bx[it] = px[it]; bg[it] = pg[it]; bp[it] = ap[it]; ps[it] = ap[it];
    sx[it] = px[it]; sg[it] = pg[it]; ss[it] = 0.0;
  }
  const double lp0 = st.logdensity();
  const double h0 = -lp0 + 0.5 * wave_sum(kin);
  double plp = lp0, ph = h0;                             // the tree's proposal: log-density and energy
  double logw = 0.0, acc_sum = 0.0;                      // the start has delta 0
  bool a_fwd = true, turning = false, divergent = false;
  int depth = 0, n_leap = 0;

  for (int j = 0; j < max_depth; ++j) {
    const Key2 kd = split_at(k_tree, 16, (uint32_t)j);
    const Key2 k_dir = split_at(kd, 3, 0), k_leaf = split_at(kd, 3, 1), k_merge = split_at(kd, 3, 2);
    const bool fwd = nuts_uniform(dr.uniform(k_dir) < 0.5);
    if (fwd != a_fwd) {                                  // the other end is extended
#pragma unroll
      for (int it = 0; it < MAXIT; ++it) {
        const float tx = ax[it], tg = ag[it]; const double tp = ap[it];
        ax[it] = bx[it]; ag[it] = bg[it]; ap[it] = bp[it];
        bx[it] = tx; bg[it] = tg; bp[it] = tp;
      }
      a_fwd = fwd;
    }
    const double e = fwd ? eps : -eps;
    const uint32_t n = 1u << j;
    double logw_s = -INFINITY, slp = lp0, sh = h0;
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) ss[it] = 0.0;
    bool stop = false;
    for (uint32_t i = 0; i < n; ++i) {
      // one leapfrog step of A (hmc_trajectory's)
#pragma unroll
      for (int it = 0; it < MAXIT; ++it) {
        const int jj = lane + 64 * it;
        if (jj < d) {
          ap[it] = ap[it] + 0.5 * e * (double)ag[it];                       // half kick
          const double m = MASS ? mi[MASS ? it : 0] : 1.0;
          ax[it] = (float)((double)ax[it] + e * (m * ap[it]));              // drift
          xs[jj] = ax[it];
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");       // the stencil reads its neighbours' elements from this wave's row
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      const double lp = __shfl(row_value_grad<MAXIT, BCRT>(T, beta, xs, d, lane, ag, gsm), 0, 64);
      __builtin_amdgcn_wave_barrier();                             // (the next drift overwrites the row)
      kin = 0.0;
#pragma unroll
      for (int it = 0; it < MAXIT; ++it) {
        const int jj = lane + 64 * it;
        if (jj < d) {
          ap[it] = ap[it] + 0.5 * e * (double)ag[it];                       // half kick
          const double m = MASS ? mi[MASS ? it : 0] : 1.0;
          kin += m * ap[it] * ap[it];
          ss[it] = ss[it] + ap[it];
        }
      }
      ++n_leap;
      const double h = -lp + 0.5 * wave_sum(kin);
      double delta = h0 - h;
      const bool nan = isnan(delta);
      if (nan) delta = -INFINITY;
      const bool div = nuts_uniform(nan || -delta > div_thr);
      acc_sum += fmin(dr(delta), 1.0);
      const double logw_n = nuts_logaddexp(logw_s, delta, dr);
      bool take = i == 0;
      if (!take) take = nuts_uniform(dr.uniform(split_at(k_leaf, n, i)) < dr(delta - logw_n));
      if (take) {
#pragma unroll
        for (int it = 0; it < MAXIT; ++it) { sx[it] = ax[it]; sg[it] = ag[it]; }
        slp = lp; sh = h;
      }
      logw_s = logw_n;
      bool turn = false;
      if (!(i & 1u)) {
        if (i + 1 < n) {                                 // (the lone leaf of doubling 0 is never checked against)
          double* const c = ck + (size_t)__popc(i >> 1) * 2 * d;
#pragma unroll
          for (int it = 0; it < MAXIT; ++it) {
            const int jj = lane + 64 * it;
            if (jj < d) { c[jj] = ap[it]; c[d + jj] = ss[it]; }
          }
        }
      } else {
        const int idx_max = __popc(i >> 1), ones = __ffs((int)~i) - 1;      // (trailing one bits of i)
        for (int slot = idx_max; slot > idx_max - ones; --slot) {
          const double* const c = ck + (size_t)slot * 2 * d;
          double dot_c = 0.0, dot_p = 0.0;
#pragma unroll
          for (int it = 0; it < MAXIT; ++it) {
            const int jj = lane + 64 * it;
            if (jj < d) {
              const double cp = c[jj], s = ss[it] - c[d + jj] + cp;
              const double m = MASS ? mi[MASS ? it : 0] : 1.0;
              dot_c += (m * cp) * s;
              dot_p += (m * ap[it]) * s;
            }
          }
          dot_c = wave_sum(dot_c); dot_p = wave_sum(dot_p);
          turn = turn || dot_c <= 0.0 || dot_p <= 0.0;
        }
        turn = nuts_uniform(turn);
      }
      if (div || turn) { divergent = divergent || div; turning = turning || turn; stop = true; break; }
    }
    if (stop) break;
    // the complete subtree joins the tree
    if (nuts_uniform(dr.uniform(k_merge) < fmin(dr(logw_s - logw), 1.0))) {
#pragma unroll
      for (int it = 0; it < MAXIT; ++it) { px[it] = sx[it]; pg[it] = sg[it]; }
      plp = slp; ph = sh;
    }
    logw = nuts_logaddexp(logw, logw_s, dr);
    depth = j + 1;
    double dot_a = 0.0, dot_b = 0.0;
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int jj = lane + 64 * it;
      if (jj < d) {
        ps[it] = ps[it] + ss[it];
        const double m = MASS ? mi[MASS ? it : 0] : 1.0;
        dot_a += (m * ap[it]) * ps[it];
        dot_b += (m * bp[it]) * ps[it];
      }
    }
    dot_a = wave_sum(dot_a); dot_b = wave_sum(dot_b);
    if (nuts_uniform(dot_a <= 0.0 || dot_b <= 0.0)) { turning = true; break; }
  }
  const NutsOut o{depth, n_leap, turning ? 1 : 0, divergent ? 1 : 0, acc_sum / (double)(n_leap > 0 ? n_leap : 1), ph};
  st.template finish<MAXIT>(o, plp, px, pg, d, lane);
}

// the wave's place in a workgroup of a.waves chains: rows and gradient scratch as mala_smem lays them out (for MALA_WAVES rows), the
// checkpoints behind them
__device__ __forceinline__ double* nuts_checkpoints(float* smem, int d, int max_depth) {
  double* const base = (double*)(smem + MALA_WAVES * (d + 2) + MALA_WAVES * MALA_MAXD_SMALL);
  return base + (size_t)(threadIdx.x >> 6) * (size_t)(max_depth - 1) * 2 * d;
}

template <int MAXIT, bool BCRT = false, bool MASS = false>
__global__ __launch_bounds__(MALA_WAVES * 64) void nuts_step_kernel(NutsArgs n) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const HmcArgs& a = n.h;
  const int d = a.T.dim, lane = threadIdx.x & 63, b = blockIdx.x * n.waves + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const ResidentChain c(smem, d, a.B, lane, b);
  c.pads();
  const Key2 kb = mcmc_chain_key(a.key, a.keys, a.n_total, a.chain_offset, b);
  NutsInHbm st{n, c.row, b};
  nuts_trajectory<MAXIT, BCRT, MASS>(a.T, a.beta, a.eps, n.max_depth, n.div_thr, kb, d, lane, c.xs, c.gsm, nuts_checkpoints(smem, d, n.max_depth),
                                     a.minv, st, NutsInline());
}

// n_steps transitions in ONE launch, the chain resident in registers (resident.hip.h): what hmc_run_kernel is to hmc_step_kernel.
// Keys as there; n_steps launches of the step kernel on the step keys give the same bits.
template <int MAXIT, bool BCRT = false, bool MASS = false>
__global__ __launch_bounds__(MALA_WAVES * 64) void nuts_run_kernel(NutsRunArgs r) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const NutsArgs& n = r.n;
  const HmcArgs& a = n.h;
  const int d = a.T.dim, lane = threadIdx.x & 63, b = blockIdx.x * n.waves + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const ResidentChain c(smem, d, a.B, lane, b);
  float* const xs = c.xs; float* const gsm = c.gsm; const size_t row = c.row;
  double* const ck = nuts_checkpoints(smem, d, n.max_depth);

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
  long long tot_leap = 0;
  int tot_div = 0, tot_depth = 0;
  double tot_acc = 0.0;
  int l_depth = 0, l_leap = 0, l_turn = 0, l_div = 0;      // the last step's info (scalars: a struct carried over the loop went to scratch)
  double l_rate = 0.0, l_energy = 0.0;

  for (int s = 0; s < r.t.n_steps; ++s) {
    const Key2 kb = run_step_key(c, a, r.t, kc, s);
    NutsResident<MAXIT> st{x, g, lp, NutsOut{0, 0, 0, 0, 0.0, 0.0}};
    nuts_trajectory<MAXIT, BCRT, MASS>(a.T, a.beta, a.eps, n.max_depth, n.div_thr, kb, d, lane, xs, gsm, ck, a.minv, st, NutsCalled());
    l_depth = st.out.depth; l_leap = st.out.n_leap; l_turn = st.out.turning; l_div = st.out.divergent; l_rate = st.out.acc_rate; l_energy = st.out.energy;
    tot_leap += l_leap; tot_div += l_div; tot_depth += l_depth; tot_acc += l_rate;
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
    if (r.tot_leap) r.tot_leap[b] = tot_leap;
    if (r.tot_acc) r.tot_acc[b] = tot_acc;
    if (r.tot_div) r.tot_div[b] = tot_div;
    if (r.tot_depth) r.tot_depth[b] = tot_depth;
    if (n.depth) n.depth[b] = l_depth;
    if (n.n_leap) n.n_leap[b] = l_leap;
    if (n.turning) n.turning[b] = (uint8_t)l_turn;
    if (n.divergent) n.divergent[b] = (uint8_t)l_div;
    if (n.acc_rate) n.acc_rate[b] = l_rate;
    if (n.energy) n.energy[b] = l_energy;
  }
}

// ---- launch: the LDS budget -------------------------------------------------------------------------------------------------
#define NUTS_MAX_DIM 256
#define NUTS_MAX_DEPTH 16
#define NUTS_MAX_WAVES MALA_WAVES          // (the rows of mala_smem; the kernels' launch bound)
#define NUTS_LDS_CU 163840                 // a CU's LDS, which one workgroup may take whole
static inline size_t nuts_ckpt_bytes(int d, int max_depth) { return (size_t)(max_depth - 1) * 2 * (size_t)d * sizeof(double); }
static inline size_t nuts_smem(int d, int max_depth, int waves) { return mala_smem(d) + (size_t)waves * nuts_ckpt_bytes(d, max_depth); }
// chains per workgroup: the count in 1 .. NUTS_MAX_WAVES that puts the most chains on a CU (the larger count on a tie); 0: not even one fits
static inline int nuts_waves(int d, int max_depth) {
  int best = 0; size_t best_chains = 0;
  for (int w = 1; w <= NUTS_MAX_WAVES; ++w) {
    const size_t sm = nuts_smem(d, max_depth, w);
    if (sm > NUTS_LDS_CU) break;
    const size_t chains = (NUTS_LDS_CU / sm) * (size_t)w;
    if (chains >= best_chains) { best = w; best_chains = chains; }
  }
  return best;
}
// the largest max_tree_depth at which one chain fits
static inline int nuts_depth_that_fits(int d) { return 1 + (int)((NUTS_LDS_CU - mala_smem(d)) / (2 * (size_t)d * sizeof(double))); }

// TAIL: what follows MASS in the kernel's template arguments -- `none` for the step and run kernels, `sums` / `nosums` for the SUMS flag
// of nuts_warmup_kernel (nuts_warmup.hip.h)
#define NUTS_TAIL_none
#define NUTS_TAIL_sums , true
#define NUTS_TAIL_nosums , false
#define NUTS_LAUNCH_(KERN, MAXIT, TAIL, ...)                                                                            \
  do {                                                                                                                  \
    auto go = [&](auto kern) {                                                                                          \
      (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm);                \
      hipLaunchKernelGGL(kern, grid, block, sm, stream, __VA_ARGS__);                                                   \
    };                                                                                                                  \
    if (mass) { if (bcrt) go(KERN<MAXIT, true, true NUTS_TAIL_##TAIL>); else go(KERN<MAXIT, false, true NUTS_TAIL_##TAIL>); }      \
    else { if (bcrt) go(KERN<MAXIT, true, false NUTS_TAIL_##TAIL>); else go(KERN<MAXIT, false, false NUTS_TAIL_##TAIL>); }         \
  } while (0)
// the instance KERN<MAXIT, BCRT, MASS, TAIL> for the dimension, the phi-four boundary and the installed mass (n: the call's NutsArgs)
#define NUTS_DISPATCH(KERN, TAIL, ...)                                                           \
  do {                                                                                           \
    const int nit = (n.h.T.dim + 63) / 64;                                                       \
    const dim3 grid((n.h.B + n.waves - 1) / n.waves), block(n.waves * 64);                       \
    const size_t sm = nuts_smem(n.h.T.dim, n.max_depth, n.waves);                                \
    const bool bcrt = n.h.T.kind == MFM_TARGET_PHI4 && !phi4_default_bc(n.h.T);                  \
    const bool mass = n.h.minv != nullptr;                                                       \
    if (nit <= 1) NUTS_LAUNCH_(KERN, 1, TAIL, __VA_ARGS__);                                      \
    else if (nit <= 2) NUTS_LAUNCH_(KERN, 2, TAIL, __VA_ARGS__);                                 \
    else if (nit <= 4) NUTS_LAUNCH_(KERN, 4, TAIL, __VA_ARGS__);                                 \
    else return -2;                                                                              \
  } while (0)

int launch_nuts_step(const NutsArgs& n, hipStream_t stream) { NUTS_DISPATCH(nuts_step_kernel, none, n); return 0; }
int launch_nuts_run(const NutsRunArgs& r, hipStream_t stream) { const NutsArgs& n = r.n; NUTS_DISPATCH(nuts_run_kernel, none, r); return 0; }
