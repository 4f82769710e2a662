// Step-size warmup of the No-U-turn sampler: n_steps NUTS transitions of every chain in ONE launch, in which every chain adapts its
// OWN step size by dual averaging on its TREE's acceptance statistic, the mean over the leaves of min(1, exp(H0 - H)) that
// nuts_trajectory reports in float64 (NutsOut.acc_rate) -- the statistic Stan, blackjax and NumPyro steer NUTS by
// (mfm_nuts_warmup / mfm_nuts_warmup_window; the recursion: include/mfm.h, DualAvg in mcmc.hip.h).
//
// nuts_warmup_kernel is to nuts_run_kernel what hmc_warmup_kernel is to hmc_run_kernel: the same mapping (one wave per chain,
// nuts_waves chains per workgroup, the checkpoints in the wave's LDS), key schedule, residency and closing stores, without the
// trajectory and the last step's info, and with this wave's step size in place of the launch's: transition m of chain b gives the bits
// of mfm_nuts_step_keys with the scalar step size eps_m[b] and the same step key (tests/test_gpu_nuts_warmup.py).  Chains at different
// step sizes build trees of different depths; with one wave per chain and no workgroup barrier that is the wave-uniform control flow the
// run kernel already has.  The adaptation's state is wave-uniform and rides in scalar registers, as in warmup.hip.
//
// SUMS (mfm_nuts_warmup_window): the state after every transition, the float32 position as a double (its square is exact), is added in
// step order to two float64 sums per element.  The sums are kept in their own elements of the output, which only this lane touches, at
// every MAXIT: nuts_trajectory already holds 16 to 18 VGPRs per element, MAXIT 4 has no room for four more, and carried in registers the
// MAXIT 1 and 2 instances took 80 bytes of scratch per lane (DESIGN.md section 4.15 has the compiler's figures for both forms).  A
// transition is a whole tree, beside which the two read-modify-writes per element do not count.
// (Included by api.hip after nuts.hip and warmup.hip: NutsRunArgs, NutsResident, NutsCalled, nuts_checkpoints, NUTS_DISPATCH; WarmupArgs,
// DualAvg, warmup_begin / warmup_next / warmup_finish, wave_first.)
#pragma once

// r.t: key_mode and n_steps, acc_sum the sum of the transitions' acceptance statistics (no n_acc: a NUTS transition has no accept /
// reject); r.tot_leap / tot_div / tot_depth as nuts_run_kernel's; r.n's info pointers and r.tot_acc unused
template <int MAXIT, bool BCRT = false, bool MASS = false, bool SUMS = false>
__global__ __launch_bounds__(MALA_WAVES * 64) void nuts_warmup_kernel(NutsRunArgs r, WarmupArgs w) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const NutsArgs& n = r.n;
  const HmcArgs& a = n.h;
  const int d = a.T.dim, lane = threadIdx.x & 63, b = blockIdx.x * n.waves + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const ResidentChain c(smem, d, a.B, lane, b);
  float* const xs = c.xs; float* const gsm = c.gsm; const size_t row = c.row, B = c.B;
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
  double acc_sum = 0.0;
  DualAvg da = warmup_begin(a.eps);
  double eps = a.eps;                                     // the first transition runs at the caller's value itself
  if constexpr (SUMS) {
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int j = lane + 64 * it;
      if (j < d) { w.pos_sum[row + j] = 0.0; w.pos_sumsq[row + j] = 0.0; }
    }
  }

  for (int s = 0; s < r.t.n_steps; ++s) {
    const Key2 kb = run_step_key(c, a, r.t, kc, s);
    if (w.step_traj && lane == 0) w.step_traj[(size_t)s * B + (size_t)b] = eps;
    NutsResident<MAXIT> st{x, g, lp, NutsOut{0, 0, 0, 0, 0.0, 0.0}};
    nuts_trajectory<MAXIT, BCRT, MASS>(a.T, a.beta, eps, n.max_depth, n.div_thr, kb, d, lane, xs, gsm, ck, a.minv, st, NutsCalled());
    tot_leap += st.out.n_leap; tot_div += st.out.divergent; tot_depth += st.out.depth;
    acc_sum = wave_first(acc_sum + wave_first(st.out.acc_rate));
    eps = warmup_next(da, s + 1, st.out.acc_rate, w.target);
    if constexpr (SUMS) {
#pragma clang fp contract(off)
#pragma unroll
      for (int it = 0; it < MAXIT; ++it) {
        const int j = lane + 64 * it;
        const double v = (double)x[it];
        if (j < d) { w.pos_sum[row + j] = w.pos_sum[row + j] + v; w.pos_sumsq[row + j] = w.pos_sumsq[row + j] + v * v; }
      }
    }
    resident_step_end();
  }

#pragma unroll
  for (int it = 0; it < MAXIT; ++it) {
    const int j = lane + 64 * it;
    if (j < d) { a.pos[row + j] = x[it]; a.grad[row + j] = g[it]; }
  }
  warmup_finish(c, r.t, w, da, eps, 0, acc_sum, a.logp, lp);
  if (lane == 0) {
    if (r.tot_leap) r.tot_leap[b] = tot_leap;
    if (r.tot_div) r.tot_div[b] = tot_div;
    if (r.tot_depth) r.tot_depth[b] = tot_depth;
  }
}

// (w.pos_sum set: the SUMS instances; the call has checked that w.pos_sumsq then is too)
int launch_nuts_warmup(const NutsRunArgs& r, const WarmupArgs& w, hipStream_t stream) {
  const NutsArgs& n = r.n;
  if (w.pos_sum) NUTS_DISPATCH(nuts_warmup_kernel, sums, r, w); else NUTS_DISPATCH(nuts_warmup_kernel, nosums, r, w);
  return 0;
}
