// Hamiltonian Monte Carlo for the log-Gaussian Cox process on the 16-chain GEMM tile: mfm_cox_hmc_step / _step_keys / _run / _warmup.
// The row kernels of hmc.hip refuse this target because its gradient needs the dense contraction K^-1 (x - mu); here a leapfrog step is
// ONE tile GEMM against the packed K^-1 (lgcp.hip's) plus elementwise work.  The arithmetic of a step of chain b with chain key kb is
// hmc_trajectory's (hmc.hip), so that oracle/hmc.py's kernel on the tempered Cox density restates it in float64:
//   k_mom = mcmc_step_key(kb, MCMC_K_INT), k_acc = mcmc_step_key(kb, MCMC_K_RMH); momentum p_j = normal64(k_mom, j, d), kept in float64
//   H0 = -logp + 1/2 sum p^2, logp the state's float64 tempered log-density (what mfm_mala_init leaves: the state is the MALA state)
//   num_steps times: p += 0.5 eps (double) g; x = (float)((double) x + eps p); y = K^-1 (x - mu) by the tile GEMM;
//                    g = cox_grad(beta, expf(x), y); p += 0.5 eps (double) g
//   the LAST leapfrog step's epilogue also forms cox_terms; logp_end = cox_logp(beta, sum lik, sum quad); H1 = -logp_end + 1/2 sum p^2
//   pa = mala_accept_p(H0 - H1), accepted when uniform01(k_acc) < pa.
//
// Mapping: mala_lgcp_kernel's (lgcp.hip).  One workgroup of LGCP_NW waves per 16 chains, column tiles (wave + LGCP_NW q) 16 + c, rows
// 4 g + i (the accumulator's layout); the position tile [16][dp + 4] in LDS is the GEMM's A operand.  x (float32), p (float64) and g
// (float32) of the tile stay in registers over the trajectory; the run and the warmup make all their steps in ONE launch.  The state
// is NOT held in registers between the steps: pos and grad in HBM are untouched until a row accepts, an accepted row stores its end
// point there, and every step reads its start from there after its momentum is drawn (the same thread wrote it; L2 serves 128 d bytes
// per tile and step next to the 4 dp^2 bytes of K^-1 that every leapfrog step streams).  A row's SCALARS -- log-density, energies, step size, dual-averaging state, tallies -- are held
// once per row by lane c of every group of 16 lanes, as in eslice_kernel (eslice.hip): every wave forms every row's decision from the
// same LDS doubles summed in the same order, so the workgroup stays uniform and a row's bits do not depend on its tile mates.
// Barriers: one before and one after each GEMM (the drift overwrites the tile the GEMM reads), one per row reduction.  A tile never
// waits for another: no atomics, no flags.
// Instances: TPW 1, 2, 4, 8 (d <= 1024).  TPW 13 (the 40 x 40 grid) is not served: x + p + g alone are 208 registers.
// (Included by api.hip after lgcp.hip, mala_run.hip, warmup.hip and eslice.hip: LGCP_NW, run_normal64 / run_uniform01 / run_exp /
// run_log, RunTail, WarmupArgs, DualAvg, eslice_row_key.)
#include "mlp.hip.h"
#include "mcmc.hip.h"

struct CoxHmcArgs {
  TargetDev T; int dp;
  int run;                 // 0: one step on the chain keys of mfm_mala_step (t.n_steps == 1); 1: t.n_steps steps on mcmc_run_key
  Key2 key; const uint32_t* keys; uint32_t n_total, chain_offset;
  int B, num_steps;
  double beta, eps;
  float* pos; double* logp; float* grad;      // state, updated in place
  float* acc_prob; uint8_t* accepted;         // the LAST step's info (each may be null)
  RunTail t;
  WarmupArgs w;            // the WARM instances only (pos_sum / pos_sumsq unused)
};

// the two step keys of a row, by a CALL for the reason eslice.hip states (the rows' Threefry chains stay out of the step loop's registers)
struct CoxHmcKeys { Key2 k_mom, k_acc; };
__device__ __attribute__((noinline)) CoxHmcKeys cox_hmc_keys(Key2 kb) {
  return CoxHmcKeys{mcmc_step_key(kb, MCMC_K_INT), mcmc_step_key(kb, MCMC_K_RMH)};
}

// Row sums of N quantities over the tile's columns: 16-lane shuffles, one double per quantity, wave and row in `r` ([N][LGCP_NW][16]),
// ONE barrier, then row c's totals from the same LDS doubles in every wave, summed in the same order (eslice_row_sum's scheme).
template <int N>
__device__ __forceinline__ void cox_hmc_row_sums(double (&v)[N][4], double* r, int wave, int g, int c, double (&out)[N]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int n = 0; n < N; ++n)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) v[n][i] += __shfl_xor(v[n][i], o, 64);
      if (c == 0) r[(n * LGCP_NW + wave) * 16 + 4 * g + i] = v[n][i];
    }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < N; ++n) {
    double sum = 0.0;
#pragma unroll
    for (int w = 0; w < LGCP_NW; ++w) sum += r[(n * LGCP_NW + w) * 16 + c];
    out[n] = sum;
  }
}

// WARM: every row adapts its own step size by dual averaging (mfm_cox_hmc_warmup); otherwise the launch's step size serves every row.
template <int TPW, bool WARM>
__global__ __launch_bounds__(LGCP_NW * 64) void cox_hmc_kernel(CoxHmcArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, c = lane & 15;
  const int d = a.T.dim, dp = a.dp, ld = dp + 4, b0 = blockIdx.x * 16;
  float* bU = lds;                                                // [16][ld] the trajectory's positions
  double* red = reinterpret_cast<double*>(lds + 16 * ld);         // [3][LGCP_NW][16] the end point's sums | [LGCP_NW][16] the start's kinetic energy | dal
  double* red0 = red + 3 * LGCP_NW * 16;
  double* dal = red + 4 * LGCP_NW * 16;                           // [6][16] WARM: the rows' dual-averaging state (mu, x0, x, hbar, xbar) and step size

  float x[TPW][4], gr[TPW][4];
  double p[TPW][4];
  // the row's scalars: lane c of every group of 16 owns row c (the same values in all four groups and all waves)
  double lp = a.logp[b0 + c];
  const bool writer = wave == 0 && lane < 16;      // lane r of the first wave writes row r's scalars
  auto rows16 = [&](bool flag) __attribute__((always_inline)) { return (uint32_t)__ballot(flag) & 0xffffu; };      // bit r: row r (lanes 0 .. 15)
  int n_acc = 0;
  double acc_sum = 0.0, pa = 0.0;
  bool acc = false;
  // WARM: a row's dual-averaging state and step size live in LDS, kept by the writer lane alone (in the registers of every lane they
  // cost the TPW 8 instance 64 B of scratch); the other lanes read the step size behind the barrier of the step's first reduction
  if constexpr (WARM) {
    if (writer) {
      const double x0 = run_log(a.eps);
      dal[0 * 16 + c] = run_log(10.0 * a.eps); dal[1 * 16 + c] = x0; dal[2 * 16 + c] = x0; dal[3 * 16 + c] = 0.0; dal[4 * 16 + c] = 0.0;
      dal[5 * 16 + c] = a.eps;                     // (the first step runs at the caller's value itself)
    }
  }

  for (int s = 0; s < a.t.n_steps; ++s) {
    // ---- the row's keys and the momentum ----
    const CoxHmcKeys ks = cox_hmc_keys(eslice_row_key(a.run, a.t.key_mode, a.key, a.keys, (uint32_t)a.t.n_steps, (uint32_t)s, a.n_total, a.chain_offset, b0 + c));
    if constexpr (WARM) {
      double* st_out = a.w.step_traj;
      asm volatile("" : "+s"(st_out));
      if (st_out && writer) st_out[(size_t)s * (size_t)a.B + (size_t)(b0 + c)] = dal[5 * 16 + c];
    }
    double kin[1][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      kin[0][i] = 0.0;
      const Key2 km{(uint32_t)__shfl((int)ks.k_mom.k0, 4 * g + i, 64), (uint32_t)__shfl((int)ks.k_mom.k1, 4 * g + i, 64)};
#pragma unroll
      for (int q = 0; q < TPW; ++q) {
        const int col = (wave + LGCP_NW * q) * 16 + c;
        p[q][i] = col < d ? run_normal64(km, (uint32_t)col, (uint32_t)d) : 0.0;
        kin[0][i] = kin[0][i] + p[q][i] * p[q][i];
      }
    }
    double k0[1];
    cox_hmc_row_sums<1>(kin, red0, wave, g, c, k0);
    const double h0 = -lp + 0.5 * k0[0];
    // the step size of the rows 4 g + i (WARM: read again from LDS at every use: four more doubles held over the GEMM spill)
    auto row_eps = [&](double (&e)[4]) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < 4; ++i) e[i] = WARM ? dal[5 * 16 + 4 * g + i] : a.eps;
    };
    // the state, from HBM at every step: it is current there (an accepted row stores its end point below), and read here, AFTER the
    // calls above, x and g are not live across them -- held over the steps they are, and the TPW 8 instance spills
    // (the addresses are formed anew at every use from opaque copies of the pointers, as eslice_kernel's: hoisted out of the step loop
    //  they are held in registers over the whole kernel and the TPW 8 instance spills them)
    {
      const float* pos_in = a.pos; const float* grad_in = a.grad;
      int r0 = b0 + 4 * g;
      asm volatile("" : "+s"(pos_in), "+s"(grad_in), "+v"(r0));
#pragma unroll
      for (int q = 0; q < TPW; ++q) {
        const int col = (wave + LGCP_NW * q) * 16 + c;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const size_t o = (size_t)(r0 + i) * d + col;
          x[q][i] = col < d ? pos_in[o] : 0.f;
          gr[q][i] = col < d ? grad_in[o] : 0.f;
        }
      }
    }

    // ---- the trajectory: one tile GEMM per leapfrog step ----
    double end[3][4];                              // the end point's likelihood, quadratic-form and kinetic sums
#pragma unroll
    for (int i = 0; i < 4; ++i) { end[0][i] = 0.0; end[1][i] = 0.0; end[2][i] = 0.0; }
#pragma unroll 1
    for (int ls = 0; ls < a.num_steps; ++ls) {
      double e[4];
      row_eps(e);
#pragma unroll
      for (int q = 0; q < TPW; ++q) {
        const int col = (wave + LGCP_NW * q) * 16 + c;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (col < d) {
            p[q][i] = p[q][i] + 0.5 * e[i] * (double)gr[q][i];              // half kick
            x[q][i] = (float)((double)x[q][i] + e[i] * p[q][i]);            // drift
          }
          if (col < dp) bU[(4 * g + i) * ld + col] = x[q][i];
        }
      }
      __syncthreads();
      const bool last = ls == a.num_steps - 1;     // interior steps need the gradient alone: their epilogue carries no reduction
      layer_gemm<1, LGCP_NW, 2>(bU, ld, a.T.KinvP, a.T.kbias, dp / 16, dp / 16, wave, lane,
                                [&](int q, int nt, int m, f32x4 av, float kb) {
                                  const int col = nt * 16 + c;
#pragma unroll
                                  for (int i = 0; i < 4; ++i) {
                                    float xv = 0.f, gv = 0.f;
#pragma unroll
                                    for (int qq = 0; qq < TPW; ++qq)
                                      if (qq == q) xv = x[qq][i];
                                    if (col < d) {
                                      const float y = av[i] + kb;
                                      const float ex = expf(xv);
                                      gv = cox_grad(a.T, a.beta, col, ex, y);
                                      if (last) cox_terms(a.T, col, xv, ex, y, end[0][i], end[1][i]);
                                    }
#pragma unroll
                                    for (int qq = 0; qq < TPW; ++qq)
                                      if (qq == q) gr[qq][i] = gv;
                                  }
                                });
      __syncthreads();                             // (the next drift overwrites the tile)
      row_eps(e);
#pragma unroll
      for (int q = 0; q < TPW; ++q) {
        const int col = (wave + LGCP_NW * q) * 16 + c;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (col < d) p[q][i] = p[q][i] + 0.5 * e[i] * (double)gr[q][i];   // half kick
      }
    }

    // ---- the decision, by the row's owner lanes ----
#pragma unroll
    for (int q = 0; q < TPW; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) end[2][i] = end[2][i] + p[q][i] * p[q][i];
    double es[3];
    cox_hmc_row_sums<3>(end, red, wave, g, c, es);
    const double lpe = cox_logp(a.T, a.beta, es[0], es[1]);
    const double h1 = -lpe + 0.5 * es[2];
    pa = mala_accept_p(h0 - h1, RunExp());
    acc = run_uniform01(ks.k_acc) < pa;
    lp = acc ? lpe : lp;
    n_acc += acc ? 1 : 0;
    acc_sum += pa;
    if constexpr (WARM) {
      if (writer) {                                // (every wave is past its read of the step size: the trajectory's barriers)
        DualAvg da{dal[0 * 16 + c], dal[1 * 16 + c], dal[2 * 16 + c], dal[3 * 16 + c], dal[4 * 16 + c]};
        dual_avg_update(da, s + 1, pa, a.w.target);
        dal[2 * 16 + c] = da.x; dal[3 * 16 + c] = da.hbar; dal[4 * 16 + c] = da.xbar;
        dal[5 * 16 + c] = run_exp(da.x);
      }
    }
    // an accepted row's end point replaces the state in HBM (a rejected row's state is untouched there); the thinned trajectory,
    // mfm_hmc_run's layout, takes the state after the decision
    const uint32_t am = rows16(acc);
    const bool snap_due = a.t.thin > 0 && (s + 1) % a.t.thin == 0;
    const size_t snap = snap_due ? (size_t)((s + 1) / a.t.thin - 1) : 0;
    float* pos_out = a.pos; float* grad_out = a.grad; float* traj_out = a.t.traj_pos;
    int g4 = 4 * g;                                // (the rows' indices and masks too)
    asm volatile("" : "+s"(pos_out), "+s"(grad_out), "+s"(traj_out), "+v"(g4));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ai = (am >> (g4 + i)) & 1u;
#pragma unroll
      for (int q = 0; q < TPW; ++q) {
        const int col = (wave + LGCP_NW * q) * 16 + c;
        if (col < d) {
          const size_t o = (size_t)(b0 + g4 + i) * d + col;
          if (ai) { pos_out[o] = x[q][i]; grad_out[o] = gr[q][i]; }
          if (snap_due && traj_out) traj_out[(snap * (size_t)a.B + (size_t)(b0 + g4 + i)) * (size_t)d + col] = ai ? x[q][i] : pos_out[o];
        }
      }
    }
    double* tlp_out = a.t.traj_logp;
    asm volatile("" : "+s"(tlp_out));
    if (snap_due && tlp_out && writer) tlp_out[snap * (size_t)a.B + (size_t)(b0 + c)] = lp;
  }

  // (pos and grad are current in HBM: every accepted step stored them)
  double* logp_out = a.logp;
  asm volatile("" : "+s"(logp_out));
  if (writer) {
    const int b = b0 + c;
    logp_out[b] = lp;
    if (a.t.n_acc) a.t.n_acc[b] = n_acc;
    if (a.t.acc_sum) a.t.acc_sum[b] = acc_sum;
    if (a.acc_prob) a.acc_prob[b] = (float)pa;
    if (a.accepted) a.accepted[b] = acc ? 1 : 0;
    if constexpr (WARM) {
      a.w.step_avg[b] = run_exp(dal[4 * 16 + c]);
      if (a.w.step_last) a.w.step_last[b] = dal[5 * 16 + c];
    }
  }
}

// column tiles per wave and dynamic LDS of the instance that serves a padded dimension dp (0 tiles: none does)
static inline void cox_hmc_plan(int dp, int* tpw, size_t* lds_bytes) {
  const int need = (dp / 16 + LGCP_NW - 1) / LGCP_NW;
  *tpw = need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : need <= 8 ? 8 : 0;
  *lds_bytes = (size_t)(16 * (dp + 4)) * 4 + (size_t)(4 * LGCP_NW * 16 + 6 * 16) * 8;
}

int launch_cox_hmc(const CoxHmcArgs& a, bool warm, hipStream_t stream) {
  int tpw; size_t sm;
  cox_hmc_plan(a.dp, &tpw, &sm);
  if (!tpw || sm > 160 * 1024 || a.B % 16) return -3;
  dim3 grid(a.B / 16), block(LGCP_NW * 64);
#define CH_LAUNCH1(T, W) do { (void)hipFuncSetAttribute((const void*)cox_hmc_kernel<T, W>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm); \
                              hipLaunchKernelGGL((cox_hmc_kernel<T, W>), grid, block, sm, stream, a); } while (0)
#define CH_LAUNCH(T) do { if (warm) CH_LAUNCH1(T, true); else CH_LAUNCH1(T, false); } while (0)
  switch (tpw) { case 1: CH_LAUNCH(1); break; case 2: CH_LAUNCH(2); break; case 4: CH_LAUNCH(4); break; default: CH_LAUNCH(8); }
#undef CH_LAUNCH
#undef CH_LAUNCH1
  return 0;
}
