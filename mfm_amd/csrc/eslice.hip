// Elliptical slice sampling (Murray, Adams & MacKay 2010) for the log-Gaussian Cox process: mfm_eslice_init / _step / _step_keys / _run.
// The reference vendors the sampler as bblackjax/mcmc/tess.py; with the linear transport T(u) = mu + L u (L the Cholesky factor of the
// prior covariance) its log-det is constant and |u|^2 + |m|^2 is constant on the ellipse, so its slice test
// logprob(T(u)) + ldj - 1/2 |m|^2 (tess.py:42-44) is a comparison of log-likelihoods alone.  One transition of chain b at inverse
// temperature beta, state x and ll(x) = sum_i (x_i c_i - a exp(x_i)) (untempered, float64):
//   (k_nu, k_u, k_theta, k_shrink) = split(k_b, 4), k_b the chain's key as mfm_mala_step derives it (mcmc_chain_key)
//   nu = L n, n = normal(k_nu, (d,))                                                 (tess.py:95, pushed through L)
//   log y = beta ll(x) + log(uniform(k_u))                                            (tess.py:98)
//   theta = 2 pi uniform(k_theta), lo = theta - 2 pi, hi = theta                     (tess.py:100-102)
//   evaluation subiter = 1, 2, ...: x' = mu + (x - mu) cos(theta) + nu sin(theta)     (tess.py:78-83); accepted when beta ll(x') is
//   finite and > log y (tess.py:121); else theta < 0 ? lo = theta : hi = theta, and
//   theta = lo + (hi - lo) uniform(k_shrink, (MFM_ESLICE_MAX_SUBITER,))[subiter - 1]  (counter-based: no chain of splits)
// After MFM_ESLICE_MAX_SUBITER evaluations the chain keeps x and ll(x), which lie inside the slice by construction, and is counted
// as capped: a non-finite position ends at the cap and does not spin.
//
// Mapping: mala_lgcp_kernel's (lgcp.hip).  One workgroup of LGCP_NW waves per 16 chains, column tiles dealt over the waves, rows
// 4 g + i.  Phase A: the 16 x dp tile of normals goes to LDS.  Phase B: layer_gemm against the packed L^T; the epilogue leaves nu in
// registers in the accumulator's layout.  Phase C: the shrink loop on the registers x[TPW][4], nu[TPW][4]: expf in float32, the row sums
// in float64 through 16-lane shuffles and the `red` LDS array; theta, lo, hi, log y and the comparison in float64, held by ONE lane per
// row and group of 16 lanes.  The loop has a barrier inside, so every wave forms every row's decision from the same LDS doubles, summed
// in the same order, and leaves together.
// (cos and sin of the float64 angle are formed to float32 accuracy from float32 functions: eslice_sincos.)
// A tile never depends on another tile: n_steps transitions run in ONE launch with the rows resident in registers; L^T is streamed
// again once per transition.
// (Included by api.hip after lgcp.hip and mala_run.hip: LGCP_NW, run_normal64, mcmc_run_key.)
#include "mlp.hip.h"
#include "mcmc.hip.h"
#include "../../include/mfm.h"      // MFM_ESLICE_MAX_SUBITER

struct EsliceArgs {
  TargetDev T; int dp;
  const float* cholP;      // L^T packed like an MLP layer (K = N = d): nu = n . L^T
  int mode;                // 0: init (eslice_init_kernel), 1: one transition on the chain keys of mfm_mala_step, 2: n_steps transitions on mcmc_run_key
  int key_mode; Key2 key; const uint32_t* keys; uint32_t n_total, chain_offset;
  int B; double beta;
  int n_steps, thin;
  float* pos; double* loglik;
  int32_t* subiter; double* theta; float* momentum;      // the LAST transition's info (each may be null)
  int32_t* subiter_sum; int32_t* n_capped; int32_t* subiter_max;      // per chain over the run (each may be null)
  float* traj_pos; double* traj_loglik;                  // [n_steps / thin][B][d], [n_steps / thin][B] (each may be null)
};

// the four step keys of a transition
enum { ESLICE_K_NU = 0, ESLICE_K_U = 1, ESLICE_K_THETA = 2, ESLICE_K_SHRINK = 3 };

// A row's key and its float64 scalars (with the float64 logarithm) are made by CALLS, like the float64 normal draw (run_normal64,
// mala_run.hip, which says why): inlined into the loop over the transitions, the double-precision coefficients are hoisted out of it
// and held in registers over the whole kernel, and the rows' Threefry chains are interleaved by the scheduler -- the first build of
// this kernel, with everything in line and a float64 sincos in the shrink loop, used all 256 VGPRs and 1.2 - 1.9 KB of scratch in
// every instance.  All the calls are made BEFORE the tile GEMM, while nu is dead, so that only x lives across them.
struct EsliceRow { double logy, theta; Key2 k_nu, k_sh; };
__device__ __attribute__((noinline)) EsliceRow eslice_row_setup(Key2 kb, double beta, double ll) {
#pragma clang fp contract(off)
  EsliceRow r;
  r.logy = beta * ll + log(uniform01(split_at(kb, 4, ESLICE_K_U), 0, 1));
  r.theta = 6.283185307179586 * uniform01(split_at(kb, 4, ESLICE_K_THETA), 0, 1);
  r.k_nu = split_at(kb, 4, ESLICE_K_NU);
  r.k_sh = split_at(kb, 4, ESLICE_K_SHRINK);
  return r;
}
__device__ __attribute__((noinline)) Key2 eslice_row_key(int run, int key_mode, Key2 key, const uint32_t* keys, uint32_t n_steps, uint32_t s,
                                                         uint32_t n_total, uint32_t chain_offset, int b) {
  if (!run) return mcmc_chain_key(key, keys, n_total, chain_offset, b);
  return mcmc_run_key(key_mode, key, key_mode ? Key2{keys[2 * b], keys[2 * b + 1]} : Key2{0, 0}, n_steps, s, n_total, chain_offset + (uint32_t)b);
}
// cos and sin of a float64 angle to float32 accuracy, from float32 functions (whose coefficients are instruction literals): the angle
// is split into its float32 head and the float32 tail of the remainder, sin(h + t) = sin h + t cos h, cos(h + t) = cos h - t sin h
// (t <= 2^-24 |h|: the next term is below 2^-49).  The result feeds float32 products; what is lost against a float64 sincos is the
// float32 functions' own error of about an ulp, the size of the rounding of x' itself.
__device__ __forceinline__ void eslice_sincos(double theta, float& cs, float& sn) {
#pragma clang fp contract(off)
  const float h = (float)theta, t = (float)(theta - (double)h);
  float sh, ch;
  sincosf(h, &sh, &ch);
  cs = fmaf(-t, sh, ch);
  sn = fmaf(t, ch, sh);
}

// One element's likelihood term x c - a e^x (cox_terms' form: expf in float32, the term in float64), and the sum of a tile's rows over
// its columns: 16-lane shuffles, one double per wave and row in `r` ([LGCP_NW][16]), ONE barrier, then row c's total from the same LDS
// doubles in every wave, summed in the same order.  Shared by the init and the transition kernels: the same bits for the same row.
__device__ __forceinline__ double eslice_term(float xv, float cnt, double pa) {
#pragma clang fp contract(off)
  const float ex = expf(xv);
  return fma((double)xv, (double)cnt, -(pa * (double)ex));
}
__device__ __forceinline__ double eslice_row_sum(double (&lik)[4], double* r, int wave, int g, int c) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) lik[i] += __shfl_xor(lik[i], o, 64);
    if (c == 0) r[wave * 16 + 4 * g + i] = lik[i];
  }
  __syncthreads();
  double sum = 0.0;
#pragma unroll
  for (int w = 0; w < LGCP_NW; ++w) sum += r[w * 16 + c];
  return sum;
}

// mfm_eslice_init: ll of every row (a kernel of its own: as a mode of eslice_kernel its path cost the TPW 13 instance 208 B of scratch)
template <int TPW>
__global__ __launch_bounds__(LGCP_NW * 64) void eslice_init_kernel(EsliceArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, c = lane & 15;
  const int d = a.T.dim, b0 = blockIdx.x * 16;
  double* red = reinterpret_cast<double*>(lds + 16 * (a.dp + 4));
  const double pa = (double)a.T.poisson_a;
  double lik[4] = {0, 0, 0, 0};
#pragma unroll
  for (int q = 0; q < TPW; ++q) {
    const int col = (wave + LGCP_NW * q) * 16 + c;
    if (col < d) {
      const float cnt = a.T.counts[col];
#pragma unroll
      for (int i = 0; i < 4; ++i) lik[i] += eslice_term(a.pos[(size_t)(b0 + 4 * g + i) * d + col], cnt, pa);
    }
  }
  const double ll = eslice_row_sum(lik, red, wave, g, c);
  if (wave == 0 && lane < 16) a.loglik[b0 + c] = ll;
}

template <int TPW>
__global__ __launch_bounds__(LGCP_NW * 64) void eslice_kernel(EsliceArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), g = lane >> 4, c = lane & 15;
  const int d = a.T.dim, dp = a.dp, ld = dp + 4, b0 = blockIdx.x * 16;
  float* bU = lds;                                                // [16][ld] the normals n
  double* red = reinterpret_cast<double*>(lds + 16 * ld);         // [2][LGCP_NW][16] row sums of an evaluation, by its parity
  const float mu = a.T.mu;
  const double pa = (double)a.T.poisson_a;

  // The tile's elements: columns (wave + LGCP_NW q) 16 + c of the rows 4 g + i, the accumulator's layout.  The SCALARS of a row -- its
  // log-likelihood, slice level, angle and bracket, counters -- are held once per row instead: lane c of every group of 16 owns row c
  // (the same values in all four groups and all waves); a group's view of its rows 4 g + i comes by shuffle and ballot.
  float x[TPW][4], nu[TPW][4], cnt[TPW];
#pragma unroll
  for (int q = 0; q < TPW; ++q) {
    const int col = (wave + LGCP_NW * q) * 16 + c;
    cnt[q] = col < d ? a.T.counts[col] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      x[q][i] = col < d ? a.pos[(size_t)(b0 + 4 * g + i) * d + col] : 0.f;
  }
  double ll = a.loglik[b0 + c];

  // ll of row c at the ellipse point (cs, sn) of every row.  Rows whose bit is set in `skip` are not evaluated (their sum is not used).
  // `ev`: the evaluation's count from 0; its parity picks the half of `red`, so that ONE barrier serves an evaluation.
  int ev = 0;
  auto ellipse = [&](float xv, float nv, float cs, float sn) __attribute__((always_inline)) {
#pragma clang fp contract(off)
    return fmaf(xv - mu, cs, fmaf(nv, sn, mu));
  };
  auto evaluate = [&](const float (&cs)[4], const float (&sn)[4], uint32_t skip) __attribute__((always_inline)) {
    double lik[4] = {0, 0, 0, 0};
#pragma unroll
    for (int q = 0; q < TPW; ++q) {
      const int col = (wave + LGCP_NW * q) * 16 + c;
      if (col < d) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (!((skip >> (4 * g + i)) & 1u)) lik[i] += eslice_term(ellipse(x[q][i], nu[q][i], cs[i], sn[i]), cnt[q], pa);
        }
      }
    }
    const double sum = eslice_row_sum(lik, red + (ev & 1) * LGCP_NW * 16, wave, g, c);
    ++ev;
    return sum;
  };
  auto rows16 = [&](bool flag) __attribute__((always_inline)) { return (uint32_t)__ballot(flag) & 0xffffu; };      // bit r: row r (lanes 0 .. 15)

  const bool writer = wave == 0 && lane < 16;      // lane r of the first wave writes row r's scalars
  const double two_pi = 6.283185307179586;
  double theta = 0.0;
  int sub = 0, sub_sum = 0, sub_max = 0, capped = 0;
  bool done = false;

  for (int s = 0; s < a.n_steps; ++s) {
    // ---- the row's key and float64 scalars, ahead of the GEMM ----
    const Key2 kb = eslice_row_key(a.mode == 2, a.key_mode, a.key, a.keys, (uint32_t)a.n_steps, (uint32_t)s, a.n_total, a.chain_offset, b0 + c);
    const EsliceRow rw = eslice_row_setup(kb, a.beta, ll);
    const double logy = rw.logy;
    const Key2 k_sh = rw.k_sh;
    theta = rw.theta;
    // ---- phase A: the tile of normals (a rolled loop over this wave's column tiles: it touches no register array) ----
    {
      Key2 k_nu[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) k_nu[i] = Key2{(uint32_t)__shfl((int)rw.k_nu.k0, 4 * g + i, 64), (uint32_t)__shfl((int)rw.k_nu.k1, 4 * g + i, 64)};
#pragma unroll 1
      for (int t = wave; t < dp / 16; t += LGCP_NW) {
        const int col = t * 16 + c;
#pragma unroll
        for (int i = 0; i < 4; ++i)
          bU[(4 * g + i) * ld + col] = col < d ? (float)run_normal64(k_nu[i], (uint32_t)col, (uint32_t)d) : 0.f;
      }
    }
    __syncthreads();
    // ---- phase B: nu = n . L^T through the tile GEMM (nu is cleared HERE, not carried over the calls above: a tile beyond dp keeps the 0) ----
#pragma unroll
    for (int q = 0; q < TPW; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) nu[q][i] = 0.f;
    layer_gemm<1, LGCP_NW, 2>(bU, ld, a.cholP, nullptr, dp / 16, dp / 16, wave, lane,
                              [&](int q, int nt, int m, f32x4 acc, float) {
                                const int col = nt * 16 + c;
#pragma unroll
                                for (int i = 0; i < 4; ++i) {
                                  const float v = col < d ? acc[i] : 0.f;
#pragma unroll
                                  for (int qq = 0; qq < TPW; ++qq)
                                    if (qq == q) nu[qq][i] = v;
                                }
                              });
    // ---- phase C: the slice and the shrinking bracket ----
    double lo = theta - two_pi, hi = theta;
    done = false; sub = 0;
#pragma unroll 1
    for (int it = 1; it <= MFM_ESLICE_MAX_SUBITER; ++it) {
      float cs1, sn1, cs[4], sn[4];
      eslice_sincos(theta, cs1, sn1);
#pragma unroll
      for (int i = 0; i < 4; ++i) { cs[i] = __shfl(cs1, 4 * g + i, 64); sn[i] = __shfl(sn1, 4 * g + i, 64); }
      const double llp = evaluate(cs, sn, rows16(done));
      bool acc = false;
      if (!done) {
#pragma clang fp contract(off)
        const double v = a.beta * llp;
        sub = it;
        if (isfinite(v) && v > logy) {
          acc = done = true; ll = llp;
        } else {
          if (theta < 0) lo = theta; else hi = theta;
          if (it < MFM_ESLICE_MAX_SUBITER) theta = lo + (hi - lo) * uniform01(k_sh, (uint32_t)(it - 1), MFM_ESLICE_MAX_SUBITER);
        }
      }
      const uint32_t am = rows16(acc);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if ((am >> (4 * g + i)) & 1u) {
#pragma unroll
          for (int q = 0; q < TPW; ++q) x[q][i] = ellipse(x[q][i], nu[q][i], cs[i], sn[i]);      // (the bits of the evaluated point)
        }
      }
      if (rows16(done) == 0xffffu) break;       // every wave holds the same decisions: the trip count is the workgroup's
    }
    sub_sum += sub; capped += done ? 0 : 1; sub_max = max(sub_max, sub);
    // the thinned trajectory, mfm_mala_run's layout
    if (a.thin > 0 && (s + 1) % a.thin == 0) {
      const size_t snap = (size_t)((s + 1) / a.thin - 1);
      if (a.traj_pos) {
#pragma unroll
        for (int q = 0; q < TPW; ++q) {
          const int col = (wave + LGCP_NW * q) * 16 + c;
          if (col < d) {
#pragma unroll
            for (int i = 0; i < 4; ++i) a.traj_pos[(snap * (size_t)a.B + (size_t)(b0 + 4 * g + i)) * (size_t)d + col] = x[q][i];
          }
        }
      }
      if (a.traj_loglik && writer) a.traj_loglik[snap * (size_t)a.B + (size_t)(b0 + c)] = ll;
    }
  }

  // (the store addresses are formed anew from an opaque copy of the pointer: taken from the loads at the top, the compiler keeps all of
  //  them alive over the kernel and the TPW 13 instance spills them)
  float* pos_out = a.pos;
  asm volatile("" : "+s"(pos_out));
#pragma unroll
  for (int q = 0; q < TPW; ++q) {
    const int col = (wave + LGCP_NW * q) * 16 + c;
    if (col < d) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const size_t o = (size_t)(b0 + 4 * g + i) * d + col;
        pos_out[o] = x[q][i];
        if (a.momentum) a.momentum[o] = nu[q][i];
      }
    }
  }
  if (writer) {
    const int b = b0 + c;
    a.loglik[b] = ll;
    if (a.subiter) a.subiter[b] = sub;
    if (a.theta) a.theta[b] = theta;
    if (a.subiter_sum) a.subiter_sum[b] = sub_sum;
    if (a.n_capped) a.n_capped[b] = capped;
    if (a.subiter_max) a.subiter_max[b] = sub_max;
  }
}

// column tiles per wave and dynamic LDS of the instance that serves a padded dimension dp (0 tiles: none does)
static inline void eslice_plan(int dp, int* tpw, size_t* lds_bytes) {
  const int need = (dp / 16 + LGCP_NW - 1) / LGCP_NW;
  *tpw = need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : need <= 8 ? 8 : need <= 13 ? 13 : 0;
  *lds_bytes = (size_t)(16 * (dp + 4)) * 4 + (size_t)(2 * LGCP_NW * 16) * 8;
}

int launch_eslice(const EsliceArgs& a, hipStream_t stream) {
  int tpw; size_t sm;
  eslice_plan(a.dp, &tpw, &sm);
  if (!tpw || sm > 160 * 1024 || a.B % 16) return -3;
  dim3 grid(a.B / 16), block(LGCP_NW * 64);
#define ES_LAUNCH(T) do { if (a.mode == 0) { (void)hipFuncSetAttribute((const void*)eslice_init_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm); \
                                             hipLaunchKernelGGL(eslice_init_kernel<T>, grid, block, sm, stream, a); } \
                          else { (void)hipFuncSetAttribute((const void*)eslice_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm); \
                                 hipLaunchKernelGGL(eslice_kernel<T>, grid, block, sm, stream, a); } } while (0)
  switch (tpw) { case 1: ES_LAUNCH(1); break; case 2: ES_LAUNCH(2); break; case 4: ES_LAUNCH(4); break; case 8: ES_LAUNCH(8); break; default: ES_LAUNCH(13); }
#undef ES_LAUNCH
  return 0;
}
