// N3: chain diagnostics on the device -- autocorrelation of a trajectory along its time axis and Geyer's initial-positive-
// sequence estimate of the integrated autocorrelation time / effective sample size.  Replaces mcmc_utils.py:131-165
// (autocorrelation; the reference pads to a fast length and goes through rfft / irfft in float64 on the host).
//
// Input x: float32 [n][S], time-major, S = n_chain * dim series: what mfm_mala_run writes with thin > 0.  Series s is the strided column
// x[t * S + s].  Per series: mean (float64), centred signal c_t = x_t - mean, lag sums A_k = sum_{t < n-k} c_t c_{t+k} for
// k = 0 .. L-1, rho_k = A_k / A_0; Gamma_m = rho_2m + rho_2m+1, tau = -1 + 2 sum of the leading run of Gamma_m > 0 (only pairs
// with 2m+1 < L), ess = n / tau.
//
// Mapping.  ONE LANE PER SERIES, consecutive lanes on consecutive s: every load of a time row is one coalesced 256-byte
// wave access, there is no transpose through LDS, no cross-lane traffic, no atomics and no temporary of the trajectory's size;
// each output element has one writer and one summation order (deterministic).  A lane serves AC_LB consecutive lags at a
// time: AC_LB accumulators plus a register ring of the AC_LB delayed values c_{u-k0-j}; the time loop is unrolled by the ring
// length, so slot (i - j) mod AC_LB of step i is a compile-time register.  One pass over u = k0 .. n-1 serves a lag block
// with two loads (x_u, x_{u-k0}; one for k0 = 0) per AC_LB FMAs.  Products and sums are float32 inside a block of AC_TB time
// steps and float64 across blocks (the scheme of metrics.hip); MFM_AUTOCORR_F64=1 (read at mfm_create) keeps the centred
// signal, the products and the sums in float64 throughout (tools/autocorr_time.py times one against the other).  The
// centring itself is float64 in both: c_t = (float)((double)x_t - mean).
//   - rho requested: one workgroup per (series block, lag block); A_k is stored as float32 in the caller's rho buffer and normalised
//     in place by autocorr_finish_kernel, which also runs Geyer's sum.
//   - rho not requested: the SAME lag-block routine, the lag blocks of a lane in sequence, Geyer's sum taken block by block,
//     and a wave stops at the first block by which all of its lanes have met a non-positive Gamma: no [L][S] buffer at all,
//     and the work is tau-sized rather than L-sized.  Same arithmetic per (series, lag) => tau / ess are bit-identical.
// mean / var (var = A_0 / n with A_0 summed in float64 from the float64-centred signal) come from autocorr_stats_kernel.
//
// Edge semantics: A_0 = 0 (constant series, n = 1) gives NaN in rho, tau and ess (the reference divides 0 / 0 with the
// warnings silenced); a non-finite input makes its own series NaN (mean is NaN) and no other: lanes never exchange data.
//
// Bound: VALU, n L / 2 FMAs per series (tau only: n * (lags up to the truncation point)).  All index arithmetic is 64-bit.
#include "common.hip.h"
#include <type_traits>

#define AC_LB MFM_AUTOCORR_LAG_BLOCK          // lags per lane and pass (include/mfm.h; even: Geyer's pairs never straddle two blocks)
#define AC_TB MFM_AUTOCORR_TIME_BLOCK         // time steps summed in float32 before the float64 flush (a multiple of AC_LB)
static_assert(AC_LB % 2 == 0 && AC_TB % AC_LB == 0, "lag block even, time block a multiple of it");

// mean and A_0 of every series in float64 (two passes over the column; the second is served from cache for short columns)
__global__ __launch_bounds__(64) void autocorr_stats_kernel(const float* __restrict__ x, int64_t n, int64_t S, double* __restrict__ mean,
                                                            double* __restrict__ var) {
  const int64_t s = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (s >= S) return;
  const float* p = x + s;
  double sum = 0.0;
#pragma unroll 8
  for (int64_t t = 0; t < n; ++t) sum += (double)p[t * S];
  const double mu = sum / (double)n;
  mean[s] = mu;
  if (var) {
    double a0 = 0.0;
#pragma unroll 8
    for (int64_t t = 0; t < n; ++t) { const double c = (double)p[t * S] - mu; a0 = fma(c, c, a0); }
    var[s] = a0 / (double)n;
  }
}

__device__ __forceinline__ float ac_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double ac_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// AC_LB time steps u0 .. u0 + AC_LB - 1 of the lag block that starts at lag k0 (GUARD: the chunk may reach past n - 1).  The loads go
// AC_SB steps ahead of the FMAs, fenced so that the scheduler keeps that distance: left to itself it hoists all 2 AC_LB loads and their
// float64 centring to the top of the chunk and spills.
#define AC_SB 8
template <bool GUARD>
__device__ __forceinline__ void lag_fetch(const float*& pq, int64_t S, int64_t k0S, int64_t left, int i0, float (&rc)[AC_SB],
                                          float (&rd)[AC_SB]) {
#pragma unroll
  for (int e = 0; e < AC_SB; ++e) {
    rc[e] = 0.f; rd[e] = 0.f;
    if (!GUARD || i0 + e < left) {
      rc[e] = *pq;
      if (k0S) rd[e] = *(pq - k0S);
    }
    pq += S;                                                        // a walking per-lane pointer: 64 uniform offsets would spill the SGPR file
  }
}
template <typename T, bool GUARD>
__device__ __forceinline__ void lag_chunk(const float* __restrict__ pc, int64_t S, int64_t k0S, int64_t left, double mu, T (&ring)[AC_LB],
                                          T (&acc)[AC_LB]) {
  float rc[AC_SB], rd[AC_SB], nc[AC_SB], nd[AC_SB];
  const float* pq = pc;
  lag_fetch<GUARD>(pq, S, k0S, left, 0, rc, rd);
#pragma unroll
  for (int i0 = 0; i0 < AC_LB; i0 += AC_SB) {
    if (i0 + AC_SB < AC_LB) lag_fetch<GUARD>(pq, S, k0S, left, i0 + AC_SB, nc, nd);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int e = 0; e < AC_SB; ++e) {
      const int i = i0 + e;
      T cur = (T)0, del = (T)0;
      if (!GUARD || i < left) {                                     // past the end: c = 0, the step adds nothing
        cur = (T)((double)rc[e] - mu);
        del = k0S ? (T)((double)rd[e] - mu) : cur;
      }
      ring[i] = del;                                                // c_{u - k0}; slot (i - j) mod AC_LB holds c_{u - k0 - j}
#pragma unroll
      for (int j = 0; j < AC_LB; ++j) acc[j] = ac_fma(cur, ring[(i - j + AC_LB) % AC_LB], acc[j]);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int e = 0; e < AC_SB; ++e) { rc[e] = nc[e]; rd[e] = nd[e]; }
  }
}

// A[j] = A_{k0 + j}, j = 0 .. AC_LB - 1, of the series whose column starts at p (lags past n - 1 come out as 0)
template <bool F64>
__device__ __forceinline__ void lag_block(const float* __restrict__ p, int64_t n, int64_t S, int64_t k0, double mu, double (&A)[AC_LB]) {
  typedef typename std::conditional<F64, double, float>::type T;
  T ring[AC_LB], acc[AC_LB];
#pragma unroll
  for (int j = 0; j < AC_LB; ++j) { ring[j] = (T)0; acc[j] = (T)0; A[j] = 0.0; }      // the zero ring is c_t = 0 for t < 0
  const int64_t k0S = k0 * S;
  const float* pc = p + k0S;
  int64_t left = n - k0;                                            // time steps u = k0 .. n - 1
  while (left > 0) {
    int64_t blk = left < AC_TB ? left : AC_TB;
    left -= blk;
    for (; blk >= AC_LB; blk -= AC_LB, pc += (int64_t)AC_LB * S) lag_chunk<T, false>(pc, S, k0S, AC_LB, mu, ring, acc);
    if (blk > 0) lag_chunk<T, true>(pc, S, k0S, blk, mu, ring, acc);      // (only the last time block has a partial chunk)
    if (!F64) {
#pragma unroll
      for (int j = 0; j < AC_LB; ++j) { A[j] += (double)acc[j]; acc[j] = 0.f; }
    }
  }
  if (F64) {
#pragma unroll
    for (int j = 0; j < AC_LB; ++j) A[j] = (double)acc[j];
  }
}

// rho_k from the float32-stored lag sums: the one formula of both paths (a0 / a0 = 1 exactly)
__device__ __forceinline__ float ac_rho(float ak, float a0, bool bad) { return bad ? __builtin_nanf("") : (float)((double)ak / (double)a0); }
__device__ __forceinline__ bool ac_bad(float a0) { return !(a0 > 0.f && a0 < __builtin_inff()); }
// Geyer's running sum: adds Gamma while the leading run of positive Gammas lasts
struct Geyer { double sum; bool done; };
__device__ __forceinline__ void geyer_pair(Geyer& g, float r0, float r1) {
  if (g.done) return;
  const double G = (double)r0 + (double)r1;
  if (G > 0.0) g.sum += G; else g.done = true;
}
__device__ __forceinline__ void geyer_store(const Geyer& g, bool bad, int64_t n, int64_t s, float* tau, float* ess) {
  const double t = bad ? (double)__builtin_nanf("") : -1.0 + 2.0 * g.sum;
  if (tau) tau[s] = (float)t;
  if (ess) ess[s] = (float)((double)n / t);
}

// rho requested: one workgroup = 64 series x one lag block; R [L][S] receives A_k as float32.  Workgroup id -> (series block, lag
// block) so that the lag blocks of a series block run at the same time on one XCD (ids that agree mod 8 share an XCD's L2 as the
// dispatcher is observed to place them; a different placement changes the speed only): they read the same delayed row at the same time
// and each other's current rows 32 steps apart, so the trajectory comes from HBM about once instead of once per lag block.
template <bool F64>
__global__ __launch_bounds__(64, 2) void autocorr_lags_kernel(const float* __restrict__ x, int64_t n, int64_t S, int L, int64_t n_sblocks,
                                                              int n_lblocks, const double* __restrict__ mean, float* __restrict__ R) {
  const int64_t id = blockIdx.x, slot = id >> 3;
  const int64_t sblock = (slot / n_lblocks) * 8 + (id & 7);
  if (sblock >= n_sblocks) return;                                  // (the grid is rounded up to 8 series blocks)
  const int64_t s = sblock * 64 + threadIdx.x, sc = s < S ? s : S - 1;      // idle lanes recompute the last series
  const int64_t k0 = (slot % n_lblocks) * AC_LB;
  double A[AC_LB];
  lag_block<F64>(x + sc, n, S, k0, mean[sc], A);
  if (s < S) {
#pragma unroll
    for (int j = 0; j < AC_LB; ++j)
      if (k0 + j < L) R[(k0 + j) * S + s] = (float)A[j];
  }
}

// rho not requested: the lag blocks of a lane in sequence, until every lane of the wave has closed its Geyer sum
template <bool F64>
__global__ __launch_bounds__(64, 2) void autocorr_tau_kernel(const float* __restrict__ x, int64_t n, int64_t S, int L, const double* __restrict__ mean,
                                                          float* __restrict__ tau, float* __restrict__ ess) {
  const int64_t s = (int64_t)blockIdx.x * 64 + threadIdx.x, sc = s < S ? s : S - 1;
  const double mu = mean[sc];
  Geyer g = {0.0, false};
  float a0 = 0.f; bool bad = false;
  for (int64_t k0 = 0; k0 < L; k0 += AC_LB) {
    double A[AC_LB];
    lag_block<F64>(x + sc, n, S, k0, mu, A);
    if (k0 == 0) { a0 = (float)A[0]; bad = ac_bad(a0); if (bad) g.done = true; }
#pragma unroll
    for (int j = 0; j < AC_LB; j += 2)
      if (k0 + j + 1 < L) geyer_pair(g, ac_rho((float)A[j], a0, bad), ac_rho((float)A[j + 1], a0, bad));
    if (__all(g.done)) break;
  }
  if (s < S) geyer_store(g, bad, n, s, tau, ess);
}

// normalise R in place (A_k -> rho_k) and take Geyer's sum over it; one lane per series
__global__ __launch_bounds__(64) void autocorr_finish_kernel(float* __restrict__ R, int64_t n, int64_t S, int L, float* __restrict__ tau,
                                                             float* __restrict__ ess) {
  const int64_t s = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (s >= S) return;
  float* r = R + s;
  const float a0 = r[0];
  const bool bad = ac_bad(a0);
  Geyer g = {0.0, bad};
  int64_t k = 0;
  for (; k + 1 < L; k += 2) {
    const float r0 = ac_rho(r[k * S], a0, bad), r1 = ac_rho(r[(k + 1) * S], a0, bad);
    r[k * S] = r0; r[(k + 1) * S] = r1;
    geyer_pair(g, r0, r1);
  }
  if (k < L) r[k * S] = ac_rho(r[k * S], a0, bad);
  if (tau || ess) geyer_store(g, bad, n, s, tau, ess);
}

// d_mean_ws: the caller's d_mean or a context buffer of S doubles.  Returns non-zero when the grid does not fit.
static int launch_autocorr(bool f64, const float* x, int64_t n, int64_t S, int L, float* rho, float* tau, float* ess, double* mean_ws, double* var,
                           hipStream_t stream) {
  const int64_t gx = (S + 63) / 64, gy = ((int64_t)L + AC_LB - 1) / AC_LB;
  const int64_t g_lags = (gx + 7) / 8 * 8 * gy;                     // autocorr_lags_kernel: 8 series blocks abreast, see there
  if (gx > 0x7fffffffLL || (rho && g_lags > 0x7fffffffLL)) return 1;
  hipLaunchKernelGGL(autocorr_stats_kernel, dim3((unsigned)gx), dim3(64), 0, stream, x, n, S, mean_ws, var);
  if (rho) {
    if (f64) hipLaunchKernelGGL(autocorr_lags_kernel<true>, dim3((unsigned)g_lags), dim3(64), 0, stream, x, n, S, L, gx, (int)gy, mean_ws, rho);
    else hipLaunchKernelGGL(autocorr_lags_kernel<false>, dim3((unsigned)g_lags), dim3(64), 0, stream, x, n, S, L, gx, (int)gy, mean_ws, rho);
    hipLaunchKernelGGL(autocorr_finish_kernel, dim3((unsigned)gx), dim3(64), 0, stream, rho, n, S, L, tau, ess);
  } else if (tau || ess) {
    if (f64) hipLaunchKernelGGL(autocorr_tau_kernel<true>, dim3((unsigned)gx), dim3(64), 0, stream, x, n, S, L, mean_ws, tau, ess);
    else hipLaunchKernelGGL(autocorr_tau_kernel<false>, dim3((unsigned)gx), dim3(64), 0, stream, x, n, S, L, mean_ws, tau, ess);
  }
  return 0;
}

// ---- cross-chain sums: split-R-hat and the multi-chain effective sample size (mfm_chain_sums / mfm_chain_diag, include/mfm.h) -----------
// Input x: float32 [n][n_chain_ld][dim]; chains 0 .. n_chain - 1 of every row are used.  Sub-chain (m, h) is the column of chain m over the
// rows [0, n_sub) (h = 0) or [n - n_sub, n) (h = 1; split only).  Per sub-chain and coordinate: the float64 mean mu and the lag sums A_k
// of the signal centred by ITS OWN mean -- lag_block above on (pointer, n_sub, row stride), unchanged, with A_0 replaced by the float64 sum
// of autocorr_stats_kernel.  New here is the sum over sub-chains: sums [L + 2][dim] = (sum mu, sum mu^2, sum A_0, .., sum A_{L-1}).
//
// Mapping.  One wave (one workgroup) per (block of 64 coordinates, lag block, slice of chains); consecutive lanes on consecutive
// coordinates, so a time row of a chain is one coalesced load for dim >= 64; for dim < 64 a wave lays 64 / dim chains side by side (lane
// = chain-in-group * dim + coordinate) and a row of those chains is still one contiguous stretch.  The wave walks the chains of its slice
// in index order, both halves of a chain in turn, and adds each sub-chain's A_k into float64 totals that live across the whole slice in
// LDS (tot [AC_LB + 2][64], every lane its own column: no exchange, no barrier inside the loop; in registers they would take the lag
// kernel past 256 VGPRs).  mu and A_0 come from chain_stats_kernel (2 doubles per sub-chain and coordinate): every lag block then does the same
// work per sub-chain, so the lag blocks of a slice stay in step and share their rows in L2 as those of autocorr_lags_kernel do (with the
// mean recomputed inside the wave, and A_0 by lag block 0 alone, block 0 fell behind the others: DESIGN.md section 4.13).  At the end the side-by-side chains of a coordinate are added in group order by the lane of group 0, and the
// wave stores its rows of the slab [n_slices][L + 2][dim]; chain_sums_reduce_kernel adds the slabs in slice order.  No atomics, one writer
// per element, a summation order fixed by (n_chain, dim) alone.  Workgroup ids are dealt as in autocorr_lags_kernel: the lag blocks of
// a (coordinate block, slice) run together on one XCD.  Offsets are 64-bit.
#define CS_SLICES_MAX MFM_CHAIN_SLICES_MAX    // cap of coordinate blocks x chain slices (include/mfm.h)

// mean and A_0 of every sub-chain and coordinate in float64, the two passes of autocorr_stats_kernel; one lane per (chain, half, coordinate)
// of the n_chain valid chains, stats [2][n_chain * n_half][dim]
__global__ __launch_bounds__(64) void chain_stats_kernel(const float* __restrict__ x, int64_t n_sub, int64_t t1, int n_half, int64_t n_chain, int64_t S, int dim,
                                                         double* __restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x, n_rows = n_chain * n_half;
  if (i >= n_rows * dim) return;
  const int64_t m = i / dim, c = m / n_half;
  const int j = (int)(i - m * dim), h = (int)(m - c * n_half);
  const float* p = x + ((h ? t1 : 0) * S + c * dim + j);
  double sum = 0.0;
#pragma unroll 8
  for (int64_t t = 0; t < n_sub; ++t) sum += (double)p[t * S];
  const double mu = sum / (double)n_sub;
  double a0 = 0.0;
#pragma unroll 8
  for (int64_t t = 0; t < n_sub; ++t) { const double cv = (double)p[t * S] - mu; a0 = fma(cv, cv, a0); }
  stats[i] = mu;
  stats[n_rows * dim + i] = a0;
}

struct ChainPlan { int n_cblocks, n_lblocks, n_slices, per_slice; int64_t n_units, grid; };
static ChainPlan chain_plan(int n_chain, int dim, int L) {
  ChainPlan q;
  const int w = dim < 64 ? dim : 64, cpw = 64 / w;
  q.n_cblocks = (dim + 63) / 64;
  q.n_lblocks = (L + AC_LB - 1) / AC_LB;
  // the slices depend on (n_chain, dim) and NOT on L: the order in which the chains are added, and with it every bit of the rows a call
  // with fewer lags also has, is the same for every L.  Coordinate blocks x slices <= CS_SLICES_MAX: one wave per CU for every lag block.
  int64_t want = CS_SLICES_MAX / q.n_cblocks;
  if (want < 1) want = 1;
  const int64_t groups = ((int64_t)n_chain + cpw - 1) / cpw;       // a group: the chains a wave holds side by side
  if (want > groups) want = groups;
  q.per_slice = (int)((groups + want - 1) / want) * cpw;
  q.n_slices = (n_chain + q.per_slice - 1) / q.per_slice;          // (no empty slice)
  q.n_units = (int64_t)q.n_cblocks * q.n_slices;
  q.grid = (q.n_units + 7) / 8 * 8 * q.n_lblocks;
  return q;
}

template <bool F64>
__global__ __launch_bounds__(64, 2) void chain_sums_kernel(const float* __restrict__ x, int64_t n_sub, int64_t t1, int n_half, int n_chain, int64_t S,
                                                           int dim, int L, int n_cblocks, int n_lblocks, int64_t n_units, int per_slice,
                                                           const double* __restrict__ stats, double* __restrict__ slab) {
  __shared__ double tot[AC_LB + 2][64];
  const int64_t id = blockIdx.x, slot = id >> 3;
  const int64_t unit = (slot / n_lblocks) * 8 + (id & 7);
  if (unit >= n_units) return;                                      // (the grid is rounded up to 8 units)
  const int lb = (int)(slot % n_lblocks), cb = (int)(unit % n_cblocks);
  const int64_t slice = unit / n_cblocks, k0 = (int64_t)lb * AC_LB;
  const int lane = threadIdx.x, w = dim < 64 ? dim : 64, cpw = 64 / w;
  const int g = lane / w, j = cb * 64 + (lane - g * w), jc = j < dim ? j : dim - 1;      // idle lanes recompute the last coordinate
  const bool lane_ok = g < cpw && j < dim;
  const int64_t c0 = slice * per_slice;
  const int64_t c1 = c0 + per_slice < n_chain ? c0 + per_slice : n_chain;
#pragma unroll
  for (int r = 0; r < AC_LB + 2; ++r) tot[r][lane] = 0.0;
  for (int64_t cbase = c0; cbase < c1; cbase += cpw) {
    const int64_t c = cbase + g, cc = c < c1 ? c : c1 - 1;         // ... and the last chain of the slice: never a chain past n_chain
    const bool ok = lane_ok && c < c1;
    for (int h = 0; h < n_half; ++h) {
      const float* p = x + ((h ? t1 : 0) * S + cc * dim + jc);
      const int64_t si = (cc * n_half + h) * dim + jc;
      const double mu = stats[si];
      double A[AC_LB];
      lag_block<F64>(p, n_sub, S, k0, mu, A);
      if (lb == 0) {
        A[0] = stats[(int64_t)n_chain * n_half * dim + si];        // A_0 in float64
        if (ok) { tot[0][lane] += mu; tot[1][lane] += mu * mu; }
      }
      if (ok) {
#pragma unroll
        for (int i = 0; i < AC_LB; ++i) tot[2 + i][lane] += A[i];
      }
    }
  }
  __syncthreads();
  if (g == 0 && j < dim) {
    double* out = slab + slice * ((int64_t)L + 2) * dim + j;
    const int r0 = lb == 0 ? 0 : 2;
    for (int r = r0; r < AC_LB + 2; ++r) {
      const int64_t row = r < 2 ? r : 2 + k0 + (r - 2);
      if (row >= (int64_t)L + 2) break;
      double s = tot[r][lane];
      for (int gg = 1; gg < cpw; ++gg) s += tot[r][lane + gg * w];
      out[row * dim] = s;
    }
  }
}

__global__ __launch_bounds__(256) void chain_sums_reduce_kernel(const double* __restrict__ slab, int64_t n_elem, int n_slices, double* __restrict__ sums) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_elem) return;
  double s = slab[i];
  for (int64_t sl = 1; sl < n_slices; ++sl) s += slab[sl * n_elem + i];
  sums[i] = s;
}

// R-hat, rho-hat, tau and ess of every coordinate from the sums over ALL sub-chains (include/mfm.h has the formulas); one lane per
// coordinate, float64 throughout, Geyer's rule as in mfm_autocorr (leading run of positive pair sums: no monotone smoothing, no clamp)
__global__ __launch_bounds__(64) void chain_diag_kernel(const double* __restrict__ sums, int64_t n_sub, int64_t M, int dim, int L, float* __restrict__ rhat,
                                                        float* __restrict__ ess, float* __restrict__ tau, float* __restrict__ rho) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= dim) return;
  const double Md = (double)M, den = Md * (double)(n_sub - 1), s0 = sums[j], s1 = sums[(int64_t)dim + j];
  const double W = sums[2 * (int64_t)dim + j] / den;
  const double Bn = (s1 - s0 * s0 / Md) / (Md - 1.0);
  const double varp = (double)(n_sub - 1) / (double)n_sub * W + Bn;
  const double inf = (double)__builtin_inff();
  const bool bad = !(W > 0.0 && W < inf) || !(varp > -inf && varp < inf);
  const float nanf_ = __builtin_nanf("");
  if (rhat) rhat[j] = bad ? nanf_ : (float)sqrt(varp / W);
  Geyer g = {0.0, bad};
  int64_t k = 0;
  for (; k + 1 < L; k += 2) {
    if (g.done && !rho) break;
    const double r0 = 1.0 - (W - sums[(2 + k) * dim + j] / den) / varp, r1 = 1.0 - (W - sums[(3 + k) * dim + j] / den) / varp;
    if (rho) { rho[k * dim + j] = bad ? nanf_ : (float)r0; rho[(k + 1) * dim + j] = bad ? nanf_ : (float)r1; }
    if (!g.done) { const double G = r0 + r1; if (G > 0.0) g.sum += G; else g.done = true; }
  }
  if (rho && k < L) rho[k * dim + j] = bad ? nanf_ : (float)(1.0 - (W - sums[(2 + k) * dim + j] / den) / varp);
  const double t = bad ? (double)nanf_ : -1.0 + 2.0 * g.sum;
  if (tau) tau[j] = (float)t;
  if (ess) ess[j] = (float)(Md * (double)n_sub / t);
}

// ws: the stats [2][n_chain * n_half][dim], then the slab [plan.n_slices][L + 2][dim] (doubles).  Returns non-zero when a grid does not fit.
static size_t chain_stats_count(int n_chain, int dim, int split) { return (size_t)2 * (size_t)n_chain * (split ? 2 : 1) * (size_t)dim; }
static int launch_chain_sums(bool f64, const float* x, int64_t n, int n_chain, int n_chain_ld, int dim, int split, int L, const ChainPlan& q, double* ws,
                             double* sums, hipStream_t stream) {
  const int64_t n_sub = split ? n / 2 : n, S = (int64_t)n_chain_ld * dim, n_elem = ((int64_t)L + 2) * dim, g_red = (n_elem + 255) / 256;
  const int n_half = split ? 2 : 1;
  const int64_t g_stats = ((int64_t)n_chain * n_half * dim + 63) / 64;
  if (q.grid > 0x7fffffffLL || g_red > 0x7fffffffLL || g_stats > 0x7fffffffLL) return 1;
  double* stats = ws;
  double* slab = ws + chain_stats_count(n_chain, dim, split);
  hipLaunchKernelGGL(chain_stats_kernel, dim3((unsigned)g_stats), dim3(64), 0, stream, x, n_sub, n - n_sub, n_half, (int64_t)n_chain, S, dim, stats);
  if (f64) hipLaunchKernelGGL(chain_sums_kernel<true>, dim3((unsigned)q.grid), dim3(64), 0, stream, x, n_sub, n - n_sub, n_half, n_chain, S, dim, L, q.n_cblocks,
                              q.n_lblocks, q.n_units, q.per_slice, stats, slab);
  else hipLaunchKernelGGL(chain_sums_kernel<false>, dim3((unsigned)q.grid), dim3(64), 0, stream, x, n_sub, n - n_sub, n_half, n_chain, S, dim, L, q.n_cblocks,
                          q.n_lblocks, q.n_units, q.per_slice, stats, slab);
  hipLaunchKernelGGL(chain_sums_reduce_kernel, dim3((unsigned)g_red), dim3(256), 0, stream, slab, n_elem, q.n_slices, sums);
  return 0;
}
static void launch_chain_diag(const double* sums, int64_t n_sub, int64_t M, int dim, int L, float* rhat, float* ess, float* tau, float* rho, hipStream_t stream) {
  hipLaunchKernelGGL(chain_diag_kernel, dim3((unsigned)((dim + 63) / 64)), dim3(64), 0, stream, sums, n_sub, M, dim, L, rhat, ess, tau, rho);
}
