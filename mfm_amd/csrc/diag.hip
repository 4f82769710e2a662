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
