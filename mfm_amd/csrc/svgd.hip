// Stein variational gradient descent on the device (bblackjax/vi/svgd.py, optimizers/cocob.py): the all-pairs interaction of one
// iteration as two f32 GEMMs on the exact-f32 matrix pipe (v_mfma_f32_16x16x4_f32), the median heuristic as an exact selection,
// and the elementwise optimizer update.  Arithmetic (include/mfm.h repeats it at the declarations):
//
//   k_ij = exp(-|x_i - x_j|^2 / h)                                                       svgd.py:94-96
//   fg_i = -(1/n) [ (K G)_i + (2/h) ( s_i x_i - (K X)_i ) ],  s_i = sum_j k_ij           :74-84
//   x <- x + optimizer(fg)                                                               :86-87
//   h <- median_{i>j} |x_i - x_j| ^2 / log n   on the NEW particles                      :99-124
//
// sqdist.  D_ij = |x_i - x_j|^2 in the Gram form q_i + q_j - 2 xc_i . xc_j on MEAN-CENTRED coordinates xc = x - column mean (the mean
// in float64, summed in a fixed order; xc and q in float32 scratch).  The Gram form cancels: its absolute error is a few ulp of
// q_i + q_j, so uncentred particles at offset 1000 with spread 1 would lose D entirely; centred, q_i + q_j is of the size of D
// itself for typical pairs and the error is bounded by (d + 8) 2^-23 (q_i + q_j) for ANY summation order (the worst case of a float32
// dot product of length d plus the four roundings of the epilogue).  This is why metrics.hip's pair kernel is NOT reused: it sums
// (x_i - x_j)^2 directly on the vector ALU and reduces to a scalar -- no cancellation, but no matrix pipe and no D or K.G either.
// D is clamped at 0 and its diagonal is set to exactly 0.
//
// gradient.  exp(-D/h) . [G | Xc] with the kernel weights formed from D while the A operand is staged; the row sums s_i are summed
// (vector ALU, fixed order) from the SAME float32 weights in LDS that the MFMAs read.  x_i - x_j = xc_i - xc_j, so the centred
// coordinates serve here too (and s_i xc_i - (K Xc)_i cancels less).  The epilogue combines the three terms per element in registers:
// a workgroup owns the G columns AND the Xc columns of its 32 output columns, so K.G and K.Xc of an element sit in the same lane.
//
// Tiles (both GEMMs): 256 threads = 2 x 2 waves, 64 x 64 tile of the product, K chunks of 32 staged through LDS; a wave holds 2 x 2
// MFMA tiles (four independent accumulators: the 16x16x4 f32 MFMA has a 40-cycle dependent latency on a 32-cycle issue).  For sqdist the
// 64 columns are 64 particles; for the gradient they are 32 columns of G and the same 32 of Xc, i.e. a 64-row x 32-column block of fg.
// LDS: row-major [64][34] float tiles (34: row stride 2 mod 32 banks, so the 32 lanes of a ds_read_b32 half -- 16 rows x 2 k -- hit 32
// banks) and a [32][80] tile for the gradient's B operand (stride 16 mod 32: 2 k-rows x 16 columns per half); sqdist 17.0 KiB, gradient
// 19.5 KiB (row sums included) per workgroup; sqdist 104 VGPRs + 16 accumulator AGPRs (four workgroups per CU), the gradient 120 + 16 with
// the next chunk's operands prefetched into registers under the MFMAs (three per CU); no scratch; LDS would admit eight of either.  Grid at n = 4096, d = 256: sqdist 64 x 64 = 4096 workgroups, gradient 8 x 64 = 512 (two per CU).  The lane -> k map of both operands is k = 4 step + (lane >>
// 4), the same on A and B, so every product is summed in ascending k: a k-ordered fmaf chain per element whatever the tile it sits in
// (a row-range call has the bits of the full call).  The MFMA operand reads are conflict-free; the row-sum reads of the gradient (one per
// weight, a quarter of the chunk per wave) are 2-way conflicted at this stride.
//
// median.  Non-negative floats order as their bit patterns: an 11 + 11 + 10 bit radix selection over the strict lower triangle of D
// (LDS histograms, integer atomics only) finds the two middle order statistics a <= b exactly in three passes over D;
// median = (sqrt a + sqrt b) / 2 and h = median^2 / log n in float64.  Identical particles give 0; what follows is IEEE arithmetic.
//
// apply.  Elementwise, in place, evaluated in float64 and rounded once per stored value.  sgd / adagrad / adam restate optax 0.1.9's
// published formulas (optax is third-party: the parity of these three with optax itself is unpinned, as for AdamW in optim.hip);
// cocob restates optimizers/cocob.py:52-86.
//
// Everything is deterministic (no float atomics; partial sums are combined in a fixed order) and nothing synchronises with the host.
#include <algorithm>
#include <cmath>
#include "common.hip.h"

namespace svgd {

enum { OPT_SGD = 0, OPT_ADAGRAD = 1, OPT_ADAM = 2, OPT_COCOB = 3 };
constexpr int TILE = 64, KC = 32, LDA = KC + 2, LDB = 80, SLABS = 64, RBITS = 11, RBINS = 1 << RBITS;

static inline int pad_to(int v, int m) { return (v + m - 1) / m * m; }

// ---- centring: column means in float64 (two fixed-order stages), xc = x - mean and q = |xc|^2 in float32 ------------------------
__global__ __launch_bounds__(64) void colsum_kernel(const float* __restrict__ x, int n, int d, int rows_per, double* __restrict__ part) {
  const int c = blockIdx.x * 64 + threadIdx.x, s = blockIdx.y;
  if (c >= d) return;
  const int r0 = s * rows_per, r1 = min(n, r0 + rows_per);
  double a = 0.0;
  for (int r = r0; r < r1; ++r) a += (double)x[(size_t)r * d + c];
  part[(size_t)s * d + c] = a;
}
__global__ __launch_bounds__(64) void colmean_kernel(const double* __restrict__ part, int n_slabs, int n, int d, double* __restrict__ mean) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= d) return;
  double a = 0.0;
  for (int s = 0; s < n_slabs; ++s) a += part[(size_t)s * d + c];
  mean[c] = a / (double)n;
}
// one wave per row of the padded scratch xc [n_pad][d_pad]: rows >= n and columns >= d are zero, so the GEMMs load unmasked
__global__ __launch_bounds__(256) void center_kernel(const float* __restrict__ x, const double* __restrict__ mean, int n, int d, int n_pad, int d_pad,
                                                     float* __restrict__ xc, float* __restrict__ q) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n_pad) return;
  double a = 0.0;
  for (int c = lane; c < d_pad; c += 64) {
    float v = 0.f;
    if (r < n && c < d) v = (float)((double)x[(size_t)r * d + c] - mean[c]);
    xc[(size_t)r * d_pad + c] = v;
    a += (double)v * (double)v;
  }
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
  if (lane == 0) q[r] = (float)a;
}

// ---- D = q_i + q_j - 2 xc xc^T ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sqdist_kernel(const float* __restrict__ xc, const float* __restrict__ q, int n, int d_pad, float* __restrict__ D) {
  __shared__ float sA[TILE * LDA], sB[TILE * LDA];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1;
  const int i0 = blockIdx.y * TILE, j0 = blockIdx.x * TILE;
  f32x4 acc[2][2];
  for (int m = 0; m < 2; ++m) for (int u = 0; u < 2; ++u) acc[m][u] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, fk = lane >> 4;
  for (int k0 = 0; k0 < d_pad; k0 += KC) {
#pragma unroll
    for (int e = 0; e < TILE * KC / 256; ++e) {
      const int idx = t + 256 * e, r = idx >> 5, k = idx & 31;
      sA[r * LDA + k] = xc[(size_t)(i0 + r) * d_pad + k0 + k];
      sB[r * LDA + k] = xc[(size_t)(j0 + r) * d_pad + k0 + k];
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < KC / 4; ++s) {
      float a[2], b[2];
      for (int m = 0; m < 2; ++m) a[m] = sA[(32 * wr + 16 * m + fr) * LDA + 4 * s + fk];
      for (int u = 0; u < 2; ++u) b[u] = sB[(32 * wc + 16 * u + fr) * LDA + 4 * s + fk];
      for (int m = 0; m < 2; ++m)
        for (int u = 0; u < 2; ++u) acc[m][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], b[u], acc[m][u], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int j = j0 + 32 * wc + 16 * u + fr;
      if (j >= n) continue;
      const float qj = q[j];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = i0 + 32 * wr + 16 * m + 4 * fk + e;
        if (i >= n) continue;
        const float v = fmaf(-2.f, acc[m][u][e], q[i] + qj);
        D[(size_t)i * n + j] = i == j ? 0.f : fmaxf(v, 0.f);
      }
    }
}

// ---- fg = -(1/n) [ K G + (2/h) (s xc - K Xc) ],  K = exp(-D/h), rows [i0, i0 + n_rows) ------------------------------------------
__global__ __launch_bounds__(256) void gradient_kernel(const float* __restrict__ xc, const float* __restrict__ g, const float* __restrict__ D,
                                                       const double* __restrict__ d_h, int n, int d, int d_pad, int i_lo, int n_rows,
                                                       float* __restrict__ fg) {
  __shared__ float sA[TILE * LDA], sB[KC * LDB], sS[TILE * 4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1;
  const int r0 = blockIdx.y * TILE, c0 = blockIdx.x * 32;          // rows relative to i_lo
  const double h = *d_h;
  const float ninv_h = (float)(-1.0 / h);
  f32x4 acc[2][2];                                                 // [m][0]: K G, [m][1]: K Xc of the same 16 x 16 elements
  for (int m = 0; m < 2; ++m) for (int u = 0; u < 2; ++u) acc[m][u] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, fk = lane >> 4;
  // row-sum role: row of the tile, quarter of the k chunk.  A wave takes one quarter of all 64 rows: with the row stride of 34 floats the
  // 32 lanes of a ds_read_b32 half sit on banks 2 row mod 32, a 2-way conflict (rows r and r + 16), which no assignment of quarters
  // removes (8 sp is even); rows x quarters mixed in one wave would be 2- to 4-way.  The sums are the same numbers in the same order.
  const int sr = t & 63, sp = t >> 6;
  float rs = 0.f;
  // the next chunk's operands are loaded into registers while the MFMAs of this one run (the loads are waited for at the LDS writes)
  float ra[TILE * KC / 256], rb[KC * 64 / 256];
  auto fetch = [&](int j0) {
#pragma unroll
    for (int e = 0; e < TILE * KC / 256; ++e) {
      const int idx = t + 256 * e, r = idx >> 5, k = idx & 31;
      const int i = r0 + r, j = j0 + k;
      ra[e] = (i < n_rows && j < n) ? D[(size_t)(i_lo + i) * n + j] * ninv_h : -INFINITY;      // (exp(-inf) = 0: no weight outside the matrix)
    }
#pragma unroll
    for (int e = 0; e < KC * 64 / 256; ++e) {
      const int idx = t + 256 * e, k = idx >> 6, c = idx & 63;
      const int j = j0 + k;                                        // j < n_pad (a multiple of 64): xc rows past n are zero
      if (c < 32) rb[e] = (j < n && c0 + c < d) ? g[(size_t)j * d + c0 + c] : 0.f;
      else rb[e] = xc[(size_t)j * d_pad + c0 + c - 32];
    }
  };
  fetch(0);
  for (int j0 = 0; j0 < n; j0 += KC) {
#pragma unroll
    for (int e = 0; e < TILE * KC / 256; ++e) {
      const int idx = t + 256 * e, r = idx >> 5, k = idx & 31;
      sA[r * LDA + k] = expf(ra[e]);
    }
#pragma unroll
    for (int e = 0; e < KC * 64 / 256; ++e) {
      const int idx = t + 256 * e, k = idx >> 6, c = idx & 63;
      sB[k * LDB + c] = rb[e];
    }
    __syncthreads();
    if (j0 + KC < n) fetch(j0 + KC);
#pragma unroll
    for (int e = 0; e < KC / 4; ++e) rs += sA[sr * LDA + sp * (KC / 4) + e];
#pragma unroll
    for (int s = 0; s < KC / 4; ++s) {
      float a[2], b[2];
      for (int m = 0; m < 2; ++m) a[m] = sA[(32 * wr + 16 * m + fr) * LDA + 4 * s + fk];
      for (int u = 0; u < 2; ++u) b[u] = sB[(4 * s + fk) * LDB + 32 * u + 16 * wc + fr];
      for (int m = 0; m < 2; ++m)
        for (int u = 0; u < 2; ++u) acc[m][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], b[u], acc[m][u], 0, 0, 0);
    }
    __syncthreads();
  }
  sS[sr * 4 + sp] = rs;
  __syncthreads();
  const int c = c0 + 16 * wc + fr;
  if (c >= d) return;
  const float two_h = (float)(2.0 / h), mninv = (float)(-1.0 / (double)n);
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int rl = 32 * wr + 16 * m + 4 * fk + e, i = r0 + rl;
      if (i >= n_rows) continue;
      const float s_i = ((sS[rl * 4] + sS[rl * 4 + 1]) + sS[rl * 4 + 2]) + sS[rl * 4 + 3];
      const float rep = fmaf(s_i, xc[(size_t)(i_lo + i) * d_pad + c], -acc[m][1][e]);
      fg[(size_t)i * d + c] = mninv * fmaf(two_h, rep, acc[m][0][e]);
    }
}

// ---- median heuristic: exact radix selection of the two middle order statistics of the strict lower triangle ----------------------
struct SelState { uint32_t prefix[2]; uint32_t pad[2]; unsigned long long rank[2]; };      // hist [2][RBINS] follows in the workspace

__global__ void select_init_kernel(SelState* st, uint32_t* hist, unsigned long long r_lo, unsigned long long r_hi) {
  for (int b = threadIdx.x; b < 2 * RBINS; b += blockDim.x) hist[b] = 0u;
  if (threadIdx.x == 0) { st->prefix[0] = st->prefix[1] = 0u; st->rank[0] = r_lo; st->rank[1] = r_hi; }
}
// pass p looks at the bits [shift, shift + bits) of the values whose higher bits equal the selection's prefix
__global__ __launch_bounds__(256) void select_hist_kernel(const float* __restrict__ D, int n, int shift, int bits, const SelState* __restrict__ st,
                                                          uint32_t* __restrict__ hist) {
  __shared__ uint32_t sh[2 * RBINS];
  for (int b = threadIdx.x; b < 2 * RBINS; b += 256) sh[b] = 0u;
  __syncthreads();
  const uint32_t p0 = st->prefix[0], p1 = st->prefix[1], mask = (1u << bits) - 1u;
  const int hi = shift + bits;                                     // (hi == 32 on the first pass: every value matches)
  for (int i = 1 + blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t* row = reinterpret_cast<const uint32_t*>(D) + (size_t)i * n;
    for (int j = threadIdx.x; j < i; j += 256) {
      const uint32_t v = row[j], top = hi >= 32 ? 0u : v >> hi, bin = (v >> shift) & mask;
      if (top == (hi >= 32 ? 0u : p0 >> hi)) atomicAdd(&sh[bin], 1u);
      if (top == (hi >= 32 ? 0u : p1 >> hi)) atomicAdd(&sh[RBINS + bin], 1u);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < 2 * RBINS; b += 256) if (sh[b]) atomicAdd(&hist[b], sh[b]);
}
// one wave per selection walks its histogram: a lane sums its 32 bins, a wave scan finds the lane whose range holds the rank, that lane
// walks its bins; the last pass turns the two values into the length scale
__global__ __launch_bounds__(128) void select_scan_kernel(SelState* st, uint32_t* hist, int shift, int bits, int last, double log_n, double* __restrict__ out) {
  __shared__ uint32_t val[2];
  constexpr int PER = RBINS / 64;
  const int t = threadIdx.x, sel = t >> 6, lane = t & 63;
  const uint32_t* hh = hist + sel * RBINS + lane * PER;
  uint32_t c[PER], tot = 0;
#pragma unroll
  for (int e = 0; e < PER; ++e) { c[e] = hh[e]; tot += c[e]; }
  unsigned long long incl = tot;
  for (int o = 1; o < 64; o <<= 1) { const unsigned long long v = __shfl_up(incl, o); if (lane >= o) incl += v; }
  const unsigned long long r = st->rank[sel], m = __ballot(incl > r);
  const int f = m ? __ffsll((long long)m) - 1 : 63;
  if (lane == f) {
    unsigned long long rr = m ? r - (incl - tot) : 0ull;
    uint32_t b = PER - 1; bool found = false;
#pragma unroll
    for (int e = 0; e < PER; ++e)
      if (!found) { if (rr < c[e]) { b = e; found = true; } else rr -= c[e]; }
    st->rank[sel] = rr;
    const uint32_t p = st->prefix[sel] | (((uint32_t)(lane * PER) + b) & ((1u << bits) - 1u)) << shift;
    st->prefix[sel] = p;
    val[sel] = p;
  }
  __syncthreads();
  for (int i = t; i < 2 * RBINS; i += 128) hist[i] = 0u;
  if (last && t == 0) {
    const double a = sqrt((double)__uint_as_float(val[0])), d = sqrt((double)__uint_as_float(val[1]));
    const double med = 0.5 * (a + d);
    *out = med * med / log_n;
  }
}

// ---- optimizer update (float64 arithmetic, one rounding per stored float) ------------------------------------------------------------
struct ApplyArgs { int kind; double hp[4]; long long count; size_t total; float* x; const float* fg; float* s[5]; };

__global__ __launch_bounds__(256) void apply_kernel(ApplyArgs a) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.total) return;
  const double c = (double)a.fg[e], p = (double)a.x[e];
  if (a.kind == OPT_SGD) {                                         // optax.sgd: updates = -learning_rate * fg
    a.x[e] = (float)(p + -(a.hp[0] * c));
  } else if (a.kind == OPT_ADAGRAD) {                              // optax 0.1.9 scale_by_rss: acc += fg^2; fg * rsqrt(acc + eps) where acc > 0, else 0
    const double acc = (double)a.s[0][e] + c * c;
    a.s[0][e] = (float)acc;
    const double u = acc > 0.0 ? c / sqrt(acc + a.hp[2]) : 0.0;
    a.x[e] = (float)(p + -(a.hp[0] * u));
  } else if (a.kind == OPT_ADAM) {                                 // optax.adam: bias-corrected moments, eps outside the square root
    const double b1 = a.hp[1], b2 = a.hp[2], tt = (double)(a.count + 1);
    const double m = b1 * (double)a.s[0][e] + (1.0 - b1) * c, v = b2 * (double)a.s[1][e] + (1.0 - b2) * c * c;
    a.s[0][e] = (float)m; a.s[1][e] = (float)v;
    const double mh = m / (1.0 - pow(b1, tt)), vh = v / (1.0 - pow(b2, tt));
    a.x[e] = (float)(p + -(a.hp[0] * (mh / (sqrt(vh) + a.hp[3]))));
  } else {                                                         // cocob.py:55-81; s = {init_particles, cumulative_gradients, scale, subgradients, reward}
    const double alpha = a.hp[0], p0 = (double)a.s[0][e];
    const double L = fmax((double)a.s[2][e], fabs(c));
    const double G = (double)a.s[3][e] + fabs(c);
    const double R = fmax((double)a.s[4][e] - c * (p - p0), 0.0);
    const double C = (double)a.s[1][e] - c;
    a.s[1][e] = (float)C; a.s[2][e] = (float)L; a.s[3][e] = (float)G; a.s[4][e] = (float)R;
    const double upd = -p + (p0 + C / (L * fmax(G + L, alpha * L)) * (L + R));
    a.x[e] = (float)(p + upd);
  }
}

// ---- launches ---------------------------------------------------------------------------------------------------------------------------
struct Scratch {                 // carved from one allocation (api.hip: svgd_ws)
  float *xc, *q; double *part, *mean; SelState* sel; uint32_t* hist;
  int n_pad, d_pad;
};
static size_t scratch_bytes(int n, int d) {
  const size_t n_pad = pad_to(n, TILE), d_pad = pad_to(d, KC);
  return n_pad * d_pad * 4 + n_pad * 4 + ((size_t)SLABS * d + d) * 8 + 256 + sizeof(SelState) + 2 * RBINS * 4 + 256;
}
static Scratch carve(void* base, int n, int d) {
  Scratch s; s.n_pad = pad_to(n, TILE); s.d_pad = pad_to(d, KC);
  char* p = (char*)base;
  s.part = (double*)p; p += (size_t)SLABS * d * 8;
  s.mean = (double*)p; p += (size_t)d * 8;
  s.sel = (SelState*)p; p += sizeof(SelState);
  s.hist = (uint32_t*)p; p += 2 * RBINS * 4;
  p = (char*)(((uintptr_t)p + 255) & ~(uintptr_t)255);
  s.xc = (float*)p; p += (size_t)s.n_pad * s.d_pad * 4;
  s.q = (float*)p;
  return s;
}

static void launch_center(const Scratch& s, const float* x, int n, int d, hipStream_t st) {
  const int n_slabs = std::min((int)SLABS, (n + 63) / 64), rows_per = (n + n_slabs - 1) / n_slabs;
  colsum_kernel<<<dim3((d + 63) / 64, n_slabs), 64, 0, st>>>(x, n, d, rows_per, s.part);
  colmean_kernel<<<(d + 63) / 64, 64, 0, st>>>(s.part, n_slabs, n, d, s.mean);
  center_kernel<<<s.n_pad / 4, 256, 0, st>>>(x, s.mean, n, d, s.n_pad, s.d_pad, s.xc, s.q);
}
static void launch_sqdist(const Scratch& s, const float* x, int n, int d, float* D, hipStream_t st) {
  launch_center(s, x, n, d, st);
  sqdist_kernel<<<dim3(s.n_pad / TILE, s.n_pad / TILE), 256, 0, st>>>(s.xc, s.q, n, s.d_pad, D);
}
// centred: s.xc already holds the centred coordinates of these particles (the composite, straight after its sqdist)
static void launch_gradient(const Scratch& s, const float* x, const float* g, const float* D, const double* d_h, int n, int d, int i0, int n_rows,
                            float* fg, bool centred, hipStream_t st) {
  if (!centred) launch_center(s, x, n, d, st);
  gradient_kernel<<<dim3((d + 31) / 32, (n_rows + TILE - 1) / TILE), 256, 0, st>>>(s.xc, g, D, d_h, n, d, s.d_pad, i0, n_rows, fg);
}
static void launch_median(const Scratch& s, const float* D, int n, double* d_out, hipStream_t st) {
  const unsigned long long m = (unsigned long long)n * (unsigned long long)(n - 1) / 2;
  select_init_kernel<<<1, 256, 0, st>>>(s.sel, s.hist, (m - 1) / 2, m / 2);
  const int shifts[3] = {21, 10, 0}, bits[3] = {11, 11, 10};
  const int grid = std::min(n - 1, 2048);
  const double log_n = std::log((double)n);
  for (int p = 0; p < 3; ++p) {
    select_hist_kernel<<<grid, 256, 0, st>>>(D, n, shifts[p], bits[p], s.sel, s.hist);
    select_scan_kernel<<<1, 128, 0, st>>>(s.sel, s.hist, shifts[p], bits[p], p == 2, log_n, d_out);
  }
}
static void launch_apply(const ApplyArgs& a, hipStream_t st) {
  apply_kernel<<<(unsigned)((a.total + 255) / 256), 256, 0, st>>>(a);
}

}  // namespace svgd
