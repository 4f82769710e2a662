// The Dormand-Prince 5(4) integrator of jax.experimental.ode.odeint (oracle/ode.py), per row and
// independent of layout: the tableau, the initial-step heuristic (Hairer II.4, order 4), the step-size controller, the
// prescribed-step replay hooks (mfm_debug_replay) and the 4th-order dense output.  Every adaptive CNF solver uses these:
// ode.hip (the generic 16-chain tile), ode_d2.hip (the d = 2 four-chain tiles), ode_fast.hip (the shape-specialised
// tiles) and wide.hip (the wide family).  What stays with a family is its data layout, its reductions and which lane
// writes.  Each expression is written once here, operand order and contraction included: the kernels compute the same
// bits through these helpers as they would with the expressions in line.
#pragma once
#include "common.hip.h"

__device__ static const float DP_TAB[8][7] = {   // [phase][j]: input = y + h * sum_j TAB[phase][j] k_j ; last column: time fraction
    {0, 0, 0, 0, 0, 0, 0.f},
    {1, 0, 0, 0, 0, 0, 1.f},
    {1.f / 5, 0, 0, 0, 0, 0, 1.f / 5},
    {3.f / 40, 9.f / 40, 0, 0, 0, 0, 3.f / 10},
    {44.f / 45, -56.f / 15, 32.f / 9, 0, 0, 0, 4.f / 5},
    {19372.f / 6561, -25360.f / 2187, 64448.f / 6561, -212.f / 729, 0, 0, 8.f / 9},
    {9017.f / 3168, -355.f / 33, 46732.f / 5247, 49.f / 176, -5103.f / 18656, 0, 1.f},
    {35.f / 384, 0, 500.f / 1113, 125.f / 192, -2187.f / 6784, 11.f / 84, 1.f}};
// error weights (5th minus 4th order) and midpoint weights of the dense output
__device__ static const float DP_E[7] = {(float)(35.0 / 384 - 1951.0 / 21600), 0.f, (float)(500.0 / 1113 - 22642.0 / 50085),
                                         (float)(125.0 / 192 - 451.0 / 720), (float)(-2187.0 / 6784 + 12231.0 / 42400),
                                         (float)(11.0 / 84 - 649.0 / 6300), (float)(-1.0 / 60)};
__device__ static const float DP_M[7] = {(float)(6025192743.0 / 30085553152.0 / 2), 0.f, (float)(51252292925.0 / 65400821598.0 / 2),
                                         (float)(-2691868925.0 / 45128329728.0 / 2), (float)(187940372067.0 / 1594534317056.0 / 2),
                                         (float)(-1776094331.0 / 19743644256.0 / 2), (float)(11237099.0 / 235043384.0 / 2)};

// initial step, part 1: d0 = ||y0 / sc||, d1 = ||f0 / sc|| (RMS norms)
__device__ __forceinline__ float dp_h0(float d0, float d1) { return (d0 < 1e-5f || d1 < 1e-5f) ? 1e-6f : 0.01f * d0 / d1; }

// initial step, part 2: d2 = ||(f1 - f0) / sc|| / h0, f1 the field at y0 + h0 f0
__device__ __forceinline__ float dp_dt0(float h0, float d1, float d2) {
  const float h1 = (d1 <= 1e-15f && d2 <= 1e-15f) ? fmaxf(1e-6f, h0 * 1e-3f) : powf(0.01f / fmaxf(d1, d2), 0.2f);
  return fminf(100.f * h0, h1);
}

// the step proposed after an attempt of size dt with error ratio `ratio` (accepted when ratio <= 1): dt clip(0.9 ratio^-1/5, dfactor,
// 10).  HW_POW: ratio^(-1/5) through the hardware's log2 / exp2 (1 ulp each; ratio is a non-negative finite number or NaN here) -- the
// library's powf spends ~150 dependent instructions on cases this call cannot meet, which the row leaders of ode_fast.hip run on ONE
// wave while the other waves wait at the barrier.  The two forms round differently, so each family keeps the one it has.
template <bool HW_POW = false>
__device__ __forceinline__ float dp_next_dt(float ratio, float dt) {
  const float dfac = ratio < 1.f ? 1.f : 0.2f;
  const float p = HW_POW ? __builtin_amdgcn_exp2f(-0.2f * __builtin_amdgcn_logf(ratio)) : powf(ratio, -0.2f);
  const float fac = fminf(10.f, fmaxf(0.9f * p, dfac));
  return fmaxf(ratio == 0.f ? dt * 10.f : dt * fac, 0.f);
}

// Replay hooks (mfm_debug_replay; `Replay` in ode.hip, `WReplay` in wide.hip).  o0: the row's slot of attempt 0 in the replay arrays;
// writer: this lane records (one lane per row).  At the initial step: record the controller's dt, return the prescribed one.
template <class R>
__device__ __forceinline__ float dp_replay_dt0(const R& rp, size_t o0, bool writer, float dt) {
  if (writer) rp.dt_own[o0] = dt;
  return rp.dt[o0];
}

// At the end of attempt j: record its error ratio and the step the controller proposed (ndt), then take the prescribed accept
// decision and next step (past the end of the arrays: reject, step 0 -- the solve stops).
template <class R>
__device__ __forceinline__ void dp_replay_attempt(const R& rp, size_t o0, bool writer, int j, float ratio, bool& acc, float& ndt) {
  const bool in = j < rp.cap, nx = j + 1 < rp.cap;
  const size_t o = o0 + (in ? j : 0);
  if (writer && in) { rp.ratio[o] = ratio; if (nx) rp.dt_own[o + 1] = ndt; }
  acc = in && rp.acc[o] != 0;
  ndt = nx ? rp.dt[o + 1] : 0.f;
}

// 4th-order dense output of a step x0 -> x1 of size h at abscissa sfrac in [0, 1]: xm = x0 + h sum_j DP_M[j] k_j, g0 = h k_1, g1 = h k_7.
// T: float or f32x4.
template <class T>
__device__ __forceinline__ T dp_dense(T x0, T x1, T xm, T g0, T g1, float sfrac) {
  const T qa = -2.f * g0 + 2.f * g1 - 8.f * x0 - 8.f * x1 + 16.f * xm;
  const T qb = 5.f * g0 - 3.f * g1 + 18.f * x0 + 14.f * x1 - 32.f * xm;
  const T qc = -4.f * g0 + g1 - 11.f * x0 - 5.f * x1 + 16.f * xm;
  return (((qa * sfrac + qb) * sfrac + qc) * sfrac + g0) * sfrac + x0;
}
