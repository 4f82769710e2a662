// The MALA step of bblackjax (mala.py:86-118, diffusions.py:19-34, proposal.py:104-112,157-159,178-186) and the accept rule HMC shares
// with it, per element and per chain, independent of layout, for every sampler kernel (mala.hip, mala_run.hip, lgcp.hip, hmc.hip,
// wide.hip's propose / accept pair; each keeps its layout, reductions, writing lane and source of draws).  Each expression is written
// once, operand order and rounding included: FMA = false, the STRICT form, rounds every operation on its own
// (mala_chain_step, mala_run_kernel, hmc_step_kernel); FMA = true, the FUSED form, writes out the multiply-adds that mala_lgcp_kernel,
// lgcp_propose_kernel and lgcp_accept_kernel make.  The two differ in the last bit; no helper leaves the choice to the compiler.
// The acceptance rule is AS WRITTEN (p = min(1, exp(prev_E - new_E)), the inverse of the textbook ratio); `textbook` flips it.
#pragma once
#include "prng.hip.h"
#include "targets.hip.h"
// a step's chain key: the caller's own (smc/base.py:122-123) or split(key, n_total)[chain] (exe_flow_matching.py:303); halves: mala.py:93
__device__ __forceinline__ Key2 mcmc_chain_key(Key2 key, const uint32_t* keys, uint32_t n_total, uint32_t chain_offset, int b) {
  return keys ? Key2{keys[2 * b], keys[2 * b + 1]} : split_at(key, n_total, chain_offset + (uint32_t)b);
}
enum { MCMC_K_INT = 0, MCMC_K_RMH = 1 };
__device__ __forceinline__ Key2 mcmc_step_key(Key2 kb, uint32_t half) { return split_at(kb, 2, half); }
// step s of a run (mfm_mala_run): key_mode 0, step-major (mcmc_utils.py:11-25); 1, chain-major (tempered.py:37-39)
__device__ __forceinline__ Key2 mcmc_run_key(int key_mode, Key2 key, Key2 chain_key, uint32_t n_steps, uint32_t s, uint32_t n_total, uint32_t chain) {
  return key_mode ? split_at(chain_key, n_steps, s) : split_at(split_at(key, n_steps, s), n_total, chain);
}
__device__ __forceinline__ double mala_s2e(double eps) { return sqrt(2.0 * eps); }
// proposal element x' = x + eps g + sqrt(2 eps) n (diffusions.py:25-30; n: util.py:80-82); th1 += |x' - x - eps g|^2 = 2 eps n^2
template <bool FMA> __device__ __forceinline__ float mala_propose(float x, float g, double n, double eps, double s2e, double& th1) {
#pragma clang fp contract(off)
  const double th = s2e * n;
  th1 = FMA ? fma(th, th, th1) : th1 + th * th;
  return (float)(FMA ? fma(s2e, n, fma(eps, (double)g, (double)x)) : (double)x + eps * (double)g + th);      // (fused: s2e n is not rounded first)
}
// back term: th2 += |x - x' - eps g'|^2, g' the gradient at the proposal (diffusions.py:32)
template <bool FMA> __device__ __forceinline__ void mala_back(float x, float xn, float gn, double eps, double& th2) {
#pragma clang fp contract(off)
  const double t = FMA ? fma(-eps, (double)gn, (double)x - (double)xn) : (double)x - (double)xn - eps * (double)gn;
  th2 = FMA ? fma(t, t, th2) : th2 + t * t;
}
struct McmcExp { __device__ __forceinline__ double operator()(double v) const { return exp(v); } };
// the rule's tail (HMC enters with H_0 - H_end): NaN rejects (proposal.py:105), p = min(1, exp(delta)) (:178), accept when u < p (:179)
template <class Exp = McmcExp> __device__ __forceinline__ double mala_accept_p(double delta, Exp ex = Exp()) {
  if (isnan(delta)) delta = -INFINITY;
  return fmin(ex(delta), 1.0);
}
// acceptance probability of a proposal with log-density lpn from a state with log-density lp; th1, th2: the reduced squared norms
template <bool FMA, class Exp = McmcExp> __device__ __forceinline__ double mala_accept_p(double lp, double lpn, double th1, double th2, double eps, int textbook, Exp ex = Exp()) {
#pragma clang fp contract(off)
  const double inv4e = 0.25 / eps;
  const double new_E = FMA ? fma(inv4e, th1, -lp) : -lp + inv4e * th1;      // mala.py:68-79, proposal.py:157
  const double prev_E = FMA ? fma(inv4e, th2, -lpn) : -lpn + inv4e * th2;   // proposal.py:158
  double delta = prev_E - new_E;                                            // proposal.py:104
  if (textbook) delta = -delta;
  return mala_accept_p(delta, ex);
}
// the proposal's weight (mala.py:104-113, a diagnostic); no kernel fuses this one
template <class Exp = McmcExp> __device__ __forceinline__ double mala_prop_weight(double lpn, double th2, double eps, Exp ex = Exp()) {
#pragma clang fp contract(off)
  return ex(lpn + 0.25 / eps * th2);
}
// The Cox process element (distributions.py:231-314), fused form only.  ex = expf(xv), y = (K^-1 (x - mu))[col]; gradient beta (c - a e^x) - y:
__device__ __forceinline__ float cox_grad(const TargetDev& T, double beta, int col, float ex, float y) {
#pragma clang fp contract(off)
  return fmaf((float)beta, fmaf(-T.poisson_a, ex, T.counts[col]), -y);
}
// likelihood term x c - a e^x (cox_process_utils.py:113-115) and quadratic-form term (x - mu) y (distributions.py:299-303)
__device__ __forceinline__ void cox_terms(const TargetDev& T, int col, float xv, float ex, float y, double& lik, double& quad) {
#pragma clang fp contract(off)
  lik += fma((double)xv, (double)T.counts[col], -((double)T.poisson_a * (double)ex));
  quad = fma((double)(xv - T.mu), (double)y, quad);
}
// log-density from the reduced sums: beta loglik - 1/2 quad + log_norm
__device__ __forceinline__ double cox_logp(const TargetDev& T, double beta, double lik, double quad) {
#pragma clang fp contract(off)
  return fma(beta, lik, -0.5 * quad) + (double)T.log_norm;
}
// Step-size warmup (warmup.hip; include/mfm.h states the recursion): Nesterov dual averaging of a chain's log step size x towards the
// acceptance probability `target`, with Hoffman & Gelman's constants t0 = 10, gamma = 0.05, kappa = 0.75.  mu = log(10 step0), x0 = log step0;
// a chain starts from x = x0, hbar = 0, xbar = 0.  Wave-uniform float64, every operation rounded on its own; m^-kappa is 1 / (sqrt(m) sqrt(sqrt(m))),
// two correctly rounded square roots, so that a host restatement makes the same numbers.
struct DualAvg {
  double mu, x0;            // the shrinkage point, and the centre of the clamp [x0 - 23, x0 + 23] that keeps exp(x) finite and positive
  double x, hbar, xbar;     // the iterate x_m, the averaged error H_m, the averaged iterate
};
// step m = 1, 2, ... has run at exp(s.x) with acceptance probability p: the next iterate and the running average
__device__ __forceinline__ void dual_avg_update(DualAvg& s, int m, double p, double target) {
#pragma clang fp contract(off)
  const double mt = (double)m + 10.0;
  s.hbar = (1.0 - 1.0 / mt) * s.hbar + (target - p) / mt;
  const double rm = sqrt((double)m);
  const double x = s.mu - rm / 0.05 * s.hbar;
  s.x = fmin(fmax(x, s.x0 - 23.0), s.x0 + 23.0);
  const double eta = 1.0 / (rm * sqrt(rm));
  s.xbar = eta * s.x + (1.0 - eta) * s.xbar;
}
