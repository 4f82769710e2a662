"""ChEES-HMC warmup restated in float64 numpy: the definition ``mfm_chees_warmup`` (mfm_amd/csrc/chees.hip, include/mfm.h) is held to.
A helper of tests/test_chees_ref.py, tests/test_chees_cases.py and tests/test_gpu_chees.py, not a test.

Nothing here is copied from blackjax's ``chees_adaptation`` (its file is not at hand): the lines follow Hoffman, Radul & Sountsov,
"An Adaptive MCMC Scheme for Setting Trajectory Lengths in Hamiltonian Monte Carlo" (AISTATS 2021), Algorithm 1 and section 3, and
blackjax's structure as remembered; each line says which.

* jitter (paper section 3.3; blackjax uses a Halton sequence): ``h_t`` the base-2 radical inverse of ``t``, ``tau_t = h_t T_t``,
  ``L_t = min(max_leapfrog, max(1, ceil(tau_t / eps_t)))`` (blackjax: ``ceil(trajectory_length / step_size)``, clipped);
* the step: ``oracle.hmc.kernel`` / ``tests.hmc_mass_ref.kernel`` line for line (the project's HMC step), which also keeps the end point,
  the end velocity ``minv p'`` and ``alpha = min(1, exp(H_0 - H_end))``; ``div = not (H_end - H_0 < threshold)`` (blackjax's
  ``is_divergent``; a NaN is divergent);
* the statistic (paper eq. 8 - 10, Algorithm 1; blackjax weighs by ``alpha`` and leaves out divergent chains):
  ``g_k = tau_t (|x'_k - xbar'|^2 - |x_k - xbar|^2) <x'_k - xbar', v'_k>``, ``ghat = sum alpha_k g_k / sum (alpha_k + 1e-20)``,
  ``hm = n / sum (1 / alpha_k)`` (the paper steers the step size by the harmonic mean of the acceptance probabilities);
* the step size: the project's dual averaging (include/mfm.h, ``mfm_hmc_warmup``) with ``p := hm``;
* the trajectory length: Adam (Kingma & Ba, bias-corrected; b1 0.9, b2 0.999, epsilon 1e-8) ASCENDING ``log T`` along ``ghat`` (paper
  Algorithm 1; blackjax hands ``-ghat`` to an optax optimizer); a non-finite ``ghat`` is skipped (blackjax: ``jnp.where(isfinite)``);
  ``log T`` clamped to ``[log eps, log eps + log max_leapfrog]`` with the NEW step size; ``ma = decay ma + (1 - decay) log T`` (paper:
  the iterates' average in log space is what is sampled with).

``float32_positions=True`` rounds the trajectory's position to float32 after every drift, as the kernel holds it."""
from collections import namedtuple

import numpy as np

from oracle import prng

ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.999, 1e-8
TRACE_FIELDS = ("eps", "T", "L", "hm", "ghat", "n_div", "mean_alpha")


def radical_inverse(t):
    """Base-2 radical inverse of ``t >= 1``: 1/2, 1/4, 3/4, 1/8, ...; exact in float64, never 0."""
    t, h, f = int(t), 0.0, 0.5
    while t:
        if t & 1:
            h += f
        t >>= 1
        f *= 0.5
    return h


def num_leapfrog(tau, eps, max_leapfrog):
    n = np.ceil(tau / eps)
    return 1 if not n >= 1.0 else int(min(n, max_leapfrog))


class DualAveraging:
    """include/mfm.h's recursion for ONE step size (t0 = 10, gamma = 0.05, kappa = 0.75, mu = log(10 step0), clamp +-23)."""

    def __init__(self, step0):
        self.x0 = np.log(step0)
        self.mu = np.log(10.0 * step0)
        self.x, self.hbar, self.xbar = self.x0, 0.0, 0.0

    def update(self, m, p, target):
        mt = m + 10.0
        self.hbar = (1.0 - 1.0 / mt) * self.hbar + (target - p) / mt
        rm = np.sqrt(float(m))
        x = self.mu - rm / 0.05 * self.hbar
        self.x = min(max(x, self.x0 - 23.0), self.x0 + 23.0)
        eta = 1.0 / (rm * np.sqrt(rm))
        self.xbar = eta * self.x + (1.0 - eta) * self.xbar


class Recursion:
    """Everything between two steps: ``eps_t, T_t, L_t`` of the iteration about to run and the optimizers' state."""

    def __init__(self, eps1, T1, learning_rate=0.025, max_leapfrog=1000, decay=0.5, target=0.651):
        self.lr, self.max_leapfrog, self.decay, self.target = float(learning_rate), int(max_leapfrog), float(decay), float(target)
        self.eps, self.T, self.t = float(eps1), float(T1), 1
        self.logT = np.log(self.T)
        self.ma = self.logT
        self.m, self.v, self.b1t, self.b2t = 0.0, 0.0, 1.0, 1.0
        self.da = DualAveraging(self.eps)
        self.L = num_leapfrog(self.tau, self.eps, self.max_leapfrog)

    @property
    def tau(self):
        return radical_inverse(self.t) * self.T

    def advance(self, hm, ghat):
        """After iteration ``t`` with the pooled ``hm`` and ``ghat``: ``eps_{t+1}, T_{t+1}, L_{t+1}``."""
        self.da.update(self.t, hm, self.target)
        eps = np.exp(self.da.x)
        if np.isfinite(ghat):
            self.m = ADAM_B1 * self.m + (1.0 - ADAM_B1) * ghat
            self.v = ADAM_B2 * self.v + (1.0 - ADAM_B2) * (ghat * ghat)
            self.b1t, self.b2t = self.b1t * ADAM_B1, self.b2t * ADAM_B2
            mhat, vhat = self.m / (1.0 - self.b1t), self.v / (1.0 - self.b2t)
            self.logT = self.logT + self.lr * (mhat / (np.sqrt(vhat) + ADAM_EPS))
        self.logT = min(max(self.logT, self.da.x), self.da.x + np.log(float(self.max_leapfrog)))
        self.ma = self.decay * self.ma + (1.0 - self.decay) * self.logT
        self.eps, self.T, self.t = float(eps), float(np.exp(self.logT)), self.t + 1
        self.L = num_leapfrog(self.tau, self.eps, self.max_leapfrog)

    @property
    def results(self):
        """``(step_size, trajectory_length, last eps, last T)``."""
        return (float(np.exp(self.da.xbar)), float(np.exp(self.ma)), self.eps, self.T)


StepRecord = namedtuple("StepRecord", "x prop vel alpha div u energy_change accepted")
State = namedtuple("State", "position logdensity logdensity_grad")


def hmc_step(keys, state, value_and_grad, eps, L, inverse_mass=None, divergence_threshold=1000.0, float32_positions=False):
    """One HMC step of every chain on ``keys [B, 2]`` with its record."""
    x, logp, g = state
    B, d = x.shape
    minv = np.ones(d) if inverse_mass is None else np.asarray(inverse_mass, dtype=np.float64)
    kk = prng.split_rows(keys, 2)
    p = prng.normal_rows(kk[:, 0], d) / np.sqrt(minv)
    h0 = -logp + 0.5 * (minv * p * p).sum(1)
    xn, pn, lpn, gn = x, p, logp, g
    with np.errstate(all="ignore"):
        for _ in range(int(L)):
            pn = pn + 0.5 * eps * gn
            xn = xn + eps * (minv * pn)
            if float32_positions:
                xn = xn.astype(np.float32).astype(np.float64)
            lpn, gn = value_and_grad(xn)
            pn = pn + 0.5 * eps * gn
        h1 = -lpn + 0.5 * (minv * pn * pn).sum(1)
        dh = h1 - h0
        div = ~(dh < divergence_threshold)
        delta = np.where(np.isnan(h0 - h1), -np.inf, h0 - h1)
        alpha = np.minimum(np.exp(delta), 1.0)
    u = prng.uniform_rows(kk[:, 1])
    acc = u < alpha
    m = acc[:, None]
    new = State(np.where(m, xn, x), np.where(acc, lpn, logp), np.where(m, gn, g))
    return new, StepRecord(x, xn, minv * pn, alpha, div, u, dh, acc)


def statistic(x, prop, vel, alpha, div, tau, n_valid=None):
    """``(ghat, hm, number of divergent chains, mean alpha)`` over the first ``n_valid`` chains."""
    n = x.shape[0] if n_valid is None else int(n_valid)
    x, prop, vel, alpha, div = (np.asarray(a)[:n] for a in (x, prop, vel, alpha, div))
    x, prop, alpha = x.astype(np.float64), prop.astype(np.float64), alpha.astype(np.float64)
    ok = ~div.astype(bool)
    with np.errstate(all="ignore"):
        dx0 = x - x.mean(0)
        dx1 = prop - prop.mean(0)
        g = tau * ((dx1 * dx1).sum(1) - (dx0 * dx0).sum(1)) * (dx1 * vel).sum(1)
        if not ok.any():
            return 0.0, 0.0, n, float(alpha.mean())
        a = alpha[ok]
        ghat = (a * g[ok]).sum() / (a + 1e-20).sum()
        hm = ok.sum() / (1.0 / a).sum()
    return float(ghat), float(hm), int(n - ok.sum()), float(alpha.mean())


def step_keys(key, key_mode, n_iter, t, n_chain):
    """The keys of iteration ``t`` (from 1): ``mfm_hmc_run``'s for step ``t - 1`` of a run of ``n_iter`` steps."""
    if key_mode:
        return prng.split_rows(np.asarray(key), n_iter)[:, t - 1]
    return prng.split(prng.split(key, n_iter)[t - 1], n_chain)


def chees_warmup(key, state, value_and_grad, eps1, n_iter, T1=None, n_valid=None, key_mode=0, inverse_mass=None, target_accept=0.651,
                 learning_rate=0.025, max_leapfrog=1000, decay=0.5, divergence_threshold=1000.0, float32_positions=False):
    """``dict(state, results, trace [n_iter, 7], records)``: the trace's columns are ``TRACE_FIELDS``, ``records`` one ``StepRecord`` per
    iteration."""
    B = state.position.shape[0]
    rs = Recursion(eps1, eps1 if T1 is None else T1, learning_rate, max_leapfrog, decay, target_accept)
    trace, records = [], []
    for t in range(1, int(n_iter) + 1):
        eps, T, L, tau = rs.eps, rs.T, rs.L, rs.tau
        state, rec = hmc_step(step_keys(key, key_mode, n_iter, t, B), state, value_and_grad, eps, L, inverse_mass, divergence_threshold,
                              float32_positions)
        ghat, hm, n_div, mean_alpha = statistic(rec.x, rec.prop, rec.vel, rec.alpha, rec.div, tau, n_valid)
        trace.append((eps, T, float(L), hm, ghat, float(n_div), mean_alpha))
        records.append(rec)
        rs.advance(hm, ghat)
    return dict(state=state, results=rs.results, trace=np.array(trace), records=records)
