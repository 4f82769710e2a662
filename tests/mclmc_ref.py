"""Microcanonical Langevin Monte Carlo (MCLMC: Robnik, De Luca, Silverstein & Seljak 2023; Robnik & Seljak 2024; ``blackjax.mclmc``)
restated in float64 numpy, batched over chains: the yardstick of ``mfm_mclmc_*`` (mfm_amd/csrc/mclmc.hip) and of
``mclmc_find_L_and_step_size`` (mfm_amd/bblackjax/adaptation/mclmc_adaptation.py).

A chain is a position ``x [d]``, a UNIT momentum ``u [d]``, ``logp`` and ``g = grad log p(x)`` of the tempered density; d >= 2.

``B(h)`` at the gradient g, the exact flow of du/dt = (I - u u^T) g / (d - 1): n = g / |g|, c = u.n, delta = h |g| / (d - 1),
zeta = exp(-delta); u <- r / |r| with r = n (1 - zeta)(1 + zeta + c (1 - zeta)) + 2 zeta u; the kinetic change is
dK = (d - 1) (delta - ln 2 + ln(1 + c + (1 - c) zeta^2)) = (d - 1) ln(cosh delta + c sinh delta); |g| = 0 leaves u and dK = 0.  c is
clamped to [-1, 1]: rounding can leave it by an ulp, and at d = 2 (u = -n) the logarithm's argument would go negative.
``A(h)``: x <- x + h u.  One step of size eps: B(b_0 eps), then for k = 1 .. K: A(a_k eps), (logp, g) = value_and_grad(x), B(b_k eps);
``SCHEDULES`` holds leapfrog (K = 1) and McLachlan's minimal-norm scheme (K = 2, blackjax's default).  The energy change of the step is
dE = sum dK - (logp_end - logp_start).  Then the partial refresh u <- (u + nu z) / |u + nu z|, nu = sqrt((exp(2 eps / L) - 1) / d),
z_j = normal64(split(kb, 2)[0], j, d) with kb the step's chain key; L = inf gives nu = 0 exactly and draws nothing.  No accept test."""
from typing import NamedTuple

import numpy as np

from oracle import prng

B1 = 0.1931833275037836
# integrator: (b_0 .. b_K, a_1 .. a_K)
SCHEDULES = {0: ((0.5, 0.5), (1.0,)), 1: ((B1, 1.0 - 2.0 * B1, B1), (0.5, 0.5))}
INTEGRATORS = {"leapfrog": 0, "mclachlan": 1}
LN2 = 0.6931471805599453


class State(NamedTuple):
    position: np.ndarray
    momentum: np.ndarray
    logdensity: np.ndarray
    logdensity_grad: np.ndarray


class Info(NamedTuple):
    logdensity: np.ndarray
    kinetic_change: np.ndarray
    energy_change: np.ndarray


def init_momentum(key, n_total, d, offset=0, n=None):
    """u_b = z / |z|, z_j = normal64(split(key, n_total)[offset + b], j, d)."""
    n = n_total - offset if n is None else n
    z = prng.normal_rows(prng.split(key, n_total)[offset:offset + n], d)
    return z / np.sqrt((z * z).sum(1))[:, None]


def init(position, value_and_grad, key, n_total=None, offset=0):
    x = np.asarray(position, np.float64)
    lp, g = value_and_grad(x)
    return State(x, init_momentum(key, n_total or x.shape[0], x.shape[1], offset, x.shape[0]), lp, g)


def momentum_update(u, g, h):
    """B(h): (new u, dK)."""
    d = u.shape[1]
    gn = np.sqrt((g * g).sum(1))
    flat = gn == 0.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ginv = np.where(flat, 0.0, 1.0 / gn)
        n = g * ginv[:, None]
        c = np.clip((u * n).sum(1), -1.0, 1.0)
        delta = h * gn / (d - 1)
        zeta = np.exp(-delta)
        omz = 1.0 - zeta
        r = n * (omz * (1.0 + zeta + c * omz))[:, None] + (2.0 * zeta)[:, None] * u
        r = r * np.where(flat, 0.5, 1.0 / np.sqrt((r * r).sum(1)))[:, None]      # (|g| = 0: r = 2 u, and u comes back bit for bit)
        dk = (d - 1) * (delta - LN2 + np.log(1.0 + c + (1.0 - c) * (zeta * zeta)))
    return r, np.where(flat, 0.0, dk)


def momentum_closed_form(u, g, h):
    """The same flow written with hyperbolic functions: u + n (sinh delta + c (cosh delta - 1)), normalised, and
    dK = (d - 1) ln(cosh delta + c sinh delta)."""
    d = u.shape[1]
    gn = np.sqrt((g * g).sum(1))
    n = g / gn[:, None]
    c = (u * n).sum(1)
    delta = h * gn / (d - 1)
    r = u + n * (np.sinh(delta) + c * (np.cosh(delta) - 1.0))[:, None]
    return r / np.sqrt((r * r).sum(1))[:, None], (d - 1) * np.log(np.cosh(delta) + c * np.sinh(delta))


def refresh_scale(eps, L, d):
    return float(np.sqrt((np.exp(2.0 * eps / L) - 1.0) / d))


def refresh(u, keys, nu):
    if nu == 0.0:
        return u
    z = prng.normal_rows(prng.split_rows(keys, 2)[:, 0], u.shape[1])
    w = u + nu * z
    return w * (1.0 / np.sqrt((w * w).sum(1)))[:, None]


def step(keys, state, value_and_grad, eps, L, integrator=1, round_position=None):
    """One step of every chain on its own key ``keys [n, 2]``: (new state, Info).  ``round_position`` (e.g. a float32 round trip) is
    applied after every A: it is how ``step_f32`` in tests/mclmc_cases.py states the device's number formats."""
    b, a = SCHEDULES[INTEGRATORS.get(integrator, integrator)]
    x, u, lp0, g = state
    d = x.shape[1]
    u, dk = momentum_update(u, g, b[0] * eps)
    lp = lp0
    for k in range(len(a)):
        x = x + (a[k] * eps) * u
        if round_position is not None:
            x = round_position(x)
        lp, g = value_and_grad(x)
        u, dkk = momentum_update(u, g, b[k + 1] * eps)
        dk = dk + dkk
    de = dk - (lp - lp0)
    u = refresh(u, keys, refresh_scale(eps, L, d))
    return State(x, u, lp, g), Info(lp, dk, de)


def chain_keys(key, n_total, offset=0, n=None):
    """The per-chain keys ``mfm_mclmc_step`` derives from one key."""
    n = n_total - offset if n is None else n
    return prng.split(key, n_total)[offset:offset + n]


class RunInfo(NamedTuple):
    energy_change_sum: np.ndarray
    energy_change_sumsq: np.ndarray
    num_nonfinite: np.ndarray
    energy_var_per_dim: float
    positions: object
    logdensities: object


def energy_var_per_dim(de_sum, de_sumsq, count, d):
    """The pooled variance of dE over chains and steps, per dimension, from the three sums."""
    m = de_sum / count
    return (de_sumsq / count - m * m) / d


def run(key, state, value_and_grad, eps, L, integrator, num_steps, thin=0):
    """``num_steps`` steps, step j on ``split(split(key, num_steps)[j], n)`` (key_mode 0 of ``mfm_mclmc_run``)."""
    n, d = state.position.shape
    s1, s2, bad = np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
    xs, lps = [], []
    for j, kj in enumerate(prng.split(key, num_steps)):
        state, info = step(prng.split(kj, n), state, value_and_grad, eps, L, integrator)
        de = info.energy_change
        s1, s2, bad = s1 + de, s2 + de * de, bad + ~np.isfinite(de)
        if thin > 0 and (j + 1) % thin == 0:
            xs.append(state.position); lps.append(state.logdensity)
    v = energy_var_per_dim(s1.sum(), s2.sum(), n * num_steps, d)
    return state, RunInfo(s1, s2, bad, float(v), np.stack(xs) if xs else None, np.stack(lps) if lps else None)


class RefAlgorithm:
    """What ``mclmc_find_L_and_step_size`` needs of an algorithm, on this restatement: ``.run(key, state, num_steps, thin)`` returning
    a state and an info with the run's sums, ``num_nonfinite`` and ``positions`` (numpy in place of device tensors)."""

    def __init__(self, value_and_grad, L, step_size, integrator):
        self.vg, self.L, self.step_size, self.integrator = value_and_grad, L, step_size, integrator

    def run(self, key, state, num_steps, thin=0):
        return run(key, state, self.vg, self.step_size, self.L, self.integrator, num_steps, thin)
