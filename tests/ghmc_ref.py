"""Generalized HMC with persistent momentum (Horowitz 1991) and the non-reversible slice accept, as Hoffman & Sountsov 2022 (MEADS) run
it (``blackjax.ghmc``), restated in float64 numpy, batched over chains: the yardstick of ``mfm_ghmc_*`` (mfm_amd/csrc/ghmc.hip).

A chain is a position ``x [d]``, a momentum ``p [d]``, ``logp`` and ``g = grad log p(x)`` of the tempered density, and a slice variable
``s`` in (-1, 1).  Parameters: step size ``eps > 0``, refresh rate ``alpha`` in (0, 1], slice drift ``delta >= 0``, the diagonal inverse
mass ``minv [d]`` (``None``: unit metric).  One transition with the chain key ``kb``:

1. ``p <- sqrt(1 - alpha) p + sqrt(alpha) n / sqrt(minv)``, ``n_j = normal64(split(kb, 2)[0], j, d)`` (oracle/hmc.py's momentum draw)
2. ``s <- fmod(s + 1 + delta, 2) - 1``
3. ``H_0 = -logp + 1/2 sum minv p^2``
4. one velocity-Verlet step: ``p += eps/2 g; x += eps minv p; (logp, g) = value_and_grad(x); p += eps/2 g``
5. ``H_1`` likewise, ``dH = H_1 - H_0``
6. accept iff ``|s| <= exp(-dH)``, a NaN ``dH`` rejecting.  Accepted: the end point, ``p <- p_end``, ``s <- s exp(dH)``.  Rejected: x,
   logp, g kept, ``p <- -p`` (the refreshed momentum, negated), s kept.
7. info: ``acceptance_rate = min(1, exp(-dH))``, ``is_accepted``, ``energy_change = dH``.

Every product with ``minv`` is written so that ``minv == 1`` gives the unit form's bits.  ``float32_positions=True`` states the device's
number formats: the position rounded to float32 after the drift (it is what the target is evaluated at) -- the caller passes a
``value_and_grad`` that evaluates the gradient in float32 arithmetic if it wants that too."""
from typing import NamedTuple

import numpy as np

from oracle import prng


class State(NamedTuple):
    position: np.ndarray
    momentum: np.ndarray
    logdensity: np.ndarray
    logdensity_grad: np.ndarray
    slice: np.ndarray


class Info(NamedTuple):
    acceptance_rate: np.ndarray
    is_accepted: np.ndarray
    energy_change: np.ndarray
    proposed_position: np.ndarray
    slice_after_drift: np.ndarray      # |this| against exp(-dH) is the decision


def chain_keys(key, n_total, offset=0, n=None):
    """The per-chain keys ``mfm_ghmc_step`` / ``mfm_ghmc_init`` derive from one key."""
    n = n_total - offset if n is None else n
    return prng.split(key, n_total)[offset:offset + n]


def init_momentum_slice(key, n_total, d, minv=None, offset=0, n=None):
    """``mfm_ghmc_init``: ``p = n / sqrt(minv)`` and ``s = 2 uniform - 1`` from the two halves of chain b's key."""
    kk = prng.split_rows(chain_keys(key, n_total, offset, n), 2)
    p = prng.normal_rows(kk[:, 0], d)
    if minv is not None:
        p = p / np.sqrt(np.asarray(minv, np.float64))[None]
    return p, 2.0 * prng.uniform_rows(kk[:, 1]) - 1.0


def init(position, value_and_grad, key, minv=None, n_total=None, offset=0):
    x = np.asarray(position, np.float64)
    lp, g = value_and_grad(x)
    p, s = init_momentum_slice(key, n_total or x.shape[0], x.shape[1], minv, offset, x.shape[0])
    return State(x, p, lp, g, s)


def refresh(p, keys, alpha, minv=None):
    """Step 1."""
    n = prng.normal_rows(prng.split_rows(keys, 2)[:, 0], p.shape[1])
    ca, sa = np.sqrt(1.0 - alpha), np.sqrt(alpha)
    if minv is None:
        return ca * p + sa * n
    return ca * p + sa * n / np.sqrt(minv)[None]


def slice_drift(s, delta):
    """Step 2."""
    return np.fmod(s + 1.0 + delta, 2.0) - 1.0


def step(keys, state, value_and_grad, eps, alpha, delta=None, minv=None, float32_positions=False):
    """One transition of every chain on its own key ``keys [n, 2]``: (new state, Info).  ``alpha`` / ``delta`` / ``eps`` may be per-chain
    arrays ``[n]`` and ``minv`` ``[n, d]`` (MEADS gives each fold its own)."""
    x, p, lp0, g, s = state
    delta = alpha / 2.0 if delta is None else delta
    m = None if minv is None else np.asarray(minv, np.float64)
    col = (lambda v: np.asarray(v, np.float64)[:, None]) if np.ndim(eps) else (lambda v: v)
    n = prng.normal_rows(prng.split_rows(keys, 2)[:, 0], x.shape[1])
    ca, sa = np.sqrt(1.0 - np.asarray(alpha, np.float64)), np.sqrt(np.asarray(alpha, np.float64))
    if np.ndim(alpha):
        ca, sa = ca[:, None], sa[:, None]
    if m is None:
        pr = ca * p + sa * n
        h0 = -lp0 + 0.5 * (pr * pr).sum(1)
    else:
        m = m if m.ndim == 2 else m[None]
        pr = ca * p + sa * n / np.sqrt(m)
        h0 = -lp0 + 0.5 * (m * pr * pr).sum(1)
    sd = slice_drift(s, delta)
    e = col(eps)
    pe = pr + 0.5 * e * g
    xe = x + e * pe if m is None else x + e * (m * pe)
    if float32_positions:
        xe = xe.astype(np.float32).astype(np.float64)
    lpe, ge = value_and_grad(xe)
    pe = pe + 0.5 * e * ge
    h1 = -lpe + 0.5 * ((pe * pe).sum(1) if m is None else (m * pe * pe).sum(1))
    de = h1 - h0
    with np.errstate(over="ignore", invalid="ignore"):
        neg = np.where(np.isnan(de), -np.inf, h0 - h1)
        rate = np.minimum(np.exp(neg), 1.0)
        acc = ~np.isnan(de) & (np.abs(sd) <= rate)
        s_new = np.where(acc, sd * np.exp(de), sd)
    a = acc[:, None]
    new = State(np.where(a, xe, x), np.where(a, pe, -pr), np.where(acc, lpe, lp0), np.where(a, ge, g), s_new)
    return new, Info(rate, acc, de, xe, sd)


class RunInfo(NamedTuple):
    num_accepted: np.ndarray
    acceptance_rate_sum: np.ndarray
    energy_change_sum: np.ndarray      # over the accepted steps
    positions: object
    logdensities: object


def run(key, state, value_and_grad, eps, alpha, delta, num_steps, minv=None, thin=0):
    """``num_steps`` transitions, step j on ``split(split(key, num_steps)[j], n)`` (key_mode 0 of ``mfm_ghmc_run``)."""
    n = state.position.shape[0]
    n_acc, acc_sum, de_sum = np.zeros(n, np.int64), np.zeros(n), np.zeros(n)
    xs, lps = [], []
    for j, kj in enumerate(prng.split(key, num_steps)):
        state, info = step(prng.split(kj, n), state, value_and_grad, eps, alpha, delta, minv)
        n_acc, acc_sum = n_acc + info.is_accepted, acc_sum + info.acceptance_rate
        de_sum = np.where(info.is_accepted, de_sum + info.energy_change, de_sum)
        if thin > 0 and (j + 1) % thin == 0:
            xs.append(state.position); lps.append(state.logdensity)
    return state, RunInfo(n_acc, acc_sum, de_sum, np.stack(xs) if xs else None, np.stack(lps) if lps else None)
