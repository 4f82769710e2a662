"""The MEADS warmup of generalized HMC (Hoffman & Sountsov 2022; ``blackjax.meads_adaptation``) restated in float64 numpy: the yardstick
of ``mfm_meads_warmup`` (mfm_amd/csrc/ghmc.hip).  Where blackjax and the paper differ, this text decides.

``n_valid`` chains form ``K`` folds of ``m = n_valid / K`` chains; chain ``perm[f m + i]`` is member i of fold f; ``perm`` starts as the
identity and, with ``shuffle_every = S > 0``, is replaced before iterations S + 1, 2 S + 1, ... by
``permutation_indices(split(shuffle_key, (n_iter - 1) // S)[r - 1], n_valid)`` (r = 1, 2, ...: jax's ``_shuffle``, as
``mfm_amd.random.permutation_indices``).  Iteration t = 1 .. n_iter, for each fold f from the state BEFORE the step:

1. column mean ``mu_f`` and population standard deviation ``sd_f`` (ddof 0) of the fold's positions
2. ``Y = (x - mu_f) / sd_f``, ``Z = grad * sd_f`` (not centred); ``lam(X) = [(sum_ij S_ij^2 - sum_i S_ii^2) / (m (m - 1))] / [sum_i S_ii / m]``
   with ``S = X X^T``
3. ``eps_f = min(1, 0.5 / sqrt(lam(Z)))``, ``gamma_f = max(1 / sqrt(lam(Y)), 1 / (t eps_f))``, ``alpha_f = 1 - exp(-2 eps_f gamma_f)``,
   ``delta_f = alpha_f / 2``, ``minv_f = sd_f^2``
4. these become the parameters of fold (f + 1) mod K for this iteration's transition, unless any of them is non-finite or
   ``eps_f <= 0``: then the receiving fold keeps what it had (before iteration 1: ``step0``, unit mass, ``alpha0``, ``alpha0 / 2``).

Then one GHMC transition (tests/ghmc_ref.py) of every chain with its fold's parameters, on the key ``mfm_hmc_run`` (n_steps = n_iter)
uses for step t - 1; rows from ``n_valid`` on are stepped with fold 0's parameters and never read.  After the last iteration the same
statistics are formed once over ALL ``n_valid`` chains with t = n_iter + 1: the values to sample with.

``trace [n_iter, K, 6]``: per fold the eps, alpha, delta it USED, lam(Z) and lam(Y) it PRODUCED, its mean acceptance rate;
``mass_trace [n_iter, K, d]``: the minv it used."""
from typing import NamedTuple

import numpy as np

from oracle import prng
from tests import ghmc_ref


def lam(X):
    """The largest-eigenvalue estimate of X^T X / m from the Gram matrix S = X X^T [m, m]."""
    m = X.shape[0]
    S = X @ X.T
    dg = np.diag(S)
    return (((S * S).sum() - (dg * dg).sum()) / (m * (m - 1))) / (dg.sum() / m)


def lam_direct(X):
    """The same number with the pair sum over i != j written out."""
    m = X.shape[0]
    num = sum(float(X[i] @ X[j]) ** 2 for i in range(m) for j in range(m) if i != j) / (m * (m - 1))
    return num / (sum(float(X[i] @ X[i]) for i in range(m)) / m)


def permutation_indices(key, n):
    """``mfm_amd.random.permutation_indices`` on oracle.prng."""
    p = np.arange(n)
    rounds = int(np.ceil(3 * np.log(max(1, n)) / np.log(np.iinfo(np.uint32).max)))
    for _ in range(rounds):
        key, sub = prng.split(key)
        p = p[np.argsort(prng.random_bits32(sub, n), kind="stable")]
    return p


def n_shuffles(n_iter, shuffle_every):
    return (n_iter - 1) // shuffle_every if shuffle_every > 0 else 0


def permutations(shuffle_key, n_iter, shuffle_every, n_valid):
    """[n_shuffles, n_valid] int32: row r - 1 is in force from iteration r S + 1 on."""
    n = n_shuffles(n_iter, shuffle_every)
    if n == 0:
        return np.zeros((0, n_valid), np.int32)
    return np.stack([permutation_indices(k, n_valid) for k in prng.split(shuffle_key, n)]).astype(np.int32)


def perm_at(perms, t, shuffle_every, n_valid):
    """The membership array of iteration t (from 1)."""
    r = (t - 1) // shuffle_every if shuffle_every > 0 else 0
    return np.arange(n_valid) if r == 0 else np.asarray(perms[r - 1])


class FoldStats(NamedTuple):
    eps: float
    alpha: float
    delta: float
    minv: np.ndarray
    lam_z: float
    lam_y: float

    @property
    def usable(self):
        v = np.array([self.eps, self.alpha, self.delta])
        return bool(np.isfinite(v).all() and np.isfinite(self.minv).all() and self.eps > 0)


def fold_stats(x, g, t):
    """Steps 1 - 3 on one fold's positions and gradients ``[m, d]`` at iteration t."""
    with np.errstate(all="ignore"):
        mu = x.mean(0)
        sd = np.sqrt(((x - mu) ** 2).mean(0))
        lz, ly = lam(g * sd), lam((x - mu) / sd)
        eps = min(1.0, 0.5 / np.sqrt(lz)) if not np.isnan(lz) else np.nan
        gamma = max(1.0 / np.sqrt(ly), 1.0 / (t * eps)) if not (np.isnan(ly) or np.isnan(eps)) else np.nan
        alpha = 1.0 - np.exp(-2.0 * eps * gamma)
    return FoldStats(float(eps), float(alpha), float(alpha / 2.0), sd * sd, float(lz), float(ly))


class Params(NamedTuple):
    eps: np.ndarray       # [K]
    alpha: np.ndarray     # [K]
    delta: np.ndarray     # [K]
    minv: np.ndarray      # [K, d]


def initial_params(K, d, step0, alpha0):
    return Params(np.full(K, float(step0)), np.full(K, float(alpha0)), np.full(K, float(alpha0) / 2.0), np.ones((K, d)))


def roll(params, stats):
    """Step 4: fold f's statistics become fold (f + 1) mod K's parameters, or the receiving fold keeps its own."""
    K = len(stats)
    eps, alpha, delta, minv = (np.array(v, np.float64, copy=True) for v in params)
    for f, s in enumerate(stats):
        if s.usable:
            r = (f + 1) % K
            eps[r], alpha[r], delta[r], minv[r] = s.eps, s.alpha, s.delta, s.minv
    return Params(eps, alpha, delta, minv)


def step_keys(key, n_iter, t, n_total):
    """The per-chain keys of iteration t (from 1): ``mfm_hmc_run``'s key_mode 0 keys of step t - 1."""
    return prng.split(prng.split(key, n_iter)[t - 1], n_total)


class Result(NamedTuple):
    state: ghmc_ref.State
    eps: float
    alpha: float
    delta: float
    minv: np.ndarray
    trace: np.ndarray
    mass_trace: np.ndarray
    decisions: np.ndarray       # [n_iter, B]
    slices: np.ndarray          # [n_iter, B] the slice variable after its drift
    energy_changes: np.ndarray  # [n_iter, B]


def warmup(key, state, value_and_grad, n_iter, n_valid, K, step0, alpha0, shuffle_every=0, shuffle_key=None, float32_positions=False,
           restart=None):
    """``state``: tests/ghmc_ref.State of all B chains.  ``restart(t, state) -> state`` (optional) replaces the state before iteration
    t: the GPU test hands in the device's own state so that each iteration is compared from the same start."""
    B, d = state.position.shape
    m = n_valid // K
    perms = permutations(shuffle_key, n_iter, shuffle_every, n_valid)
    par = initial_params(K, d, step0, alpha0)
    trace, mass_trace = np.zeros((n_iter, K, 6)), np.zeros((n_iter, K, d))
    dec, sl, des = [], [], []
    for t in range(1, n_iter + 1):
        if restart is not None:
            state = restart(t, state)
        perm = perm_at(perms, t, shuffle_every, n_valid)
        stats = [fold_stats(state.position[perm[f * m:(f + 1) * m]], state.logdensity_grad[perm[f * m:(f + 1) * m]], t) for f in range(K)]
        par = roll(par, stats)
        fold_of = np.zeros(B, np.int64)
        fold_of[perm] = np.arange(n_valid) // m
        state, info = ghmc_ref.step(step_keys(key, n_iter, t, B), state, value_and_grad, par.eps[fold_of], par.alpha[fold_of], par.delta[fold_of],
                                    par.minv[fold_of], float32_positions=float32_positions)
        for f in range(K):
            trace[t - 1, f] = [par.eps[f], par.alpha[f], par.delta[f], stats[f].lam_z, stats[f].lam_y,
                               info.acceptance_rate[perm[f * m:(f + 1) * m]].mean()]
        mass_trace[t - 1] = par.minv
        dec.append(info.is_accepted); sl.append(info.slice_after_drift); des.append(info.energy_change)
    last = fold_stats(state.position[:n_valid], state.logdensity_grad[:n_valid], n_iter + 1)
    return Result(state, last.eps, last.alpha, last.delta, last.minv, trace, mass_trace, np.stack(dec), np.stack(sl), np.stack(des))
