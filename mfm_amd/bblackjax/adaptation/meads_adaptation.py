"""MEADS: the step size, the diagonal preconditioner, the momentum refresh rate and the slice drift of ``bblackjax/mcmc/ghmc.py`` set
from cross-chain statistics -- blackjax's ``meads_adaptation`` (Hoffman & Sountsov 2022), a BUILD-SIDE MODE like ``chees_adaptation.py``.

The chains are cut into folds; every iteration each fold's positions and gradients give a largest-eigenvalue estimate of the
preconditioned Hessian (the step size) and of the standardised covariance (the damping, hence ``alpha``), and the fold's column variances
give the inverse mass; the NEXT fold is stepped with them, so no chain is steered by its own state.  No trajectory length, no tree
depth.  The whole warmup is ONE library call (``mfm_meads_warmup``: six launches per iteration, no host round trip; the algorithm line by
line: ``include/mfm.h``, ``tests/meads_ref.py``).  One rank; the Cox process is not served.

    warmup = meads_adaptation(logdensity_fn, num_chains, num_folds=4)
    (state, parameters), info = warmup.run(rng_key, positions, num_steps)
    algo = ghmc(logdensity_fn, **parameters)
    state, run_info = algo.step.run(rng_key, state, n)
"""
from typing import Callable, NamedTuple

import numpy as np

from ... import random as jr
from ...distributions import resolve_logdensity
from ..mcmc.ghmc import GHMCState, _refuse_cox, _target_engine, check_parameters, init as ghmc_init
from ..mcmc.hmc import _device_keys

__all__ = ["meads_adaptation", "MeadsAdaptationInfo", "check_folds", "shuffle_permutations"]


class MeadsAdaptationInfo(NamedTuple):
    """Per iteration and fold (float64 CPU tensors ``[num_steps, num_folds]``): the step size, ``alpha`` and ``delta`` the fold USED, the
    eigenvalue estimates ``lam(Z)`` / ``lam(Y)`` it PRODUCED, its mean acceptance rate; ``inverse_mass`` ``[num_steps, num_folds, dim]``,
    the diagonal inverse mass it used (``None`` unless asked for)."""
    step_size: object
    alpha: object
    delta: object
    max_eigen_gradient: object
    max_eigen_position: object
    mean_acceptance: object
    inverse_mass: object


def check_folds(num_chains, num_folds):
    """``ValueError`` unless the chains split into ``num_folds >= 2`` folds of at least 2."""
    num_chains, num_folds = int(num_chains), int(num_folds)
    if num_folds < 2:
        raise ValueError(f"meads_adaptation needs num_folds >= 2: a fold is steered by another fold's statistics (got {num_folds})")
    if num_chains % num_folds or num_chains < 2 * num_folds:
        raise ValueError(f"meads_adaptation: num_chains ({num_chains}) must be a multiple of num_folds ({num_folds}) with at least 2 chains per fold")
    return num_chains // num_folds


def shuffle_permutations(rng_key, num_steps, shuffle_every, num_chains):
    """The membership arrays of a warmup, int32 ``[(num_steps - 1) // shuffle_every, num_chains]``: row r - 1 is in force from iteration
    ``r shuffle_every + 1`` on; drawn on the host, ``permutation_indices(split(rng_key, rows)[r - 1], num_chains)``."""
    rows = (int(num_steps) - 1) // int(shuffle_every) if shuffle_every > 0 else 0
    if rows == 0:
        return np.zeros((0, int(num_chains)), np.int32)
    return np.stack([jr.permutation_indices(k, int(num_chains)) for k in jr.split(rng_key, rows)]).astype(np.int32)


class meads_adaptation:
    """``meads_adaptation(logdensity_fn, num_chains=None, num_folds=4, shuffle_every=0, initial_step_size=..., initial_alpha=...)``.
    ``num_chains``: the chains the statistics are formed over (``None``: the engine's valid chains); ``shuffle_every = S > 0`` redraws
    the fold membership before iterations S + 1, 2 S + 1, ...  The initial values are used only by a fold whose first statistics are
    not finite."""

    def __init__(self, logdensity_fn: Callable, num_chains=None, num_folds: int = 4, shuffle_every: int = 0, initial_step_size: float = 0.1,
                 initial_alpha: float = 0.5):
        self.logdensity_fn = logdensity_fn
        dist = resolve_logdensity(logdensity_fn)[0]
        _refuse_cox(dist)
        self.num_chains = None if num_chains is None else int(num_chains)
        self.num_folds, self.shuffle_every = int(num_folds), int(shuffle_every)
        if self.shuffle_every < 0:
            raise ValueError(f"meads_adaptation: shuffle_every must not be negative (got {shuffle_every})")
        check_folds(2 * max(self.num_folds, 1) if self.num_chains is None else self.num_chains, self.num_folds)
        self.step0, self.alpha0, _ = check_parameters(initial_step_size, initial_alpha, None)

    def run(self, rng_key, positions, num_steps: int, keep_inverse_mass: bool = False):
        """``num_steps`` MEADS iterations from ``positions [n_chain_local, dim]`` (or a ``GHMCState``).  ``rng_key`` is split three ways:
        the initial momenta and slice variables, the transitions (step-major, as ``ghmc(...).step.run``), the shuffles.  Returns
        ``((state, parameters), info)``: the ``GHMCState`` after the warmup, ``parameters = dict(step_size, alpha, delta,
        momentum_inverse_scale)`` for ``ghmc`` (the scale a float64 device tensor ``[dim]``, the closing pass's ``sd``), and a
        ``MeadsAdaptationInfo``."""
        eng, beta = _target_engine(self.logdensity_fn)
        t = eng.torch
        num_steps = int(num_steps)
        if num_steps < 1:
            raise ValueError(f"meads_adaptation: num_steps must be at least 1 (got {num_steps})")
        n_rows = (positions.position if isinstance(positions, GHMCState) else positions).shape[0]
        n_valid = int(getattr(eng, "n_valid", n_rows)) if self.num_chains is None else self.num_chains
        check_folds(n_valid, self.num_folds)
        k_init, k_run, k_shuffle = jr.split(rng_key, 3)
        state = positions if isinstance(positions, GHMCState) else ghmc_init(positions.clone(), self.logdensity_fn, k_init)
        pos, mom, logp, grad, s = (x.clone() for x in state)
        dev, K, d = pos.device, self.num_folds, pos.shape[1]
        perms = None
        if self.shuffle_every > 0 and (num_steps - 1) // self.shuffle_every > 0:
            perms = t.as_tensor(shuffle_permutations(k_shuffle, num_steps, self.shuffle_every, n_valid), device=dev)
        trace = t.empty((num_steps, K, 6), device=dev, dtype=t.float64)
        mass_trace = t.empty((num_steps, K, d), device=dev, dtype=t.float64) if keep_inverse_mass else None
        minv = t.empty(d, device=dev, dtype=t.float64)
        if getattr(k_run, "ndim", 1) == 2:
            k_run = _device_keys(t, k_run, dev)
        eps, alpha, delta = eng.ctx.meads_warmup(k_run, beta, self.step0, self.alpha0, num_steps, pos, logp, grad, mom, s, n_folds=K, n_valid=n_valid,
                                                 shuffle_every=self.shuffle_every, perms=perms, inverse_mass_out=minv, trace=trace, mass_trace=mass_trace)
        tr = trace.cpu()
        info = MeadsAdaptationInfo(tr[:, :, 0], tr[:, :, 1], tr[:, :, 2], tr[:, :, 3], tr[:, :, 4], tr[:, :, 5],
                                   None if mass_trace is None else mass_trace.cpu())
        if not (np.isfinite([eps, alpha, delta]).all() and eps > 0 and bool(t.isfinite(minv).all()) and bool((minv > 0).all())):
            raise RuntimeError(f"meads_adaptation: the closing statistics are not usable (step_size {eps}, alpha {alpha}, delta {delta}): "
                               "the chains have collapsed or diverged")
        parameters = dict(step_size=eps, alpha=alpha, delta=delta, momentum_inverse_scale=t.sqrt(minv))
        return (GHMCState(pos, mom, logp, grad, s), parameters), info
