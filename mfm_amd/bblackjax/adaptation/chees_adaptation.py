"""ChEES-HMC: the step size and the trajectory length of ``bblackjax/mcmc/hmc.py`` adapted ACROSS the chains -- blackjax's
``chees_adaptation`` (Hoffman, Radul & Sountsov 2021), a BUILD-SIDE MODE like ``window_adaptation.py`` (the reference vendors neither).

Every iteration all chains take the same number of leapfrog steps, a jittered trajectory length ``h_t T`` over a shared step size
(``h_t``: the base-2 radical inverse of ``t``); ``T`` climbs the gradient of the Change in the Estimator of the Expected Square pooled
over the chains (Adam on ``log T``), the step size follows the chains' harmonic-mean acceptance by dual averaging.  The whole warmup is
ONE library call (``mfm_chees_warmup``: four launches per iteration, no host round trip; the algorithm line by line: ``include/mfm.h``,
``tests/chees_ref.py``).  One rank; the Cox process is not served; the mass is used as given.

    warmup = chees_adaptation(logdensity_fn, num_chains)
    (state, parameters), info = warmup.run(rng_key, state, step_size, adam(0.025), num_steps)
    algo = hmc(logdensity_fn, parameters["step_size"], 1, parameters["inverse_mass_matrix"])
    lengths = [parameters["integration_steps_fn"](i) for i in range(n)]
    state, run_info = algo.step.run(rng_key, state, n, num_integration_steps_per_step=lengths)
"""
import math
from typing import Callable, NamedTuple

import numpy as np

from ...distributions import resolve_logdensity
from ..mcmc.hmc import HMCState, _device_keys, _mass_engine, check_inverse_mass
from ..optimizers import Optimizer

__all__ = ["chees_adaptation", "CheesAdaptationInfo", "radical_inverse", "integration_steps"]


def radical_inverse(t):
    """Base-2 radical inverse of ``t >= 1``: 1/2, 1/4, 3/4, 1/8, ... (the jitter of iteration / sampling step ``t``)."""
    t, h, f = int(t), 0.0, 0.5
    while t:
        if t & 1:
            h += f
        t >>= 1
        f *= 0.5
    return h


def integration_steps(i, step_size, trajectory_length, max_leapfrog=1000):
    """The leapfrog steps of sampling step ``i`` (from 0): ``min(max_leapfrog, max(1, ceil(h_{i+1} T / eps)))``."""
    n = math.ceil(radical_inverse(int(i) + 1) * float(trajectory_length) / float(step_size))
    return int(min(max(n, 1), int(max_leapfrog)))


class CheesAdaptationInfo(NamedTuple):
    """Per iteration (float64 CPU tensors ``[num_steps]``): the step size and trajectory length USED, the leapfrog steps, the chains'
    harmonic-mean acceptance, the pooled ChEES gradient, the number of divergent chains, the mean acceptance probability."""
    step_size: object
    trajectory_length: object
    num_integration_steps: object
    harmonic_mean_acceptance: object
    trajectory_gradient: object
    num_divergent: object
    mean_acceptance: object


def _learning_rate(optimizer):
    if not isinstance(optimizer, Optimizer) or optimizer.kind != "adam":
        raise TypeError("optimizer must be mfm_amd.bblackjax.optimizers.adam(learning_rate): the update of log T runs on the device "
                        f"(got {getattr(optimizer, 'kind', type(optimizer).__name__)})")
    lr, b1, b2, eps = optimizer.hyper
    if (b1, b2, eps) != (0.9, 0.999, 1e-8):
        raise ValueError(f"the device's update of log T fixes adam's b1 = 0.9, b2 = 0.999, eps = 1e-8 (got {b1}, {b2}, {eps})")
    return lr


class chees_adaptation:
    """``num_chains``: how many of the state's chains count (default: the engine's valid chains; padding rows are stepped but not
    pooled)."""

    def __init__(self, logdensity_fn: Callable, num_chains=None, target_acceptance_rate: float = 0.651, decay_rate: float = 0.5,
                 max_leapfrog: int = 1000, inverse_mass_matrix=None):
        self.logdensity_fn = logdensity_fn
        self.num_chains = None if num_chains is None else int(num_chains)
        self.target_acceptance_rate = float(target_acceptance_rate)
        self.decay_rate = float(decay_rate)
        self.max_leapfrog = int(max_leapfrog)
        self.inverse_mass_matrix = check_inverse_mass(inverse_mass_matrix, getattr(resolve_logdensity(logdensity_fn)[0], "dim", None))

    def run(self, rng_key, state: HMCState, step_size: float, optimizer, num_steps: int, trajectory_length=None,
            divergence_threshold: float = 1000.0):
        """``rng_key``: one key (step-major) or keys ``[n_chain_local, 2]`` (chain-major), as ``hmc(...).step.run``'s.  Returns
        ``(last_state, parameters), info``."""
        lr = _learning_rate(optimizer)                 # (before any device work)
        num_steps = int(num_steps)
        dist, beta = resolve_logdensity(self.logdensity_fn)
        eng = _mass_engine(dist, self.inverse_mass_matrix)
        t = eng.torch
        pos, logp, grad = state.position.clone(), state.logdensity.clone(), state.logdensity_grad.clone()      # states are values
        n, dev = pos.shape[0], pos.device
        trace = t.zeros((max(num_steps, 1), 7), device=dev, dtype=t.float64)
        if getattr(rng_key, "ndim", 1) == 2:
            rng_key = _device_keys(t, rng_key, dev)
        n_valid = self.num_chains if self.num_chains is not None else getattr(eng, "n_valid", n)
        eps, T, _, _ = eng.ctx.chees_warmup(rng_key, beta, step_size, num_steps, pos, logp, grad, traj0=trajectory_length, n_valid=n_valid,
                                            target_accept=self.target_acceptance_rate, learning_rate=lr, max_leapfrog=self.max_leapfrog,
                                            decay=self.decay_rate, divergence_threshold=divergence_threshold, trace=trace)
        tr = trace.cpu()
        minv = self.inverse_mass_matrix if self.inverse_mass_matrix is not None else np.ones(pos.shape[1], dtype=np.float64)
        max_leapfrog = self.max_leapfrog
        parameters = {"step_size": eps, "trajectory_length": T, "inverse_mass_matrix": minv,
                      "integration_steps_fn": lambda i: integration_steps(i, eps, T, max_leapfrog)}
        return (HMCState(pos, logp, grad), parameters), CheesAdaptationInfo(*(tr[:, j].clone() for j in range(7)))
