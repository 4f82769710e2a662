"""Step size and diagonal mass matrix of the HMC kernel together, on Stan's window schedule -- blackjax's ``window_adaptation`` for
``bblackjax/mcmc/hmc.py`` (a BUILD-SIDE MODE like that module: the reference vendors neither).

The warmup's ``num_steps`` steps fall into segments (``window_schedule``): an initial fast buffer, slow windows of doubling length, a
final fast buffer.  Every segment is ONE launch (``mfm_hmc_warmup_window``) on ``split(rng_key, n_segments)[i]``: every chain adapts its
own step size by dual averaging from the pooled step size of the segment before (``mcmc_utils.pooled_step_size``), restarted in every
segment as Stan restarts it after a metric change, and the launch leaves per chain and coordinate the sums of the positions and of
their squares over its steps -- no trajectory is kept, whatever the window's length.  After a slow window of n steps the inverse mass
matrix becomes the regularised variance estimate ``n / (n + 5) W + 1e-3 * 5 / (n + 5)`` (Stan's shrinkage).

``W`` is the WITHIN-chain variance of the window, ``(sum x^2 - (sum x)^2 / n) / (n - 1)`` per chain, averaged over the chains of all
ranks -- not the variance across the chains.  A launch holds thousands of chains, so the average is a low-noise estimate after a few
dozen steps; and on the multimodal targets this project exists for, the variance across chains measures how far apart the modes are,
not the local scale a mass matrix is to match.  (A short window's within-chain variance is biased low by autocorrelation; the doubling
windows are the schedule's answer to that.)

``nuts_window_adaptation`` is the same loop -- schedule, pooling, shrinkage -- on ``mfm_nuts_warmup_window``: every segment's chains adapt
on their trees' acceptance statistic, and no ``num_integration_steps`` has to be chosen."""
from typing import Callable, NamedTuple

import numpy as np

from ... import random as jr
from ...distributions import resolve_logdensity
from ..mcmc.hmc import HMCState, _engine

__all__ = ["window_schedule", "pooled_variance", "regularized_inverse_mass", "window_adaptation", "WindowAdaptationInfo",
           "nuts_window_adaptation", "NUTSWindowAdaptationInfo"]

INITIAL_BUFFER, FINAL_BUFFER, FIRST_WINDOW = 75, 50, 25


def window_schedule(num_steps):
    """Stan's schedule as a list of ``(kind, start, end)`` with ``kind`` ``"fast"`` or ``"slow"``, tiling ``[0, num_steps)``.

    Fewer than 20 steps: one fast segment.  Otherwise an initial buffer of 75 steps, a final buffer of 50 and a first slow window of
    25; if those 150 exceed ``num_steps``, 15 % initial, 10 % final (rounded down) and one slow window for the rest.  Slow windows
    double in length; a window whose successor would end at or beyond the start of the final buffer runs up to it."""
    n = int(num_steps)
    if n < 1:
        raise ValueError(f"num_steps must be at least 1 (got {n})")
    if n < 20:
        return [("fast", 0, n)]
    initial, final, window = INITIAL_BUFFER, FINAL_BUFFER, FIRST_WINDOW
    if initial + window + final > n:
        initial, final = int(0.15 * n), int(0.1 * n)
        window = n - initial - final
    slow_end = n - final
    out = [("fast", 0, initial)] if initial > 0 else []
    start = initial
    while start < slow_end:
        end = start + window
        if end + 2 * window >= slow_end:          # the successor (twice as long) would reach the final buffer
            end = slow_end
        out.append(("slow", start, end))
        start, window = end, 2 * window
    if final > 0:
        out.append(("fast", slow_end, n))
    return out


def pooled_variance(pos_sum, pos_sumsq, n, n_valid=None):
    """``W [dim]``: the within-chain variance ``(sum x^2 - (sum x)^2 / n) / (n - 1)`` of a window of ``n`` steps, averaged over the
    chains of ALL ranks.  ``pos_sum`` / ``pos_sumsq``: float64 ``[n_chain_local, dim]`` as ``mfm_hmc_warmup_window`` leaves them (device
    or CPU tensors, or arrays); rows from ``n_valid`` on are padding and are left out.  The sums over the chains and the count go
    through ONE all-reduce (``engine.allreduce_sum_``), so every rank holds the same vector."""
    import torch
    from ...engine import allreduce_sum_
    n = int(n)
    if n < 2:
        raise ValueError(f"a variance needs a window of at least 2 steps (got {n})")
    s, q = (torch.as_tensor(a, dtype=torch.float64) for a in (pos_sum, pos_sumsq))
    if n_valid is not None:
        s, q = s[:int(n_valid)], q[:int(n_valid)]
    var = (q - s * s / n) / (n - 1)
    packed = torch.cat([var.sum(0), torch.tensor([float(var.shape[0])], dtype=torch.float64, device=var.device)])
    allreduce_sum_(packed)
    return packed[:-1] / packed[-1]


def regularized_inverse_mass(variance, n):
    """Stan's shrinkage of a window's variance estimate towards 1e-3: ``n / (n + 5) * W + 1e-3 * 5 / (n + 5)``."""
    n = float(n)
    return (n / (n + 5.0)) * variance + 1e-3 * (5.0 / (n + 5.0))


class WindowAdaptationInfo(NamedTuple):
    """Per segment, in order: ``schedule`` (``window_schedule``'s), the pooled ``step_sizes`` each segment ENDED with, the mean
    acceptance probability over its steps and chains (``acceptance_rates``); ``inverse_mass_matrices``, the vector after every slow
    window."""
    schedule: list
    step_sizes: list
    acceptance_rates: list
    inverse_mass_matrices: list


class NUTSWindowAdaptationInfo(NamedTuple):
    """``WindowAdaptationInfo``'s fields (``acceptance_rates``: of the trees' acceptance statistic), and per segment the mean number of
    leapfrog steps per transition over its transitions and chains (``mean_integration_steps``)."""
    schedule: list
    step_sizes: list
    acceptance_rates: list
    inverse_mass_matrices: list
    mean_integration_steps: list


def _run_segments(logdensity_fn, initial_step_size, rng_key, state, num_steps, make_info, launch, name):
    """The segment loop both classes share: schedule, one launch per segment from the pooled step size of the one before, the mass after
    every slow window, and the ``finally`` that clears the mass.  ``make_info(schedule)`` gives the info, whose first four fields are
    ``WindowAdaptationInfo``'s; ``launch(eng, info, key, beta, step, n, pos, logp, grad, step_avg, pos_sum, pos_sumsq, acc_sum)`` runs one
    segment of ``n`` steps in place (and may add to ``info`` what only its sampler reports)."""
    from ...engine import global_mean_std
    from ...mcmc_utils import pooled_step_size
    if getattr(rng_key, "ndim", 1) != 1:
        raise ValueError(f"{name}.run takes ONE key (the segments' keys are its children)")
    dist, beta = resolve_logdensity(logdensity_fn)
    schedule = window_schedule(num_steps)
    info = make_info(schedule)
    eng = _engine(dist)
    t = eng.torch
    pos, logp, grad = state.position.clone(), state.logdensity.clone(), state.logdensity_grad.clone()      # states are values
    n_chain, dev = pos.shape[0], pos.device
    f64 = dict(device=dev, dtype=t.float64)
    step_avg, acc_sum = t.empty(n_chain, **f64), t.empty(n_chain, **f64)
    pos_sum, pos_sumsq = t.empty(tuple(pos.shape), **f64), t.empty(tuple(pos.shape), **f64)
    keys = jr.split(rng_key, len(schedule))
    step, minv = initial_step_size, None
    try:
        for key, (kind, start, end) in zip(keys, schedule):
            n = end - start
            eng.ctx.set_inverse_mass(minv)
            launch(eng, info, key, beta, step, n, pos, logp, grad, step_avg, pos_sum, pos_sumsq, acc_sum)
            step = pooled_step_size(step_avg, eng.n_valid)
            info.step_sizes.append(step)
            info.acceptance_rates.append(global_mean_std(acc_sum[:eng.n_valid] / n, eng.n_total)[0].item())
            if kind == "slow":
                minv = regularized_inverse_mass(pooled_variance(pos_sum, pos_sumsq, n, eng.n_valid), n).cpu().numpy()
                info.inverse_mass_matrices.append(minv)
    finally:
        eng.ctx.set_inverse_mass(None)              # a later call's mass is its own argument
    if minv is None:
        minv = np.ones(pos.shape[1], dtype=np.float64)
    return HMCState(pos, logp, grad), {"step_size": step, "inverse_mass_matrix": minv}, info


class window_adaptation:
    """``window_adaptation(logdensity_fn, num_integration_steps, initial_step_size, target_acceptance_rate=0.8).run(rng_key, state,
    num_steps)`` returns ``(state, {"step_size", "inverse_mass_matrix"}, info)``: the chains after the warmup, the parameters to hand
    to ``hmc(logdensity_fn, step_size, num_integration_steps, inverse_mass_matrix)`` (a float and a float64 vector ``[dim]``), and a
    ``WindowAdaptationInfo``.  ``rng_key`` is ONE key (every segment's launch is step-major)."""

    def __init__(self, logdensity_fn: Callable, num_integration_steps: int, initial_step_size: float, target_acceptance_rate: float = 0.8):
        self.logdensity_fn = logdensity_fn
        self.num_integration_steps = int(num_integration_steps)
        self.initial_step_size = float(initial_step_size)
        self.target_acceptance_rate = float(target_acceptance_rate)

    def run(self, rng_key, state: HMCState, num_steps: int):
        def launch(eng, info, key, beta, step, n, pos, logp, grad, step_avg, pos_sum, pos_sumsq, acc_sum):
            eng.ctx.hmc_warmup_window(key, beta, step, self.num_integration_steps, n, self.target_acceptance_rate, pos, logp, grad,
                                      step_avg, pos_sum, pos_sumsq, acc_sum=acc_sum)
        return _run_segments(self.logdensity_fn, self.initial_step_size, rng_key, state, num_steps,
                             lambda schedule: WindowAdaptationInfo(schedule, [], [], []), launch, "window_adaptation")


class nuts_window_adaptation:
    """``nuts_window_adaptation(logdensity_fn, max_num_doublings, initial_step_size, target_acceptance_rate=0.8,
    divergence_threshold=1000).run(rng_key, state, num_steps)`` returns ``(state, {"step_size", "inverse_mass_matrix"}, info)`` as
    ``window_adaptation`` does, every segment one ``mfm_nuts_warmup_window`` launch: the parameters to hand to ``nuts(logdensity_fn,
    step_size, max_num_doublings, inverse_mass_matrix)``, and a ``NUTSWindowAdaptationInfo``."""

    def __init__(self, logdensity_fn: Callable, max_num_doublings: int, initial_step_size: float, target_acceptance_rate: float = 0.8,
                 divergence_threshold: float = 1000.0):
        self.logdensity_fn = logdensity_fn
        self.max_num_doublings = int(max_num_doublings)
        self.initial_step_size = float(initial_step_size)
        self.target_acceptance_rate = float(target_acceptance_rate)
        self.divergence_threshold = float(divergence_threshold)

    def run(self, rng_key, state: HMCState, num_steps: int):
        from ...engine import global_mean_std

        def launch(eng, info, key, beta, step, n, pos, logp, grad, step_avg, pos_sum, pos_sumsq, acc_sum):
            leap = eng.torch.empty(pos.shape[0], device=pos.device, dtype=eng.torch.int64)
            eng.ctx.nuts_warmup_window(key, beta, step, self.max_num_doublings, n, self.target_acceptance_rate, pos, logp, grad, step_avg,
                                       pos_sum, pos_sumsq, divergence_threshold=self.divergence_threshold, acc_sum=acc_sum, leapfrog_sum=leap)
            info.mean_integration_steps.append(global_mean_std(leap[:eng.n_valid].double() / n, eng.n_total)[0].item())
        return _run_segments(self.logdensity_fn, self.initial_step_size, rng_key, state, num_steps,
                             lambda schedule: NUTSWindowAdaptationInfo(schedule, [], [], [], []), launch, "nuts_window_adaptation")
