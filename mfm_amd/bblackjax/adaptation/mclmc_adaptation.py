"""``blackjax.mclmc_find_L_and_step_size``: the step size and the momentum decoherence length of MCLMC (``mcmc/mclmc.py``) from the
chains themselves.  A host loop of ``run`` launches (``mfm_mclmc_run``); nothing but three sums per launch comes back to the host.

``algorithm_fn(L, step_size)`` gives the sampler at those values: ``mclmc(logdensity_fn, L, step_size, integrator)`` or anything whose
``.step.run`` (or ``.run``) is ``run(rng_key, state, num_steps, thin=0) -> (state, info)`` with ``info.energy_var_per_dim``,
``info.num_nonfinite`` and ``info.positions`` -- tests/test_mclmc_ref.py hands it the float64 restatement on numpy arrays.

Phase 1, step size (``frac_tune1 * num_steps`` steps in ``num_rounds`` rounds of equal length, at L = sqrt(dim)): after each round v
is the variance of the steps' energy changes pooled over chains and steps, per dimension, and eps <- eps clip((target / v)^(1/6), 1/3, 3):
the energy error of the second-order schedules grows as eps^3, its variance as eps^6.  A non-finite v or any non-finite energy change
halves eps.  Phase 2, L (``frac_tune2 * num_steps`` steps): L = sqrt(sum_j Var x_j) over the chains and the kept steps of a thinned
run, then one more phase-1 round at that L.  Phase 3 (``frac_tune3 > 0``): L = 0.4 eps mean_j tau_j with tau the integrated
autocorrelation time (``mcmc_utils.effective_sample_size``, ``mfm_autocorr``) of a run's trajectory.  With more than one rank every
pooled figure goes through one all-reduce, as ``mcmc_utils.pooled_step_size``.  The chains carry on from round to round; the returned
state is where they ended."""
import math
from typing import NamedTuple

__all__ = ["MCLMCAdaptationState", "mclmc_find_L_and_step_size", "step_size_update"]

KEPT = 32            # states a phase-2 / phase-3 run keeps at most (thinned: they are [kept, n_chain, dim] on the device)


class MCLMCAdaptationState(NamedTuple):
    L: float
    step_size: float


def step_size_update(eps, v, n_nonfinite, target):
    """One phase-1 update (module docstring)."""
    if n_nonfinite > 0 or not math.isfinite(v) or v < 0:
        return 0.5 * eps
    if v == 0.0:
        return 3.0 * eps
    return eps * min(max((target / v) ** (1.0 / 6.0), 1.0 / 3.0), 3.0)


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def _allreduce(values, like):
    """``values`` (floats) summed over the ranks -- as they are for numpy states or one rank."""
    if not _is_torch(like):
        return values
    import torch
    from ...engine import allreduce_sum_
    s = torch.tensor(values, dtype=torch.float64, device=like.device)
    allreduce_sum_(s)
    return s.tolist()


def _position_variance(positions, n_valid):
    """sum_j Var x_j over chains and kept steps of ``positions [kept, n_chain, dim]``."""
    p = positions if n_valid is None else positions[:, :int(n_valid)]
    d = p.shape[-1]
    p = p.reshape(-1, d)
    p = p.double() if _is_torch(p) else p.astype("float64")
    if _is_torch(p):
        import torch
        from ...engine import allreduce_sum_
        s = torch.cat([p.sum(0), (p * p).sum(0), torch.tensor([float(p.shape[0])], dtype=torch.float64, device=p.device)])
        allreduce_sum_(s)
        m = s[:d] / s[-1]
        return float((s[d:2 * d] / s[-1] - m * m).sum().item())
    m = p.mean(0)
    return float(((p * p).mean(0) - m * m).sum())


def _run_of(algo):
    run = getattr(algo, "run", None)
    return run if run is not None else algo.step.run


def _thinned(n):
    """(steps, thin) of a run of about n steps that keeps at most KEPT states."""
    thin = max(1, -(-n // KEPT))                       # ceil(n / KEPT): n // thin <= KEPT
    return max(thin, n // thin * thin), thin


def mclmc_find_L_and_step_size(algorithm_fn, state, rng_key, num_steps, frac_tune1=0.1, frac_tune2=0.1, frac_tune3=0.1,
                               desired_energy_var=5e-4, num_rounds=8, initial_step_size=0.01, n_valid=None, ess_fn=None, history=None):
    """``(state, MCLMCAdaptationState(L, step_size))`` (module docstring).  ``initial_step_size``: where phase 1 starts (a round moves
    it by at most a factor 3).  ``n_valid``: chains from there on are padding rows and stay out of the position statistics.
    ``history``: a list that takes ``(phase, L, step_size, energy_var_per_dim)`` of every launch."""
    from ... import random as jr
    dim = int(state.position.shape[-1])
    num_steps, num_rounds = int(num_steps), max(1, int(num_rounds))
    if not (desired_energy_var > 0):
        raise ValueError(f"desired_energy_var must be positive (got {desired_energy_var})")
    if not (initial_step_size > 0):
        raise ValueError(f"initial_step_size must be positive (got {initial_step_size})")
    round_len = max(1, int(num_steps * frac_tune1) // num_rounds)
    n2, n3 = int(num_steps * frac_tune2), int(num_steps * frac_tune3)
    keys = jr.split(rng_key, num_rounds + 3)
    L, eps = math.sqrt(dim), float(initial_step_size)

    def tune_round(key, state, L, eps, phase):
        state, info = _run_of(algorithm_fn(L, eps))(key, state, round_len, thin=0)
        v = float(info.energy_var_per_dim)
        bad = _allreduce([float(info.num_nonfinite.sum())], state.position)[0]
        if history is not None:
            history.append((phase, L, eps, v))
        return state, step_size_update(eps, v, bad, desired_energy_var)

    for r in range(num_rounds):
        state, eps = tune_round(keys[r], state, L, eps, 1)
    if n2 > 0:
        steps, thin = _thinned(n2)
        state, info = _run_of(algorithm_fn(L, eps))(keys[num_rounds], state, steps, thin=thin)
        if history is not None:
            history.append((2, L, eps, float(info.energy_var_per_dim)))
        var = _position_variance(info.positions, n_valid)
        if math.isfinite(var) and var > 0:
            L = math.sqrt(var)
        state, eps = tune_round(keys[num_rounds + 1], state, L, eps, 2)
    if n3 > 0:
        if ess_fn is None:
            from ...mcmc_utils import effective_sample_size as ess_fn
        steps, thin = _thinned(n3)
        state, info = _run_of(algorithm_fn(L, eps))(keys[num_rounds + 2], state, steps, thin=thin)
        if history is not None:
            history.append((3, L, eps, float(info.energy_var_per_dim)))
        pos = info.positions if n_valid is None else info.positions[:, :int(n_valid)]
        _, tau = ess_fn(pos)
        tau = tau.double() if _is_torch(tau) else tau.astype("float64")
        s = _allreduce([float(tau.sum()), float(tau.size if not _is_torch(tau) else tau.numel())], state.position)
        tau_steps = thin * s[0] / s[1]                                  # (tau of the kept states, in steps)
        if math.isfinite(tau_steps) and tau_steps > 0:
            L = 0.4 * eps * tau_steps
    return state, MCLMCAdaptationState(L, eps)
