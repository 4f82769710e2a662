"""No-U-turn sampler on MI355X -- a BUILD-SIDE MODE beside ``hmc.py``: the reference vendors neither.

Multinomial NUTS in the iterative, checkpointed form (Betancourt's "Conceptual Introduction", appendix A; the formulation of blackjax
and NumPyro; device: ``mfm_nuts_step`` / ``mfm_nuts_run``, ``csrc/nuts.hip``; restated in ``tests/nuts_ref.py``), with the conventions of
``hmc.py``: ``state.position`` is ``[n_chain_local, dim]`` (CUDA float32), ``rng_key`` the key BEFORE the per-chain split or the
caller's own keys ``[n_chain_local, 2]``, ``logdensity_fn`` built from a device target, ``inverse_mass_matrix`` the DIAGONAL as a
vector ``[dim]`` (a call's mass is its argument: every launch installs or clears it first).  The integrator and the metric are HMC's,
so a step size and a mass adapted by ``hmc(...).step.warmup`` / ``adaptation.window_adaptation`` carry over.  The kernel carries
``kernel.run(rng_key, state, logdensity_fn, step_size, num_steps, thin=0, ...)``: ``num_steps`` transitions in ONE launch with the
chain resident on the device, bit-identical with the loop of single steps (key schedule: ``hmc.py``), and ``kernel.warmup(rng_key,
state, logdensity_fn, step_size, num_steps, target_acceptance_rate=0.8, return_step_sizes=False, ...)``: ``num_steps`` transitions in one
launch (``mfm_nuts_warmup``) in which every chain adapts its own step size from ``step_size`` by dual averaging on its tree's acceptance
statistic -- NUTS tunes itself, no ``num_integration_steps`` has to be chosen (``adaptation.nuts_window_adaptation`` adds the mass)."""
from typing import Callable, NamedTuple

from ...distributions import resolve_logdensity
from ..base import SamplingAlgorithm
from .hmc import HMCState as NUTSState, _device_keys, _mass_engine, check_inverse_mass, init

__all__ = ["NUTSState", "NUTSInfo", "NUTSRunInfo", "NUTSWarmupInfo", "init", "build_kernel", "nuts"]


class NUTSInfo(NamedTuple):
    """blackjax's field names.  Per chain: the completed doublings, the leapfrog steps, whether the tree ended on a U-turn / on a
    divergent leaf, the mean of ``min(1, exp(H0 - H))`` over every leaf integrated (the statistic dual averaging would use), the
    proposal's energy."""
    num_trajectory_expansions: object
    num_integration_steps: object
    is_turning: object
    is_divergent: object
    acceptance_rate: object
    energy: object


class NUTSRunInfo(NamedTuple):
    """What ``kernel.run`` reports.  Per chain over the run: the mean acceptance rate, the leapfrog steps (int64), the divergent
    transitions, the mean depth; the LAST transition's ``NUTSInfo``; with ``thin`` the kept states ``positions [num_steps / thin,
    n_chain, dim]`` / ``logdensities [num_steps / thin, n_chain]`` (``None`` without)."""
    acceptance_rate: object
    num_integration_steps: object
    num_divergent: object
    mean_trajectory_expansions: object
    last: NUTSInfo
    positions: object
    logdensities: object


class NUTSWarmupInfo(NamedTuple):
    """What ``kernel.warmup`` reports.  Per chain (``[n_chain_local]``): ``step_size`` (float64), the averaged iterate ``exp(xbar_n)`` --
    the result; ``pooled_step_size``, ONE float, the geometric mean of ``step_size`` over the chains of all ranks without the padding
    rows (``mcmc_utils.pooled_step_size``); per chain the mean over the warmup of the trees' acceptance statistic, the leapfrog steps
    (int64), the divergent transitions and the mean depth; ``step_sizes [num_steps, n_chain_local]``, the step size USED at every
    transition (``None`` unless asked for)."""
    step_size: object
    pooled_step_size: float
    acceptance_rate: object
    num_integration_steps: object
    num_divergent: object
    mean_depth: object
    step_sizes: object


def _info_buffers(t, n, dev):
    return dict(depth=t.empty(n, device=dev, dtype=t.int32), num_leapfrog=t.empty(n, device=dev, dtype=t.int32),
                is_turning=t.empty(n, device=dev, dtype=t.uint8), is_divergent=t.empty(n, device=dev, dtype=t.uint8),
                acceptance_rate=t.empty(n, device=dev, dtype=t.float64), energy=t.empty(n, device=dev, dtype=t.float64))


def _info(b):
    return NUTSInfo(b["depth"], b["num_leapfrog"], b["is_turning"].bool(), b["is_divergent"].bool(), b["acceptance_rate"], b["energy"])


def build_kernel():
    def kernel(rng_key, state: NUTSState, logdensity_fn: Callable, step_size: float, max_num_doublings: int = 10, inverse_mass_matrix=None,
               divergence_threshold: float = 1000.0):
        """One key: chain b draws from ``split(rng_key, n_chain_total)[chain_offset + b]``; keys ``[n_chain_local, 2]``: the caller's
        own vmap, chain b draws from ``rng_key[b]``."""
        dist, beta = resolve_logdensity(logdensity_fn)
        eng = _mass_engine(dist, inverse_mass_matrix)
        t = eng.torch
        pos, logp, grad = state.position.clone(), state.logdensity.clone(), state.logdensity_grad.clone()      # states are values
        buf = _info_buffers(t, pos.shape[0], pos.device)
        if getattr(rng_key, "ndim", 1) == 2:
            eng.ctx.nuts_step_keys(_device_keys(t, rng_key, pos.device), beta, step_size, max_num_doublings, pos, logp, grad,
                                   divergence_threshold=divergence_threshold, **buf)
        else:
            eng.ctx.nuts_step(rng_key, beta, step_size, max_num_doublings, pos, logp, grad, divergence_threshold=divergence_threshold, **buf)
        return NUTSState(pos, logp, grad), _info(buf)

    def run(rng_key, state: NUTSState, logdensity_fn: Callable, step_size: float, num_steps: int, thin: int = 0, max_num_doublings: int = 10,
            inverse_mass_matrix=None, divergence_threshold: float = 1000.0):
        """``num_steps`` calls of ``kernel`` in one: with ONE key step j uses ``split(rng_key, num_steps)[j]`` (the scan of
        ``inference_loop0``); with keys ``[n_chain_local, 2]`` step j of chain b uses ``split(rng_key[b], num_steps)[j]``.
        Bit-identical with that loop.  ``thin >= 1`` keeps the state after every ``thin``-th step."""
        dist, beta = resolve_logdensity(logdensity_fn)
        eng = _mass_engine(dist, inverse_mass_matrix)
        t = eng.torch
        num_steps, thin = int(num_steps), int(thin)
        pos, logp, grad = state.position.clone(), state.logdensity.clone(), state.logdensity_grad.clone()
        n, dev = pos.shape[0], pos.device
        buf = _info_buffers(t, n, dev)
        leap = t.empty(n, device=dev, dtype=t.int64)
        acc_sum = t.empty(n, device=dev, dtype=t.float64)
        n_div = t.empty(n, device=dev, dtype=t.int32)
        depth_sum = t.empty(n, device=dev, dtype=t.int32)
        traj_pos = traj_logp = None
        if thin > 0 and num_steps >= thin and num_steps % thin == 0:       # (anything else: the library names the bad argument)
            traj_pos = t.empty((num_steps // thin,) + tuple(pos.shape), device=dev, dtype=t.float32)
            traj_logp = t.empty((num_steps // thin, n), device=dev, dtype=t.float64)
        if getattr(rng_key, "ndim", 1) == 2:
            rng_key = _device_keys(t, rng_key, dev)
        eng.ctx.nuts_run(rng_key, beta, step_size, max_num_doublings, num_steps, pos, logp, grad, divergence_threshold=divergence_threshold,
                         thin=thin, leapfrog_sum=leap, acc_sum=acc_sum, n_divergent=n_div, depth_sum=depth_sum, traj_pos=traj_pos,
                         traj_logp=traj_logp, **buf)
        return NUTSState(pos, logp, grad), NUTSRunInfo(acc_sum / num_steps, leap, n_div, depth_sum.double() / num_steps, _info(buf), traj_pos, traj_logp)

    def warmup(rng_key, state: NUTSState, logdensity_fn: Callable, step_size: float, num_steps: int, target_acceptance_rate: float = 0.8,
               return_step_sizes: bool = False, max_num_doublings: int = 10, inverse_mass_matrix=None, divergence_threshold: float = 1000.0):
        """``num_steps`` transitions in one launch, from ``step_size``, every chain adapting its own step size towards
        ``target_acceptance_rate`` on its tree's acceptance statistic; keys as ``run``'s (one key: step-major; ``[n_chain_local, 2]``:
        chain-major).  Returns the state after the transitions and a ``NUTSWarmupInfo``; ``info.pooled_step_size`` is the value to
        sample with."""
        from ...mcmc_utils import pooled_step_size
        dist, beta = resolve_logdensity(logdensity_fn)
        eng = _mass_engine(dist, inverse_mass_matrix)
        t = eng.torch
        num_steps = int(num_steps)
        pos, logp, grad = state.position.clone(), state.logdensity.clone(), state.logdensity_grad.clone()      # states are values
        n, dev = pos.shape[0], pos.device
        step_avg = t.empty(n, device=dev, dtype=t.float64)
        acc_sum = t.empty(n, device=dev, dtype=t.float64)
        leap = t.empty(n, device=dev, dtype=t.int64)
        n_div = t.empty(n, device=dev, dtype=t.int32)
        depth_sum = t.empty(n, device=dev, dtype=t.int32)
        traj = t.empty((num_steps, n), device=dev, dtype=t.float64) if return_step_sizes and num_steps >= 1 else None
        if getattr(rng_key, "ndim", 1) == 2:
            rng_key = _device_keys(t, rng_key, dev)
        eng.ctx.nuts_warmup(rng_key, beta, step_size, max_num_doublings, num_steps, target_acceptance_rate, pos, logp, grad, step_avg,
                            divergence_threshold=divergence_threshold, acc_sum=acc_sum, step_traj=traj, leapfrog_sum=leap, n_divergent=n_div,
                            depth_sum=depth_sum)
        return NUTSState(pos, logp, grad), NUTSWarmupInfo(step_avg, pooled_step_size(step_avg, eng.n_valid), acc_sum / num_steps, leap, n_div,
                                                          depth_sum.double() / num_steps, traj)

    kernel.run = run
    kernel.warmup = warmup
    return kernel


class nuts:
    init = staticmethod(init)
    build_kernel = staticmethod(build_kernel)

    def __new__(cls, logdensity_fn: Callable, step_size: float, max_num_doublings: int = 10, inverse_mass_matrix=None,
                divergence_threshold: float = 1000.0) -> SamplingAlgorithm:
        kernel = cls.build_kernel()
        minv = check_inverse_mass(inverse_mass_matrix, getattr(resolve_logdensity(logdensity_fn)[0], "dim", None))

        def init_fn(position):
            return cls.init(position, logdensity_fn)

        def step_fn(rng_key, state):
            return kernel(rng_key, state, logdensity_fn, step_size, max_num_doublings, minv, divergence_threshold)

        def run_fn(rng_key, state, num_steps, thin=0):
            return kernel.run(rng_key, state, logdensity_fn, step_size, num_steps, thin, max_num_doublings, minv, divergence_threshold)

        def warmup_fn(rng_key, state, num_steps, target_acceptance_rate=0.8, return_step_sizes=False):
            return kernel.warmup(rng_key, state, logdensity_fn, step_size, num_steps, target_acceptance_rate, return_step_sizes, max_num_doublings,
                                 minv, divergence_threshold)

        step_fn.run = run_fn
        step_fn.warmup = warmup_fn
        return SamplingAlgorithm(init_fn, step_fn)
