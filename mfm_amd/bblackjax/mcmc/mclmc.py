"""Microcanonical Langevin Monte Carlo on MI355X -- ``blackjax.mclmc``, a BUILD-SIDE MODE beside ``hmc.py`` / ``nuts.py``.

The unadjusted sampler of Robnik, De Luca, Silverstein & Seljak (2023) and Robnik & Seljak (2024): a chain is a position and a UNIT
momentum; a step of size ``step_size`` runs a palindromic schedule of the exact momentum flow and the drift (``integrator``:
``"leapfrog"``, one gradient per step, or ``"mclachlan"``, McLachlan's minimal-norm scheme, two -- blackjax's default) and then refreshes
the momentum partially, ``u <- (u + nu z) / |u + nu z|`` with ``nu = sqrt((exp(2 step_size / L) - 1) / dim)``; ``L = inf`` never
refreshes.  There is NO accept test: every step is taken, and the step's energy change is its diagnostic -- the tuner
(``adaptation/mclmc_adaptation.mclmc_find_L_and_step_size``) steers its variance per dimension to 5e-4.  ``tests/mclmc_ref.py`` restates
the algorithm in float64; the device kernels are ``mfm_mclmc_*`` (``csrc/mclmc.hip``).

Conventions as ``hmc.py``: ``state.position`` is ``[n_chain_local, dim]`` (CUDA float32), ``state.momentum`` ``[n_chain_local, dim]``
float64, ``rng_key`` the key BEFORE the per-chain split (keys ``[n_chain_local, 2]``: the caller's own vmap, ``mfm_mclmc_step_keys``),
states are values.  ``algo.step.run(rng_key, state, num_steps, thin=0, keep_energy=False)`` is ``num_steps`` steps in ONE launch
(``mfm_mclmc_run``), bit-identical with the loop, and ``inference_loop0`` picks it up.  phi-four and mixture targets, unit metric:
the Cox process is a ``ValueError`` before any device work."""
from typing import Callable, NamedTuple

import numpy as np

from ...distributions import resolve_logdensity
from ..base import SamplingAlgorithm
from .hmc import _device_keys, _is_cox
from .mala import _engine

__all__ = ["IntegratorState", "MCLMCInfo", "MCLMCRunInfo", "INTEGRATORS", "init", "build_kernel", "mclmc", "integrator_id", "energy_var_per_dim"]

INTEGRATORS = {"leapfrog": 0, "mclachlan": 1}


def integrator_id(integrator):
    """``"leapfrog"`` / ``"mclachlan"`` / 0 / 1 as the library's 0 / 1; ``ValueError`` for anything else."""
    if isinstance(integrator, str):
        if integrator not in INTEGRATORS:
            raise ValueError(f"integrator must be 'leapfrog' or 'mclachlan' (got {integrator!r})")
        return INTEGRATORS[integrator]
    if integrator in (0, 1):
        return int(integrator)
    raise ValueError(f"integrator must be 'leapfrog', 'mclachlan', 0 or 1 (got {integrator!r})")


class IntegratorState(NamedTuple):
    position: object
    momentum: object
    logdensity: object
    logdensity_grad: object

    @classmethod
    def from_run(cls, info):
        """The stacked states of a run's kept steps (``inference_loop0``): positions and log-densities; momenta and gradients are not kept."""
        return cls(info.positions, None, info.logdensities, None)


class MCLMCInfo(NamedTuple):
    logdensity: object
    kinetic_change: object
    energy_change: object


class MCLMCRunInfo(NamedTuple):
    """What ``step.run`` reports.  Per chain (float64 / int32 ``[n_chain_local]``): the sums of the steps' energy changes and of their
    squares and the number of steps whose energy change is not finite; ``energy_var_per_dim``, ONE float, the variance of the energy
    change pooled over the chains of all ranks and the steps, divided by ``dim``; with ``thin`` the kept states ``positions
    [num_steps / thin, n_chain, dim]`` / ``logdensities [num_steps / thin, n_chain]`` (``None`` without); ``last``, the final step's
    ``MCLMCInfo`` with ``energy_change`` only; ``energy_changes [num_steps, n_chain]`` with ``keep_energy`` (``None`` without)."""
    energy_change_sum: object
    energy_change_sumsq: object
    num_nonfinite: object
    energy_var_per_dim: float
    positions: object
    logdensities: object
    last: MCLMCInfo
    energy_changes: object


def energy_var_per_dim(de_sum, de_sumsq, num_steps, dim, n_valid=None):
    """The pooled variance of the energy change per dimension from a run's per-chain sums (rows from ``n_valid`` on are padding), the
    three sums going through one all-reduce with more than one rank, as ``mcmc_utils.pooled_step_size``."""
    import torch
    from ...engine import allreduce_sum_
    s1 = de_sum if n_valid is None else de_sum[:int(n_valid)]
    s2 = de_sumsq if n_valid is None else de_sumsq[:int(n_valid)]
    s = torch.stack([s1.sum(), s2.sum(), torch.tensor(float(s1.numel()) * int(num_steps), dtype=torch.float64, device=s1.device)])
    allreduce_sum_(s)
    m = s[0] / s[2]
    return float(((s[1] / s[2] - m * m) / int(dim)).item())


def _target_engine(logdensity_fn):
    dist, beta = resolve_logdensity(logdensity_fn)
    if _is_cox(dist):
        raise ValueError("mclmc is not served on the Cox process: its gradient needs the K^-1 GEMM tile (use hmc or elliptical_slice)")
    eng = _engine(dist)
    eng.ctx.set_inverse_mass(None)            # unit metric: the context may carry a vector from an HMC call
    return eng, beta


def init(position, logdensity_fn: Callable, rng_key) -> IntegratorState:
    """The state at ``position [n_chain_local, dim]`` with unit momenta drawn from ``split(rng_key, n_chain_total)[chain_offset + b]``."""
    eng, beta = _target_engine(logdensity_fn)
    t = eng.torch
    logp = t.empty(position.shape[0], device=position.device, dtype=t.float64)
    grad = t.empty_like(position)
    mom = t.empty(position.shape, device=position.device, dtype=t.float64)
    eng.ctx.mala_init(position, beta, logp, grad)
    eng.ctx.mclmc_init(rng_key, mom)
    return IntegratorState(position, mom, logp, grad)


def build_kernel(integrator="mclachlan"):
    integ = integrator_id(integrator)

    def kernel(rng_key, state: IntegratorState, logdensity_fn: Callable, L: float, step_size: float):
        eng, beta = _target_engine(logdensity_fn)
        t = eng.torch
        pos, mom, logp, grad = (x.clone() for x in state)      # states are values
        de = t.empty(pos.shape[0], device=pos.device, dtype=t.float64)
        dk = t.empty_like(de)
        if getattr(rng_key, "ndim", 1) == 2:
            eng.ctx.mclmc_step_keys(_device_keys(t, rng_key, pos.device), beta, step_size, L, integ, pos, logp, grad, mom, de, dk)
        else:
            eng.ctx.mclmc_step(rng_key, beta, step_size, L, integ, pos, logp, grad, mom, de, dk)
        return IntegratorState(pos, mom, logp, grad), MCLMCInfo(logp, dk, de)

    def run(rng_key, state: IntegratorState, logdensity_fn: Callable, L: float, step_size: float, num_steps: int, thin: int = 0,
            keep_energy: bool = False):
        """``num_steps`` calls of ``kernel`` in one launch; keys as ``hmc``'s ``run`` (one key: step-major; ``[n_chain_local, 2]``:
        chain-major).  ``thin >= 1`` keeps the state after every ``thin``-th step, ``keep_energy`` every step's energy change."""
        eng, beta = _target_engine(logdensity_fn)
        t = eng.torch
        num_steps, thin = int(num_steps), int(thin)
        pos, mom, logp, grad = (x.clone() for x in state)
        n, dev = pos.shape[0], pos.device
        s1 = t.empty(n, device=dev, dtype=t.float64)
        s2 = t.empty(n, device=dev, dtype=t.float64)
        bad = t.empty(n, device=dev, dtype=t.int32)
        trace = t.empty((max(num_steps, 1), n), device=dev, dtype=t.float64) if keep_energy else None
        traj_pos = traj_logp = None
        if thin > 0 and num_steps >= thin and num_steps % thin == 0:       # (anything else: the library names the bad argument)
            traj_pos = t.empty((num_steps // thin,) + tuple(pos.shape), device=dev, dtype=t.float32)
            traj_logp = t.empty((num_steps // thin, n), device=dev, dtype=t.float64)
        if getattr(rng_key, "ndim", 1) == 2:
            rng_key = _device_keys(t, rng_key, dev)
        eng.ctx.mclmc_run(rng_key, beta, step_size, L, integ, num_steps, pos, logp, grad, mom, thin=thin, de_sum=s1, de_sumsq=s2,
                          n_nonfinite=bad, energy_trace=trace, traj_pos=traj_pos, traj_logp=traj_logp)
        v = energy_var_per_dim(s1, s2, num_steps, pos.shape[1], getattr(eng, "n_valid", None))
        info = MCLMCRunInfo(s1, s2, bad, v, traj_pos, traj_logp, MCLMCInfo(logp, None, None if trace is None else trace[-1]), trace)
        return IntegratorState(pos, mom, logp, grad), info

    kernel.run = run
    return kernel


class mclmc:
    init = staticmethod(init)
    build_kernel = staticmethod(build_kernel)

    def __new__(cls, logdensity_fn: Callable, L: float, step_size: float, integrator="mclachlan") -> SamplingAlgorithm:
        kernel = cls.build_kernel(integrator)
        dist = resolve_logdensity(logdensity_fn)[0]
        if _is_cox(dist):
            raise ValueError("mclmc is not served on the Cox process: its gradient needs the K^-1 GEMM tile (use hmc or elliptical_slice)")
        L, step_size = float(L), float(step_size)
        if not (L > 0) or not (step_size > 0) or np.isinf(step_size):
            raise ValueError(f"mclmc needs L > 0 (inf allowed) and a finite step_size > 0 (got L = {L}, step_size = {step_size})")

        def init_fn(position, rng_key):
            return cls.init(position, logdensity_fn, rng_key)

        def step_fn(rng_key, state):
            return kernel(rng_key, state, logdensity_fn, L, step_size)

        def run_fn(rng_key, state, num_steps, thin=0, keep_energy=False):
            return kernel.run(rng_key, state, logdensity_fn, L, step_size, num_steps, thin, keep_energy)

        step_fn.run = run_fn
        return SamplingAlgorithm(init_fn, step_fn)
