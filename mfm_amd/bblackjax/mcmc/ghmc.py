"""Generalized HMC with persistent momentum on MI355X -- ``blackjax.ghmc``, a BUILD-SIDE MODE beside ``hmc.py`` / ``mclmc.py``.

Horowitz's (1991) sampler with the non-reversible slice accept, as Hoffman & Sountsov (2022, MEADS) run it: a transition is ALWAYS one
leapfrog step -- as cheap and as uniform across chains as a MALA step -- the momentum is refreshed only partially
(``p <- sqrt(1 - alpha) p + sqrt(alpha) n / sqrt(minv)``) and so persists across transitions, a rejection negates it, and the accept test
compares a slice variable ``s`` in (-1, 1), drifting by ``delta`` per transition, against ``exp(-dH)``; the sampler is exact.
``tests/ghmc_ref.py`` restates the transition in float64; the device kernels are ``mfm_ghmc_*`` (``csrc/ghmc.hip``).

Conventions as ``hmc.py``: ``state.position`` is ``[n_chain_local, dim]`` (CUDA float32), ``state.momentum`` ``[n_chain_local, dim]`` and
``state.slice`` ``[n_chain_local]`` float64, ``rng_key`` the key BEFORE the per-chain split (keys ``[n_chain_local, 2]``: the caller's own
vmap, ``mfm_ghmc_step_keys``), states are values.  ``momentum_inverse_scale`` is blackjax's: a vector sigma ``[dim]`` with
``minv = sigma^2`` the diagonal inverse mass (``None``: unit metric).  It is the CALL's mass: the inverse mass an ``hmc`` call left on the
context is not read.  ``algo.step.run(rng_key, state, num_steps, thin=0)`` is ``num_steps`` transitions in ONE launch (``mfm_ghmc_run``),
bit-identical with the loop, and ``inference_loop0`` picks it up.  phi-four and mixture targets: the Cox process is a ``ValueError``
before any device work."""
from typing import Callable, NamedTuple

import numpy as np

from ...distributions import resolve_logdensity
from ..base import SamplingAlgorithm
from .hmc import _device_keys, _is_cox, check_inverse_mass
from .mala import _engine

__all__ = ["GHMCState", "GHMCInfo", "GHMCRunInfo", "init", "build_kernel", "ghmc", "check_parameters"]


class GHMCState(NamedTuple):
    position: object
    momentum: object
    logdensity: object
    logdensity_grad: object
    slice: object

    @classmethod
    def from_run(cls, info):
        """The stacked states of a run's kept steps (``inference_loop0``): positions and log-densities; the rest is not kept."""
        return cls(info.positions, None, info.logdensities, None, None)


class GHMCInfo(NamedTuple):
    acceptance_rate: object
    is_accepted: object
    energy_change: object


class GHMCRunInfo(NamedTuple):
    """What ``step.run`` reports, the shape of ``HMCRunInfo`` plus one field: per chain the mean acceptance rate and the number of
    accepted transitions, the LAST transition's ``GHMCInfo``, (with ``thin``) the kept states ``positions [num_steps / thin, n_chain,
    dim]`` / ``logdensities [num_steps / thin, n_chain]`` (``None`` without), and ``energy_change_sum``, per chain the sum of ``dH``
    over the accepted transitions."""
    acceptance_rate: object
    num_accepted: object
    last: GHMCInfo
    positions: object
    logdensities: object
    energy_change_sum: object


def check_parameters(step_size, alpha, delta):
    """``(step_size, alpha, delta)`` as floats, ``delta`` defaulting to ``alpha / 2``; ``ValueError`` for what ``mfm_ghmc_step`` refuses."""
    step_size, alpha = float(step_size), float(alpha)
    delta = alpha / 2.0 if delta is None else float(delta)
    if not (step_size > 0) or np.isinf(step_size):
        raise ValueError(f"ghmc needs a finite step_size > 0 (got {step_size})")
    if not (0 < alpha <= 1):
        raise ValueError(f"ghmc needs alpha in (0, 1] (got {alpha})")
    if not (delta >= 0) or np.isinf(delta):
        raise ValueError(f"ghmc needs a finite delta >= 0 (got {delta})")
    return step_size, alpha, delta


def _refuse_cox(dist):
    if _is_cox(dist):
        raise ValueError("ghmc is not served on the Cox process: its gradient needs the K^-1 GEMM tile (use hmc or elliptical_slice)")


def _target_engine(logdensity_fn):
    dist, beta = resolve_logdensity(logdensity_fn)
    _refuse_cox(dist)
    return _engine(dist), beta


def _inverse_mass(eng, dist, momentum_inverse_scale, device):
    """sigma -> the float64 device vector ``sigma^2`` (``None``: unit metric).  A float64 device tensor passes through squared."""
    if momentum_inverse_scale is None:
        return None
    t = eng.torch
    if t.is_tensor(momentum_inverse_scale) and momentum_inverse_scale.is_cuda:
        s = momentum_inverse_scale.to(t.float64)
        if s.ndim != 1 or (getattr(dist, "dim", None) is not None and s.numel() != int(dist.dim)):
            raise ValueError(f"momentum_inverse_scale must be a vector of dim entries (got shape {tuple(s.shape)})")
        return (s * s).contiguous()
    s = check_inverse_mass(momentum_inverse_scale, getattr(dist, "dim", None))      # (a vector of finite, positive entries)
    return t.as_tensor(s * s, device=device)


def init(position, logdensity_fn: Callable, rng_key, momentum_inverse_scale=None) -> GHMCState:
    """The state at ``position [n_chain_local, dim]`` with momenta ``n / sigma`` and slice variables ``2 u - 1`` drawn from
    ``split(rng_key, n_chain_total)[chain_offset + b]``."""
    eng, beta = _target_engine(logdensity_fn)
    t = eng.torch
    minv = _inverse_mass(eng, resolve_logdensity(logdensity_fn)[0], momentum_inverse_scale, position.device)
    logp = t.empty(position.shape[0], device=position.device, dtype=t.float64)
    grad = t.empty_like(position)
    mom = t.empty(position.shape, device=position.device, dtype=t.float64)
    s = t.empty(position.shape[0], device=position.device, dtype=t.float64)
    eng.ctx.mala_init(position, beta, logp, grad)
    eng.ctx.ghmc_init(rng_key, mom, s, minv)
    return GHMCState(position, mom, logp, grad, s)


def build_kernel():
    def kernel(rng_key, state: GHMCState, logdensity_fn: Callable, step_size: float, alpha: float, delta: float = None, momentum_inverse_scale=None):
        eng, beta = _target_engine(logdensity_fn)
        t = eng.torch
        step_size, alpha, delta = check_parameters(step_size, alpha, delta)
        pos, mom, logp, grad, s = (x.clone() for x in state)      # states are values
        minv = _inverse_mass(eng, resolve_logdensity(logdensity_fn)[0], momentum_inverse_scale, pos.device)
        n, dev = pos.shape[0], pos.device
        acc = t.empty(n, device=dev, dtype=t.float32)
        isacc = t.empty(n, device=dev, dtype=t.uint8)
        de = t.empty(n, device=dev, dtype=t.float64)
        if getattr(rng_key, "ndim", 1) == 2:
            eng.ctx.ghmc_step_keys(_device_keys(t, rng_key, dev), beta, step_size, alpha, delta, pos, logp, grad, mom, s, minv, acc, isacc, de)
        else:
            eng.ctx.ghmc_step(rng_key, beta, step_size, alpha, delta, pos, logp, grad, mom, s, minv, acc, isacc, de)
        return GHMCState(pos, mom, logp, grad, s), GHMCInfo(acc, isacc.bool(), de)

    def run(rng_key, state: GHMCState, logdensity_fn: Callable, step_size: float, alpha: float, delta: float, num_steps: int, thin: int = 0,
            momentum_inverse_scale=None):
        """``num_steps`` calls of ``kernel`` in one launch; keys as ``hmc``'s ``run`` (one key: step-major; ``[n_chain_local, 2]``:
        chain-major).  ``thin >= 1`` keeps the state after every ``thin``-th transition."""
        eng, beta = _target_engine(logdensity_fn)
        t = eng.torch
        step_size, alpha, delta = check_parameters(step_size, alpha, delta)
        num_steps, thin = int(num_steps), int(thin)
        pos, mom, logp, grad, s = (x.clone() for x in state)
        minv = _inverse_mass(eng, resolve_logdensity(logdensity_fn)[0], momentum_inverse_scale, pos.device)
        n, dev = pos.shape[0], pos.device
        n_acc = t.empty(n, device=dev, dtype=t.int32)
        acc_sum = t.empty(n, device=dev, dtype=t.float64)
        de_sum = t.empty(n, device=dev, dtype=t.float64)
        acc = t.empty(n, device=dev, dtype=t.float32)
        isacc = t.empty(n, device=dev, dtype=t.uint8)
        de = t.empty(n, device=dev, dtype=t.float64)
        traj_pos = traj_logp = None
        if thin > 0 and num_steps >= thin and num_steps % thin == 0:       # (anything else: the library names the bad argument)
            traj_pos = t.empty((num_steps // thin,) + tuple(pos.shape), device=dev, dtype=t.float32)
            traj_logp = t.empty((num_steps // thin, n), device=dev, dtype=t.float64)
        if getattr(rng_key, "ndim", 1) == 2:
            rng_key = _device_keys(t, rng_key, dev)
        eng.ctx.ghmc_run(rng_key, beta, step_size, alpha, delta, num_steps, pos, logp, grad, mom, s, minv, thin=thin, n_acc=n_acc, acc_sum=acc_sum,
                         energy_sum=de_sum, acc=acc, is_acc=isacc, energy_change=de, traj_pos=traj_pos, traj_logp=traj_logp)
        info = GHMCRunInfo(acc_sum / num_steps, n_acc, GHMCInfo(acc, isacc.bool(), de), traj_pos, traj_logp, de_sum)
        return GHMCState(pos, mom, logp, grad, s), info

    kernel.run = run
    return kernel


class ghmc:
    init = staticmethod(init)
    build_kernel = staticmethod(build_kernel)

    def __new__(cls, logdensity_fn: Callable, step_size: float, alpha: float, delta: float = None, momentum_inverse_scale=None) -> SamplingAlgorithm:
        kernel = cls.build_kernel()
        _refuse_cox(resolve_logdensity(logdensity_fn)[0])
        step_size, alpha, delta = check_parameters(step_size, alpha, delta)
        if momentum_inverse_scale is not None and not hasattr(momentum_inverse_scale, "is_cuda"):
            check_inverse_mass(momentum_inverse_scale, getattr(resolve_logdensity(logdensity_fn)[0], "dim", None))

        def init_fn(position, rng_key):
            return cls.init(position, logdensity_fn, rng_key, momentum_inverse_scale)

        def step_fn(rng_key, state):
            return kernel(rng_key, state, logdensity_fn, step_size, alpha, delta, momentum_inverse_scale)

        def run_fn(rng_key, state, num_steps, thin=0):
            return kernel.run(rng_key, state, logdensity_fn, step_size, alpha, delta, num_steps, thin, momentum_inverse_scale)

        step_fn.run = run_fn
        return SamplingAlgorithm(init_fn, step_fn)
