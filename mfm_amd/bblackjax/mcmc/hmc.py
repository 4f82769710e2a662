"""Hamiltonian Monte Carlo kernel on MI355X -- a BUILD-SIDE MODE beside ``mala.py``.

BASELINE.json's north star names a "MALA/HMC log-density-and-grad step"; the reference's MFM loop uses MALA only and its vendored
``bblackjax/mcmc`` has no ``hmc.py`` (SURVEY.md note 7), so this module has no counterpart to be a drop-in for.  It follows the kernel of
blackjax (the package ``bblackjax`` was cut from) with the same conventions as ``mala.py`` here: ``state.position`` is
``[n_chain_local, dim]`` (CUDA float32), ``rng_key`` the key BEFORE the per-chain split, ``logdensity_fn`` built from a device target;
velocity Verlet, acceptance ``min(1, exp(H_0 - H_end))`` (``oracle/hmc.py``; device: ``mfm_hmc_step``); unit mass matrix unless
``inverse_mass_matrix`` is given: a vector ``[dim]``, the DIAGONAL of blackjax's ``inverse_mass_matrix`` (momentum
``n / sqrt(minv)``, kinetic energy ``sum(minv p^2) / 2``, drift ``eps minv p``; ``mfm_hmc_set_inverse_mass``).  A call's mass is its
argument, never what an earlier call left on the context: every launch installs or clears it first (the context keeps a host copy and
uploads only a change).  ``adaptation/window_adaptation.py`` estimates one.  As in
``mala.py``, a caller that vmaps over its OWN keys passes ``rng_key`` of shape ``[n_chain_local, 2]`` (``mfm_hmc_step_keys``), and the
kernel carries ``kernel.run(rng_key, state, logdensity_fn, step_size, num_integration_steps, num_steps, thin=0)``: ``num_steps`` HMC
steps in ONE launch (``mfm_hmc_run``) with the chain resident on the device between steps, and ``kernel.warmup(rng_key, state,
logdensity_fn, step_size, num_integration_steps, num_steps, target_acceptance_rate=0.8, keep_step_sizes=False)``: ``num_steps`` HMC
steps in one launch (``mfm_hmc_warmup``) in which every chain adapts its own step size from ``step_size`` by dual averaging towards
the target acceptance probability (Hoffman & Gelman's constants; the recursion: ``include/mfm.h``).

The kernel dispatches by target: the log-Gaussian Cox process (``--example pines``), whose gradient needs the ``K^-1`` GEMM tile, goes
to ``mfm_cox_hmc_step`` / ``_step_keys`` / ``_run`` / ``_warmup`` (``lgcp_hmc.hip``) with the same states and infos; every other
target goes to ``mfm_hmc_*``.  The Cox kernel runs at unit mass and at one leapfrog count: ``inverse_mass_matrix`` or
``num_integration_steps_per_step`` with a Cox target is a ``ValueError`` before any device work."""
from typing import Callable, NamedTuple

import numpy as np

from ...distributions import resolve_logdensity
from ..base import SamplingAlgorithm
from .mala import MALAState as HMCState, _engine, init

__all__ = ["HMCState", "HMCInfo", "HMCRunInfo", "HMCRunLengthsInfo", "HMCWarmupInfo", "init", "build_kernel", "hmc", "check_inverse_mass", "integration_step_counts"]


def check_inverse_mass(inverse_mass_matrix, dim=None):
    """``None``, or the diagonal as a float64 vector; ``ValueError`` for anything that is not a vector of ``dim`` finite, positive
    entries (before any device work)."""
    if inverse_mass_matrix is None:
        return None
    if hasattr(inverse_mass_matrix, "detach"):
        inverse_mass_matrix = inverse_mass_matrix.detach().cpu().numpy()
    v = np.array(inverse_mass_matrix, dtype=np.float64)
    if v.ndim != 1:
        raise ValueError(f"inverse_mass_matrix must be a vector, the diagonal (got shape {v.shape}); dense mass matrices are not served")
    if dim is not None and v.size != int(dim):
        raise ValueError(f"inverse_mass_matrix must have dim = {int(dim)} entries (got {v.size})")
    if not (np.isfinite(v) & (v > 0)).all():
        raise ValueError("inverse_mass_matrix: every entry must be finite and positive")
    return v


class HMCInfo(NamedTuple):
    acceptance_rate: object
    is_accepted: object


class HMCRunInfo(NamedTuple):
    """What ``kernel.run`` reports, field for field ``MALARunInfo``: per chain the mean acceptance probability and the number of
    accepted steps, the LAST step's ``HMCInfo``, and (with ``thin``) the kept states ``positions [num_steps / thin, n_chain, dim]`` /
    ``logdensities [num_steps / thin, n_chain]`` (``None`` without).  ``num_leapfrog`` is an attribute beside the five tuple fields
    (which stay ``MALARunInfo``'s): ``None``, or for a run with ``num_integration_steps_per_step`` (an ``HMCRunLengthsInfo``) the leapfrog
    steps of one chain over the run."""
    acceptance_rate: object
    num_accepted: object
    last: HMCInfo
    positions: object
    logdensities: object
    num_leapfrog = None


class HMCRunLengthsInfo(HMCRunInfo):
    """``HMCRunInfo`` of a run with one leapfrog count per step: the same tuple, and ``num_leapfrog`` (int), their sum."""

    def __new__(cls, acceptance_rate, num_accepted, last, positions, logdensities, num_leapfrog):
        self = super().__new__(cls, acceptance_rate, num_accepted, last, positions, logdensities)
        self.num_leapfrog = num_leapfrog
        return self


class HMCWarmupInfo(NamedTuple):
    """What ``kernel.warmup`` reports.  Per chain (``[n_chain_local]``, float64): ``step_size``, the averaged iterate ``exp(xbar_n)``
    -- the result -- and ``last_step_size`` ``exp(x_n)``; ``pooled_step_size``, ONE float, the geometric mean of ``step_size`` over
    the chains of all ranks without the padding rows (``mcmc_utils.pooled_step_size``); per chain the mean acceptance probability
    over the warmup and the number of accepted steps; ``step_sizes [num_steps, n_chain_local]``, the step size USED at every step
    (``None`` unless asked for)."""
    step_size: object
    last_step_size: object
    pooled_step_size: float
    acceptance_rate: object
    num_accepted: object
    step_sizes: object


def _warmup(call, eng, rng_key, state, num_steps, keep_step_sizes):
    """The buffers of a warmup call, ``call(rng_key, pos, logp, grad, **outputs)``, and its info (shared with ``mala.py``)."""
    from ...mcmc_utils import pooled_step_size
    t = eng.torch
    num_steps = int(num_steps)
    pos, logp, grad = state.position.clone(), state.logdensity.clone(), state.logdensity_grad.clone()      # states are values
    n, dev = pos.shape[0], pos.device
    step_avg = t.empty(n, device=dev, dtype=t.float64)
    step_last = t.empty(n, device=dev, dtype=t.float64)
    n_acc = t.empty(n, device=dev, dtype=t.int32)
    acc_sum = t.empty(n, device=dev, dtype=t.float64)
    traj = t.empty((num_steps, n), device=dev, dtype=t.float64) if keep_step_sizes and num_steps >= 1 else None
    if getattr(rng_key, "ndim", 1) == 2:
        rng_key = _device_keys(t, rng_key, dev)
    call(rng_key, pos, logp, grad, step_avg=step_avg, step_last=step_last, n_acc=n_acc, acc_sum=acc_sum, step_traj=traj)
    return HMCState(pos, logp, grad), HMCWarmupInfo(step_avg, step_last, pooled_step_size(step_avg, eng.n_valid), acc_sum / num_steps, n_acc, traj)


def _device_keys(t, rng_key, dev):
    """Per-chain keys ``[n_chain, 2]`` as the int32 device tensor the library takes (a device tensor passes through)."""
    return rng_key if t.is_tensor(rng_key) else t.as_tensor(np.ascontiguousarray(rng_key, dtype=np.uint32).view(np.int32), device=dev)


def integration_step_counts(per_step, num_steps):
    """``num_integration_steps_per_step`` as an int32 array ``[num_steps]``: an array-like of that length, or a callable ``i -> int``;
    ``ValueError`` for a wrong length or an entry outside [1, 100000] (before any device work)."""
    num_steps = int(num_steps)
    v = [per_step(i) for i in range(num_steps)] if callable(per_step) else per_step
    v = np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v)
    if v.ndim != 1 or v.size != num_steps:
        raise ValueError(f"num_integration_steps_per_step must hold num_steps = {num_steps} counts (got shape {v.shape})")
    if num_steps and not ((v == np.floor(v)) & (v >= 1) & (v <= 100000)).all():
        raise ValueError("num_integration_steps_per_step: every count must be an integer in [1, 100000]")
    return np.ascontiguousarray(v, dtype=np.int32)


def _mass_engine(dist, inverse_mass_matrix):
    """The engine of ``dist`` with this call's mass installed on (or cleared from) its context."""
    minv = check_inverse_mass(inverse_mass_matrix, getattr(dist, "dim", None))
    eng = _engine(dist)
    eng.ctx.set_inverse_mass(minv)
    return eng


def _is_cox(dist):
    return getattr(dist, "kind", None) == "lgcp"


def _cox_engine(dist, inverse_mass_matrix, num_integration_steps_per_step=None):
    """The engine of a Cox process target for the ``cox_hmc_*`` calls; ``ValueError`` (before any device work) for what its kernel
    does not serve.  Unit mass is installed: the context may carry a vector from another call."""
    if inverse_mass_matrix is not None:
        raise ValueError("inverse_mass_matrix is not served on the Cox process: its HMC kernel (mfm_cox_hmc_*) runs at unit mass")
    if num_integration_steps_per_step is not None:
        raise ValueError("num_integration_steps_per_step is not served on the Cox process: mfm_hmc_run_lengths / ChEES have no Cox kernel")
    eng = _engine(dist)
    eng.ctx.set_inverse_mass(None)
    return eng


def build_kernel():
    def kernel(rng_key, state: HMCState, logdensity_fn: Callable, step_size: float, num_integration_steps: int, inverse_mass_matrix=None):
        """One key: chain b draws from ``split(rng_key, n_chain_total)[chain_offset + b]``; keys ``[n_chain_local, 2]``: the caller's
        own vmap, chain b draws from ``rng_key[b]``."""
        dist, beta = resolve_logdensity(logdensity_fn)
        cox = _is_cox(dist)
        eng = _cox_engine(dist, inverse_mass_matrix) if cox else _mass_engine(dist, inverse_mass_matrix)
        step, step_keys = (eng.ctx.cox_hmc_step, eng.ctx.cox_hmc_step_keys) if cox else (eng.ctx.hmc_step, eng.ctx.hmc_step_keys)
        t = eng.torch
        pos, logp, grad = state.position.clone(), state.logdensity.clone(), state.logdensity_grad.clone()      # states are values
        acc = t.empty(pos.shape[0], device=pos.device, dtype=t.float32)
        isacc = t.empty(pos.shape[0], device=pos.device, dtype=t.uint8)
        if getattr(rng_key, "ndim", 1) == 2:
            step_keys(_device_keys(t, rng_key, pos.device), beta, step_size, num_integration_steps, pos, logp, grad, acc, isacc)
        else:
            step(rng_key, beta, step_size, num_integration_steps, pos, logp, grad, acc, isacc)
        return HMCState(pos, logp, grad), HMCInfo(acc, isacc.bool())

    def run(rng_key, state: HMCState, logdensity_fn: Callable, step_size: float, num_integration_steps: int, num_steps: int, thin: int = 0,
            inverse_mass_matrix=None, num_integration_steps_per_step=None):
        """``num_steps`` calls of ``kernel`` in one: with ONE key step j uses ``split(rng_key, num_steps)[j]`` (the scan of
        ``inference_loop0``); with keys ``[n_chain_local, 2]`` step j of chain b uses ``split(rng_key[b], num_steps)[j]``.
        Bit-identical with that loop.  ``thin >= 1`` keeps the state after every ``thin``-th step.
        ``num_integration_steps_per_step`` (array-like of ``num_steps`` ints, or a callable ``i -> int``) gives step j its own number of
        leapfrog steps in place of ``num_integration_steps`` (``mfm_hmc_run_lengths``: the sampler ``chees_adaptation`` adapts)."""
        dist, beta = resolve_logdensity(logdensity_fn)
        cox = _is_cox(dist)
        if cox:
            eng = _cox_engine(dist, inverse_mass_matrix, num_integration_steps_per_step)
        lengths = None if num_integration_steps_per_step is None else integration_step_counts(num_integration_steps_per_step, num_steps)
        if not cox:
            eng = _mass_engine(dist, inverse_mass_matrix)
        t = eng.torch
        num_steps, thin = int(num_steps), int(thin)
        pos, logp, grad = state.position.clone(), state.logdensity.clone(), state.logdensity_grad.clone()
        n, dev = pos.shape[0], pos.device
        n_acc = t.empty(n, device=dev, dtype=t.int32)
        acc_sum = t.empty(n, device=dev, dtype=t.float64)
        acc = t.empty(n, device=dev, dtype=t.float32)
        isacc = t.empty(n, device=dev, dtype=t.uint8)
        traj_pos = traj_logp = None
        if thin > 0 and num_steps >= thin and num_steps % thin == 0:       # (anything else: the library names the bad argument)
            traj_pos = t.empty((num_steps // thin,) + tuple(pos.shape), device=dev, dtype=t.float32)
            traj_logp = t.empty((num_steps // thin, n), device=dev, dtype=t.float64)
        if getattr(rng_key, "ndim", 1) == 2:
            rng_key = _device_keys(t, rng_key, dev)
        if lengths is not None:
            total = t.zeros(1, device=dev, dtype=t.int64)
            eng.ctx.hmc_run_lengths(rng_key, beta, step_size, t.as_tensor(lengths, device=dev), pos, logp, grad, thin=thin, n_acc=n_acc,
                                    acc_sum=acc_sum, acc=acc, is_acc=isacc, traj_pos=traj_pos, traj_logp=traj_logp, total_leapfrog=total)
            return HMCState(pos, logp, grad), HMCRunLengthsInfo(acc_sum / num_steps, n_acc, HMCInfo(acc, isacc.bool()), traj_pos, traj_logp, int(total.item()))
        (eng.ctx.cox_hmc_run if cox else eng.ctx.hmc_run)(rng_key, beta, step_size, num_integration_steps, num_steps, pos, logp, grad, thin=thin,
                                                          n_acc=n_acc, acc_sum=acc_sum, acc=acc, is_acc=isacc, traj_pos=traj_pos, traj_logp=traj_logp)
        return HMCState(pos, logp, grad), HMCRunInfo(acc_sum / num_steps, n_acc, HMCInfo(acc, isacc.bool()), traj_pos, traj_logp)

    def warmup(rng_key, state: HMCState, logdensity_fn: Callable, step_size: float, num_integration_steps: int, num_steps: int,
               target_acceptance_rate: float = 0.8, keep_step_sizes: bool = False, inverse_mass_matrix=None):
        """``num_steps`` HMC steps in one launch, from ``step_size``, every chain adapting its own step size towards
        ``target_acceptance_rate``; keys as ``run``'s (one key: step-major; ``[n_chain_local, 2]``: chain-major).  Returns the state
        after the steps and an ``HMCWarmupInfo``; ``info.pooled_step_size`` is the value to sample with."""
        dist, beta = resolve_logdensity(logdensity_fn)
        cox = _is_cox(dist)
        eng = _cox_engine(dist, inverse_mass_matrix) if cox else _mass_engine(dist, inverse_mass_matrix)
        call = eng.ctx.cox_hmc_warmup if cox else eng.ctx.hmc_warmup
        return _warmup(lambda key, pos, logp, grad, **out: call(key, beta, step_size, num_integration_steps, int(num_steps),
                                                                target_acceptance_rate, pos, logp, grad, **out),
                       eng, rng_key, state, num_steps, keep_step_sizes)

    kernel.run = run
    kernel.warmup = warmup
    return kernel


class hmc:
    init = staticmethod(init)
    build_kernel = staticmethod(build_kernel)

    def __new__(cls, logdensity_fn: Callable, step_size: float, num_integration_steps: int, inverse_mass_matrix=None) -> SamplingAlgorithm:
        kernel = cls.build_kernel()
        dist = resolve_logdensity(logdensity_fn)[0]
        if _is_cox(dist) and inverse_mass_matrix is not None:
            raise ValueError("inverse_mass_matrix is not served on the Cox process: its HMC kernel (mfm_cox_hmc_*) runs at unit mass")
        minv = check_inverse_mass(inverse_mass_matrix, getattr(dist, "dim", None))

        def init_fn(position):
            return cls.init(position, logdensity_fn)

        def step_fn(rng_key, state):
            return kernel(rng_key, state, logdensity_fn, step_size, num_integration_steps, minv)

        def run_fn(rng_key, state, num_steps, thin=0, num_integration_steps_per_step=None):
            return kernel.run(rng_key, state, logdensity_fn, step_size, num_integration_steps, num_steps, thin, minv, num_integration_steps_per_step)

        def warmup_fn(rng_key, state, num_steps, target_acceptance_rate=0.8, keep_step_sizes=False):
            return kernel.warmup(rng_key, state, logdensity_fn, step_size, num_integration_steps, num_steps, target_acceptance_rate, keep_step_sizes, minv)

        step_fn.run = run_fn
        step_fn.warmup = warmup_fn
        return SamplingAlgorithm(init_fn, step_fn)
