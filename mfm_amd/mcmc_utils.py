"""``mcmc_utils.py:11-25``: run an MCMC kernel ``n_iter`` times and keep the trajectory.

The reference scans ``kernel(key, state)`` over ``split(rng, n_iter)`` and returns the stacked ``(states, info)``.  Here a kernel
that carries ``.run`` (``mala(logdensity_fn, step_size).step``, ``bblackjax/mcmc/mala.py``; ``hmc(logdensity_fn, step_size, L).step``,
``bblackjax/mcmc/hmc.py``) does the whole scan in ONE library call (``mfm_mala_run`` / ``mfm_hmc_run`` with ``thin = 1``: the
chains stay on the device between steps, same keys, same bits as the loop); any other kernel is looped on the host.  (The
sample-quality metrics of the reference's module are ``Context.stein_disc`` / ``Context.max_mean_disc``.)

``mcmc_utils.py:131-165``: ``autocorrelation`` of a trajectory along one axis, and -- not in the reference, from the same lag sums --
``effective_sample_size`` (Geyer's initial positive sequence).  Both run on the device (``mfm_autocorr``, ``csrc/diag.hip``): direct
lag sums with one lane per series, no FFT and no copy of the trajectory.
"""
from . import random as jr

__all__ = ["inference_loop", "inference_loop0", "autocorrelation", "effective_sample_size"]


def _stack(items):
    """Stack a list of equally structured results along a new leading axis: tuples (named or not), lists and dicts leaf by leaf,
    ``None`` stays ``None``, device tensors stay on the device."""
    first = items[0]
    if first is None:
        return None
    if isinstance(first, tuple) and hasattr(first, "_fields"):
        return type(first)(*(_stack([it[i] for it in items]) for i in range(len(first))))
    if isinstance(first, (tuple, list)):
        return type(first)(_stack([it[i] for it in items]) for i in range(len(first)))
    if isinstance(first, dict):
        return {k: _stack([it[k] for it in items]) for k in first}
    if type(first).__module__.split(".")[0] == "torch":
        import torch
        return torch.stack(list(items))
    import numpy as np
    return np.stack([np.asarray(it) for it in items])


def inference_loop0(rng, init_state, kernel, n_iter):
    """``states, info = inference_loop0(rng, init_state, kernel, n_iter)`` with ``kernel(key, state) -> (state, info)``.

    ``states`` holds the state AFTER each of the ``n_iter`` steps along a leading axis.  With a kernel that carries ``.run`` the
    per-step gradients are not kept (``states.logdensity_grad is None``) and ``info`` is the run's ``MALARunInfo`` / ``HMCRunInfo``
    (acceptance per chain over the run, the last step's ``MALAInfo`` / ``HMCInfo``; any tuple with ``positions`` and
    ``logdensities`` serves) rather than ``n_iter`` stacked infos.  The stacked states are ``type(init_state)(positions, logdensities,
    None)``, the three fields of ``MALAState``; a state type with other fields gives a classmethod ``from_run(info)`` that builds them
    (``mclmc``'s four-field ``IntegratorState``: positions and log-densities, momenta and gradients ``None``)."""
    n_iter = int(n_iter)
    run = getattr(kernel, "run", None)
    if run is not None:
        _, info = run(rng, init_state, n_iter, thin=1)
        from_run = getattr(type(init_state), "from_run", None)      # (a state with more fields than MALAState's three builds itself: mclmc's IntegratorState)
        return (from_run(info) if from_run else type(init_state)(info.positions, info.logdensities, None)), info
    if n_iter < 1:
        raise ValueError(f"n_iter must be at least 1 (got {n_iter})")
    keys = jr.split(rng, n_iter)
    state, states, infos = init_state, [], []
    for j in range(n_iter):
        state, info = kernel(keys[j], state)
        states.append(state)
        infos.append(info)
    return _stack(states), _stack(infos)


def inference_loop(rng, init_state, kernel, n_iter, param):
    """``mcmc_utils.py:11-17``: ``inference_loop0`` for a kernel that takes a parameter, ``kernel(key, state, param) -> (state, info)``
    (the same ``param`` at every step), looped on the host over ``split(rng, n_iter)``."""
    n_iter = int(n_iter)
    if n_iter < 1:
        raise ValueError(f"n_iter must be at least 1 (got {n_iter})")
    keys = jr.split(rng, n_iter)
    state, states, infos = init_state, [], []
    for j in range(n_iter):
        state, info = kernel(keys[j], state, param)
        states.append(state)
        infos.append(info)
    return _stack(states), _stack(infos)


def pooled_step_size(step_size, n_valid=None):
    """The one step size a warmup's per-chain results stand for: ``exp(mean(log step_size[:n_valid]))``, the geometric mean over the
    chains of ALL ranks (``kernel.warmup`` of ``bblackjax/mcmc/hmc.py`` / ``mala.py``; rows from ``n_valid`` on are padding and are
    left out).  With more than one rank the sum of the logs and the count go through the default process group in one all-reduce
    (``engine.allreduce_sum_``, the group of the engine's all-gathers), so every rank holds the same float.  ``step_size``: a
    float64 tensor ``[n_chain_local]`` on the device or on the CPU."""
    import torch
    from .engine import allreduce_sum_
    x = step_size if n_valid is None else step_size[:int(n_valid)]
    s = torch.stack([x.double().log().sum(), torch.tensor(float(x.numel()), dtype=torch.float64, device=x.device)])
    allreduce_sum_(s)
    return float(torch.exp(s[0] / s[1]).item())


_diag = None


def _diag_ctx(ctx=None):
    """The context the diagnostics run on: the caller's, or a minimal one of this module's own (``mfm_autocorr`` needs no target, no
    Fourier block and no parameters), created at the first call and bound to the current stream at every call."""
    global _diag
    if ctx is None:
        if _diag is None or not _diag.h:
            from . import _lib
            _diag = _lib.Context(dim=2, n_chain_local=16, fourier_dim=16, hidden_t=(16, 16), hidden_x=(16, 16), hidden_xt=(16, 16))
        ctx = _diag
        ctx.use_current_stream()
    return ctx


def _device_f32(x, axis):
    """``x`` as a contiguous float32 CUDA tensor with ``axis`` in front (no copy for such a tensor with ``axis = 0``), and whether it
    came as a host array."""
    import torch
    host = not torch.is_tensor(x)
    if host:
        import numpy as np
        x = torch.as_tensor(np.ascontiguousarray(np.moveaxis(np.asarray(x), axis, 0), dtype=np.float32)).cuda()
    else:
        if not x.is_cuda:
            x = x.cuda()
        x = x.movedim(axis, 0).to(torch.float32).contiguous()
    return x, host


def autocorrelation(x, axis=0, ctx=None):
    """``mcmc_utils.py:131-165``: the autocorrelation of ``x`` along ``axis``, same shape in and out, AS WRITTEN there: the lag sums
    ``A_k = sum_t c_t c_{t+k}`` of the centred signal divided by ``A_0`` and then by 2, so lag 0 is 0.5 (exactly: the halving happens
    here).  A constant series gives NaN (the reference's 0 / 0).  A CUDA tensor with ``axis = 0`` goes to the kernel as it is, any
    other axis is moved to the front with one ``.contiguous()``; a numpy array is uploaded and a numpy array comes back.  Computed
    from the float32 values of ``x`` (float32 products, float64 across blocks of time steps); the reference works in float64."""
    import torch
    xs, host = _device_f32(x, axis)
    rho = torch.empty_like(xs)
    if xs.numel():
        _diag_ctx(ctx).autocorr(xs, rho=rho)
        rho *= 0.5
    out = rho.movedim(0, axis)
    return out.cpu().numpy() if host else out


def effective_sample_size(positions, max_lag=None, ctx=None):
    """``(ess, tau)`` of a trajectory ``positions [n, n_chain, dim]`` (time first; each of shape ``[n_chain, dim]``, float32): Geyer's
    initial-positive-sequence estimate ``tau = -1 + 2 sum_m (rho_2m + rho_2m+1)`` over the leading run of positive pair sums among the
    first ``max_lag`` lags (default: all ``n``), ``ess = n / tau``.  No ``[max_lag, n_chain, dim]`` array is formed."""
    import torch
    xs, host = _device_f32(positions, 0)
    n = xs.shape[0]
    tau = torch.empty(xs.shape[1:], device=xs.device, dtype=torch.float32)
    ess = torch.empty_like(tau)
    _diag_ctx(ctx).autocorr(xs, n_lags=n if max_lag is None else int(max_lag), tau=tau, ess=ess)
    return (ess.cpu().numpy(), tau.cpu().numpy()) if host else (ess, tau)
