"""``mcmc_utils.py:11-25``: run an MCMC kernel ``n_iter`` times and keep the trajectory.

The reference scans ``kernel(key, state)`` over ``split(rng, n_iter)`` and returns the stacked ``(states, info)``.  Here a kernel
that carries ``.run`` (``mala(logdensity_fn, step_size).step``, ``bblackjax/mcmc/mala.py``) does the whole scan in ONE library
call (``mfm_mala_run`` with ``thin = 1``: the chains stay on the device between steps, same keys, same bits as the loop); any
other kernel is looped on the host.  (The sample-quality metrics of the reference's module are ``Context.stein_disc`` /
``Context.max_mean_disc``.)
"""
from . import random as jr

__all__ = ["inference_loop0"]


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
    per-step gradients are not kept (``states.logdensity_grad is None``) and ``info`` is the run's ``MALARunInfo`` (acceptance
    per chain over the run, the last step's ``MALAInfo``) rather than ``n_iter`` stacked infos."""
    n_iter = int(n_iter)
    run = getattr(kernel, "run", None)
    if run is not None:
        _, info = run(rng, init_state, n_iter, thin=1)
        return type(init_state)(info.positions, info.logdensities, None), info
    if n_iter < 1:
        raise ValueError(f"n_iter must be at least 1 (got {n_iter})")
    keys = jr.split(rng, n_iter)
    state, states, infos = init_state, [], []
    for j in range(n_iter):
        state, info = kernel(keys[j], state)
        states.append(state)
        infos.append(info)
    return _stack(states), _stack(infos)
