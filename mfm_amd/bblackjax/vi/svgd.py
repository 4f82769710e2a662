"""Stein variational gradient descent on MI355X -- drop-in for ``bblackjax/vi/svgd.py``.

Same names and argument meaning as the reference (``SVGDState`` ``:16-19``, ``init`` ``:22-40``, ``build_kernel`` ``:43-91``,
``rbf_kernel`` ``:94-96``, ``update_median_heuristic`` ``:115-124``, ``svgd`` ``:127-168``, ``coin_svgd`` ``:171-216``).  One iteration
is the all-pairs interaction ``mfm_svgd_step`` runs on the device (arithmetic: ``include/mfm.h``).  Differences forced by the C-ABI
boundary, each an error raised BEFORE any device work rather than a fallback:

* ``grad_logdensity_fn`` is whatever ``distributions.resolve_logdensity`` resolves -- ``dist.logprob``, or the tempered closure
  ``lambda x: beta * dist.loglik(x) + dist.logprior(x)`` -- or the ``dist.grad_logprob`` marker (beta = 1); the gradient itself is
  evaluated inside the library.  Anything else: ``NotImplementedError``;
* ``optimizer`` is a descriptor of ``bblackjax.optimizers`` (``sgd`` / ``adagrad`` / ``adam`` / ``cocob``), not an optax closure pair:
  ``TypeError`` otherwise;
* ``kernel`` must be ``rbf_kernel`` and ``update_kernel_parameters`` ``update_median_heuristic`` or ``None`` (a fixed length scale):
  ``NotImplementedError`` otherwise;
* particles are ``[n_chain_local, dim]`` float32 on the device (the engine's ``n_chain_valid`` rows are the particles; padding rows
  stay as they are); more than one rank raises (the library's ``MFM_EUNSUPPORTED``).

States are values: ``step`` never changes its input.  ``kernel_parameters["length_scale"]`` is a float64 device tensor of one element
after the first step (a Python float is accepted going in).  ``step_fn.run(state, num_steps, keep_length_scales=False)`` is
``num_steps`` iterations in ONE library call with the bits of ``num_steps`` calls of ``step_fn``; with ``keep_length_scales`` it returns
``(state, length_scales [num_steps])``, the scale every iteration used.
"""
from typing import Any, Callable, Dict, NamedTuple

from ...distributions import Distribution, resolve_logdensity
from ..base import SamplingAlgorithm
from ..optimizers import check_optimizer
from ..optimizers.cocob import cocob

__all__ = ["SVGDState", "init", "build_kernel", "svgd", "coin_svgd", "rbf_kernel", "update_median_heuristic"]

_last_engine = None        # the engine of the last resolved target: the stand-alone update_median_heuristic launches through its context


class SVGDState(NamedTuple):
    particles: Any
    kernel_parameters: Dict[str, Any]
    opt_state: Any


def init(initial_particles, kernel_parameters: Dict[str, Any], optimizer) -> SVGDState:
    """svgd.py:22-40."""
    return SVGDState(initial_particles, dict(kernel_parameters), check_optimizer(optimizer).init(initial_particles))


def rbf_kernel(x, y, length_scale=1):
    """svgd.py:94-96: ``exp(-(1 / length_scale) * sum((x - y)^2))`` of two device tensors (or anything torch can subtract)."""
    import torch
    x, y = torch.as_tensor(x), torch.as_tensor(y)
    return torch.exp(-(1 / length_scale) * ((x - y) ** 2).sum())


def _resolve(grad_logdensity_fn):
    """(engine, beta) of a target's gradient; NotImplementedError for anything the library cannot evaluate itself."""
    owner = getattr(grad_logdensity_fn, "__self__", None)
    if isinstance(owner, Distribution) and getattr(grad_logdensity_fn, "__name__", "") == "grad_logprob":
        dist, beta = owner, 1.0
    else:
        try:
            dist, beta = resolve_logdensity(grad_logdensity_fn)
        except NotImplementedError:
            raise
        except Exception as err:
            raise NotImplementedError("grad_logdensity_fn must be dist.grad_logprob or be built from dist.loglik / dist.logprior / "
                                      f"dist.logprob of one device target ({type(err).__name__}: {err})") from err
    return dist, float(beta)


def _engine(dist):
    global _last_engine
    if dist._engine is None:
        raise RuntimeError("attach the distribution to a device engine first (mfm_amd.engine.Engine(dist, args))")
    _last_engine = dist._engine
    return dist._engine


def _length_scale_tensor(t, kernel_parameters, dev):
    ls = kernel_parameters["length_scale"]
    if t.is_tensor(ls):
        return ls.to(device=dev, dtype=t.float64).reshape(1).clone()
    return t.full((1,), float(ls), device=dev, dtype=t.float64)


def _open_engine(particles):
    """The engine the stand-alone pieces launch through: the one last resolved, if its context is still open and lives on the particles'
    device.  Anything else raises -- a closed or foreign context is never used."""
    eng = _last_engine
    if eng is None:
        raise RuntimeError("update_median_heuristic launches through a device engine: create one (mfm_amd.engine.Engine) and resolve a target first")
    if not getattr(eng.ctx, "h", None):
        raise RuntimeError("update_median_heuristic: the engine of the last resolved target has been closed; resolve a target of an open engine first")
    if not getattr(particles, "is_cuda", False) or particles.device != eng.dev:
        raise RuntimeError(f"update_median_heuristic: particles must be a device tensor on {eng.dev}, the device of the last resolved target's engine")
    return eng


def update_median_heuristic(state: SVGDState) -> SVGDState:
    """svgd.py:99-124 on the device: ``length_scale = median(pairwise distances)^2 / log n`` of ``state.particles`` (every row).  The
    two launches are free-shape and read nothing of a target, so they go through the engine of the LAST resolved target (``svgd(...)``'s
    steps run the heuristic inside ``mfm_svgd_step`` on their own engine instead)."""
    eng = _open_engine(state.particles)
    t = eng.torch
    if state.particles.ndim != 2 or state.particles.dtype != t.float32:
        raise ValueError(f"update_median_heuristic: particles must be float32 [n, dim] (got {state.particles.dtype} {tuple(state.particles.shape)})")
    x = state.particles.contiguous()
    D = t.empty((x.shape[0], x.shape[0]), device=x.device, dtype=t.float32)
    ls = t.empty(1, device=x.device, dtype=t.float64)
    eng.ctx.svgd_sqdist(x, D)
    eng.ctx.svgd_median(D, ls)
    return SVGDState(state.particles, {**state.kernel_parameters, "length_scale": ls}, state.opt_state)


def _check_state(eng, particles, arrays):
    """The library takes raw pointers to ``[n_chain_local, dim]`` float32 rows: anything else would be read and written out of bounds."""
    t = eng.torch
    want = (eng.n_local, eng.dim)
    for name, a in [("particles", particles)] + [(f"opt_state[{i}]", a) for i, a in enumerate(arrays)]:
        if not t.is_tensor(a) or not a.is_cuda or a.dtype != t.float32 or tuple(a.shape) != want:
            raise ValueError(f"svgd: {name} must be a float32 device tensor of shape [n_chain_local, dim] = {list(want)} "
                             f"(got {getattr(a, 'dtype', type(a).__name__)} {tuple(getattr(a, 'shape', ()))})")


def _check_plugins(kernel, update_kernel_parameters):
    if kernel is not rbf_kernel:
        raise NotImplementedError("kernel must be mfm_amd.bblackjax.vi.svgd.rbf_kernel (the device evaluates the RBF kernel only)")
    if update_kernel_parameters is not None and update_kernel_parameters is not update_median_heuristic:
        raise NotImplementedError("update_kernel_parameters must be update_median_heuristic or None (a fixed length scale)")


def build_kernel(optimizer):
    """svgd.py:43-91; the returned kernel also takes ``update_kernel_parameters`` (the reference applies it in ``step_fn``, ``:164-166``;
    here it is part of the same library call) and carries ``kernel.run``."""
    opt = check_optimizer(optimizer)

    def run(state: SVGDState, grad_logdensity_fn: Callable, kernel: Callable = rbf_kernel, num_steps: int = 1,
            update_kernel_parameters=update_median_heuristic, keep_length_scales: bool = False):
        _check_plugins(kernel, update_kernel_parameters)
        dist, beta = _resolve(grad_logdensity_fn)
        eng = _engine(dist)
        t = eng.torch
        particles, kernel_params, opt_state = state
        *arrays, count = opt_state
        _check_state(eng, particles, arrays)
        x = particles.contiguous().clone()                                  # states are values
        arrays = [a.contiguous().clone() for a in arrays]
        ls = _length_scale_tensor(t, kernel_params, x.device)
        used = t.empty(int(num_steps), device=x.device, dtype=t.float64) if keep_length_scales and int(num_steps) >= 1 else None
        eng.ctx.svgd_step(beta, opt.kind, opt.hyper, int(count), int(num_steps), x, arrays, ls,
                          update_median=update_kernel_parameters is not None, ls_used=used)
        new = SVGDState(x, {**kernel_params, "length_scale": ls}, tuple(arrays) + (int(count) + int(num_steps),))
        return (new, used) if keep_length_scales else new

    def kernel(state: SVGDState, grad_logdensity_fn: Callable, kernel: Callable = rbf_kernel, update_kernel_parameters=None) -> SVGDState:
        """One step WITHOUT the kernel-parameter update unless one is given (svgd.py:71-89 leaves ``kernel_params`` as they are)."""
        return run(state, grad_logdensity_fn, kernel, 1, update_kernel_parameters)

    kernel.run = run
    return kernel


def _algorithm(cls, grad_logdensity_fn, optimizer, kernel, update_kernel_parameters):
    _check_plugins(kernel, update_kernel_parameters)
    _resolve(grad_logdensity_fn)                                            # unresolvable targets raise here, before any device work
    kernel_ = cls.build_kernel(optimizer)

    def init_fn(initial_position, kernel_parameters: Dict[str, Any] = {"length_scale": 1.0}):
        return cls.init(initial_position, kernel_parameters, optimizer)

    def step_fn(state):
        return kernel_(state, grad_logdensity_fn, kernel, update_kernel_parameters)

    def run_fn(state, num_steps, keep_length_scales=False):
        return kernel_.run(state, grad_logdensity_fn, kernel, num_steps, update_kernel_parameters, keep_length_scales)

    step_fn.run = run_fn
    return SamplingAlgorithm(init_fn, step_fn)


class svgd:
    """svgd.py:127-168."""
    init = staticmethod(init)
    build_kernel = staticmethod(build_kernel)

    def __new__(cls, grad_logdensity_fn: Callable, optimizer, kernel: Callable = rbf_kernel,
                update_kernel_parameters: Callable = update_median_heuristic):
        return _algorithm(cls, grad_logdensity_fn, check_optimizer(optimizer), kernel, update_kernel_parameters)


class coin_svgd:
    """svgd.py:171-216: SVGD on the COCOB optimizer (Sharrock & Nemeth 2023, algorithm 6)."""
    init = staticmethod(init)
    build_kernel = staticmethod(build_kernel)

    def __new__(cls, grad_logdensity_fn: Callable, kernel: Callable = rbf_kernel,
                update_kernel_parameters: Callable = update_median_heuristic, *, alpha: float = 100):
        return _algorithm(cls, grad_logdensity_fn, cocob(alpha), kernel, update_kernel_parameters)
