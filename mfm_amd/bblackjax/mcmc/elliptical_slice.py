"""Elliptical slice sampling (Murray, Adams & MacKay 2010) on MI355X -- a BUILD-SIDE MODE beside ``hmc.py`` / ``nuts.py``, after
blackjax's ``elliptical_slice(loglikelihood_fn, *, mean, cov)``.

The sampler for a latent Gaussian model: no step size, no gradient, every transition moves.  It serves the one built target with a
Gaussian prior factor, the log-Gaussian Cox process (``--example pines``), which the HMC / NUTS / ChEES / parallel-tempering kernels
refuse.  The reference vendors the same sampler as ``bblackjax/mcmc/tess.py``: under the linear transport ``T(u) = mu + L u`` its
log-det is constant and ``|u|^2 + |m|^2`` is constant on the ellipse, so its slice test (``tess.py:42-44``) compares log-likelihoods
alone -- this module is ``tess`` under that transport (``include/mfm.h`` states the transition, ``tests/eslice_ref.py`` restates it).

* ``loglikelihood_fn`` is built from ``dist.loglik`` of the Cox process, e.g. ``lambda x: beta * dist.loglik(x)``; a prior term, a
  distribution without a prior factor or an arbitrary closure raise ``NotImplementedError`` (no CPU fallback);
* the Gaussian is the distribution's own prior ``N(dist.mu, dist.gram)``, so ``mean`` / ``cov`` other than ``None`` raise; its
  Cholesky factor ``dist.chol`` is installed on the device at first use (``mfm_set_lgcp_chol``);
* ``state.position`` is ``[n_chain_local, dim]`` (CUDA float32); ``state.logdensity`` is the library's state, the UNTEMPERED
  log-likelihood ``dist.loglik(position)`` in float64 (``loglikelihood_fn`` itself at ``beta = 1``);
* ``rng_key`` of shape ``[n_chain, 2]`` selects the per-chain-key calls, as in ``mala.py`` / ``hmc.py``;
* ``step.run(rng_key, state, num_steps, thin=0)``: ``num_steps`` transitions in ONE launch (``mfm_eslice_run``), bit-identical with
  the loop over ``split(rng_key, num_steps)``; ``mcmc_utils.inference_loop0`` picks it up.
"""
from typing import Callable, NamedTuple

import numpy as np

from ...distributions import LogDensityExpr, Sym
from ..base import SamplingAlgorithm
from .mala import _engine

__all__ = ["EllipSliceState", "EllipSliceInfo", "EllipSliceRunInfo", "init", "build_kernel", "elliptical_slice", "resolve_loglikelihood"]


class EllipSliceState(NamedTuple):
    position: object
    logdensity: object
    logdensity_grad: object = None      # always None (the sampler uses no gradient): the slot inference_loop0 fills with None


class EllipSliceInfo(NamedTuple):
    """``momentum [n_chain, dim]``: the auxiliary prior draw ``nu = L n`` about the mean; ``theta [n_chain]`` float64: the last angle
    evaluated (the accepted one unless the chain was capped); ``subiter [n_chain]`` int32: the likelihood evaluations made."""
    momentum: object
    theta: object
    subiter: object


class EllipSliceRunInfo(NamedTuple):
    """``mean_subiter [n_chain]``: likelihood evaluations per transition; ``max_subiter [n_chain]``: the most any one transition made; ``num_capped [n_chain]``: transitions that reached the
    iteration cap and kept their state; with ``thin`` the kept ``positions [num_steps / thin, n_chain, dim]`` / ``logdensities
    [num_steps / thin, n_chain]`` (``None`` without); ``last``: the last transition's ``EllipSliceInfo``."""
    mean_subiter: object
    num_capped: object
    positions: object
    logdensities: object
    last: object
    max_subiter: object = None


def resolve_loglikelihood(fn):
    """Evaluate a ``loglikelihood_fn`` on a placeholder -> ``(dist, beta)`` with ``fn = beta * dist.loglik``."""
    e = fn if isinstance(fn, LogDensityExpr) else fn(Sym())
    if not isinstance(e, LogDensityExpr):
        raise NotImplementedError("loglikelihood_fn must be built from dist.loglik of the Cox process (no CPU fallback)")
    if not e.dist.has_prior:
        raise NotImplementedError(f"elliptical slice sampling needs a Gaussian prior factor: {type(e.dist).__name__} has none "
                                  "(only the log-Gaussian Cox process does)")
    if e.prior_coef != 0.0:
        raise NotImplementedError(f"loglikelihood_fn carries the prior with coefficient {e.prior_coef:g}: the Gaussian prior is the "
                                  "sampler's own ellipse, pass the likelihood alone (beta * dist.loglik)")
    return e.dist, e.lik_coef


def _attach(dist):
    """The engine of ``dist`` with the prior's Cholesky factor installed on its context (once per context)."""
    eng = _engine(dist)
    if getattr(eng.ctx, "_eslice_chol_of", None) is not dist:
        eng.ctx.set_lgcp_chol(dist.chol)
        eng.ctx._eslice_chol_of = dist
    return eng


def _keys_tensor(t, rng_key, dev):
    if getattr(rng_key, "ndim", 1) == 2 and not t.is_tensor(rng_key):
        return t.as_tensor(np.ascontiguousarray(rng_key, dtype=np.uint32).view(np.int32), device=dev)
    return rng_key


def init(position, loglikelihood_fn: Callable) -> EllipSliceState:
    dist, _ = resolve_loglikelihood(loglikelihood_fn)
    eng = _attach(dist)
    t = eng.torch
    if position.ndim != 2:
        raise NotImplementedError("elliptical_slice takes the batched state [n_chain_local, dim]")
    ll = t.empty(position.shape[0], device=position.device, dtype=t.float64)
    eng.ctx.eslice_init(position, ll)
    return EllipSliceState(position, ll)


def build_kernel():
    def kernel(rng_key, state: EllipSliceState, loglikelihood_fn: Callable):
        """One transition.  ONE key: chain b draws from ``split(rng_key, n_chain_total)[chain_offset + b]``; keys ``[n_chain_local, 2]``:
        the caller's own."""
        dist, beta = resolve_loglikelihood(loglikelihood_fn)
        eng = _attach(dist)
        t = eng.torch
        pos, ll = state.position.clone(), state.logdensity.clone()
        n, dev = pos.shape[0], pos.device
        sub = t.empty(n, device=dev, dtype=t.int32)
        theta = t.empty(n, device=dev, dtype=t.float64)
        mom = t.empty_like(pos)
        rng_key = _keys_tensor(t, rng_key, dev)
        if getattr(rng_key, "ndim", 1) == 2:
            eng.ctx.eslice_step_keys(rng_key, beta, pos, ll, sub, theta, mom)
        else:
            eng.ctx.eslice_step(rng_key, beta, pos, ll, sub, theta, mom)
        return EllipSliceState(pos, ll), EllipSliceInfo(mom, theta, sub)

    def run(rng_key, state: EllipSliceState, loglikelihood_fn: Callable, num_steps: int, thin: int = 0):
        """``num_steps`` calls of ``kernel`` in one launch: with ONE key transition j uses ``split(rng_key, num_steps)[j]``, with keys
        ``[n_chain_local, 2]`` transition j of chain b uses ``split(rng_key[b], num_steps)[j]``.  Bit-identical with that loop."""
        dist, beta = resolve_loglikelihood(loglikelihood_fn)
        eng = _attach(dist)
        t = eng.torch
        num_steps, thin = int(num_steps), int(thin)
        pos, ll = state.position.clone(), state.logdensity.clone()
        n, dev = pos.shape[0], pos.device
        sub_sum = t.empty(n, device=dev, dtype=t.int32)
        capped = t.empty(n, device=dev, dtype=t.int32)
        sub_max = t.empty(n, device=dev, dtype=t.int32)
        sub = t.empty(n, device=dev, dtype=t.int32)
        theta = t.empty(n, device=dev, dtype=t.float64)
        mom = t.empty_like(pos)
        traj_pos = traj_ll = None
        if thin > 0 and num_steps >= thin and num_steps % thin == 0:       # (anything else: the library names the bad argument)
            traj_pos = t.empty((num_steps // thin,) + tuple(pos.shape), device=dev, dtype=t.float32)
            traj_ll = t.empty((num_steps // thin, n), device=dev, dtype=t.float64)
        eng.ctx.eslice_run(_keys_tensor(t, rng_key, dev), beta, num_steps, pos, ll, thin=thin, subiter_sum=sub_sum, n_capped=capped,
                           traj_pos=traj_pos, traj_loglik=traj_ll, subiter=sub, theta=theta, momentum=mom, subiter_max=sub_max)
        return EllipSliceState(pos, ll), EllipSliceRunInfo(sub_sum.double() / num_steps, capped, traj_pos, traj_ll, EllipSliceInfo(mom, theta, sub), sub_max)

    kernel.run = run
    return kernel


class elliptical_slice:
    """``elliptical_slice(loglikelihood_fn, *, mean=None, cov=None) -> SamplingAlgorithm(init, step)`` after blackjax."""

    init = staticmethod(init)
    build_kernel = staticmethod(build_kernel)

    def __new__(cls, loglikelihood_fn: Callable, *, mean=None, cov=None) -> SamplingAlgorithm:
        if mean is not None or cov is not None:
            raise NotImplementedError("the Gaussian of the ellipse is the distribution's own prior N(dist.mu, dist.gram): "
                                      "mean and cov must stay None")
        resolve_loglikelihood(loglikelihood_fn)       # (the refusals name their reason before any device work)
        kernel = cls.build_kernel()

        def init_fn(position):
            return cls.init(position, loglikelihood_fn)

        def step_fn(rng_key, state):
            return kernel(rng_key, state, loglikelihood_fn)

        def run_fn(rng_key, state, num_steps, thin=0):
            return kernel.run(rng_key, state, loglikelihood_fn, num_steps, thin)

        step_fn.run = run_fn
        return SamplingAlgorithm(init_fn, step_fn)
