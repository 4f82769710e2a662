"""Parallel tempering (replica exchange) on MI355X -- a BUILD-SIDE MODE beside ``hmc.py`` / ``mala.py``: the reference vendors none.

``K = len(betas)`` temperatures, ``R`` independent ladders: ``state.position`` is ``[R * K, dim]`` (CUDA float32), chain ``r * K + k``
is slot ``k`` of ladder ``r`` and targets ``logprior + betas[k] * loglikelihood`` with its own step size; slot 0 (usually
``betas[0] = 1``) is the one that is kept.  A round is ``num_mcmc_steps`` local steps of every chain -- HMC with
``num_integration_steps`` leapfrog steps or MALA -- and one exchange sweep of deterministic even-odd parity (Syed et al. 2019), a
Metropolis move on the joint density, correct for any tempering path.  ``step(rng_key, state)`` is one round;
``step.run(rng_key, state, num_rounds, thin=0)`` is ``num_rounds`` rounds in ONE library call (``mfm_pt_run``; the key schedule and the
exchange: ``include/mfm.h``, restated in ``tests/pt_ref.py``).  A round's sweep parity is the round's number within its call, so
``step`` always sweeps the even pairs.

Refused or absent: NUTS as the local move, mass matrices, more than one rank, a per-temperature step-size warmup, stochastic even / odd
schedules, round-trip counting; the Cox process (the library returns ``MFM_EUNSUPPORTED``).

Host helpers (numpy only): ``geometric_ladder``, ``communication_barrier``, ``adapt_ladder``."""
from typing import NamedTuple

import numpy as np

from ...distributions import resolve_logdensity
from ..base import SamplingAlgorithm
from .mala import _engine

__all__ = ["PTState", "PTInfo", "parallel_tempering", "geometric_ladder", "communication_barrier", "adapt_ladder"]

MALA_TEXTBOOK_DEFAULT = False      # mala.build_kernel's default: the acceptance rule as the reference writes it


class PTState(NamedTuple):
    position: object
    logdensity: object
    logdensity_grad: object
    replica: object              # int32 [R * K]: which start replica sits in which slot


class PTInfo(NamedTuple):
    """``swap_acceptance_rate [K - 1]`` (accepted swaps over attempted ones, pooled over the ladders; NaN for a pair never attempted),
    ``swap_accepted [R, K - 1]``, ``acceptance_rate [R * K]`` (the local steps' mean acceptance probability per slot), and with ``thin``
    slot 0's kept ``positions [num_rounds / thin, R, dim]`` / ``logdensities [num_rounds / thin, R]`` (``None`` without)."""
    swap_acceptance_rate: object
    swap_accepted: object
    acceptance_rate: object
    positions: object
    logdensities: object


def geometric_ladder(K, beta_min):
    """``K`` inverse temperatures from 1 down to ``beta_min``, evenly spaced in the logarithm."""
    K = int(K)
    if K < 2 or not 0.0 < float(beta_min) < 1.0:
        raise ValueError(f"geometric_ladder needs K >= 2 and 0 < beta_min < 1 (got K = {K}, beta_min = {beta_min})")
    b = np.exp(np.linspace(0.0, np.log(float(beta_min)), K))
    b[0], b[-1] = 1.0, float(beta_min)
    return b


def communication_barrier(rates):
    """The global communication barrier's estimate: the sum of the pairs' rejection rates."""
    return float(np.sum(1.0 - np.asarray(rates, dtype=np.float64)))


def adapt_ladder(betas, rates):
    """The equal-rejection update (Syed et al. 2019, algorithm 4): new betas at which the cumulative barrier ``Lambda(beta)``, linearly
    interpolated through ``(betas[k], sum_{i < k} (1 - rates[i]))``, takes equally spaced values.  The end points stay; the result is
    monotone; equal rates give the ladder back."""
    betas, rates = np.asarray(betas, dtype=np.float64), np.asarray(rates, dtype=np.float64)
    if betas.ndim != 1 or rates.shape != (betas.size - 1,):
        raise ValueError(f"adapt_ladder needs betas [K] and rates [K - 1] (got {betas.shape} and {rates.shape})")
    rej = np.clip(1.0 - rates, 1e-12, None)            # (a pair that never rejects still gets a sliver: the interpolation stays monotone)
    cum = np.concatenate([[0.0], np.cumsum(rej)])
    new = np.interp(np.linspace(0.0, cum[-1], betas.size), cum, betas)
    new[0], new[-1] = betas[0], betas[-1]
    return new


def check_arguments(betas, mcmc, step_size, num_integration_steps, num_mcmc_steps, exchange):
    """``(betas [K], step sizes [K], kernel, exchange flag)``; ``ValueError`` before any device work."""
    betas = np.array(betas, dtype=np.float64).reshape(-1)
    K = betas.size
    if not 2 <= K <= 64:
        raise ValueError(f"betas must hold 2 to 64 temperatures (got {K})")
    if not (np.isfinite(betas) & (betas > 0)).all():
        raise ValueError("betas: every entry must be finite and positive")
    if mcmc not in ("hmc", "mala"):
        raise ValueError(f"mcmc must be 'hmc' or 'mala' (got {mcmc!r}): NUTS is not served as the local move")
    if exchange not in ("even_odd", "none"):
        raise ValueError(f"exchange must be 'even_odd' or 'none' (got {exchange!r})")
    s = np.array(step_size, dtype=np.float64)
    if s.ndim == 0:
        s = float(s) / np.sqrt(betas)                  # a scalar s means s / sqrt(beta_k): the tempered target is 1 / sqrt(beta) wider
    elif s.shape != (K,):
        raise ValueError(f"step_size must be a scalar or hold K = {K} entries (got shape {s.shape})")
    if not (np.isfinite(s) & (s > 0)).all():
        raise ValueError("step_size: every entry must be finite and positive")
    if int(num_mcmc_steps) < 1 or (mcmc == "hmc" and int(num_integration_steps) < 1):
        raise ValueError("num_mcmc_steps and num_integration_steps must be at least 1")
    return betas, s, mcmc, exchange == "even_odd"


class parallel_tempering:
    def __new__(cls, logprior_fn, loglikelihood_fn, betas, mcmc="hmc", step_size=0.1, num_integration_steps=10, num_mcmc_steps=1,
                exchange="even_odd", textbook=MALA_TEXTBOOK_DEFAULT) -> SamplingAlgorithm:
        betas, eps, mcmc, do_exchange = check_arguments(betas, mcmc, step_size, num_integration_steps, num_mcmc_steps, exchange)
        K = betas.size
        dist, _ = resolve_logdensity(lambda x: logprior_fn(x) + 1.0 * loglikelihood_fn(x))      # as smc/tempered.py's tempered_logposterior_fn

        def ladders(n):
            if n % K or n < K:
                raise ValueError(f"position must hold R * K rows, K = {K} temperatures (got {n})")
            return n // K

        def full(eng, x):
            """``x [R * K, ...]`` as the first rows of an ``n_chain_local`` batch (the library never reads the rest)."""
            t = eng.torch
            if x.shape[0] > eng.n_local:
                raise ValueError(f"R * K = {x.shape[0]} chains exceed the engine's n_chain_local = {eng.n_local}")
            out = t.zeros((eng.n_local,) + tuple(x.shape[1:]), device=x.device, dtype=x.dtype)
            out[:x.shape[0]] = x
            return out

        def init_fn(position):
            eng = _engine(dist)
            t = eng.torch
            n = position.shape[0]
            ladders(n)
            pos = full(eng, position.to(t.float32))
            logp = t.zeros(eng.n_local, device=pos.device, dtype=t.float64); grad = t.zeros_like(pos)
            lp_k = t.empty_like(logp); g_k = t.empty_like(pos)
            for k in range(K):                          # every slot at its own beta
                eng.ctx.mala_init(pos, float(betas[k]), lp_k, g_k)
                logp[k:n:K] = lp_k[k:n:K]; grad[k:n:K] = g_k[k:n:K]
            return PTState(pos[:n].clone(), logp[:n].clone(), grad[:n].clone(), t.arange(n, device=pos.device, dtype=t.int32))

        def run_fn(rng_key, state, num_rounds, thin=0):
            eng = _engine(dist)
            t = eng.torch
            num_rounds, thin = int(num_rounds), int(thin)
            n = state.position.shape[0]
            R = ladders(n)
            pos, logp, grad = full(eng, state.position), full(eng, state.logdensity), full(eng, state.logdensity_grad)      # states are values
            replica = state.replica.clone()
            dev = pos.device
            n_acc = t.empty(n, device=dev, dtype=t.int32); acc_sum = t.empty(n, device=dev, dtype=t.float64)
            swap_acc = t.empty((R, K - 1), device=dev, dtype=t.int32); swap_prob = t.empty((R, K - 1), device=dev, dtype=t.float64)
            traj_pos = traj_logp = None
            if thin > 0 and num_rounds >= thin and num_rounds % thin == 0:       # (anything else: the library names the bad argument)
                traj_pos = t.empty((num_rounds // thin, R, pos.shape[1]), device=dev, dtype=t.float32)
                traj_logp = t.empty((num_rounds // thin, R), device=dev, dtype=t.float64)
            eng.ctx.set_inverse_mass(None)
            eng.ctx.pt_run(rng_key, betas, eps, R, int(num_mcmc_steps), num_rounds, pos, logp, grad, kernel=mcmc, num_steps=int(num_integration_steps),
                           textbook=textbook, exchange=do_exchange, thin=thin, n_acc=n_acc, acc_sum=acc_sum, replica=replica,
                           swap_accepted=swap_acc, swap_prob=swap_prob, traj_pos=traj_pos, traj_logp=traj_logp)
            attempts = t.as_tensor([R * len(range(k % 2, num_rounds, 2)) for k in range(K - 1)], device=dev, dtype=t.float64)
            rate = swap_acc.sum(0).double() / attempts if do_exchange else t.full((K - 1,), float("nan"), device=dev, dtype=t.float64)
            info = PTInfo(rate, swap_acc, acc_sum / (num_rounds * int(num_mcmc_steps)), traj_pos, traj_logp)
            return PTState(pos[:n].clone(), logp[:n].clone(), grad[:n].clone(), replica), info

        def step_fn(rng_key, state):
            return run_fn(rng_key, state, 1)

        step_fn.run = run_fn
        return SamplingAlgorithm(init_fn, step_fn)
