"""The HMC step with a diagonal inverse mass matrix and the window adaptation around it, restated in float64 numpy.  A helper of
tests/test_hmc_mass_host.py and tests/test_gpu_hmc_mass.py, not a test.

``kernel`` is ``oracle.hmc.kernel`` line for line with the three changes a diagonal ``minv`` makes: momentum ``p = n / sqrt(minv)`` from
the same normal draws, energy ``H = -logp + sum(minv p^2) / 2``, drift ``x += eps minv p``.  tests/test_hmc_mass_host.py pins it to that
oracle: equal with ``minv = 1``, and equal to the oracle on the rescaled target ``y = x / sqrt(minv)`` otherwise.

``window_adaptation`` is the driver of mfm_amd/bblackjax/adaptation/window_adaptation.py on tests/warmup_ref.py's dual averaging: the
segments of ``window_schedule``, each on ``split(key, n_segments)[i]`` with the step-major key schedule of the device inside, from the
pooled step size of the segment before; after a slow window the regularised within-chain variance, averaged over the chains."""
import numpy as np

from oracle import prng
from oracle.hmc import HMCInfo
from oracle.mala import MALAState
from tests import warmup_ref as wr


def kernel(keys, state, value_and_grad, step_size, num_integration_steps, inverse_mass, momentum=None):
    """``keys`` [B, 2]: one key per chain; ``inverse_mass`` [d]; ``momentum`` overrides the draw."""
    x, logp, g = state
    B, d = x.shape
    minv = np.asarray(inverse_mass, dtype=np.float64)
    kk = prng.split_rows(keys, 2)
    p = prng.normal_rows(kk[:, 0], d) / np.sqrt(minv) if momentum is None else np.asarray(momentum, dtype=np.float64)
    h0 = -logp + 0.5 * (minv * p * p).sum(1)
    xn, pn, lpn, gn = x, p, logp, g
    for _ in range(int(num_integration_steps)):
        pn = pn + 0.5 * step_size * gn
        xn = xn + step_size * (minv * pn)
        lpn, gn = value_and_grad(xn)
        pn = pn + 0.5 * step_size * gn
    h1 = -lpn + 0.5 * (minv * pn * pn).sum(1)
    delta = h0 - h1
    delta = np.where(np.isnan(delta), -np.inf, delta)
    with np.errstate(over="ignore"):
        p_accept = np.minimum(np.exp(delta), 1.0)
    u = prng.uniform_rows(kk[:, 1])
    acc = u < p_accept
    m = acc[:, None]
    return MALAState(np.where(m, xn, x), np.where(acc, lpn, logp), np.where(m, gn, g)), HMCInfo(p_accept, acc, xn, delta), u


def log_spaced_mass(d, lo=0.25, hi=4.0, seed=5):
    """``d`` values log-spaced over ``[lo, hi]`` in a fixed permutation."""
    v = np.exp(np.linspace(np.log(lo), np.log(hi), d)) if d > 1 else np.array([hi])
    return v[np.random.RandomState(seed).permutation(d)]


def warmup_window(key, state, value_and_grad, step0, num_integration_steps, n_steps, target, inverse_mass):
    """One segment: ``warmup_ref.hmc_warmup`` with the mass step, plus the window's sums of the positions after accept / reject."""
    n, d = state.position.shape
    da = wr.DualAveraging(step0, target, n)
    step_keys = prng.split(key, n_steps)
    s, q, acc = np.zeros((n, d)), np.zeros((n, d)), []
    for j in range(n_steps):
        state, info, _ = kernel(prng.split(step_keys[j], n), state, value_and_grad, da.step[:, None], num_integration_steps, inverse_mass)
        da.update(info.acceptance_rate)
        acc.append(info.acceptance_rate)
        s += state.position
        q += state.position * state.position
    return dict(state=state, step_avg=da.averaged, pos_sum=s, pos_sumsq=q, acc=np.stack(acc))


def window_adaptation(key, state, value_and_grad, num_integration_steps, step0, num_steps, target=0.8):
    """``(state, step_size, inverse_mass, per-segment pooled step sizes)``."""
    from mfm_amd.bblackjax.adaptation.window_adaptation import window_schedule
    schedule = window_schedule(num_steps)
    d = state.position.shape[1]
    step, minv, steps = float(step0), np.ones(d), []
    for k, (kind, start, end) in zip(prng.split(key, len(schedule)), schedule):
        n = end - start
        w = warmup_window(k, state, value_and_grad, step, num_integration_steps, n, target, minv)
        state, step = w["state"], wr.pooled(w["step_avg"])[0]
        steps.append(step)
        if kind == "slow":
            var = ((w["pos_sumsq"] - w["pos_sum"] ** 2 / n) / (n - 1)).mean(0)
            minv = n / (n + 5.0) * var + 1e-3 * 5.0 / (n + 5.0)
    return state, step, minv, steps
