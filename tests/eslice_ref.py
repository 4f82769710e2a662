"""Float64 restatement of the elliptical slice transition of include/mfm.h (mfm_eslice_step / mfm_eslice_run; csrc/eslice.hip).

The sampler is the reference's ``bblackjax/mcmc/tess.py`` under the linear transport ``T(u) = mu + L u``: the log-det is constant and
``|u|^2 + |m|^2`` is constant on the ellipse, so the slice test ``logprob(T(u)) + ldj - 1/2 |m|^2`` (``tess.py:42-44``) compares
log-likelihoods alone, and the ellipse of ``tess.py:78-83`` in u-space is ``x' = mu + (x - mu) cos + nu sin`` with ``nu = L m``.
What the library fixes beyond ``tess.py``: the four step keys come from ONE ``split(k_b, 4)`` (``tess.py:93`` splits three ways and
chains a split per shrink, ``:111``; here the shrink draws are counter-based, ``uniform(k_shrink, (64,))[subiter - 1]``), and the
loop ends after ``MAX_SUBITER`` evaluations with the state kept.

Draws: ``oracle/prng`` (the jax conventions).  Everything is float64 except that a position is rounded to float32 where the kernel
stores it (every point that is evaluated is a float32 row), so the log-likelihood of the state is the log-likelihood OF the stored
row.  Each transition returns every decision's margin ``beta * ll(x') - log y`` per chain, so that a test can leave out the chains
whose decision a float32 kernel may legitimately make the other way."""
from collections import namedtuple

import numpy as np

from oracle import prng

MAX_SUBITER = 64           # include/mfm.h: MFM_ESLICE_MAX_SUBITER
TWO_PI = 2.0 * np.pi

Info = namedtuple("Info", "momentum theta subiter capped margins normals")


def loglik(dist, x):
    """``sum_i (x_i c_i - a exp(x_i))`` (cox_process_utils.py:113-115), float64, of float64 or float32 rows."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return (x * dist.counts[None] - dist.poisson_a * np.exp(x)).sum(1)


def chain_keys(key, n_total, offset=0, n_local=None):
    """The chains' keys of a launch on ONE key: ``split(key, n_total)[offset + b]`` (mcmc_chain_key)."""
    n_local = n_total - offset if n_local is None else n_local
    return prng.split_at(np.asarray(key, dtype=np.uint32), n_total, offset + np.arange(n_local))


def run_keys(key_mode, key, chain_keys_, n_steps, s, n_total, offset=0, n_local=None):
    """Step ``s`` of a run (mcmc_run_key): key_mode 0 ``split(split(key, n)[s], n_total)[chain]``; 1 ``split(keys[b], n)[s]``."""
    if key_mode:
        return prng.split_rows(chain_keys_, n_steps)[:, s]
    return chain_keys(prng.split(np.asarray(key, dtype=np.uint32), n_steps)[s], n_total, offset, n_local)


def ellipse(dist, x, nu, theta):
    """``tess.py:78-83``, position half, pushed through T; rounded to float32 as the kernel's registers hold it."""
    xp = dist.mu + (x - dist.mu) * np.cos(theta)[:, None] + nu * np.sin(theta)[:, None]
    return xp.astype(np.float32).astype(np.float64)


def transition(kb, x, ll, beta, dist, max_subiter=MAX_SUBITER):
    """One transition of every chain.  ``kb [B, 2]``: the chains' keys; ``x [B, d]``: float32-valued rows; ``ll [B]``: their untempered
    log-likelihood.  Returns ``(x_new, ll_new, Info)``; ``Info.margins [B, max evaluations made]``: ``beta ll(x') - log y`` of every
    evaluation (NaN where the chain had finished)."""
    x = np.asarray(x, dtype=np.float64)
    ll = np.asarray(ll, dtype=np.float64)
    B, d = x.shape
    ks = prng.split_rows(kb, 4)                                   # (k_nu, k_u, k_theta, k_shrink)
    n = prng.normal_rows(ks[:, 0], d)                             # tess.py:95
    nu = n @ dist.chol.T                                          # ... pushed through L: the prior draw about the mean
    with np.errstate(divide="ignore"):
        logy = beta * ll + np.log(prng.uniform_rows(ks[:, 1]))    # tess.py:98
    theta = TWO_PI * prng.uniform_rows(ks[:, 2])                  # tess.py:100
    lo, hi = theta - TWO_PI, theta.copy()                         # tess.py:101-102
    shrink = prng.uniform_rows(ks[:, 3], max_subiter)             # counter-based: no chain of splits
    done = np.zeros(B, dtype=bool)
    sub = np.zeros(B, dtype=np.int32)
    x_new, ll_new = x.copy(), ll.copy()
    margins = []
    for it in range(1, max_subiter + 1):
        live = ~done
        xp = ellipse(dist, x, nu, theta)
        llp = loglik(dist, xp)
        with np.errstate(invalid="ignore"):
            v = beta * llp
            acc = live & np.isfinite(v) & (v > logy)              # tess.py:121
            margins.append(np.where(live, v - logy, np.nan))
        sub[live] = it
        x_new[acc], ll_new[acc] = xp[acc], llp[acc]
        done |= acc
        if done.all():
            break
        rej = ~done
        neg = rej & (theta < 0)
        lo = np.where(neg, theta, lo)                             # tess.py:115-116
        hi = np.where(rej & ~neg, theta, hi)
        if it < max_subiter:
            theta = np.where(rej, lo + (hi - lo) * shrink[:, it - 1], theta)      # tess.py:112
    return x_new, ll_new, Info(nu, theta, sub, ~done, np.stack(margins, axis=1), n)


def run(key_mode, key, keys, beta, n_steps, x, ll, dist, n_total=None, offset=0, thin=0):
    """``n_steps`` transitions on the key schedule of mfm_mala_run.  Returns ``(x, ll, infos, traj_x, traj_ll)``, ``infos`` the list of
    every transition's ``Info``."""
    B = x.shape[0]
    n_total = B if n_total is None else n_total
    infos, tx, tl = [], [], []
    for s in range(n_steps):
        kb = run_keys(key_mode, key, keys, n_steps, s, n_total, offset, B)
        x, ll, info = transition(kb, x, ll, beta, dist)
        infos.append(info)
        if thin > 0 and (s + 1) % thin == 0:
            tx.append(x.copy()); tl.append(ll.copy())
    return x, ll, infos, (np.stack(tx) if tx else None), (np.stack(tl) if tl else None)


def min_margin(infos):
    """Per chain the smallest ``|margin|`` over every decision of every transition in ``infos``."""
    return np.min([np.nanmin(np.abs(i.margins), axis=1) for i in infos], axis=0)
