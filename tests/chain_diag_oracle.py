"""Float64 numpy yardstick of ``mfm_chain_sums`` / ``mfm_chain_diag`` (mfm_amd/csrc/diag.hip), written from the formulas in include/mfm.h.

Everything works on ``x [n, n_chain, dim]`` (time first) in float64 whatever the input's type, by DIRECT lag sums and ``np.var``: the
variances are not taken through the ``sums`` decomposition that the kernel uses (``sums`` is restated separately, for the tests of it).

* ``subchains(x, split)``: ``[n_sub, M, dim]``; with ``split`` the first and the last ``n // 2`` rows of every chain side by side along
  the chain axis (first halves, then second halves), the middle row of an odd ``n`` left out.
* ``diag(x, L, split)``: ``dict(rhat, ess, tau, rho [L, dim], G, m_stop, W, Bn, varp)`` per coordinate.
* ``sums(x, L, split)``: ``[L + 2, dim]``: sum of the sub-chain means, of their squares, of the lag sums ``A_0 .. A_{L-1}``.
* ``stuck(...)``: the construction of the stuck-chain tests: AR(1) chains, half of them shifted by +4 and half by -4 in coordinate 0.
"""
import numpy as np

from tests import autocorr_oracle as ao


def subchains(x, split=True):
    x = np.asarray(x, dtype=np.float64)
    if not split:
        return x
    n = x.shape[0]
    h = n // 2
    return np.concatenate([x[:h], x[n - h:]], axis=1)


def lag_sums(y, L):
    """``A [L, M, dim]`` of sub-chains ``y [n_sub, M, dim]``, each centred by its own mean."""
    n_sub, M, d = y.shape
    return ao.lag_sums(y.reshape(n_sub, M * d), L).reshape(L, M, d)


def sums(x, L, split=True):
    y = subchains(x, split)
    mu = y.mean(axis=0)
    return np.concatenate([mu.sum(axis=0)[None], (mu * mu).sum(axis=0)[None], lag_sums(y, L).sum(axis=1)], axis=0)


def diag(x, L, split=True):
    y = subchains(x, split)
    n_sub, M, d = y.shape
    with np.errstate(invalid="ignore", divide="ignore"):
        W = y.var(axis=0, ddof=1).mean(axis=0)                      # mean within-sub-chain variance
        Bn = y.mean(axis=0).var(axis=0, ddof=1)                     # variance of the sub-chain means: B / n
        varp = (n_sub - 1) / n_sub * W + Bn
        rhat = np.sqrt(varp / W)
        acov = lag_sums(y, L).mean(axis=1) / (n_sub - 1)            # chain-averaged autocovariance, normalised as W is: acov[0] = W
        rho = 1.0 - (W[None] - acov) / varp[None]
        bad = ~((W > 0) & np.isfinite(W) & np.isfinite(varp))
        rho[:, bad] = np.nan
        rhat = np.where(bad, np.nan, rhat)
        tau, m_stop, G = ao.geyer(rho)
        ess = M * n_sub / tau
    return dict(rhat=rhat, ess=ess, tau=tau, rho=rho, G=G, m_stop=m_stop, W=W, Bn=Bn, varp=varp, n_sub=n_sub, M=M)


def case_data(n, B, d, seed):
    """The recipe of the GPU cases: every coordinate has one phi across the chains."""
    phi = np.tile(np.random.default_rng(100 + seed).uniform(0.0, 0.9, d), B)
    return ao.ar1(n, B * d, seed, phi=phi).reshape(n, B, d)


def stuck(n=128, B=32, d=4, phi=0.5, shift=4.0, seed=0):
    x = ao.ar1(n, B * d, seed, phi=phi).reshape(n, B, d).copy()
    x[:, :B // 2, 0] += np.float32(shift)
    x[:, B // 2:, 0] -= np.float32(shift)
    return x
