"""Float64 numpy yardstick of ``mfm_autocorr`` (mfm_amd/csrc/diag.hip), written from the definition in include/mfm.h.

Everything works on an array ``x [n, S]`` (time-major, one series per column) and in float64 whatever the input's type:

* ``rho(x, L)``: ``rho[k, s] = A_k / A_0`` with ``A_k = sum_{t < n-k} c_t c_{t+k}``, ``c = x - mean``, by DIRECT lag sums (no FFT).
* ``geyer(rho)``: ``Gamma_m = rho_2m + rho_2m+1``, ``tau = -1 + 2 sum`` of the leading run of ``Gamma_m > 0`` over the pairs that fit
  in ``rho.shape[0]`` lags; also the Gammas and, per series, the index of the first non-positive Gamma (the number of pairs when none is).
* ``ar1(n, S, seed)``: stationary AR(1) series ``x_t = phi_s x_{t-1} + e_t + 3`` in float32.
"""
import numpy as np


def lag_sums(x, L):
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    c = x - x.mean(axis=0, keepdims=True)
    A = np.empty((L,) + x.shape[1:], dtype=np.float64)
    for k in range(L):
        A[k] = (c[:n - k] * c[k:]).sum(axis=0)
    return A


def rho(x, L):
    A = lag_sums(x, L)
    with np.errstate(invalid="ignore", divide="ignore"):
        return A / A[:1]


def gammas(r):
    M = r.shape[0] // 2
    return r[0:2 * M:2] + r[1:2 * M:2]


def tau_truncated(G, m_stop):
    """tau with the sum cut at pair ``m_stop[s]`` (exclusive) whatever the signs."""
    keep = np.arange(G.shape[0])[:, None] < np.asarray(m_stop)[None, :]
    return -1.0 + 2.0 * np.where(keep, G, 0.0).sum(axis=0)


def geyer(r):
    """``(tau, m_stop, G)`` for ``r [L, S]``; a series whose ``rho_0`` is NaN has ``tau = NaN``."""
    r = np.asarray(r, dtype=np.float64)
    G = gammas(r)
    M, S = G.shape[0], r.shape[1]
    pos = G > 0
    m_stop = np.where(pos.all(axis=0), M, np.argmin(pos, axis=0)) if M else np.zeros(S, dtype=np.int64)
    tau = tau_truncated(G, m_stop) if M else np.full(S, -1.0)
    tau = np.where(np.isnan(r[0]), np.nan, tau)
    return tau, m_stop, G


def ess(x, L):
    """``(ess, tau)`` of ``x [n, S]`` with ``rho`` taken up to ``L`` lags."""
    tau = geyer(rho(x, L))[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        return x.shape[0] / tau, tau


def ar1(n, S, seed, phi=None):
    g = np.random.default_rng(seed)
    phi = g.uniform(0.0, 0.9, size=S) if phi is None else np.broadcast_to(np.asarray(phi, dtype=np.float64), (S,))
    e = g.standard_normal((n, S))
    x = np.empty((n, S))
    x[0] = e[0] / np.sqrt(1.0 - phi * phi)          # the stationary law
    for t in range(1, n):
        x[t] = phi * x[t - 1] + e[t]
    return (x + 3.0).astype(np.float32)
