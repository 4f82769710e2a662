"""The float64 yardstick of the autocorrelation kernel (tests/autocorr_oracle.py) against an independent computation and against theory."""
import numpy as np

from tests import autocorr_oracle as ao


def _fft_lag_sums(x, L):
    """The same sums through the Wiener-Khinchin route (zero-padded to 2 n so the circular sums do not wrap)."""
    n = x.shape[0]
    c = x - x.mean(axis=0, keepdims=True)
    f = np.fft.rfft(c, n=2 * n, axis=0)
    return np.fft.irfft(f * np.conj(f), n=2 * n, axis=0)[:L]


def test_direct_sums_agree_with_the_fft():
    g = np.random.default_rng(3)
    for n, S, L in ((1, 2, 1), (2, 3, 2), (37, 5, 37), (257, 4, 100), (500, 3, 500)):
        x = np.cumsum(g.standard_normal((n, S)), axis=0) * 0.1 + g.standard_normal((n, S)) + 3.0
        A = ao.lag_sums(x, L)
        F = _fft_lag_sums(x, L)
        np.testing.assert_allclose(A, F, rtol=0, atol=1e-10 * max(1.0, np.abs(A).max()))
        if n > 1:
            r = ao.rho(x, L)
            np.testing.assert_allclose(r, F / F[:1], rtol=0, atol=1e-10)
            assert (r[0] == 1.0).all()


def test_rho_works_in_float64_on_float32_input():
    x = ao.ar1(64, 3, 1)
    assert x.dtype == np.float32
    assert ao.rho(x, 8).dtype == np.float64
    np.testing.assert_array_equal(ao.rho(x, 8), ao.rho(x.astype(np.float64), 8))


def test_constant_series_is_nan():
    x = np.full((10, 2), 2.5)
    x[:, 1] = np.arange(10)
    r = ao.rho(x, 4)
    assert np.isnan(r[:, 0]).all() and r[0, 1] == 1.0
    tau = ao.geyer(r)[0]
    assert np.isnan(tau[0]) and np.isfinite(tau[1])


def test_geyer_on_known_sequences():
    r = np.array([[1.0, 1.0, 1.0], [0.5, 0.5, -2.0], [0.25, -0.6, 0.3], [0.125, 0.5, 0.3], [0.0625, 0.9, 0.9]])      # 5 lags: 2 pairs fit
    tau, m_stop, G = ao.geyer(r)
    np.testing.assert_allclose(G, [[1.5, 1.5, -1.0], [0.375, -0.1, 0.6]])
    np.testing.assert_array_equal(m_stop, [2, 1, 0])
    np.testing.assert_allclose(tau, [-1 + 2 * 1.875, -1 + 2 * 1.5, -1.0])
    assert ao.geyer(r[:1])[0].tolist() == [-1.0, -1.0, -1.0]        # no pair fits in one lag


def test_ar1_tau_matches_theory():
    """AR(1), phi = 0.5, n = 20000: tau = (1 + phi) / (1 - phi) = 3 to 10 %.  One series' estimate has a standard deviation of about
    tau sqrt(2 (2 K + 1) / n) with K ~ 10 lags kept, i.e. 4 to 6 %, so a single draw sits outside 10 % every tenth time or so; the
    average of 16 independent series (1.5 %, plus the small upward bias of stopping at the first non-positive pair) does not."""
    phi, n = 0.5, 20000
    x = ao.ar1(n, 16, 7, phi=phi)
    assert x.dtype == np.float32 and abs(x.mean() - 3.0) < 0.1
    ess, tau = ao.ess(x, 200)
    np.testing.assert_allclose(tau.mean(), (1 + phi) / (1 - phi), rtol=0.10)
    assert (np.abs(tau / 3.0 - 1) < 0.10).mean() >= 0.75              # and most single series are inside, too
    np.testing.assert_allclose(ess, n / tau)


def test_ar1_is_stationary_and_seeded():
    a, b = ao.ar1(50, 200, 0), ao.ar1(50, 200, 0)
    np.testing.assert_array_equal(a, b)
    phi = np.random.default_rng(0).uniform(0.0, 0.9, size=200)
    assert (phi >= 0).all() and (phi <= 0.9).all()
    big = ao.ar1(4000, 8, 2, phi=0.8).astype(np.float64)
    np.testing.assert_allclose(big.var(axis=0).mean(), 1 / (1 - 0.64), rtol=0.15)
