"""CPU tests of the float64 yardstick ``tests/chain_diag_oracle.py`` that the GPU tests of ``mfm_chain_sums`` / ``mfm_chain_diag`` lean on,
and of the pieces around the kernels that need no GPU (the binding's entries, the new module's exports)."""
import os
import re

import numpy as np

from tests import autocorr_oracle as ao, chain_diag_oracle as co


def test_rhat_is_the_textbook_form_on_the_split_array():
    x = co.case_data(101, 12, 5, 3)
    n = x.shape[0]
    h = n // 2
    y = np.concatenate([x[:h], x[n - h:]], axis=1).astype(np.float64)           # the middle row of the odd n belongs to neither half
    W = np.var(y, axis=0, ddof=1).mean(axis=0)
    Bn = np.var(y.mean(axis=0), axis=0, ddof=1)
    want = np.sqrt(((h - 1) / h * W + Bn) / W)
    got = co.diag(x, 8, split=True)
    np.testing.assert_allclose(got["rhat"], want, rtol=1e-14, atol=0)
    assert got["n_sub"] == 50 and got["M"] == 24
    np.testing.assert_allclose(got["rho"][0], 1.0, rtol=0, atol=1e-14)
    whole = co.diag(x, 8, split=False)
    y = x.astype(np.float64)
    W, Bn = np.var(y, axis=0, ddof=1).mean(axis=0), np.var(y.mean(axis=0), axis=0, ddof=1)
    np.testing.assert_allclose(whole["rhat"], np.sqrt(((n - 1) / n * W + Bn) / W), rtol=1e-14, atol=0)


def test_stuck_chains_show_in_rhat_and_in_the_multichain_ess_and_not_in_the_per_chain_ess():
    x = co.stuck()
    n, B, d = x.shape
    got = co.diag(x, n // 2, split=True)
    assert got["rhat"][0] > 3.0 and (got["rhat"][1:] < 1.05).all()
    assert got["ess"][0] < 0.1 * got["ess"][1:].min()                           # of 4096 draws: tens against more than a thousand
    assert got["ess"][0] < 100 and got["ess"][1:].min() > 1000
    per_chain, _ = ao.ess(x.reshape(n, B * d), n)                               # Geyer's ESS of every chain by itself cannot tell them apart
    per_chain = per_chain.reshape(B, d)
    assert 0.7 < np.median(per_chain[:, 0]) / np.median(per_chain[:, 1:]) < 1.4


def test_sums_are_additive_over_disjoint_chain_sets():
    x = co.case_data(64, 32, 3, 0)
    for split in (True, False):
        a, b, u = co.sums(x[:, :16], 20, split), co.sums(x[:, 16:], 20, split), co.sums(x, 20, split)
        np.testing.assert_allclose(a + b, u, rtol=1e-12, atol=0)


def test_sums_give_the_diagnostics_of_the_direct_form():
    """The decomposition the kernel uses: W, B/n and rho from ``sums`` alone equal the np.var / direct form."""
    x = co.case_data(96, 10, 4, 10)
    L = 30
    got = co.diag(x, L)
    s, M, n_sub = co.sums(x, L), got["M"], got["n_sub"]
    W = s[2] / (M * (n_sub - 1))
    Bn = (s[1] - s[0] ** 2 / M) / (M - 1)
    np.testing.assert_allclose(W, got["W"], rtol=1e-12)
    np.testing.assert_allclose(Bn, got["Bn"], rtol=1e-9)                       # (the cancellation: about 1e-16 mean^2 / (B/n))
    varp = (n_sub - 1) / n_sub * W + Bn
    np.testing.assert_allclose(1.0 - (W - s[2:] / (M * (n_sub - 1))) / varp, got["rho"], rtol=0, atol=1e-11)


def test_no_split_on_concatenated_halves_equals_split():
    x = co.case_data(100, 6, 3, 4)
    halves = np.concatenate([x[:50], x[50:]], axis=1)
    a, b = co.diag(x, 25, split=True), co.diag(halves, 25, split=False)
    for k in ("rhat", "ess", "tau", "rho"):
        np.testing.assert_array_equal(a[k], b[k])
    np.testing.assert_array_equal(co.sums(x, 25, True), co.sums(halves, 25, False))


def test_constant_coordinate_is_nan_in_the_oracle_too():
    x = co.case_data(40, 4, 3, 1).copy()
    x[:, :, 1] = 2.5
    got = co.diag(x, 10)
    for k in ("rhat", "ess", "tau"):
        assert np.isnan(got[k][1]) and np.isfinite(got[k][[0, 2]]).all()
    assert np.isnan(got["rho"][:, 1]).all()


def test_binding_and_module_export_the_entries():
    from mfm_amd import _lib, diagnostics
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mfm.h")).read()
    for name in ("mfm_chain_sums", "mfm_chain_diag"):
        assert name in _lib.EXPORTS and f"int {name}(" in header
    assert int(re.search(r"#define MFM_CHAIN_SLICES_MAX (\d+)", header).group(1)) >= 1
    assert callable(_lib.Context.chain_sums) and callable(_lib.Context.chain_diag)
    assert set(diagnostics.__all__) == {"ChainDiagnostics", "chain_diagnostics", "potential_scale_reduction"}
    assert diagnostics.ChainDiagnostics._fields == ("rhat", "ess", "tau")
