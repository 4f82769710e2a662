"""CPU tests of the oracle's absolute-product sums (oracle/fm.py: abs_sums / operands) and of the summation-order bound built on
them (tests/wgrad_cases.py: order_bound): the bound that lets a stream-K gradient differ from its friendly-shard sum by rounding
alone must FAIL a gradient that lost one 16-chain tile of one 64 x 64 block, or counted one twice."""
import numpy as np
import pytest

from tests import wgrad_cases as wc


def test_abs_sums_bound_the_gradient_and_leave_the_plain_results_alone():
    from oracle import fm, prng
    args, dist, model, params, x32 = wc.setup("R", 48)
    key = wc.case_key("R", 48)
    l0, g0 = fm.loss_and_grad(model, params, key, x32.astype(np.float64), args.sigma)
    l1, g1, S, ops = fm.loss_and_grad(model, params, key, x32.astype(np.float64), args.sigma, abs_sums=True, operands=True)
    assert l0 == l1 and len(S) == len(g0) == len(ops)
    for a, b, s, (A, dZ), (K, N) in zip(g0, g1, S, ops, model.layer_shapes()):
        assert A.shape == (48, K) and dZ.shape == (48, N) and A.dtype == dZ.dtype == np.float64
        for kk in ("kernel", "bias"):
            np.testing.assert_array_equal(a[kk], b[kk])
            assert s[kk].dtype == np.float64 and s[kk].shape == a[kk].shape and (s[kk] >= 0).all()
            assert (np.abs(b[kk]) <= s[kk] * (1 + 1e-6) + 1e-300).all()
        np.testing.assert_allclose(s["kernel"], np.einsum("bk,bn->kn", np.abs(A), np.abs(dZ)), rtol=1e-12)
        np.testing.assert_allclose(A.T @ dZ, b["kernel"], rtol=1e-6, atol=1e-6 * np.abs(b["kernel"]).max())


def test_the_block_table_covers_every_parameter_once():
    for net, n_jobs in (("S", 8), ("R", 9), ("H", 52), ("M", 8)):
        args, dist, model, params, x32 = wc.setup(net, 16)
        el = wc.block_elements(model)
        assert len(el) == n_jobs
        allidx = np.concatenate(el)
        assert np.array_equal(np.sort(allidx), np.arange(wc.flat64(params).size)), net


@pytest.mark.parametrize("net,B", wc.CASES_A)
def test_a_dropped_or_doubled_chain_tile_breaks_the_summation_order_bound(net, B):
    """In float64: take one 16-chain tile out of one 64 x 64 block of the gradient, or add it a second time -- in EVERY block of the
    network, the tile moving with the block -- and the element-wise bound 2 (B + 2) 2^-24 S_e is exceeded at least tenfold inside
    that block.  So a kernel whose second segment fetched a wrong tile row, or whose ring counted a tile twice, cannot pass it."""
    args, dist, model, params, x32 = wc.setup(net, B)
    o = wc.oracle(net, B, operands=True)
    bound = wc.order_bound(B, o["S"])
    off, shapes = wc.layer_offsets(model), model.layer_shapes()
    nbb = B // 16
    worst = np.inf
    for j, (l, k, n) in enumerate(wc.blocks(model)):
        A, dZ = o["ops"][l]
        tile = slice(16 * (j % nbb), 16 * (j % nbb) + 16)
        exact, T = A[:, k].T @ dZ[:, n], A[tile][:, k].T @ dZ[tile][:, n]          # the block, and what that tile adds to it
        bnd = bound[off[l][0] + k[:, None] * shapes[l][1] + n[None, :]]
        if k[0] == 0:                                                          # the block that also carries the bias sums
            exact = np.concatenate([exact.reshape(-1), dZ[:, n].sum(0)]); T = np.concatenate([T.reshape(-1), dZ[tile][:, n].sum(0)])
            bnd = np.concatenate([bnd.reshape(-1), bound[off[l][1] + n]])
        exact, T, bnd = exact.reshape(-1), T.reshape(-1), np.maximum(bnd.reshape(-1), 1e-300)
        ratio = min((np.abs((exact - T) - exact) / bnd).max(), (np.abs((exact + T) - exact) / bnd).max())      # dropped, doubled
        assert ratio >= 10.0, (net, B, j, l, ratio)
        worst = min(worst, ratio)
    print(f"mutation {net}@{B}: smallest block-wise violation {worst:.3g} x bound")


@pytest.mark.parametrize("net,B,n_valid", wc.ORACLE_CASES)
def test_no_relu_unit_of_a_case_sits_within_float32_rounding_of_its_kink(net, B, n_valid):
    """The float64 gradient is a reference for a float32 kernel only where no ReLU unit can take the other branch in float32
    (tests/wgrad_cases.py: KEYS)."""
    m = wc.relu_margin(net, B, n_valid)
    print(f"relu margin {net}@{B}: {m / wc.U32:.2f} u")
    assert m >= wc.RELU_MARGIN, (net, B, n_valid, m / wc.U32)
