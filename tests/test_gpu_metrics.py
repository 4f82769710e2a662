"""GPU parity: kernelised Stein discrepancy and maximum mean discrepancy (mfm_stein_disc / mfm_max_mean_disc) vs the
float64 oracle (oracle/metrics.py, follows mcmc_utils.py:28-111).  Stated tolerance: 1e-5 relative (float32 pair
terms, float64 accumulation).

Measured on an MI355X, largest deviation of U or V in units of |V| (the tolerance is 1e-5): n in {2, 3, 63, 64, 65, 129} x beta in
{-0.25, -0.5, -0.9} at d = 2: 2.3e-7, d = 40: 2.4e-7, d = 42: 1.2e-7 (mfm_create accepts 42), d = 100: 2.3e-7; ragged chunk
(n = 2945): 9.4e-10; duplicated rows: 2.1e-8 (a U that drops every r2 = 0 pair misses by 25,711 tolerances); x = 1000 + N(0, 1):
7.1e-8 at d = 2, 3.7e-8 at d = 40 (r2 by the Gram expansion in float32 misses V by 1,004 / 32,199 tolerances and the MMD by 3,304 /
519,417).  MMD at m = 2, 65, 1000 (x against y, against itself and against a set 50 away): <= 0.01 of 1e-5 |mmd| + 1e-8."""
import numpy as np
import pytest

from oracle import metrics, prng

pytestmark = pytest.mark.gpu


def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).cuda()


@pytest.mark.parametrize("n", [256, 333])           # ragged: n not a multiple of the 64-pair tile
def test_stein_disc_phi4_matches_oracle(n):
    from tests import gpu_util as gu
    d = 64
    args, dist, k, model, state = gu.phi4_setup(d=d, B=64, hidden=32, F=16)
    ctx = gu.make_ctx(dist, args, fourier=model.f, params=state.params)
    rng = np.random.default_rng(5)
    x32 = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    g32 = dist.grad_logprob(x32.astype(np.float64)).astype(np.float32)
    u, v = ctx.stein_disc(_dev(x32), _dev(g32))
    # oracle on the SAME float32-rounded inputs
    uo, vo = metrics.stein_disc(x32.astype(np.float64), lambda x: g32.astype(np.float64))
    np.testing.assert_allclose([u, v], [uo, vo], rtol=1e-5)
    # permutation invariance (size-independent property)
    p = rng.permutation(n)
    u2, v2 = ctx.stein_disc(_dev(x32[p]), _dev(g32[p]))
    np.testing.assert_allclose([u2, v2], [u, v], rtol=1e-6)
    ctx.close()


def test_stein_and_mmd_mixture_match_oracle():
    from tests import gpu_util as gu
    args, dist, k, model, state = gu.gmm4_setup(B=64)
    ctx = gu.make_ctx(dist, args, fourier=model.f, params=state.params)
    rng = np.random.default_rng(6)
    n = 1000
    x32 = (8.0 * rng.choice([-1.0, 1.0], (n, 2)) + rng.standard_normal((n, 2))).astype(np.float32)
    y32 = (8.0 * rng.choice([-1.0, 1.0], (n, 2)) + 1.3 * rng.standard_normal((n, 2))).astype(np.float32)
    g32 = dist.grad_logprob(x32.astype(np.float64)).astype(np.float32)
    u, v = ctx.stein_disc(_dev(x32), _dev(g32))
    uo, vo = metrics.stein_disc(x32.astype(np.float64), lambda x: g32.astype(np.float64))
    np.testing.assert_allclose(v, vo, rtol=1e-5)
    np.testing.assert_allclose(u, uo, rtol=1e-5, atol=1e-5 * abs(vo))
    mmd = ctx.max_mean_disc(_dev(x32), _dev(y32))
    mo = metrics.max_mean_disc(x32.astype(np.float64), y32.astype(np.float64))
    np.testing.assert_allclose(mmd, mo, rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(ctx.max_mean_disc(_dev(y32), _dev(x32)), mmd, rtol=1e-6)        # symmetric (tile sums in another order)
    ctx.close()


# ---- edges of the all-pairs kernel (pair_sum_kernel<0|1>): tiny and tile-boundary n, other beta, d past one 32-coordinate LDS chunk,
# a ragged last chunk of j tiles, duplicated rows, a cloud far from the origin.  Oracle: oracle.metrics on the same float32-rounded
# inputs; tolerance: the 1e-5 relative stated above, U on V's scale (U = V's sum minus its diagonal, over n (n - 1)).
def _stein_np(x, g, beta=-0.5, r2=None, drop_zero=False):
    """oracle.metrics.stein_disc written out for PLANTED variants: `r2` replaces the pair distances, `drop_zero` takes the diagonal
    as "every pair with r2 == 0" instead of by index."""
    x, g = x.astype(np.float64), g.astype(np.float64)
    T, d = x.shape
    b = -beta
    diff = x[:, None, :] - x[None, :, :]
    r2 = (diff ** 2).sum(-1) if r2 is None else np.asarray(r2, dtype=np.float64)
    gd = ((g[:, None, :] - g[None, :, :]) * diff).sum(-1)
    term = -4 * b * (b + 1) * r2 / (1 + r2) ** (b + 2) + 2 * b * (d + gd) / (1 + r2) ** (1 + b) + (g @ g.T) / (1 + r2) ** b
    off = term[r2 != 0].sum() if drop_zero else term.sum() - np.trace(term)
    return off / (T * (T - 1)), term.sum() / T ** 2


def _gram_r2_f32(x, y):
    """The Gram-matrix expansion |x|^2 + |y|^2 - 2 x.y in float32: what the kernel's header says it avoids."""
    x, y = x.astype(np.float32), y.astype(np.float32)
    return ((x * x).sum(-1)[:, None] + (y * y).sum(-1)[None, :] - np.float32(2) * (x @ y.T)).astype(np.float32)


def _metric_ctx(d):
    from tests import gpu_util as gu
    if d == 2:
        args, dist, k, model, state = gu.gmm4_setup(B=16)
    else:
        args, dist, k, model, state = gu.phi4_setup(d=d, B=16, hidden=32, F=16)
    return dist, gu.make_ctx(dist, args, fourier=model.f, params=state.params)


def _check_stein(ctx, x32, g32, beta, tag):
    u, v = ctx.stein_disc(_dev(x32), _dev(g32), beta=beta)
    uo, vo = metrics.stein_disc(x32.astype(np.float64), lambda x: g32.astype(np.float64), beta=beta)
    print(f"stein {tag}: U {u:.10g} (oracle {uo:.10g}), V {v:.10g} (oracle {vo:.10g}); off by {abs(u - uo) / abs(vo):.1e}, {abs(v - vo) / abs(vo):.1e} of V")
    np.testing.assert_allclose(v, vo, rtol=1e-5)
    np.testing.assert_allclose(u, uo, rtol=1e-5, atol=1e-5 * abs(vo))
    return u, v, uo, vo


# d = 42: above one 32-coordinate chunk and no multiple of 4 (the loader's guard `k + e < d` cuts inside a quad of coordinates)
@pytest.mark.parametrize("d", [2, 40, 42, 100])
def test_stein_disc_small_n_and_other_beta_match_oracle(d):
    """n below one 64-pair tile, at its edge and one past it; beta of powf(base, -beta) and of the three coefficients."""
    dist, ctx = _metric_ctx(d)
    rng = np.random.default_rng(40 + d)
    for n in (2, 3, 63, 64, 65, 129):
        x32 = (dist.sample_model_rows(prng.split(prng.PRNGKey(n), n)) if d == 2 else rng.uniform(-1, 1, (n, d))).astype(np.float32)
        g32 = dist.grad_logprob(x32.astype(np.float64)).astype(np.float32)
        for beta in (-0.25, -0.5, -0.9):
            _check_stein(ctx, x32, g32, beta, f"d={d} n={n} beta={beta}")
    ctx.close()


def test_stein_disc_ragged_last_chunk_of_j_tiles():
    """n = 2945 at d = 2: 47 row tiles, the last holding one row; 2048 / 47 = 43 chunks of ceil(47 / 43) = 2 j tiles -> 24 chunks, the
    last with ONE tile (jt_hi cut at nj_tiles)."""
    dist, ctx = _metric_ctx(2)
    n = 2945
    x32 = dist.sample_model_rows(prng.split(prng.PRNGKey(8), n)).astype(np.float32)
    g32 = dist.grad_logprob(x32.astype(np.float64)).astype(np.float32)
    _check_stein(ctx, x32, g32, -0.5, "ragged chunk n=2945")
    ctx.close()


def test_stein_disc_duplicated_rows_stay_off_diagonal():
    """40 rows of which rows 10-19 repeat rows 0-9: the U-statistic drops the pairs i == j, not the pairs at distance 0."""
    dist, ctx = _metric_ctx(2)
    x32 = dist.sample_model_rows(prng.split(prng.PRNGKey(9), 40)).astype(np.float32)
    x32[10:20] = x32[:10]
    g32 = dist.grad_logprob(x32.astype(np.float64)).astype(np.float32)
    u, v, uo, vo = _check_stein(ctx, x32, g32, -0.5, "duplicates")
    up, vp = _stein_np(x32, g32, drop_zero=True)
    np.testing.assert_allclose(_stein_np(x32, g32), [uo, vo], rtol=1e-12)
    tol = 1e-5 * max(abs(uo), abs(vo))
    print(f"stein duplicates: planted U {up:.8g} misses the oracle by {abs(up - uo) / tol:.0f} tol, the device by {abs(up - u) / tol:.0f} tol")
    assert abs(up - uo) >= 10 * tol and abs(up - u) >= 10 * tol
    ctx.close()


@pytest.mark.parametrize("d", [2, 40])
def test_stein_and_mmd_far_from_the_origin(d):
    """x = 1000 + N(0, 1): squared distances must come from sum (x_i - x_j)^2.  The Gram expansion in float32 (planted, on the host)
    misses by >= 10 tolerances."""
    dist, ctx = _metric_ctx(d)
    rng = np.random.default_rng(70 + d)
    n = 129
    x32 = (1000.0 + rng.standard_normal((n, d))).astype(np.float32)
    y32 = (1000.0 + 1.3 * rng.standard_normal((n, d))).astype(np.float32)
    g32 = (-(x32.astype(np.float64) - 1000.0)).astype(np.float32)              # grad log N(1000, I)
    u, v, uo, vo = _check_stein(ctx, x32, g32, -0.5, f"far cloud d={d}")
    up, vp = _stein_np(x32, g32, r2=np.maximum(_gram_r2_f32(x32, x32), 0))
    assert abs(vp - vo) >= 10 * 1e-5 * abs(vo) and abs(vp - v) >= 10 * 1e-5 * abs(vo), (vp, vo, v)
    mmd = ctx.max_mean_disc(_dev(x32), _dev(y32))
    mo = metrics.max_mean_disc(x32.astype(np.float64), y32.astype(np.float64))
    ks = lambda r2: np.exp(-0.5 * np.maximum(r2.astype(np.float64), 0)).sum()
    m2 = n * n
    mp = (ks(_gram_r2_f32(x32, x32)) - n) / (m2 - n) - 2 * ks(_gram_r2_f32(x32, y32)) / m2 + (ks(_gram_r2_f32(y32, y32)) - n) / (m2 - n)
    tol = 1e-5 * abs(mo) + 1e-8
    print(f"far cloud d={d}: mmd {mmd:.10g} (oracle {mo:.10g}, off by {abs(mmd - mo) / tol:.2f} tol); planted Gram r2: V misses by {abs(vp - vo) / (1e-5 * abs(vo)):.0f} tol, mmd by {abs(mp - mo) / tol:.0f} tol")
    np.testing.assert_allclose(mmd, mo, rtol=1e-5, atol=1e-8)
    assert abs(mp - mo) >= 10 * tol and abs(mp - mmd) >= 10 * tol
    ctx.close()


@pytest.mark.parametrize("m", [2, 65, 1000])
def test_max_mean_disc_edges_match_oracle(m):
    """m below a tile, one past it and many tiles; X = Y; two sets 50 apart (every cross term underflows to 0); symmetry."""
    dist, ctx = _metric_ctx(2)
    rng = np.random.default_rng(90 + m)
    x32 = rng.standard_normal((m, 2)).astype(np.float32)
    y32 = (0.5 + 1.3 * rng.standard_normal((m, 2))).astype(np.float32)
    far = (y32 + np.float32(50.0)).astype(np.float32)
    for tag, a, b in (("x,y", x32, y32), ("x,x", x32, x32), ("50 apart", x32, far)):
        got = ctx.max_mean_disc(_dev(a), _dev(b))
        mo = metrics.max_mean_disc(a.astype(np.float64), b.astype(np.float64))
        print(f"mmd m={m} {tag}: {got:.10g} (oracle {mo:.10g}), off by {abs(got - mo) / (1e-5 * abs(mo) + 1e-8):.2f} tol")
        np.testing.assert_allclose(got, mo, rtol=1e-5, atol=1e-8)
        np.testing.assert_allclose(ctx.max_mean_disc(_dev(b), _dev(a)), got, rtol=1e-6, atol=1e-12)      # symmetric (tile sums in another order)
    ctx.close()


def test_run_returns_finite_metrics():
    """exe_flow_matching.run fills the reference's result vectors (:561): logpdf, KSD U / V, MMD, train time."""
    from mfm_amd import distributions as D, exe_flow_matching as E
    from oracle import loop
    modes, covs, w = 8.0 * np.array([[1, 1], [1, -1], [-1, 1], [-1, -1.0]]), np.ones((4, 2)), np.ones(4) / 4
    dg = D.GaussianMixture(modes, covs, w)
    args = loop.default_args(example="4-mode", dim=2, num_chain=64, learning_iter=6, mcmc_per_flow_steps=2.0, hutchs=False,
                             fourier_dim=16, hidden_x=[32, 32], hidden_t=[32, 32], hidden_xt=[32, 32], seed=3, eval_iter=2, step_size=0.2)
    res, res_ = E.run(dg, args, dg.sample_model, log_every=1000)
    assert np.all(np.isfinite(res)) and np.all(np.isfinite(res_))
    assert res[2] >= 0 and res_[2] >= 0            # V-statistics
