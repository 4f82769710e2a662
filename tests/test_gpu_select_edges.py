"""Edge-case parity of the decision kernels -- cis.hip (CIS categorical selection), smc.hip (ESS bisection, weights, the four
resampling schemes, choice_logw, acc_stats, gather_rows) and anneal.hip (beta bisection) -- against the float64 oracle on SYNTHETIC
inputs: no ODE solve runs here.  Their outputs are integers and accept / reject flags, so the comparisons are exact; the sizes are
those at which the one-wave lane loop (d = 100: ragged tail, d = 256: four passes) and the 1024-thread stride loops (n = 1, n not a
multiple of 64, n just past 1024, the 4096 / 8192 of the real configurations) take another path, and the tables include vanished,
overflowing and NaN weights.

Where a float64 device exp / log that differs from numpy's by an ulp could flip a decision, the oracle-side margin of every decision
is computed on the CPU (tests/select_cases.py) and asserted to clear its bound for the seeds used here: NO case is left out.  The
margins observed on the CPU are quoted in each docstring."""
import numpy as np
import pytest

from oracle import prng, smc, targets
from tests import select_cases as sc

pytestmark = pytest.mark.gpu


def _dev(x, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def _ctx(d=64, B=32, ref_dist="stdgauss", n_total=None, offset=0):
    from tests import gpu_util as gu
    if d == 2:
        args, dist, k, model, state = gu.gmm4_setup(B=B, ref_dist=ref_dist)
    else:
        args, dist, k, model, state = gu.phi4_setup(d=d, B=B, hidden=32, F=16, ref_dist=ref_dist)
    return gu.make_ctx(dist, args, n_local=B, n_total=n_total, offset=offset)


def _cis_run(ctx, key, n_is, inp, optional=True):
    """One mfm_cis_select launch on copies of the inputs; every buffer it may write comes back as numpy."""
    import torch
    B, d = inp["pos"].shape
    pos, logp, grad = _dev(inp["pos"]), _dev(inp["logp"]), _dev(inp["grad"])
    out = {}
    if optional:
        out = dict(acc=torch.full((B,), -7.0, device="cuda"), is_acc=torch.full((B,), 9, dtype=torch.uint8, device="cuda"),
                   proposed=torch.full((B, d), -7.0, device="cuda"), weight=torch.full((B,), -7.0, device="cuda"))
    ctx.cis_select(key, n_is, _dev(inp["u0"]), _dev(inp["vol0"]), _dev(inp["refs"]), _dev(inp["xs"]), _dev(inp["vols"]), _dev(inp["lps"]),
                   pos, logp, **out)
    ctx.sync()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update(pos=pos.cpu().numpy(), logp=logp.cpu().numpy(), grad=grad.cpu().numpy())
    return res


def _cis_check(got, inp, n_is, state, info, stats, rows=slice(None), equal_nan=False):
    """Exact decisions and copies; the two float32 weights are roundings of float64 values that agree to ~1e-12."""
    ch = sc.choice_from_pos(got["pos"], inp, n_is)
    np.testing.assert_array_equal(ch[rows], stats["choice"][rows])
    np.testing.assert_array_equal(got["is_acc"][rows], info.is_accepted[rows].astype(np.uint8))
    np.testing.assert_array_equal(got["pos"][rows], state.position.astype(np.float32)[rows])
    np.testing.assert_array_equal(got["proposed"][rows], info.proposed_position.astype(np.float32)[rows])
    np.testing.assert_array_equal(got["logp"][rows], state.logdensity[rows])
    np.testing.assert_array_equal(got["grad"], inp["grad"])                       # :295 the gradient is not refreshed
    np.testing.assert_allclose(got["acc"][rows], info.acceptance_rate[rows], rtol=1e-6, equal_nan=equal_nan)
    np.testing.assert_allclose(got["weight"][rows], info.proposed_weight[rows], rtol=1e-6, equal_nan=equal_nan)


# d, n_is, ref_dist, seed (inputs and key); seeds are the first for which the ORACLE alone has no chain within 1e-9 of a boundary
# and an accept rate inside (0.1, 0.9) -- see test_cis_select_regular
CIS_CASES = [(2, 1, "stdgauss", 0), (64, 5, "stdgauss", 0), (100, 33, "widegauss", 26), (256, 5, "stdgauss", 0)]
N_TOTAL, OFFSET, B_CIS = 96, 32, 32


def _cis_case(d, n_is, ref_dist, seed):
    ref_var = targets.REF_VARS[ref_dist]
    inp = sc.cis_inputs(d, n_is, B_CIS, ref_var, seed)
    key = prng.PRNGKey(1000 + seed)
    keys = prng.split_at(key, N_TOTAL, OFFSET + np.arange(B_CIS))
    return inp, key, sc.cis_oracle(inp, keys, n_is, ref_var)


@pytest.mark.parametrize("d,n_is,ref_dist,seed", CIS_CASES)
def test_cis_select_regular(d, n_is, ref_dist, seed):
    """32 local chains of 96 at chain_offset 32, O(1) log-weights.  Oracle-side margins min_b min_i |cum_i - r| observed on the CPU:
    1.2e-3, 4.4e-4, 2.8e-5, 2.2e-3 in the order of CIS_CASES (bound 1e-9); accept rates 0.31, 0.875, 0.875, 0.81.  With n_is = 33 exchangeable weights the expected accept rate is 33 / 34, so the seed of that
    case is one of the few whose draw keeps the current state in at least 4 of the 32 chains."""
    inp, key, (state, info, stats, margin) = _cis_case(d, n_is, ref_dist, seed)
    assert np.isfinite(stats["norm"]).all()
    assert (margin < 1e-9).sum() == 0, margin.min()
    assert 0.1 < info.is_accepted.mean() < 0.9, info.is_accepted.mean()
    ctx = _ctx(d, B_CIS, ref_dist, N_TOTAL, OFFSET)
    got = _cis_run(ctx, key, n_is, inp)
    print(f"cis d={d} n_is={n_is}: margin {margin.min():.3e} rate {info.is_accepted.mean():.3f} choices {np.bincount(stats['choice'], minlength=n_is + 1)}")
    _cis_check(got, inp, n_is, state, info, stats)
    bare = _cis_run(ctx, key, n_is, inp, optional=False)                 # NULL acc / is_acc / proposed / weight
    np.testing.assert_array_equal(bare["pos"], got["pos"])
    np.testing.assert_array_equal(bare["logp"], got["logp"])
    np.testing.assert_array_equal(bare["grad"], inp["grad"])
    ctx.close()


def test_cis_select_shard_matches_offset_context():
    """The chains of the d = 64 case as rows 32..63 of a 64-chain context at offset 0: the per-chain key is
    split(key, n_total)[chain_offset + b] either way, so every output matches the offset context bit for bit."""
    d, n_is, ref_dist, seed = CIS_CASES[1]
    inp, key, (state, info, stats, margin) = _cis_case(d, n_is, ref_dist, seed)
    other = sc.cis_inputs(d, n_is, B_CIS, 1.0, seed + 500)
    both = {k: np.concatenate([other[k], inp[k]]) for k in inp}
    ctx_a, ctx_b = _ctx(d, B_CIS, ref_dist, N_TOTAL, OFFSET), _ctx(d, 2 * B_CIS, ref_dist, N_TOTAL, 0)
    a, b = _cis_run(ctx_a, key, n_is, inp), _cis_run(ctx_b, key, n_is, both)
    for k in a:
        np.testing.assert_array_equal(b[k][B_CIS:], a[k], err_msg=k)
    _cis_check(a, inp, n_is, state, info, stats)
    ctx_a.close(); ctx_b.close()


def test_cis_select_degenerate_tables():
    """One launch, one scenario per chain (tests/select_cases.py: DEGENERATE; the indices are pinned on the CPU in
    tests/test_oracle_select_edges.py): the NaN-last order of searchsorted decides, a vanished table keeps the current state and an
    overflowing sample is the one selected.  The regular chains' margin observed on the CPU: 6.5e-3."""
    inp = sc.cis_degenerate_inputs()
    B, n_is, nd = inp["pos"].shape[0], 5, len(sc.DEGENERATE)
    key = prng.PRNGKey(77)
    state, info, stats, margin = sc.cis_oracle(inp, prng.split_at(key, B, np.arange(B)), n_is, 1.0)
    np.testing.assert_array_equal(stats["choice"][:nd], [e for _, _, e in sc.DEGENERATE])
    assert (margin[nd:] < 1e-9).sum() == 0
    ctx = _ctx(64, B)
    got = _cis_run(ctx, key, n_is, inp)
    print("cis degenerate: gpu", sc.choice_from_pos(got["pos"], inp, n_is), "oracle", stats["choice"], "margin", margin[nd:].min())
    _cis_check(got, inp, n_is, state, info, stats, equal_nan=True)
    ctx.close()


# ---- mfm_choice_logw ------------------------------------------------------------------------------------------------------------
CHOICE_PAIRS = [(1, 7), (50, 50), (1000, 1025), (1025, 64), (4133, 4133), (8192, 300)]


def _choice_case(n, m, spread):
    rng = np.random.default_rng(n + 3 * m + int(spread))
    return prng.PRNGKey(n * 7 + m), spread * rng.standard_normal(n)


def _choice_gpu(ctx, key, logw, m):
    import torch
    n = logw.shape[0]
    idx = torch.full((m,), -1, dtype=torch.int32, device="cuda"); scr = torch.empty(n, dtype=torch.float64, device="cuda")
    ctx.choice_logw(key, _dev(logw), m, scr, idx)
    ctx.sync()
    return idx.cpu().numpy()


def test_choice_logw_matches_oracle():
    """n tables against m draws on both sides of the 1024-thread stride, logw ~ N(0, 3^2) and N(0, 800^2) (most weights underflow to
    exact zeros, so the cumulative table is flat almost everywhere).  Relative margins min_j |cum - r_j| / tot observed on the CPU:
    1.5e-9 at (4133, 4133, sigma 3), 1.2e-7 or more everywhere else (bound 1e-12)."""
    ctx = _ctx()
    for n, m in CHOICE_PAIRS:
        for spread in (3.0, 800.0):
            key, logw = _choice_case(n, m, spread)
            want, margin = sc.choice_logw_oracle(key, logw, m)
            assert int(margin < 1e-12) == 0, (n, m, spread, margin)
            got = _choice_gpu(ctx, key, logw, m)
            print(f"choice_logw n={n} m={m} spread={spread}: margin {margin:.3e} distinct {np.unique(want).size}")
            np.testing.assert_array_equal(got, want, err_msg=f"n={n} m={m} spread={spread}")
    ctx.close()


@pytest.mark.parametrize("kind", ["all_neg_inf", "one_pos_inf", "one_nan"])
def test_choice_logw_non_finite(kind):
    """exp(logw - max) on non-finite log-weights: all -inf and one NaN poison the whole table (-inf - -inf, max = NaN: index 0 for
    every draw), one +inf leaves [0 .. 0, NaN, NaN ..] with a NaN query: the +inf entry is drawn every time."""
    n, m = 1000, 1025
    key, logw = _choice_case(n, m, 3.0)
    if kind == "all_neg_inf":
        logw[:] = -np.inf; expect = 0
    elif kind == "one_pos_inf":
        logw[613] = np.inf; expect = 613
    else:
        logw[613] = np.nan; expect = 0
    want, _ = sc.choice_logw_oracle(key, logw, m)
    np.testing.assert_array_equal(want, np.full(m, expect))
    ctx = _ctx()
    got = _choice_gpu(ctx, key, logw, m)
    np.testing.assert_array_equal(got, want)
    ctx.close()


# ---- the resampling schemes -----------------------------------------------------------------------------------------------------
SIZES = [1, 63, 65, 1000, 1025, 4133, 8192]
SCHEMES = ("systematic", "stratified", "multinomial", "residual")
KINDS = ("softmax", "dominant", "zeros", "equal")


def _resample_case(n, kind):
    rng = np.random.default_rng(n + 17 * KINDS.index(kind))
    return prng.PRNGKey(n * 31 + KINDS.index(kind)), sc.resample_weights(kind, n, rng)


def _resample_gpu(ctx, scheme, key, w):
    import torch
    from mfm_amd.bblackjax.smc import resampling as R
    n = w.shape[0]
    if scheme == "systematic":          # the dedicated kernel; the scheme entry point routes to it as well
        idx = torch.full((n,), -1, dtype=torch.int32, device="cuda"); scr = torch.empty(n, dtype=torch.float64, device="cuda")
        ctx.smc_resample(key, _dev(w), scr, idx)
        via_scheme = R.systematic(key, _dev(w), n).cpu().numpy()
        np.testing.assert_array_equal(via_scheme, idx.cpu().numpy())
        return idx.cpu().numpy()
    return getattr(R, scheme)(key, _dev(w), n).cpu().numpy()


@pytest.fixture
def smc_ctx():
    from types import SimpleNamespace
    from mfm_amd.bblackjax.smc import base as smc_base
    ctx = _ctx()
    smc_base._ENGINE[0] = SimpleNamespace(ctx=ctx)
    yield ctx
    smc_base._ENGINE[0] = None
    ctx.close()


@pytest.mark.parametrize("n", SIZES)
def test_resampling_schemes_match_oracle(n, smc_ctx):
    """Systematic and stratified queries are the same IEEE operations on both sides: bit-exact.  Multinomial and residual queries go
    through the device log (-log u): exact given that no query is within 1e-12 of a cumulative weight.  Margins observed on the CPU
    (min over kinds of the multinomial / residual queries, per n): 0.48, 4.1e-6, 2.0e-5, 8.2e-8, 2.7e-7, 1.3e-9, 1.3e-9."""
    for kind in KINDS:
        key, w = _resample_case(n, kind)
        for scheme in SCHEMES:
            with np.errstate(invalid="ignore", divide="ignore"):
                want = getattr(smc, scheme)(key, w, n)
                margin = sc.resample_margin(scheme, key, w)
            if scheme in ("multinomial", "residual"):
                assert int(margin < 1e-12) == 0, (n, kind, scheme, margin)
            got = _resample_gpu(smc_ctx, scheme, key, w)
            np.testing.assert_array_equal(got, want, err_msg=f"n={n} {kind} {scheme} margin={margin:.3e}")


def test_resampling_clips_unnormalised_weights(smc_ctx):
    """Weights that sum to 0.9: every query above the last cumulative weight finds nothing and takes the n - 1 clip of
    resampling.py:135 (np.clip in oracle/smc.py), about a tenth of the outputs.  Margins observed on the CPU: 3.1e-8, 1.4e-7, 3.2e-7."""
    n = 1025
    key, w = _resample_case(n, "softmax")
    w = 0.9 * w
    for scheme in ("systematic", "stratified", "multinomial"):
        want = getattr(smc, scheme)(key, w, n)
        raw = np.searchsorted(np.cumsum(w), sc.resample_queries(scheme, key, n))
        assert 0.05 * n < (raw == n).sum() < 0.15 * n and (want[raw == n] == n - 1).all()
        assert int(sc.resample_margin(scheme, key, w) < 1e-12) == 0
        np.testing.assert_array_equal(_resample_gpu(smc_ctx, scheme, key, w), want, err_msg=scheme)


# ---- ESS bisection, weights, beta bisection, acc_stats --------------------------------------------------------------------------
def _logliks(n, seed=0):
    return np.random.default_rng(100 + n + seed).standard_normal(n) * 40 - 300


@pytest.mark.parametrize("n", SIZES)
def test_smc_delta_weights_beta_sizes(n):
    """The project's tolerances (delta 1e-12 + 1e-9 |delta|, weights rtol 1e-12, lognorm 1e-10, beta 1e-9) at every stride count.
    Both bisections are sequences of decisions: the oracle's own f is never within 1e-9 of a decision boundary for these inputs
    (smallest margin per n observed on the CPU: 9.0e-5, 3.6e-8, 4.2e-7, 1.7e-6, 3.3e-7, 5.8e-8, 1.0e-6)."""
    import torch
    ctx = _ctx()
    ll = _logliks(n)
    for target, maxd in ((0.95, 1.0), (0.5, 0.3), (0.9, 1e-4)):
        d_o, margin = sc.delta_oracle(ll, target, maxd)
        assert int(margin < 1e-9) == 0, (n, target, maxd, margin)
        d_g = ctx.smc_delta(_dev(ll), target, maxd)
        assert abs(d_g - d_o) <= 1e-12 + 1e-9 * abs(d_o), (n, target, maxd, d_g, d_o)
    w = torch.empty(n, dtype=torch.float64, device="cuda")
    lognorm = ctx.smc_weights(_dev(ll), 0.037, w)
    lw = 0.037 * ll
    np.testing.assert_allclose(w.cpu().numpy(), np.exp(lw - smc.logsumexp(lw)), rtol=1e-12)
    assert abs(lognorm - (smc.logsumexp(lw) - np.log(n))) < 1e-10
    for prev, alpha in ((0.0, 0.9), (0.3, 0.5), (0.999, 0.9), (0.999, 0.9999)):
        b_o, sign, margin = sc.beta_oracle(prev, ll, alpha)
        assert int(margin < 1e-9) == 0, (n, prev, alpha, margin)
        b_g = ctx.beta_update(prev, _dev(ll), alpha)
        assert abs(b_g - b_o) < 1e-9, (n, prev, alpha, b_g, b_o, sign)
    ctx.close()


def test_smc_delta_degenerate():
    """All-equal log-likelihoods (ESS = n at every delta -> max_delta), target_ess = 1 (f_a = 2 L - L - L = 0 exactly, not > 0 -> NaN,
    solver.py:76-81, which the clip of adaptive_tempered.py:70 propagates), -inf entries (nan_to_num -> +max double at delta > 0,
    0 * inf = NaN -> 0 at delta = 0: f_b = inf - inf = NaN, the loop test fails at once -> delta = 0) and one NaN entry
    (nan_to_num -> 0; margins observed on the CPU: 3.8e-6, 5.9e-6, 1.9e-6)."""
    ctx = _ctx()
    for n in (65, 1025, 8192):
        ll = _logliks(n)
        flat = np.full(n, -123.456)
        d_o, _ = sc.delta_oracle(flat, 0.9, 0.37)
        assert d_o == 0.37 and ctx.smc_delta(_dev(flat), 0.9, 0.37) == 0.37
        d_o, _ = sc.delta_oracle(ll, 1.0, 1.0)
        assert np.isnan(d_o) and np.isnan(ctx.smc_delta(_dev(ll), 1.0, 1.0)), (n, d_o)
        inf = ll.copy(); inf[[3, n // 2, n - 1]] = -np.inf
        d_o, _ = sc.delta_oracle(inf, 0.9, 1.0)
        assert d_o == 0.0 and ctx.smc_delta(_dev(inf), 0.9, 1.0) == 0.0
        nan = ll.copy(); nan[n // 3] = np.nan
        d_o, margin = sc.delta_oracle(nan, 0.9, 1.0)
        assert int(margin < 1e-9) == 0 and 0.0 < d_o < 1.0
        d_g = ctx.smc_delta(_dev(nan), 0.9, 1.0)
        assert abs(d_g - d_o) <= 1e-12 + 1e-9 * abs(d_o), (n, d_g, d_o)
    ctx.close()


def test_beta_update_no_bracket():
    """Flat log-likelihoods: ess_zero = n (1 - alpha) > 0 at both ends, sign = 0, every step moves ``low`` and the 30th midpoint is
    returned."""
    ctx = _ctx()
    for n in (1, 1025, 8192):
        flat = np.full(n, -45.6)
        b_o, sign, margin = sc.beta_oracle(0.25, flat, 0.9)
        assert sign == 0 and margin > 1e-9 and b_o == 1.0 - 0.75 * 2.0 ** -30
        assert ctx.beta_update(0.25, _dev(flat), 0.9) == b_o
    ctx.close()


def test_acc_stats_sizes():
    import torch
    ctx = _ctx()
    for n in (1, 1000, 1025, 4133):
        x = np.random.default_rng(n).uniform(0.0, 1.5, n).astype(np.float32)
        out = torch.full((2,), np.nan, dtype=torch.float64, device="cuda")
        ctx.acc_stats(_dev(x), out)
        ctx.sync()
        x64 = x.astype(np.float64)
        np.testing.assert_allclose(out.cpu().numpy(), [x64.sum(), (x64 * x64).sum()], rtol=1e-9)
    ctx.close()


# ---- gather_rows ----------------------------------------------------------------------------------------------------------------
def test_gather_rows_shapes():
    """Rows of a source with 3 n rows: random indices with repeats, the identity on the first n rows, the last source row."""
    import torch
    ctx = _ctx()
    for dim in (1, 2, 100, 256):
        for n in (1, 1025):
            rng = np.random.default_rng(dim * 3 + n)
            src = rng.standard_normal((3 * n, dim)).astype(np.float32)
            rand = rng.integers(0, 3 * n, n); rand[-1] = 3 * n - 1; rand[n // 2:n // 2 + 3] = rand[0]
            for idx in (rand, np.arange(n), np.full(n, 3 * n - 1)):
                dst = torch.full((n, dim), np.nan, device="cuda")
                ctx.gather_rows(_dev(src), _dev(idx.astype(np.int32)), dst)
                ctx.sync()
                np.testing.assert_array_equal(dst.cpu().numpy(), src[idx], err_msg=f"dim={dim} n={n}")
    ctx.close()
