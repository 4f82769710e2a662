"""GPU tests of ``mfm_chain_sums`` / ``mfm_chain_diag`` (mfm_amd/csrc/diag.hip), of ``mfm_amd.diagnostics`` and of the figures that
``--ess_steps`` logs from them.

Yardstick: the float64 oracle ``tests/chain_diag_oracle.py`` (direct lag sums, ``np.var``) on the SAME float32 inputs.

Figures, per case and ``split`` (every test prints them before it asserts):

* ``mom``: largest relative error of ``sums[0]``, ``sums[1]``, ``sums[2]`` (float64 moments; section 4.9 of DESIGN.md measured 1e-12 for the
  like quantities of ``mfm_autocorr``, which is the ceiling here);
* ``lag``: largest ``|sums[2 + k] - oracle| / sums[2]`` over ``k >= 1`` (float32 products inside ``AUTOCORR_TIME_BLOCK`` steps, float64 across);
* ``rho``: largest ``|rho - oracle|``; ``rhat`` and ``tau``: largest relative errors of ``rhat`` and of ``tau`` / ``ess``.

``MEASURED`` holds what an MI355X gave; the bound of a figure is ``MARGIN = 4`` times it (the margin section 4.9 gives for FMA contraction
and summation order), never below a floor: 1e-13 for ``mom`` (a float64 sum of up to 515 terms of size 3 in another order than numpy's:
n eps), half a float32 ulp (6e-8) for the float32 outputs.  Whatever was measured, 1e-5 (relative for ``tau`` / ``ess`` / ``rhat``, absolute
for ``rho``, and for ``lag``) is the line above which the accumulation scheme is wrong.

Geyer's truncation point is a decision: a coordinate any of whose oracle ``Gamma_m``, up to and including its first non-positive one,
is within 1e-4 of zero is "borderline" (at most 2 % of a case's coordinates); its ``tau`` must then equal the oracle's sum truncated at
one of the neighbouring stopping points.  The oracle finds 1 of 70 in ``two_cblocks`` and 1 of 130 in ``three_cblocks...``, at ``split = 1`` and
at ``split = 0`` alike, and none elsewhere (two ``split = 0`` runs after their seed was replaced: ``SEED_SPLIT0``).
"""
import functools

import numpy as np
import pytest

from tests import chain_diag_oracle as co

pytestmark = pytest.mark.gpu

MARGIN = 4.0
F32_FLOOR, F64_FLOOR = 6e-8, 1e-13
CEIL = dict(mom=1e-12, lag=1e-5, rho=1e-5, rhat=1e-5, tau=1e-5)
MAX_BORDER = 0.02

# (n, B, d, n_lags, seed)
CASES = {
    "smallest": (64, 16, 3, 31, 0),
    "two_cblocks": (257, 48, 70, 64, 1),
    "n_sub_eq_time_block": (512, 64, 16, 255, 2),
    "odd_n_odd_chains_small_dim": (101, 33, 2, 50, 3),
    "three_cblocks_lag_block_plus_1": (200, 16, 130, 33, 4),
    "time_block_plus_1_all_lags": (514, 24, 5, 257, 5),
    "odd_n_at_time_block": (515, 24, 5, 256, 6),
    "padded": (96, 40, 64, 40, 10),
}
# split = 0 of these two has borderline coordinates with the seed above (2 of 16 and 1 of 5: past the 2 % cap): the seed is replaced
SEED_SPLIT0 = {"n_sub_eq_time_block": 21, "time_block_plus_1_all_lags": 20}
CASE_IDS = [(name, split) for name in CASES for split in (1, 0)]

# measured on an MI355X (this file's own printout): (case, split) -> (mom, lag, rho, rhat, tau); bound = MARGIN x max(measured, floor)
MEASURED = {
    ("smallest", 1): (4.44e-16, 1.94e-08, 2.28e-08, 5.86e-08, 3.64e-08),
    ("smallest", 0): (0.00e+00, 2.30e-08, 3.99e-08, 3.75e-08, 3.98e-08),
    ("two_cblocks", 1): (6.66e-16, 2.31e-08, 4.58e-08, 5.88e-08, 5.78e-08),
    ("two_cblocks", 0): (2.22e-16, 7.47e-08, 8.02e-08, 5.85e-08, 7.49e-08),
    ("n_sub_eq_time_block", 1): (6.66e-16, 2.71e-08, 4.47e-08, 5.14e-08, 5.32e-08),
    ("n_sub_eq_time_block", 0): (5.55e-16, 1.66e-08, 3.77e-08, 5.37e-08, 5.33e-08),
    ("odd_n_odd_chains_small_dim", 1): (4.44e-16, 6.17e-09, 5.85e-09, 4.31e-08, 2.37e-08),
    ("odd_n_odd_chains_small_dim", 0): (0.00e+00, 8.11e-09, 8.12e-09, 3.97e-08, 2.26e-08),
    ("three_cblocks_lag_block_plus_1", 1): (6.66e-16, 4.61e-08, 6.85e-08, 5.91e-08, 7.35e-08),
    ("three_cblocks_lag_block_plus_1", 0): (2.22e-16, 1.16e-07, 1.15e-07, 5.91e-08, 1.09e-07),
    ("time_block_plus_1_all_lags", 1): (4.44e-16, 3.44e-08, 4.94e-08, 5.77e-08, 4.47e-08),
    ("time_block_plus_1_all_lags", 0): (2.22e-16, 1.71e-08, 3.34e-08, 4.42e-08, 4.42e-08),
    ("odd_n_at_time_block", 1): (4.44e-16, 3.12e-08, 4.50e-08, 4.85e-08, 4.17e-08),
    ("odd_n_at_time_block", 0): (4.44e-16, 3.18e-08, 4.37e-08, 5.65e-08, 4.38e-08),
    ("padded", 1): (8.88e-16, 2.41e-08, 4.64e-08, 5.71e-08, 5.81e-08),
    ("padded", 0): (4.44e-16, 3.95e-08, 4.55e-08, 5.81e-08, 6.46e-08),
}
# 256 MALA steps, 64 chains, split = 1, all 128 lags: target -> (mom, lag, rho, rhat, tau)
E2E_MEASURED = {
    "phi4": (9.99e-16, 5.84e-08, 3.00e-08, 4.98e-08, 5.40e-08),
    "4-mode": (6.66e-16, 4.11e-08, 2.99e-08, 9.54e-09, 3.80e-08),
}
# the stuck-chain arrays (seed 0: 5.55e-16, 6.83e-09, 2.87e-08, 4.98e-08, 4.40e-08; seed 7, the additivity test: 4.44e-16, 1.78e-08, 2.97e-08,
# 5.28e-08, 4.28e-08): the larger of the two per figure
STUCK_MEASURED = (5.55e-16, 1.78e-08, 2.97e-08, 5.28e-08, 4.40e-08)


def _bounds(measured):
    mom, lag, rho, rhat, tau = measured
    b = dict(mom=MARGIN * max(mom, F64_FLOOR), lag=MARGIN * max(lag, F32_FLOOR), rho=MARGIN * max(rho, F32_FLOOR),
             rhat=MARGIN * max(rhat, F32_FLOOR), tau=MARGIN * max(tau, F32_FLOOR))
    return {k: min(v, CEIL[k]) for k, v in b.items()}


@functools.lru_cache(maxsize=None)
def _oracle(name, split):
    """(x float32 [n, B, d], oracle dict, oracle sums) of a case; computed once and handed out read-only."""
    n, B, d, L, seed = CASES[name]
    x = co.case_data(n, B, d, seed if split else SEED_SPLIT0.get(name, seed))
    o = co.diag(x, L, bool(split))
    s = co.sums(x, L, bool(split))
    for a in [x, s] + [v for v in o.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return x, o, s


@pytest.fixture(scope="module")
def ctx():
    from mfm_amd import _lib
    c = _lib.Context(dim=2, n_chain_local=16, fourier_dim=16, hidden_t=(16, 16), hidden_x=(16, 16), hidden_xt=(16, 16))
    yield c
    c.close()


def _dev(x):
    import torch
    return x if torch.is_tensor(x) else torch.tensor(np.asarray(x), device="cuda")       # (a copy: the oracle's arrays are read-only)


def _run(ctx, x, L, split, n_chain=None, chain_offset=0, want=("rhat", "ess", "tau", "rho")):
    """One chain_sums + one chain_diag; every buffer pre-filled with a marker so that an element nobody wrote shows."""
    import torch
    xd = _dev(x)
    d = xd.shape[2]
    sums = torch.full((L + 2, d), -7.0, device="cuda", dtype=torch.float64)
    n_sub, M = ctx.chain_sums(xd, sums, n_chain=n_chain, split=bool(split), chain_offset=chain_offset)
    out = _diag(ctx, sums, n_sub, M, want)
    out.update(sums=sums.cpu().numpy(), n_sub=n_sub, M=M)
    return out


def _diag(ctx, sums, n_sub, M, want=("rhat", "ess", "tau", "rho")):
    import torch
    L, d = sums.shape[0] - 2, sums.shape[1]
    out = {k: torch.full((L, d) if k == "rho" else (d,), -7.0, device="cuda") for k in want}
    ctx.chain_diag(sums, n_sub, M, **out)
    ctx.sync()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _compare(tag, got, o, osums, bounds):
    """Print the five figures of the module docstring, then assert them against ``bounds``; returns the figures."""
    from tests.test_gpu_autocorr import _check_tau
    assert got["n_sub"] == o["n_sub"] and got["M"] == o["M"]
    s = got["sums"]
    fig = dict(mom=np.abs(s[:3] / osums[:3] - 1.0).max(),
               lag=(np.abs(s[3:] - osums[3:]) / osums[2][None]).max(initial=0.0))
    assert (np.isnan(got["rho"]) == np.isnan(o["rho"])).all()
    fig["rho"] = np.nanmax(np.abs(got["rho"].astype(np.float64) - o["rho"]), initial=0.0)
    fig["rhat"] = np.nanmax(np.abs(got["rhat"].astype(np.float64) / o["rhat"] - 1.0), initial=0.0)
    print(f"[chain_diag] {tag}: mom {fig['mom']:.3g} (bound {bounds['mom']:.3g}), lag {fig['lag']:.3g} ({bounds['lag']:.3g}), "
          f"rho {fig['rho']:.3g} ({bounds['rho']:.3g}), rhat {fig['rhat']:.3g} ({bounds['rhat']:.3g})")
    fig["tau"] = _check_tau("chain_diag " + tag, o["M"] * o["n_sub"], got["tau"], got["ess"], o["tau"], o["m_stop"], o["G"], bounds["tau"],
                            max_border=MAX_BORDER)
    print(f"[chain_diag] {tag}: FIGURES ({fig['mom']:.2e}, {fig['lag']:.2e}, {fig['rho']:.2e}, {fig['rhat']:.2e}, {fig['tau']:.2e})")
    for k in ("mom", "lag", "rho", "rhat"):
        assert fig[k] <= CEIL[k], (tag, k, fig[k])
        assert fig[k] <= bounds[k], (tag, k, fig[k], bounds[k])
    assert (got["rho"][0] == 1.0).all()                             # 1 - 0 / var+
    return fig


@pytest.mark.parametrize("name,split", CASE_IDS)
def test_against_the_float64_oracle(ctx, name, split):
    n, B, d, L, seed = CASES[name]
    x, o, osums = _oracle(name, split)
    got = _run(ctx, x, L, split)
    _compare(f"{name} split={split} {(n, B, d, L)}", got, o, osums, _bounds(MEASURED[(name, split)]))


@pytest.mark.parametrize("split", [1, 0])
def test_padding_chains_never_reach_an_output(ctx, split):
    """n_chain_ld = 48 with 8 padding chains of NaN behind the 40 valid ones: the same bits as the trajectory without them."""
    n, B, d, L, seed = CASES["padded"]
    x, o, osums = _oracle("padded", split)
    padded = np.full((n, 48, d), np.nan, dtype=np.float32)
    padded[:, :B] = x
    got = _run(ctx, padded, L, split, n_chain=B)
    plain = _run(ctx, x, L, split)
    for k in ("sums", "rhat", "ess", "tau", "rho"):
        assert np.isfinite(got[k]).all(), k
        np.testing.assert_array_equal(got[k], plain[k], err_msg=k)
    _compare(f"padded ld=48 split={split}", got, o, osums, _bounds(MEASURED[("padded", split)]))


def test_stuck_chains_on_the_device(ctx):
    x = co.stuck()
    n, B, d = x.shape
    L = n // 2
    got = _run(ctx, x, L, 1)
    assert got["rhat"][0] > 3.0 and (got["rhat"][1:] < 1.05).all()
    assert got["ess"][0] < 0.1 * got["ess"][1:].min()
    _compare("stuck", got, co.diag(x, L), co.sums(x, L), _bounds(STUCK_MEASURED))


def test_sums_are_additive_over_chain_sets_and_the_diagnostics_follow(ctx):
    import torch
    x = co.stuck(seed=7)                                            # 32 chains
    n, B, d = x.shape
    L = n // 2
    xd = _dev(x)
    whole = _run(ctx, xd, L, 1)
    lo = _run(ctx, xd, L, 1, n_chain=16)
    hi = _run(ctx, xd, L, 1, n_chain=16, chain_offset=16)          # a pointer offset; n_chain_ld stays 32
    added = lo["sums"] + hi["sums"]
    np.testing.assert_allclose(added, whole["sums"], rtol=1e-12, atol=0)
    o, osums = co.diag(x, L), co.sums(x, L)
    d_added = _diag(ctx, torch.from_numpy(added).cuda(), lo["n_sub"], lo["M"] + hi["M"])
    d_added.update(sums=added, n_sub=lo["n_sub"], M=lo["M"] + hi["M"])
    _compare("additivity", d_added, o, osums, _bounds(STUCK_MEASURED))
    np.testing.assert_allclose(d_added["rhat"], whole["rhat"], rtol=4 * F32_FLOOR)


@pytest.mark.parametrize("name,split", [("two_cblocks", 1), ("odd_n_odd_chains_small_dim", 1), ("odd_n_odd_chains_small_dim", 0)])
def test_same_call_twice_gives_the_same_bits_and_rho_changes_nothing(ctx, name, split):
    n, B, d, L, seed = CASES[name]
    x = _dev(_oracle(name, split)[0])
    a, b = _run(ctx, x, L, split), _run(ctx, x, L, split)
    np.testing.assert_array_equal(a["sums"].view(np.int64), b["sums"].view(np.int64))
    for k in ("rhat", "ess", "tau", "rho"):
        np.testing.assert_array_equal(a[k].view(np.int32), b[k].view(np.int32), err_msg=k)
    no_rho = _run(ctx, x, L, split, want=("rhat", "ess", "tau"))
    for k in ("rhat", "ess", "tau"):
        np.testing.assert_array_equal(a[k].view(np.int32), no_rho[k].view(np.int32), err_msg=k)
    one = _run(ctx, x, L, split, want=("tau",))                    # a single output is a valid request
    np.testing.assert_array_equal(a["tau"].view(np.int32), one["tau"].view(np.int32))


@pytest.mark.parametrize("name", ["two_cblocks", "odd_n_odd_chains_small_dim"])
def test_potential_scale_reduction_is_the_rhat_of_chain_diagnostics(name):
    import torch
    from mfm_amd import diagnostics
    n, B, d, L, seed = CASES[name]
    x, o, _ = _oracle(name, 1)
    xd = _dev(x)
    cd = diagnostics.chain_diagnostics(xd)
    psr = diagnostics.potential_scale_reduction(xd)
    assert psr.is_cuda and psr.shape == (d,) and all(v.is_cuda and v.shape == (d,) for v in cd)
    assert torch.equal(psr.view(torch.int32), cd.rhat.view(torch.int32))
    np.testing.assert_allclose(psr.cpu().numpy(), o["rhat"], rtol=CEIL["rhat"])
    whole = diagnostics.potential_scale_reduction(x, split=False)   # numpy in, numpy out
    assert isinstance(whole, np.ndarray)
    np.testing.assert_allclose(whole, co.diag(x, 1, False)["rhat"], rtol=CEIL["rhat"])
    part = diagnostics.chain_diagnostics(xd, max_lag=L, n_valid=B - 5)
    op = co.diag(x[:, :B - 5], L)
    np.testing.assert_allclose(part.rhat.cpu().numpy(), op["rhat"], rtol=CEIL["rhat"])


@pytest.mark.parametrize("target", ["phi4", "4-mode"])
def test_end_to_end_on_a_mala_run(target):
    """256 MALA steps in one launch, then the cross-chain diagnostics on the trajectory where it lies."""
    from mfm_amd import diagnostics, mcmc_utils, random as jr
    from mfm_amd.bblackjax.mcmc.mala import mala
    from tests.test_gpu_autocorr import _engine
    eng, dist, args, pos = _engine(target)
    algo = mala(dist.logprob, args.step_size)
    _, info = algo.step.run(jr.PRNGKey(11), algo.init(pos), 256, thin=1)
    traj = info.positions
    n, B, d = traj.shape
    assert (n, B) == (256, 64)
    host = traj.cpu().numpy()
    L = n // 2
    o, osums = co.diag(host, L), co.sums(host, L)
    got = _run(mcmc_utils._diag_ctx(), traj, L, 1)
    _compare("e2e " + target, got, o, osums, _bounds(E2E_MEASURED[target]))
    cd = diagnostics.chain_diagnostics(traj)                       # CUDA in, CUDA out; max_lag defaults to n_sub
    assert all(v.is_cuda and v.shape == (d,) for v in cd)
    as_numpy = diagnostics.chain_diagnostics(host)                 # numpy in, numpy out
    for k, v in zip(cd._fields, as_numpy):
        assert isinstance(v, np.ndarray)
        np.testing.assert_array_equal(v, got[k], err_msg=k)
        np.testing.assert_array_equal(getattr(cd, k).cpu().numpy(), got[k], err_msg=k)
    eng.close()


def _bits(d):
    return {k: v.view(np.int32 if v.dtype == np.float32 else np.int64) for k, v in d.items() if isinstance(v, np.ndarray)}


@pytest.mark.parametrize("n,B,d,L", [(100, 12, 70, 40), (100, 12, 5, 40)])
def test_constant_coordinate_is_nan_in_its_own_outputs_only(ctx, n, B, d, L):
    x = co.case_data(n, B, d, 0).copy()
    clean = _bits(_run(ctx, x, L, 1))
    j = d - 2
    x[:, :, j] = 2.5                                                # constant in every chain: W = 0
    got = _run(ctx, x, L, 1)
    for k in ("rhat", "ess", "tau", "rho"):
        assert np.isnan(got[k][..., j]).all(), k
    assert (got["sums"][2:, j] == 0.0).all() and got["sums"][0, j] == 2.5 * got["M"]
    others = np.arange(d) != j
    for k, v in _bits(got).items():
        assert np.isfinite(got[k][..., others]).all(), k
        np.testing.assert_array_equal(v[..., others], clean[k][..., others], err_msg=k)


@pytest.mark.parametrize("n,B,d,L", [(100, 12, 70, 40), (100, 12, 5, 40)])
def test_one_inf_spoils_its_own_coordinate_only(ctx, n, B, d, L):
    x = co.case_data(n, B, d, 0).copy()
    clean = _bits(_run(ctx, x, L, 1))
    j = d - 1
    x[51, 7, j] = np.inf
    got = _run(ctx, x, L, 1)
    for k in ("rhat", "ess", "tau", "rho"):
        assert np.isnan(got[k][..., j]).all(), k
    others = np.arange(d) != j
    for k, v in _bits(got).items():
        assert np.isfinite(got[k][..., others]).all(), k
        np.testing.assert_array_equal(v[..., others], clean[k][..., others], err_msg=k)


def test_argument_errors_name_the_argument(ctx):
    import ctypes as C
    import torch
    from mfm_amd import _lib
    x = torch.zeros((8, 4, 3), device="cuda")
    sums = torch.zeros((4, 3), device="cuda", dtype=torch.float64)
    out = torch.zeros(3, device="cuda")
    px, ps, po = C.c_void_p(x.data_ptr()), C.c_void_p(sums.data_ptr()), C.c_void_p(out.data_ptr())
    f, g = ctx.lib.mfm_chain_sums, ctx.lib.mfm_chain_diag

    def err(fn, *args):
        assert fn(ctx.h, *args) == -1                               # MFM_EINVAL
        return ctx.lib.mfm_last_error().decode()

    # mfm_chain_sums(ctx, d_x, n, n_chain, n_chain_ld, dim, split, n_lags, d_sums)
    assert "n_sub" in err(f, px, 3, 4, 4, 3, 1, 1, ps)              # n = 3 split: n_sub = 1
    assert "n_sub" in err(f, px, 1, 4, 4, 3, 0, 1, ps)
    assert "n_chain" in err(f, px, 8, 0, 4, 3, 1, 2, ps)
    assert "n_chain" in err(f, px, 8, 5, 4, 3, 1, 2, ps)
    assert "dim" in err(f, px, 8, 4, 4, 0, 1, 2, ps)
    assert "n_lags" in err(f, px, 8, 4, 4, 3, 1, 0, ps)
    assert "n_lags" in err(f, px, 8, 4, 4, 3, 1, 5, ps)             # n_sub = 4
    assert "split" in err(f, px, 8, 4, 4, 3, 2, 2, ps)
    assert "d_x" in err(f, None, 8, 4, 4, 3, 1, 2, ps)
    assert "d_sums" in err(f, px, 8, 4, 4, 3, 1, 2, None)
    assert f(ctx.h, px, 8, 4, 4, 3, 0, 2, ps) == 0
    # mfm_chain_diag(ctx, d_sums, n_sub, n_subchains, dim, n_lags, d_rhat, d_ess, d_tau, d_rho)
    assert "n_sub" in err(g, ps, 1, 8, 3, 1, po, None, None, None)
    assert "n_subchains" in err(g, ps, 4, 1, 3, 2, po, None, None, None)
    assert "dim" in err(g, ps, 4, 8, 0, 2, po, None, None, None)
    assert "n_lags" in err(g, ps, 4, 8, 3, 0, po, None, None, None)
    assert "n_lags" in err(g, ps, 4, 8, 3, 5, po, None, None, None)
    assert "d_sums" in err(g, None, 4, 8, 3, 2, po, None, None, None)
    assert "output" in err(g, ps, 4, 8, 3, 2, None, None, None, None)
    assert g(ctx.h, ps, 8, 4, 3, 2, po, None, None, None) == 0
    ctx.sync()
    with pytest.raises(_lib.MfmError, match="float32"):
        ctx.chain_sums(x.double(), sums)
    with pytest.raises(_lib.MfmError, match="float64"):
        ctx.chain_sums(x, sums.float())
    with pytest.raises(_lib.MfmError, match="contiguous"):
        ctx.chain_sums(x[:, :2], sums)
    with pytest.raises(_lib.MfmError, match="n_chain"):
        ctx.chain_sums(x, sums, n_chain=0)
    with pytest.raises(_lib.MfmError, match="chain_offset"):
        ctx.chain_sums(x, sums, n_chain=3, chain_offset=2)
    with pytest.raises(_lib.MfmError, match="shape"):
        ctx.chain_diag(sums, 4, 8, rhat=torch.zeros(4, device="cuda"))


@pytest.mark.parametrize("kernel", ["hmc", "mala"])
def test_ess_steps_logs_the_cross_chain_figures(kernel):
    """``--ess_steps`` with the arguments of ``test_ess_steps_with_the_hmc_kernel``: the new keys, recomputed here from the trajectory
    reproduced from the same chains and key; the per-chain keys keep their values."""
    from mfm_amd import diagnostics, distributions as D, exe_flow_matching as E, mcmc_utils, random as jr
    from oracle import loop
    kw = dict(example="phi-four", dim=64, num_chain=32, learning_iter=5, mcmc_per_flow_steps=4.0, hutchs=True, fourier_dim=16, seed=7, eval_iter=1,
              step_size=0.03, hidden_x=[32, 32], hidden_t=[32, 32], hidden_xt=[32, 32], ess_steps=64)
    dist = D.PhiFour(64)
    if kernel == "hmc":
        from mfm_amd.bblackjax.mcmc.hmc import hmc
        args = loop.default_args(mcmc_kernel="hmc", hmc_steps=4, **kw)
    else:
        from mfm_amd.bblackjax.mcmc.mala import mala
        args = loop.default_args(mcmc_kernel="mala", **dict(kw, step_size=1e-4))
    _, _, ex = E.run(dist, args, None, log_every=1000, return_extras=True)
    eng = ex["engine"]
    new = ["rhat_max", "rhat_median", "ess_multichain_per_step_min", "ess_multichain_per_step_median", "ess_multichain_per_step_mean"]
    grad = ["ess_multichain_per_grad_min", "ess_multichain_per_grad_median", "ess_multichain_per_grad_mean"]
    for k in new + (grad if kernel == "hmc" else []):
        assert isinstance(ex[k], float) and np.isfinite(ex[k]), k
    assert not (kernel == "mala" and any(k in ex for k in grad))
    assert ex["rhat_max"] >= ex["rhat_median"] > 0.9
    algo = hmc(dist.logprob, args.step_size, 4) if kernel == "hmc" else mala(dist.logprob, args.step_size)
    _, info = algo.step.run(jr.split(ex["key_gen"], 3)[2], algo.init(ex["states"].position), 64, thin=1)
    cd = diagnostics.chain_diagnostics(info.positions, n_valid=eng.n_valid, ctx=eng.ctx)
    multi = cd.ess.double() / (32 * 64)
    assert ex["rhat_max"] == cd.rhat.double().max().item() and ex["rhat_median"] == cd.rhat.double().median().item()
    assert ex["ess_multichain_per_step_min"] == multi.min().item()
    assert ex["ess_multichain_per_step_median"] == multi.median().item()
    assert ex["ess_multichain_per_step_mean"] == multi.mean().item()
    if kernel == "hmc":
        for name in ("min", "median", "mean"):
            assert ex["ess_multichain_per_grad_" + name] == ex["ess_multichain_per_step_" + name] / 4
    ess, _ = mcmc_utils.effective_sample_size(info.positions[:, :eng.n_valid], ctx=eng.ctx)      # the per-chain keys: unchanged
    per_step = (ess.double() / 64).reshape(-1)
    for name, want in (("min", per_step.min().item()), ("median", per_step.median().item()), ("mean", per_step.mean().item())):
        # (a MALA chain that no proposal moved in a coordinate is a constant series: NaN per chain, then and now; W > 0 keeps the new keys finite)
        np.testing.assert_array_equal(np.float64(ex["ess_per_step_" + name]), np.float64(want), err_msg=name)
    eng.close()
