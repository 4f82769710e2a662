"""GPU tests of ``mfm_autocorr`` (mfm_amd/csrc/diag.hip) and of ``mcmc_utils.autocorrelation`` / ``effective_sample_size``.

Yardstick: the float64 direct-sum oracle ``tests/autocorr_oracle.py`` on the SAME float32 inputs (``ar1(n, S, 0)``).

Tolerances.  The kernel sums float32 products of the float64-centred signal in float32 inside ``AUTOCORR_TIME_BLOCK`` time steps and in
float64 across, stores the lag sums as float32 and divides in float64.  ``MEASURED`` holds, per case, the largest ``|rho - oracle|`` and
the largest relative error of ``tau`` observed on an MI355X (every test prints its figures before it asserts); the bound of a case is
``MARGIN = 4`` times that: the margin covers FMA contraction and the summation order of other inputs.  A float64 oracle value rounded to
float32 is already 6e-8 away, which is the floor used where the measured figure is smaller (exact cases).  Anything above 1e-5 at
n <= 1000 would mean the accumulation scheme is wrong.

Geyer's truncation point is a decision: a series any of whose oracle ``Gamma_m``, up to and including its first non-positive one, has
``|Gamma_m| < 1e-4`` is "borderline" (at most 3 % of a case's series); its ``tau`` must then equal the oracle's sum truncated at one of
the neighbouring stopping points.
"""
import functools

import numpy as np
import pytest

from tests import autocorr_oracle as ao

pytestmark = pytest.mark.gpu

MARGIN = 4.0
F32_FLOOR = 6e-8            # half an ulp of a float32 near 1: the rounding of the float32 OUTPUT alone
BORDER = 1e-4


def _consts():
    from mfm_amd import _lib
    return _lib.AUTOCORR_LAG_BLOCK, _lib.AUTOCORR_TIME_BLOCK


def _cases():
    LB, TB = _consts()
    return {
        "n1": (1, 3, 1), "n2": (2, 1, 2),
        "partial_wave_L_eq_n": (37, 70, 37),
        "pow2_plus_1": (257, 130, 257),
        "n1000_L100": (1000, 261, 100), "n512_L512": (512, 200, 512),
        "lag_block_minus_1": (100, 70, LB - 1), "lag_block_plus_1": (100, 70, LB + 1),
        "time_block_minus_1": (TB - 1, 70, 40), "time_block_plus_1": (TB + 1, 70, 40),
    }


CASE_NAMES = ("n1", "n2", "partial_wave_L_eq_n", "pow2_plus_1", "n1000_L100", "n512_L512", "lag_block_minus_1", "lag_block_plus_1",
              "time_block_minus_1", "time_block_plus_1")

# measured on an MI355X (this file's own printout): case -> (max |rho - oracle|, max relative error of tau and of ess); bound = MARGIN x
MEASURED = {
    "n1": (0.0, 0.0), "n2": (0.0, 0.0),                             # exact (all NaN; rho = 1, -0.5): bounded by the float32 floor
    "partial_wave_L_eq_n": (2.17e-7, 2.05e-7),                      # -> 8.7e-7, 8.2e-7
    "pow2_plus_1": (5.94e-7, 5.40e-7),                              # -> 2.4e-6, 2.2e-6
    "n1000_L100": (3.56e-7, 2.39e-7),                               # -> 1.4e-6, 9.6e-7
    "n512_L512": (4.47e-7, 4.11e-7),                                # -> 1.8e-6, 1.6e-6
    "lag_block_minus_1": (5.16e-7, 3.40e-7), "lag_block_plus_1": (5.16e-7, 3.40e-7),      # -> 2.1e-6, 1.4e-6
    "time_block_minus_1": (6.33e-7, 6.30e-7),                       # -> 2.5e-6, 2.5e-6
    "time_block_plus_1": (9.10e-7, 6.56e-7),                        # -> 3.6e-6, 2.6e-6
    "index64": (1.16e-7, 3.99e-7),                                  # n = 33, first 64 / last 67 of 2^26 + 3 series -> 4.6e-7, 1.6e-6
}
# end to end on a 256-step MALA trajectory: (max relative error of tau / ess, max |autocorrelation - oracle rho / 2|); bound = MARGIN x
E2E_MEASURED = {"phi4": (1.04e-6, 7.85e-7), "4-mode": (1.05e-6, 5.88e-7)}


def _bound(measured):
    return MARGIN * max(measured, F32_FLOOR)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(x float32 [n, S], rho, tau, m_stop, Gamma) of a case; computed once and handed out read-only."""
    n, S, L = _cases()[name]
    x = ao.ar1(n, S, 0)
    r = ao.rho(x, L)
    tau, m_stop, G = ao.geyer(r)
    for a in (x, r, tau, m_stop, G):
        a.setflags(write=False)
    return x, r, tau, m_stop, G


@pytest.fixture(scope="module")
def ctx():
    from mfm_amd import _lib
    c = _lib.Context(dim=2, n_chain_local=16, fourier_dim=16, hidden_t=(16, 16), hidden_x=(16, 16), hidden_xt=(16, 16))
    yield c
    c.close()


def _run(ctx, x, L, want=("rho", "tau", "ess", "mean", "var")):
    import torch
    xd = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    S = xd.shape[1]
    out = {}
    if "rho" in want:
        out["rho"] = torch.full((L, S), -7.0, device="cuda")
    for k in ("tau", "ess"):
        if k in want:
            out[k] = torch.full((S,), -7.0, device="cuda")
    for k in ("mean", "var"):
        if k in want:
            out[k] = torch.full((S,), -7.0, device="cuda", dtype=torch.float64)
    ctx.autocorr(xd, n_lags=L, **out)
    ctx.sync()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_tau(tag, n, got_tau, got_ess, tau, m_stop, G, rtol, max_border=0.03):
    """tau / ess against the oracle with the borderline rule of the module docstring; returns the figures it printed."""
    S, M = tau.shape[0], G.shape[0]
    upto = np.arange(M)[:, None] <= m_stop[None, :]                      # Gamma_0 .. Gamma_mstop (the first non-positive one included)
    border = (np.abs(np.where(upto, G, 1.0)) < BORDER).any(axis=0) if M else np.zeros(S, bool)
    border &= ~np.isnan(tau)
    assert border.mean() <= max_border, f"{tag}: {border.mean():.3%} borderline series"
    ok = ~border
    with np.errstate(invalid="ignore", divide="ignore"):
        ess = n / tau
        rel_tau = np.abs(got_tau[ok].astype(np.float64) - tau[ok]) / np.abs(tau[ok])
        rel_ess = np.abs(got_ess[ok].astype(np.float64) - ess[ok]) / np.abs(ess[ok])
    finite = np.isfinite(rel_tau) & np.isfinite(rel_ess)
    worst = max(rel_tau[finite].max(initial=0.0), rel_ess[finite].max(initial=0.0))
    print(f"[autocorr] {tag}: max rel err tau/ess {worst:.3g} (bound {rtol:.3g}), borderline {border.sum()} of {S}")
    np.testing.assert_allclose(got_tau[ok], tau[ok], rtol=rtol, atol=0, equal_nan=True, err_msg=tag + " tau")
    np.testing.assert_allclose(got_ess[ok], ess[ok], rtol=rtol, atol=0, equal_nan=True, err_msg=tag + " ess")
    for s in np.nonzero(border)[0]:
        # the neighbouring stopping points: every borderline pair (stop there), and where the sum stops if that pair counts as positive
        cands = {int(m_stop[s])}
        for m in np.nonzero(np.abs(G[:m_stop[s] + 1, s]) < BORDER)[0]:
            later = np.nonzero(~(G[m + 1:, s] > 0))[0]
            cands |= {int(m), int(m + 1 + later[0]) if later.size else M}
        vals = np.array([-1.0 + 2.0 * G[:m, s].sum() for m in sorted(cands)])
        assert (np.abs(got_tau[s] - vals) <= rtol * np.abs(vals)).any(), (tag, s, got_tau[s], vals)
        assert (np.abs(got_ess[s] - n / vals) <= rtol * np.abs(n / vals)).any(), (tag, s, got_ess[s], n / vals)
    return worst


@pytest.mark.parametrize("name", CASE_NAMES)
def test_against_the_float64_oracle(ctx, name):
    n, S, L = _cases()[name]
    x, r, tau, m_stop, G = _oracle(name)
    got = _run(ctx, x, L)
    err = np.abs(got["rho"].astype(np.float64) - r)
    assert (np.isnan(got["rho"]) == np.isnan(r)).all()
    worst = np.nanmax(err, initial=0.0)
    bound_rho, bound_tau = _bound(MEASURED[name][0]), _bound(MEASURED[name][1])
    print(f"[autocorr] {name} {(n, S, L)}: max |rho - oracle| {worst:.3g} (bound {bound_rho:.3g})")
    assert worst < 1e-5                                             # above this the accumulation scheme is wrong, whatever was measured
    assert worst <= bound_rho
    if not np.isnan(r[0]).any():
        assert (got["rho"][0] == 1.0).all()                         # A_0 / A_0
    _check_tau(name, n, got["tau"], got["ess"], tau, m_stop, G, bound_tau)
    x64 = x.astype(np.float64)
    np.testing.assert_allclose(got["mean"], x64.mean(axis=0), rtol=1e-12, atol=0)
    np.testing.assert_allclose(got["var"], ((x64 - x64.mean(axis=0)) ** 2).sum(axis=0) / n, rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_tau_without_rho_is_bit_identical(ctx, name):
    n, S, L = _cases()[name]
    x = _oracle(name)[0]
    full = _run(ctx, x, L)
    only = _run(ctx, x, L, want=("tau", "ess"))
    np.testing.assert_array_equal(only["tau"].view(np.int32), full["tau"].view(np.int32))
    np.testing.assert_array_equal(only["ess"].view(np.int32), full["ess"].view(np.int32))
    one = _run(ctx, x, L, want=("tau",))                           # a single output is a valid request
    np.testing.assert_array_equal(one["tau"].view(np.int32), full["tau"].view(np.int32))


def _bits(d):
    return {k: v.view(np.int32 if v.dtype == np.float32 else np.int64) for k, v in d.items()}


@pytest.mark.parametrize("want_rho", [True, False])
def test_constant_series_is_nan_in_its_own_outputs_only(ctx, want_rho):
    n, S, L = 100, 70, 40
    x = ao.ar1(n, S, 0).copy()
    want = ("rho", "tau", "ess", "mean", "var") if want_rho else ("tau", "ess", "mean", "var")
    clean = _bits(_run(ctx, x, L, want))
    j = 37
    x[:, j] = 2.5
    got = _run(ctx, x, L, want)
    for k in ("rho", "tau", "ess") if want_rho else ("tau", "ess"):
        assert np.isnan(got[k][..., j]).all(), k
    assert got["mean"][j] == 2.5 and got["var"][j] == 0.0
    others = np.arange(S) != j
    for k, v in _bits(got).items():
        np.testing.assert_array_equal(v[..., others], clean[k][..., others], err_msg=k)


@pytest.mark.parametrize("want_rho", [True, False])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_input_spoils_its_own_series_only(ctx, want_rho, bad):
    n, S, L = 100, 70, 40
    x = ao.ar1(n, S, 0).copy()
    want = ("rho", "tau", "ess", "mean", "var") if want_rho else ("tau", "ess", "mean", "var")
    clean = _bits(_run(ctx, x, L, want))
    j = 64                                                          # first lane of the second wave
    x[51, j] = bad
    got = _run(ctx, x, L, want)
    for k in ("rho", "tau", "ess") if want_rho else ("tau", "ess"):
        assert np.isnan(got[k][..., j]).all(), k
    assert not np.isfinite(got["mean"][j]) and np.isnan(got["var"][j])
    others = np.arange(S) != j
    for k, v in _bits(got).items():
        np.testing.assert_array_equal(v[..., others], clean[k][..., others], err_msg=k)


def test_index_arithmetic_is_64_bit(ctx):
    """n S = 33 (2^26 + 3) = 2.2e9 elements: the offsets t S + s pass 2^31 from t = 32 on, and 2^32 bytes much earlier."""
    import torch
    n, S, L = 33, 2 ** 26 + 3, 4
    if torch.cuda.mem_get_info()[0] < 24e9:
        pytest.skip("needs 24 GB of free device memory")
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.empty((n, S), device="cuda")
    for t in range(n):
        x[t].normal_(generator=g)
    x += 3.0
    head, tail = x[:, :64].cpu().numpy(), x[:, -67:].cpu().numpy()
    out = {"rho": torch.empty((L, S), device="cuda"), "tau": torch.empty(S, device="cuda"), "ess": torch.empty(S, device="cuda"),
           "mean": torch.empty(S, device="cuda", dtype=torch.float64), "var": torch.empty(S, device="cuda", dtype=torch.float64)}
    ctx.autocorr(x, n_lags=L, **out)
    tau_only = torch.empty(S, device="cuda")
    ctx.autocorr(x, n_lags=L, tau=tau_only)
    ctx.sync()
    assert torch.equal(tau_only.view(torch.int32), out["tau"].view(torch.int32))
    bound = _bound(MEASURED["index64"][0])
    for part, sl in ((head, slice(0, 64)), (tail, slice(S - 67, S))):
        r = ao.rho(part, L)
        tau, m_stop, G = ao.geyer(r)
        err = np.abs(out["rho"][:, sl].cpu().numpy() - r).max()
        print(f"[autocorr] 64-bit {sl}: max |rho - oracle| {err:.3g} (bound {bound:.3g})")
        assert err <= bound
        _check_tau(f"64-bit {sl.start}", n, out["tau"][sl].cpu().numpy(), out["ess"][sl].cpu().numpy(), tau, m_stop, G,
                   _bound(MEASURED["index64"][1]))
        p64 = part.astype(np.float64)
        np.testing.assert_allclose(out["mean"][sl].cpu().numpy(), p64.mean(axis=0), rtol=1e-12)
        np.testing.assert_allclose(out["var"][sl].cpu().numpy(), p64.var(axis=0), rtol=1e-12)
    del x, out


def test_argument_errors_name_the_argument(ctx):
    import ctypes as C
    import torch
    from mfm_amd import _lib
    x = torch.zeros((8, 4), device="cuda")
    tau = torch.zeros(4, device="cuda")
    px, pt = C.c_void_p(x.data_ptr()), C.c_void_p(tau.data_ptr())
    f = ctx.lib.mfm_autocorr

    def err(*args):
        assert f(ctx.h, *args) == -1                                # MFM_EINVAL
        return ctx.lib.mfm_last_error().decode()

    assert "n must" in err(px, 0, 4, 1, None, pt, None, None, None)
    assert "n_series" in err(px, 8, 0, 1, None, pt, None, None, None)
    assert "n_lags" in err(px, 8, 4, 0, None, pt, None, None, None)
    assert "n_lags" in err(px, 8, 4, 9, None, pt, None, None, None)
    assert "d_x" in err(None, 8, 4, 1, None, pt, None, None, None)
    assert "output" in err(px, 8, 4, 1, None, None, None, None, None)
    assert f(ctx.h, px, 8, 4, 8, None, pt, None, None, None) == 0    # n_lags = n is the largest valid value
    ctx.sync()
    with pytest.raises(_lib.MfmError, match="n_lags"):
        ctx.autocorr(x, n_lags=9, tau=tau)
    with pytest.raises(_lib.MfmError, match="float32"):
        ctx.autocorr(x.double(), tau=tau)


def _engine(target):
    import torch
    from mfm_amd import distributions as D
    from mfm_amd.engine import Engine
    from tests import gpu_util as gu
    if target == "phi4":
        args, odist, k, model, state = gu.phi4_setup(d=16, B=64, hidden=32, F=16)
        dist = D.PhiFour(16)
    else:
        args, odist, k, model, state = gu.gmm4_setup(B=64)
        dist = D.GaussianMixture(odist.modes, odist.covs, odist.weights)
    args.ot_cond_flow = False
    eng = Engine(dist, args, model.f)
    return eng, dist, args, torch.as_tensor(odist.init_params.astype(np.float32)).cuda()


@pytest.mark.parametrize("target", ["phi4", "4-mode"])
def test_end_to_end_on_a_mala_run(target):
    """256 MALA steps in one launch, then the diagnostics on the trajectory where it lies."""
    from mfm_amd import mcmc_utils, random as jr
    from mfm_amd.bblackjax.mcmc.mala import mala
    eng, dist, args, pos = _engine(target)
    algo = mala(dist.logprob, args.step_size)
    _, info = algo.step.run(jr.PRNGKey(11), algo.init(pos), 256, thin=1)
    traj = info.positions
    n, B, d = traj.shape
    assert (n, B) == (256, 64)
    ess, tau = mcmc_utils.effective_sample_size(traj)
    assert ess.shape == tau.shape == (B, d) and ess.is_cuda
    host = traj.cpu().numpy().reshape(n, B * d)
    r = ao.rho(host, n)
    otau, m_stop, G = ao.geyer(r)
    _check_tau("e2e " + target, n, tau.cpu().numpy().reshape(-1), ess.cpu().numpy().reshape(-1), otau, m_stop, G, _bound(E2E_MEASURED[target][0]))
    ac = mcmc_utils.autocorrelation(traj)
    assert ac.shape == traj.shape and ac.is_cuda
    assert (ac[0] == 0.5).all()
    err = np.abs(ac.cpu().numpy().reshape(n, B * d) - r / 2).max()
    print(f"[autocorr] e2e {target}: max |autocorrelation - oracle rho / 2| {err:.3g} (bound {_bound(E2E_MEASURED[target][1]):.3g})")
    assert err <= _bound(E2E_MEASURED[target][1])
    last = mcmc_utils.autocorrelation(traj.permute(1, 2, 0), axis=-1)          # time axis last
    np.testing.assert_array_equal(last.cpu().numpy(), ac.permute(1, 2, 0).cpu().numpy())
    as_numpy = mcmc_utils.autocorrelation(traj[:, :2].cpu().numpy())           # numpy in, numpy out
    assert isinstance(as_numpy, np.ndarray)
    np.testing.assert_array_equal(as_numpy, ac[:, :2].cpu().numpy())
    ess32, tau32 = mcmc_utils.effective_sample_size(traj, max_lag=32)          # max_lag reaches the kernel
    t32, m32, G32 = ao.geyer(r[:32])
    _check_tau("e2e max_lag=32 " + target, n, tau32.cpu().numpy().reshape(-1), ess32.cpu().numpy().reshape(-1), t32, m32, G32,
               _bound(E2E_MEASURED[target][0]))
    eng.close()
