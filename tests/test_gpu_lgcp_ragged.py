"""GPU parity of every kernel that touches the log-Gaussian Cox process on grids whose cell count d = n x n is NOT a multiple of 16.

The Cox process is the one target whose gradient needs a dense contraction, K^-1 (x - mu); its kernels pad the lattice to
dp = ceil16(d) and rely on ``col < d`` guards and zero-filled packs (api.hip: mfm_set_target; lgcp.hip: mala_lgcp_kernel; ode.hip and
fm.hip: the gradient / H z tiles; wide.hip: lgcp_propose_kernel, lgcp_accept_kernel, the kinv(...) GEMMs, the target kernel; mala.hip:
loglik_kernel).  The bundled grids (4, 8, 16, 32, 40) all give dp == d, so none of those guards is ever false there.  Here the counts
come from binning tests/golden/finpines.csv (tests/gpu_util.py: lgcp_setup), on the smallest grids that reach each code path:

    n    d     dp    fused MALA instance   what it adds
    5    25    32    TPW 1                 d < 64; the last column tile has 9 live columns
    10   100   112   TPW 1                 7 column tiles, the last with 4 live columns
    18   324   336   TPW 4                 first run of this instance; 21 tiles over 8 waves
    20   400   400   TPW 4                 the same instance with dp == d (an instance bug, not a padding bug, shows here too)
    23   529   544   TPW 8                 34 tiles: waves 2-7 have a q whose tile lies beyond dp
    30   900   912   TPW 8                 near the fused kernel's limit
    33   1089  1104  none                  the d > 1024 fall-back to the wide propose / K^-1 GEMM / accept split, ragged

A wrong guard or pad gives a plausible result, not a crash: each spurious padded cell adds -beta a exp(0) = -beta / d to the
log-density and a row of garbage to the K^-1 product.  The planted check below hands the ORACLE exactly that error and requires the
device to miss it.  Tolerances are those of the aligned-grid tests named at each assertion.

Sensitivity, measured once on an MI355X with a library built for the purpose: with the ``col < d`` guard of mala_lgcp_kernel's GEMM
epilogue widened to ``col < dp`` (every access stays in bounds) the fused-kernel cases fail on all five ragged grids -- log-density off
by 0.126 / 0.054 / 0.017 / 0.013 / 0.006 at n = 5 / 10 / 18 / 23 / 30, beta = 0.45 -- while 20 x 20 and every other test pass."""
import functools

import numpy as np
import pytest

from oracle import fm, mala, ode, prng, targets

pytestmark = pytest.mark.gpu

# step sizes with which the float64 oracle ALONE (4 steps on the keys split(PRNGKey(KEY_BASE + n), 4)[j]) accepts 25 - 97 % of 32 chains in
# every step of every case below, beta = 0.45 and 1.0 alike, and leaves at most 2 of 32 decisions within 1e-2 of the uniform draw: both
# branches of the accept select are taken in every launch (_oracle_alone asserts it)
STEP = {5: 0.01, 10: 0.02, 18: 0.03, 20: 0.03, 23: 0.04, 30: 0.04, 33: 0.04}
N_STEPS = 4
KEY_BASE = 61


def _dev(x, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def _keys_dev(keys):
    return _dev(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32))


def _relerr(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def _ceil16(d):
    return (d + 15) // 16 * 16


@functools.lru_cache(maxsize=None)
def _setup(n, B, hidden=32, F=16, hutch=True):
    """(args, dist, key, model, state) of tests/gpu_util.py: lgcp_setup, computed once per shape and left unchanged."""
    from tests import gpu_util as gu
    return gu.lgcp_setup(n=n, B=B, hidden=hidden, F=F, hutch=hutch)


def _family(fam):
    from mfm_amd import _lib
    return {"tile": _lib.FAMILY_TILE, "wide": _lib.FAMILY_WIDE, None: None}[fam]


def _make_ctx(dist, args, fam, **kw):
    """A context of the named kernel family.  The tile family may decline a shape with a named MFM_ETOOLARGE: correct behaviour --
    the message is checked and the case runs on the wide family."""
    from mfm_amd import _lib
    from tests import gpu_util as gu
    try:
        return gu.make_ctx(dist, args, family=_family(fam), **kw)
    except _lib.MfmError as e:
        if fam != "tile":
            raise
        assert "does not fit" in str(e), str(e)
        print(f"tile family declined d = {args.dim}: {e}; running on the wide family")
        return gu.make_ctx(dist, args, family=_lib.FAMILY_WIDE, **kw)


def _planted_miss(tag, device, oracle, shift, rtol, atol):
    """The planted padding error: the oracle with one extra zero-count cell per padded column (log-density - shift).  Returns the
    factor by which the device misses it, in units of the comparison's tolerance, over the chains (minimum); asserts >= 10 wherever
    the shift itself is >= 11 tolerances (the device lies within one tolerance of the true oracle, asserted by the caller)."""
    planted = oracle - shift
    tol = atol + rtol * np.abs(planted)
    factor = (np.abs(device - planted) / tol).min()
    can_show = shift >= 11 * tol.max()
    print(f"{tag}: planted padding shift {shift:.4f} = {shift / tol.max():.1f} tolerances; device misses it by {factor:.1f} tolerances, "
          f"and the true oracle by {(np.abs(device - oracle) / (atol + rtol * np.abs(oracle))).max():.3f}")
    # measured miss factors (MI355X; init at atol 1e-3 / after a step at atol 2e-3; beta = 0.45 | beta = 1.0), fused kernel, 32 chains:
    #    5 x 5    95.7 / 54.1  | 154.9 / 100.7        10 x 10   50.3 / 26.2 |  79.1 / 46.9       18 x 18   8.8 / 5.8 | 23.9 / 14.9
    #   23 x 23    4.9 /  3.6  |  12.5 /   8.8        30 x 30    1.6 /  1.3 |   4.0 /  3.1       33 x 33   1.4 / 1.2 |  3.5 /  2.8 (wide split)
    # wide split, 128 chains: 10 x 10  48.2 / 25.9 | 78.5 / 47.0;  18 x 18  8.8 / 5.8 | 24.1 / 14.8;  33 x 33  1.4 / 1.2 | 3.4 / 2.8
    # mfm_loglik (shift (dp - d) / d, atol 1e-3): 5 x 5  148.0;  10 x 10  65.4;  30 x 30  7.5;  33 x 33  7.6
    # The grids from 18 x 18 (beta = 0.45) and 23 x 23 on CANNOT show 10 x: the shift beta (dp - d) / d falls with d while the bound
    # 1e-3 + 2e-6 |logp| grows with it (|logp| up to 1670), so the shift itself is only 1.2 - 9 tolerances there.  The tolerance stays
    # as it is; what separates the device from the planted error on those grids is the measured agreement with the true oracle,
    # <= 0.05 tolerances on every grid (printed above).
    if can_show:
        assert factor >= 10, (tag, factor)
    return factor


def _step_keys(n, B, j, per_chain):
    """(the key mfm_mala_step takes, the chains' keys): chain b of a launch on ``key`` draws from split(key, B)[b]; with per-chain keys
    (mfm_mala_step_keys) the caller's own array."""
    kj = prng.split(prng.PRNGKey(KEY_BASE + n), N_STEPS)[j]
    return kj, (prng.split(prng.PRNGKey(1000 + j), B) if per_chain else prng.split(kj, B))


@functools.lru_cache(maxsize=None)
def _oracle_alone(n, B, beta, per_chain=False):
    """The float64 oracle on its own trajectory: both decisions occur in every step, at most 2 of 32 chains per step are borderline."""
    args, dist, k, model, state = _setup(n, B)
    vg = targets.Tempered(dist, beta).value_and_grad
    st = mala.init(dist.init_params.astype(np.float32).astype(np.float64), vg)
    for j in range(N_STEPS):
        st, info, u = mala.kernel(_step_keys(n, B, j, per_chain)[1], st, vg, STEP[n])
        assert 0 < info.is_accepted.sum() < B, (n, B, beta, j, info.is_accepted.sum())
        assert (np.abs(u - info.acceptance_rate) <= 1e-2).sum() <= 2 * B // 32, (n, B, beta, j)
    return True


def _mala_case(n, B, fam, betas=(0.45, 1.0), per_chain=False):
    """Init and four steps against the oracle: structure and tolerances of tests/test_gpu_mala.py: test_mala_init_and_step_match_oracle
    (the oracle is restarted from the kernel's float32 state before every step)."""
    import torch
    args, dist, k, model, state = _setup(n, B)
    d, dp, eps = n * n, _ceil16(n * n), STEP[n]
    ctx = _make_ctx(dist, args, fam)
    x32 = dist.init_params.astype(np.float32)
    for beta in betas:
        vg = targets.Tempered(dist, beta).value_and_grad
        st = mala.init(x32.astype(np.float64), vg)
        pos, logp, grad = _dev(x32), torch.empty(B, dtype=torch.float64, device="cuda"), torch.empty(B, d, device="cuda")
        ctx.mala_init(pos, beta, logp, grad)
        lp0, g0 = logp.cpu().numpy(), grad.cpu().numpy()
        print(f"n={n} B={B} {fam or 'auto'} beta={beta}: init |dlogp| {np.abs(lp0 - st.logdensity).max():.2e} (|logp| {np.abs(st.logdensity).max():.0f}), "
              f"|dgrad| {np.abs(g0 - st.logdensity_grad).max():.2e} (|grad| {np.abs(st.logdensity_grad).max():.1f})")
        np.testing.assert_allclose(lp0, st.logdensity, rtol=2e-6, atol=1e-3)          # measured <= 1.6e-4 (30 x 30, |logp| 1383): 0.05 tolerances
        np.testing.assert_allclose(g0, st.logdensity_grad, rtol=2e-5, atol=2e-3)      # measured <= 6.6e-6 (|grad| 8 - 91)
        if dp != d:
            # one extra zero-count cell per padded column: -beta a exp(0) each, and a gradient term on no real cell
            _planted_miss(f"n={n} B={B} {fam or 'auto'} beta={beta} init", lp0, st.logdensity, beta * (dp - d) / d, 2e-6, 1e-3)
        assert _oracle_alone(n, B, beta, per_chain)
        n_border = n_acc = 0
        for j in range(N_STEPS):
            kj, keys = _step_keys(n, B, j, per_chain)
            st_in = mala.MALAState(pos.cpu().numpy().astype(np.float64), logp.cpu().numpy(), grad.cpu().numpy().astype(np.float64))
            new, info, u = mala.kernel(keys, st_in, vg, eps)
            acc = torch.empty(B, device="cuda"); isacc = torch.empty(B, dtype=torch.uint8, device="cuda")
            prop = torch.empty(B, d, device="cuda"); w = torch.empty(B, device="cuda")
            if per_chain:
                ctx.mala_step_keys(_keys_dev(keys), beta, eps, pos, logp, grad, acc, isacc, prop, w)
            else:
                ctx.mala_step(kj, beta, eps, pos, logp, grad, acc, isacc, prop, w)
            ia = isacc.cpu().numpy().astype(bool)
            decided = np.abs(u - info.acceptance_rate) > 1e-2          # decisions may only differ on a knife edge
            same = ia == info.is_accepted
            print(f"   step {j}: oracle accepts {info.is_accepted.sum()}/{B}, borderline {(~decided).sum()}, |dprop| {np.abs(prop.cpu().numpy() - info.proposed_position).max():.2e}, "
                  f"|dp| {np.abs(acc.cpu().numpy() - info.acceptance_rate).max():.2e}, |dlogp| {np.abs(logp.cpu().numpy() - new.logdensity)[same].max():.2e}, "
                  f"|dgrad| {np.abs(grad.cpu().numpy() - new.logdensity_grad)[same].max():.2e}")
            n_border += int((~decided).sum()); n_acc += int(info.is_accepted.sum())
            np.testing.assert_allclose(prop.cpu().numpy(), info.proposed_position, rtol=1e-6, atol=1e-6)      # measured <= 4.8e-7
            np.testing.assert_allclose(acc.cpu().numpy(), info.acceptance_rate, rtol=5e-3, atol=5e-3)         # measured <= 1.4e-4
            np.testing.assert_array_equal(ia[decided], info.is_accepted[decided])
            np.testing.assert_allclose(pos.cpu().numpy()[same], new.position[same], rtol=1e-6, atol=1e-6)
            np.testing.assert_allclose(logp.cpu().numpy()[same], new.logdensity[same], rtol=2e-6, atol=2e-3)  # measured <= 1.5e-4
            np.testing.assert_allclose(grad.cpu().numpy()[same], new.logdensity_grad[same], rtol=3e-5, atol=3e-3)   # measured <= 7.0e-6
            if dp != d and info.is_accepted.any():
                a = same & info.is_accepted
                _planted_miss(f"   step {j}", logp.cpu().numpy()[a], new.logdensity[a], beta * (dp - d) / d, 2e-6, 2e-3)
        assert n_border <= 0.1 * B * N_STEPS, n_border                 # the borderline exclusion: at most 10 % of the chain-steps
        assert 0 < n_acc < B * N_STEPS                                 # both decisions were compared
    ctx.close()


@pytest.mark.parametrize("n", [5, 10, 18, 20, 23, 30, 33])
def test_mala_init_and_steps_match_oracle_on_the_fused_kernel(n):
    """32 chains: every grid up to 30 x 30 takes mala_lgcp_kernel<TPW> (api.hip: lgcp_mala_dispatch, fewer than 128 chains); 33 x 33
    (dp = 1104 > 1024) is declined by launch_mala_lgcp and falls through to the wide split."""
    _mala_case(n, 32, None)


@pytest.mark.parametrize("n", [10, 18, 33])
def test_mala_init_and_steps_match_oracle_on_the_wide_split(n):
    """128 chains in a wide-family context: propose -> wide K^-1 GEMM -> accept (wide.hip: mala_lgcp)."""
    _mala_case(n, 128, "wide")


def test_mala_steps_with_per_chain_keys_match_oracle():
    """mfm_mala_step_keys on the 10 x 10 grid: every chain draws from its own key."""
    _mala_case(10, 32, None, betas=(0.45,), per_chain=True)


@pytest.mark.parametrize("n", [5, 10, 30, 33])
def test_loglik_matches_oracle(n):
    """mfm_loglik (mala.hip: loglik_kernel) against dist.loglik at the tolerance of tests/test_gpu_mala.py."""
    import torch
    B = 32
    args, dist, k, model, state = _setup(n, B)
    d, dp = n * n, _ceil16(n * n)
    ctx = _make_ctx(dist, args, None)
    x32 = dist.init_params.astype(np.float32)
    ll = torch.empty(B, dtype=torch.float64, device="cuda")
    ctx.loglik(_dev(x32), ll)
    ref = dist.loglik(x32.astype(np.float64))
    print(f"loglik n={n}: |dll| {np.abs(ll.cpu().numpy() - ref).max():.2e} (|ll| {np.abs(ref).max():.1f})")
    np.testing.assert_allclose(ll.cpu().numpy(), ref, rtol=2e-6, atol=1e-3)            # measured <= 8.2e-6 (|ll| 390 - 450)
    _planted_miss(f"loglik n={n}", ll.cpu().numpy(), ref, (dp - d) / d, 2e-6, 1e-3)
    ctx.close()


@pytest.mark.parametrize("n,B,fam", [(10, 48, None), (18, 128, "wide")])
def test_mala_run_is_bit_identical_with_single_step_launches(n, B, fam):
    """mfm_mala_run on the Cox process (a loop of the step inside the library): the fused tile at 10 x 10, the wide split with 128 chains
    at 18 x 18 -- step-major and chain-major keys, the comparison of tests/test_gpu_mala_run.py."""
    import torch
    from tests.test_gpu_mala_run import _assert_run_equals_steps, _init, _run, _stepwise
    args, dist, k, model, state = _setup(n, B)
    ctx = _make_ctx(dist, args, fam)
    pos0 = torch.as_tensor(dist.init_params.astype(np.float32)).cuda()
    beta, eps = 1.0, STEP[n]              # (oracle alone: mean acceptance probability 0.5 at 10 x 10, 0.65 at 18 x 18)
    state0 = _init(ctx, pos0, beta)
    for key in (prng.PRNGKey(3), prng.split(prng.PRNGKey(4), B)):            # step-major, chain-major
        steps = _stepwise(ctx, state0, key, beta, eps, N_STEPS)
        run = _run(ctx, state0, key, beta, eps, N_STEPS, 1)
        _assert_run_equals_steps(run, steps)
    ctx.close()


# ---- flow matching: loss, gradient, eval loss, vector field and JVP (tolerances of tests/test_gpu_fm.py) ------------------------------
@pytest.mark.parametrize("fam,n", [("tile", 5), ("tile", 10), ("wide", 10), ("wide", 18)])
def test_fm_loss_grad_field_and_jvp_match_oracle(fam, n):
    import torch
    from tests import gpu_util as gu
    B, d = 32, n * n
    args, dist, k, model, state = _setup(n, B)
    params = gu.rand_params(model, seed=3)
    ctx = _make_ctx(dist, args, fam, fourier=model.f, params=params, max_eval=B)
    x32 = dist.init_params.astype(np.float32)
    key = prng.PRNGKey(11)
    loss_o, grads_o = fm.loss_and_grad(model, params, key, x32.astype(np.float64), args.sigma)
    loss = torch.zeros(1, dtype=torch.float64, device="cuda"); grads = torch.full((ctx.n_params,), float("nan"), device="cuda")
    ctx.fm_loss_grad(key, _dev(x32), loss, grads)
    g = gu.unflat_params(model, grads.cpu().numpy())
    worst = max(_relerr(gg[kk], go[kk].astype(np.float64)) for gg, go in zip(g, grads_o) for kk in ("kernel", "bias"))
    l2 = torch.zeros(1, dtype=torch.float64, device="cuda")
    ctx.fm_loss(key, _dev(x32), l2)
    print(f"fm {fam} n={n}: loss rel {abs(loss.item() - loss_o) / abs(loss_o):.2e}, eval loss rel {abs(l2.item() - loss_o) / abs(loss_o):.2e}, worst gradient tensor {worst:.2e}")
    assert abs(loss.item() - loss_o) <= 2e-5 * abs(loss_o), (loss.item(), loss_o)      # measured <= 8.3e-10 (loss and eval loss)
    for i, (gg, go) in enumerate(zip(g, grads_o)):
        for kk in ("kernel", "bias"):
            assert np.isfinite(gg[kk]).all()                      # every element of the gradient vector is written
            assert _relerr(gg[kk], go[kk].astype(np.float64)) < 2e-4, (i, kk, _relerr(gg[kk], go[kk]))      # measured <= 3.2e-7
    assert abs(l2.item() - loss_o) <= 2e-5 * abs(loss_o)
    if n == 10:
        # an eval set that is not a multiple of 16: 23 samples, the last 7 through the staged 16-row tile
        ne = 23
        lo, _ = fm.loss_and_grad(model, params, key, x32[:ne].astype(np.float64), args.sigma, n_total=ne, start=0, need_grad=False)
        l3 = torch.zeros(1, dtype=torch.float64, device="cuda")
        ctx.fm_loss(key, _dev(x32[:ne]), l3, n_total=ne, offset=0)
        print(f"   eval loss on {ne} samples: rel {abs(l3.item() - lo) / abs(lo):.2e}")
        assert abs(l3.item() - lo) <= 2e-5 * abs(lo), (l3.item(), lo)                  # measured 1.3e-9 (tile), 7.6e-10 (wide)
    # vector field and JVP
    params = gu.rand_params(model, seed=6)
    ctx.set_params(gu.flat_params(params))
    rng = np.random.default_rng(1)
    t = rng.uniform(0, 1, B).astype(np.float32)
    z = rng.standard_normal((B, d)).astype(np.float32)
    v_o, jv_o = model.forward(params, x32.astype(np.float64), t.astype(np.float64), tangent=z.astype(np.float64))
    v = torch.empty(B, d, device="cuda"); jv = torch.empty(B, d, device="cuda")
    ctx.vf_apply(_dev(x32), _dev(t), v, _dev(z), jv)
    v2 = torch.empty(B, d, device="cuda")
    ctx.vf_apply(_dev(x32), _dev(t), v2)
    print(f"   field rel {_relerr(v.cpu().numpy(), v_o):.2e}, JVP rel {_relerr(jv.cpu().numpy(), jv_o):.2e}, field alone rel {_relerr(v2.cpu().numpy(), v_o):.2e}")
    assert _relerr(v.cpu().numpy(), v_o) < 2e-5                      # measured <= 5.2e-7
    assert _relerr(jv.cpu().numpy(), jv_o) < 2e-5                    # measured <= 3.1e-7
    assert _relerr(v2.cpu().numpy(), v_o) < 2e-5
    ctx.close()


# ---- CNF transform and flow-MH step on prescribed step sequences -------------------------------------------------------------------
def _tamed(model, out_scale):
    """The gentler field of the existing Cox cases at d = 64 (tests/test_gpu_replay.py, tests/test_gpu_wide.py): output scale 0.3, gate
    scale 0.05.  (Below d = 128 the gradient clip is off: a larger output layer sends exp(x) to infinity in the float64 oracle.)"""
    from tests import gpu_util as gu
    p = gu.rand_params(model, seed=9, out_scale=out_scale)
    p[4]["kernel"] *= 0.05; p[4]["bias"] *= 0.05
    return p


@pytest.mark.parametrize("fam,n,hutch", [("tile", 5, True), ("tile", 10, True), ("wide", 10, True), ("tile", 5, False), ("wide", 10, False)])
@pytest.mark.parametrize("direction", [1, -1])
def test_transform_on_prescribed_steps_matches_oracle(fam, n, hutch, direction):
    """Both sides integrate on the oracle's float32-rounded step sequence (tests/test_gpu_replay.py): attempt counts exact, outputs at
    float32 rounding, the log-det at the tolerances of test_transform_on_prescribed_steps_matches_oracle (Hutchinson) and
    tests/test_gpu_wide.py: test_wide_exact_trace_transform_on_prescribed_steps (exact trace)."""
    import torch
    from tests.test_gpu_replay import _check_controller_tight, _replay_arrays
    B, d = 32, n * n
    args, dist, k, model, state = _setup(n, B, hutch=hutch)
    params = _tamed(model, 0.3)
    ctx = _make_ctx(dist, args, fam, fourier=model.f, params=params)
    x64 = dist.init_params.astype(np.float32).astype(np.float64)
    keys = prng.split(prng.PRNGKey(21), B)
    fn = ode.transform_and_logdet if direction > 0 else ode.inverse_and_logdet
    o = (hutch, args.rtol, args.atol, args.mxstep)
    st = {}
    fn(model, params, keys, x64, *o, stats=st)                       # the oracle's own controller: records the step sequence
    dt, acc = _replay_arrays([st])
    st_o = {}
    y_o, l_o = fn(model, params, keys, x64, *o, stats=st_o, replay=dict(dt=dt[0].astype(np.float64), acc=acc[0]))
    np.testing.assert_array_equal(st_o["n_attempted"], st["n_attempted"])
    assert st["n_attempted"].mean() > 5, st["n_attempted"].mean()     # a non-trivial integration (oracle: 11 - 13 attempts with Hutchinson, 6 - 9 exact)
    ratio = torch.zeros(dt[0].shape, device="cuda"); own = torch.zeros(dt[0].shape, device="cuda")
    ctx.debug_replay(_dev(dt[0]), _dev(acc[0]), ratio, own)
    out = torch.empty(B, d, device="cuda"); ldj = torch.empty(B, device="cuda"); ns = torch.empty(B, dtype=torch.int32, device="cuda")
    ctx.ode_transform(direction, _dev(x64.astype(np.float32)), out, ldj, keys=_keys_dev(keys), nsteps=ns)
    y, l, nn = out.cpu().numpy(), ldj.cpu().numpy(), ns.cpu().numpy()
    np.testing.assert_array_equal(nn, st["n_attempted"])             # same step sequence => same attempt count, exactly
    assert np.abs(y_o - x64).max() > 0.3                             # the flow moves the points
    assert np.abs(l_o).max() > 0.05                                  # a log-det worth comparing
    ey, el, ls = np.abs(y - y_o).max(1), np.abs(l - l_o), max(1.0, np.abs(l_o).max())
    mr, md = _check_controller_tight(f"lgcp n={n} dir={direction}", st_o, ratio.cpu().numpy(), own.cpu().numpy(), nn)
    print(f"replay transform lgcp n={n} {fam} {'hutch' if hutch else 'exact'} dir={direction}: attempts {nn.mean():.0f}, |dy| {ey.max():.2e} (|y| {np.abs(y_o).max():.1f}), "
          f"|dl| q90 {np.quantile(el, 0.9):.2e} max {el.max():.2e} (|l| {ls:.2f}), controller medians {mr:.1e} {md:.1e}")
    assert ey.max() < 3e-5 * max(1.0, np.abs(y_o).max()), ey.max()   # measured <= 2.1e-5 against a bound of 2.6e-4 (|y| 8.7)
    # measured log-det errors: Hutchinson q90 <= 4.7e-7, max <= 1.5e-6 (|l| 1.3 - 2.3); exact trace max <= 1.7e-6 (|l| 1.0)
    if hutch:
        assert np.quantile(el, 0.9) < 2e-5 * ls and el.max() < 2e-3 * ls, (np.quantile(el, 0.9), el.max(), ls)
        assert abs((l - l_o).mean()) < 1e-4 * ls                     # no systematic log-det bias
    else:
        assert np.quantile(el, 0.9) < 1e-4 * ls and el.max() < 1e-4 * ls, (np.quantile(el, 0.9), el.max(), ls)
    ctx.close()


@pytest.mark.parametrize("fam", ["tile", "wide"])
def test_flow_step_on_prescribed_steps_matches_oracle(fam):
    """One random-walk flow-MH step on the 10 x 10 grid, both solves on the oracle's step sequences: the Cox case of
    tests/test_gpu_replay.py: test_flow_step_on_prescribed_steps_other_targets_and_activations, same parameters and bounds."""
    from tests import gpu_util as gu
    from tests.test_gpu_replay import _flow_replay_raw, _tamed as _tamed_replay
    B, n = 32, 10
    args, dist, k, model, state = _setup(n, B)
    params = _tamed_replay(model, out_scale=0.3, gate=0.05)
    ctx = _make_ctx(dist, args, fam, fourier=model.f, params=params)
    r = _flow_replay_raw(ctx, model, params, args, dist, 0.8, dist.init_params.astype(np.float32), prng.PRNGKey(41))
    so, dg, info_o = r["so"], r["diag"], r["info_o"]
    np.testing.assert_array_equal(r["n_g"], r["n_o"])                 # attempt counts of both solves: exact
    assert r["n_o"].mean() > 15
    e_p = np.abs(r["prop"] - info_o.proposed_position).max()
    vs = max(1.0, np.abs(so["vol0"]).max(), np.abs(so["volp"]).max())
    e_v0, e_vp, e_la = np.abs(dg[:, 0] - so["vol0"]), np.abs(dg[:, 1] - so["volp"]), np.abs(dg[:, 3] - so["log_alpha"])
    print(f"replay flow step lgcp n={n} {fam}: attempts {r['n_o'].mean():.0f}, |dx'| {e_p:.2e}, |dvol0| {e_v0.max():.2e}, |dvolp| {e_vp.max():.2e} (scale {vs:.1f}), "
          f"|d log alpha| med {np.median(e_la):.2e} max {e_la.max():.2e}")
    # measured (tile / wide): |dx'| 2.2e-5 / 1.8e-5, log-dets 3.4e-6 / 2.6e-6 of scale 2.9, |d log alpha| max 3.2e-4 / 3.3e-4
    assert e_p < 3e-5 * max(1.0, np.abs(info_o.proposed_position).max())
    for e in (e_v0, e_vp):
        assert np.quantile(e, 0.9) < 2e-5 * vs and e.max() < 2e-3 * vs, (np.quantile(e, 0.9), e.max(), vs)
    vg = targets.Tempered(dist, 0.8).value_and_grad
    gn = vg(info_o.proposed_position.astype(np.float64))[1]
    bound = 2.0 * np.linalg.norm(gn, axis=1) * np.linalg.norm(r["prop"] - info_o.proposed_position, axis=1) + 1e-4 * vs + 1e-3
    assert (e_la <= bound).all(), (e_la / bound).max()
    same = r["isacc"] == info_o.is_accepted
    assert same.mean() > 0.9
    ctx.close()


def test_pines_loop_on_a_ragged_grid_matches_oracle():
    """The whole loop on the 10 x 10 grid (counts binned from the fixture by the product's class), asserted as
    tests/test_gpu_loop.py: test_pines_loop_matches_oracle asserts the 16 x 16 loop."""
    from tests import gpu_util as gu
    from tests.test_gpu_loop import _run_both
    out, res, ex = _run_both("pines", 100, 32, 8, 3, step_size=0.01, file_path=gu.PINES_CSV)
    tr, m = out["trace"], ex["metrics"]
    g = ex["states"].position.cpu().numpy().astype(np.float64)
    print(f"ragged pines loop: loss rel {np.abs(m[:, 0] / np.array(tr['loss']) - 1).max():.2e} (first three {np.abs(m[:3, 0] / np.array(tr['loss'][:3]) - 1).max():.2e}), "
          f"beta rel {np.abs(np.array(ex['betas']) / np.array(tr['beta']) - 1).max():.2e}, |d mean position| {np.abs(g.mean(0) - out['states'].position.mean(0)).max():.2e}")
    np.testing.assert_allclose(m[:3, 0], tr["loss"][:3], rtol=1e-5)                    # measured 1.8e-9
    np.testing.assert_allclose(m[:, 0], tr["loss"], rtol=5e-3)                         # measured 1.8e-4
    np.testing.assert_allclose(ex["betas"], tr["beta"], rtol=2e-3)                     # measured 4.8e-4
    np.testing.assert_allclose(g.mean(0), out["states"].position.mean(0), atol=2e-2)   # measured 5.2e-3
    np.testing.assert_allclose(ex["states"].logdensity.cpu().numpy().mean(), out["states"].logdensity.mean(), rtol=2e-3)
    assert np.isfinite(res[0])
    ex["engine"].close()
