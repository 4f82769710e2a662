"""libmfm_ref (oracle/cref/mfm_ref.c: the C / OpenMP float64 restatement of the headline configuration's inner loop) against the numpy
restatement, function by function on the same inputs.  CPU only.  Both are oracles (test infrastructure, PARITY UNPINNED): this
file says they state the same arithmetic -- values to rounding (the summation orders differ: BLAS / pairwise sums vs plain loops),
attempted-step counts of the adaptive solves equal."""
import numpy as np
import pytest

from oracle import cref, flow, fm, loop, mala, metrics, ode, prng, targets
from tests import gpu_util as gu


def _setup(d, B, hidden=32, F=16, seed=3):
    args, dist, k, model, state = gu.phi4_setup(d=d, B=B, hidden=hidden, F=F, seed=seed)
    params = gu.rand_params(model, seed=seed, out_scale=0.05)
    return args, dist, model, params, cref.CRef(model, params)


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def test_library_builds_and_reports_its_threads():
    assert cref.build().endswith("libmfm_ref.so")
    assert cref.lib().mfmref_threads() >= 1


@pytest.mark.parametrize("d", [64, 160])
def test_target_and_mala_step_equal_the_numpy_restatement(d):
    args, dist, model, params, cr = _setup(d, 24)
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, (24, d))
    for temper in (1.0, 0.37):
        vg = targets.Tempered(dist, temper).value_and_grad
        lp, g = vg(x)
        lpc, gc = cr.value_and_grad(x, temper)
        assert _rel(lpc, lp) < 1e-13 and _rel(gc, g) < 1e-13
        keys = prng.split(prng.PRNGKey(5), 24)
        noise = rng.standard_normal((24, d))
        seen = set()
        for step in (1e-4, 2e-5, 1e-5):     # far from equilibrium the rule as written (min(1, 1 / alpha)) rejects at 1e-4 and accepts at 1e-5
            for textbook in (False, True):
                st, info, u = mala.kernel(keys, mala.MALAState(x, lp, g), vg, step, textbook=textbook, noise=noise)
                stc, p, acc = cr.mala_step(mala.MALAState(x, lp, g), noise, u, step, temper, textbook=textbook)
                assert (acc == info.is_accepted).all()
                seen |= set(acc.tolist())
                assert np.abs(p - info.acceptance_rate).max() < 1e-9           # |log p| ~ 1e4 * 1e-13
                assert _rel(stc.position, st.position) < 1e-14 and _rel(stc.logdensity, st.logdensity) < 1e-13 and _rel(stc.logdensity_grad, st.logdensity_grad) < 1e-13
        assert seen == {True, False}


@pytest.mark.parametrize("d", [64, 160])          # 160 > 128: the clipped gate term (exe_flow_matching.py:88-89)
def test_vector_field_forward_and_jvp_equal_the_numpy_restatement(d):
    args, dist, model, params, cr = _setup(d, 16)
    assert (model.grad_clip is not None) == (d > 128)
    rng = np.random.default_rng(1)
    x, t, z = rng.uniform(-1, 1, (16, d)), rng.uniform(0, 1, 16), rng.standard_normal((16, d))
    v, jv = model.forward(params, x, t, tangent=z)
    vc, jvc = cr.forward(x, t, tangent=z)
    assert _rel(vc, v) < 1e-12 and _rel(jvc, jv) < 1e-12
    assert _rel(cr.forward(x, t), v) < 1e-12
    if d > 128:
        g = dist.grad_logprob(x)
        assert (np.abs(g) > 1.0).any() and (np.abs(g) <= 1.0).any()      # both sides of the clip are exercised


def test_flow_matching_loss_and_gradient_equal_the_numpy_restatement():
    args, dist, model, params, cr = _setup(160, 40)
    x1 = np.random.default_rng(2).uniform(-1, 1, (40, 160))
    key = prng.PRNGKey(11)
    loss, grads = fm.loss_and_grad(model, params, key, x1, args.sigma)
    t, cond, target = fm.cond_flow_batch(key, x1, args.sigma)
    lc, gc = cr.fm_loss_grad(t, cond, target)
    assert abs(lc - loss) < 1e-11 * abs(loss)
    for a, b in zip(gc, grads):
        for nm in ("kernel", "bias"):
            assert a[nm].dtype == np.float32 and a[nm].shape == b[nm].shape
            assert np.abs(a[nm].astype(np.float64) - b[nm]).max() <= 2e-7 * max(np.abs(b[nm]).max(), 1e-30), nm      # both round a float64 sum to float32


@pytest.mark.parametrize("sign", [+1, -1])
@pytest.mark.parametrize("strength", ["mild", "stiff"])
def test_adaptive_cnf_solve_equals_the_numpy_restatement(sign, strength):
    args, dist, model, params, cr = _setup(64, 12, hidden=32, F=16)
    # a field strong enough for the controller to work (rejections among the attempted steps); the gate layer is scaled down: unclipped
    # at d <= 128, grad log pi of a lattice far from equilibrium is O(1e3) and the field would blow up
    sc, osc = (1.0, 0.3) if strength == "mild" else (1.5, 1.0)
    params = gu.rand_params(model, seed=4, scale=sc, out_scale=osc)
    gl = model.zero_layers()[0]
    params[gl]["kernel"] *= np.float32(1e-3 / osc); params[gl]["bias"] *= np.float32(1e-3)
    cr.set_params(params)
    rng = np.random.default_rng(3)
    x0, z = rng.uniform(-1, 1, (12, 64)), rng.standard_normal((12, 64))
    st = {}
    f = ode.transform_and_logdet if sign > 0 else ode.inverse_and_logdet
    xo, ldj = f(model, params, None, x0, True, 1e-5, 1e-5, 1000, z=z, stats=st)
    sc_ = {}
    xc, lc = cr.solve(x0, z, sign, 1e-5, 1e-5, 1000, stats=sc_)
    n = st["n_attempted"]
    rejected = sum(int((~st["acc_seq"][b, :n[b]]).sum()) for b in range(12))
    assert n.min() >= 15 and rejected >= 12 and (n.max() >= 100) == (strength == "stiff")
    assert (sc_["n_attempted"] == n).all(), (sc_["n_attempted"], n)
    assert sc_["n_evals_total"] == int((2 + 6 * n).sum())
    # measured: 6e-12 / 5e-11 (mild, ~22 attempted steps), 6e-8 / 1.5e-6 (stiff, up to 130: every relu kink a step crosses amplifies
    # the rounding difference of the two summation orders)
    tol = 1e-9 if strength == "mild" else 1e-4
    assert np.abs(xc - xo).max() < tol and np.abs(lc - ldj).max() < tol * max(1.0, np.abs(ldj).max())


def test_keyed_mala_kernel_and_flow_mh_step_equal_the_numpy_restatement():
    """The two composed steps the CPU baseline of bench.py times (keys -> draws by oracle/prng.py, arithmetic in C)."""
    args, dist, model, params, cr = _setup(64, 12, hidden=32, F=16)
    params = gu.rand_params(model, seed=4, scale=1.0, out_scale=0.3)
    gl = model.zero_layers()[0]
    params[gl]["kernel"] *= np.float32(1e-3 / 0.3); params[gl]["bias"] *= np.float32(1e-3)
    cr.set_params(params)
    vg = targets.Tempered(dist, 1.0).value_and_grad
    x = np.random.default_rng(5).uniform(-1, 1, (12, 64))
    st0 = mala.init(x, vg)
    keys = prng.split(prng.PRNGKey(9), 12)
    a, ia, _ = mala.kernel(keys, st0, vg, 1e-5)
    b, ib = cr.mala_kernel(keys, st0, 1e-5)
    assert (ib.is_accepted == ia.is_accepted).all() and _rel(b.position, a.position) < 1e-14 and _rel(b.logdensity, a.logdensity) < 1e-13
    args.beta = 1.0
    so, sc = {}, {}
    fo, io = flow.rwmh_step(keys, st0, vg, model, params, args, so)
    fc, ic = cr.rwmh_step(keys, st0, args, stats=sc)
    assert (sc["n_att_inv"] == so["n_att_inv"]).all() and (sc["n_att_fwd"] == so["n_att_fwd"]).all()
    assert np.abs(sc["log_alpha"] - so["log_alpha"]).max() < 1e-7 * max(1.0, np.abs(so["log_alpha"]).max())
    assert (ic.is_accepted == io.is_accepted).all()
    assert _rel(fc.position, fo.position) < 1e-9 and _rel(fc.logdensity, fo.logdensity) < 1e-9


def test_recorded_step_sequences_and_their_replay_equal_the_numpy_restatement():
    """ode.odeint's parity instrumentation in C: the recorded step sequence of a natural solve equals numpy's (float64 step sizes to rounding,
    decisions exactly), and replaying a float32-rounded sequence gives numpy's replayed result."""
    args, dist, model, params, cr = _setup(64, 12, hidden=32, F=16)
    params = gu.rand_params(model, seed=4, scale=1.0, out_scale=0.3)
    gl = model.zero_layers()[0]
    params[gl]["kernel"] *= np.float32(1e-3 / 0.3); params[gl]["bias"] *= np.float32(1e-3)
    cr.set_params(params)
    rng = np.random.default_rng(3)
    x0, z = rng.uniform(-1, 1, (12, 64)), rng.standard_normal((12, 64))
    st, sc = {}, {}
    ode.transform_and_logdet(model, params, None, x0, True, 1e-5, 1e-5, 1000, z=z, stats=st)
    cr.solve(x0, z, +1, 1e-5, 1e-5, 1000, stats=sc, record=64)
    A = st["acc_seq"].shape[1]
    np.testing.assert_array_equal(sc["acc_seq"][:, :A], st["acc_seq"])
    assert not sc["acc_seq"][:, A:].any()
    np.testing.assert_allclose(sc["dt_seq"][:, :A + 1], st["dt_seq"], rtol=1e-7, atol=0)      # (the controller amplifies the rounding of the error norm: measured 4e-9)
    rp = dict(dt=st["dt_seq"].astype(np.float32).astype(np.float64), acc=st["acc_seq"])
    so = {}
    xo, lo = ode.transform_and_logdet(model, params, None, x0, True, 1e-5, 1e-5, 1000, z=z, stats=so, replay=rp)
    s2 = {}
    xc, lc = cr.solve(x0, z, +1, 1e-5, 1e-5, 1000, stats=s2, replay=rp)
    assert (s2["n_attempted"] == so["n_attempted"]).all()
    assert np.abs(xc - xo).max() < 1e-11 and np.abs(lc - lo).max() < 1e-10


# ---- the mixture and LGCP targets, the exact trace, n_ts = 5 and the metrics' pair sums ----------------------------------------------

def _target_setup(which, B=16, hidden=32, F=16, seed=3):
    if which == "gmm4":
        args, dist, k, model, state = gu.gmm4_setup(B=B, hidden=hidden, F=F, seed=seed, hutchs=False)
    elif which == "gmm16":
        args, dist, k, model, state = gu.gmm16_setup(B=B, hidden=hidden, F=F, seed=seed, hutchs=False)
    else:
        args, dist, k, model, state = gu.lgcp_setup(n=8, B=B, hidden=hidden, F=F, seed=seed)
    params = gu.rand_params(model, seed=seed, out_scale=0.3)
    return args, dist, model, params, cref.CRef(model, params)


def _points(which, dist, B, seed=0):
    rng = np.random.default_rng(seed)
    if which == "lgcp":
        return dist.mu + rng.standard_normal((B, dist.dim)) @ dist.chol.T
    return dist.modes[rng.integers(0, len(dist.weights), B)] + 1.5 * rng.standard_normal((B, 2))


@pytest.mark.parametrize("which", ["gmm4", "gmm16", "lgcp"])
def test_mixture_and_lgcp_targets_equal_the_numpy_restatement(which):
    args, dist, model, params, cr = _target_setup(which)
    x = _points(which, dist, 24)
    v = np.random.default_rng(1).standard_normal(x.shape)
    for temper in (1.0, 0.37):
        lp, g = targets.Tempered(dist, temper).value_and_grad(x)
        lpc, gc = cr.value_and_grad(x, temper)
        assert _rel(lpc, lp) < 1e-12 and _rel(gc, g) < 1e-12, (_rel(lpc, lp), _rel(gc, g))
    assert _rel(cr.hvp(x, v), dist.hvp_logprob(x, v)) < 1e-12


def test_mixture_far_from_every_mode_underflows_as_the_numpy_restatement():
    """Product of pdfs, then log (distributions.py:59-61): far from every mode the sum underflows to 0 -- log p = -inf, grad = hvp =
    NaN (0 / 0) -- while nearer points that still underflow PER COMPONENT in one coordinate only keep finite values."""
    args, dist, model, params, cr = _target_setup("gmm16")
    x = np.array([[1e3, 1e3], [-60.0, 0.0], [40.0, 3.0], [0.0, 0.0], [25.0, -25.0], [1e8, -1e8]])
    lp, g = targets.Tempered(dist, 0.5).value_and_grad(x)
    lpc, gc = cr.value_and_grad(x, 0.5)
    assert np.isneginf(lp).any() and np.isfinite(lp).any()
    np.testing.assert_array_equal(np.isneginf(lpc), np.isneginf(lp))
    np.testing.assert_array_equal(np.isnan(gc), np.isnan(g))
    f = np.isfinite(lp)
    assert _rel(lpc[f], lp[f]) < 1e-12 and _rel(gc[f], g[f]) < 1e-12
    v = np.ones_like(x)
    h, hc = dist.hvp_logprob(x, v), cr.hvp(x, v)
    np.testing.assert_array_equal(np.isnan(hc), np.isnan(h))
    assert _rel(hc[f], h[f]) < 1e-12
    # the MALA step from a finite state into the underflow region rejects on both sides (NaN delta -> -inf, proposal.py:105)
    st = mala.MALAState(x[f], lp[f], g[f])
    noise = np.full((int(f.sum()), 2), 1e3)
    u = np.full(int(f.sum()), 1e-300)
    keys = prng.split(prng.PRNGKey(1), int(f.sum()))
    so, info, _ = mala.kernel(keys, st, targets.Tempered(dist, 0.5).value_and_grad, 0.2, noise=noise)
    sc, p, acc = cr.mala_step(st, noise, u, 0.2, 0.5)
    assert not acc.any() and (p == 0).all() and not info.is_accepted.any()


@pytest.mark.parametrize("which", ["gmm16", "lgcp"])
def test_mala_step_on_mixture_and_lgcp_equals_the_numpy_restatement(which):
    args, dist, model, params, cr = _target_setup(which)
    x = _points(which, dist, 32)
    step = 1.5 if which != "lgcp" else 0.01
    for temper in (1.0, 0.37):
        vg = targets.Tempered(dist, temper).value_and_grad
        st0 = mala.init(x, vg)
        keys = prng.split(prng.PRNGKey(7), 32)
        a, ia, _ = mala.kernel(keys, st0, vg, step)
        b, ib = cr.mala_kernel(keys, st0, step, temper)
        assert (ia.is_accepted == ib.is_accepted).all() and 0 < ia.is_accepted.sum() < 32
        assert np.abs(ia.acceptance_rate - ib.acceptance_rate).max() < 1e-10
        assert _rel(b.position, a.position) < 1e-14 and _rel(b.logdensity, a.logdensity) < 1e-12 and _rel(b.logdensity_grad, a.logdensity_grad) < 1e-12


@pytest.mark.parametrize("which", ["gmm16", "lgcp"])
def test_field_jvp_exact_trace_and_loss_on_mixture_and_lgcp_equal_the_numpy_restatement(which):
    args, dist, model, params, cr = _target_setup(which)
    rng = np.random.default_rng(2)
    x, t = _points(which, dist, 16), rng.uniform(0, 1, 16)
    z = rng.standard_normal(x.shape)
    v, jv = model.forward(params, x, t, tangent=z)
    vc, jvc = cr.forward(x, t, tangent=z)
    assert _rel(vc, v) < 1e-12 and _rel(jvc, jv) < 1e-12
    if which != "lgcp":
        assert _rel(cr.jacobian_trace(x, t), model.jacobian_trace(params, x, t)) < 1e-12
    key = prng.PRNGKey(11)
    loss, grads = fm.loss_and_grad(model, params, key, x, args.sigma)
    lc, gc = cr.fm_loss_grad(*fm.cond_flow_batch(key, x, args.sigma))
    assert abs(lc - loss) < 1e-11 * abs(loss)
    for a, b in zip(gc, grads):
        for nm in ("kernel", "bias"):
            assert np.abs(a[nm].astype(np.float64) - b[nm]).max() <= 2e-7 * max(np.abs(b[nm]).max(), 1e-30), nm


@pytest.mark.parametrize("which", ["gmm4", "gmm16"])
def test_exact_trace_solves_equal_the_numpy_restatement_and_n_ts_keeps_the_step_sequence(which):
    """The d = 2 configurations' solves (exact trace, exe_flow_matching.py:216-217; 4-mode: n_ts = 5, :347): attempted-step counts equal,
    the recorded sequences equal, the replay of a float32-rounded sequence equal -- and n_ts = 5 takes exactly the step sequence of n_ts = 2
    (the attempt counter that restarts per output time bounds only mxstep)."""
    args, dist, model, params, cr = _target_setup(which, hidden=32, F=16)
    params = gu.rand_params(model, seed=4, scale=1.0, out_scale=1.0)
    cr.set_params(params)
    x0 = _points(which, dist, 12, seed=3)
    assert args.n_ts == (5 if which == "gmm4" else 2)
    for sign, f in ((+1, ode.transform_and_logdet), (-1, ode.inverse_and_logdet)):
        st, sc = {}, {}
        xo, lo = f(model, params, None, x0, False, args.rtol, args.atol, args.mxstep, n_ts=args.n_ts, stats=st)
        xc, lc = cr.solve(x0, None, sign, args.rtol, args.atol, args.mxstep, stats=sc, record=400, n_ts=args.n_ts)
        n = st["n_attempted"]
        assert n.min() >= 10 and sum(int((~st["acc_seq"][b, :n[b]]).sum()) for b in range(12)) >= 3
        np.testing.assert_array_equal(sc["n_attempted"], n)
        assert sc["n_evals_total"] == int((2 + 6 * n).sum())
        A = st["acc_seq"].shape[1]
        np.testing.assert_array_equal(sc["acc_seq"][:, :A], st["acc_seq"])
        # (d + 1 = 3 state components: the error estimate cancels harder than on the wide states above, the controller amplifies the
        # rounding of the two summation orders: the median step to 1e-9, the worst of several hundred to 3e-4 next to a relu kink)
        live = st["dt_seq"] > 0
        rd = np.abs(sc["dt_seq"][:, :A + 1] - st["dt_seq"])[live] / st["dt_seq"][live]
        assert np.median(rd) < 1e-8 and rd.max() < 1e-3, (np.median(rd), rd.max())
        np.testing.assert_array_equal(sc["dt_seq"][:, :A + 1] > 0, live)
        # (measured 1e-8 on gmm4, 7e-7 on gmm16: the relu kinks a solve crosses amplify the rounding difference of the two summation orders)
        assert np.abs(xc - xo).max() < 1e-5 * max(1.0, np.abs(xo).max()) and np.abs(lc - lo).max() < 1e-5 * max(1.0, np.abs(lo).max())
        # n_ts: the other number of output times gives the same sequence and the same result, on both sides
        other = 2 if args.n_ts == 5 else 5
        st2, sc2 = {}, {}
        xo2, lo2 = f(model, params, None, x0, False, args.rtol, args.atol, args.mxstep, n_ts=other, stats=st2)
        xc2, lc2 = cr.solve(x0, None, sign, args.rtol, args.atol, args.mxstep, stats=sc2, record=400, n_ts=other)
        np.testing.assert_array_equal(st2["acc_seq"], st["acc_seq"]); np.testing.assert_array_equal(st2["dt_seq"], st["dt_seq"])
        np.testing.assert_array_equal(sc2["acc_seq"], sc["acc_seq"]); np.testing.assert_array_equal(sc2["dt_seq"], sc["dt_seq"])
        np.testing.assert_array_equal(xc2, xc); np.testing.assert_array_equal(lc2, lc)
        np.testing.assert_array_equal(xo2, xo); np.testing.assert_array_equal(lo2, lo)
        # replay
        rp = dict(dt=st["dt_seq"].astype(np.float32).astype(np.float64), acc=st["acc_seq"])
        so, s2 = {}, {}
        xo3, lo3 = f(model, params, None, x0, False, args.rtol, args.atol, args.mxstep, n_ts=args.n_ts, stats=so, replay=rp)
        xc3, lc3 = cr.solve(x0, None, sign, args.rtol, args.atol, args.mxstep, stats=s2, replay=rp, n_ts=args.n_ts)
        np.testing.assert_array_equal(s2["n_attempted"], so["n_attempted"])
        assert np.abs(xc3 - xo3).max() < 1e-11 * max(1.0, np.abs(xo3).max()) and np.abs(lc3 - lo3).max() < 1e-10 * max(1.0, np.abs(lo3).max())


def test_mxstep_restarts_per_output_time_as_in_the_numpy_restatement():
    """The one place n_ts matters: with a tight mxstep the 5-output-time solve gets mxstep attempts per output time."""
    args, dist, model, params, cr = _target_setup("gmm4", hidden=32, F=16)
    params = gu.rand_params(model, seed=4, scale=1.0, out_scale=1.0)
    cr.set_params(params)
    x0 = _points("gmm4", dist, 8, seed=3)
    for n_ts in (2, 5):
        st, sc = {}, {}
        xo, lo = ode.transform_and_logdet(model, params, None, x0, False, args.rtol, args.atol, 6, n_ts=n_ts, stats=st)
        xc, lc = cr.solve(x0, None, +1, args.rtol, args.atol, 6, stats=sc, n_ts=n_ts)
        np.testing.assert_array_equal(sc["n_attempted"], st["n_attempted"])
        assert np.abs(xc - xo).max() < 1e-9 * max(1.0, np.abs(xo).max())
        assert st["n_attempted"].max() == (6 if n_ts == 2 else 24) or n_ts == 5 and st["n_attempted"].max() > 6


def test_exact_trace_flow_mh_step_on_gmm16_equals_the_numpy_restatement():
    args, dist, model, params, cr = _target_setup("gmm16", hidden=32, F=16)
    vg = targets.Tempered(dist, 1.0).value_and_grad
    st0 = mala.init(_points("gmm16", dist, 12, seed=5), vg)
    keys = prng.split(prng.PRNGKey(9), 12)
    so, sc = {}, {}
    fo, io = flow.rwmh_step(keys, st0, vg, model, params, args, so)
    fc, ic = cr.rwmh_step(keys, st0, args, stats=sc)
    np.testing.assert_array_equal(sc["n_att_inv"], so["n_att_inv"]); np.testing.assert_array_equal(sc["n_att_fwd"], so["n_att_fwd"])
    assert np.abs(sc["log_alpha"] - so["log_alpha"]).max() < 1e-9 * max(1.0, np.abs(so["log_alpha"]).max())
    assert (ic.is_accepted == io.is_accepted).all() and _rel(fc.position, fo.position) < 1e-10


def test_lgcp_hutchinson_solve_equals_the_numpy_restatement():
    args, dist, model, params, cr = _target_setup("lgcp", hidden=32, F=16)
    gl = model.zero_layers()[0]                       # unclipped at d = 64: grad log pi is O(10 - 100), the gate scaled down
    params[gl]["kernel"] *= np.float32(1e-2); params[gl]["bias"] *= np.float32(1e-2)
    cr.set_params(params)
    x0 = _points("lgcp", dist, 8, seed=6)
    z = np.random.default_rng(4).standard_normal(x0.shape)
    for sign, f in ((+1, ode.transform_and_logdet), (-1, ode.inverse_and_logdet)):
        st, sc = {}, {}
        xo, lo = f(model, params, None, x0, True, args.rtol, args.atol, args.mxstep, z=z, stats=st)
        xc, lc = cr.solve(x0, z, sign, args.rtol, args.atol, args.mxstep, stats=sc)
        assert st["n_attempted"].min() >= 5
        np.testing.assert_array_equal(sc["n_attempted"], st["n_attempted"])
        assert np.abs(xc - xo).max() < 1e-9 * max(1.0, np.abs(xo).max()) and np.abs(lc - lo).max() < 1e-9 * max(1.0, np.abs(lo).max())


def test_libmfm_ref_refuses_what_it_does_not_cover():
    args, dist, model, params, cr = _target_setup("gmm16")
    x = _points("gmm16", dist, 4)
    with pytest.raises(AssertionError, match="Hutchinson"):
        cr.solve(x, np.ones_like(x), +1, 1e-5, 1e-5, 100)
    a2 = loop.default_args(example="gaussian-mixture", dim=2, num_chain=4, hutchs=False, num_importance_samples=-1)
    st0 = mala.init(x, targets.Tempered(dist, 1.0).value_and_grad)
    with pytest.raises(AssertionError, match="IMH"):
        cr.rwmh_step(prng.split(prng.PRNGKey(1), 4), st0, a2)
    from oracle.vfield import VectorFieldNet
    m2 = VectorFieldNet(model.f, dist, model.hidden_x, model.hidden_t, model.hidden_xt, "tanh")
    with pytest.raises(AssertionError, match="relu"):
        cref.CRef(m2, params)
    with pytest.raises(AssertionError, match="targets"):
        cref.CRef(model, params, target=targets.IndepGaussian(2))


@pytest.mark.parametrize("n", [333, 1000])
def test_stein_and_mmd_pair_sums_equal_the_numpy_restatement(n):
    args, dist, model, params, cr = _target_setup("gmm16")
    x, y = _points("gmm16", dist, n, seed=1), _points("gmm16", dist, n, seed=2)
    g = dist.grad_logprob(x)
    for beta in (-0.5, -0.3):
        u, v = cref.stein_disc(x, g, beta)
        uo, vo = metrics.stein_disc(x, lambda _: g, beta)
        assert abs(u - uo) < 1e-11 * abs(vo) and abs(v - vo) < 1e-11 * abs(vo)
    assert abs(cref.max_mean_disc(x, y) - metrics.max_mean_disc(x, y)) < 1e-12


# ---- planted errors: each changes the oracle far beyond its agreement with the numpy restatement --------------------------------------

def test_planted_errors_move_the_oracle():
    """The GPU full-size tests (tests/test_gpu_fullsize_configs.py) require the device to MISS each of these planted oracle errors by 10x
    its bound; here: each is a real change, orders of magnitude above the C / numpy agreement pinned above."""
    # one JVP of the exact trace dropped
    args, dist, model, params, cr = _target_setup("gmm16", hidden=32, F=16)
    x0 = _points("gmm16", dist, 8, seed=3)
    _, l_ok = cr.solve(x0, None, +1, args.rtol, args.atol, args.mxstep)
    _, l_bad = cr.solve(x0, None, +1, args.rtol, args.atol, args.mxstep, drop_jvp=1)
    assert np.median(np.abs(l_bad - l_ok)) > 1e-4                      # (C vs numpy: 1e-8 above)
    # one mixture component dropped
    from oracle.targets import GaussianMixture
    cut = GaussianMixture(dist.modes[1:], dist.covs[1:], dist.weights[1:])
    x = _points("gmm16", dist, 64, seed=4)
    lp, g = cr.value_and_grad(x)
    lp2, g2 = cref.CRef(model, params, target=cut).value_and_grad(x)
    assert np.abs(lp2 - lp).max() > 1e-2
    # the K^-1 term with mu shifted by 1e-3
    import copy
    args, dist, model, params, cr = _target_setup("lgcp")
    sh = copy.copy(dist); sh.mu = dist.mu + 1e-3
    x = _points("lgcp", dist, 8)
    lp, g = cr.value_and_grad(x)
    lp2, g2 = cref.CRef(model, params, target=sh).value_and_grad(x)
    assert np.abs(g2 - g).max() > 1e-6 * np.abs(g).max()                # (C vs numpy: 1e-12)
    # the U-statistic without its diagonal removed
    args, dist, model, params, cr = _target_setup("gmm16")
    x = _points("gmm16", dist, 500, seed=5)
    tot, diag = cref.stein_sums(x, dist.grad_logprob(x))
    u = (tot - diag) / (500 * 499)
    assert abs(tot / (500 * 499) - u) > 1e-3 * abs(tot / 500 ** 2)
