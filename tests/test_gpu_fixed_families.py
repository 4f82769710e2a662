"""GPU parity of the FIXED-STEP mode (mfm_config.ode_method / ode_steps: N equal steps of classical RK4 or forward Euler) on the
solvers beyond the shape-specialised tile: the wide family (mfm_amd/csrc/wide.hip: solve_fixed -- every network that is not the
default two-layer one, the pines widths, the exact-trace solves of fused-family contexts) and the d = 2 four-chain tiles
(mfm_amd/csrc/ode_d2.hip: solve_fixed -- the 4-mode and gaussian-mixture examples).  The oracle is oracle/ode.py: odeint_fixed through
the oracle's transforms and flow steps with the same integrator (oracle/flow.py: fixed_mode): same steps and stages, float32 against
float64, so the bounds are those of tests/test_gpu_fixed.py."""
import numpy as np
import pytest

from oracle import flow, mala, ode, prng, targets

pytestmark = pytest.mark.gpu


def _dev(x, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def _tamed(model, seed, out_scale, gate):
    from tests import gpu_util as gu
    p = gu.rand_params(model, seed=seed, out_scale=out_scale)
    g = model.zero_layers()[0]                         # the gate layer (t.., x.., GATE, joint.., out)
    p[g]["kernel"] *= gate; p[g]["bias"] *= gate
    return p


def _setup(kind, d, B, hidden, F, **kw):
    from tests import gpu_util as gu
    if kind == "phi4":
        return gu.phi4_setup(d=d, B=B, hidden=hidden, F=F, **kw)
    return gu.lgcp_setup(n=int(np.sqrt(d)), B=B, hidden=hidden, F=F, **kw)


def _wide_ctx(dist, args, model, params):
    from mfm_amd import _lib
    from tests import gpu_util as gu
    ctx = gu.make_ctx(dist, args, fourier=model.f, params=params, family=_lib.FAMILY_WIDE)
    assert ctx.cfg.kernel_family == _lib.FAMILY_WIDE
    return ctx


def _check_transforms(ctx, model, params, x32, hutch, method, steps, label, directions=(1, -1), n_ts=2, kink=False):
    """Both directions against the oracle; per-chain probe keys with --hutch.  `kink`: d <= 128, where the reference does not clip
    grad log pi (exe_flow_matching.py:351) and an isolated chain's log-det meets a ReLU kink within float32 rounding (tests/test_gpu_fixed.py)."""
    import torch
    B, d = x32.shape
    keys = prng.split(prng.PRNGKey(21), B)
    for direction in directions:
        fn = ode.transform_and_logdet if direction > 0 else ode.inverse_and_logdet
        y_o, l_o = fn(model, params, keys if hutch else None, x32.astype(np.float64), hutch, 0, 0, 0, n_ts=n_ts, fixed=(method, steps))
        out = torch.empty(B, d, device="cuda"); ldj = torch.empty(B, device="cuda"); ns = torch.empty(B, dtype=torch.int32, device="cuda")
        if hutch:
            ctx.ode_transform(direction, _dev(x32), out, ldj, keys=_dev(keys.astype(np.uint32).view(np.int32)), nsteps=ns)
        else:
            ctx.ode_transform(direction, _dev(x32), out, ldj, key=prng.PRNGKey(1), nsteps=ns)
        y, l = out.cpu().numpy(), ldj.cpu().numpy()
        ey, el, ls = np.abs(y - y_o).max(), np.abs(l - l_o), max(1.0, np.abs(l_o).max())
        print(f"{label} {method} x {steps} dir {direction:+d}: |dy| {ey:.2e} (|y - x| {np.abs(y_o - x32).max():.2f}), "
              f"|dl| q90 {np.quantile(el, 0.9):.2e} max {el.max():.2e} (|l| {np.abs(l_o).max():.2f})")
        assert np.abs(y_o - x32).max() > 0.05 and np.abs(l_o).max() > 0.05          # a non-trivial flow
        assert ey < 3e-5 * max(1.0, np.abs(y_o).max()), ey
        assert np.quantile(el, 0.9) < 2e-5 * ls and el.max() < (1e-3 if kink else 5e-5) * ls, (np.quantile(el, 0.9), el.max(), ls)
        np.testing.assert_array_equal(ns.cpu().numpy(), steps)


# ---- wide family ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,steps", [("rk4", 8), ("rk4", 7), ("euler", 12)])
@pytest.mark.parametrize("kind,gate", [("phi4", 1e-3), ("lgcp", 0.05)])
def test_wide_fixed_transform_and_inverse_match_oracle(kind, gate, method, steps):
    """An RK4 time batch serves two steps, an Euler one five: 7 and 12 steps end on a partial batch."""
    B, d = 32, 64
    args, dist, k, model, state = _setup(kind, d, B, 32, 16, ode_method=method, ode_steps=steps)
    params = _tamed(model, 9, 0.5, gate)
    ctx = _wide_ctx(dist, args, model, params)
    _check_transforms(ctx, model, params, dist.init_params.astype(np.float32), True, method, steps, f"wide {kind} d = {d}", kink=True)
    ctx.close()


@pytest.mark.parametrize("kind,d,hidden", [("lgcp", 256, 64), ("phi4", 144, 48)])
def test_wide_fixed_exact_trace_matches_oracle(kind, d, hidden):
    """No --hutch: the exact Jacobian trace of the wide family (wide.hip: exact_trace) as the log-det integrand, on the shapes of
    tests/test_gpu_wide.py's exact-trace test (phi-four d = 144 > 128 switches the clip on)."""
    B = 32
    args, dist, k, model, state = _setup(kind, d, B, hidden, 16, hutch=False, ode_method="rk4", ode_steps=12)
    params = _tamed(model, 9, 3.0, 0.05) if kind == "lgcp" else _tamed(model, 9, 4.0, 1e-3)
    ctx = _wide_ctx(dist, args, model, params)
    _check_transforms(ctx, model, params, dist.init_params.astype(np.float32), False, "rk4", 12, f"wide exact {kind} d = {d}")
    ctx.close()


def test_wide_fixed_transform_on_a_three_layer_network():
    """`--hidden_x a b c`: three hidden layers per branch (tests/test_gpu_depth.py: THREE) run on the wide family."""
    from tests.test_gpu_depth import DEPTHS
    B, d = 32, 64
    args, dist, k, model, state = _setup("phi4", d, B, DEPTHS["3-3-3"], 16, ode_method="rk4", ode_steps=6)
    params = _tamed(model, 9, 0.5, 1e-3)
    ctx = _wide_ctx(dist, args, model, params)
    _check_transforms(ctx, model, params, dist.init_params.astype(np.float32), True, "rk4", 6, "wide depth 3", directions=(1,), kink=True)
    ctx.close()


def test_wide_fixed_transform_at_the_pines_shape():
    """BASELINE configs[4]'s network: 32 x 32 grid, hidden width 1024 (the wide family's by mfm_create's own choice)."""
    from tests import gpu_util as gu
    B = 32
    args, dist, k, model, state = gu.lgcp_setup(n=32, B=B, hidden=1024, F=128, ode_method="rk4", ode_steps=8)
    params = _tamed(model, 2, 0.2, 0.02)
    ctx = gu.make_ctx(dist, args, fourier=model.f, params=params)
    _check_transforms(ctx, model, params, dist.init_params.astype(np.float32), True, "rk4", 8, "wide pines", directions=(1,))
    ctx.close()


def _flow_check(ctx, dist, model, params, args, mode, beta, steps, label):
    """One flow-MH step against the oracle's with the same integrator (exe_flow_matching.py:246-278): proposal, unclipped acceptance
    ratio (bounded as in tests/test_gpu_fixed.py), decisions, accepted states, 2 N steps per chain."""
    import torch
    from mfm_amd import _lib
    x32 = dist.init_params.astype(np.float32)
    B, d = x32.shape
    vg = targets.Tempered(dist, beta).value_and_grad
    pos = _dev(x32); logp = torch.empty(B, dtype=torch.float64, device="cuda"); grad = torch.empty(B, d, device="cuda")
    ctx.mala_init(pos, beta, logp, grad)
    st = mala.MALAState(x32.astype(np.float64), logp.cpu().numpy(), grad.cpu().numpy().astype(np.float64))
    key = prng.PRNGKey(31)
    so = {}
    step = flow.rwmh_step if mode == "rwmh" else flow.imh_step
    new, info = step(prng.split(key, B), st, vg, model, params, args, so)
    acc = torch.empty(B, device="cuda"); isacc = torch.empty(B, dtype=torch.uint8, device="cuda")
    prop = torch.empty(B, d, device="cuda"); ns = torch.empty(B, dtype=torch.int32, device="cuda")
    ctx.reset_counters()
    ctx.flow_step(_lib.FLOW_RWMH if mode == "rwmh" else _lib.FLOW_IMH, key, beta, pos, logp, grad, acc, isacc, prop, ns)
    p = prop.cpu().numpy()
    e_p = np.abs(p - info.proposed_position).max()
    with np.errstate(divide="ignore"):
        la_g, la_o = np.log(acc.cpu().numpy().astype(np.float64)), so["log_alpha"]
    fin = np.isfinite(la_g) & (la_o > -80)
    dla = np.abs(la_g[fin] - la_o[fin])
    gn = np.linalg.norm(vg(info.proposed_position)[1], axis=1)
    print(f"{label} {args.ode_method} x {steps} {mode}: |dx'| {e_p:.2e}, |d log alpha| median {np.median(dla):.2e} max {dla.max():.2e}; "
          f"accepted gpu {int(isacc.sum().item())} oracle {int(info.is_accepted.sum())}")
    assert e_p < 3e-5 * max(1.0, np.abs(info.proposed_position).max())
    assert fin.sum() >= B // 2 and (dla <= 3.0 * gn[fin] * np.linalg.norm(p - info.proposed_position, axis=1)[fin] + 2e-3).all()
    same = isacc.cpu().numpy().astype(bool) == info.is_accepted
    assert same.mean() >= 0.9
    np.testing.assert_allclose(pos.cpu().numpy()[same], new.position[same], atol=3e-5 * max(1.0, np.abs(new.position).max()))
    np.testing.assert_array_equal(ns.cpu().numpy(), 2 * steps)
    c = ctx.counters()
    assert c["dopri_attempts"] == 2 * steps * B
    assert c["field_evals"] == (4 if args.ode_method == "rk4" else 1) * c["dopri_attempts"]


# beta: phi-four's independent proposals at beta = 0.7 all have log alpha < -80 (nothing to compare); 1e-3 gives ratios of order one
@pytest.mark.parametrize("kind,mode,gate,out_scale,beta", [("lgcp", "rwmh", 0.05, 0.3, 0.7), ("phi4", "imh", 1e-3, 0.05, 1e-3)])
def test_wide_fixed_flow_step_matches_oracle(kind, mode, gate, out_scale, beta):
    """RWMH on the Cox target (its K^-1 GEMM in the accept step), IMH on phi-four, both solves on fixed steps."""
    B, d = 32, 64
    args, dist, k, model, state = _setup(kind, d, B, 32, 16, ode_method="rk4", ode_steps=8)
    params = _tamed(model, 9, out_scale, gate)
    ctx = _wide_ctx(dist, args, model, params)
    _flow_check(ctx, dist, model, params, args, mode, beta, 8, f"wide {kind}")
    ctx.close()


# ---- d = 2 four-chain tiles ----------------------------------------------------------------------------------------------------
def _d2_setup(which, B, method, steps):
    from tests import gpu_util as gu
    if which == "gmm16":
        args, dist, k, model, state = gu.gmm16_setup(B=B, hutchs=False, ode_method=method, ode_steps=steps)
    else:
        args, dist, k, model, state = gu.gmm4_setup(B=B, hidden=128, F=128, hutchs=False, ode_method=method, ode_steps=steps)
    params = gu.rand_params(model, seed=9, out_scale=0.3)
    return gu, args, dist, model, params


@pytest.mark.parametrize("tile", ["4", "4s"])
def test_d2_fixed_transform_matches_oracle(monkeypatch, tile):
    """4-mode (n_ts = 5: the oracle's intermediate outputs fall on step boundaries, N a multiple of 4), exact trace, both directions,
    on the resident-weight tile and the streamed one (MFM_D2_TILE=4s)."""
    monkeypatch.setenv("MFM_D2_TILE", tile)
    B = 64
    gu, args, dist, model, params = _d2_setup("gmm4", B, "rk4", 16)
    assert args.n_ts == 5
    x32 = (4.0 * np.random.default_rng(3).standard_normal((B, 2))).astype(np.float32)
    ctx = gu.make_ctx(dist, args, fourier=model.f, params=params)
    _check_transforms(ctx, model, params, x32, False, "rk4", 16, f"d2 tile {tile}", n_ts=args.n_ts)
    ctx.close()


@pytest.mark.parametrize("tile", ["4", "4s"])
@pytest.mark.parametrize("which,mode,method,steps", [("gmm4", "rwmh", "rk4", 8), ("gmm4", "imh", "rk4", 8), ("gmm16", "rwmh", "euler", 12)])
def test_d2_fixed_flow_step_matches_oracle(monkeypatch, tile, which, mode, method, steps):
    monkeypatch.setenv("MFM_D2_TILE", tile)
    gu, args, dist, model, params = _d2_setup(which, 32, method, steps)
    if mode == "imh":
        args.num_importance_samples = -1
    ctx = gu.make_ctx(dist, args, fourier=model.f, params=params)
    _flow_check(ctx, dist, model, params, args, mode, 0.7, steps, f"d2 {which} tile {tile}")
    ctx.close()


def test_d2_fixed_steps_still_decline_on_the_generic_tile(monkeypatch):
    import torch
    from mfm_amd import _lib
    monkeypatch.setenv("MFM_D2_TILE", "16")
    gu, args, dist, model, params = _d2_setup("gmm4", 32, "rk4", 8)
    ctx = gu.make_ctx(dist, args, fourier=model.f, params=params)
    x = _dev(np.zeros((32, 2), np.float32)); out = torch.empty(32, 2, device="cuda"); ldj = torch.empty(32, device="cuda")
    with pytest.raises(_lib.MfmError, match="fixed-step mode"):
        ctx.ode_transform(1, x, out, ldj, key=(0, 1))
    ctx.close()


# ---- the headline tile's counter ---------------------------------------------------------------------------------------------
def test_field_eval_counter_of_the_headline_tile_in_fixed_step_mode():
    from tests import gpu_util as gu
    args, dist, k, model, state = gu.phi4_setup(d=256, B=32, ode_method="euler", ode_steps=10)
    params = _tamed(model, 9, 0.05, 1e-3)
    ctx = gu.make_ctx(dist, args, fourier=model.f, params=params)
    _flow_check(ctx, dist, model, params, args, "rwmh", 1e-3, 10, "headline tile")
    ctx.close()


# ---- whole runs ------------------------------------------------------------------------------------------------------------------
def _check_run(out, res, ex, steps, loss_rtol):
    tr, m = out["trace"], ex["metrics"]
    np.testing.assert_allclose(m[:3, 0], tr["loss"][:3], rtol=1e-5)
    np.testing.assert_allclose(m[:, 0], tr["loss"], rtol=loss_rtol)
    np.testing.assert_allclose(ex["betas"], tr["beta"], rtol=2e-3)
    c = ex["engine"].ctx.counters()
    print(f"run: {c['ode_solves']} solves, {c['dopri_attempts']} attempted steps, {c['field_evals']} field evaluations")
    assert c["ode_solves"] > 0 and c["dopri_attempts"] == steps * c["ode_solves"]      # every solve takes exactly N steps
    assert np.isfinite(res).all() and np.isfinite(m[:, 0]).all()
    ex["engine"].close()


def test_fixed_step_4mode_run_matches_oracle():
    """`--example 4-mode --ode_method rk4 --ode_steps 16` through run() (d = 2 tile, exact trace, n_ts = 5)."""
    from tests.test_gpu_loop import _run_both
    out, res, ex = _run_both("4-mode", 2, 64, 8, 3, hutch=False, step_size=0.2, ode_method="rk4", ode_steps=16)
    _check_run(out, res, ex, 16, 1e-2)


def test_fixed_step_depth3_run_matches_oracle():
    """`--hidden_x 32 48 32 ...` (three hidden layers per branch: the wide family) with `--ode_method rk4 --ode_steps 8`."""
    from tests.test_gpu_depth import DEPTHS
    from tests.test_gpu_loop import _run_both
    out, res, ex = _run_both("phi-four", 64, 32, 8, 3, width=DEPTHS["3-3-3"], step_size=1e-4, ode_method="rk4", ode_steps=8)
    _check_run(out, res, ex, 8, 1e-2)
