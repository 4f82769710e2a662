"""GPU parity of the remaining phi-four boundary paths against the restated oracle (tests/phi4_bc_oracle.py), periodic and Dirichlet 1:
the training kernel's grad log pi input (fm_loss_grad: static headline instance, non-static instances, generic widths), the eval
kernel (fm_loss at d = 16, both row counts), the fused MALA of mfm_train_iter against MFM_NO_FUSED_MALA, the HMC step, vf_apply on
both families, fixed-step RK4 on the headline tile, the wide family with exact trace, and a short exe_flow_matching.run against
oracle.loop.run.  As in tests/test_gpu_phi4_bc.py, each comparison also requires the device to miss the Dirichlet-0 oracle by at
least 10x its tolerance; tolerances are those of the existing tests of the same paths."""
import numpy as np
import pytest

from oracle import fm, hmc, mala, ode, prng, targets
from tests.phi4_bc_oracle import PhiFourBC

pytestmark = pytest.mark.gpu

BCS = [("pbc", 0.0), ("dirichlet", 1.0)]


def _dev(x, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def _relerr(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def _setup(d, B, bc, hidden=128, F=128, **kw):
    from tests import gpu_util as gu
    args, dist0, k, model0, state = gu.phi4_setup(d=d, B=B, hidden=hidden, F=F, **kw)
    dist = PhiFourBC(d, dist0.a, dist0.beta, bc)
    dist.init_params = dist0.init_params
    model = type(model0).__new__(type(model0)); model.__dict__.update(model0.__dict__); model.dist = dist     # the oracle field of this boundary
    return args, dist, dist0, model, model0


def _ctx(dist, args, **kw):
    from mfm_amd import _lib
    from tests import gpu_util as gu
    ctx = gu.make_ctx(dist, args, **kw)
    ctx.set_target(_lib.PHI4, dist.block())
    return ctx


# (d, B, hidden, F): the static headline instance, the non-static one-tile-per-wave instance, generic widths
@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("d,B,hidden,F", [(256, 64, 128, 128), (64, 32, 32, 16), (40, 16, 48, 10)])
def test_fm_loss_and_grad(d, B, hidden, F, bc):
    import torch
    from tests import gpu_util as gu
    args, dist, dist0, model, model0 = _setup(d, B, bc, hidden, F)
    params = gu.rand_params(model, seed=3)
    ctx = _ctx(dist, args, fourier=model.f, params=params)
    x32 = dist.init_params.astype(np.float32)
    key = prng.PRNGKey(11)
    loss_o, grads_o = fm.loss_and_grad(model, params, key, x32.astype(np.float64), args.sigma)
    loss_0, grads_0 = fm.loss_and_grad(model0, params, key, x32.astype(np.float64), args.sigma)
    loss = torch.zeros(1, dtype=torch.float64, device="cuda"); grads = torch.zeros(ctx.n_params, device="cuda")
    ctx.fm_loss_grad(key, _dev(x32), loss, grads)
    assert abs(loss.item() - loss_o) <= 2e-5 * abs(loss_o), (loss.item(), loss_o)
    g = gu.unflat_params(model, grads.cpu().numpy())
    miss = abs(loss.item() - loss_0) / (2e-5 * abs(loss_0))
    for i, (gg, go, g0) in enumerate(zip(g, grads_o, grads_0)):
        for kk in ("kernel", "bias"):
            assert _relerr(gg[kk], go[kk].astype(np.float64)) < 2e-4, (i, kk, _relerr(gg[kk], go[kk]))
            miss = max(miss, _relerr(gg[kk], g0[kk].astype(np.float64)) / 2e-4)
    l2 = torch.zeros(1, dtype=torch.float64, device="cuda")
    ctx.fm_loss(key, _dev(x32), l2)
    assert abs(l2.item() - loss_o) <= 2e-5 * abs(loss_o)
    print(f"fm_loss_grad {bc} d={d}: loss {loss.item():.6g}, miss vs Dirichlet 0: {miss:.0f}x tol")
    assert miss >= 10.0, miss
    ctx.close()


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("rows", ["32", "64"])
def test_eval_kernel_loss(monkeypatch, rows, bc):
    """fm_eval_kernel (d <= 16, >= 16384 samples): 32- and 64-row instances."""
    import torch
    from tests import gpu_util as gu
    monkeypatch.setenv("MFM_EVAL_ROWS", rows)
    d, n = 16, 16384
    args, dist, dist0, model, model0 = _setup(d, 16, bc, 32, 16)
    params = gu.rand_params(model, seed=3)
    ctx = _ctx(dist, args, fourier=model.f, params=params, max_eval=n)
    from mfm_amd import _lib
    assert ctx.fm_eval_instance(n) == int(rows) | _lib.EVAL_BCRT            # fm_eval_kernel<2 | 4, -1, false, BCRT>
    x = np.random.default_rng(5).uniform(-1, 1, (n, d)).astype(np.float32)
    key = prng.PRNGKey(12)
    loss_o, _ = fm.loss_and_grad(model, params, key, x.astype(np.float64), args.sigma)
    loss_0, _ = fm.loss_and_grad(model0, params, key, x.astype(np.float64), args.sigma)
    l = torch.zeros(1, dtype=torch.float64, device="cuda")
    ctx.fm_loss(key, _dev(x), l)
    assert abs(l.item() - loss_o) <= 2e-5 * abs(loss_o), (l.item(), loss_o)
    miss = abs(l.item() - loss_0) / (2e-5 * abs(loss_0))
    print(f"eval loss {bc} rows={rows}: miss vs Dirichlet 0: {miss:.0f}x tol")
    assert miss >= 10.0, miss
    ctx.close()


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("d,hidden,F", [(256, 128, 128), (64, 32, 16)])
def test_fused_mala_train_iter_equals_separate(monkeypatch, d, hidden, F, bc):
    """mfm_train_iter's MALA step inside the training kernel (static headline instance / one tile per wave) against the same iteration
    with MFM_NO_FUSED_MALA (stand-alone MALA kernel + training kernel): bit-identical; and the gradient left in the state is the
    boundary's, not Dirichlet 0's."""
    import torch
    from mfm_amd._lib import FLOW_RWMH
    from tests import gpu_util as gu
    B = 64
    args, dist, dist0, model, model0 = _setup(d, B, bc, hidden, F)
    params = gu.rand_params(model, seed=3, out_scale=0.05)
    x0 = dist.init_params.astype(np.float32)
    eps = 1e-7 if d == 256 else args.step_size      # (the as-written acceptance rule rejects every d = 256 proposal at 1e-4)
    out = []
    for fused in (True, False):
        if fused:
            monkeypatch.delenv("MFM_NO_FUSED_MALA", raising=False)
        else:
            monkeypatch.setenv("MFM_NO_FUSED_MALA", "1")
        ctx = _ctx(dist, args, fourier=model.f, params=params)
        pos = _dev(x0); logp = torch.empty(B, device="cuda", dtype=torch.float64); grad = torch.empty_like(pos)
        acc = torch.empty(B, device="cuda"); loss = torch.zeros(1, device="cuda", dtype=torch.float64); grads = torch.zeros(ctx.n_params, device="cuda")
        ctx.mala_init(pos, 1.0, logp, grad)
        ks, losses = prng.PRNGKey(5), []
        for count in range(1, 4):
            ks, kg, kt = prng.split(ks, 3)
            ctx.train_iter(count, 100, FLOW_RWMH, kg, kt, 1.0, eps, pos, logp, grad, loss, grads, acc=acc)
            losses.append(loss.item())
        out.append((pos.cpu().numpy(), logp.cpu().numpy(), grad.cpu().numpy(), np.array(losses), ctx.get_params(), acc.cpu().numpy()))
        ctx.close()
    for u, v in zip(*out):
        np.testing.assert_array_equal(u, v)
    p, lp, g = out[0][0].astype(np.float64), out[0][1], out[0][2]
    assert (out[0][5] > 0).any()                                            # some proposals were accepted
    np.testing.assert_allclose(lp, dist.loglik(p), rtol=2e-6, atol=2e-3)
    g0 = dist0.grad_logprob(p)
    tol = 3e-3 + 3e-5 * np.abs(g0)
    np.testing.assert_allclose(g, dist.grad_logprob(p), rtol=3e-5, atol=3e-3)
    assert (np.abs(g - g0) / tol).max() >= 10.0


@pytest.mark.parametrize("bc", BCS)
def test_hmc_step(bc):
    import torch
    d, B, eps, L, beta = 64, 64, 2e-4, 12, 0.7
    args, dist, dist0, model, model0 = _setup(d, B, bc, 32, 16)
    ctx = _ctx(dist, args)
    x32 = dist.init_params.astype(np.float32)
    pos = _dev(x32); logp = torch.empty(B, dtype=torch.float64, device="cuda"); grad = torch.empty(B, d, device="cuda")
    ctx.mala_init(pos, beta, logp, grad)
    vg, vg0 = targets.Tempered(dist, beta).value_and_grad, targets.Tempered(dist0, beta).value_and_grad
    st = mala.MALAState(x32.astype(np.float64), logp.cpu().numpy(), grad.cpu().numpy().astype(np.float64))
    acc = torch.empty(B, device="cuda"); isacc = torch.empty(B, dtype=torch.uint8, device="cuda")
    key = prng.PRNGKey(50)
    ctx.hmc_step(key, beta, eps, L, pos, logp, grad, acc, isacc)
    st_o, info, u = hmc.kernel(prng.split(key, B), st, vg, eps, L)
    st_0, info0, _ = hmc.kernel(prng.split(key, B), st, vg0, eps, L)
    ia_g = isacc.cpu().numpy().astype(bool)
    tol = 5e-6 * max(1.0, np.abs(st.logdensity).max())
    assert np.abs(np.log(np.maximum(acc.cpu().numpy(), 1e-30)) - np.log(np.maximum(info.acceptance_rate, 1e-30))).max() < tol + 1e-5
    border = np.abs(u - info.acceptance_rate) < 10 * tol * np.maximum(info.acceptance_rate, 1e-30) + 1e-6
    assert (ia_g == info.is_accepted)[~border].all() and ia_g.any()
    # the trajectory's end point (accepted or not) is the proposal of both sides
    pe = np.where(ia_g[:, None], pos.cpu().numpy().astype(np.float64), np.nan)
    po, p0 = info.proposed_position[ia_g], info0.proposed_position[ia_g]
    e, e0 = np.abs(pe[ia_g] - po).max(), np.abs(pe[ia_g] - p0).max()
    scale = 3e-6 * max(1.0, np.abs(po).max())
    print(f"hmc {bc}: |dx| {e:.1e}, miss vs Dirichlet 0: {e0 / scale:.0f}x tol")
    assert e < scale and e0 >= 10 * scale, (e, e0, scale)
    ctx.close()


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("family", ["tile", "wide"])
@pytest.mark.parametrize("d,hidden,F", [(256, 128, 128), (40, 32, 10)])
def test_vector_field_and_jvp(d, hidden, F, family, bc):
    import torch
    from mfm_amd import _lib
    from tests import gpu_util as gu
    B = 32
    args, dist, dist0, model, model0 = _setup(d, B, bc, hidden, F)
    params = gu.rand_params(model, seed=6)
    ctx = _ctx(dist, args, fourier=model.f, params=params, **(dict(family=_lib.FAMILY_WIDE) if family == "wide" else {}))
    rng = np.random.default_rng(1)
    x = dist.init_params.astype(np.float32); t = rng.uniform(0, 1, B).astype(np.float32)
    z = rng.standard_normal((B, d)).astype(np.float32)
    v_o, jv_o = model.forward(params, x.astype(np.float64), t.astype(np.float64), tangent=z.astype(np.float64))
    v_0, jv_0 = model0.forward(params, x.astype(np.float64), t.astype(np.float64), tangent=z.astype(np.float64))
    v = torch.empty(B, d, device="cuda"); jv = torch.empty(B, d, device="cuda")
    ctx.vf_apply(_dev(x), _dev(t), v, _dev(z), jv)
    v, jv = v.cpu().numpy(), jv.cpu().numpy()
    assert _relerr(v, v_o) < 2e-5 and _relerr(jv, jv_o) < 2e-5, (_relerr(v, v_o), _relerr(jv, jv_o))
    miss = max(_relerr(v, v_0), _relerr(jv, jv_0)) / 2e-5
    print(f"vf_apply {bc} d={d} {family}: miss vs Dirichlet 0: {miss:.0f}x tol")
    assert miss >= 10.0, miss
    ctx.close()


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("family,hutch", [(None, True), ("wide", False)])
def test_fixed_step_rk4_transform(family, hutch, bc):
    """RK4 x 16 on the headline tile (flow_step_fixed / ode_transform_fixed, PHI4_BCRT), and the wide family with EXACT trace (d = 64)."""
    import torch
    from mfm_amd import _lib
    d, hidden, F = (256, 128, 128) if family is None else (64, 48, 16)
    B, steps = 32, 16
    args, dist, dist0, model, model0 = _setup(d, B, bc, hidden, F, hutch=hutch, ode_method="rk4", ode_steps=steps)
    from tests import gpu_util as gu
    params = gu.rand_params(model, seed=9, out_scale=0.5)
    params[4]["kernel"] *= 1e-2; params[4]["bias"] *= 1e-2
    ctx = _ctx(dist, args, fourier=model.f, params=params, **(dict(family=_lib.FAMILY_WIDE) if family else {}))
    x32 = dist.init_params.astype(np.float32)
    keys = prng.split(prng.PRNGKey(21), B)
    y_o, l_o = ode.transform_and_logdet(model, params, keys, x32.astype(np.float64), hutch, 0, 0, 0, fixed=("rk4", steps))
    y_0, l_0 = ode.transform_and_logdet(model0, params, keys, x32.astype(np.float64), hutch, 0, 0, 0, fixed=("rk4", steps))
    out = torch.empty(B, d, device="cuda"); ldj = torch.empty(B, device="cuda"); ns = torch.empty(B, dtype=torch.int32, device="cuda")
    ctx.ode_transform(1, _dev(x32), out, ldj, keys=_dev(keys.astype(np.uint32).view(np.int32)), nsteps=ns)
    y, l = out.cpu().numpy(), ldj.cpu().numpy()
    ys, ls = max(1.0, np.abs(y_o).max()), max(1.0, np.abs(l_o).max())
    ey, el = np.abs(y - y_o).max(), np.abs(l - l_o)
    assert ey < 3e-5 * ys and np.quantile(el, 0.9) < 2e-5 * ls and el.max() < 1e-3 * ls, (ey, np.quantile(el, 0.9), el.max())
    np.testing.assert_array_equal(ns.cpu().numpy(), steps)
    miss = max(np.abs(y - y_0).max() / (3e-5 * ys), np.quantile(np.abs(l - l_0), 0.9) / (2e-5 * ls))
    print(f"rk4 x {steps} {bc} d={d} {family or 'fast'} hutch={hutch}: |dy| {ey:.1e}, |dl| {el.max():.1e}, miss vs Dirichlet 0: {miss:.0f}x tol")
    assert miss >= 10.0, miss
    ctx.close()


@pytest.mark.parametrize("bc", [("pbc", 0.0)])
def test_fixed_step_rk4_flow_step_headline(bc):
    """The RK4 x 16 flow-MH step on the headline tile: proposal and log acceptance ratio against the oracle on the same keys."""
    import torch
    from mfm_amd import _lib
    from oracle import flow
    from tests import gpu_util as gu
    d, B, steps, beta = 256, 32, 16, 1e-3
    args, dist, dist0, model, model0 = _setup(d, B, bc, ode_method="rk4", ode_steps=steps)
    params = gu.rand_params(model, seed=9, out_scale=0.05)
    params[4]["kernel"] *= 1e-3; params[4]["bias"] *= 1e-3
    ctx = _ctx(dist, args, fourier=model.f, params=params)
    vg, vg0 = targets.Tempered(dist, beta).value_and_grad, targets.Tempered(dist0, beta).value_and_grad
    x32 = dist.init_params.astype(np.float32)
    pos = _dev(x32); logp = torch.empty(B, dtype=torch.float64, device="cuda"); grad = torch.empty(B, d, device="cuda")
    ctx.mala_init(pos, beta, logp, grad)
    st = mala.MALAState(x32.astype(np.float64), logp.cpu().numpy(), grad.cpu().numpy().astype(np.float64))
    key = prng.PRNGKey(31)
    so, s0 = {}, {}
    new, info = flow.rwmh_step(prng.split(key, B), st, vg, model, params, args, so)
    flow.rwmh_step(prng.split(key, B), st, vg0, model0, params, args, s0)
    acc = torch.empty(B, device="cuda"); isacc = torch.empty(B, dtype=torch.uint8, device="cuda")
    prop = torch.empty(B, d, device="cuda"); ns = torch.empty(B, dtype=torch.int32, device="cuda")
    ctx.flow_step(_lib.FLOW_RWMH, key, beta, pos, logp, grad, acc, isacc, prop, ns)
    e_p = np.abs(prop.cpu().numpy() - info.proposed_position).max()
    assert e_p < 3e-5 * max(1.0, np.abs(info.proposed_position).max())
    with np.errstate(divide="ignore"):
        la_g = np.log(acc.cpu().numpy().astype(np.float64))
    fin = np.isfinite(la_g) & (so["log_alpha"] > -80)
    dla, dla0 = np.abs(la_g - so["log_alpha"])[fin], np.abs(la_g - s0["log_alpha"])[fin]
    print(f"rk4 flow step {bc}: |dx'| {e_p:.1e}, |d log alpha| median {np.median(dla):.1e}, vs Dirichlet 0 median {np.median(dla0):.1e}")
    assert fin.sum() >= B // 2 and np.median(dla) < 5e-3 and np.median(dla0) >= 10 * 5e-3
    np.testing.assert_array_equal(ns.cpu().numpy(), 2 * steps)
    ctx.close()


def test_loop_with_a_periodic_lattice_matches_the_oracle_loop():
    """exe_flow_matching.run on a periodic d = 64 lattice against oracle.loop.run with the restated target (as test_gpu_hmc.py's loop
    test): losses before the first flow step, all losses loosely, the chains at the end; and the losses are not Dirichlet 0's."""
    from mfm_amd import distributions as D, exe_flow_matching as E
    from oracle import loop
    kw = dict(example="phi-four", dim=64, num_chain=64, learning_iter=9, mcmc_per_flow_steps=4.0, hutchs=True, fourier_dim=16, seed=7, eval_iter=1,
              step_size=2e-4, hidden_x=[32, 32], hidden_t=[32, 32], hidden_xt=[32, 32])
    out = loop.run(PhiFourBC(64, bc=("pbc", 0.0)), loop.default_args(**kw))
    res, res_, ex = E.run(D.PhiFour(64, bc=("pbc", 0)), loop.default_args(**kw), None, log_every=1000, return_extras=True)
    lg, lo = ex["metrics"][:, 0], np.asarray(out["trace"]["loss"])
    np.testing.assert_allclose(lg[:4], lo[:4], rtol=2e-5)            # before the first flow step: MALA moves + training only
    np.testing.assert_allclose(lg, lo, rtol=5e-2)
    pg, po = ex["states"].position.cpu().numpy().astype(np.float64), out["states"].position
    close = np.abs(pg - po).max(1) < 1e-3
    assert close.mean() > 0.6, close.mean()
    assert np.abs(pg.mean(0) - po.mean(0)).max() < 0.05 and np.abs((pg ** 2).mean(0) - (po ** 2).mean(0)).max() < 0.05
    ex["engine"].close()
    _, _, ex0 = E.run(D.PhiFour(64), loop.default_args(**kw), None, log_every=1000, return_extras=True)
    l0 = ex0["metrics"][:4, 0]
    assert (np.abs(lg[:4] - l0) / (2e-5 * np.abs(l0))).max() >= 10.0, (lg[:4], l0)
    ex0["engine"].close()
