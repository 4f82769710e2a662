"""GPU parity of phi-four with periodic and Dirichlet-1 boundaries against the restated oracle (tests/phi4_bc_oracle.py), on the
same keys and at the tolerances of the existing tests for the same paths (tests/test_gpu_mala.py, tests/test_gpu_replay.py).
Every comparison also requires the device to MISS the Dirichlet-0 oracle by at least 10x its tolerance, so a kernel that ignores
the boundary fails.  The block {a, beta, 0, 0} must give exactly what {a, beta} gives."""
import numpy as np
import pytest

from oracle import flow, mala, ode, prng, targets
from tests.phi4_bc_oracle import PhiFourBC

pytestmark = pytest.mark.gpu

BCS = [("pbc", 0.0), ("dirichlet", 1.0)]


def _dev(x, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def _close_and_sensitive(tag, got, want, want_d0, rtol, atol, reduce=np.max):
    """got ~ want within rtol / atol, and got misses want_d0 by >= 10x that tolerance somewhere."""
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=tag)
    miss = np.abs(got - want_d0) / (atol + rtol * np.abs(want_d0))
    assert reduce(miss) >= 10.0, (tag, "indistinguishable from Dirichlet 0", reduce(miss))


def _setup(d, B, bc, hidden=128, F=128):
    from tests import gpu_util as gu
    args, dist0, k, model, state = gu.phi4_setup(d=d, B=B, hidden=hidden, F=F)
    dist = PhiFourBC(d, dist0.a, dist0.beta, bc)
    dist.init_params = dist0.init_params
    return args, dist, dist0, model


def _ctx(dist, args, **kw):
    from mfm_amd import _lib
    from tests import gpu_util as gu
    ctx = gu.make_ctx(dist, args, **kw)
    ctx.set_target(_lib.PHI4, dist.block())
    return ctx


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("d", [40, 64, 256])
def test_mala_init_step_loglik(d, bc):
    import torch
    B, eps, beta = 64, 1e-4, 0.37
    args, dist, dist0, model = _setup(d, B, bc, hidden=32, F=16)
    ctx = _ctx(dist, args)
    x32 = dist.init_params.astype(np.float32)
    x64 = x32.astype(np.float64)
    vg, vg0 = targets.Tempered(dist, beta).value_and_grad, targets.Tempered(dist0, beta).value_and_grad
    st, st0 = mala.init(x64, vg), mala.init(x64, vg0)
    pos, logp, grad = _dev(x32), torch.empty(B, dtype=torch.float64, device="cuda"), torch.empty(B, d, device="cuda")
    ctx.mala_init(pos, beta, logp, grad)
    _close_and_sensitive("init logp", logp.cpu().numpy(), st.logdensity, st0.logdensity, 2e-6, 1e-3)
    _close_and_sensitive("init grad", grad.cpu().numpy(), st.logdensity_grad, st0.logdensity_grad, 2e-5, 2e-3)
    ll = torch.empty(B, dtype=torch.float64, device="cuda")
    ctx.loglik(pos, ll)
    _close_and_sensitive("loglik", ll.cpu().numpy(), dist.loglik(x64), dist0.loglik(x64), 2e-6, 1e-3)
    key = prng.PRNGKey(77)
    keys = prng.split(key, B)
    st_in = mala.MALAState(x64, logp.cpu().numpy(), grad.cpu().numpy().astype(np.float64))
    new, info, u = mala.kernel(keys, st_in, vg, eps)
    acc = torch.empty(B, device="cuda"); isacc = torch.empty(B, dtype=torch.uint8, device="cuda")
    prop = torch.empty(B, d, device="cuda"); w = torch.empty(B, device="cuda")
    ctx.mala_step(key, beta, eps, pos, logp, grad, acc, isacc, prop, w)
    np.testing.assert_allclose(prop.cpu().numpy(), info.proposed_position, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(acc.cpu().numpy(), info.acceptance_rate, rtol=5e-3, atol=5e-3)
    decided = np.abs(u - info.acceptance_rate) > 1e-2
    np.testing.assert_array_equal(isacc.cpu().numpy()[decided].astype(bool), info.is_accepted[decided])
    same = isacc.cpu().numpy().astype(bool) == info.is_accepted
    assert same.sum() > B // 2
    np.testing.assert_allclose(pos.cpu().numpy()[same], new.position[same], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(logp.cpu().numpy()[same], new.logdensity[same], rtol=2e-6, atol=2e-3)
    g_new = grad.cpu().numpy()[same]
    _close_and_sensitive("step grad", g_new, new.logdensity_grad[same], dist0.grad_logprob(new.position[same]) * beta, 3e-5, 3e-3)
    ctx.close()


def _tamed(model, out_scale=4.0, seed=9, gate=1e-3):
    from tests import gpu_util as gu
    p = gu.rand_params(model, seed=seed, out_scale=out_scale)
    p[4]["kernel"] *= gate; p[4]["bias"] *= gate
    return p


def _replay_arrays(stats_list):
    A = max(s["acc_seq"].shape[1] for s in stats_list)
    cap = A + 2
    B = stats_list[0]["acc_seq"].shape[0]
    dt = np.zeros((len(stats_list), B, cap), np.float32); acc = np.zeros((len(stats_list), B, cap), np.uint8)
    for s, st in enumerate(stats_list):
        dt[s, :, :st["dt_seq"].shape[1]] = st["dt_seq"].astype(np.float32)
        acc[s, :, :st["acc_seq"].shape[1]] = st["acc_seq"]
    return dt, acc


# (d, hidden, F, family, generic): the shape-specialised solver at 256, 128 and 64 (zero-padded to its 128 tile), the generic tile
# (forced at d = 40: not a multiple of 16), the wide family with Hutchinson
SHAPES = [(256, 128, 128, None, False), (128, 128, 128, None, False), (64, 128, 128, None, False), (40, 32, 16, None, True),
          (64, 48, 16, "wide", False)]


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("d,hidden,F,fam,generic", SHAPES)
def test_transform_on_prescribed_steps(monkeypatch, d, hidden, F, fam, generic, bc):
    import torch
    from mfm_amd import _lib
    if generic:
        monkeypatch.setenv("MFM_GENERIC_ODE", "1")
    B = 32
    args, dist, dist0, model = _setup(d, B, bc, hidden, F)
    params = _tamed(model)
    ctx = _ctx(dist, args, fourier=model.f, params=params, **(dict(family=_lib.FAMILY_WIDE) if fam else {}))
    x64 = dist.init_params.astype(np.float32).astype(np.float64)
    keys = prng.split(prng.PRNGKey(21), B)
    o = (True, args.rtol, args.atol, args.mxstep)
    st = {}
    # the oracle's model evaluates grad log pi of ITS dist: one model per boundary
    m_bc = type(model).__new__(type(model)); m_bc.__dict__.update(model.__dict__); m_bc.dist = dist
    ode.transform_and_logdet(m_bc, params, keys, x64, *o, stats=st)
    dt, acc = _replay_arrays([st])
    rp = dict(dt=dt[0].astype(np.float64), acc=acc[0])
    y_o, l_o = ode.transform_and_logdet(m_bc, params, keys, x64, *o, stats={}, replay=rp)
    y_0, l_0 = ode.transform_and_logdet(model, params, keys, x64, *o, stats={}, replay=rp)     # Dirichlet 0, same steps
    ratio = torch.zeros(dt[0].shape, device="cuda"); own = torch.zeros(dt[0].shape, device="cuda")
    ctx.debug_replay(_dev(dt[0]), _dev(acc[0]), ratio, own)
    out = torch.empty(B, d, device="cuda"); ldj = torch.empty(B, device="cuda"); ns = torch.empty(B, dtype=torch.int32, device="cuda")
    ctx.ode_transform(1, _dev(x64.astype(np.float32)), out, ldj, keys=_dev(keys.astype(np.uint32).view(np.int32)), nsteps=ns)
    y, l, n = out.cpu().numpy(), ldj.cpu().numpy(), ns.cpu().numpy()
    np.testing.assert_array_equal(n, st["n_attempted"])
    ys, ls = max(1.0, np.abs(y_o).max()), max(1.0, np.abs(l_o).max())
    ey, el = np.abs(y - y_o).max(), np.abs(l - l_o)
    assert ey < 3e-5 * ys, ey
    assert np.quantile(el, 0.9) < 2e-5 * ls and el.max() < 2e-3 * ls, (np.quantile(el, 0.9), el.max(), ls)
    miss = max(np.abs(y - y_0).max() / (3e-5 * ys), np.quantile(np.abs(l - l_0), 0.9) / (2e-5 * ls))
    print(f"transform {bc} d={d} {fam or ('generic' if generic else 'fast')}: |dy| {ey:.1e}, |dl| {el.max():.1e}, miss vs Dirichlet 0: {miss:.0f}x tol")
    assert miss >= 10.0, miss
    ctx.close()


FLOW_SHAPES = [(256, 128, 128, None, False), (64, 128, 128, None, False), (40, 32, 16, None, True), (256, 128, 128, "wide", False)]


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("d,hidden,F,fam,generic", FLOW_SHAPES)
def test_flow_step_on_prescribed_steps(monkeypatch, d, hidden, F, fam, generic, bc):
    import torch
    from mfm_amd import _lib
    monkeypatch.setenv("MFM_FLOW_LIVE", "16")
    if generic:
        monkeypatch.setenv("MFM_GENERIC_ODE", "1")
    B, beta = 32, 0.8
    args, dist, dist0, model = _setup(d, B, bc, hidden, F)
    params = _tamed(model, out_scale=2.0)
    ctx = _ctx(dist, args, fourier=model.f, params=params, **(dict(family=_lib.FAMILY_WIDE) if fam else {}))
    m_bc = type(model).__new__(type(model)); m_bc.__dict__.update(model.__dict__); m_bc.dist = dist
    x32 = dist.init_params.astype(np.float32)
    vg, vg0 = targets.Tempered(dist, beta).value_and_grad, targets.Tempered(dist0, beta).value_and_grad
    pos = _dev(x32); logp = torch.empty(B, dtype=torch.float64, device="cuda"); grad = torch.empty(B, d, device="cuda")
    ctx.mala_init(pos, beta, logp, grad)
    st0 = mala.MALAState(x32.astype(np.float64), logp.cpu().numpy(), grad.cpu().numpy().astype(np.float64))
    key = prng.PRNGKey(31)
    keys = prng.split(key, B)
    nat = {}
    flow.rwmh_step(keys, st0, vg, m_bc, params, args, nat)
    dt, acc = _replay_arrays([nat["inv"], nat["fwd"]])
    rp = dict(inv=dict(dt=dt[0].astype(np.float64), acc=acc[0]), fwd=dict(dt=dt[1].astype(np.float64), acc=acc[1]))
    so, s0 = {}, {}
    new_o, info_o = flow.rwmh_step(keys, st0, vg, m_bc, params, args, so, replay=rp)
    flow.rwmh_step(keys, st0, vg0, model, params, args, s0, replay=rp)
    ratio = torch.zeros(dt.shape, device="cuda"); own = torch.zeros(dt.shape, device="cuda")
    diag = torch.zeros(B, 4, dtype=torch.float64, device="cuda")
    ctx.debug_replay(_dev(dt), _dev(acc), ratio, own, diag)
    a = torch.empty(B, device="cuda"); isacc = torch.empty(B, dtype=torch.uint8, device="cuda")
    prop = torch.empty(B, d, device="cuda"); ns = torch.empty(B, dtype=torch.int32, device="cuda")
    ctx.flow_step(_lib.FLOW_RWMH, key, beta, pos, logp, grad, a, isacc, prop, ns)
    dg = diag.cpu().numpy()
    np.testing.assert_array_equal(ns.cpu().numpy(), so["n_att_inv"] + so["n_att_fwd"])
    e_p = np.abs(prop.cpu().numpy() - info_o.proposed_position).max()
    assert e_p < 3e-5 * max(1.0, np.abs(info_o.proposed_position).max()), e_p
    vs = max(1.0, np.abs(so["vol0"]).max(), np.abs(so["volp"]).max())
    for e in (np.abs(dg[:, 0] - so["vol0"]), np.abs(dg[:, 1] - so["volp"])):
        assert np.quantile(e, 0.9) < 2e-5 * vs and e.max() < 2e-3 * vs, (np.quantile(e, 0.9), e.max(), vs)
    e_la = np.abs(dg[:, 3] - so["log_alpha"])
    assert np.median(e_la) < 5e-3 and e_la.max() < 5e-2, (np.median(e_la), e_la.max())
    miss = np.median(np.abs(dg[:, 3] - s0["log_alpha"])) / 5e-3
    print(f"flow step {bc} d={d} {fam or ('generic' if generic else 'fast')}: |dx'| {e_p:.1e}, |d log alpha| max {e_la.max():.1e}, miss vs Dirichlet 0: {miss:.0f}x tol")
    assert miss >= 10.0, miss
    sure = np.abs(so["log_alpha"] - np.log(np.maximum(prng.uniform_rows(prng.split_rows(keys, 4)[:, 1]), 1e-300))) > 0.1
    np.testing.assert_array_equal(isacc.cpu().numpy().astype(bool)[sure], info_o.is_accepted[sure])
    same = isacc.cpu().numpy().astype(bool) == info_o.is_accepted
    np.testing.assert_allclose(pos.cpu().numpy()[same], new_o.position[same], atol=3e-5 * max(1.0, np.abs(new_o.position).max()))
    np.testing.assert_allclose(logp.cpu().numpy()[same], new_o.logdensity[same], rtol=2e-6, atol=2e-3)
    ctx.close()


def test_explicit_dirichlet_zero_block_is_bit_identical():
    """{a, beta, 0, 0} selects exactly the default kernels' results: fm_loss_grad, MALA step and flow step at the headline shape d = 256."""
    import torch
    from mfm_amd import _lib
    from tests import gpu_util as gu
    B, d, beta = 64, 256, 0.6
    args, dist0, k, model, state = gu.phi4_setup(d=d, B=B)
    params = _tamed(model, out_scale=2.0)
    outs = []
    for blk in ([dist0.a, dist0.beta], [dist0.a, dist0.beta, 0.0, 0.0]):
        ctx = gu.make_ctx(dist0, args, fourier=model.f, params=params)
        ctx.set_target(_lib.PHI4, blk)
        pos = _dev(dist0.init_params.astype(np.float32)); logp = torch.empty(B, dtype=torch.float64, device="cuda")
        grad = torch.empty(B, d, device="cuda")
        loss = torch.zeros(1, dtype=torch.float64, device="cuda"); grads = torch.zeros(ctx.n_params, device="cuda")
        ctx.fm_loss_grad(prng.PRNGKey(7), pos, loss, grads)                  # the static headline training instance
        r = [loss.cpu().numpy().copy(), grads.cpu().numpy().copy()]
        ctx.mala_init(pos, beta, logp, grad)
        ctx.mala_step(prng.PRNGKey(5), beta, 1e-4, pos, logp, grad)
        r += [pos.cpu().numpy().copy(), logp.cpu().numpy().copy(), grad.cpu().numpy().copy()]
        a = torch.empty(B, device="cuda"); isacc = torch.empty(B, dtype=torch.uint8, device="cuda")
        prop = torch.empty(B, d, device="cuda"); ns = torch.empty(B, dtype=torch.int32, device="cuda")
        ctx.flow_step(_lib.FLOW_RWMH, prng.PRNGKey(6), beta, pos, logp, grad, a, isacc, prop, ns)
        r += [t.cpu().numpy() for t in (pos, logp, grad, a, isacc, prop, ns)]
        outs.append(r)
        ctx.close()
    for u, v in zip(*outs):
        np.testing.assert_array_equal(u, v)
