"""GPU parity of phi-four on an L x L lattice (dim_phys = 2) against the restated oracle (tests/phi4_2d_oracle.py): the cases of
tests/test_gpu_phi4_bc.py on the same keys and AT THE TOLERANCES THAT FILE STATES, for Dirichlet 0, Dirichlet 0.7 and periodic
boundaries, on L = 16 (d = 256, the headline tile), L = 8 (d = 64, padded to the 128 tile) and L = 6 (d = 36, generic tile / wide
family).  Every value, gradient and solver comparison also requires the device to MISS the one-dimensional oracle of the same d
and boundary by at least 10x its tolerance, so a build that ignores dim_phys fails.  The block {a, beta, kind, b, 1} must give
exactly what {a, beta, kind, b} gives."""
import numpy as np
import pytest

from oracle import flow, mala, ode, prng, targets
from tests.phi4_2d_oracle import PhiFour2D
from tests.phi4_bc_oracle import PhiFourBC

pytestmark = pytest.mark.gpu

BCS = [("dirichlet", 0.0), ("dirichlet", 0.7), ("pbc", 0.0)]


def _dev(x, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def _close_and_sensitive(tag, got, want, want_1d, rtol, atol, reduce=np.max):
    """got ~ want within rtol / atol, and got misses want_1d (the chain of the same d and boundary) by >= 10x that tolerance somewhere."""
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=tag)
    miss = np.abs(got - want_1d) / (atol + rtol * np.abs(want_1d))
    assert reduce(miss) >= 10.0, (tag, "indistinguishable from the one-dimensional chain", reduce(miss))


def _with_dist(model, dist):
    m = type(model).__new__(type(model)); m.__dict__.update(model.__dict__); m.dist = dist
    return m


def _setup(d, B, bc, hidden=128, F=128):
    """args, the lattice, the chain of the same d and boundary, and the oracle field of each."""
    from tests import gpu_util as gu
    args, dist0, k, model0, state = gu.phi4_setup(d=d, B=B, hidden=hidden, F=F)
    dist, dist1 = PhiFour2D(d, dist0.a, dist0.beta, bc), PhiFourBC(d, dist0.a, dist0.beta, bc)
    dist.init_params = dist1.init_params = dist0.init_params
    return args, dist, dist1, _with_dist(model0, dist), _with_dist(model0, dist1)


def _ctx(dist, args, **kw):
    from mfm_amd import _lib
    from tests import gpu_util as gu
    ctx = gu.make_ctx(dist, args, **kw)
    ctx.set_target(_lib.PHI4, dist.block())
    return ctx


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("d", [36, 64, 256])
def test_mala_init_step_loglik(d, bc):
    import torch
    B, eps, beta = 64, 1e-4, 0.37
    args, dist, dist1, model, model1 = _setup(d, B, bc, hidden=32, F=16)
    ctx = _ctx(dist, args)
    x32 = dist.init_params.astype(np.float32)
    x64 = x32.astype(np.float64)
    vg, vg1 = targets.Tempered(dist, beta).value_and_grad, targets.Tempered(dist1, beta).value_and_grad
    st, st1 = mala.init(x64, vg), mala.init(x64, vg1)
    pos, logp, grad = _dev(x32), torch.empty(B, dtype=torch.float64, device="cuda"), torch.empty(B, d, device="cuda")
    ctx.mala_init(pos, beta, logp, grad)
    _close_and_sensitive("init logp", logp.cpu().numpy(), st.logdensity, st1.logdensity, 2e-6, 1e-3)
    _close_and_sensitive("init grad", grad.cpu().numpy(), st.logdensity_grad, st1.logdensity_grad, 2e-5, 2e-3)
    ll = torch.empty(B, dtype=torch.float64, device="cuda")
    ctx.loglik(pos, ll)
    _close_and_sensitive("loglik", ll.cpu().numpy(), dist.loglik(x64), dist1.loglik(x64), 2e-6, 1e-3)
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
    _close_and_sensitive("step grad", g_new, new.logdensity_grad[same], dist1.grad_logprob(new.position[same]) * beta, 3e-5, 3e-3)
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


# (d, hidden, F, family, generic, hutch): the shape-specialised solver at L = 16 and at L = 8 (zero-padded to its 128 tile), the generic
# tile at L = 6 and (forced) at L = 8, the wide family with Hutchinson at L = 8 and L = 6 and with the EXACT trace at L = 8 and L = 6
SHAPES = [(256, 128, 128, None, False, True), (64, 128, 128, None, False, True), (36, 32, 16, None, True, True), (64, 32, 16, None, True, True),
          (64, 48, 16, "wide", False, True), (36, 48, 16, "wide", False, True), (64, 48, 16, "wide", False, False), (36, 48, 16, "wide", False, False)]


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("d,hidden,F,fam,generic,hutch", SHAPES)
def test_transform_on_prescribed_steps(monkeypatch, d, hidden, F, fam, generic, hutch, bc):
    import torch
    from mfm_amd import _lib
    from tests import gpu_util as gu
    if generic:
        monkeypatch.setenv("MFM_GENERIC_ODE", "1")
    B = 32
    args, dist0, k, model0, state = gu.phi4_setup(d=d, B=B, hidden=hidden, F=F, hutch=hutch)
    dist, dist1 = PhiFour2D(d, dist0.a, dist0.beta, bc), PhiFourBC(d, dist0.a, dist0.beta, bc)
    dist.init_params = dist0.init_params
    m_2d, m_1d = _with_dist(model0, dist), _with_dist(model0, dist1)      # the oracle's model evaluates grad log pi of ITS dist
    params = _tamed(model0)
    ctx = _ctx(dist, args, fourier=model0.f, params=params, **(dict(family=_lib.FAMILY_WIDE) if fam else {}))
    x64 = dist.init_params.astype(np.float32).astype(np.float64)
    keys = prng.split(prng.PRNGKey(21), B)
    o = (hutch, args.rtol, args.atol, args.mxstep)
    st = {}
    ode.transform_and_logdet(m_2d, params, keys, x64, *o, stats=st)
    dt, acc = _replay_arrays([st])
    rp = dict(dt=dt[0].astype(np.float64), acc=acc[0])
    y_o, l_o = ode.transform_and_logdet(m_2d, params, keys, x64, *o, stats={}, replay=rp)
    y_1, l_1 = ode.transform_and_logdet(m_1d, params, keys, x64, *o, stats={}, replay=rp)     # the chain, same steps
    ratio = torch.zeros(dt[0].shape, device="cuda"); own = torch.zeros(dt[0].shape, device="cuda")
    ctx.debug_replay(_dev(dt[0]), _dev(acc[0]), ratio, own)
    out = torch.empty(B, d, device="cuda"); ldj = torch.empty(B, device="cuda"); ns = torch.empty(B, dtype=torch.int32, device="cuda")
    ctx.ode_transform(1, _dev(x64.astype(np.float32)), out, ldj, keys=_dev(keys.astype(np.uint32).view(np.int32)), nsteps=ns)
    y, l, n = out.cpu().numpy(), ldj.cpu().numpy(), ns.cpu().numpy()
    np.testing.assert_array_equal(n, st["n_attempted"])
    ys, ls = max(1.0, np.abs(y_o).max()), max(1.0, np.abs(l_o).max())
    ey, el = np.abs(y - y_o).max(), np.abs(l - l_o)
    tag = f"transform {bc} d={d} {fam or ('generic' if generic else 'fast')} hutch={hutch}"
    miss = max(np.abs(y - y_1).max() / (3e-5 * ys), np.quantile(np.abs(l - l_1), 0.9) / (2e-5 * ls))
    print(f"{tag}: |dy| {ey:.1e} (tol {3e-5 * ys:.1e}), |dl| q90 {np.quantile(el, 0.9):.1e} max {el.max():.1e} (scale {ls:.2g}), miss vs the chain: {miss:.0f}x tol")
    assert ey < 3e-5 * ys, ey
    assert np.quantile(el, 0.9) < 2e-5 * ls and el.max() < 2e-3 * ls, (np.quantile(el, 0.9), el.max(), ls)
    assert miss >= 10.0, miss
    ctx.close()


FLOW_SHAPES = [(256, 128, 128, None, False), (64, 128, 128, None, False), (36, 32, 16, None, True), (256, 128, 128, "wide", False),
               (36, 48, 16, "wide", False)]


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("d,hidden,F,fam,generic", FLOW_SHAPES)
def test_flow_step_on_prescribed_steps(monkeypatch, d, hidden, F, fam, generic, bc):
    import torch
    from mfm_amd import _lib
    monkeypatch.setenv("MFM_FLOW_LIVE", "16")
    if generic:
        monkeypatch.setenv("MFM_GENERIC_ODE", "1")
    B, beta = 32, 0.8
    args, dist, dist1, m_2d, m_1d = _setup(d, B, bc, hidden, F)
    params = _tamed(m_2d, out_scale=2.0)
    ctx = _ctx(dist, args, fourier=m_2d.f, params=params, **(dict(family=_lib.FAMILY_WIDE) if fam else {}))
    x32 = dist.init_params.astype(np.float32)
    vg, vg1 = targets.Tempered(dist, beta).value_and_grad, targets.Tempered(dist1, beta).value_and_grad
    pos = _dev(x32); logp = torch.empty(B, dtype=torch.float64, device="cuda"); grad = torch.empty(B, d, device="cuda")
    ctx.mala_init(pos, beta, logp, grad)
    st0 = mala.MALAState(x32.astype(np.float64), logp.cpu().numpy(), grad.cpu().numpy().astype(np.float64))
    key = prng.PRNGKey(31)
    keys = prng.split(key, B)
    nat = {}
    flow.rwmh_step(keys, st0, vg, m_2d, params, args, nat)
    dt, acc = _replay_arrays([nat["inv"], nat["fwd"]])
    rp = dict(inv=dict(dt=dt[0].astype(np.float64), acc=acc[0]), fwd=dict(dt=dt[1].astype(np.float64), acc=acc[1]))
    so, s1 = {}, {}
    new_o, info_o = flow.rwmh_step(keys, st0, vg, m_2d, params, args, so, replay=rp)
    flow.rwmh_step(keys, st0, vg1, m_1d, params, args, s1, replay=rp)
    ratio = torch.zeros(dt.shape, device="cuda"); own = torch.zeros(dt.shape, device="cuda")
    diag = torch.zeros(B, 4, dtype=torch.float64, device="cuda")
    ctx.debug_replay(_dev(dt), _dev(acc), ratio, own, diag)
    a = torch.empty(B, device="cuda"); isacc = torch.empty(B, dtype=torch.uint8, device="cuda")
    prop = torch.empty(B, d, device="cuda"); ns = torch.empty(B, dtype=torch.int32, device="cuda")
    ctx.flow_step(_lib.FLOW_RWMH, key, beta, pos, logp, grad, a, isacc, prop, ns)
    dg = diag.cpu().numpy()
    np.testing.assert_array_equal(ns.cpu().numpy(), so["n_att_inv"] + so["n_att_fwd"])
    e_p = np.abs(prop.cpu().numpy() - info_o.proposed_position).max()
    e_la = np.abs(dg[:, 3] - so["log_alpha"])
    miss = np.median(np.abs(dg[:, 3] - s1["log_alpha"])) / 5e-3
    print(f"flow step {bc} d={d} {fam or ('generic' if generic else 'fast')}: |dx'| {e_p:.1e}, |d log alpha| median {np.median(e_la):.1e} max {e_la.max():.1e}, "
          f"miss vs the chain: {miss:.0f}x tol")
    assert e_p < 3e-5 * max(1.0, np.abs(info_o.proposed_position).max()), e_p
    vs = max(1.0, np.abs(so["vol0"]).max(), np.abs(so["volp"]).max())
    for e in (np.abs(dg[:, 0] - so["vol0"]), np.abs(dg[:, 1] - so["volp"])):
        assert np.quantile(e, 0.9) < 2e-5 * vs and e.max() < 2e-3 * vs, (np.quantile(e, 0.9), e.max(), vs)
    assert np.median(e_la) < 5e-3 and e_la.max() < 5e-2, (np.median(e_la), e_la.max())
    assert miss >= 10.0, miss
    sure = np.abs(so["log_alpha"] - np.log(np.maximum(prng.uniform_rows(prng.split_rows(keys, 4)[:, 1]), 1e-300))) > 0.1
    np.testing.assert_array_equal(isacc.cpu().numpy().astype(bool)[sure], info_o.is_accepted[sure])
    same = isacc.cpu().numpy().astype(bool) == info_o.is_accepted
    np.testing.assert_allclose(pos.cpu().numpy()[same], new_o.position[same], atol=3e-5 * max(1.0, np.abs(new_o.position).max()))
    np.testing.assert_allclose(logp.cpu().numpy()[same], new_o.logdensity[same], rtol=2e-6, atol=2e-3)
    ctx.close()


@pytest.mark.parametrize("bc", BCS)
def test_dim_phys_one_block_is_bit_identical(bc):
    """{a, beta, kind, b, 1} selects exactly the results of {a, beta, kind, b}: fm_loss_grad, MALA step and flow step at d = 256."""
    import torch
    from mfm_amd import _lib
    from tests import gpu_util as gu
    B, d, beta = 64, 256, 0.6
    args, dist0, k, model, state = gu.phi4_setup(d=d, B=B)
    params = _tamed(model, out_scale=2.0)
    blk4 = PhiFourBC(d, dist0.a, dist0.beta, bc).block()
    outs = []
    for blk in (blk4, blk4 + [1.0]):
        ctx = gu.make_ctx(dist0, args, fourier=model.f, params=params)
        ctx.set_target(_lib.PHI4, blk)
        pos = _dev(dist0.init_params.astype(np.float32)); logp = torch.empty(B, dtype=torch.float64, device="cuda")
        grad = torch.empty(B, d, device="cuda")
        loss = torch.zeros(1, dtype=torch.float64, device="cuda"); grads = torch.zeros(ctx.n_params, device="cuda")
        ctx.fm_loss_grad(prng.PRNGKey(7), pos, loss, grads)
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


def test_set_target_accepts_and_rejects_the_five_double_block():
    from mfm_amd import _lib
    from tests import gpu_util as gu
    args, dist0, k, model, state = gu.phi4_setup(d=40, B=16, hidden=32, F=16)
    ctx = gu.make_ctx(dist0, args)
    ctx.set_target(_lib.PHI4, [0.1, 20.0, 1.0, 0.0, 1.0])
    with pytest.raises(_lib.MfmError, match="square"):
        ctx.set_target(_lib.PHI4, [0.1, 20.0, 1.0, 0.0, 2.0])                # d = 40 is no L * L
    for dp in (0.0, 3.0, 1.5):
        with pytest.raises(_lib.MfmError, match="dim_phys"):
            ctx.set_target(_lib.PHI4, [0.1, 20.0, 0.0, 0.0, dp])
    for n in (1, 3, 6):
        with pytest.raises(_lib.MfmError, match="phi4 target takes"):
            ctx.set_target(_lib.PHI4, [0.1, 20.0, 0.0, 0.0, 2.0, 0.0][:n])
    ctx.close()
    args, dist0, k, model, state = gu.phi4_setup(d=36, B=16, hidden=32, F=16)
    ctx = gu.make_ctx(dist0, args)
    ctx.set_target(_lib.PHI4, [0.1, 20.0, 0.0, 0.7, 2.0])
    ctx.close()
