"""Oracle parity of the row kernels (one wave per chain, lane l owns elements l + 64 it) on the dispatch instances above d = 256, which
no other test executes: ``mala_init_kernel``, ``loglik_kernel``, ``mala_step_kernel`` (mala.hip) and ``hmc_step_kernel`` (hmc.hip) as
MAXIT 16 and 32, BCRT false and true, each at its first and last dimension (tests/row_instance_cases.py has the table, the start states
and the step sizes; d = 65 is the first dimension of MAXIT 4), and the size limit d = 2049 of every entry point that dispatches them.

Every comparison is with the float64 oracle (oracle/mala.py, oracle/hmc.py on tests/phi4_bc_oracle.py / tests/phi4_2d_oracle.py) on the
same keys, 16 chains, 3 steps, restarted at every step from the device's state so that both sides continue from the kernel's
decisions, at the tolerances the project states for these quantities:

* init / loglik: tests/test_gpu_mala.py::test_mala_init_and_step_match_oracle (log-density rtol 2e-6 atol 1e-3, gradient rtol 2e-5
  atol 2e-3);
* MALA step: the same test and tests/test_gpu_phi4_bc.py / test_gpu_phi4_2d.py::test_mala_init_step_loglik (proposal 1e-6,
  acceptance probability 5e-3, decisions equal outside |u - p| <= 1e-2, position 1e-6, log-density rtol 2e-6 atol 2e-3, gradient
  rtol 3e-5 atol 3e-3), the proposal weight as tests/test_gpu_mala_api.py::_check_step (log within 5e-2 where representable);
* HMC step: tests/test_gpu_hmc.py / tests/test_gpu_hmc_run.py::_oracle_step_check (log acceptance probability 5e-6 max(1, |log pi|)
  + 1e-5, decisions equal outside 10 tol p + 1e-6, position 3e-6 max(1, |x|), log-density 2e-6 max(1, |log pi|)); those tests state
  no tolerance for the gradient after a step, which takes the MALA step's form.  The two energy forms scale with |log pi|, which
  near a mode is as small as 0.5 (periodic start states) while the energies' float32 content does not shrink with it: the end
  point is a float32 row, and rounding it moves log pi by sum_j g_j dx_j whatever |log pi| is.  A numpy restatement of the step with
  the device's number formats (``row_instance_cases.hmc_step_f32``: float32 positions after every drift, float32 gradient arithmetic,
  float64 momentum and energies) differs from the float64 oracle on the same inputs by up to 1.8e-4 in the log acceptance
  probability and 2.2e-4 in the end point's log-density (d = 2048; 1.2e-5 at d = 65; ``HMC_F32_DISTANCE`` has every case), against
  forms of 1.5e-5 and 2e-6 at |log pi| < 1.  So each of the two takes the LARGER of its stated form and 4 x the case's restatement
  distance (factor 4: the ratio of stated tolerance to measured distance of docs/HISTORY.md section 2).  The borderline band keeps
  the stated form.

Gradients and positions are compared element by element; a failure names (chain, element, it = j // 64, lane = j % 64), and the seam
set (both sides of every 64-element seam, the row's ends, the lattice's first and last row and column) is asserted on its own, since
a stencil that drops a neighbour at a seam is wrong only there.  At most 1 of 16 chains per step may lie in the borderline band, and
the device must take both decisions within the three steps (tests/test_row_instance_cases.py asserts the same of the oracle alone).
Every test prints the largest error of each quantity in units of its tolerance."""
import functools

import numpy as np
import pytest

from oracle import mala as omala
from tests import row_instance_cases as rc
from tests.mcmc_bits_cases import VARIANTS

pytestmark = pytest.mark.gpu

B = rc.N_CHAINS


def _dev(x, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def _keys_dev(keys):
    import torch
    return torch.as_tensor(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32)).cuda()


@functools.lru_cache(maxsize=None)
def _setup(d):
    from tests import gpu_util as gu
    args, dist0, *_ = gu.phi4_setup(d=d, B=B, hidden=32, F=16)
    assert (dist0.a, dist0.beta) == (rc.A, rc.TBETA)
    return args, dist0


def _ctx(case):
    """A 16-chain context on the case's target (network: hidden 32, F = 16, kernel family AUTO) and its start state on the device."""
    from mfm_amd import _lib
    from tests import gpu_util as gu
    d, L, bc, n_total, off = rc.CASES[case]
    args, dist0 = _setup(d)
    ctx = gu.make_ctx(dist0, args, n_local=B, n_total=n_total, offset=off)
    if rc.block(case) is not None:
        ctx.set_target(_lib.PHI4, rc.block(case))
    return ctx, _dev(rc.start_state(case))


def _state(ctx, pos, beta):
    import torch
    logp = torch.empty(B, dtype=torch.float64, device="cuda"); grad = torch.empty_like(pos)
    ctx.mala_init(pos, beta, logp, grad)
    return logp, grad


def _rows(tag, case, got, want, rtol, atol):
    """got ~ want element by element within atol + rtol |want|, on the seam set and on every element; the largest error / tolerance."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    ratio = np.abs(got - want) / (atol + rtol * np.abs(want))
    worst = {}
    for name, cols in (("seam set", rc.seam_set(case)), ("all elements", np.arange(got.shape[1]))):
        r = ratio[:, cols]
        b, k = np.unravel_index(np.argmax(r), r.shape)
        j = cols[k]
        worst[name] = r[b, k]
        assert r[b, k] <= 1.0, (f"{tag} [{name}]: chain {b}, {rc.where(j)}: got {got[b, j]!r}, oracle {want[b, j]!r}, "
                                f"|error| {abs(got[b, j] - want[b, j]):.3g} = {r[b, k]:.3g} tolerances")
    return worst["all elements"]


def _vec(tag, got, want, rtol, atol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    ratio = np.abs(got - want) / (atol + rtol * np.abs(want))
    b = int(np.argmax(ratio))
    assert ratio[b] <= 1.0, f"{tag}: chain {b}: got {got[b]!r}, oracle {want[b]!r} = {ratio[b]:.3g} tolerances"
    return ratio[b]


def _report(case, what, worst):
    d = rc.CASES[case][0]
    print(f"\nROW {case} {what} d={d} MAXIT={rc.maxit(d)} BCRT={int(rc.bcrt(case))} " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", list(rc.CASES))
def test_init_and_loglik_match_oracle(case, variant):
    import torch
    beta = VARIANTS[variant][0]
    ctx, pos = _ctx(case)
    x64 = rc.start_state(case).astype(np.float64)
    st = omala.init(x64, rc.value_and_grad(case, variant))
    logp, grad = _state(ctx, pos, beta)
    worst = {"scale": np.abs(st.logdensity).max()}
    worst["logp"] = _vec("init log-density", logp.cpu().numpy(), st.logdensity, 2e-6, 1e-3)
    worst["grad"] = _rows("init gradient", case, grad.cpu().numpy(), st.logdensity_grad, 2e-5, 2e-3)
    ll = torch.empty(B, dtype=torch.float64, device="cuda")
    ctx.loglik(pos, ll)
    worst["loglik"] = _vec("loglik", ll.cpu().numpy(), rc.oracle_dist(case).loglik(x64), 2e-6, 1e-3)
    np.testing.assert_array_equal(pos.cpu().numpy(), rc.start_state(case))     # neither kernel writes the positions
    _report(case, f"init/{variant}", worst)
    ctx.close()


def _merge(worst, **kw):
    for k, v in kw.items():
        worst[k] = max(worst.get(k, 0.0), float(v))


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", list(rc.CASES))
def test_mala_step_and_step_keys_match_oracle(case, variant):
    """``mfm_mala_step`` on the step's key and ``mfm_mala_step_keys`` on the per-chain keys it derives: bit-identical to each other, and
    against the oracle step from the same state."""
    import torch
    beta, textbook = VARIANTS[variant]
    eps = rc.STEP_SIZES[case]["mala"][variant]
    d = rc.CASES[case][0]
    ctx, pos = _ctx(case)
    vg = rc.value_and_grad(case, variant)
    logp, grad = _state(ctx, pos, beta)
    names = ("pos", "logp", "grad", "acc", "isacc", "prop", "w")
    info = lambda: (torch.empty(B, device="cuda"), torch.empty(B, dtype=torch.uint8, device="cuda"), torch.empty(B, d, device="cuda"),
                    torch.empty(B, device="cuda"))
    seen, worst = set(), {}
    for j in range(rc.N_STEPS):
        key, keys = rc.step_keys(case, j, "mala")
        x0, lp0, g0 = pos.cpu().numpy().astype(np.float64), logp.cpu().numpy(), grad.cpu().numpy().astype(np.float64)
        st = omala.MALAState(x0, lp0, g0)
        new, o, u = rc.oracle_step("mala", variant, st, vg, keys, eps)
        by_keys = (pos.clone(), logp.clone(), grad.clone()) + info()
        ctx.mala_step_keys(_keys_dev(keys), beta, eps, *by_keys, textbook=textbook)
        acc, isacc, prop, w = info()
        ctx.mala_step(key, beta, eps, pos, logp, grad, acc, isacc, prop, w, textbook=textbook)
        for name, a, b in zip(names, (pos, logp, grad, acc, isacc, prop, w), by_keys):
            np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy(), err_msg=f"step {j}: mala_step vs mala_step_keys, {name}")
        ia_g = isacc.cpu().numpy().astype(bool)
        _merge(worst, scale=np.abs(lp0).max(),
               prop=_rows(f"step {j} proposal", case, prop.cpu().numpy(), o.proposed_position, 1e-6, 1e-6),
               p=_vec(f"step {j} acceptance probability", acc.cpu().numpy(), o.acceptance_rate, 5e-3, 5e-3))
        w_g, w_o = w.cpu().numpy().astype(np.float64), o.proposed_weight
        fin = np.isfinite(w_o) & (w_o > 1e-30) & (w_o < 1e30)
        if fin.any():
            _merge(worst, weight=_vec(f"step {j} log proposal weight", np.log(w_g[fin]), np.log(w_o[fin]), 0.0, 5e-2))
        border = rc.borderline("mala", st, o, u)
        assert border.sum() <= 1, (j, int(border.sum()))
        np.testing.assert_array_equal(ia_g[~border], o.is_accepted[~border], err_msg=f"step {j} decisions")
        seen |= set(ia_g.tolist())
        # the oracle's state on the KERNEL's branch: a rejected chain keeps its state to the bit
        lpn, gn = vg(o.proposed_position)
        m = ia_g[:, None]
        np.testing.assert_array_equal(pos.cpu().numpy()[~ia_g], x0[~ia_g].astype(np.float32))
        np.testing.assert_array_equal(logp.cpu().numpy()[~ia_g], lp0[~ia_g])
        np.testing.assert_array_equal(grad.cpu().numpy()[~ia_g], g0[~ia_g].astype(np.float32))
        _merge(worst, x=_rows(f"step {j} position", case, pos.cpu().numpy(), np.where(m, o.proposed_position, x0), 1e-6, 1e-6),
               logp=_vec(f"step {j} log-density", logp.cpu().numpy(), np.where(ia_g, lpn, lp0), 2e-6, 2e-3),
               grad=_rows(f"step {j} gradient", case, grad.cpu().numpy(), np.where(m, gn, g0), 3e-5, 3e-3))
    assert seen == {True, False}, seen
    _report(case, f"mala/{variant}", worst)
    ctx.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case", list(rc.CASES))
def test_hmc_step_and_step_keys_match_oracle(case, variant):
    """``mfm_hmc_step`` and ``mfm_hmc_step_keys`` (3 leapfrog steps): bit-identical to each other, and against the oracle step."""
    import torch
    beta = VARIANTS[variant][0]
    eps = rc.STEP_SIZES[case]["hmc"][variant]
    ctx, pos = _ctx(case)
    vg = rc.value_and_grad(case, variant)
    logp, grad = _state(ctx, pos, beta)
    info = lambda: (torch.empty(B, device="cuda"), torch.empty(B, dtype=torch.uint8, device="cuda"))
    seen, worst = set(), {}
    for j in range(rc.N_STEPS):
        key, keys = rc.step_keys(case, j, "hmc")
        x0, lp0, g0 = pos.cpu().numpy().astype(np.float64), logp.cpu().numpy(), grad.cpu().numpy().astype(np.float64)
        st = omala.MALAState(x0, lp0, g0)
        new, o, u = rc.oracle_step("hmc", variant, st, vg, keys, eps)
        by_keys = (pos.clone(), logp.clone(), grad.clone()) + info()
        ctx.hmc_step_keys(_keys_dev(keys), beta, eps, rc.HMC_LEAPFROG, *by_keys)
        acc, isacc = info()
        ctx.hmc_step(key, beta, eps, rc.HMC_LEAPFROG, pos, logp, grad, acc, isacc)
        for name, a, b in zip(("pos", "logp", "grad", "acc", "isacc"), (pos, logp, grad, acc, isacc), by_keys):
            np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy(), err_msg=f"step {j}: hmc_step vs hmc_step_keys, {name}")
        ia_g, pa_g = isacc.cpu().numpy().astype(bool), acc.cpu().numpy().astype(np.float64)
        tol = 5e-6 * max(1.0, np.abs(lp0).max())
        f32_p, f32_lp = (4 * v for v in rc.HMC_F32_DISTANCE[case][variant])
        _merge(worst, scale=np.abs(lp0).max(),
               p=_vec(f"step {j} log acceptance probability", np.log(np.maximum(pa_g, 1e-30)), np.log(np.maximum(o.acceptance_rate, 1e-30)), 0.0,
                      max(tol + 1e-5, f32_p)))
        border = rc.borderline("hmc", st, o, u)
        assert border.sum() <= 1, (j, int(border.sum()))
        np.testing.assert_array_equal(ia_g[~border], o.is_accepted[~border], err_msg=f"step {j} decisions")
        seen |= set(ia_g.tolist())
        lpn, gn = vg(o.proposed_position)
        m = ia_g[:, None]
        ref_x, ref_lp, ref_g = np.where(m, o.proposed_position, x0), np.where(ia_g, lpn, lp0), np.where(m, gn, g0)
        np.testing.assert_array_equal(pos.cpu().numpy()[~ia_g], x0[~ia_g].astype(np.float32))
        np.testing.assert_array_equal(logp.cpu().numpy()[~ia_g], lp0[~ia_g])
        np.testing.assert_array_equal(grad.cpu().numpy()[~ia_g], g0[~ia_g].astype(np.float32))
        _merge(worst, x=_rows(f"step {j} position", case, pos.cpu().numpy(), ref_x, 0.0, 3e-6 * max(1.0, np.abs(ref_x).max())),
               logp=_vec(f"step {j} log-density", logp.cpu().numpy(), ref_lp, 0.0, max(2e-6 * max(1.0, np.abs(ref_lp).max()), f32_lp)),
               grad=_rows(f"step {j} gradient", case, grad.cpu().numpy(), ref_g, 3e-5, 3e-3))
    assert seen == {True, False}, seen
    _report(case, f"hmc/{variant}", worst)
    ctx.close()


def test_dimension_2049_is_refused_by_every_entry_point_and_touches_nothing():
    """nit = ceil(2049 / 64) = 33 > 32: MALA_DISPATCH launches nothing and the entry point raises MFM_ETOOLARGE naming the dimension and
    the kernel; the state and every output buffer keep their bits and the step counters do not move.  (d = 2048 succeeds: the cases above.)"""
    import torch
    from mfm_amd import _lib
    from oracle import prng
    from tests import gpu_util as gu
    d = 2049
    args, dist0 = _setup(d)
    ctx = gu.make_ctx(dist0, args)
    rng = np.random.default_rng(0)
    pos, grad = _dev(rng.standard_normal((B, d)).astype(np.float32)), _dev(rng.standard_normal((B, d)).astype(np.float32))
    logp = _dev(rng.standard_normal(B))
    f64 = lambda *s: _dev(rng.standard_normal(s))
    f32 = lambda *s: _dev(rng.standard_normal(s).astype(np.float32))
    bufs = dict(pos=pos, logp=logp, grad=grad, acc=f32(B), isacc=_dev(rng.integers(0, 2, B).astype(np.uint8)), prop=f32(B, d), w=f32(B),
                out=f64(B), n_acc=_dev(rng.integers(0, 9, B).astype(np.int32)), acc_sum=f64(B), traj_pos=f32(2, B, d), traj_logp=f64(2, B),
                avg=f64(B), last=f64(B), traj=f64(2, B))
    before = {k: v.clone() for k, v in bufs.items()}
    counters = ctx.counters()
    key, keys = prng.PRNGKey(1), _keys_dev(prng.split(prng.PRNGKey(2), B))
    b = bufs
    run_out = dict(thin=1, n_acc=b["n_acc"], acc_sum=b["acc_sum"], acc=b["acc"], is_acc=b["isacc"], traj_pos=b["traj_pos"], traj_logp=b["traj_logp"])
    warm_out = dict(step_last=b["last"], n_acc=b["n_acc"], acc_sum=b["acc_sum"], step_traj=b["traj"])
    calls = {
        "mfm_mala_init": ("MALA", lambda: ctx.mala_init(pos, 1.0, logp, grad)),
        "mfm_loglik": ("loglik", lambda: ctx.loglik(pos, b["out"])),
        "mfm_mala_step": ("MALA", lambda: ctx.mala_step(key, 1.0, 1e-5, pos, logp, grad, b["acc"], b["isacc"], b["prop"], b["w"])),
        "mfm_mala_step_keys": ("MALA", lambda: ctx.mala_step_keys(keys, 1.0, 1e-5, pos, logp, grad, b["acc"], b["isacc"], b["prop"], b["w"])),
        "mfm_hmc_step": ("HMC", lambda: ctx.hmc_step(key, 1.0, 1e-3, 3, pos, logp, grad, b["acc"], b["isacc"])),
        "mfm_hmc_step_keys": ("HMC", lambda: ctx.hmc_step_keys(keys, 1.0, 1e-3, 3, pos, logp, grad, b["acc"], b["isacc"])),
        "mfm_mala_run": ("MALA", lambda: ctx.mala_run(key, 1.0, 1e-5, 2, pos, logp, grad, proposed=b["prop"], weight=b["w"], **run_out)),
        "mfm_mala_run (chain-major)": ("MALA", lambda: ctx.mala_run(keys, 1.0, 1e-5, 2, pos, logp, grad, **run_out)),
        "mfm_hmc_run": ("HMC", lambda: ctx.hmc_run(key, 1.0, 1e-3, 3, 2, pos, logp, grad, **run_out)),
        "mfm_hmc_run (chain-major)": ("HMC", lambda: ctx.hmc_run(keys, 1.0, 1e-3, 3, 2, pos, logp, grad, **run_out)),
        "mfm_mala_warmup": ("MALA", lambda: ctx.mala_warmup(key, 1.0, 1e-5, 2, 0.574, pos, logp, grad, b["avg"], **warm_out)),
        "mfm_hmc_warmup": ("HMC", lambda: ctx.hmc_warmup(key, 1.0, 1e-3, 3, 2, 0.8, pos, logp, grad, b["avg"], **warm_out)),
    }
    for blk in (None, [rc.A, rc.TBETA, 1.0, 0.0]):             # the Dirichlet-0 instances, then the run-time-boundary ones
        if blk is not None:
            ctx.set_target(_lib.PHI4, blk)
        for name, (kernel, call) in calls.items():
            with pytest.raises(_lib.MfmError, match=f"dim 2049 too large for the {kernel} kernel"):
                call()
            ctx.sync()
            for k, v in bufs.items():
                assert torch.equal(v, before[k]), (name, k)
    assert ctx.counters() == counters
    ctx.close()
