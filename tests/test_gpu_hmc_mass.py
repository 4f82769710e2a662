"""GPU tests of the diagonal mass matrix of the HMC kernels (``mfm_hmc_set_inverse_mass``, the MASS instances of hmc.hip / hmc_run.hip /
warmup.hip, ``mfm_hmc_warmup_window``) and of the window adaptation built on them (bblackjax/adaptation/window_adaptation.py).

* ONES ARE FREE: with a vector of ones installed every HMC entry point gives the bits it gives with none installed (the mass
  instances against the unit instances), one shape per instance family: the mixture d = 2, phi-four d = 64 / 256 / 272 / 1040
  (MAXIT 1 / 4 / 16 / 32) and the periodic chain at d = 64 and d = 272 (the run-time boundary at MAXIT 1 and 16);``mfm_hmc_warmup_window`` with none installed equals
  ``mfm_hmc_warmup``.  Chain counts are 16 and 32: ``mfm_create`` takes multiples of 16 only, so a chain count that is not a multiple of
  the four chains of a workgroup cannot be built.
* THE STEP against the float64 restatement (tests/hmc_mass_ref.py, pinned to oracle/hmc.py by tests/test_hmc_mass_host.py) with
  ``minv`` log-spaced over [0.25, 4] in a fixed permutation: the cases, step sizes, protocol and tolerances of tests/test_gpu_hmc.py.
* RUN AND WARMUP ARE LOOPS OF THE STEP under a non-trivial ``minv``: a run equals its single-step launches bit for bit; a window
  replays as single steps at the step sizes it used (the protocol of tests/test_gpu_warmup.py), and its sums equal a sequential float64
  loop over the replayed float32 positions, bit for bit.  Step sizes: chosen with the float64 restatement on the same positions and
  keys just below the stability limit of velocity Verlet under this ``minv`` (0.6 to 0.65 of the unit-mass sizes of
  tests/test_gpu_hmc_run.py), so that accepted and rejected steps both occur -- restatement, accepted steps of a 6-step run on the
  step-major / chain-major keys: d = 64 at 0.0572: 167 / 166 of 192, periodic at 0.0572: 87 / 86 of 96, d = 256 at 0.0267: 21 / 21,
  d = 272 at 0.0259: 49 / 56 (Dirichlet and periodic alike), d = 1040 at 0.0133: 16 / 16, the mixture at 0.9: 60 of 96.  From these starts every chain's acceptance
  probability is exactly 0 or 1 at first, so the chains' step sizes part late: the windows run 8 steps where the restatement parts
  by the 8th (mixture: 2nd step; d = 64, also periodic: 8th) and 14 steps above d = 64 (d = 256 and 272: 12th; d = 1040: 13th).
* The errors, the adaptation end to end against the restated driver, ``--adapt_mass``."""
import numpy as np
import pytest

from oracle import mala as omala, prng, targets
from tests import hmc_mass_ref as mr, row_instance_cases as rc, warmup_ref as wr
from tests.test_gpu_hmc_run import L, _assert_run_equals_steps, _ctx, _init, _keys_dev, _run, _stepwise

pytestmark = pytest.mark.gpu

N_STEPS, TARGET = 6, 0.8

# name: (target, d, phi-four block tail or None, chains, unit-mass step size, step size under log_spaced_mass, steps of a window)
FAMILIES = {
    "gmm4": ("gmm", 2, None, 16, 1.8, 0.9, 8),
    "phi4_d64": ("phi4", 64, None, 32, 0.088, 0.0572, 8),
    "phi4_d256": ("phi4", 256, None, 16, 0.0445, 0.0267, 14),
    "phi4_d272": ("phi4", 272, None, 16, 0.0432, 0.0259, 14),
    "phi4_d1040": ("phi4", 1040, None, 16, 0.0221, 0.0133, 14),
    "phi4_d64_pbc": ("phi4", 64, [1.0, 0.0], 16, 0.088, 0.0572, 8),
    "phi4_d272_pbc": ("phi4", 272, [1.0, 0.0], 16, 0.0432, 0.0259, 14),        # the run-time boundary on a MAXIT 16 mass instance
}


def _window(ctx, state0, key, beta, step0, n_steps, target=TARGET, window=True):
    """``hmc_warmup_window`` (or ``hmc_warmup``) on a clone of the state; every output as numpy."""
    import torch
    pos, logp, grad = (t.clone() for t in state0)
    n, d = pos.shape
    f64 = dict(dtype=torch.float64, device="cuda")
    avg, last, acc_sum = torch.empty(n, **f64), torch.empty(n, **f64), torch.empty(n, **f64)
    n_acc = torch.empty(n, dtype=torch.int32, device="cuda")
    tr = torch.empty(n_steps, n, **f64)
    s, q = torch.full((n, d), np.nan, **f64), torch.full((n, d), np.nan, **f64)
    key = _keys_dev(key) if np.ndim(key) == 2 else key
    if window:
        ctx.hmc_warmup_window(key, beta, step0, L, n_steps, target, pos, logp, grad, avg, s, q, step_last=last, n_acc=n_acc, acc_sum=acc_sum, step_traj=tr)
    else:
        ctx.hmc_warmup(key, beta, step0, L, n_steps, target, pos, logp, grad, avg, step_last=last, n_acc=n_acc, acc_sum=acc_sum, step_traj=tr)
    names = ("pos", "logp", "grad", "step_avg", "step_last", "n_acc", "acc_sum", "step_traj", "pos_sum", "pos_sumsq")
    return {k: t.cpu().numpy() for k, t in zip(names, (pos, logp, grad, avg, last, n_acc, acc_sum, tr, s, q))}


def _every_entry_point(ctx, state0, beta, eps, n):
    """The outputs of hmc_step, hmc_step_keys, hmc_run (both key modes, thin = 2) and hmc_warmup on fixed keys, as one flat dict."""
    key, keys = prng.PRNGKey(11), prng.split(prng.PRNGKey(12), n)
    out = {}
    for tag, k in (("step", key), ("step_keys", keys)):
        out.update({f"{tag}.{name}": v for name, v in _stepwise(ctx, state0, k, beta, eps, 1).items()})
    for tag, k in (("run", key), ("run_keys", keys)):
        out.update({f"{tag}.{name}": v for name, v in _run(ctx, state0, k, beta, eps, N_STEPS, 2).items()})
    for tag, k in (("warmup", key), ("warmup_keys", keys)):
        w = _window(ctx, state0, k, beta, eps, N_STEPS, window=False)
        out.update({f"{tag}.{name}": v for name, v in w.items() if not name.startswith("pos_sum")})
    return out


@pytest.mark.parametrize("case", list(FAMILIES))
def test_ones_are_free(case):
    kind, d, tail, n, eps, _, _ = FAMILIES[case]
    ctx, pos0, _ = _ctx(kind, d, tail, n)
    state0 = _init(ctx, pos0, 1.0)
    assert ctx.get_inverse_mass()[1] is False
    unit = _every_entry_point(ctx, state0, 1.0, eps, n)
    win = _window(ctx, state0, prng.PRNGKey(11), 1.0, eps, N_STEPS)           # no mass set: the mass instance on ones
    for name, v in win.items():
        if not name.startswith("pos_sum"):
            np.testing.assert_array_equal(v, unit["warmup." + name], err_msg="window " + name)
    assert np.isfinite(win["pos_sum"]).all() and (win["pos_sumsq"] >= 0).all()
    ctx.set_inverse_mass(np.ones(d))
    got, is_set = ctx.get_inverse_mass()
    assert is_set and (got == 1).all()
    ones = _every_entry_point(ctx, state0, 1.0, eps, n)
    assert set(ones) == set(unit)
    for name in unit:
        np.testing.assert_array_equal(ones[name], unit[name], err_msg=name)
    moved = [name for name in unit if name.endswith(".isacc")]
    assert any(unit[name].any() for name in moved)                              # (chains move: the comparison is not of untouched states)
    ctx.set_inverse_mass(None)
    assert ctx.get_inverse_mass()[1] is False
    ctx.close()


# Both decisions.  At tests/test_gpu_hmc.py's phi-four step size, 2e-4, no proposal is ever rejected: the restatement's smallest
# acceptance probability over the four steps of 64 chains is 0.99998 (d = 64), 1.0 (d = 256), 0.99998 (d = 48), so those three cases can
# only assert that proposals are accepted, as that file does.  The two mixture cases hold a rejection each (restatement: 64, 64, 64, 63
# and 64, 63, 64, 64 accepted).  For phi-four the rejected branch is covered by two further cases at a step size inside the stable band
# of velocity Verlet under this ``minv`` where the restatement rejects: d = 64 at 0.065 (64, 64, 61, 61 accepted), d = 48 at 0.07 (64, 64,
# 57, 62); the restatement with the position rounded to float32 after every drift and a float32 gradient stays within 0.13 of the
# tolerances there.  d = 256 has no such step size: between 0.0304 (all accepted) and 0.0311 (2 to 19 of 64) the same emulation uses up
# to 0.7 of the position tolerance, the integrator being at its stability limit.
BOTH_DECISIONS = {"gmm4", "gmm16", "phi4-64-large", "phi4-48-large"}
LARGE_EPS = {"phi4-64-large": 0.065, "phi4-48-large": 0.07}


STEP_CASES = ["phi4-64", "phi4-256", "phi4-48", "gmm4", "gmm16", "phi4-64-large", "phi4-48-large"]


@pytest.mark.parametrize("case", STEP_CASES)
def test_mass_step_matches_the_float64_restatement(case):
    """tests/test_gpu_hmc.py::test_hmc_step_matches_oracle with ``minv`` log-spaced over [0.25, 4]: same cases, step sizes, protocol
    (both sides continue from the kernel's decisions, borderline decisions excluded) and tolerances."""
    import torch
    from tests import gpu_util as gu
    from tests.test_gpu_hmc import _dev
    if case.startswith("phi4"):
        d = int(case.split("-")[1]); B = 64
        args, dist, k, model, state = gu.phi4_setup(d=d, B=B, hidden=32, F=16)
        eps, L_, beta = (LARGE_EPS.get(case, 2e-4), 12, 0.7)
    elif case == "gmm4":
        B = 64; args, dist, k, model, state = gu.gmm4_setup(B=B); eps, L_, beta = (0.15, 8, 1.0)
    else:
        B = 64; args, dist, k, model, state = gu.gmm16_setup(B=B, hidden=32, F=16); eps, L_, beta = (0.1, 6, 0.5)
    d = args.dim
    minv = mr.log_spaced_mass(d)
    ctx = gu.make_ctx(dist, args, fourier=model.f, params=state.params)
    ctx.set_inverse_mass(minv)
    np.testing.assert_array_equal(ctx.get_inverse_mass()[0], minv)
    x32 = dist.init_params.astype(np.float32)
    pos = _dev(x32); logp = torch.empty(B, dtype=torch.float64, device="cuda"); grad = torch.empty(B, d, device="cuda")
    ctx.mala_init(pos, beta, logp, grad)
    vg = targets.Tempered(dist, beta).value_and_grad
    st = omala.MALAState(x32.astype(np.float64), logp.cpu().numpy(), grad.cpu().numpy().astype(np.float64))
    acc = torch.empty(B, device="cuda"); isacc = torch.empty(B, dtype=torch.uint8, device="cuda")
    seen = set()
    for it in range(4):
        key = prng.PRNGKey(50 + it)
        ctx.hmc_step(key, beta, eps, L_, pos, logp, grad, acc, isacc)
        st_o, info, u = mr.kernel(prng.split(key, B), st, vg, eps, L_, minv)
        pa_g, ia_g = acc.cpu().numpy().astype(np.float64), isacc.cpu().numpy().astype(bool)
        tol = 5e-6 * max(1.0, np.abs(st.logdensity).max()) + (5e-4 if case.startswith("gmm") else 0.0)
        err_p = np.abs(np.log(np.maximum(pa_g, 1e-30)) - np.log(np.maximum(info.acceptance_rate, 1e-30))).max()
        border = np.abs(u - info.acceptance_rate) < 10 * tol * np.maximum(info.acceptance_rate, 1e-30) + 1e-6
        m = ia_g[:, None]
        st = omala.MALAState(np.where(m, info.proposed_position, st.position), np.where(ia_g, vg(info.proposed_position)[0], st.logdensity),
                             np.where(m, vg(info.proposed_position)[1], st.logdensity_grad))
        e = np.abs(pos.cpu().numpy().astype(np.float64) - st.position).max()
        e_lp = np.abs(logp.cpu().numpy() - st.logdensity).max()
        print(f"{case} step {it}: log acceptance probability off by {err_p:.3g} (tolerance {tol + 1e-5:.3g}), position by {e:.3g} "
              f"({3e-6 * max(1.0, np.abs(st.position).max()):.3g}), log-density by {e_lp:.3g}; accepted {ia_g.sum()} of {B}, borderline {border.sum()}")
        assert err_p < tol + 1e-5, case
        assert (ia_g == info.is_accepted)[~border].all()
        seen |= set(ia_g.tolist())
        assert e < 3e-6 * max(1.0, np.abs(st.position).max()), (case, it, e)
        assert e_lp < 2e-6 * max(1.0, np.abs(st.logdensity).max()) + (5e-4 if case.startswith("gmm") else 0.0)
        st = omala.MALAState(pos.cpu().numpy().astype(np.float64), logp.cpu().numpy(), grad.cpu().numpy().astype(np.float64))
    assert True in seen, case                                   # chains move
    assert False in seen or case not in BOTH_DECISIONS, case    # at least one proposal rejected (see BOTH_DECISIONS)
    ctx.close()


@pytest.mark.parametrize("variant", list(rc.VARIANTS))
@pytest.mark.parametrize("case", rc.MASS_CASES)
def test_mass_step_matches_the_float64_restatement_above_d_256(case, variant):
    """``hmc_trajectory<MAXIT 16 / 32, BCRT false / true, MASS>`` (and BCRT at MAXIT 4: d65_pbc) against tests/hmc_mass_ref.py, element by element: the protocol of
    tests/test_gpu_row_instances.py::test_hmc_step_and_step_keys_match_oracle (16 chains from ``rc.start_state``, 3 steps of 3 leapfrog
    steps, both sides continue from the kernel's decisions, the seam set asserted on its own) with ``minv = rc.inverse_mass(case)``
    installed -- log-spaced over [0.25, 4] in a fixed permutation, so a ``minv`` read at another element moves x by up to 16 x eps p.
    Tolerances: that test's, with ``rc.HMC_MASS_F32_DISTANCE`` (the restatement against its device-format variant under this mass, on
    the CPU) where it has ``HMC_F32_DISTANCE``.  tests/test_row_instance_cases.py asserts on the restatement alone that both decisions
    occur and at most 1 of 16 chains per step lies in the band.
    Measured on MI355X, largest error / tolerance over both variants (log acceptance probability, position, log-density, gradient):
    d65_pbc 0.24 0.040 0.14 0.013; d257_d0 0.084 0.047 0.11 0.060; 17x17_db 0.021 0.045 0.023 0.0090; d1025_d0 0.12 0.047 0.27 0.25;
    d2048_pbc 0.20 0.057 0.30 0.59."""
    import torch
    from tests.test_gpu_row_instances import B, _ctx as _row_ctx, _merge, _report, _rows, _state, _vec
    beta = rc.VARIANTS[variant][0]
    eps = rc.MASS_STEP_SIZES[case][variant]
    minv = rc.inverse_mass(case)
    ctx, pos = _row_ctx(case)
    ctx.set_inverse_mass(minv)
    vg = rc.value_and_grad(case, variant)
    logp, grad = _state(ctx, pos, beta)
    info = lambda: (torch.empty(B, device="cuda"), torch.empty(B, dtype=torch.uint8, device="cuda"))
    seen, worst = set(), {}
    for j in range(rc.N_STEPS):
        key, keys = rc.step_keys(case, j, "hmc_mass")
        x0, lp0, g0 = pos.cpu().numpy().astype(np.float64), logp.cpu().numpy(), grad.cpu().numpy().astype(np.float64)
        st = omala.MALAState(x0, lp0, g0)
        new, o, u = rc.oracle_step("hmc_mass", variant, st, vg, keys, eps)
        by_keys = (pos.clone(), logp.clone(), grad.clone()) + info()
        ctx.hmc_step_keys(_keys_dev(keys), beta, eps, rc.HMC_LEAPFROG, *by_keys)
        acc, isacc = info()
        ctx.hmc_step(key, beta, eps, rc.HMC_LEAPFROG, pos, logp, grad, acc, isacc)
        for name, a, b in zip(("pos", "logp", "grad", "acc", "isacc"), (pos, logp, grad, acc, isacc), by_keys):
            np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy(), err_msg=f"step {j}: hmc_step vs hmc_step_keys, {name}")
        ia_g, pa_g = isacc.cpu().numpy().astype(bool), acc.cpu().numpy().astype(np.float64)
        tol = 5e-6 * max(1.0, np.abs(lp0).max())
        f32_p, f32_lp = (4 * v for v in rc.HMC_MASS_F32_DISTANCE[case][variant])
        _merge(worst, scale=np.abs(lp0).max(),
               p=_vec(f"step {j} log acceptance probability", np.log(np.maximum(pa_g, 1e-30)), np.log(np.maximum(o.acceptance_rate, 1e-30)), 0.0,
                      max(tol + 1e-5, f32_p)))
        border = rc.borderline("hmc_mass", st, o, u)
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
    _report(case, f"hmc_mass/{variant}", worst)
    ctx.close()


@pytest.mark.parametrize("case", list(FAMILIES))
def test_run_equals_single_step_launches_under_a_mass(case):
    kind, d, tail, n, _, eps, _ = FAMILIES[case]
    ctx, pos0, _ = _ctx(kind, d, tail, n)
    state0 = _init(ctx, pos0, 1.0)
    ctx.set_inverse_mass(mr.log_spaced_mass(d))
    for key in (prng.PRNGKey(21), prng.split(prng.PRNGKey(22), n)):            # step-major, chain-major
        _assert_run_equals_steps(_run(ctx, state0, key, 1.0, eps, N_STEPS, 1), _stepwise(ctx, state0, key, 1.0, eps, N_STEPS))
    # the mass is what moved the chains: the same run under unit mass ends elsewhere
    with_mass = _run(ctx, state0, prng.PRNGKey(21), 1.0, eps, N_STEPS, 0, traj=False)["pos"]
    ctx.set_inverse_mass(None)
    assert (with_mass != _run(ctx, state0, prng.PRNGKey(21), 1.0, eps, N_STEPS, 0, traj=False)["pos"]).any()
    ctx.close()


def _replay(ctx, state0, key, beta, step_traj):
    """tests/test_gpu_warmup.py's replay -- one ``hmc_step_keys`` launch per step and distinct step size on the window's step keys,
    keeping the rows of the chains that used it -- which also keeps the positions after every step."""
    import torch
    from tests.test_gpu_warmup import _step_keys
    cur = [t.clone() for t in state0]
    n = cur[0].shape[0]
    acc = torch.empty(n, device="cuda"); isacc = torch.empty(n, dtype=torch.uint8, device="cuda")
    keys = _step_keys(key, len(step_traj), n_total=n, n=n)
    p_all, ia_all, pos_all = [], [], []
    for m, row in enumerate(step_traj):
        nxt = [t.clone() for t in cur]
        p_m, ia_m = np.zeros(n, np.float32), np.zeros(n, bool)
        kd = _keys_dev(keys[m])
        for eps in np.unique(row):
            pos, logp, grad = (t.clone() for t in cur)
            ctx.hmc_step_keys(kd, beta, float(eps), L, pos, logp, grad, acc, isacc)
            sel = torch.as_tensor(row == eps).cuda()
            for dst, src in zip(nxt, (pos, logp, grad)):
                dst[sel] = src[sel]
            p_m[row == eps] = acc.cpu().numpy()[row == eps]
            ia_m[row == eps] = isacc.cpu().numpy().astype(bool)[row == eps]
        cur = nxt
        p_all.append(p_m); ia_all.append(ia_m); pos_all.append(cur[0].cpu().numpy().copy())
    return dict(pos=cur[0].cpu().numpy(), logp=cur[1].cpu().numpy(), grad=cur[2].cpu().numpy(), acc=np.stack(p_all), isacc=np.stack(ia_all),
                positions=np.stack(pos_all))


WINDOW_CASES = [(c, False) for c in FAMILIES] + [("phi4_d64", True), ("gmm4", True)]


@pytest.mark.parametrize("case,chain_major", WINDOW_CASES, ids=[c + ("-chain_major" if cm else "") for c, cm in WINDOW_CASES])
def test_window_replays_as_single_steps_and_sums_in_step_order(case, chain_major):
    from tests.test_gpu_warmup import _assert_warmup_equals_replay
    kind, d, tail, n, _, eps, n_steps = FAMILIES[case]
    ctx, pos0, _ = _ctx(kind, d, tail, n)
    state0 = _init(ctx, pos0, 1.0)
    ctx.set_inverse_mass(mr.log_spaced_mass(d))
    key = prng.split(prng.PRNGKey(33), n) if chain_major else prng.PRNGKey(21)
    w = _window(ctx, state0, key, 1.0, eps, n_steps)
    rep = _replay(ctx, state0, key, 1.0, w["step_traj"])
    mixed, parted = _assert_warmup_equals_replay(w, rep, eps, TARGET)
    assert mixed and parted, (mixed, parted)
    s, q = np.zeros((n, d)), np.zeros((n, d))
    for x in rep["positions"]:                                                  # float32 positions, summed as float64 in step order
        x = x.astype(np.float64)
        s = s + x
        q = q + x * x
    np.testing.assert_array_equal(w["pos_sum"], s)
    np.testing.assert_array_equal(w["pos_sumsq"], q)
    # hmc_warmup under the same mass is the window without the sums
    plain = _window(ctx, state0, key, 1.0, eps, n_steps, window=False)
    for name in ("pos", "logp", "grad", "step_avg", "step_last", "n_acc", "acc_sum", "step_traj"):
        np.testing.assert_array_equal(plain[name], w[name], err_msg=name)
    ctx.close()


def test_errors_name_inv_mass_and_change_nothing():
    import torch
    from mfm_amd import _lib
    ctx, pos0, _ = _ctx("phi4", 64, None)
    good = mr.log_spaced_mass(64)
    ctx.set_inverse_mass(good)
    for bad in (np.ones(63), np.ones(65), np.r_[good[:63], 0.0], np.r_[good[:63], -1.0], np.r_[np.nan, good[1:]], np.r_[good[:63], np.inf]):
        with pytest.raises(_lib.MfmError, match="inv_mass"):
            ctx.set_inverse_mass(bad)
        got, is_set = ctx.get_inverse_mass()
        assert is_set
        np.testing.assert_array_equal(got, good)
    # the device's copy is unchanged too: a step after the rejected calls equals a step before them
    state0 = _init(ctx, pos0, 1.0)
    a = _stepwise(ctx, state0, prng.PRNGKey(3), 1.0, 0.044, 1)
    with pytest.raises(_lib.MfmError, match="inv_mass"):
        ctx.set_inverse_mass(np.full(64, -2.0))
    b = _stepwise(ctx, state0, prng.PRNGKey(3), 1.0, 0.044, 1)
    for name in a:
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
    # the window's own arguments
    pos, logp, grad = state0
    f64 = dict(dtype=torch.float64, device="cuda")
    avg, s, q = torch.empty(16, **f64), torch.empty(16, 64, **f64), torch.empty(16, 64, **f64)
    before = pos.clone()
    with pytest.raises(_lib.MfmError, match="d_pos_sum"):
        ctx.hmc_warmup_window(prng.PRNGKey(1), 1.0, 1e-2, L, 4, 0.8, pos, logp, grad, avg, None, q)
    with pytest.raises(_lib.MfmError, match="d_pos_sum"):
        ctx.hmc_warmup_window(prng.PRNGKey(1), 1.0, 1e-2, L, 4, 0.8, pos, logp, grad, avg, s, None)
    with pytest.raises(_lib.MfmError, match="pos_sumsq"):
        ctx.hmc_warmup_window(prng.PRNGKey(1), 1.0, 1e-2, L, 4, 0.8, pos, logp, grad, avg, s, torch.empty(16, 63, **f64))
    with pytest.raises(_lib.MfmError, match="n_steps"):
        ctx.hmc_warmup_window(prng.PRNGKey(1), 1.0, 1e-2, L, 0, 0.8, pos, logp, grad, avg, s, q)
    with pytest.raises(_lib.MfmError, match="target_accept"):
        ctx.hmc_warmup_window(prng.PRNGKey(1), 1.0, 1e-2, L, 4, 1.0, pos, logp, grad, avg, s, q)
    assert torch.equal(pos, before)
    ctx.close()
    # the Cox process: both new HMC calls refuse it with the step's message
    cox, cpos0, _ = _ctx("lgcp", 16, None)
    cpos, clogp, cgrad = _init(cox, cpos0, 1.0)
    cox.set_inverse_mass(np.full(16, 2.0))                                      # (installing a vector needs no target)
    with pytest.raises(_lib.MfmError, match="Cox"):
        cox.hmc_step(prng.PRNGKey(1), 1.0, 1e-2, L, cpos, clogp, cgrad)
    with pytest.raises(_lib.MfmError, match="Cox"):
        cox.hmc_warmup_window(prng.PRNGKey(1), 1.0, 1e-2, L, 4, 0.8, cpos, clogp, cgrad, avg, torch.empty(16, 16, **f64), torch.empty(16, 16, **f64))
    cox.close()


def test_python_kernels_install_their_own_mass():
    """``hmc(..., inverse_mass_matrix=v)``: step, run and warmup equal the context calls under ``v``; a later call without the argument
    runs under unit mass whatever the earlier one installed; a bad vector raises ``ValueError``."""
    from mfm_amd import random as jr
    from mfm_amd.bblackjax.mcmc import hmc as H
    from tests.test_gpu_hmc_run import _gmm_engine
    eng, dist, pos = _gmm_engine(16)
    minv = np.array([0.25, 4.0])
    unit, mass = H.hmc(dist.logprob, 0.9, L), H.hmc(dist.logprob, 0.9, L, inverse_mass_matrix=minv)
    state = unit.init(pos)
    key = jr.PRNGKey(6)
    eng.ctx.set_inverse_mass(minv)
    want_mass = _run(eng.ctx, tuple(state), key, 1.0, 0.9, N_STEPS, 0, traj=False)
    eng.ctx.set_inverse_mass(None)
    want_unit = _run(eng.ctx, tuple(state), key, 1.0, 0.9, N_STEPS, 0, traj=False)
    assert (want_mass["pos"] != want_unit["pos"]).any()
    got_mass, _ = mass.step.run(key, state, N_STEPS)
    assert eng.ctx.get_inverse_mass()[1]
    got_unit, _ = unit.step.run(key, state, N_STEPS)                            # after a mass call: cleared first
    assert not eng.ctx.get_inverse_mass()[1]
    np.testing.assert_array_equal(got_mass.position.cpu().numpy(), want_mass["pos"])
    np.testing.assert_array_equal(got_unit.position.cpu().numpy(), want_unit["pos"])
    k = H.build_kernel()
    s1, _ = k(key, state, dist.logprob, 0.9, L, inverse_mass_matrix=minv)
    s2, _ = mass.step(key, state)
    np.testing.assert_array_equal(s1.position.cpu().numpy(), s2.position.cpu().numpy())
    _, wi = mass.step.warmup(key, state, N_STEPS)
    _, wk = k.warmup(key, state, dist.logprob, 0.9, L, N_STEPS, inverse_mass_matrix=minv)
    np.testing.assert_array_equal(wi.step_size.cpu().numpy(), wk.step_size.cpu().numpy())
    _, wu = unit.step.warmup(key, state, N_STEPS)
    assert (wi.step_size != wu.step_size).any()
    with pytest.raises(ValueError, match="inverse_mass_matrix"):
        k(key, state, dist.logprob, 0.9, L, inverse_mass_matrix=np.ones(3))
    with pytest.raises(ValueError, match="inverse_mass_matrix"):
        k.run(key, state, dist.logprob, 0.9, L, N_STEPS, inverse_mass_matrix=np.array([1.0, 0.0]))
    eng.close()


# ---- the adaptation end to end -------------------------------------------------------------------------------------------------------
AD_VAR = np.array([0.04, 1.0, 25.0, 0.25])
AD_CHAINS, AD_L, AD_STEPS, AD_STEP0 = 1024, 8, 300, 0.05


def _ad_oracle():
    dist = targets.GaussianMixture(np.zeros((1, 4)), AD_VAR[None], np.ones(1))
    dist.dim = 4
    return dist, targets.Tempered(dist, 1.0).value_and_grad


def _ad_start():
    """The initial chains: draws from the target itself (float32, as the device holds them)."""
    return (prng.normal_rows(prng.split(prng.PRNGKey(1), AD_CHAINS), 4) * np.sqrt(AD_VAR)).astype(np.float32)


@pytest.fixture(scope="module")
def adaptation_restated():
    """The restated driver on the device's key (0) and on 8 other keys, on the CPU: ``log minv [4]`` and ``log step_size`` of key 0, and
    the standard deviation of each over the 8 others."""
    _, vg = _ad_oracle()
    state = omala.init(_ad_start().astype(np.float64), vg)

    def one(seed):
        _, step, minv, _ = mr.window_adaptation(prng.PRNGKey(seed), state, vg, AD_L, AD_STEP0, AD_STEPS, TARGET)
        return np.r_[np.log(minv), np.log(step)]
    ref = one(0)
    others = np.stack([one(s) for s in range(1, 9)])
    return ref, others.std(axis=0, ddof=1)


def test_window_adaptation_against_the_restated_driver(adaptation_restated):
    """A one-mode mixture in d = 4 with variances (0.04, 1, 25, 0.25), 1024 chains, L = 8, 300 steps: the device's ``log minv_j`` and
    log pooled step size lie within three times the restatement's own spread (its standard deviation over 8 other keys) of the
    restatement on the same key.  Float32 and float64 chains part at the first borderline decision, so the bound is statistical.
    On an MI355X: device ``minv`` (0.03693, 0.9324, 24.24, 0.2293), step size 0.7869; restatement (0.03678, 0.9274, 23.64, 0.2291) and 0.7940.
    In the log: the restatement's spread over the 8 other keys (0.0074, 0.0099, 0.0090, 0.0046) and 0.0038, the device's distance (0.0040,
    0.0054, 0.0251, 0.0005) and 0.0090, i.e. 0.54, 0.54, 2.81, 0.11 and 2.35 spreads."""
    import torch
    from mfm_amd import distributions as D, random as jr
    from mfm_amd.bblackjax.adaptation.window_adaptation import window_adaptation, window_schedule
    from mfm_amd.bblackjax.mcmc import hmc as H
    from mfm_amd.engine import Engine
    from oracle import loop
    ref, sd = adaptation_restated
    dist = D.GaussianMixture(np.zeros((1, 4)), AD_VAR[None], np.ones(1))
    dist.dim = 4
    args = loop.default_args(example="gaussian-mixture", dim=4, num_chain=AD_CHAINS, fourier_dim=16, hidden_x=[32, 32], hidden_t=[32, 32], hidden_xt=[32, 32])
    eng = Engine(dist, args, None)
    state = H.init(torch.as_tensor(_ad_start()).cuda(), dist.logprob)
    new, params, info = window_adaptation(dist.logprob, AD_L, AD_STEP0, TARGET).run(jr.PRNGKey(0), state, AD_STEPS)
    assert info.schedule == window_schedule(AD_STEPS) and len(info.step_sizes) == 4 and len(info.inverse_mass_matrices) == 2
    assert not eng.ctx.get_inverse_mass()[1]                                    # the context is left at unit mass
    minv, step = params["inverse_mass_matrix"], params["step_size"]
    assert minv.shape == (4,) and minv.dtype == np.float64 and np.isfinite(minv).all() and (minv > 0).all() and step > 0
    dev = np.r_[np.log(minv), np.log(step)]
    print(f"device   log minv {dev[:4]}, log step size {dev[4]:.5f} (minv {minv}, step size {step:.5f})")
    print(f"restated log minv {ref[:4]}, log step size {ref[4]:.5f}")
    print(f"spread over 8 keys {sd}; distance {np.abs(dev - ref)}; distance / spread {np.abs(dev - ref) / sd}")
    print(f"acceptance per segment {info.acceptance_rates}, step sizes {info.step_sizes}")
    assert (np.abs(dev - ref) <= 3 * sd).all(), (dev, ref, sd)
    assert not torch.equal(new.position, state.position)
    eng.close()


def test_adapt_mass_on_the_command_line_path():
    """``--mcmc_kernel hmc --adapt_steps 40 --adapt_mass`` on phi-four d = 64: a positive, finite mass of length 64 in the extras, on the
    engine's context for the training loop; without the flag the run has tests/test_gpu_warmup.py's behaviour (the pooled step size of
    one ``warmup`` on ``split(key_gen, 4)[3]``, no mass anywhere)."""
    from mfm_amd import distributions as D, exe_flow_matching as E, random as jr
    from mfm_amd.bblackjax.mcmc.hmc import hmc
    from oracle import loop
    kw = dict(example="phi-four", dim=64, num_chain=32, learning_iter=3, mcmc_per_flow_steps=4.0, hutchs=True, fourier_dim=16, seed=7, eval_iter=1,
              step_size=0.03, hidden_x=[32, 32], hidden_t=[32, 32], hidden_xt=[32, 32], mcmc_kernel="hmc", hmc_steps=4, adapt_steps=40,
              adapt_target=0.8, ess_steps=16)
    args = loop.default_args(adapt_mass=True, **kw)
    _, _, ex = E.run(D.PhiFour(64), args, None, log_every=1000, return_extras=True)
    minv = ex["adapted_inverse_mass"]
    assert minv.shape == (64,) and np.isfinite(minv).all() and (minv > 0).all()
    assert ex["adapted_inverse_mass_min"] == minv.min() and ex["adapted_inverse_mass_max"] == minv.max()
    assert np.isfinite(ex["adapted_step_size"]) and ex["adapted_step_size"] > 0 and args.step_size == ex["adapted_step_size"]
    assert 0.0 < ex["adapt_acceptance"] <= 1.0 and np.isfinite(ex["ess_per_grad_mean"])
    got, is_set = ex["engine"].ctx.get_inverse_mass()
    assert is_set
    np.testing.assert_array_equal(got, minv)
    ex["engine"].close()
    with pytest.raises(ValueError, match="adapt_mass"):
        E.check_adapt_args(loop.default_args(adapt_mass=True, **dict(kw, adapt_steps=0)))

    dist0 = D.PhiFour(64)
    args0 = loop.default_args(**kw)
    _, _, ex0 = E.run(dist0, args0, None, log_every=1000, return_extras=True)
    eng = ex0["engine"]
    assert "adapted_inverse_mass" not in ex0 and not eng.ctx.get_inverse_mass()[1]
    algo = hmc(dist0.logprob, 0.03, 4)
    _, info = algo.step.warmup(jr.split(ex0["key_gen"], 4)[3], algo.init(eng.local(dist0.init_params)), 40, 0.8)
    assert info.pooled_step_size == ex0["adapted_step_size"] == args0.step_size
    eng.close()
