"""GPU tests of ``mfm_hmc_run`` / ``mfm_hmc_step_keys`` (mfm_amd/csrc/hmc_run.hip, hmc.hip): many HMC steps in one launch with the chain
resident in registers, and the HMC step on a caller's own per-chain keys.

The yardstick of the run is the single-step kernel: a run of n steps must give the BITS of n launches of ``mfm_hmc_step`` /
``mfm_hmc_step_keys`` on the step keys the run derives (step-major: ``split(key, n)[j]``; chain-major: ``split_rows(keys, n)[:, j]``),
for every kernel instance (MAXIT 1 / 4 / 16 / 32, each with the run-time boundary, a partial last lane group, the mixture path).  The per-chain-key
step and the run are anchored in the float64 oracle (oracle/hmc.py) at the per-step tolerances of tests/test_gpu_hmc.py; then thinning,
the Python API with ``inference_loop0``, the argument errors and ``--ess_steps`` under ``--mcmc_kernel hmc``.

Step sizes (16 chains, 6 steps of L = 3 leapfrog steps): chosen with the float64 oracle on the same initial positions and keys so that
the six steps hold accepted and rejected trajectories.  HMC accepts nearly everything while velocity Verlet is stable and nearly nothing
beyond its stability limit (eps * omega_max = 2), so the bit-identity cases sit just below that limit, where the energy error is O(1):
oracle counts of accepted trajectories out of 96: phi-four d = 64 with 0.088: 80, d = 100 with 0.071: 56, d = 256 with 0.0445: 28,
periodic with 0.088: 77, the 8 x 8 lattice with 0.14: 57, beta = 0.3 with 0.16: 63, the 4-mode mixture with 1.8: 50 (chain-major keys:
77 at d = 64, 48 on the mixture).  The comparisons WITH the oracle use steps inside the stable region, where one step does not amplify
the float32 rounding of the state and the per-step tolerances of tests/test_gpu_hmc.py apply as they stand: phi-four 0.03 (oracle: 90 of
96 on the chain-major keys, 78 of 80 on the run's), the mixture 1.0 (80 of 96).  Every test asserts that both outcomes occur."""
import numpy as np
import pytest

from oracle import hmc as ohmc, mala as omala, prng, targets
from tests import row_instance_cases as rc

pytestmark = pytest.mark.gpu

B, N_STEPS, L = 16, 6, 3

# name: (target, d, phi-four block tail {kind, b[, dim_phys]} or None, beta, step size)
CASES = {
    "phi4_d64": ("phi4", 64, None, 1.0, 0.088),
    "phi4_d100": ("phi4", 100, None, 1.0, 0.071),
    "phi4_d256": ("phi4", 256, None, 1.0, 0.0445),
    "phi4_d64_pbc": ("phi4", 64, [1.0, 0.0], 1.0, 0.088),
    "phi4_8x8_dirichlet": ("phi4", 64, [0.0, 0.7, 2.0], 1.0, 0.14),
    "gmm4": ("gmm", 2, None, 1.0, 1.8),
    "phi4_d64_beta03": ("phi4", 64, None, 0.3, 0.16),
}
# The dispatch instances above d = 256 (and MAXIT 4 with a run-time boundary), which tie hmc_run_kernel and the warmup kernels there to the
# step kernel that tests/test_gpu_row_instances.py holds to the oracle: target "row", the case of tests/row_instance_cases.py in the place
# of d -- its start state near a mode (16 chains), its boundary and its beta = 1 step size, ROW_STEPS steps.  (MAXIT, BCRT): d65_pbc
# (4, true), d257_d0 (16, false), 17x17_pbc (16, true), d2048_d0 (32, false), d1025_pbc and 33x33_db (32, true).
ROW_STEPS = 5
ROW_CASES = ("d65_pbc", "d257_d0", "17x17_pbc", "d2048_d0", "d1025_pbc", "33x33_db")
CASES.update({"row_" + c: ("row", c, None, 1.0, rc.STEP_SIZES[c]["hmc"]["b1"]) for c in ROW_CASES})
ORACLE_EPS = {"phi4_d64": 0.03, "gmm4": 1.0}      # inside the stable region of velocity Verlet (module docstring)


def _n_steps(case):
    return ROW_STEPS if CASES[case][0] == "row" else N_STEPS


def _ctx(kind, d, tail, n=B):
    """A context on the target, the initial positions (float32, on the device) and the oracle's target."""
    import torch
    from mfm_amd import _lib
    from tests import gpu_util as gu
    if kind == "row":                               # d: a case of tests/row_instance_cases.py, with its own chains and start state
        args, dist0, *_ = gu.phi4_setup(d=rc.CASES[d][0], B=rc.N_CHAINS, hidden=32, F=16)
        ctx = gu.make_ctx(dist0, args)
        if rc.block(d) is not None:
            ctx.set_target(_lib.PHI4, rc.block(d))
        return ctx, torch.as_tensor(rc.start_state(d)).cuda(), rc.oracle_dist(d)
    if kind == "phi4":
        args, dist, k, model, state = gu.phi4_setup(d=d, B=n, hidden=32, F=16)
    elif kind == "gmm":
        args, dist, k, model, state = gu.gmm4_setup(B=n)
    else:
        args, dist, k, model, state = gu.lgcp_setup(n=int(np.sqrt(d)), B=n)
    ctx = gu.make_ctx(dist, args)
    if tail is not None:
        ctx.set_target(_lib.PHI4, [dist.a, dist.beta] + tail)
    return ctx, torch.as_tensor(dist.init_params.astype(np.float32)).cuda(), dist


def _init(ctx, pos0, beta):
    import torch
    pos = pos0.clone()
    logp = torch.empty(pos.shape[0], dtype=torch.float64, device="cuda"); grad = torch.empty_like(pos)
    ctx.mala_init(pos, beta, logp, grad)
    return pos, logp, grad


def _keys_dev(keys):
    import torch
    return torch.as_tensor(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32)).cuda()


def _stepwise(ctx, state0, key, beta, eps, n_steps):
    """n single-step launches on the run's step keys; the state after, and the info of, every launch (numpy)."""
    import torch
    from mfm_amd import random as jr
    pos, logp, grad = (t.clone() for t in state0)
    n = pos.shape[0]
    acc = torch.empty(n, device="cuda"); isacc = torch.empty(n, dtype=torch.uint8, device="cuda")
    per_chain = np.ndim(key) == 2
    step_keys = jr.split_rows(key, n_steps) if per_chain else jr.split(key, n_steps)
    out = dict(pos=[], logp=[], grad=[], acc=[], isacc=[])
    for j in range(n_steps):
        if per_chain:
            ctx.hmc_step_keys(_keys_dev(step_keys[:, j]), beta, eps, L, pos, logp, grad, acc, isacc)
        else:
            ctx.hmc_step(step_keys[j], beta, eps, L, pos, logp, grad, acc, isacc)
        for name, t in zip(out, (pos, logp, grad, acc, isacc)):
            out[name].append(t.cpu().numpy().copy())
    return {k: np.stack(v) for k, v in out.items()}


def _run(ctx, state0, key, beta, eps, n_steps, thin, traj=True):
    import torch
    pos, logp, grad = (t.clone() for t in state0)
    n, d = pos.shape
    acc = torch.empty(n, device="cuda"); isacc = torch.empty(n, dtype=torch.uint8, device="cuda")
    n_acc = torch.empty(n, dtype=torch.int32, device="cuda"); acc_sum = torch.empty(n, dtype=torch.float64, device="cuda")
    tp = tl = None
    if traj and thin > 0:
        tp = torch.empty(n_steps // thin, n, d, device="cuda"); tl = torch.empty(n_steps // thin, n, dtype=torch.float64, device="cuda")
    ctx.hmc_run(_keys_dev(key) if np.ndim(key) == 2 else key, beta, eps, L, n_steps, pos, logp, grad, thin=thin, n_acc=n_acc, acc_sum=acc_sum,
                acc=acc, is_acc=isacc, traj_pos=tp, traj_logp=tl)
    names = ("pos", "logp", "grad", "acc", "isacc", "n_acc", "acc_sum", "traj_pos", "traj_logp")
    return {k: (None if t is None else t.cpu().numpy()) for k, t in zip(names, (pos, logp, grad, acc, isacc, n_acc, acc_sum, tp, tl))}


def _assert_run_equals_steps(run, steps):
    """The run with thin = 1 against the launches, bit for bit (the sum of the acceptance probabilities to float32 rounding of each term)."""
    print(f"mean acceptance probability {steps['acc'].astype(np.float64).mean():.4f}, accepted {steps['isacc'].sum()} of {steps['isacc'].size}")
    assert 0 < steps["isacc"].sum() < steps["isacc"].size                      # both branches of the select are exercised
    for name in ("pos", "logp", "grad"):
        np.testing.assert_array_equal(run[name], steps[name][-1], err_msg=name)
    np.testing.assert_array_equal(run["traj_pos"], steps["pos"])
    np.testing.assert_array_equal(run["traj_logp"], steps["logp"])
    np.testing.assert_array_equal(run["n_acc"], steps["isacc"].astype(np.int64).sum(0))
    for name in ("acc", "isacc"):
        np.testing.assert_array_equal(run[name], steps[name][-1], err_msg="last " + name)
    # the run sums the float64 probabilities, the launches report them rounded to float32: 2^-24 relative per term, all terms >= 0
    # (and 2^-150 absolute per term where a tiny probability lands among float32's denormals)
    # and the two float64 sums of n terms differ by at most n ulps of float64 more
    n = steps["acc"].shape[0]
    np.testing.assert_allclose(run["acc_sum"], steps["acc"].astype(np.float64).sum(0), rtol=2.0 ** -24 + n * 2.0 ** -52, atol=n * 2.0 ** -150)


@pytest.mark.parametrize("case", list(CASES))
def test_run_is_bit_identical_with_single_step_launches(case):
    kind, d, tail, beta, eps = CASES[case]
    ctx, pos0, _ = _ctx(kind, d, tail)
    state0 = _init(ctx, pos0, beta)
    key = prng.PRNGKey(21)
    steps = _stepwise(ctx, state0, key, beta, eps, _n_steps(case))
    run = _run(ctx, state0, key, beta, eps, _n_steps(case), 1)
    _assert_run_equals_steps(run, steps)
    ctx.close()


@pytest.mark.parametrize("case", ["phi4_d64", "gmm4"])
def test_chain_major_keys(case):
    """key_mode 1: step j of chain b draws from split(keys[b], n)[j], what mfm_hmc_step_keys draws from split_rows(keys, n)[:, j]."""
    kind, d, tail, beta, eps = CASES[case]
    ctx, pos0, _ = _ctx(kind, d, tail)
    state0 = _init(ctx, pos0, beta)
    keys = prng.split(prng.PRNGKey(33), B)
    steps = _stepwise(ctx, state0, keys, beta, eps, N_STEPS)
    run = _run(ctx, state0, keys, beta, eps, N_STEPS, 1)
    _assert_run_equals_steps(run, steps)
    ctx.close()


def _oracle_step_check(case, st, keys, vg, eps, pos, logp, pa_g, ia_g):
    """One device step against one oracle step from the same state ``st`` on the same per-chain keys: the tolerances and the
    borderline-decision rule of tests/test_gpu_hmc.py:42-55.  Returns the device's decisions that were compared."""
    gmm = case.startswith("gmm")
    st_o, info, u = ohmc.kernel(keys, st, vg, eps, L)
    tol = 5e-6 * max(1.0, np.abs(st.logdensity).max()) + (5e-4 if gmm else 0.0)
    err_p = np.abs(np.log(np.maximum(pa_g, 1e-30)) - np.log(np.maximum(info.acceptance_rate, 1e-30))).max()
    border = np.abs(u - info.acceptance_rate) < 10 * tol * np.maximum(info.acceptance_rate, 1e-30) + 1e-6
    m = ia_g[:, None]
    lpn, gn = vg(info.proposed_position)
    ref = omala.MALAState(np.where(m, info.proposed_position, st.position), np.where(ia_g, lpn, st.logdensity), np.where(m, gn, st.logdensity_grad))
    e = np.abs(pos.astype(np.float64) - ref.position).max()
    e_lp = np.abs(logp - ref.logdensity).max()
    print(f"{case}: |log p - oracle| {err_p:.3g} (tol {tol + 1e-5:.3g}), |x - oracle| {e:.3g}, |logp - oracle| {e_lp:.3g}, borderline {border.sum()}")
    assert err_p < tol + 1e-5, case
    assert (ia_g == info.is_accepted)[~border].all()
    assert e < 3e-6 * max(1.0, np.abs(ref.position).max()), (case, e)
    assert e_lp < 2e-6 * max(1.0, np.abs(ref.logdensity).max()) + (5e-4 if gmm else 0.0)


@pytest.mark.parametrize("case", ["phi4_d64", "gmm4"])
def test_step_keys_matches_the_float64_oracle(case):
    """``mfm_hmc_step_keys`` against ``oracle.hmc.kernel`` on the same [B, 2] keys, one step at a time: the oracle restarts every step
    from the device's state (float32 positions), as tests/test_gpu_hmc.py does, over the six keys split_rows(keys, 6)[:, j]."""
    import torch
    kind, d, tail, beta, _ = CASES[case]
    eps = ORACLE_EPS[case]
    ctx, pos0, dist = _ctx(kind, d, tail)
    pos, logp, grad = _init(ctx, pos0, beta)
    vg = targets.Tempered(dist, beta).value_and_grad
    acc = torch.empty(B, device="cuda"); isacc = torch.empty(B, dtype=torch.uint8, device="cuda")
    step_keys = prng.split_rows(prng.split(prng.PRNGKey(33), B), N_STEPS)
    seen = set()
    for j in range(N_STEPS):
        st = omala.MALAState(pos.cpu().numpy().astype(np.float64), logp.cpu().numpy(), grad.cpu().numpy().astype(np.float64))
        ctx.hmc_step_keys(_keys_dev(step_keys[:, j]), beta, eps, L, pos, logp, grad, acc, isacc)
        ia_g = isacc.cpu().numpy().astype(bool)
        _oracle_step_check(case, st, step_keys[:, j], vg, eps, pos.cpu().numpy(), logp.cpu().numpy(), acc.cpu().numpy().astype(np.float64), ia_g)
        seen |= set(ia_g.tolist())
    assert seen == {True, False}, seen
    ctx.close()


def test_run_matches_the_float64_oracle():
    """phi-four d = 64, 16 chains, 5 steps, thin = 1.  The oracle's kernel restarts at every step from the device's previous kept state
    (float32 positions; log-density and gradient of the oracle at them), so each comparison is ONE step at the per-step tolerances of
    tests/test_gpu_hmc.py; the decisions are read from which rows moved and take that file's borderline rule.  The acceptance
    probability is compared where the device reports it: the last step's, and the run's sum through the per-step figures' mean."""
    _run_against_the_oracle("phi4", 64, ORACLE_EPS["phi4_d64"])


def test_run_matches_the_float64_oracle_at_d1025():
    """The same comparison on the MAXIT 32 instance: the Dirichlet-0 chain of d = 1025 from its start state near a mode
    (tests/row_instance_cases.py), at that table's step size and at the per-step tolerances tests/test_gpu_row_instances.py holds the
    step kernel to there: the two energy forms are floored by 4 x the float32 restatement's distance from the oracle
    (``row_instance_cases.HMC_F32_DISTANCE``, that module's docstring has the reason)."""
    f32 = tuple(4 * v for v in rc.HMC_F32_DISTANCE["d1025_d0"]["b1"])
    _run_against_the_oracle("row", "d1025_d0", rc.STEP_SIZES["d1025_d0"]["hmc"]["b1"], *f32)


def _run_against_the_oracle(kind, d, eps, f32_p=0.0, f32_lp=0.0):
    """f32_p / f32_lp: floors of the log acceptance probability's and the log-density's tolerance (0: the forms as they stand)."""
    n_steps, beta = 5, 1.0
    ctx, pos0, dist = _ctx(kind, d, None)
    state0 = _init(ctx, pos0, beta)
    vg = targets.Tempered(dist, beta).value_and_grad
    key = prng.PRNGKey(1)
    run = _run(ctx, state0, key, beta, eps, n_steps, 1)
    prev = pos0.cpu().numpy()
    tol_sum, p_sum, seen = 0.0, np.zeros(B), set()
    for j in range(n_steps):
        x = prev.astype(np.float64)
        lp, g = vg(x)
        st = omala.MALAState(x, lp, g)
        keys = prng.split(prng.split(key, n_steps)[j], B)
        st_o, info, u = ohmc.kernel(keys, st, vg, eps, L)
        moved = np.abs(run["traj_pos"][j] - prev).max(1) > 0
        tol = 5e-6 * max(1.0, np.abs(lp).max())
        border = np.abs(u - info.acceptance_rate) < 10 * tol * np.maximum(info.acceptance_rate, 1e-30) + 1e-6
        assert (moved == info.is_accepted)[~border].all(), j
        ref_x = np.where(moved[:, None], info.proposed_position, x)
        ref_lp = np.where(moved, vg(info.proposed_position)[0], lp)
        e = np.abs(run["traj_pos"][j].astype(np.float64) - ref_x).max()
        e_lp = np.abs(run["traj_logp"][j] - ref_lp).max()
        print(f"step {j}: |x - oracle| {e:.3g}, |logp - oracle| {e_lp:.3g}, accepted {moved.sum()}, borderline {border.sum()}")
        assert e < 3e-6 * max(1.0, np.abs(ref_x).max()), (j, e)
        assert e_lp < max(2e-6 * max(1.0, np.abs(ref_lp).max()), f32_lp), (j, e_lp)
        p_sum += info.acceptance_rate
        tol_sum += max(tol + 1e-5, f32_p)
        seen |= set(moved.tolist())
        prev = run["traj_pos"][j]
        if j == n_steps - 1:
            err_p = np.abs(np.log(np.maximum(run["acc"].astype(np.float64), 1e-30)) - np.log(np.maximum(info.acceptance_rate, 1e-30))).max()
            print(f"last step: |log p - oracle| {err_p:.3g} (tol {max(tol + 1e-5, f32_p):.3g})")
            assert err_p < max(tol + 1e-5, f32_p)
            np.testing.assert_array_equal(run["isacc"].astype(bool), moved)
    assert seen == {True, False}, seen
    np.testing.assert_array_equal(run["n_acc"], (np.abs(np.diff(np.concatenate([pos0.cpu().numpy()[None], run["traj_pos"]]), axis=0)).max(-1) > 0).sum(0))
    # p = min(1, exp(delta)) with delta within a step's tol of the oracle's: each term of the sum is within e^tol - 1 <= 2 tol of it
    np.testing.assert_allclose(run["acc_sum"], p_sum, rtol=0, atol=2 * tol_sum)
    np.testing.assert_array_equal(run["pos"], run["traj_pos"][-1])
    np.testing.assert_array_equal(run["logp"], run["traj_logp"][-1])
    ctx.close()


def test_thinning_and_no_trajectory():
    kind, d, tail, beta, eps = CASES["phi4_d100"]
    ctx, pos0, _ = _ctx(kind, d, tail)
    state0 = _init(ctx, pos0, beta)
    key = prng.PRNGKey(21)
    full = _run(ctx, state0, key, beta, eps, N_STEPS, 1)
    thinned = _run(ctx, state0, key, beta, eps, N_STEPS, 2)
    assert thinned["traj_pos"].shape == (3, B, d) and thinned["traj_logp"].shape == (3, B)
    np.testing.assert_array_equal(thinned["traj_pos"], full["traj_pos"][[1, 3, 5]])
    np.testing.assert_array_equal(thinned["traj_logp"], full["traj_logp"][[1, 3, 5]])
    none = _run(ctx, state0, key, beta, eps, N_STEPS, 0, traj=False)           # thin = 0, null trajectory pointers
    for r in (thinned, none):
        for name in ("pos", "logp", "grad", "n_acc", "acc_sum", "acc", "isacc"):
            np.testing.assert_array_equal(r[name], full[name], err_msg=name)
    assert 0 < full["n_acc"].sum() < N_STEPS * B
    ctx.close()


def _gmm_engine(n):
    import torch
    from mfm_amd import distributions as D
    from mfm_amd.engine import Engine
    from tests import gpu_util as gu
    args, odist, k, model, state = gu.gmm4_setup(B=n)
    dist = D.GaussianMixture(odist.modes, odist.covs, odist.weights)
    args.ot_cond_flow = False
    eng = Engine(dist, args, model.f)
    return eng, dist, torch.as_tensor(odist.init_params.astype(np.float32)).cuda()


def test_api_run_and_inference_loop0():
    """``hmc(logdensity_fn, eps, L).step.run`` and ``inference_loop0`` on the same key: the stacked states ARE the thin = 1 trajectory,
    and both equal ``inference_loop0``'s host loop (the same kernel with ``.run`` removed) bit for bit."""
    from mfm_amd import mcmc_utils, random as jr
    from mfm_amd.bblackjax.mcmc.hmc import HMCInfo, HMCRunInfo, HMCState, hmc
    eng, dist, pos = _gmm_engine(B)
    algo = hmc(dist.logprob, CASES["gmm4"][4], L)
    state = algo.init(pos)
    key = jr.PRNGKey(6)
    before = [t.clone() for t in state]
    new, info = algo.step.run(key, state, N_STEPS, thin=1)
    assert isinstance(new, HMCState) and isinstance(info, HMCRunInfo) and isinstance(info.last, HMCInfo)
    assert info.positions.shape == (N_STEPS, B, 2) and info.logdensities.shape == (N_STEPS, B)
    for t, b in zip(state, before):
        assert (t == b).all()                                                  # functional: the input state is not modified
    states, info0 = mcmc_utils.inference_loop0(key, state, algo.step, N_STEPS)
    assert isinstance(info0, HMCRunInfo) and states.logdensity_grad is None
    np.testing.assert_array_equal(states.position.cpu().numpy(), info.positions.cpu().numpy())
    np.testing.assert_array_equal(states.logdensity.cpu().numpy(), info.logdensities.cpu().numpy())
    np.testing.assert_array_equal(states.position[-1].cpu().numpy(), new.position.cpu().numpy())
    traj = np.concatenate([state.position.cpu().numpy()[None], info.positions.cpu().numpy()])
    changes = (np.abs(np.diff(traj, axis=0)).max(-1) > 0).sum(0)
    np.testing.assert_array_equal(info.num_accepted.cpu().numpy(), changes)
    assert 0 < changes.sum() < N_STEPS * B
    # the host loop: the same step function without .run
    plain = lambda k, s: algo.step(k, s)
    assert getattr(plain, "run", None) is None
    h_states, h_infos = mcmc_utils.inference_loop0(key, state, plain, N_STEPS)
    np.testing.assert_array_equal(h_states.position.cpu().numpy(), info.positions.cpu().numpy())
    np.testing.assert_array_equal(h_states.logdensity.cpu().numpy(), info.logdensities.cpu().numpy())
    np.testing.assert_array_equal(h_infos.is_accepted.sum(0).cpu().numpy(), info.num_accepted.cpu().numpy())
    np.testing.assert_array_equal(h_infos.acceptance_rate[-1].cpu().numpy(), info.last.acceptance_rate.cpu().numpy())
    np.testing.assert_array_equal(h_infos.is_accepted[-1].cpu().numpy(), info.last.is_accepted.cpu().numpy())
    # the launches report float32 probabilities: 2^-24 relative per term, and 2^-150 absolute where a tiny one lands among the denormals
    np.testing.assert_allclose(info.acceptance_rate.cpu().numpy(), h_infos.acceptance_rate.double().sum(0).cpu().numpy() / N_STEPS,
                               rtol=2.0 ** -24 + (N_STEPS + 1) * 2.0 ** -52, atol=2.0 ** -150)
    # per-chain keys through the kernel API: the run on keys[b] against the kernel looped over split_rows(keys, n)[:, j]
    keys = jr.split(jr.PRNGKey(7), B)
    _, info_k = algo.step.run(keys, state, N_STEPS, thin=1)
    st = state
    for j in range(N_STEPS):
        st, _ = algo.step(jr.split_rows(keys, N_STEPS)[:, j], st)
        np.testing.assert_array_equal(st.position.cpu().numpy(), info_k.positions[j].cpu().numpy())
    no_traj = algo.step.run(key, state, N_STEPS)[1]
    assert no_traj.positions is None and no_traj.logdensities is None
    eng.close()


def test_argument_errors_name_the_argument():
    import torch
    from mfm_amd import _lib
    ctx, pos0, _ = _ctx("phi4", 64, None)
    pos, logp, grad = _init(ctx, pos0, 1.0)
    key = prng.PRNGKey(1)
    tp = torch.empty(4, B, 64, device="cuda")
    before = pos.clone()
    with pytest.raises(_lib.MfmError, match="n_steps"):
        ctx.hmc_run(key, 1.0, 1e-2, L, 0, pos, logp, grad)
    with pytest.raises(_lib.MfmError, match="num_steps"):
        ctx.hmc_run(key, 1.0, 1e-2, 0, 4, pos, logp, grad)
    with pytest.raises(_lib.MfmError, match="thin"):
        ctx.hmc_run(key, 1.0, 1e-2, L, 4, pos, logp, grad, thin=-1, traj_pos=tp)
    with pytest.raises(_lib.MfmError, match="thin .* n_steps"):
        ctx.hmc_run(key, 1.0, 1e-2, L, 4, pos, logp, grad, thin=3, traj_pos=tp)
    with pytest.raises(_lib.MfmError, match="d_traj_pos"):
        ctx.hmc_run(key, 1.0, 1e-2, L, 4, pos, logp, grad, thin=2)
    with pytest.raises(_lib.MfmError, match="key_mode"):
        ctx.hmc_run(key, 1.0, 1e-2, L, 4, pos, logp, grad, key_mode=2)
    with pytest.raises(_lib.MfmError, match="d_keys"):
        ctx.hmc_run(key, 1.0, 1e-2, L, 4, pos, logp, grad, key_mode=1)
    with pytest.raises(_lib.MfmError, match="step_size"):
        ctx.hmc_run(key, 1.0, 0.0, L, 4, pos, logp, grad)
    with pytest.raises(_lib.MfmError, match="num_steps"):
        ctx.hmc_step_keys(_keys_dev(prng.split(key, B)), 1.0, 1e-2, 0, pos, logp, grad)
    with pytest.raises(_lib.MfmError, match="key"):
        ctx.hmc_step_keys(None, 1.0, 1e-2, L, pos, logp, grad)
    assert torch.equal(pos, before)                                            # a rejected call touches nothing
    ctx.close()
    cox, cpos0, _ = _ctx("lgcp", 16, None)
    cpos, clogp, cgrad = _init(cox, cpos0, 1.0)
    with pytest.raises(_lib.MfmError, match="Cox"):
        cox.hmc_run(key, 1.0, 1e-2, L, 4, cpos, clogp, cgrad)
    with pytest.raises(_lib.MfmError, match="Cox"):
        cox.hmc_step_keys(_keys_dev(prng.split(key, B)), 1.0, 1e-2, L, cpos, clogp, cgrad)
    cox.close()


def test_ess_steps_with_the_hmc_kernel():
    """``--ess_steps`` under ``--mcmc_kernel hmc``: the figures belong to HMC steps of ``--hmc_steps`` leapfrog steps (recomputed here
    from ``hmc(...).step.run`` on the same final chains and key), and come per gradient evaluation too; MALA keeps its three keys."""
    from mfm_amd import distributions as D, exe_flow_matching as E, mcmc_utils, random as jr
    from mfm_amd.bblackjax.mcmc.hmc import hmc
    from oracle import loop
    kw = dict(example="phi-four", dim=64, num_chain=32, learning_iter=5, mcmc_per_flow_steps=4.0, hutchs=True, fourier_dim=16, seed=7, eval_iter=1,
              step_size=0.03, hidden_x=[32, 32], hidden_t=[32, 32], hidden_xt=[32, 32], ess_steps=64)
    step_keys = ["ess_per_step_min", "ess_per_step_median", "ess_per_step_mean"]
    grad_keys = ["ess_per_grad_min", "ess_per_grad_median", "ess_per_grad_mean"]
    dist = D.PhiFour(64)
    args = loop.default_args(mcmc_kernel="hmc", hmc_steps=4, **kw)
    _, _, ex = E.run(dist, args, None, log_every=1000, return_extras=True)
    eng = ex["engine"]
    for ks, kg in zip(step_keys, grad_keys):
        assert isinstance(ex[ks], float) and np.isfinite(ex[ks])               # (Geyer's tau, and with it the ESS, is negative for an antithetic chain)
        assert ex[kg] == ex[ks] / 4                                            # bit for bit in float64
    algo = hmc(dist.logprob, args.step_size, 4)
    _, info = algo.step.run(jr.split(ex["key_gen"], 3)[2], algo.init(ex["states"].position), 64, thin=1)
    ess, _ = mcmc_utils.effective_sample_size(info.positions[:, :eng.n_valid], ctx=eng.ctx)
    per_step = (ess.double() / 64).reshape(-1)
    assert ex["ess_per_step_min"] == per_step.min().item()
    assert ex["ess_per_step_median"] == per_step.median().item()
    assert ex["ess_per_step_mean"] == per_step.mean().item()
    assert 0 < info.num_accepted.sum().item()                                  # the chains moved: the figures are of a trajectory
    eng.close()
    _, _, ex_m = E.run(D.PhiFour(64), loop.default_args(mcmc_kernel="mala", **dict(kw, step_size=1e-4)), None, log_every=1000, return_extras=True)
    assert all(k in ex_m for k in step_keys) and not any(k in ex_m for k in grad_keys)
    ex_m["engine"].close()
