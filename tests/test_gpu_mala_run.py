"""GPU tests of ``mfm_mala_run`` (mfm_amd/csrc/mala_run.hip): many MALA steps in one launch with the chain resident in registers.

The yardstick is the single-step kernel: a run of n steps must give the BITS of n launches of ``mfm_mala_step`` /
``mfm_mala_step_keys`` on the step keys the run derives (step-major: ``split(key, n)[j]``; chain-major: ``split_rows(keys, n)[:, j]``),
for every kernel instance (MAXIT 1 / 4 / 16 / 32, each with the run-time boundary, the mixture path), plus one comparison with the float64 oracle
at the tolerances stated for the MALA tests (docs/HISTORY.md section 2), the Cox process (a loop of its tile step inside the library),
the SMC move that uses the run, the Python API and the argument errors.

Step sizes: chosen with the float64 oracle (oracle/mala.py on the same initial positions, 48 chains, 7 steps) so that the mean
acceptance probability lies well inside (0.1, 0.9) -- both branches of the accept select are taken; the tests assert that window.
(The acceptance rule AS WRITTEN rejects more with growing step, so the phi-four steps are small: oracle means 0.52 at d = 64 with
4e-5, 0.38 at d = 100 with 2e-5, 0.36 at d = 256 with 3e-6, 0.52 periodic, 0.58 on the 8 x 8 lattice with 4e-4, 0.53 at beta = 0.3
with 2.5e-4, 0.29 on the 4-mode mixture with 0.2; the textbook rule on the mixture: 0.71 with 1.5.)"""
import numpy as np
import pytest

from oracle import mala as omala, prng, targets
from tests import row_instance_cases as rc

pytestmark = pytest.mark.gpu

B, N_STEPS = 48, 7

# name: (target, d, phi-four block tail {kind, b[, dim_phys]} or None, beta, step size, textbook)
CASES = {
    "phi4_d64": ("phi4", 64, None, 1.0, 4e-5, False),
    "phi4_d100": ("phi4", 100, None, 1.0, 2e-5, False),
    "phi4_d256": ("phi4", 256, None, 1.0, 3e-6, False),
    "phi4_d64_pbc": ("phi4", 64, [1.0, 0.0], 1.0, 4e-5, False),
    "phi4_8x8_dirichlet": ("phi4", 64, [0.0, 0.7, 2.0], 1.0, 4e-4, False),
    "gmm4": ("gmm", 2, None, 1.0, 0.2, False),
    "phi4_d64_beta03": ("phi4", 64, None, 0.3, 2.5e-4, False),
    "gmm4_textbook": ("gmm", 2, None, 1.0, 1.5, True),
}
# The dispatch instances above d = 256 (and MAXIT 4 with a run-time boundary), which tie mala_run_kernel and the warmup kernel there to the
# step kernel that tests/test_gpu_row_instances.py holds to the oracle: target "row", the case of tests/row_instance_cases.py in the place
# of d -- its start state near a mode (16 chains), its boundary and its step sizes (beta = 1 as written; beta = 0.37 textbook, which the
# warmup tests take), ROW_STEPS steps.  Oracle means of the acceptance probability over the 5 steps: 0.45 ... 0.75 as written, 0.33 ...
# 0.67 textbook.  (MAXIT, BCRT): d65_pbc (4, true), d257_d0 (16, false), 17x17_pbc (16, true), d2048_d0 (32, false), d1025_pbc and
# 33x33_db (32, true).
ROW_STEPS = 5
ROW_CASES = ("d65_pbc", "d257_d0", "17x17_pbc", "d2048_d0", "d1025_pbc", "33x33_db")
for _c in ROW_CASES:
    CASES["row_" + _c] = ("row", _c, None, 1.0, rc.STEP_SIZES[_c]["mala"]["b1"], False)
    CASES["row_" + _c + "_textbook"] = ("row", _c, None, 0.37, rc.STEP_SIZES[_c]["mala"]["b037_textbook"], True)


def _n_steps(case):
    return ROW_STEPS if CASES[case][0] == "row" else N_STEPS


def _ctx(kind, d, tail, n=B):
    """A context on the target and the initial positions (float32, on the device)."""
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


def _info_buffers(n, d):
    import torch
    return (torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, d, device="cuda"),
            torch.empty(n, device="cuda"))


def _stepwise(ctx, state0, key, beta, eps, n_steps, textbook=False):
    """n single-step launches on the run's step keys; the state after, and the info of, every launch (numpy)."""
    from mfm_amd import random as jr
    pos, logp, grad = (t.clone() for t in state0)
    n, d = pos.shape
    acc, isacc, prop, w = _info_buffers(n, d)
    per_chain = np.ndim(key) == 2
    step_keys = jr.split_rows(key, n_steps) if per_chain else jr.split(key, n_steps)
    out = dict(pos=[], logp=[], grad=[], acc=[], isacc=[], prop=[], w=[])
    for j in range(n_steps):
        if per_chain:
            ctx.mala_step_keys(_keys_dev(step_keys[:, j]), beta, eps, pos, logp, grad, acc, isacc, prop, w, textbook=textbook)
        else:
            ctx.mala_step(step_keys[j], beta, eps, pos, logp, grad, acc, isacc, prop, w, textbook=textbook)
        for name, t in zip(out, (pos, logp, grad, acc, isacc, prop, w)):
            out[name].append(t.cpu().numpy().copy())
    return {k: np.stack(v) for k, v in out.items()}


def _keys_dev(keys):
    import torch
    return torch.as_tensor(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32)).cuda()


def _run(ctx, state0, key, beta, eps, n_steps, thin, textbook=False, traj=True):
    import torch
    pos, logp, grad = (t.clone() for t in state0)
    n, d = pos.shape
    acc, isacc, prop, w = _info_buffers(n, d)
    n_acc = torch.empty(n, dtype=torch.int32, device="cuda"); acc_sum = torch.empty(n, dtype=torch.float64, device="cuda")
    tp = tl = None
    if traj and thin > 0:
        tp = torch.empty(n_steps // thin, n, d, device="cuda"); tl = torch.empty(n_steps // thin, n, dtype=torch.float64, device="cuda")
    ctx.mala_run(_keys_dev(key) if np.ndim(key) == 2 else key, beta, eps, n_steps, pos, logp, grad, thin=thin, n_acc=n_acc, acc_sum=acc_sum,
                 acc=acc, is_acc=isacc, proposed=prop, weight=w, traj_pos=tp, traj_logp=tl, textbook=textbook)
    names = ("pos", "logp", "grad", "acc", "isacc", "prop", "w", "n_acc", "acc_sum", "traj_pos", "traj_logp")
    return {k: (None if t is None else t.cpu().numpy()) for k, t in zip(names, (pos, logp, grad, acc, isacc, prop, w, n_acc, acc_sum, tp, tl))}


def _assert_run_equals_steps(run, steps, window=True):
    """The run with thin = 1 against the launches, bit for bit (the sum of the acceptance probabilities to float32 rounding)."""
    p_mean = steps["acc"].astype(np.float64).mean()
    print(f"mean acceptance probability {p_mean:.4f}, accepted fraction {steps['isacc'].mean():.4f}")
    if window:
        assert 0.1 < p_mean < 0.9, p_mean                                      # both branches of the select are exercised
        assert 0 < steps["isacc"].sum() < steps["isacc"].size
    for name in ("pos", "logp", "grad"):
        np.testing.assert_array_equal(run[name], steps[name][-1], err_msg=name)
    np.testing.assert_array_equal(run["traj_pos"], steps["pos"])
    np.testing.assert_array_equal(run["traj_logp"], steps["logp"])
    np.testing.assert_array_equal(run["n_acc"], steps["isacc"].astype(np.int64).sum(0))
    for name in ("acc", "isacc", "prop", "w"):
        np.testing.assert_array_equal(run[name], steps[name][-1], err_msg="last " + name)
    np.testing.assert_allclose(run["acc_sum"], steps["acc"].astype(np.float64).sum(0), rtol=1e-6)


@pytest.mark.parametrize("case", list(CASES))
def test_run_is_bit_identical_with_single_step_launches(case):
    kind, d, tail, beta, eps, textbook = CASES[case]
    ctx, pos0, _ = _ctx(kind, d, tail)
    state0 = _init(ctx, pos0, beta)
    key = prng.PRNGKey(21)
    steps = _stepwise(ctx, state0, key, beta, eps, _n_steps(case), textbook)
    run = _run(ctx, state0, key, beta, eps, _n_steps(case), 1, textbook)
    _assert_run_equals_steps(run, steps)
    ctx.close()


@pytest.mark.parametrize("case", ["phi4_d64", "gmm4"])
def test_chain_major_keys(case):
    """key_mode 1: step j of chain b draws from split(keys[b], n)[j], what mfm_mala_step_keys draws from split_rows(keys, n)[:, j]."""
    kind, d, tail, beta, eps, textbook = CASES[case]
    ctx, pos0, _ = _ctx(kind, d, tail)
    state0 = _init(ctx, pos0, beta)
    keys = prng.split(prng.PRNGKey(33), B)
    steps = _stepwise(ctx, state0, keys, beta, eps, N_STEPS)
    run = _run(ctx, state0, keys, beta, eps, N_STEPS, 1)
    _assert_run_equals_steps(run, steps)
    ctx.close()


def test_thinning_and_no_trajectory():
    kind, d, tail, beta, eps, textbook = CASES["phi4_d100"]
    ctx, pos0, _ = _ctx(kind, d, tail)
    state0 = _init(ctx, pos0, beta)
    key = prng.PRNGKey(8)
    full = _run(ctx, state0, key, beta, eps, 12, 1)
    thinned = _run(ctx, state0, key, beta, eps, 12, 4)
    assert thinned["traj_pos"].shape == (3, B, d) and thinned["traj_logp"].shape == (3, B)
    np.testing.assert_array_equal(thinned["traj_pos"], full["traj_pos"][[3, 7, 11]])
    np.testing.assert_array_equal(thinned["traj_logp"], full["traj_logp"][[3, 7, 11]])
    none = _run(ctx, state0, key, beta, eps, 12, 0, traj=False)                # thin = 0, null trajectory pointers
    for r in (thinned, none):
        for name in ("pos", "logp", "grad", "n_acc", "acc_sum", "acc", "isacc", "prop", "w"):
            np.testing.assert_array_equal(r[name], full[name], err_msg=name)
    assert 0 < full["n_acc"].sum() < 12 * B
    ctx.close()


ORACLE_SEED = 4      # the first seed whose 80 decisions all have |u - p| > 1e-2 in the float64 oracle (asserted below)


ORACLE_SEED_D1025 = 0      # the first seed with the same property for the d = 1025 periodic case


def test_run_matches_the_float64_oracle():
    """phi-four d = 64, 16 chains, 5 steps from ``oracle.mala.init``: the oracle's kernel looped over split(key, 5)[j] -> split(., 16).
    Tolerances of the MALA tests (docs/HISTORY.md section 2; the several-step forms of tests/test_gpu_mala_api.py): proposal 1e-6,
    acceptance probability 5e-3, decisions identical -- every chain: the seed keeps all 80 decisions off the knife edge."""
    _run_against_the_oracle("phi4", 64, 4e-5, ORACLE_SEED)


def test_run_matches_the_float64_oracle_at_d1025():
    """The same comparison on the MAXIT 32 run-time-boundary instance: the periodic chain of d = 1025 from its start state near a mode
    (tests/row_instance_cases.py), at that table's step size."""
    _run_against_the_oracle("row", "d1025_pbc", rc.STEP_SIZES["d1025_pbc"]["mala"]["b1"], ORACLE_SEED_D1025)


def _run_against_the_oracle(kind, d, eps, seed):
    import torch
    n, n_steps, beta = 16, 5, 1.0
    ctx, pos0, dist = _ctx(kind, d, None, n=n)
    vg = targets.Tempered(dist, beta).value_and_grad
    st = omala.init(pos0.cpu().numpy().astype(np.float64), vg)
    state0 = (pos0.clone(), torch.as_tensor(st.logdensity).cuda(), torch.as_tensor(st.logdensity_grad.astype(np.float32)).cuda())
    key = prng.PRNGKey(seed)
    o_pos, o_logp, o_p, o_acc, margin = [], [], [], [], []
    for j in range(n_steps):
        st, info, u = omala.kernel(prng.split(prng.split(key, n_steps)[j], n), st, vg, eps)
        o_pos.append(st.position); o_logp.append(st.logdensity); o_p.append(info.acceptance_rate); o_acc.append(info.is_accepted)
        margin.append(np.abs(u - info.acceptance_rate))
    assert np.min(margin) > 1e-2, np.min(margin)                               # no decision on a knife edge: no chain is left out
    assert 0 < np.sum(o_acc) < n * n_steps
    run = _run(ctx, state0, key, beta, eps, n_steps, 1)
    print("max |p_last - oracle|", np.abs(run["acc"] - o_p[-1]).max(), "max |traj - oracle|", np.abs(run["traj_pos"] - np.stack(o_pos)).max())
    np.testing.assert_array_equal(run["n_acc"], np.sum(o_acc, 0))              # decisions identical ...
    np.testing.assert_array_equal(run["isacc"].astype(bool), o_acc[-1])
    moved = np.abs(np.diff(np.concatenate([pos0.cpu().numpy()[None], run["traj_pos"]]), axis=0)).max(-1) > 0
    np.testing.assert_array_equal(moved, np.stack(o_acc))                      # ... at every step
    # "Proposal 1e-6" is the stated tolerance of the MALA tests (docs/HISTORY.md section 2) in the form those tests give it
    # (tests/test_gpu_mala_api.py: rtol = 1e-6 with atol = 1e-6): relative to the field's scale, which is O(1).  The absolute term is
    # not slack: the state is float32 by the data layout and the oracle float64, so an element carries up to 2^-24 |x| ~ 6e-8 of
    # rounding, and where the noise cancels the position (|x'| << |x|) no bound relative to |x'| itself can hold -- measured on an
    # MI355X: an error of 1.9e-5 of |x'| at such an element, while no element of the trajectory is off by more than 1.05e-7.
    err = np.abs(run["prop"] - info.proposed_position)
    print("proposal: max |x' - oracle|", err.max(), "max relative to |x'|", (err / np.abs(info.proposed_position)).max())
    np.testing.assert_allclose(run["prop"], info.proposed_position, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(run["acc"], o_p[-1], rtol=5e-3, atol=5e-3)
    np.testing.assert_allclose(run["acc_sum"] / n_steps, np.mean(o_p, 0), rtol=5e-3, atol=5e-3)
    np.testing.assert_allclose(run["traj_pos"], np.stack(o_pos), rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(run["traj_logp"], np.stack(o_logp), rtol=2e-6, atol=5e-3)      # (the several-step form of test_gpu_mala_api.py)
    ctx.close()


def test_cox_process_run_equals_its_step_launches():
    """The Cox process: n launches of the 16-chain tile step inside the library, keys derived on the device -- 4 x 4 grid, 16 chains."""
    ctx, pos0, _ = _ctx("lgcp", 16, None, n=16)
    beta, eps = 0.45, 0.01
    state0 = _init(ctx, pos0, beta)
    for key in (prng.PRNGKey(3), prng.split(prng.PRNGKey(4), 16)):            # step-major, chain-major
        steps = _stepwise(ctx, state0, key, beta, eps, 3)
        run = _run(ctx, state0, key, beta, eps, 3, 1)
        _assert_run_equals_steps(run, steps, window=False)
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


def test_smc_step_with_the_run_equals_the_stepwise_loop(monkeypatch):
    """One tempered SMC step (32 particles, 5 MCMC steps per temperature): the move as ONE mfm_mala_run with the per-particle keys
    against the Python loop of single-step launches (MFM_SMC_STEPWISE=1) -- particles, weights and the last info bit for bit."""
    from mfm_amd.bblackjax.mcmc import mala
    from mfm_amd.bblackjax.smc import base as smc_base, resampling, tempered
    eng, dist, pos = _gmm_engine(32)
    smc_base.attach(eng)
    algo = tempered.tempered_smc(dist.logprior, dist.loglik, mala.build_kernel(), mala.init, dict(step_size=0.2), resampling.systematic,
                                 num_mcmc_steps=5)
    s0 = algo.init(pos)
    s0 = tempered.TemperedSMCState(s0.particles, s0.weights, 0.4)            # the move targets logprior + 0.4 loglik
    calls = []
    real_run = eng.ctx.mala_run
    monkeypatch.setattr(eng.ctx, "mala_run", lambda *a, **k: (calls.append(1), real_run(*a, **k))[1])
    res = []
    for stepwise in ("1", "0"):
        monkeypatch.setenv("MFM_SMC_STEPWISE", stepwise)
        state, info = algo.step(prng.PRNGKey(17), s0, 0.7)
        res.append((state, info))
    assert len(calls) == 1                                                     # the loop made none, the run path exactly one
    (sa, ia), (sb, ib) = res
    assert sa.lmbda == sb.lmbda == 0.7
    np.testing.assert_array_equal(sa.particles.cpu().numpy(), sb.particles.cpu().numpy())
    np.testing.assert_array_equal(sa.weights.cpu().numpy(), sb.weights.cpu().numpy())
    np.testing.assert_array_equal(ia.ancestors.cpu().numpy(), ib.ancestors.cpu().numpy())
    assert ia.log_likelihood_increment == ib.log_likelihood_increment
    for name in mala.MALAInfo._fields:
        np.testing.assert_array_equal(getattr(ia.update_info, name).cpu().numpy(), getattr(ib.update_info, name).cpu().numpy(), err_msg=name)
    assert (sa.particles != s0.particles).any()
    smc_base.attach(None)
    eng.close()


def test_api_run_and_inference_loop0():
    """``mala(logdensity_fn, eps).step.run`` and ``inference_loop0`` on the same key: the stacked states ARE the thin = 1 trajectory, and
    both equal the host loop of ``step`` over split(key, 6)."""
    from mfm_amd import mcmc_utils, random as jr
    from mfm_amd.bblackjax.mcmc.mala import MALARunInfo, MALAState, mala
    eng, dist, pos = _gmm_engine(B)
    algo = mala(dist.logprob, 0.2)
    state = algo.init(pos)
    key = jr.PRNGKey(6)
    before = state.position.clone()
    new, info = algo.step.run(key, state, 6, thin=1)
    assert isinstance(new, MALAState) and isinstance(info, MALARunInfo) and info.positions.shape == (6, B, 2)
    assert (state.position == before).all()                                   # functional: the input state is not modified
    states, info0 = mcmc_utils.inference_loop0(key, state, algo.step, 6)
    assert states.logdensity_grad is None
    np.testing.assert_array_equal(states.position.cpu().numpy(), info.positions.cpu().numpy())
    np.testing.assert_array_equal(states.logdensity.cpu().numpy(), info.logdensities.cpu().numpy())
    np.testing.assert_array_equal(states.position[-1].cpu().numpy(), new.position.cpu().numpy())
    np.testing.assert_array_equal(info0.acceptance_rate.cpu().numpy(), info.acceptance_rate.cpu().numpy())
    # acceptance_rate = acc_sum / 6 and the trajectory, against the kernel looped on the host
    st, ps, accs, traj = state, [], [], []
    for k in jr.split(key, 6):
        st, inf = algo.step(k, st)
        traj.append(st.position.cpu().numpy()); ps.append(inf.acceptance_rate.cpu().numpy().astype(np.float64)); accs.append(inf.is_accepted.cpu().numpy())
    np.testing.assert_array_equal(info.positions.cpu().numpy(), np.stack(traj))
    np.testing.assert_array_equal(info.num_accepted.cpu().numpy(), np.sum(accs, 0))
    np.testing.assert_allclose(info.acceptance_rate.cpu().numpy(), np.sum(ps, 0) / 6, rtol=1e-6)
    for name in ("acceptance_rate", "is_accepted", "proposed_position", "proposed_weight"):
        np.testing.assert_array_equal(getattr(info.last, name).cpu().numpy(), getattr(inf, name).cpu().numpy(), err_msg=name)
    no_traj = algo.step.run(key, state, 6)[1]
    assert no_traj.positions is None and no_traj.logdensities is None
    with pytest.raises(NotImplementedError):
        algo.step.run(key, MALAState(state.position[0], state.logdensity[0], state.logdensity_grad[0]), 6)
    eng.close()


def test_argument_errors_name_the_argument():
    import torch
    from mfm_amd import _lib
    ctx, pos0, _ = _ctx("phi4", 64, None, n=16)
    pos, logp, grad = _init(ctx, pos0, 1.0)
    key = prng.PRNGKey(1)
    tp = torch.empty(4, 16, 64, device="cuda")
    before = pos.clone()
    with pytest.raises(_lib.MfmError, match="n_steps"):
        ctx.mala_run(key, 1.0, 1e-4, 0, pos, logp, grad)
    with pytest.raises(_lib.MfmError, match="thin"):
        ctx.mala_run(key, 1.0, 1e-4, 4, pos, logp, grad, thin=-1, traj_pos=tp)
    with pytest.raises(_lib.MfmError, match="thin .* n_steps"):
        ctx.mala_run(key, 1.0, 1e-4, 4, pos, logp, grad, thin=3, traj_pos=tp)
    with pytest.raises(_lib.MfmError, match="d_traj_pos"):
        ctx.mala_run(key, 1.0, 1e-4, 4, pos, logp, grad, thin=2)
    with pytest.raises(_lib.MfmError, match="key_mode"):
        ctx.mala_run(key, 1.0, 1e-4, 4, pos, logp, grad, key_mode=2)
    with pytest.raises(_lib.MfmError, match="d_keys"):
        ctx.mala_run(key, 1.0, 1e-4, 4, pos, logp, grad, key_mode=1)
    for bad in (0.0, -1e-4, float("nan")):
        with pytest.raises(_lib.MfmError, match="step_size must be positive"):
            ctx.mala_run(key, 1.0, bad, 4, pos, logp, grad)
    assert torch.equal(pos, before)                                            # a rejected call touches nothing
    ctx2 = _lib.Context(dim=64, n_chain_local=16)
    with pytest.raises(_lib.MfmError, match="mfm_set_target"):
        ctx2.mala_run(key, 1.0, 1e-4, 4, pos, logp, grad)
    ctx2.close()
    ctx.close()
