"""GPU tests of ``mfm_mclmc_init`` / ``_step`` / ``_step_keys`` / ``_run`` (mfm_amd/csrc/mclmc.hip), ``bblackjax.mclmc``,
``mclmc_find_L_and_step_size`` and ``--mcmc_kernel mclmc``.

The yardstick of a step is tests/mclmc_ref.py, the float64 restatement, restarted at every step from the device's state (float32
position, float64 momentum); the tolerance is the larger of the existing HMC tests' forms -- 5e-6 max(1, |logp|) for energies,
4 * 2^-23 max(1, |x|) for positions and the momentum -- and 4 x what the device's number formats cost between the two restatements
(``mclmc_cases.F32_DISTANCE``, derived on the CPU).  The yardstick of the run is the single-step kernel, bit for bit.  Cases, start
states and step sizes: tests/mclmc_cases.py (16 chains, every dispatch instance)."""
import numpy as np
import pytest

from oracle import prng
from tests import mclmc_cases as mc
from tests import mclmc_ref as ref
from tests import row_instance_cases as rc

pytestmark = pytest.mark.gpu

B = mc.N_CHAINS
RUN_STEPS = 4


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _keys_dev(keys):
    return _dev(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32))


def _ctx(case, n_local=B, n_total=None, offset=None):
    """A context on the case's target and its start state on the device."""
    from mfm_amd import _lib
    from tests import gpu_util as gu
    tot, off = mc.shard(case)
    n_total, offset = tot if n_total is None else n_total, off if offset is None else offset
    if case == "gmm4":
        args, dist, *_ = gu.gmm4_setup(B=n_local)
        ctx = gu.make_ctx(dist, args, n_local=n_local, n_total=n_total, offset=offset)
    else:
        args, dist0, *_ = gu.phi4_setup(d=mc.dim(case), B=n_local, hidden=32, F=16)
        ctx = gu.make_ctx(dist0, args, n_local=n_local, n_total=n_total, offset=offset)
        if rc.block(case) is not None:
            ctx.set_target(_lib.PHI4, rc.block(case))
    return ctx, _dev(mc.start_state(case))


def _init(ctx, pos0, key):
    """(pos, logp, grad, momentum) on the device: ``mfm_mala_init`` at beta = 1 and ``mfm_mclmc_init``."""
    import torch
    pos = pos0.clone()
    logp = torch.empty(pos.shape[0], dtype=torch.float64, device="cuda"); grad = torch.empty_like(pos)
    mom = torch.empty(pos.shape, dtype=torch.float64, device="cuda")
    ctx.mala_init(pos, 1.0, logp, grad)
    ctx.mclmc_init(key, mom)
    return pos, logp, grad, mom


def _np(state):
    return tuple(t.cpu().numpy().copy() for t in state)


def _L(case):
    return float(np.sqrt(mc.dim(case)))


def _stepwise(ctx, state0, key, eps, L, integrator, n_steps):
    """n single-step launches on the run's step keys: the state after, and dE / dK of, every launch (numpy)."""
    import torch
    from mfm_amd import random as jr
    st = tuple(t.clone() for t in state0)
    n = st[0].shape[0]
    de = torch.empty(n, dtype=torch.float64, device="cuda"); dk = torch.empty_like(de)
    per_chain = np.ndim(key) == 2
    step_keys = jr.split_rows(key, n_steps) if per_chain else jr.split(key, n_steps)
    out = dict(pos=[], logp=[], grad=[], mom=[], de=[], dk=[])
    for j in range(n_steps):
        if per_chain:
            ctx.mclmc_step_keys(_keys_dev(step_keys[:, j]), 1.0, eps, L, integrator, *st, de, dk)
        else:
            ctx.mclmc_step(step_keys[j], 1.0, eps, L, integrator, *st, de, dk)
        for name, t in zip(out, st + (de, dk)):
            out[name].append(t.cpu().numpy().copy())
    return {k: np.stack(v) for k, v in out.items()}


def _run(ctx, state0, key, eps, L, integrator, n_steps, thin, traj=True, trace=True):
    import torch
    st = tuple(t.clone() for t in state0)
    n, d = st[0].shape
    s1 = torch.empty(n, dtype=torch.float64, device="cuda"); s2 = torch.empty_like(s1)
    bad = torch.empty(n, dtype=torch.int32, device="cuda")
    tr = torch.empty(n_steps, n, dtype=torch.float64, device="cuda") if trace else None
    tp = tl = None
    if traj and thin > 0:
        tp = torch.empty(n_steps // thin, n, d, device="cuda"); tl = torch.empty(n_steps // thin, n, dtype=torch.float64, device="cuda")
    ctx.mclmc_run(_keys_dev(key) if np.ndim(key) == 2 else key, 1.0, eps, L, integrator, n_steps, *st, thin=thin, de_sum=s1, de_sumsq=s2,
                  n_nonfinite=bad, energy_trace=tr, traj_pos=tp, traj_logp=tl)
    names = ("pos", "logp", "grad", "mom", "de_sum", "de_sumsq", "bad", "trace", "traj_pos", "traj_logp")
    return {k: (None if t is None else t.cpu().numpy()) for k, t in zip(names, st + (s1, s2, bad, tr, tp, tl))}


# ---- 1. parity with the float64 restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", mc.INTEGRATORS)
@pytest.mark.parametrize("case", mc.CASES)
def test_step_matches_the_float64_restatement(case, integrator):
    ctx, pos0 = _ctx(case)
    state = _init(ctx, pos0, mc.momentum_key(case))
    vg, eps, L = mc.value_and_grad(case), mc.STEP_SIZES[case][integrator], _L(case)
    n_total, off = mc.shard(case)
    np.testing.assert_allclose(_np(state)[3], ref.init_momentum(mc.momentum_key(case), n_total, mc.dim(case), off, B), rtol=0, atol=4e-16)
    f32 = mc.F32_DISTANCE[case][integrator]
    import torch
    de = torch.empty(B, dtype=torch.float64, device="cuda"); dk = torch.empty_like(de)
    worst = np.zeros(6)
    for j in range(mc.N_STEPS):
        x0, lp0, g0, u0 = _np(state)
        key, keys = mc.step_key(case, j)
        lp_r, g_r = vg(x0.astype(np.float64))
        new, info = ref.step(keys, ref.State(x0.astype(np.float64), u0, lp_r, g_r), vg, eps, L, integrator)
        ctx.mclmc_step(key, 1.0, eps, L, integrator, *state, de, dk)
        x, lp, g, u = _np(state)
        # the device's dE is against ITS log-density of the start state; the restatement's against its own: the same state, so the
        # difference of the two is part of what the log-density tolerance covers
        tol_x = max(4 * 2.0 ** -23 * max(1.0, np.abs(new.position).max()), 4 * f32[0])
        tol_u = max(4 * 2.0 ** -23, 4 * f32[1])
        tol_lp = max(5e-6 * max(1.0, np.abs(new.logdensity).max()), 4 * f32[2])
        tol_e = max(5e-6 * max(1.0, np.abs(new.logdensity).max()), 4 * f32[3])
        err = np.array([np.abs(x - new.position).max(), np.abs(u - new.momentum).max(), np.abs(lp - new.logdensity).max(),
                        np.abs(de.cpu().numpy() - info.energy_change).max(), np.abs(dk.cpu().numpy() - info.kinetic_change).max(),
                        np.abs((u * u).sum(1) - 1.0).max()])
        worst = np.maximum(worst, err)
        print(f"{case} integrator {integrator} step {j}: |x| {err[0]:.3g} (tol {tol_x:.3g}), |u| {err[1]:.3g} (tol {tol_u:.3g}), "
              f"|logp| {err[2]:.3g} (tol {tol_lp:.3g}), |dE| {err[3]:.3g}, |dK| {err[4]:.3g} (tol {tol_e:.3g}), ||u|^2 - 1| {err[5]:.3g}")
        assert err[0] <= tol_x and err[1] <= tol_u and err[2] <= tol_lp and err[3] <= tol_e and err[4] <= tol_e, (case, integrator, j, err)
        assert err[5] <= 1e-14
        assert np.abs(de.cpu().numpy()).max() > 0                                # a step was taken
    ctx.close()


# ---- 2. step == step_keys -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["gmm4", "d65_d0", "d2048_d0_shard"])
def test_step_equals_step_keys_on_the_split_keys(case):
    import torch
    ctx, pos0 = _ctx(case)
    state0 = _init(ctx, pos0, mc.momentum_key(case))
    key, keys = mc.step_key(case, 0)
    eps, L = mc.STEP_SIZES[case][1], _L(case)
    a, b = tuple(t.clone() for t in state0), tuple(t.clone() for t in state0)
    info_a = [torch.empty(B, dtype=torch.float64, device="cuda") for _ in range(2)]
    info_b = [torch.empty(B, dtype=torch.float64, device="cuda") for _ in range(2)]
    ctx.mclmc_step(key, 1.0, eps, L, 1, *a, *info_a)
    ctx.mclmc_step_keys(_keys_dev(keys), 1.0, eps, L, 1, *b, *info_b)
    for name, ta, tb in zip(("pos", "logp", "grad", "mom", "dE", "dK"), a + tuple(info_a), b + tuple(info_b)):
        np.testing.assert_array_equal(ta.cpu().numpy(), tb.cpu().numpy(), err_msg=name)
    assert not torch.equal(a[0], state0[0])
    ctx.close()


# ---- 3. run == n_steps single steps --------------------------------------------------------------------------------------------------
def _assert_run_equals_steps(run, steps):
    for name in ("pos", "logp", "grad", "mom"):
        np.testing.assert_array_equal(run[name], steps[name][-1], err_msg=name)
    np.testing.assert_array_equal(run["trace"], steps["de"])
    np.testing.assert_array_equal(run["traj_pos"], steps["pos"])
    np.testing.assert_array_equal(run["traj_logp"], steps["logp"])
    s1, s2 = np.zeros(steps["de"].shape[1]), np.zeros(steps["de"].shape[1])
    for de in steps["de"]:                                                      # the kernel's order: step by step, each product rounded
        s1, s2 = s1 + de, s2 + de * de
    np.testing.assert_array_equal(run["de_sum"], s1)
    np.testing.assert_array_equal(run["de_sumsq"], s2)
    np.testing.assert_array_equal(run["bad"], (~np.isfinite(steps["de"])).sum(0))
    assert np.isfinite(steps["de"]).all() and (np.abs(steps["de"]) > 0).all()


@pytest.mark.parametrize("integrator", mc.INTEGRATORS)
@pytest.mark.parametrize("case", mc.CASES)
def test_run_is_bit_identical_with_single_step_launches(case, integrator):
    ctx, pos0 = _ctx(case)
    state0 = _init(ctx, pos0, mc.momentum_key(case))
    eps, L, key = mc.STEP_SIZES[case][integrator], _L(case), prng.PRNGKey(21)
    steps = _stepwise(ctx, state0, key, eps, L, integrator, RUN_STEPS)
    run = _run(ctx, state0, key, eps, L, integrator, RUN_STEPS, 1)
    _assert_run_equals_steps(run, steps)
    ctx.close()


@pytest.mark.parametrize("case", ["gmm4", "d257_pbc"])
def test_chain_major_keys_thinning_and_no_trajectory(case):
    ctx, pos0 = _ctx(case)
    state0 = _init(ctx, pos0, mc.momentum_key(case))
    eps, L = mc.STEP_SIZES[case][1], _L(case)
    keys = prng.split(prng.PRNGKey(33), B)
    steps = _stepwise(ctx, state0, keys, eps, L, 1, RUN_STEPS)
    full = _run(ctx, state0, keys, eps, L, 1, RUN_STEPS, 1)
    _assert_run_equals_steps(full, steps)
    thinned = _run(ctx, state0, keys, eps, L, 1, RUN_STEPS, 2)
    assert thinned["traj_pos"].shape == (RUN_STEPS // 2, B, mc.dim(case))
    np.testing.assert_array_equal(thinned["traj_pos"], steps["pos"][[1, 3]])
    np.testing.assert_array_equal(thinned["traj_logp"], steps["logp"][[1, 3]])
    none = _run(ctx, state0, keys, eps, L, 1, RUN_STEPS, 0, traj=False, trace=False)
    for r in (thinned, none):
        for name in ("pos", "logp", "grad", "mom", "de_sum", "de_sumsq", "bad"):
            np.testing.assert_array_equal(r[name], full[name], err_msg=name)
    ctx.close()


# ---- 4. shard invariance -------------------------------------------------------------------------------------------------------------
def test_two_shards_reproduce_the_whole_run():
    """32 chains of d65_d0 (the 16 start states twice) in one context, and as two contexts of 16 at offsets 0 and 16 of 32."""
    import torch
    case, eps, L, key, kmom = "d65_d0", mc.STEP_SIZES["d65_d0"][1], _L("d65_d0"), prng.PRNGKey(5), prng.PRNGKey(6)
    pos32 = np.concatenate([mc.start_state(case), mc.start_state(case)[::-1]])
    whole, _ = _ctx(case, n_local=32, n_total=32, offset=0)
    w = _run(whole, _init(whole, _dev(pos32), kmom), key, eps, L, 1, RUN_STEPS, 2)
    w_mom0 = _np(_init(whole, _dev(pos32), kmom))[3]
    whole.close()
    for off in (0, 16):
        part, _ = _ctx(case, n_local=16, n_total=32, offset=off)
        st = _init(part, _dev(pos32[off:off + 16]), kmom)
        np.testing.assert_array_equal(_np(st)[3], w_mom0[off:off + 16])
        p = _run(part, st, key, eps, L, 1, RUN_STEPS, 2)
        for name in ("pos", "logp", "grad", "mom", "de_sum", "de_sumsq", "bad"):
            np.testing.assert_array_equal(p[name], w[name][off:off + 16], err_msg=f"{name} at offset {off}")
        for name in ("trace", "traj_pos", "traj_logp"):
            np.testing.assert_array_equal(p[name], w[name][:, off:off + 16], err_msg=f"{name} at offset {off}")
        part.close()


# ---- 5. L = inf draws nothing --------------------------------------------------------------------------------------------------------
def test_no_refresh_makes_the_keys_irrelevant():
    case = "d65_d0"
    ctx, pos0 = _ctx(case)
    state0 = _init(ctx, pos0, mc.momentum_key(case))
    eps = mc.STEP_SIZES[case][1]
    a = _stepwise(ctx, state0, prng.PRNGKey(1), eps, np.inf, 1, 1)
    b = _run(ctx, state0, prng.PRNGKey(2), eps, np.inf, 1, 1, 0, traj=False)
    np.testing.assert_array_equal(a["mom"][0], b["mom"])
    np.testing.assert_array_equal(a["pos"][0], b["pos"])
    c = _run(ctx, state0, prng.PRNGKey(2), eps, _L(case), 1, 1, 0, traj=False)
    np.testing.assert_array_equal(c["pos"], b["pos"])                          # the refresh moves the momentum alone
    assert np.abs(c["mom"] - b["mom"]).max() > 1e-3
    ctx.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_touch_nothing():
    import torch
    from mfm_amd import _lib
    from tests import gpu_util as gu
    case = "d65_d0"
    ctx, pos0 = _ctx(case)
    state = _init(ctx, pos0, mc.momentum_key(case))
    before = tuple(t.clone() for t in state)
    key, eps, L = prng.PRNGKey(1), 0.1, 8.0
    tp = torch.empty(2, B, 65, device="cuda")
    bad_calls = [
        ("step_size", lambda: ctx.mclmc_step(key, 1.0, 0.0, L, 1, *state)),
        ("step_size", lambda: ctx.mclmc_run(key, 1.0, float("nan"), L, 1, 4, *state)),
        ("L must be positive", lambda: ctx.mclmc_step(key, 1.0, eps, 0.0, 1, *state)),
        ("L must be positive", lambda: ctx.mclmc_step(key, 1.0, eps, float("nan"), 1, *state)),
        ("L must be positive", lambda: ctx.mclmc_run(key, 1.0, eps, -1.0, 1, 4, *state)),
        ("L = .* is too small", lambda: ctx.mclmc_step(key, 1.0, eps, 1e-4, 1, *state)),            # exp(2 eps / L) overflows: nu is not finite
        ("L = .* is too small", lambda: ctx.mclmc_run(key, 1.0, eps, 1e-300, 1, 4, *state)),
        ("null device pointer", lambda: ctx.mclmc_init(key, None)),
        ("integrator", lambda: ctx.mclmc_step(key, 1.0, eps, L, 2, *state)),
        ("integrator", lambda: ctx.mclmc_run(key, 1.0, eps, L, -1, 4, *state)),
        ("null device pointer", lambda: ctx.mclmc_step(key, 1.0, eps, L, 1, state[0], state[1], state[2], None)),
        ("null key array", lambda: ctx.mclmc_step_keys(None, 1.0, eps, L, 1, *state)),
        ("n_steps", lambda: ctx.mclmc_run(key, 1.0, eps, L, 1, 0, *state)),
        ("thin", lambda: ctx.mclmc_run(key, 1.0, eps, L, 1, 4, *state, thin=-1, traj_pos=tp)),
        ("thin .* n_steps", lambda: ctx.mclmc_run(key, 1.0, eps, L, 1, 4, *state, thin=3, traj_pos=tp)),
        ("d_traj_pos", lambda: ctx.mclmc_run(key, 1.0, eps, L, 1, 4, *state, thin=2)),
        ("key_mode", lambda: ctx.mclmc_run(key, 1.0, eps, L, 1, 4, *state, key_mode=2)),
        ("d_keys", lambda: ctx.mclmc_run(key, 1.0, eps, L, 1, 4, *state, key_mode=1)),
    ]
    for pattern, call in bad_calls:
        with pytest.raises(_lib.MfmError, match=pattern):
            call()
    ctx.set_inverse_mass(np.full(65, 2.0))
    for call in (lambda: ctx.mclmc_step(key, 1.0, eps, L, 1, *state), lambda: ctx.mclmc_run(key, 1.0, eps, L, 1, 4, *state)):
        with pytest.raises(_lib.MfmError, match="unit mass"):
            call()
    ctx.set_inverse_mass(None)
    for t, b in zip(state, before):
        assert torch.equal(t, b)                                                # a rejected call touches nothing
    ctx.mclmc_step(key, 1.0, eps, np.inf, 1, *state)                            # +inf is allowed, and the context still serves
    assert not torch.equal(state[0], before[0])
    ctx.close()
    args, dist, *_ = gu.lgcp_setup(n=4, B=B)
    cox = gu.make_ctx(dist, args)
    cstate = (_dev(dist.init_params.astype(np.float32)), torch.zeros(B, dtype=torch.float64, device="cuda"),
              torch.zeros(B, 16, device="cuda"), torch.zeros(B, 16, dtype=torch.float64, device="cuda"))
    for call in (lambda: cox.mclmc_init(key, cstate[3]), lambda: cox.mclmc_step(key, 1.0, eps, L, 1, *cstate),
                 lambda: cox.mclmc_step_keys(_keys_dev(prng.split(key, B)), 1.0, eps, L, 1, *cstate),
                 lambda: cox.mclmc_run(key, 1.0, eps, L, 1, 4, *cstate)):
        with pytest.raises(_lib.MfmError, match="the HMC step serves the phi-four and mixture targets"):
            call()
    assert cstate[3].abs().max().item() == 0.0
    cox.close()


def test_dim_one_is_refused_by_every_entry_point():
    """d - 1 = 0 divides in the momentum flow: a one-dimensional context (phi-four, d = 1) is refused by all four calls, buffers untouched."""
    import torch
    from mfm_amd import _lib
    ctx = _lib.Context(dim=1, n_chain_local=B, fourier_dim=16, hidden_t=(16, 16), hidden_x=(16, 16), hidden_xt=(16, 16))
    ctx.set_target(_lib.PHI4, [rc.A, rc.TBETA])
    key = prng.PRNGKey(1)
    state = (torch.full((B, 1), 0.5, device="cuda"), torch.full((B,), -1.0, dtype=torch.float64, device="cuda"),
             torch.full((B, 1), 0.25, device="cuda"), torch.full((B, 1), 1.0, dtype=torch.float64, device="cuda"))
    before = tuple(t.clone() for t in state)
    for call in (lambda: ctx.mclmc_init(key, state[3]), lambda: ctx.mclmc_step(key, 1.0, 0.1, 1.0, 1, *state),
                 lambda: ctx.mclmc_step_keys(_keys_dev(prng.split(key, B)), 1.0, 0.1, 1.0, 1, *state),
                 lambda: ctx.mclmc_run(key, 1.0, 0.1, 1.0, 1, 4, *state)):
        with pytest.raises(_lib.MfmError, match="dim must be at least 2 for MCLMC"):
            call()
    for t, b in zip(state, before):
        assert torch.equal(t, b)
    ctx.close()


# ---- 7. the Python API -------------------------------------------------------------------------------------------------------------------
def _gmm_engine(n):
    from mfm_amd import distributions as D
    from mfm_amd.engine import Engine
    from tests import gpu_util as gu
    args, odist, k, model, state = gu.gmm4_setup(B=n)
    dist = D.GaussianMixture(odist.modes, odist.covs, odist.weights)
    args.ot_cond_flow = False
    return Engine(dist, args, model.f), dist


def test_api_equals_the_context_calls():
    import torch
    from mfm_amd import mcmc_utils, random as jr
    from mfm_amd.bblackjax import mclmc
    from mfm_amd.bblackjax.mcmc.mclmc import IntegratorState, MCLMCInfo, MCLMCRunInfo
    eng, dist = _gmm_engine(B)
    eps, L = mc.STEP_SIZES["gmm4"][1], _L("gmm4")
    algo = mclmc(dist.logprob, L, eps)                                          # McLachlan by default
    pos = _dev(mc.start_state("gmm4"))
    kmom, key = jr.PRNGKey(3), jr.PRNGKey(6)
    state = algo.init(pos, kmom)
    assert isinstance(state, IntegratorState) and state.momentum.dtype == torch.float64
    raw = _init(eng.ctx, pos, kmom)
    for t, r in zip((state.position, state.logdensity, state.logdensity_grad, state.momentum), raw):
        assert torch.equal(t, r)
    before = [t.clone() for t in state]
    new, info = algo.step(key, state)
    assert isinstance(new, IntegratorState) and isinstance(info, MCLMCInfo)
    for t, b in zip(state, before):
        assert torch.equal(t, b)                                                # states are values
    de = torch.empty(B, dtype=torch.float64, device="cuda"); dk = torch.empty_like(de)
    st = tuple(t.clone() for t in raw)
    eng.ctx.mclmc_step(key, 1.0, eps, L, 1, *st, de, dk)
    for t, r in zip((new.position, new.logdensity, new.logdensity_grad, new.momentum, info.energy_change, info.kinetic_change, info.logdensity),
                    st + (de, dk, st[1])):
        assert torch.equal(t, r)
    keys = jr.split(jr.PRNGKey(7), B)
    new_k, _ = algo.step(keys, state)
    st = tuple(t.clone() for t in raw)
    eng.ctx.mclmc_step_keys(_keys_dev(keys), 1.0, eps, L, 1, *st)
    assert torch.equal(new_k.position, st[0]) and torch.equal(new_k.momentum, st[3])
    # the run, and inference_loop0 on it and on the host loop
    new_r, rinfo = algo.step.run(key, state, RUN_STEPS, thin=1, keep_energy=True)
    assert isinstance(rinfo, MCLMCRunInfo) and rinfo.positions.shape == (RUN_STEPS, B, 2) and rinfo.energy_changes.shape == (RUN_STEPS, B)
    ctx_run = _run(eng.ctx, raw, key, eps, L, 1, RUN_STEPS, 1)
    np.testing.assert_array_equal(new_r.position.cpu().numpy(), ctx_run["pos"])
    np.testing.assert_array_equal(new_r.momentum.cpu().numpy(), ctx_run["mom"])
    np.testing.assert_array_equal(rinfo.energy_change_sum.cpu().numpy(), ctx_run["de_sum"])
    np.testing.assert_array_equal(rinfo.energy_change_sumsq.cpu().numpy(), ctx_run["de_sumsq"])
    np.testing.assert_array_equal(rinfo.num_nonfinite.cpu().numpy(), ctx_run["bad"])
    np.testing.assert_array_equal(rinfo.energy_changes.cpu().numpy(), ctx_run["trace"])
    np.testing.assert_array_equal(rinfo.last.energy_change.cpu().numpy(), ctx_run["trace"][-1])
    tr = ctx_run["trace"]
    assert rinfo.energy_var_per_dim == pytest.approx(tr.var() / 2, rel=1e-9)
    states, info0 = mcmc_utils.inference_loop0(key, state, algo.step, RUN_STEPS)
    assert isinstance(info0, MCLMCRunInfo) and isinstance(states, IntegratorState) and states.momentum is None
    np.testing.assert_array_equal(states.position.cpu().numpy(), ctx_run["traj_pos"])
    np.testing.assert_array_equal(states.logdensity.cpu().numpy(), ctx_run["traj_logp"])
    plain = lambda k, s: algo.step(k, s)
    h_states, h_infos = mcmc_utils.inference_loop0(key, state, plain, RUN_STEPS)
    np.testing.assert_array_equal(h_states.position.cpu().numpy(), ctx_run["traj_pos"])
    np.testing.assert_array_equal(h_states.momentum[-1].cpu().numpy(), ctx_run["mom"])
    np.testing.assert_array_equal(h_infos.energy_change.cpu().numpy(), ctx_run["trace"])
    no = algo.step.run(key, state, RUN_STEPS)[1]
    assert no.positions is None and no.energy_changes is None
    assert mclmc(dist.logprob, L, eps, "leapfrog").step(key, state)[0].position.ne(new.position).any()
    with pytest.raises(ValueError, match="integrator"):
        mclmc(dist.logprob, L, eps, "verlet")
    eng.close()


# ---- 8. the tuner -----------------------------------------------------------------------------------------------------------------------
def _phi4_engine(d, n):
    from mfm_amd import distributions as D
    from mfm_amd.engine import Engine
    from tests import gpu_util as gu
    args, odist, k, model, state = gu.phi4_setup(d=d, B=n, hidden=32, F=16)
    dist = D.PhiFour(d)
    args.ot_cond_flow = False
    return Engine(dist, args, model.f), dist


def test_the_tuner_reaches_the_target_energy_variance():
    from mfm_amd import random as jr
    from mfm_amd.bblackjax import mclmc, mclmc_find_L_and_step_size
    eng, dist = _phi4_engine(65, 32)
    pos = _dev(np.concatenate([mc.start_state("d65_d0"), mc.start_state("d65_d0")[::-1]]))
    make = lambda L, eps: mclmc(dist.logprob, L, eps)
    state = make(1.0, 1.0).init(pos, jr.PRNGKey(11))
    history = []
    state, params = mclmc_find_L_and_step_size(make, state, jr.PRNGKey(12), 2000, desired_energy_var=mc.TARGET_VAR, history=history)
    assert [h[0] for h in history] == [1] * 8 + [2, 2, 3]
    _, info = make(params.L, params.step_size).step.run(jr.PRNGKey(13), state, 25)
    r = info.energy_var_per_dim / mc.TARGET_VAR
    print(f"step_size {params.step_size:.4g}, L {params.L:.4g} (sqrt(d) = {np.sqrt(65):.4g}), fresh round v / target {r:.3g}")
    assert params.L > 0 and np.isfinite(params.L) and int(info.num_nonfinite.sum()) == 0
    assert 1.0 / 3.0 <= r <= 3.0
    eng.close()


# ---- 9. the training loop -----------------------------------------------------------------------------------------------------------------
def test_training_loop_with_the_mclmc_kernel():
    from mfm_amd import distributions as D, exe_flow_matching as E
    from oracle import loop
    kw = dict(example="phi-four", dim=64, num_chain=32, learning_iter=5, mcmc_per_flow_steps=4.0, hutchs=True, fourier_dim=16, seed=7, eval_iter=1,
              step_size=0.05, hidden_x=[32, 32], hidden_t=[32, 32], hidden_xt=[32, 32], ess_steps=16, adapt_steps=400)
    args = loop.default_args(mcmc_kernel="mclmc", **kw)
    _, _, ex = E.run(D.PhiFour(64), args, None, log_every=1000, return_extras=True)
    for k in ("adapted_step_size", "adapted_L", "adapt_energy_var", "energy_var_per_dim"):
        assert isinstance(ex[k], float) and np.isfinite(ex[k]), (k, ex.get(k))
    assert ex["adapted_step_size"] > 0 and ex["adapted_L"] > 0
    for s in ("min", "median", "mean"):
        assert np.isfinite(ex[f"ess_per_step_{s}"])
        assert ex[f"ess_per_grad_{s}"] == ex[f"ess_per_step_{s}"] / 2            # McLachlan: two gradients per step
    ex["engine"].close()
