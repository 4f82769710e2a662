"""GPU tests of ``mfm_ghmc_init`` / ``_step`` / ``_step_keys`` / ``_run`` (mfm_amd/csrc/ghmc.hip) and ``bblackjax.ghmc``.

The yardstick of a transition is tests/ghmc_ref.py, the float64 restatement.  Each of a case's transitions starts from a state the CPU
has fixed (``ghmc_cases.states``: the restatement's own trajectory in the device's number formats), uploaded to the device; the
tolerance is ``ghmc_cases.TOLERANCE``, 4 x what the device's number formats cost between the two restatements, and tests/test_ghmc_ref.py
has checked on the CPU that no decision of these transitions is within it of its boundary, so every decision must agree.  The yardstick
of the run is the single-step kernel, bit for bit; of alpha = 1, ``mfm_hmc_step_keys`` at one leapfrog step, bit for bit."""
import numpy as np
import pytest

from oracle import prng
from tests import ghmc_cases as gc
from tests import ghmc_ref as ref

pytestmark = pytest.mark.gpu

RUN_STEPS = 4
ALPHA, DELTA = gc.ALPHA, gc.DELTA


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _keys_dev(keys):
    return _dev(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32))


def _ctx(case, n_local=None, n_total=None, offset=0):
    from mfm_amd import _lib
    from tests import gpu_util as gu
    n_local = gc.n_chains(case) if n_local is None else n_local
    ctx = _lib.Context(dim=gc.dim(case), n_chain_local=n_local, n_chain_total=n_total or n_local, chain_offset=offset, fourier_dim=16,
                       hidden_t=(16, 16), hidden_x=(16, 16), hidden_xt=(16, 16))
    if case == "gmm4":
        ctx.set_target(*gu.target_block(gc.oracle_dist(case)))
    else:
        ctx.set_target(_lib.PHI4, gc.block(case) or [gc.A, gc.TBETA])
    return ctx


def _minv_dev(case, mass):
    return _dev(gc.inverse_mass(gc.dim(case))) if mass else None


def _upload(ctx, st):
    """The device state at a restatement state: positions uploaded, log-density and gradient by ``mfm_mala_init``, p and s uploaded."""
    import torch
    pos = _dev(st.position.astype(np.float32))
    logp = torch.empty(pos.shape[0], dtype=torch.float64, device="cuda"); grad = torch.empty_like(pos)
    ctx.mala_init(pos, 1.0, logp, grad)
    return pos, logp, grad, _dev(st.momentum), _dev(st.slice)


def _init(ctx, pos0, key, minv):
    import torch
    pos = pos0.clone()
    logp = torch.empty(pos.shape[0], dtype=torch.float64, device="cuda"); grad = torch.empty_like(pos)
    mom = torch.empty(pos.shape, dtype=torch.float64, device="cuda"); s = torch.empty(pos.shape[0], dtype=torch.float64, device="cuda")
    ctx.mala_init(pos, 1.0, logp, grad)
    ctx.ghmc_init(key, mom, s, minv)
    return pos, logp, grad, mom, s


def _np(state):
    return tuple(t.cpu().numpy().copy() for t in state)


def _infos(n):
    import torch
    return (torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda"))


# ---- 1. parity with the float64 restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", gc.MASSES)
@pytest.mark.parametrize("case", gc.CASES)
def test_step_matches_the_float64_restatement(case, mass):
    """Measured on MI355X on the run-time-boundary cases at MAXIT 4 / 16 / 32, largest error / tolerance over both masses and the three
    transitions (x, p, logp, dH, s): d65_pbc 0.25 0.25 0.24 0.24 0.24; 32x32_db 0.25 0.24 0.21 0.27 0.22; d1025_pbc 0.24 0.25 0.25 0.28
    0.25 -- the device lands on the device-format restatement, a quarter of the tolerance from the float64 one."""
    ctx = _ctx(case)
    n, d = gc.n_chains(case), gc.dim(case)
    vg, eps, m = gc.value_and_grad(case), gc.STEP_SIZES[case][mass], gc.minv(case, mass)
    minv = _minv_dev(case, mass)
    tol = gc.TOLERANCE[case][mass]
    # mfm_ghmc_init against the restatement's draws
    st0 = _init(ctx, _dev(gc.start_state(case)), gc.init_key(case), minv)
    p_ref, s_ref = ref.init_momentum_slice(gc.init_key(case), n, d, m)
    np.testing.assert_allclose(_np(st0)[3], p_ref, rtol=0, atol=4e-15)
    np.testing.assert_allclose(_np(st0)[4], s_ref, rtol=0, atol=4e-16)
    seen = np.zeros(2, int)
    for j, st in enumerate(gc.states(case, mass)):
        key, keys = gc.step_key(case, j)
        lp_r, g_r = vg(st.position)
        new, info = ref.step(keys, st._replace(logdensity=lp_r, logdensity_grad=g_r), vg, eps, ALPHA, DELTA, m)
        dstate = _upload(ctx, st)
        acc, isacc, de = _infos(n)
        ctx.ghmc_step(key, 1.0, eps, ALPHA, DELTA, *dstate, minv, acc, isacc, de)
        x, lp, g, p, s = _np(dstate)
        a = isacc.cpu().numpy().astype(bool)
        np.testing.assert_array_equal(a, info.is_accepted, err_msg=f"{case} mass {mass} step {j}: decisions")
        err = np.array([np.abs(x - new.position).max(), np.abs(p - new.momentum).max(), np.abs(lp - new.logdensity).max(),
                        np.abs(de.cpu().numpy() - info.energy_change).max(), np.abs(s - new.slice).max(),
                        np.abs(acc.cpu().numpy() - info.acceptance_rate).max()])
        print(f"{case} mass {mass} step {j}: accepted {a.sum()} of {n}; |x| {err[0]:.3g} (tol {tol[0]:.3g}), |p| {err[1]:.3g} (tol {tol[1]:.3g}), "
              f"|logp| {err[2]:.3g} (tol {tol[2]:.3g}), |dH| {err[3]:.3g} (tol {tol[3]:.3g}), |s| {err[4]:.3g} (tol {tol[4]:.3g}), |rate| {err[5]:.3g}")
        assert (err[:5] <= np.array(tol)).all(), (case, mass, j, err, tol)
        assert err[5] <= tol[3] + 2.0 ** -23                              # the rate is min(1, exp(-dH)) stored in float32
        rej = ~a
        np.testing.assert_array_equal(x[rej], st.position[rej].astype(np.float32))       # a rejection keeps x bit for bit
        assert (np.abs(s) <= 1.0).all()
        seen += [a.sum(), rej.sum()]
    assert seen.min() >= 2                                                 # both decisions were exercised
    ctx.close()


# ---- 2. step == step_keys; run == n single steps, both key modes, thinning ----------------------------------------------------------
def _stepwise(ctx, state0, key, eps, minv, n_steps):
    """n single-step launches on the run's step keys: the state after, and the infos of, every launch (numpy)."""
    from mfm_amd import random as jr
    st = tuple(t.clone() for t in state0)
    n = st[0].shape[0]
    acc, isacc, de = _infos(n)
    per_chain = np.ndim(key) == 2
    step_keys = jr.split_rows(key, n_steps) if per_chain else jr.split(key, n_steps)
    names = ("pos", "logp", "grad", "mom", "slice", "acc", "isacc", "de")
    out = {k: [] for k in names}
    for j in range(n_steps):
        if per_chain:
            ctx.ghmc_step_keys(_keys_dev(step_keys[:, j]), 1.0, eps, ALPHA, DELTA, *st, minv, acc, isacc, de)
        else:
            ctx.ghmc_step(step_keys[j], 1.0, eps, ALPHA, DELTA, *st, minv, acc, isacc, de)
        for name, t in zip(names, st + (acc, isacc, de)):
            out[name].append(t.cpu().numpy().copy())
    return {k: np.stack(v) for k, v in out.items()}


def _run(ctx, state0, key, eps, minv, n_steps, thin, traj=True):
    import torch
    st = tuple(t.clone() for t in state0)
    n, d = st[0].shape
    n_acc = torch.empty(n, dtype=torch.int32, device="cuda")
    acc_sum = torch.empty(n, dtype=torch.float64, device="cuda"); de_sum = torch.empty_like(acc_sum)
    acc, isacc, de = _infos(n)
    tp = tl = None
    if traj and thin > 0:
        tp = torch.empty(n_steps // thin, n, d, device="cuda"); tl = torch.empty(n_steps // thin, n, dtype=torch.float64, device="cuda")
    ctx.ghmc_run(_keys_dev(key) if np.ndim(key) == 2 else key, 1.0, eps, ALPHA, DELTA, n_steps, *st, minv, thin=thin, n_acc=n_acc, acc_sum=acc_sum,
                 energy_sum=de_sum, acc=acc, is_acc=isacc, energy_change=de, traj_pos=tp, traj_logp=tl)
    names = ("pos", "logp", "grad", "mom", "slice", "n_acc", "acc_sum", "de_sum", "acc", "isacc", "de", "traj_pos", "traj_logp")
    return {k: (None if t is None else t.cpu().numpy()) for k, t in zip(names, st + (n_acc, acc_sum, de_sum, acc, isacc, de, tp, tl))}


def _assert_run_equals_steps(run, steps):
    for name in ("pos", "logp", "grad", "mom", "slice"):
        np.testing.assert_array_equal(run[name], steps[name][-1], err_msg=name)
    for name in ("acc", "isacc", "de"):
        np.testing.assert_array_equal(run[name], steps[name][-1], err_msg=name)
    np.testing.assert_array_equal(run["traj_pos"], steps["pos"])
    np.testing.assert_array_equal(run["traj_logp"], steps["logp"])
    n = steps["de"].shape[1]
    a_sum, d_sum = np.zeros(n), np.zeros(n)
    for a, ia, de in zip(steps["acc"], steps["isacc"], steps["de"]):           # the kernel's order: step by step
        a_sum = a_sum + a.astype(np.float64)
        d_sum = np.where(ia.astype(bool), d_sum + de, d_sum)
    np.testing.assert_array_equal(run["n_acc"], steps["isacc"].astype(np.int64).sum(0))
    # the run tallies the float64 rate, a single step reports it rounded to float32: equal after that rounding per step
    np.testing.assert_allclose(run["acc_sum"], a_sum, rtol=0, atol=steps["acc"].shape[0] * 2.0 ** -24)
    np.testing.assert_array_equal(run["de_sum"], d_sum)
    assert steps["isacc"].any() and not steps["isacc"].all()


@pytest.mark.parametrize("mass", gc.MASSES)
@pytest.mark.parametrize("case", gc.CASES)
def test_run_is_bit_identical_with_single_step_launches(case, mass):
    ctx = _ctx(case)
    minv = _minv_dev(case, mass)
    state0 = _init(ctx, _dev(gc.start_state(case)), gc.init_key(case), minv)
    eps, key = gc.STEP_SIZES[case][mass], prng.PRNGKey(21)
    steps = _stepwise(ctx, state0, key, eps, minv, RUN_STEPS)
    run = _run(ctx, state0, key, eps, minv, RUN_STEPS, 1)
    _assert_run_equals_steps(run, steps)
    ctx.close()


@pytest.mark.parametrize("case,mass", [("gmm4", False), ("d320_d0", True)])
def test_chain_major_keys_thinning_and_no_trajectory(case, mass):
    ctx = _ctx(case)
    n = gc.n_chains(case)
    minv = _minv_dev(case, mass)
    state0 = _init(ctx, _dev(gc.start_state(case)), gc.init_key(case), minv)
    eps = gc.STEP_SIZES[case][mass]
    keys = prng.split(prng.PRNGKey(33), n)
    steps = _stepwise(ctx, state0, keys, eps, minv, RUN_STEPS)
    full = _run(ctx, state0, keys, eps, minv, RUN_STEPS, 1)
    _assert_run_equals_steps(full, steps)
    thinned = _run(ctx, state0, keys, eps, minv, RUN_STEPS, 2)
    assert thinned["traj_pos"].shape == (RUN_STEPS // 2, n, gc.dim(case))
    np.testing.assert_array_equal(thinned["traj_pos"], steps["pos"][[1, 3]])
    np.testing.assert_array_equal(thinned["traj_logp"], steps["logp"][[1, 3]])
    none = _run(ctx, state0, keys, eps, minv, RUN_STEPS, 0, traj=False)
    for r in (thinned, none):
        for name in ("pos", "logp", "grad", "mom", "slice", "n_acc", "acc_sum", "de_sum"):
            np.testing.assert_array_equal(r[name], full[name], err_msg=name)
    ctx.close()


@pytest.mark.parametrize("case", ["gmm4", "d65_d0", "d1100_d0"] + list(gc.ROW_CASES))
def test_step_equals_step_keys_on_the_split_keys(case):
    import torch
    ctx = _ctx(case)
    n = gc.n_chains(case)
    state0 = _init(ctx, _dev(gc.start_state(case)), gc.init_key(case), None)
    key, keys = gc.step_key(case, 0)
    eps = gc.STEP_SIZES[case][False]
    a, b = tuple(t.clone() for t in state0), tuple(t.clone() for t in state0)
    ia, ib = _infos(n), _infos(n)
    ctx.ghmc_step(key, 1.0, eps, ALPHA, DELTA, *a, None, *ia)
    ctx.ghmc_step_keys(_keys_dev(keys), 1.0, eps, ALPHA, DELTA, *b, None, *ib)
    for name, ta, tb in zip(("pos", "logp", "grad", "mom", "slice", "acc", "isacc", "dH"), a + ia, b + ib):
        np.testing.assert_array_equal(ta.cpu().numpy(), tb.cpu().numpy(), err_msg=name)
    assert not torch.equal(a[3], state0[3])
    ctx.close()


# ---- 3. alpha = 1: the bits of mfm_hmc_step_keys at one leapfrog step -------------------------------------------------------------------
@pytest.mark.parametrize("mass", gc.MASSES)
@pytest.mark.parametrize("case", gc.CASES)
def test_alpha_one_has_the_bits_of_hmc_at_one_leapfrog_step(case, mass):
    """The refresh is 0 p + 1 n: the proposal (the state of every accepted chain, and of the chains HMC accepted) and acceptance_rate of
    every chain are those of ``mfm_hmc_step_keys(num_steps = 1)`` on the same keys, with the same mass installed on the context."""
    import torch
    ctx = _ctx(case)
    n = gc.n_chains(case)
    minv = _minv_dev(case, mass)
    pos, logp, grad, mom, s = _init(ctx, _dev(gc.start_state(case)), gc.init_key(case), minv)
    s.fill_(0.0)                                                           # |s| = |fmod(1 + 0.5, 2) - 1| = 0.5: a mix of decisions at these step sizes
    eps = gc.STEP_SIZES[case][mass]
    keys = _keys_dev(gc.step_key(case, 0)[1])
    h = (pos.clone(), logp.clone(), grad.clone())
    hacc = torch.empty(n, device="cuda"); hisacc = torch.empty(n, dtype=torch.uint8, device="cuda")
    ctx.set_inverse_mass(gc.inverse_mass(gc.dim(case)) if mass else None)
    ctx.hmc_step_keys(keys, 1.0, eps, 1, *h, hacc, hisacc)
    ctx.set_inverse_mass(None)                                             # (GHMC does not read it: its mass is the call's argument)
    acc, isacc, de = _infos(n)
    ctx.ghmc_step_keys(keys, 1.0, eps, 1.0, 0.5, pos, logp, grad, mom, s, minv, acc, isacc, de)
    np.testing.assert_array_equal(acc.cpu().numpy(), hacc.cpu().numpy())
    both = (isacc.bool() & hisacc.bool()).cpu().numpy()
    assert both.sum() >= 1, "no chain accepted by both: nothing compared"
    for name, g_, h_ in zip(("pos", "logp", "grad"), (pos, logp, grad), h):
        np.testing.assert_array_equal(g_.cpu().numpy()[both], h_.cpu().numpy()[both], err_msg=name)
    # and the decision is the slice rule on the reported energy change
    np.testing.assert_array_equal(isacc.bool().cpu().numpy(), 0.5 <= np.exp(-de.cpu().numpy()))
    ctx.close()


# ---- 4. shard invariance -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", gc.MASSES)
def test_two_shards_reproduce_the_whole_run(mass):
    """32 chains of d65_d0 (the 16 start states twice) in one context, and as two contexts of 16 at offsets 0 and 16 of 32: init, the
    step-major run (whose keys are drawn by global chain id) and a single step."""
    case, key, kinit = "d65_d0", prng.PRNGKey(5), prng.PRNGKey(6)
    eps = gc.STEP_SIZES[case][mass]
    minv = _minv_dev(case, mass)
    pos32 = np.concatenate([gc.start_state(case), gc.start_state(case)[::-1]])
    whole = _ctx(case, n_local=32, n_total=32, offset=0)
    w0 = _init(whole, _dev(pos32), kinit, minv)
    w = _run(whole, w0, key, eps, minv, RUN_STEPS, 2)
    ws = _stepwise(whole, w0, key, eps, minv, 1)
    w0 = _np(w0)
    whole.close()
    for off in (0, 16):
        part = _ctx(case, n_local=16, n_total=32, offset=off)
        st = _init(part, _dev(pos32[off:off + 16]), kinit, minv)
        np.testing.assert_array_equal(_np(st)[3], w0[3][off:off + 16])
        np.testing.assert_array_equal(_np(st)[4], w0[4][off:off + 16])
        p = _run(part, st, key, eps, minv, RUN_STEPS, 2)
        for name in ("pos", "logp", "grad", "mom", "slice", "n_acc", "acc_sum", "de_sum", "acc", "isacc", "de"):
            np.testing.assert_array_equal(p[name], w[name][off:off + 16], err_msg=f"{name} at offset {off}")
        for name in ("traj_pos", "traj_logp"):
            np.testing.assert_array_equal(p[name], w[name][:, off:off + 16], err_msg=f"{name} at offset {off}")
        ps = _stepwise(part, st, key, eps, minv, 1)
        for name in ps:
            np.testing.assert_array_equal(ps[name], ws[name][:, off:off + 16], err_msg=f"step {name} at offset {off}")
        part.close()


# ---- 5. refusals and their order --------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_touch_nothing():
    import torch
    from mfm_amd import _lib
    from tests import gpu_util as gu
    case = "d65_d0"
    ctx = _ctx(case)
    n = gc.n_chains(case)
    state = _init(ctx, _dev(gc.start_state(case)), gc.init_key(case), None)
    before = tuple(t.clone() for t in state)
    key, eps = prng.PRNGKey(1), 0.02
    tp = torch.empty(2, n, 65, device="cuda")
    nan = float("nan")
    bad_calls = [
        ("step_size", lambda: ctx.ghmc_step(key, 1.0, 0.0, ALPHA, DELTA, *state)),
        ("step_size", lambda: ctx.ghmc_run(key, 1.0, nan, ALPHA, DELTA, 4, *state)),
        ("alpha", lambda: ctx.ghmc_step(key, 1.0, eps, 0.0, DELTA, *state)),
        ("alpha", lambda: ctx.ghmc_step(key, 1.0, eps, 1.5, DELTA, *state)),
        ("alpha", lambda: ctx.ghmc_run(key, 1.0, eps, nan, DELTA, 4, *state)),
        ("delta", lambda: ctx.ghmc_step(key, 1.0, eps, ALPHA, -0.1, *state)),
        ("delta", lambda: ctx.ghmc_run(key, 1.0, eps, ALPHA, nan, 4, *state)),
        ("null device pointer", lambda: ctx.ghmc_init(key, None, state[4])),
        ("null device pointer", lambda: ctx.ghmc_init(key, state[3], None)),
        ("null device pointer", lambda: ctx.ghmc_step(key, 1.0, eps, ALPHA, DELTA, state[0], state[1], state[2], None, state[4])),
        ("null device pointer", lambda: ctx.ghmc_step(key, 1.0, eps, ALPHA, DELTA, state[0], state[1], state[2], state[3], None)),
        ("null key array", lambda: ctx.ghmc_step_keys(None, 1.0, eps, ALPHA, DELTA, *state)),
        ("n_steps", lambda: ctx.ghmc_run(key, 1.0, eps, ALPHA, DELTA, 0, *state)),
        ("thin", lambda: ctx.ghmc_run(key, 1.0, eps, ALPHA, DELTA, 4, *state, thin=-1, traj_pos=tp)),
        ("thin .* n_steps", lambda: ctx.ghmc_run(key, 1.0, eps, ALPHA, DELTA, 4, *state, thin=3, traj_pos=tp)),
        ("d_traj_pos", lambda: ctx.ghmc_run(key, 1.0, eps, ALPHA, DELTA, 4, *state, thin=2)),
        ("key_mode", lambda: ctx.ghmc_run(key, 1.0, eps, ALPHA, DELTA, 4, *state, key_mode=2)),
        ("d_keys", lambda: ctx.ghmc_run(key, 1.0, eps, ALPHA, DELTA, 4, *state, key_mode=1)),
        # the order: the shared checks before the sampler's own, step_size before alpha before delta
        ("null device pointer", lambda: ctx.ghmc_step(key, 1.0, 0.0, ALPHA, DELTA, state[0], state[1], state[2], None, state[4])),
        ("n_steps", lambda: ctx.ghmc_run(key, 1.0, 0.0, 2.0, -1.0, 0, *state)),
        ("thin", lambda: ctx.ghmc_run(key, 1.0, 0.0, 2.0, -1.0, 4, *state, thin=-1, traj_pos=tp)),
        ("step_size", lambda: ctx.ghmc_step(key, 1.0, 0.0, 2.0, -1.0, *state)),
        ("alpha", lambda: ctx.ghmc_step(key, 1.0, eps, 2.0, -1.0, *state)),
    ]
    for pattern, call in bad_calls:
        with pytest.raises(_lib.MfmError, match=pattern):
            call()
    for t, b in zip(state, before):
        assert torch.equal(t, b)                                                # a rejected call touches nothing
    ctx.set_inverse_mass(np.full(65, 2.0))                                      # an installed mass is neither refused nor read
    a, b = tuple(t.clone() for t in state), tuple(t.clone() for t in state)
    ctx.ghmc_step(key, 1.0, eps, ALPHA, DELTA, *a)
    ctx.set_inverse_mass(None)
    ctx.ghmc_step(key, 1.0, eps, ALPHA, DELTA, *b)
    for ta, tb in zip(a, b):
        assert torch.equal(ta, tb)
    assert not torch.equal(a[3], before[3])
    ctx.close()
    args, dist, *_ = gu.lgcp_setup(n=4, B=16)
    cox = gu.make_ctx(dist, args)
    cstate = (_dev(dist.init_params.astype(np.float32)), torch.zeros(16, dtype=torch.float64, device="cuda"),
              torch.zeros(16, 16, device="cuda"), torch.zeros(16, 16, dtype=torch.float64, device="cuda"), torch.zeros(16, dtype=torch.float64, device="cuda"))
    for call in (lambda: cox.ghmc_init(key, cstate[3], cstate[4]), lambda: cox.ghmc_step(key, 1.0, 0.0, ALPHA, DELTA, *cstate),
                 lambda: cox.ghmc_step_keys(_keys_dev(prng.split(key, 16)), 1.0, eps, ALPHA, DELTA, *cstate),
                 lambda: cox.ghmc_run(key, 1.0, eps, 2.0, DELTA, 4, *cstate)):
        with pytest.raises(_lib.MfmError, match="the HMC step serves the phi-four and mixture targets"):      # ahead of step_size / alpha
            call()
    assert cstate[3].abs().max().item() == 0.0
    cox.close()


# ---- 6. the Python API -------------------------------------------------------------------------------------------------------------------
def test_api_equals_the_context_calls():
    import torch
    from mfm_amd import distributions as D, mcmc_utils, random as jr
    from mfm_amd.bblackjax import ghmc
    from mfm_amd.bblackjax.mcmc.ghmc import GHMCInfo, GHMCRunInfo, GHMCState
    from mfm_amd.engine import Engine
    from tests import gpu_util as gu
    n = 16
    args, odist, k, model, state = gu.gmm4_setup(B=n)
    dist = D.GaussianMixture(odist.modes, odist.covs, odist.weights)
    args.ot_cond_flow = False
    eng = Engine(dist, args, model.f)
    eps = gc.STEP_SIZES["gmm4"][True]
    sigma = np.sqrt(gc.inverse_mass(2))
    minv = _dev(sigma * sigma)
    algo = ghmc(dist.logprob, eps, ALPHA, momentum_inverse_scale=sigma)        # delta defaults to alpha / 2
    pos = _dev(gc.start_state("gmm4"))
    kinit, key = jr.PRNGKey(3), jr.PRNGKey(6)
    st = algo.init(pos, kinit)
    assert isinstance(st, GHMCState) and st.momentum.dtype == torch.float64 and st.slice.shape == (n,)
    raw = _init(eng.ctx, pos, kinit, minv)
    for t, r in zip((st.position, st.logdensity, st.logdensity_grad, st.momentum, st.slice), raw):
        assert torch.equal(t, r)
    before = [t.clone() for t in st]
    new, info = algo.step(key, st)
    assert isinstance(new, GHMCState) and isinstance(info, GHMCInfo) and info.is_accepted.dtype == torch.bool
    for t, b in zip(st, before):
        assert torch.equal(t, b)                                                # states are values
    r = tuple(t.clone() for t in raw)
    acc, isacc, de = _infos(n)
    eng.ctx.ghmc_step(key, 1.0, eps, ALPHA, ALPHA / 2, *r, minv, acc, isacc, de)
    for t, u in zip((new.position, new.logdensity, new.logdensity_grad, new.momentum, new.slice, info.acceptance_rate, info.energy_change),
                    r + (acc, de)):
        assert torch.equal(t, u)
    new_r, rinfo = algo.step.run(key, st, RUN_STEPS, thin=1)
    assert isinstance(rinfo, GHMCRunInfo) and rinfo.positions.shape == (RUN_STEPS, n, 2)
    assert ALPHA / 2 == DELTA
    ctx_run = _run(eng.ctx, raw, key, eps, minv, RUN_STEPS, 1)
    np.testing.assert_array_equal(new_r.position.cpu().numpy(), ctx_run["pos"])
    np.testing.assert_array_equal(new_r.momentum.cpu().numpy(), ctx_run["mom"])
    np.testing.assert_array_equal(rinfo.num_accepted.cpu().numpy(), ctx_run["n_acc"])
    np.testing.assert_array_equal(rinfo.energy_change_sum.cpu().numpy(), ctx_run["de_sum"])
    np.testing.assert_array_equal(rinfo.acceptance_rate.cpu().numpy(), ctx_run["acc_sum"] / RUN_STEPS)
    states, info0 = mcmc_utils.inference_loop0(key, st, algo.step, RUN_STEPS)
    assert isinstance(info0, GHMCRunInfo) and isinstance(states, GHMCState) and states.momentum is None
    np.testing.assert_array_equal(states.position.cpu().numpy(), ctx_run["traj_pos"])
    h_states, h_infos = mcmc_utils.inference_loop0(key, st, lambda k_, s_: algo.step(k_, s_), RUN_STEPS)
    np.testing.assert_array_equal(h_states.position.cpu().numpy(), ctx_run["traj_pos"])
    np.testing.assert_array_equal(h_states.slice[-1].cpu().numpy(), ctx_run["slice"])
    for bad in (dict(step_size=0.0, alpha=0.5), dict(step_size=0.1, alpha=0.0), dict(step_size=0.1, alpha=1.1), dict(step_size=0.1, alpha=0.5, delta=-1.0)):
        with pytest.raises(ValueError, match="ghmc needs"):
            ghmc(dist.logprob, **bad)
    eng.close()
