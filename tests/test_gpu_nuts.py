"""GPU tests of the No-U-turn sampler: ``mfm_nuts_step`` / ``mfm_nuts_step_keys`` / ``mfm_nuts_run`` (mfm_amd/csrc/nuts.hip) and
``mfm_amd.bblackjax.mcmc.nuts``.

The yardstick of a transition is tests/nuts_ref.py, the float64 restatement with the kernel's rounding points (tests/test_nuts_ref.py
holds it to a recursive restatement and to oracle.hmc.kernel).  A tree is a chain of yes/no decisions, so the comparison sets aside the
chains whose reference tree hung on a decision too close to call in float32-fed arithmetic -- a chain is BORDERLINE in a transition when
the reference's smallest margin is under the border:

* selection / merge draws (and, by the same argument, the divergence test): ``|log u - log ratio| < 10 tol_e`` with ``tol_e`` the energy
  tolerance of tests/test_gpu_hmc.py, ``5e-6 max(1, max |logp|)`` (+ ``5e-4`` for the mixtures, whose log-density is float32 per mode);
* U-turn tests: ``|dot| / (|v| |s|) < 1e-4``.

Every other chain must match the reference exactly in depth, leapfrog count and both flags, in position and log-density within
test_gpu_hmc.py's bounds, and in acceptance rate within ``tol_e`` (the rate is a mean of ``min(1, exp(delta))``, whose slope in delta is
at most 1).  At most a quarter of a case's chains may be borderline in any transition: asserted on the reference alone, continued from its
own states, before the kernel runs.

Step sizes and burn-in (``max_tree_depth`` 6): phi-four 0.03 at d <= 64 and 0.02 at d = 256, the mixtures 0.3 / 0.15; ``BURN``
transitions of the reference itself from the initial draw, where |logp| is 4e3 (d = 64) to 5e4 (d = 256) and ``tol_e`` would swallow
every decision; after them it is 50 to 200.  Reference alone, unit mass: at d <= 64 two thirds of the trees end on a U-turn at depths 3 to
6 and the borderline shares are 0.02 to 0.16; at d = 256 the slow modes outlast 63 steps of 0.02, nearly every tree is cut by the limit
and the shares are 0.14 to 0.17; the mixtures' trees have depths 1 to 5 and shares under 0.08.

The helpers (setup, burn-in, the borderline rule, the comparison) live in tests/nuts_util.py, shared with
tests/test_gpu_nuts_instances.py, which runs the same comparison on every kernel instance and launch geometry."""
import numpy as np
import pytest

from oracle import mala as omala, prng, targets
from tests import nuts_ref as nr, nuts_util as nu
from tests.nuts_util import (B, BURN, DEPTH, INFO, N_TRANS, _borderline, _compare, _ctx, _dev_info, _init, _keys_dev, _ref_state,      # noqa: F401
                             _run, _setup, _stepwise, _tol_e)      # (re-exported: tests/test_gpu_nuts_warmup.py takes them from here)

pytestmark = pytest.mark.gpu

# name: (target, d, phi-four block tail or None, step size)
CASES = {
    "phi4-64": ("phi4", 64, None, 0.03),
    "phi4-256": ("phi4", 256, None, 0.02),
    "phi4-48": ("phi4", 48, None, 0.03),
    "phi4-64-pbc": ("phi4", 64, [1.0, 0.0], 0.03),
    "gmm4": ("gmm4", 2, None, 0.3),
    "gmm16": ("gmm16", 2, None, 0.15),
}


def _burned(case, mass):
    """The case's start: the reference's own state after BURN transitions from the initial draw, and the reference-only pass of
    N_TRANS transitions from it with the share of borderline chains in each (tests/nuts_util.py: computed once)."""
    kind, d, tail, eps = CASES[case]
    r = nu.burned(kind, d, None if tail is None else tuple(tail), eps, DEPTH, mass)
    return r["start"], r["minv"], r["shares"], r["infos"]


@pytest.mark.parametrize("mass", [False, True], ids=["unit", "mass"])
@pytest.mark.parametrize("case", list(CASES))
def test_transitions_match_the_reference(case, mass):
    kind, d, tail, eps = CASES[case]
    start, minv, shares, infos = _burned(case, mass)
    print(f"{case} mass={mass}: borderline shares of the reference-only pass {shares}; depths {[np.bincount(i.depth).tolist() for i in infos]}")
    assert max(shares) <= 0.25, shares                                         # the condition of the comparison, before the kernel runs
    if case == "phi4-64":                                                      # what the cases must cover
        assert max(i.depth.max() for i in infos) >= 4
        assert any((i.directions > 0).any() for i in infos) and any((i.directions < 0).any() for i in infos)
        assert any(i.stopped_in_subtree.any() for i in infos)
    # N_TRANS transitions of nuts_step on keys 50 + it against nr.kernel over the non-borderline chains, each with its own share
    # asserted <= 0.25, both sides continued from the kernel's state (tests/nuts_util.py)
    nu._transitions_against_the_reference(kind, d, tail, eps, DEPTH, minv, start, f"{case} mass={mass}")


# ---- device only ------------------------------------------------------------------------------------------------------------
# name: (target, d, phi-four block tail or None, step size, max_tree_depth); the chains per workgroup at the deep limits are 1 (d = 64
# at 12, d = 128 at 14) and 2 (d = 256 at 14), asserted through the launch plan in tests/test_nuts_cases.py
BITS = {"phi4-64": ("phi4", 64, None, 0.03, 5), "phi4-100": ("phi4", 100, None, 0.03, 5), "phi4-256": ("phi4", 256, None, 0.02, 5),
        "phi4-64-pbc": ("phi4", 64, [1.0, 0.0], 0.03, 5), "gmm4": ("gmm4", 2, None, 0.3, 5),
        "phi4-64-limit12": ("phi4", 64, None, 0.03, 12), "phi4-128-limit14": ("phi4", 128, None, 0.03, 14),
        "phi4-256-limit14": ("phi4", 256, None, 0.02, 14)}
N_RUN, NB = 4, 16


def _assert_run_equals_steps(run, steps):
    for name in ("pos", "logp", "grad") + INFO:
        np.testing.assert_array_equal(run[name], steps[name][-1], err_msg=name)
    np.testing.assert_array_equal(run["traj_pos"], steps["pos"])
    np.testing.assert_array_equal(run["traj_logp"], steps["logp"])
    np.testing.assert_array_equal(run["leapfrog_sum"], steps["num_leapfrog"].astype(np.int64).sum(0))
    np.testing.assert_array_equal(run["depth_sum"], steps["depth"].sum(0))
    np.testing.assert_array_equal(run["n_divergent"], steps["is_divergent"].astype(np.int64).sum(0))
    acc = np.zeros(steps["pos"].shape[1])
    for a in steps["acceptance_rate"]:                                         # the run's own order of summation: bit for bit
        acc = acc + a
    np.testing.assert_array_equal(run["acc_sum"], acc)


@pytest.mark.parametrize("case", list(BITS))
def test_run_has_the_bits_of_the_single_steps(case):
    """``mfm_nuts_run`` over n steps against n launches of ``mfm_nuts_step`` on ``split(key, n)[j]`` and of ``mfm_nuts_step_keys`` on
    ``split(keys[b], n)[j]``: state, thinned trajectory, totals, last info; and a mass of ones against the unit instances."""
    kind, d, tail, eps, limit = BITS[case]
    ctx, pos0, _ = _ctx(kind, d, tail, NB)
    state0 = _init(ctx, pos0)
    key, keys = prng.PRNGKey(21), prng.split(prng.PRNGKey(22), NB)
    unit = None
    for k in (key, keys):
        steps = _stepwise(ctx, state0, k, eps, N_RUN, limit)
        run = _run(ctx, state0, k, eps, N_RUN, limit)
        _assert_run_equals_steps(run, steps)
        assert len(set(steps["depth"].reshape(-1).tolist())) > 1 and (steps["pos"][-1] != state0[0].cpu().numpy()).any()
        unit = run if unit is None else unit
    thinned = _run(ctx, state0, key, eps, N_RUN, limit, thin=2)
    np.testing.assert_array_equal(thinned["traj_pos"], unit["traj_pos"][1::2])
    np.testing.assert_array_equal(thinned["traj_logp"], unit["traj_logp"][1::2])
    ctx.set_inverse_mass(np.ones(d))
    ones = _run(ctx, state0, key, eps, N_RUN, limit)
    for name in unit:
        np.testing.assert_array_equal(ones[name], unit[name], err_msg="mass of ones: " + name)
    np.testing.assert_array_equal(_stepwise(ctx, state0, key, eps, N_RUN, limit)["pos"], unit["traj_pos"])      # (the step kernel's mass instances)
    ctx.close()


def test_prefix_property_and_depth_limit_on_the_device():
    ctx, pos0, _ = _ctx("phi4", 64, None)
    state0 = _init(ctx, pos0)
    key = prng.PRNGKey(31)
    a = _stepwise(ctx, state0, key, 0.05, 1, 3)
    b = _stepwise(ctx, state0, key, 0.05, 1, 4)
    m = a["depth"][0] < 3
    assert m.any() and (~m).any()
    for name in a:
        np.testing.assert_array_equal(a[name][0][m], b[name][0][m], err_msg=name)
    assert (b["num_leapfrog"][0][~m] >= a["num_leapfrog"][0][~m]).all()
    # the limit: at a tiny step nothing turns, every tree is cut at depth 2 after 1 + 2 leapfrog steps
    c = _stepwise(ctx, state0, key, 1e-5, 1, 2)
    assert (c["depth"] == 2).all() and (c["num_leapfrog"] == 3).all() and not c["is_turning"].any() and not c["is_divergent"].any()
    assert (np.abs(c["acceptance_rate"] - 1.0) < 1e-3).all()
    ctx.close()


def test_divergent_transitions_match_the_reference():
    """A step far beyond the integrator's stability limit: an ordinary finite-arithmetic path.  Flags and the unchanged states of the
    divergent chains against the reference."""
    import torch
    kind, d, tail, _ = CASES["phi4-64"]
    eps = 0.6
    start, _, _, _ = _burned("phi4-64", False)
    ctx, _, odist = _ctx(kind, d, tail)
    vg = targets.Tempered(odist, 1.0).value_and_grad
    pos, logp, grad = _init(ctx, torch.as_tensor(start).cuda())
    before = pos.cpu().numpy().copy()
    st = omala.MALAState(before.astype(np.float64), logp.cpu().numpy(), grad.cpu().numpy().astype(np.float64))
    buf = _dev_info(B)
    key = prng.PRNGKey(41)
    ctx.nuts_step(key, 1.0, eps, DEPTH, pos, logp, grad, **buf)
    st_o, info = nr.kernel(prng.split(key, B), st, vg, eps, DEPTH)
    assert info.is_divergent.sum() >= B // 4, info.is_divergent.sum()
    ok = ~_borderline(kind, st.logdensity, info)
    print(f"divergent {info.is_divergent.sum()} of {B}, compared {ok.sum()}")
    assert ok.mean() >= 0.75
    np.testing.assert_array_equal(buf["is_divergent"].cpu().numpy().astype(bool)[ok], info.is_divergent[ok])
    np.testing.assert_array_equal(buf["depth"].cpu().numpy()[ok], info.depth[ok])
    np.testing.assert_array_equal(buf["num_leapfrog"].cpu().numpy()[ok], info.num_leapfrog[ok])
    same = ok & (st_o.position == st.position).all(1)                          # the reference kept the state: so must the kernel, to the bit
    assert same.any()
    np.testing.assert_array_equal(pos.cpu().numpy()[same], before[same])
    assert np.isfinite(pos.cpu().numpy()).all()
    ctx.close()


def _one_mode_engine(n):
    import torch
    from mfm_amd import distributions as D
    from mfm_amd.engine import Engine
    from tests import gpu_util as gu
    args, _, _, model, _ = gu.gmm4_setup(B=n)
    args.ot_cond_flow = False
    mean, var = np.array([[1.0, -2.0]]), np.array([[0.25, 4.0]])
    dist = D.GaussianMixture(mean, var, np.ones(1))
    eng = Engine(dist, args, model.f)
    x = mean + np.sqrt(var) * np.random.default_rng(3).standard_normal((n, 2))
    return eng, dist, torch.as_tensor(x.astype(np.float32)).cuda(), mean[0], var[0]


def test_a_gaussian_is_sampled_with_the_right_moments():
    """A one-mode mixture (d = 2, variances 0.25 and 4) from exact draws, 64 chains x 512 transitions through ``.step.run``: means and
    variances within 6 standard errors, the effective sample size from ``chain_diagnostics``."""
    from mfm_amd import diagnostics, random as jr
    from mfm_amd.bblackjax.mcmc.nuts import nuts
    n, steps = 64, 512
    eng, dist, pos, mean, var = _one_mode_engine(n)
    algo = nuts(dist.logprob, 0.35, 8)
    _, info = algo.step.run(jr.PRNGKey(5), algo.init(pos), steps, thin=1)
    assert info.num_divergent.sum().item() == 0 and 1.0 <= info.mean_trajectory_expansions.mean().item() <= 8.0
    x = info.positions.double()
    for series, truth in ((x, mean), ((x - x.new_tensor(mean)) ** 2, var)):
        ess = diagnostics.chain_diagnostics(series.float().contiguous(), ctx=eng.ctx).ess.double().cpu().numpy()
        ess = np.minimum(ess, 4.0 * n * steps)                                 # (antithetic: capped, so that the error bar is not understated)
        flat = series.reshape(-1, 2).cpu().numpy()
        est, se = flat.mean(0), flat.std(0) / np.sqrt(ess)
        print("estimate", est, "truth", truth, "standard error", se, "ess", ess)
        assert (ess > 100).all() and (np.abs(est - truth) < 6 * se).all(), (est, truth, se)
    eng.close()


def test_api_inference_loop0_and_errors():
    import torch
    from mfm_amd import _lib, mcmc_utils, random as jr
    from mfm_amd.bblackjax.mcmc import nuts as N
    eng, dist, pos, _, _ = _one_mode_engine(NB)
    algo = N.nuts(dist.logprob, 0.3, max_num_doublings=5, inverse_mass_matrix=np.array([0.5, 2.0]))
    state = algo.init(pos)
    before = [t.clone() for t in state]
    key = jr.PRNGKey(6)
    new, info = algo.step(key, state)
    assert isinstance(new, N.NUTSState) and isinstance(info, N.NUTSInfo) and info.is_turning.dtype == torch.bool
    assert info.num_integration_steps.shape == (NB,) and (info.num_integration_steps >= 1).all() and (info.num_trajectory_expansions <= 5).all()
    run_state, run_info = algo.step.run(key, state, N_RUN, thin=1)
    assert isinstance(run_info, N.NUTSRunInfo) and run_info.positions.shape == (N_RUN, NB, 2)
    states, info0 = mcmc_utils.inference_loop0(key, state, algo.step, N_RUN)
    assert isinstance(info0, N.NUTSRunInfo) and states.logdensity_grad is None
    assert torch.equal(states.position, run_info.positions) and torch.equal(states.position[-1], run_state.position)
    h_states, h_infos = mcmc_utils.inference_loop0(key, state, lambda k, s: algo.step(k, s), N_RUN)      # the host loop: no .run
    assert torch.equal(h_states.position, run_info.positions) and torch.equal(h_states.logdensity, run_info.logdensities)
    assert torch.equal(h_infos.num_integration_steps.sum(0).long(), run_info.num_integration_steps)
    assert torch.equal(h_infos.energy[-1], run_info.last.energy)
    for t, b in zip(state, before):
        assert torch.equal(t, b)                                               # states are values
    eng.close()

    ctx, pos0, _ = _ctx("phi4", 64, None, NB)
    pos, logp, grad = _init(ctx, pos0)
    kept = pos.clone()
    tp = torch.empty(4, NB, 64, device="cuda")
    k = prng.PRNGKey(1)
    bad = [("max_tree_depth", lambda: ctx.nuts_step(k, 1.0, 1e-2, 0, pos, logp, grad)),
           ("max_tree_depth", lambda: ctx.nuts_step(k, 1.0, 1e-2, 17, pos, logp, grad)),
           ("divergence_threshold", lambda: ctx.nuts_step(k, 1.0, 1e-2, 5, pos, logp, grad, divergence_threshold=0.0)),
           ("step_size", lambda: ctx.nuts_step(k, 1.0, 0.0, 5, pos, logp, grad)),
           ("null device pointer", lambda: ctx.nuts_step(k, 1.0, 1e-2, 5, pos, None, grad)),
           ("key", lambda: ctx.nuts_step_keys(None, 1.0, 1e-2, 5, pos, logp, grad)),
           ("n_steps", lambda: ctx.nuts_run(k, 1.0, 1e-2, 5, 0, pos, logp, grad)),
           ("max_tree_depth", lambda: ctx.nuts_run(k, 1.0, 1e-2, 0, 4, pos, logp, grad)),
           ("thin", lambda: ctx.nuts_run(k, 1.0, 1e-2, 5, 4, pos, logp, grad, thin=-1, traj_pos=tp)),
           ("thin .* n_steps", lambda: ctx.nuts_run(k, 1.0, 1e-2, 5, 4, pos, logp, grad, thin=3, traj_pos=tp)),
           ("d_traj_pos", lambda: ctx.nuts_run(k, 1.0, 1e-2, 5, 4, pos, logp, grad, thin=2)),
           ("key_mode", lambda: ctx.nuts_run(k, 1.0, 1e-2, 5, 4, pos, logp, grad, key_mode=2)),
           ("d_keys", lambda: ctx.nuts_run(k, 1.0, 1e-2, 5, 4, pos, logp, grad, key_mode=1))]
    for match, call in bad:
        with pytest.raises(_lib.MfmError, match=match):
            call()
    assert torch.equal(pos, kept)                                              # a rejected call touches nothing
    ctx.close()
    from tests import gpu_util as gu
    args, dist512, *_ = gu.phi4_setup(d=512, B=NB, hidden=32, F=16)
    big = gu.make_ctx(dist512, args)
    bpos, blogp, bgrad = _init(big, torch.as_tensor(dist512.init_params.astype(np.float32)).cuda())
    kept = bpos.clone()
    with pytest.raises(_lib.MfmError, match="dim <= 256"):
        big.nuts_step(k, 1.0, 1e-2, 5, bpos, blogp, bgrad)
    with pytest.raises(_lib.MfmError, match="dim <= 256"):
        big.nuts_run(k, 1.0, 1e-2, 5, 4, bpos, blogp, bgrad)
    assert torch.equal(bpos, kept)
    big.close()
    args, cdist, *_ = gu.lgcp_setup(n=4, B=NB)
    cox = gu.make_ctx(cdist, args)
    cpos = torch.as_tensor(cdist.init_params.astype(np.float32)).cuda()
    clogp = torch.zeros(NB, dtype=torch.float64, device="cuda"); cgrad = torch.zeros_like(cpos)
    with pytest.raises(_lib.MfmError, match="Cox"):
        cox.nuts_step(k, 1.0, 1e-2, 5, cpos, clogp, cgrad)
    with pytest.raises(_lib.MfmError, match="Cox"):
        cox.nuts_run(k, 1.0, 1e-2, 5, 4, cpos, clogp, cgrad)
    cox.close()


def test_loop_and_ess_steps_with_the_nuts_kernel():
    """A tiny ``--mcmc_kernel nuts --ess_steps 64`` run: finite figures, and ``ess_per_grad`` is ``ess_per_step`` over the logged mean
    leapfrog count, which is the run's own (recomputed from ``nuts(...).step.run`` on the same final chains and key)."""
    from mfm_amd import distributions as D, exe_flow_matching as E, random as jr
    from mfm_amd.bblackjax.mcmc.nuts import nuts
    from oracle import loop
    kw = dict(example="phi-four", dim=64, num_chain=32, learning_iter=5, mcmc_per_flow_steps=4.0, hutchs=True, fourier_dim=16, seed=7, eval_iter=1,
              step_size=0.03, hidden_x=[32, 32], hidden_t=[32, 32], hidden_xt=[32, 32], ess_steps=64, mcmc_kernel="nuts", max_tree_depth=5)
    dist = D.PhiFour(64)
    args = loop.default_args(**kw)
    _, _, ex = E.run(dist, args, None, log_every=1000, return_extras=True)
    eng = ex["engine"]
    assert np.isfinite(ex["metrics"]).all()
    for name in ("min", "median", "mean"):
        for k in ("ess_per_step_", "ess_per_grad_", "ess_multichain_per_step_", "ess_multichain_per_grad_"):
            assert isinstance(ex[k + name], float) and np.isfinite(ex[k + name]), k + name
        assert ex["ess_per_grad_" + name] == ex["ess_per_step_" + name] / ex["nuts_mean_leapfrog"]
    assert np.isfinite(ex["rhat_max"]) and 1.0 <= ex["nuts_mean_depth"] <= 5.0 and ex["nuts_divergent"] == 0
    algo = nuts(dist.logprob, args.step_size, 5)
    _, info = algo.step.run(jr.split(ex["key_gen"], 3)[2], algo.init(ex["states"].position), 64, thin=1)
    mean_leap = info.num_integration_steps[:eng.n_valid].double().sum().item() / (64 * eng.n_valid)
    assert abs(ex["nuts_mean_leapfrog"] - mean_leap) < 1e-9 * mean_leap and 1.0 <= mean_leap <= 31.0
    eng.close()
