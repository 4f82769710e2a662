"""GPU tests of the NUTS warmup, ``mfm_nuts_warmup`` / ``mfm_nuts_warmup_window`` (mfm_amd/csrc/nuts_warmup.hip.h): many No-U-turn
transitions in one launch in which every chain adapts its own step size by dual averaging on its tree's acceptance statistic (the
recursion: include/mfm.h).

The yardstick of the arithmetic is the single-step kernel, as in tests/test_gpu_warmup.py.  The warmup keeps the step size every chain
USED at every transition; the REPLAY makes, for each transition m and each distinct step size among the chains, one launch of
``mfm_nuts_step_keys`` on a clone of the current state with that scalar step size and the warmup's step keys, and keeps the rows of the
chains that used it: final state and the trees' totals must be bit-equal.  The RECURSION is checked by feeding the host restatement
(tests/warmup_ref.py) the replay's float64 acceptance statistics: no float32 rounding of p enters, what remains is last-place
differences of exp / log and a possible contraction in the recursion times its gain sqrt(8) / 0.05 = 57, about 1e-14; the tolerance is
1e-12, the floor term of tests/test_gpu_warmup.py's.  Then chain-major keys, the closed loop against the float64 restatement
(statistically), shard invariance, the window's sums, the argument errors, the Python kernels and ``--nuts_adapt tree``.

Cases and step sizes are those of tests/test_gpu_nuts.py: 16 chains, 8 transitions, ``max_tree_depth`` 6, target 0.8, key
``PRNGKey(21)``, from the initial draw, each with unit mass and with ``hmc_mass_ref.log_spaced_mass(d)``.  Every case asserts that the
chains' step sizes differ at some transition from the second on and that at least three distinct tree depths occur.  The restatement
alone (tests/nuts_warmup_ref.py, on the CPU) meets both in every case but one -- distinct step sizes per transition: phi4-64 unit 1 1 1 1
2 10 14 16, mass 1 1 1 1 1 2 8 14; phi4-256 unit 1 1 1 1 1 1 3 12; phi4-48 unit 1 1 1 1 15 16 16 16, mass 1 1 1 12 12 15 16 16;
phi4-64-pbc unit 1 1 1 1 2 12 15 16, mass 1 1 1 1 1 2 7 13; gmm4 unit 1 7 7 8 13 16 16 16, mass 1 4 4 7 15 16 16 16; depths 0 to 6
everywhere (gmm4 mass: 0 to 5).  phi4-256 under the mass has p of 1, 0, 0, 1, 1, 1 in every chain and parts at the eighth transition
only (1 ... 1 2 7 12 15 16 over twelve), so that case runs 12 transitions.  phi4-128-limit14 is the same replay at ``max_tree_depth``
14, where the launch holds ONE chain per workgroup (tests/test_nuts_cases.py asserts it through ``mfm_nuts_launch_plan``); the step
kernel at that geometry is held to the reference in tests/test_gpu_nuts_instances.py."""
import numpy as np
import pytest

from oracle import prng
from tests import hmc_mass_ref as hm, nuts_warmup_ref as nw, warmup_ref as wr
from tests.test_gpu_nuts import CASES, _ctx, _dev_info, _init, _keys_dev
from tests.test_gpu_warmup import _step_keys

pytestmark = pytest.mark.gpu

B, N_STEPS, DEPTH, TARGET = 16, 8, 6, 0.8
RTOL = 1e-12
TOTALS = ("leapfrog_sum", "n_divergent", "depth_sum")
SHARED = ("pos", "logp", "grad", "step_avg", "step_last", "acc_sum", "step_traj") + TOTALS


def _warmup(ctx, state0, key, step0, n_steps, depth=DEPTH, target=TARGET, window=False, traj=True, **kw):
    import torch
    pos, logp, grad = (t.clone() for t in state0)
    n, d = pos.shape
    f64 = dict(dtype=torch.float64, device="cuda")
    out = dict(step_avg=torch.empty(n, **f64), step_last=torch.empty(n, **f64), acc_sum=torch.empty(n, **f64),
               step_traj=torch.empty(n_steps, n, **f64) if traj else None, leapfrog_sum=torch.empty(n, dtype=torch.int64, device="cuda"),
               n_divergent=torch.empty(n, dtype=torch.int32, device="cuda"), depth_sum=torch.empty(n, dtype=torch.int32, device="cuda"))
    key = _keys_dev(key) if np.ndim(key) == 2 else key
    avg = out.pop("step_avg")
    if window:
        sums = dict(pos_sum=torch.empty(n, d, **f64), pos_sumsq=torch.empty(n, d, **f64))
        ctx.nuts_warmup_window(key, 1.0, step0, depth, n_steps, target, pos, logp, grad, avg, sums["pos_sum"], sums["pos_sumsq"], **out, **kw)
        out.update(sums)
    else:
        ctx.nuts_warmup(key, 1.0, step0, depth, n_steps, target, pos, logp, grad, avg, **out, **kw)
    out.update(pos=pos, logp=logp, grad=grad, step_avg=avg)
    return {k: (None if t is None else t.cpu().numpy()) for k, t in out.items()}


def _replay(ctx, state0, key, step_traj, depth=DEPTH):
    """Single-transition launches at the step sizes the warmup used: the final state, and per transition the float64 acceptance
    statistic, the tree's depth, leapfrog count and divergence flag, and the position after it (numpy)."""
    import torch
    cur = [t.clone() for t in state0]
    n = cur[0].shape[0]
    buf = _dev_info(n)
    keys = _step_keys(key, len(step_traj))
    rec = {k: [] for k in ("acceptance_rate", "depth", "num_leapfrog", "is_divergent", "positions")}
    for m, row in enumerate(step_traj):
        nxt = [t.clone() for t in cur]
        got = {k: np.zeros(n, dtype=buf[k].cpu().numpy().dtype) for k in ("acceptance_rate", "depth", "num_leapfrog", "is_divergent")}
        kd = _keys_dev(keys[m])
        for eps in np.unique(row):                                             # one launch per distinct step size; keep the chains that used it
            pos, logp, grad = (t.clone() for t in cur)
            ctx.nuts_step_keys(kd, 1.0, float(eps), depth, pos, logp, grad, **buf)
            sel = torch.as_tensor(row == eps).cuda()
            for dst, src in zip(nxt, (pos, logp, grad)):
                dst[sel] = src[sel]
            for k in got:
                got[k][row == eps] = buf[k].cpu().numpy()[row == eps]
        cur = nxt
        for k in got:
            rec[k].append(got[k])
        rec["positions"].append(cur[0].cpu().numpy())
    out = {k: np.stack(v) for k, v in rec.items()}
    out.update(pos=cur[0].cpu().numpy(), logp=cur[1].cpu().numpy(), grad=cur[2].cpu().numpy())
    return out


def _assert_warmup_equals_replay(w, rep, step0, target=TARGET):
    """Bit-equal state and totals, the statistic's sum to n 2^-52, and the recursion on the replay's float64 statistics; returns whether
    the chains' step sizes part from the second transition on and how many distinct depths occurred."""
    n = rep["acceptance_rate"].shape[0]
    print(f"mean acceptance statistic {rep['acceptance_rate'].mean():.4f}; distinct step sizes per transition {[len(np.unique(r)) for r in w['step_traj']]}; "
          f"depths {np.bincount(rep['depth'].reshape(-1)).tolist()}; divergent {int(rep['is_divergent'].sum())}")
    for name in ("pos", "logp", "grad"):
        np.testing.assert_array_equal(w[name], rep[name], err_msg=name)
    np.testing.assert_array_equal(w["leapfrog_sum"], rep["num_leapfrog"].astype(np.int64).sum(0))
    np.testing.assert_array_equal(w["depth_sum"], rep["depth"].astype(np.int64).sum(0))
    np.testing.assert_array_equal(w["n_divergent"], rep["is_divergent"].astype(np.int64).sum(0))
    acc = np.zeros(rep["acceptance_rate"].shape[1])
    for a in rep["acceptance_rate"]:                                           # step order
        acc = acc + a
    np.testing.assert_allclose(w["acc_sum"], acc, rtol=n * 2.0 ** -52, atol=0)
    np.testing.assert_array_equal(w["step_traj"][0], step0)                    # the caller's value itself, not exp(log(step0))
    traj, last, avg = wr.replay(rep["acceptance_rate"], step0, target)
    err = {k: np.abs(a / b - 1).max() for k, a, b in (("step_traj", w["step_traj"], traj), ("step_last", w["step_last"], last), ("step_avg", w["step_avg"], avg))}
    print(f"recursion: largest relative differences {err} (tolerance {RTOL:.3g})")
    np.testing.assert_allclose(w["step_traj"], traj, rtol=RTOL, atol=0)
    np.testing.assert_allclose(w["step_last"], last, rtol=RTOL, atol=0)
    np.testing.assert_allclose(w["step_avg"], avg, rtol=RTOL, atol=0)
    parted = max(len(np.unique(r)) for r in w["step_traj"][1:]) >= 2           # from transition 2 on: the per-chain wiring
    return parted, len(np.unique(rep["depth"]))


# name: (target, d, phi-four block tail or None, first step size, max_tree_depth); d = 128 at limit 14 runs one chain per workgroup
REPLAY_CASES = {**{name: CASES[name] + (DEPTH,) for name in ("phi4-64", "phi4-256", "phi4-48", "phi4-64-pbc", "gmm4")},
                "phi4-128-limit14": ("phi4", 128, None, 0.03, 14)}
LONGER = {("phi4-256", True): 12}                                              # (module docstring)


@pytest.mark.parametrize("mass", [False, True], ids=["unit", "mass"])
@pytest.mark.parametrize("case", REPLAY_CASES)
def test_warmup_replays_as_single_transitions_and_follows_the_recursion(case, mass):
    kind, d, tail, step0, limit = REPLAY_CASES[case]
    n_steps = LONGER.get((case, mass), N_STEPS)
    ctx, pos0, _ = _ctx(kind, d, tail, B)
    ctx.set_inverse_mass(hm.log_spaced_mass(d) if mass else None)
    state0 = _init(ctx, pos0)
    key = prng.PRNGKey(21)
    w = _warmup(ctx, state0, key, step0, n_steps, depth=limit)
    parted, n_depths = _assert_warmup_equals_replay(w, _replay(ctx, state0, key, w["step_traj"], depth=limit), step0)
    assert parted and n_depths >= 3, (parted, n_depths)
    ctx.close()


def test_chain_major_keys():
    """key_mode 1 on phi-four d = 64: transition j of chain b draws from split(keys[b], n)[j]."""
    kind, d, tail, step0 = CASES["phi4-64"]
    ctx, pos0, _ = _ctx(kind, d, tail, B)
    state0 = _init(ctx, pos0)
    keys = prng.split(prng.PRNGKey(33), B)
    w = _warmup(ctx, state0, keys, step0, N_STEPS)
    parted, n_depths = _assert_warmup_equals_replay(w, _replay(ctx, state0, keys, w["step_traj"]), step0)
    assert parted and n_depths >= 3, (parted, n_depths)
    ctx.close()


@pytest.fixture(scope="module")
def restatement():
    """phi-four d = 64, 16 chains, max_tree_depth 6, 40 transitions from 0.003 and from 0.3: the restatement's pooled log step size for
    key 0, the one the device gets, and its spread over 8 keys.  Computed once on the CPU."""
    _, vg, state = wr.phi4_start(64, B)
    out = {}
    for step0 in (0.003, 0.3):
        logs = np.array([wr.pooled(nw.nuts_warmup(prng.PRNGKey(s), state, vg, step0, 40, TARGET, DEPTH)["step_avg"])[1] for s in range(8)])
        out[step0] = (logs[0], logs.std(ddof=1))
    return out


@pytest.mark.parametrize("step0", [0.003, 0.3])
def test_closed_loop_against_the_float64_restatement(step0, restatement):
    """The device's pooled log step size after 40 transitions lies within 4 standard deviations of the restatement's for the same key;
    the standard deviation is the restatement's own spread over keys 0 to 7.  The restatement on the CPU: from 0.003 it pools to 0.02717
    (log -3.6055), spread 0.0159; from 0.3 to 0.02793 (log -3.5780), spread 0.0174.  On an MI355X: from 0.003 the device
    pools to 0.02828 (log -3.5658), 2.5 spreads away; from 0.3 to 0.02785 (log -3.5810), 0.2 spreads."""
    ctx, pos0, _ = _ctx("phi4", 64, None, B)
    state0 = _init(ctx, pos0)
    w = _warmup(ctx, state0, prng.PRNGKey(0), step0, 40, traj=False)
    dev = wr.pooled(w["step_avg"])[1]
    ref, sd = restatement[step0]
    print(f"step0 {step0}: device pooled step size {np.exp(dev):.5f} (log {dev:.4f}), restatement {np.exp(ref):.5f} (log {ref:.4f}), spread over 8 keys {sd:.4f}")
    assert abs(dev - ref) <= 4 * sd, (dev, ref, sd)
    ctx.close()


def test_shard_invariance():
    """Step-major keys: 32 chains in one context against two contexts of 16 with chain_offset 0 / 16 of n_chain_total = 32."""
    import torch
    from tests import gpu_util as gu
    args, dist, k, model, state = gu.phi4_setup(d=64, B=32, hidden=32, F=16)
    pos0 = torch.as_tensor(dist.init_params.astype(np.float32)).cuda()
    key, step0 = prng.PRNGKey(21), CASES["phi4-64"][3]
    ctx = gu.make_ctx(dist, args)
    whole = _warmup(ctx, _init(ctx, pos0), key, step0, N_STEPS)
    ctx.close()
    for off in (0, 16):
        part_ctx = gu.make_ctx(dist, args, n_local=16, n_total=32, offset=off)
        part = _warmup(part_ctx, _init(part_ctx, pos0[off:off + 16].contiguous()), key, step0, N_STEPS)
        for name in SHARED:
            np.testing.assert_array_equal(part[name], whole[name][..., off:off + 16] if name == "step_traj" else whole[name][off:off + 16], err_msg=name)
        part_ctx.close()
    assert len(np.unique(whole["step_avg"])) > 1


@pytest.mark.parametrize("case", ["phi4-64", "phi4-256", "gmm4"])
def test_window_has_the_warmups_bits_and_the_sums_of_the_replay(case):
    """``nuts_warmup_window`` with no mass installed and with ones installed against ``nuts_warmup`` (the unit instances) in everything
    they share; ``pos_sum`` / ``pos_sumsq`` against float64 sums, in step order, of the replay's positions and of their squares."""
    kind, d, tail, step0 = CASES[case]
    ctx, pos0, _ = _ctx(kind, d, tail, B)
    state0 = _init(ctx, pos0)
    key = prng.PRNGKey(21)
    plain = _warmup(ctx, state0, key, step0, N_STEPS)
    bare = _warmup(ctx, state0, key, step0, N_STEPS, window=True)
    assert not ctx.get_inverse_mass()[1]                                       # nothing was installed by the call
    rep = _replay(ctx, state0, key, plain["step_traj"])
    ctx.set_inverse_mass(np.ones(d))
    ones = _warmup(ctx, state0, key, step0, N_STEPS, window=True)
    for name in SHARED:
        np.testing.assert_array_equal(bare[name], plain[name], err_msg="no mass installed: " + name)
        np.testing.assert_array_equal(ones[name], plain[name], err_msg="ones installed: " + name)
    s, q = np.zeros((B, d)), np.zeros((B, d))
    for x in rep["positions"]:
        v = x.astype(np.float64)
        s = s + v
        q = q + v * v
    for win in (bare, ones):
        np.testing.assert_array_equal(win["pos_sum"], s)
        np.testing.assert_array_equal(win["pos_sumsq"], q)
    assert (rep["positions"][-1] != rep["positions"][0]).any() and len(np.unique(plain["step_traj"][-1])) > 1
    ctx.close()


def test_argument_errors_name_the_argument():
    import torch
    from mfm_amd import _lib
    from tests import gpu_util as gu
    ctx, pos0, _ = _ctx("phi4", 64, None, B)
    pos, logp, grad = _init(ctx, pos0)
    key = prng.PRNGKey(1)
    f64 = dict(dtype=torch.float64, device="cuda")
    avg, s, q = torch.empty(B, **f64), torch.empty(B, 64, **f64), torch.empty(B, 64, **f64)
    before = [t.clone() for t in (pos, logp, grad)]

    def plain(step0=1e-2, depth=5, n_steps=4, target=0.8, key=key, avg=avg, **kw):
        ctx.nuts_warmup(key, 1.0, step0, depth, n_steps, target, pos, logp, grad, avg, **kw)

    def window(step0=1e-2, depth=5, n_steps=4, target=0.8, key=key, avg=avg, s=s, q=q, **kw):
        ctx.nuts_warmup_window(key, 1.0, step0, depth, n_steps, target, pos, logp, grad, avg, s, q, **kw)
    for go in (plain, window):
        with pytest.raises(_lib.MfmError, match="n_steps"):
            go(n_steps=0)
        with pytest.raises(_lib.MfmError, match="step_size"):
            go(step0=0.0)
        for bad in (0.0, 1.0):
            with pytest.raises(_lib.MfmError, match="target_accept"):
                go(target=bad)
        for bad in (0, 17):
            with pytest.raises(_lib.MfmError, match="max_tree_depth"):
                go(depth=bad)
        with pytest.raises(_lib.MfmError, match="divergence_threshold"):
            go(divergence_threshold=0.0)
        with pytest.raises(_lib.MfmError, match="d_step_avg"):
            go(avg=None)
        with pytest.raises(_lib.MfmError, match="key_mode"):
            go(key_mode=2)
        with pytest.raises(_lib.MfmError, match="d_keys"):
            go(key_mode=1)
    with pytest.raises(_lib.MfmError, match="d_pos_sum"):
        window(s=None)
    with pytest.raises(_lib.MfmError, match="d_pos_sumsq"):
        window(q=None)
    for t, b in zip((pos, logp, grad), before):
        assert torch.equal(t, b)                                               # a rejected call touches nothing
    assert not ctx.get_inverse_mass()[1]
    ctx.close()
    args, dist512, *_ = gu.phi4_setup(d=512, B=B, hidden=32, F=16)
    big = gu.make_ctx(dist512, args)
    bpos, blogp, bgrad = _init(big, torch.as_tensor(dist512.init_params.astype(np.float32)).cuda())
    kept = bpos.clone()
    bs = torch.empty(B, 512, **f64)
    with pytest.raises(_lib.MfmError, match="dim <= 256"):
        big.nuts_warmup(key, 1.0, 1e-2, 5, 4, 0.8, bpos, blogp, bgrad, avg)
    with pytest.raises(_lib.MfmError, match="dim <= 256"):
        big.nuts_warmup_window(key, 1.0, 1e-2, 5, 4, 0.8, bpos, blogp, bgrad, avg, bs, bs.clone())
    assert torch.equal(bpos, kept)
    big.close()
    args, cdist, *_ = gu.lgcp_setup(n=4, B=B)
    cox = gu.make_ctx(cdist, args)
    cpos = torch.as_tensor(cdist.init_params.astype(np.float32)).cuda()
    clogp = torch.zeros(B, dtype=torch.float64, device="cuda"); cgrad = torch.zeros_like(cpos)
    kept = cpos.clone()
    cs = torch.empty(B, cpos.shape[1], **f64)
    with pytest.raises(_lib.MfmError, match="Cox"):
        cox.nuts_warmup(key, 1.0, 1e-2, 5, 4, 0.8, cpos, clogp, cgrad, avg)
    with pytest.raises(_lib.MfmError, match="Cox"):
        cox.nuts_warmup_window(key, 1.0, 1e-2, 5, 4, 0.8, cpos, clogp, cgrad, avg, cs, cs.clone())
    assert torch.equal(cpos, kept)
    cox.close()


def test_python_kernel_returns_what_the_context_call_returns():
    """``nuts(...).step.warmup`` and ``build_kernel().warmup`` against ``Context.nuts_warmup`` on the same key and state; ``step_sizes``
    only when asked for; the input state is left as it was."""
    from mfm_amd import mcmc_utils, random as jr
    from mfm_amd.bblackjax.mcmc import nuts as N
    from tests.test_gpu_hmc_run import _gmm_engine
    eng, dist, pos = _gmm_engine(B)
    step0 = CASES["gmm4"][3]
    algo = N.nuts(dist.logprob, step0, DEPTH)
    state = algo.init(pos)
    before = [t.clone() for t in state]
    key = jr.PRNGKey(6)
    direct = _warmup(eng.ctx, tuple(state), key, step0, N_STEPS)
    new, info = algo.step.warmup(key, state, N_STEPS, return_step_sizes=True)
    assert isinstance(new, N.NUTSState) and isinstance(info, N.NUTSWarmupInfo)
    for t, b in zip(state, before):
        assert (t == b).all()                                                  # states are values
    for got, name in ((new.position, "pos"), (new.logdensity, "logp"), (new.logdensity_grad, "grad"), (info.step_size, "step_avg"),
                      (info.num_integration_steps, "leapfrog_sum"), (info.num_divergent, "n_divergent"), (info.step_sizes, "step_traj")):
        np.testing.assert_array_equal(got.cpu().numpy(), direct[name], err_msg=name)
    np.testing.assert_array_equal(info.acceptance_rate.cpu().numpy(), direct["acc_sum"] / N_STEPS)
    np.testing.assert_array_equal(info.mean_depth.cpu().numpy(), direct["depth_sum"].astype(np.float64) / N_STEPS)
    assert info.pooled_step_size == mcmc_utils.pooled_step_size(info.step_size, eng.n_valid)
    assert info.pooled_step_size == pytest.approx(wr.pooled(direct["step_avg"])[0], rel=1e-14)
    _, info_k = N.build_kernel().warmup(key, state, dist.logprob, step0, N_STEPS, TARGET, max_num_doublings=DEPTH)
    assert info_k.step_sizes is None
    np.testing.assert_array_equal(info_k.step_size.cpu().numpy(), direct["step_avg"])
    keys = jr.split(jr.PRNGKey(7), B)                                          # per-chain keys: chain-major
    _, info_c = algo.step.warmup(keys, state, N_STEPS)
    np.testing.assert_array_equal(info_c.step_size.cpu().numpy(), _warmup(eng.ctx, tuple(state), keys, step0, N_STEPS)["step_avg"])
    eng.close()


def test_nuts_window_adaptation_gives_parameters_that_nuts_takes():
    """phi-four d = 64, 32 chains, 100 steps: a finite positive step size and mass, ``window_schedule(100)`` in the info, the context left
    at unit mass, and the parameters run through ``nuts(..., inverse_mass_matrix=...)``."""
    import torch
    from mfm_amd import distributions as D, random as jr
    from mfm_amd.bblackjax.adaptation.window_adaptation import NUTSWindowAdaptationInfo, nuts_window_adaptation, window_schedule
    from mfm_amd.bblackjax.mcmc import nuts as N
    from mfm_amd.engine import Engine
    from oracle import loop
    dist = D.PhiFour(64)
    dist.initialize_model(jr.PRNGKey(3), 32)
    args = loop.default_args(example="phi-four", dim=64, num_chain=32, fourier_dim=16, hidden_x=[32, 32], hidden_t=[32, 32], hidden_xt=[32, 32])
    eng = Engine(dist, args, None)
    state = N.init(torch.as_tensor(dist.init_params.astype(np.float32)).cuda(), dist.logprob)
    new, params, info = nuts_window_adaptation(dist.logprob, DEPTH, 0.03).run(jr.PRNGKey(0), state, 100)
    step, minv = params["step_size"], params["inverse_mass_matrix"]
    print(f"step size {step:.5f}; mass min {minv.min():.4g} max {minv.max():.4g}; per segment: step sizes {info.step_sizes}, acceptance "
          f"{info.acceptance_rates}, mean leapfrog {info.mean_integration_steps}")
    assert isinstance(info, NUTSWindowAdaptationInfo) and info.schedule == window_schedule(100)
    assert len(info.step_sizes) == len(info.acceptance_rates) == len(info.mean_integration_steps) == len(info.schedule)
    assert len(info.inverse_mass_matrices) == sum(kind == "slow" for kind, _, _ in info.schedule) >= 1
    assert isinstance(step, float) and np.isfinite(step) and step > 0
    assert minv.shape == (64,) and minv.dtype == np.float64 and np.isfinite(minv).all() and (minv > 0).all()
    assert all(1.0 <= m <= 2 ** DEPTH - 1 for m in info.mean_integration_steps) and all(0.0 < a <= 1.0 for a in info.acceptance_rates)
    assert not eng.ctx.get_inverse_mass()[1] and not torch.equal(new.position, state.position)
    algo = N.nuts(dist.logprob, step, DEPTH, inverse_mass_matrix=minv)
    nxt, step_info = algo.step(jr.PRNGKey(1), new)
    assert torch.isfinite(nxt.position).all() and (step_info.num_integration_steps >= 1).all()
    eng.close()


@pytest.mark.parametrize("adapt_mass", [False, True], ids=["step", "mass"])
def test_nuts_adapt_tree_on_the_command_line_path(adapt_mass):
    """A 5-iteration phi-four run with ``--mcmc_kernel nuts --adapt_steps 30 --nuts_adapt tree --max_tree_depth 5``: finite figures in the
    extras, the mean leapfrog count inside a depth-5 tree's range, and the adapted value replaces ``--step_size``; with ``--adapt_mass``
    the two mass figures too.  Without the mass the value is the pooled one of a direct ``warmup`` on ``split(key_gen, 4)[3]``."""
    from mfm_amd import distributions as D, exe_flow_matching as E, random as jr
    from mfm_amd.bblackjax.mcmc.nuts import nuts
    from oracle import loop
    kw = dict(example="phi-four", dim=64, num_chain=32, learning_iter=5, mcmc_per_flow_steps=4.0, hutchs=True, fourier_dim=16, seed=7, eval_iter=1,
              step_size=0.03, hidden_x=[32, 32], hidden_t=[32, 32], hidden_xt=[32, 32], mcmc_kernel="nuts", max_tree_depth=5, adapt_steps=30,
              adapt_target=0.8, nuts_adapt="tree", hmc_steps=-1)                # (--hmc_steps plays no part: an HMC warmup would refuse -1)
    dist = D.PhiFour(64)
    args = loop.default_args(adapt_mass=adapt_mass, **kw)
    _, _, ex = E.run(dist, args, None, log_every=1000, return_extras=True)
    eng = ex["engine"]
    for name in ("adapted_step_size", "adapt_acceptance", "adapt_mean_leapfrog"):
        assert isinstance(ex[name], float) and np.isfinite(ex[name]), name
    assert ex["adapted_step_size"] > 0 and args.step_size == ex["adapted_step_size"] and ex["adapted_step_size"] != 0.03
    assert 0.0 < ex["adapt_acceptance"] <= 1.0 and 1.0 <= ex["adapt_mean_leapfrog"] <= 31.0
    assert np.isfinite(ex["metrics"]).all()
    if adapt_mass:
        minv = ex["adapted_inverse_mass"]
        assert minv.shape == (64,) and np.isfinite(minv).all() and (minv > 0).all()
        assert ex["adapted_inverse_mass_min"] == minv.min() and ex["adapted_inverse_mass_max"] == minv.max()
        got, is_set = eng.ctx.get_inverse_mass()
        assert is_set
        np.testing.assert_array_equal(got, minv)
    else:
        assert "adapted_inverse_mass" not in ex and not eng.ctx.get_inverse_mass()[1]
        algo = nuts(dist.logprob, 0.03, 5)
        _, info = algo.step.warmup(jr.split(ex["key_gen"], 4)[3], algo.init(eng.local(dist.init_params)), 30, 0.8)
        assert info.pooled_step_size == ex["adapted_step_size"]
    eng.close()
