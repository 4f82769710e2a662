"""GPU tests of the step-size warmup, ``mfm_hmc_warmup`` / ``mfm_mala_warmup`` (mfm_amd/csrc/warmup.hip): many sampler steps in one
launch in which every chain adapts its own step size by dual averaging (the recursion: include/mfm.h).

The yardstick of the arithmetic is the single-step kernel.  The warmup keeps the step size every chain USED at every step; the REPLAY
makes, for each step m and each distinct step size among the chains, one launch of ``mfm_hmc_step_keys`` (``mfm_mala_step_keys`` with
``textbook = 1``) on a clone of the current state with that scalar step size and the warmup's step keys, and keeps the rows of the chains
that used it: final state and accepted counts must be bit-equal.  The RECURSION is checked by feeding the host restatement
(tests/warmup_ref.py) the replay's reported float32 acceptance probabilities: the rounding of p to float32, amplified by the
recursion's largest gain sqrt(n) / gamma, is the tolerance.  Then the closed loop against the float64 restatement (statistically: chain
histories part at the first flipped borderline decision), shard invariance, the argument errors, the Python kernels and ``--adapt_steps``.

Cases and step sizes are those of tests/test_gpu_hmc_run.py and tests/test_gpu_mala_run.py, 16 chains, 8 steps.  From a common start
the adaptation is the same for every chain while every chain's p is exactly 1 or 0 (the restatement on these inputs: p = 1, 0, 0, 1, 1,
1 at the first six HMC steps of the phi-four cases), so the chains' step sizes part late: at the eighth step for the phi-four HMC cases,
from the second for the mixture.  Every case, HMC and MALA, asserts that accepted and rejected steps both occur and that the chains'
step sizes differ at some step from the second on -- with one exception.  The MALA cases take the step sizes tuned for the rule AS
WRITTEN and run under the textbook rule; phi-four d = 256 at 3e-6 then has p of 0 or 1 in every chain for twelve steps (restatement:
the chains part at the thirteenth step and all sixteen differ from the sixteenth), so its 8-step case can only assert the accept /
reject mix, and the same case runs once more over 20 steps, where the MAXIT 4 instance sees sixteen step sizes and asserts both.
The recursion's tolerance follows the number of steps: 2 (sqrt(n) / gamma) 2^-24 + 1e-12."""
import numpy as np
import pytest

from oracle import prng
from tests import warmup_ref as wr
from tests.test_gpu_hmc_run import CASES as HMC_CASES, L, _ctx, _init, _keys_dev
from tests.test_gpu_mala_run import CASES as MALA_CASES

pytestmark = pytest.mark.gpu

B, N_STEPS, TARGET = 16, 8, 0.8
MALA_TARGET = 0.574


def _rtol_recursion(n_steps):
    """The rounding of p to float32, amplified by the recursion's largest gain over ``n_steps`` steps."""
    return 2 * (np.sqrt(n_steps) / wr.GAMMA) * 2.0 ** -24 + 1e-12


def _warmup(ctx, state0, key, beta, step0, n_steps, target, sampler="hmc", traj=True, **kw):
    import torch
    pos, logp, grad = (t.clone() for t in state0)
    n = pos.shape[0]
    f64 = dict(dtype=torch.float64, device="cuda")
    avg, last, acc_sum = torch.empty(n, **f64), torch.empty(n, **f64), torch.empty(n, **f64)
    n_acc = torch.empty(n, dtype=torch.int32, device="cuda")
    tr = torch.empty(n_steps, n, **f64) if traj else None
    key = _keys_dev(key) if np.ndim(key) == 2 else key
    if sampler == "hmc":
        ctx.hmc_warmup(key, beta, step0, L, n_steps, target, pos, logp, grad, avg, step_last=last, n_acc=n_acc, acc_sum=acc_sum, step_traj=tr, **kw)
    else:
        ctx.mala_warmup(key, beta, step0, n_steps, target, pos, logp, grad, avg, step_last=last, n_acc=n_acc, acc_sum=acc_sum, step_traj=tr, **kw)
    names = ("pos", "logp", "grad", "step_avg", "step_last", "n_acc", "acc_sum", "step_traj")
    return {k: (None if t is None else t.cpu().numpy()) for k, t in zip(names, (pos, logp, grad, avg, last, n_acc, acc_sum, tr))}


def _step_keys(key, n_steps, n_total=B, offset=0, n=B):
    """[n_steps, n, 2]: the per-chain key of every step, as mcmc_run_key derives it."""
    if np.ndim(key) == 2:
        return np.swapaxes(prng.split_rows(key, n_steps), 0, 1)
    return np.stack([prng.split(k, n_total)[offset:offset + n] for k in prng.split(key, n_steps)])


def _replay(ctx, state0, key, beta, step_traj, sampler="hmc"):
    """Single-step launches at the step sizes the warmup used; the final state, and per step the float32 acceptance probabilities and
    the decisions (numpy)."""
    import torch
    cur = [t.clone() for t in state0]
    n = cur[0].shape[0]
    acc = torch.empty(n, device="cuda"); isacc = torch.empty(n, dtype=torch.uint8, device="cuda")
    keys = _step_keys(key, len(step_traj))
    p_all, ia_all = [], []
    for m, row in enumerate(step_traj):
        nxt = [t.clone() for t in cur]
        p_m, ia_m = np.zeros(n, np.float32), np.zeros(n, bool)
        kd = _keys_dev(keys[m])
        for eps in np.unique(row):                                             # one launch per distinct step size; keep the chains that used it
            pos, logp, grad = (t.clone() for t in cur)
            if sampler == "hmc":
                ctx.hmc_step_keys(kd, beta, float(eps), L, pos, logp, grad, acc, isacc)
            else:
                ctx.mala_step_keys(kd, beta, float(eps), pos, logp, grad, acc, isacc, textbook=True)
            sel = torch.as_tensor(row == eps).cuda()
            for dst, src in zip(nxt, (pos, logp, grad)):
                dst[sel] = src[sel]
            p_m[row == eps] = acc.cpu().numpy()[row == eps]
            ia_m[row == eps] = isacc.cpu().numpy().astype(bool)[row == eps]
        cur = nxt
        p_all.append(p_m); ia_all.append(ia_m)
    return dict(pos=cur[0].cpu().numpy(), logp=cur[1].cpu().numpy(), grad=cur[2].cpu().numpy(), acc=np.stack(p_all), isacc=np.stack(ia_all))


def _assert_warmup_equals_replay(w, rep, step0, target):
    """The replay (bit-equal state and counts; the probability sum to the tolerance of test_gpu_hmc_run._assert_run_equals_steps) and
    the recursion on the replay's float32 probabilities."""
    n = rep["acc"].shape[0]
    print(f"mean acceptance probability {rep['acc'].astype(np.float64).mean():.4f}, accepted {rep['isacc'].sum()} of {rep['isacc'].size}; "
          f"distinct step sizes per step {[len(np.unique(r)) for r in w['step_traj']]}")
    for name in ("pos", "logp", "grad"):
        np.testing.assert_array_equal(w[name], rep[name], err_msg=name)
    np.testing.assert_array_equal(w["n_acc"], rep["isacc"].astype(np.int64).sum(0))
    np.testing.assert_allclose(w["acc_sum"], rep["acc"].astype(np.float64).sum(0), rtol=2.0 ** -24 + n * 2.0 ** -52, atol=n * 2.0 ** -150)
    np.testing.assert_array_equal(w["step_traj"][0], step0)                    # the caller's value itself, not exp(log(step0))
    traj, last, avg = wr.replay(rep["acc"], step0, target)
    rtol = _rtol_recursion(n)
    err = {k: np.abs(a / b - 1).max() for k, a, b in (("step_traj", w["step_traj"], traj), ("step_last", w["step_last"], last), ("step_avg", w["step_avg"], avg))}
    print(f"recursion: largest relative differences {err} (tolerance {rtol:.3g})")
    np.testing.assert_allclose(w["step_traj"], traj, rtol=rtol, atol=0)
    np.testing.assert_allclose(w["step_last"], last, rtol=rtol, atol=0)
    np.testing.assert_allclose(w["step_avg"], avg, rtol=rtol, atol=0)
    mixed = 0 < rep["isacc"].sum() < rep["isacc"].size                         # both branches of the select
    parted = max(len(np.unique(r)) for r in w["step_traj"][1:]) >= 2           # from step 2 on: the per-chain wiring
    return mixed, parted


# the "row_" cases: the warmup kernels on the dispatch instances above d = 256 and on MAXIT 4 with a run-time boundary (the tables of
# tests/test_gpu_hmc_run.py and tests/test_gpu_mala_run.py; start states near a mode, where the chains' step sizes part at the second step)
ROW = ["row_d65_pbc", "row_d257_d0", "row_17x17_pbc", "row_d2048_d0", "row_d1025_pbc", "row_33x33_db"]


@pytest.mark.parametrize("case", ["phi4_d64", "phi4_d100", "phi4_d256", "phi4_d64_pbc", "gmm4"] + ROW)
def test_hmc_warmup_replays_as_single_steps_and_follows_the_recursion(case):
    kind, d, tail, beta, step0 = HMC_CASES[case]
    ctx, pos0, _ = _ctx(kind, d, tail)
    state0 = _init(ctx, pos0, beta)
    key = prng.PRNGKey(21)
    w = _warmup(ctx, state0, key, beta, step0, N_STEPS, TARGET)
    mixed, parted = _assert_warmup_equals_replay(w, _replay(ctx, state0, key, beta, w["step_traj"]), step0, TARGET)
    assert mixed and parted, (mixed, parted)
    ctx.close()


def test_hmc_warmup_chain_major_keys():
    """key_mode 1 on phi-four d = 64: step j of chain b draws from split(keys[b], n)[j]."""
    kind, d, tail, beta, step0 = HMC_CASES["phi4_d64"]
    ctx, pos0, _ = _ctx(kind, d, tail)
    state0 = _init(ctx, pos0, beta)
    keys = prng.split(prng.PRNGKey(33), B)
    w = _warmup(ctx, state0, keys, beta, step0, N_STEPS, TARGET)
    mixed, parted = _assert_warmup_equals_replay(w, _replay(ctx, state0, keys, beta, w["step_traj"]), step0, TARGET)
    assert mixed and parted, (mixed, parted)
    ctx.close()


# (case, steps, whether the chains' step sizes part within those steps: module docstring)
MALA_RUNS = [("phi4_d64", N_STEPS, True), ("phi4_d256", N_STEPS, False), ("phi4_d256", 20, True), ("gmm4", N_STEPS, True)]
# (the MAXIT 1 run-time-boundary instance: as d = 256 at 8 steps, every chain's p is 0 or 1 until the eighth step of the restatement)
MALA_RUNS += [("phi4_d64_pbc", N_STEPS, False)] + [(c + "_textbook", N_STEPS, True) for c in ROW]


@pytest.mark.parametrize("case,n_steps,parts", MALA_RUNS, ids=[f"{c}-{n}" for c, n, _ in MALA_RUNS])
def test_mala_warmup_replays_as_single_steps_and_follows_the_recursion(case, n_steps, parts):
    """phi-four d = 64 (MAXIT 1), d = 256 (MAXIT 4) and the 4-mode mixture under the textbook rule; the periodic d = 64 chain and the
    "row_" cases (MAXIT 4 with a run-time boundary, MAXIT 16 and 32 with and without)."""
    kind, d, tail, beta, step0, _ = MALA_CASES[case]
    ctx, pos0, _ = _ctx(kind, d, tail)
    state0 = _init(ctx, pos0, beta)
    key = prng.PRNGKey(21)
    w = _warmup(ctx, state0, key, beta, step0, n_steps, MALA_TARGET, sampler="mala")
    mixed, parted = _assert_warmup_equals_replay(w, _replay(ctx, state0, key, beta, w["step_traj"], sampler="mala"), step0, MALA_TARGET)
    assert mixed and (parted or not parts), (mixed, parted)
    ctx.close()


@pytest.fixture(scope="module")
def restatement():
    """phi-four d = 64, 16 chains, L = 3, 40 steps from 0.003 and from 0.3: the restatement's pooled log step size for key 0, the one the
    device gets, and its spread over 8 keys.  Computed once on the CPU."""
    _, vg, state = wr.phi4_start(64, B)
    out = {}
    for step0 in (0.003, 0.3):
        logs = np.array([wr.pooled(wr.hmc_warmup(prng.PRNGKey(s), state, vg, step0, L, 40, TARGET)["step_avg"])[1] for s in range(8)])
        out[step0] = (logs[0], logs.std(ddof=1))
    return out


@pytest.mark.parametrize("step0", [0.003, 0.3])
def test_closed_loop_against_the_float64_restatement(step0, restatement):
    """The device's pooled log step size after 40 steps lies within 4 standard deviations of the restatement's for the same key; the
    standard deviation is the restatement's own spread over 8 keys.  On an MI355X: from 0.003 the device pools to 0.02345 (log -3.7528)
    and the restatement to 0.02346 (log -3.7525), spread 0.0224; from 0.3, 0.02327 (log -3.7605) against 0.02336 (log -3.7567), spread
    0.0237."""
    ctx, pos0, _ = _ctx("phi4", 64, None)
    state0 = _init(ctx, pos0, 1.0)
    w = _warmup(ctx, state0, prng.PRNGKey(0), 1.0, step0, 40, TARGET, traj=False)
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
    key, step0 = prng.PRNGKey(21), HMC_CASES["phi4_d64"][4]
    ctx = gu.make_ctx(dist, args)
    whole = _warmup(ctx, _init(ctx, pos0, 1.0), key, 1.0, step0, N_STEPS, TARGET)
    ctx.close()
    for off in (0, 16):
        part_ctx = gu.make_ctx(dist, args, n_local=16, n_total=32, offset=off)
        part = _warmup(part_ctx, _init(part_ctx, pos0[off:off + 16].contiguous(), 1.0), key, 1.0, step0, N_STEPS, TARGET)
        for name in ("step_avg", "step_last", "step_traj", "pos", "logp", "grad", "n_acc", "acc_sum"):
            np.testing.assert_array_equal(part[name], whole[name][..., off:off + 16] if name == "step_traj" else whole[name][off:off + 16], err_msg=name)
        part_ctx.close()
    assert len(np.unique(whole["step_avg"])) > 1


def test_argument_errors_name_the_argument():
    import torch
    from mfm_amd import _lib
    ctx, pos0, _ = _ctx("phi4", 64, None)
    pos, logp, grad = _init(ctx, pos0, 1.0)
    key = prng.PRNGKey(1)
    avg = torch.empty(B, dtype=torch.float64, device="cuda")
    before = pos.clone()
    for call, extra in ((ctx.hmc_warmup, (L,)), (ctx.mala_warmup, ())):
        def go(step0=1e-2, n_steps=4, target=0.8, key=key, avg=avg, lead=extra, **kw):
            call(key, 1.0, step0, *lead, n_steps, target, pos, logp, grad, avg, **kw)
        with pytest.raises(_lib.MfmError, match="n_steps"):
            go(n_steps=0)
        with pytest.raises(_lib.MfmError, match="step_size"):
            go(step0=0.0)
        for bad in (0.0, 1.0, -0.1, float("nan")):
            with pytest.raises(_lib.MfmError, match="target_accept"):
                go(target=bad)
        with pytest.raises(_lib.MfmError, match="key_mode"):
            go(key_mode=2)
        with pytest.raises(_lib.MfmError, match="d_keys"):
            go(key_mode=1)
        with pytest.raises(_lib.MfmError, match="d_step_avg"):
            go(avg=None)
        with pytest.raises(_lib.MfmError, match="step_traj"):
            go(step_traj=torch.empty(3, B, dtype=torch.float64, device="cuda"))        # 4 steps need 4 rows
    with pytest.raises(_lib.MfmError, match="num_steps"):
        ctx.hmc_warmup(key, 1.0, 1e-2, 0, 4, 0.8, pos, logp, grad, avg)
    with pytest.raises(_lib.MfmError, match="null device pointer"):
        ctx.hmc_warmup(key, 1.0, 1e-2, L, 4, 0.8, None, logp, grad, avg)
    with pytest.raises(_lib.MfmError, match="textbook"):
        ctx.mala_warmup(key, 1.0, 1e-4, 4, 0.574, pos, logp, grad, avg, textbook=False)
    assert torch.equal(pos, before)                                            # a rejected call touches nothing
    ctx.close()
    cox, cpos0, _ = _ctx("lgcp", 16, None)
    cpos, clogp, cgrad = _init(cox, cpos0, 1.0)
    with pytest.raises(_lib.MfmError, match="Cox"):
        cox.hmc_warmup(key, 1.0, 1e-2, L, 4, 0.8, cpos, clogp, cgrad, avg)
    with pytest.raises(_lib.MfmError, match="Cox"):
        cox.mala_warmup(key, 1.0, 1e-2, 4, 0.574, cpos, clogp, cgrad, avg)
    cox.close()


def test_python_kernels_return_what_the_context_call_returns():
    """``hmc.build_kernel().warmup``, ``hmc(...).step.warmup`` and ``mala.build_kernel(textbook=True).warmup`` against ``Context.hmc_warmup``
    / ``mala_warmup`` on the same key and state; ``step_sizes`` only when asked for; the as-written MALA kernel raises."""
    from mfm_amd import _lib, mcmc_utils, random as jr
    from mfm_amd.bblackjax.mcmc import hmc as H, mala as M
    from tests.test_gpu_hmc_run import _gmm_engine
    eng, dist, pos = _gmm_engine(B)
    step0 = HMC_CASES["gmm4"][4]
    algo = H.hmc(dist.logprob, step0, L)
    state = algo.init(pos)
    before = [t.clone() for t in state]
    key = jr.PRNGKey(6)
    direct = _warmup(eng.ctx, tuple(state), key, 1.0, step0, N_STEPS, TARGET)
    new, info = algo.step.warmup(key, state, N_STEPS, keep_step_sizes=True)
    assert isinstance(new, H.HMCState) and isinstance(info, H.HMCWarmupInfo)
    for t, b in zip(state, before):
        assert (t == b).all()                                                  # functional: the input state is not modified
    for got, name in ((new.position, "pos"), (new.logdensity, "logp"), (new.logdensity_grad, "grad"), (info.step_size, "step_avg"),
                      (info.last_step_size, "step_last"), (info.num_accepted, "n_acc"), (info.step_sizes, "step_traj")):
        np.testing.assert_array_equal(got.cpu().numpy(), direct[name], err_msg=name)
    np.testing.assert_array_equal(info.acceptance_rate.cpu().numpy(), direct["acc_sum"] / N_STEPS)
    assert info.pooled_step_size == mcmc_utils.pooled_step_size(info.step_size, eng.n_valid)
    assert info.pooled_step_size == pytest.approx(wr.pooled(direct["step_avg"])[0], rel=1e-14)
    _, info_k = H.build_kernel().warmup(key, state, dist.logprob, step0, L, N_STEPS, TARGET)
    assert info_k.step_sizes is None
    np.testing.assert_array_equal(info_k.step_size.cpu().numpy(), direct["step_avg"])
    keys = jr.split(jr.PRNGKey(7), B)                                          # per-chain keys: chain-major
    _, info_c = algo.step.warmup(keys, state, N_STEPS)
    np.testing.assert_array_equal(info_c.step_size.cpu().numpy(), _warmup(eng.ctx, tuple(state), keys, 1.0, step0, N_STEPS, TARGET)["step_avg"])
    # MALA: the textbook kernel carries the warmup (default target 0.574), the kernel as written raises from the library's message
    m_direct = _warmup(eng.ctx, tuple(state), key, 1.0, 1.5, N_STEPS, MALA_TARGET, sampler="mala")
    m_new, m_info = M.build_kernel(textbook=True).warmup(key, M.MALAState(*state), dist.logprob, 1.5, N_STEPS, keep_step_sizes=True)
    assert isinstance(m_new, M.MALAState)
    np.testing.assert_array_equal(m_info.step_size.cpu().numpy(), m_direct["step_avg"])
    np.testing.assert_array_equal(m_info.step_sizes.cpu().numpy(), m_direct["step_traj"])
    np.testing.assert_array_equal(m_new.position.cpu().numpy(), m_direct["pos"])
    with pytest.raises(_lib.MfmError, match="textbook"):
        M.build_kernel().warmup(key, M.MALAState(*state), dist.logprob, 1.5, N_STEPS)
    eng.close()


def test_adapt_steps_on_the_command_line_path(monkeypatch):
    """A tiny phi-four run with ``--mcmc_kernel hmc --adapt_steps 20``: the adapted step size is the pooled value of a direct ``warmup``
    on the same key (``split(key_gen, 4)[3]``) and initial chains, it replaces ``--step_size``, and the chains the training starts from
    are those of the same run with ``--adapt_steps 0``."""
    from mfm_amd import distributions as D, exe_flow_matching as E, random as jr
    from mfm_amd.bblackjax.mcmc.hmc import hmc
    from oracle import loop
    kw = dict(example="phi-four", dim=64, num_chain=32, learning_iter=3, mcmc_per_flow_steps=4.0, hutchs=True, fourier_dim=16, seed=7, eval_iter=1,
              step_size=0.03, hidden_x=[32, 32], hidden_t=[32, 32], hidden_xt=[32, 32], mcmc_kernel="hmc", hmc_steps=4)
    starts = []
    real = E.create_train_data_gn

    def spy(*a, **k):
        gen, init_fn, tr = real(*a, **k)

        def init_and_keep(pos, beta=1.0):
            st = init_fn(pos, beta)
            if not starts[-1]:
                starts[-1].extend(t.clone() for t in st)                       # the first call: the state the training starts from
            return st
        return gen, init_and_keep, tr
    monkeypatch.setattr(E, "create_train_data_gn", spy)

    starts.append([])
    dist = D.PhiFour(64)
    args = loop.default_args(adapt_steps=20, adapt_target=0.8, **kw)
    _, _, ex = E.run(dist, args, None, log_every=1000, return_extras=True)
    eng = ex["engine"]
    adapted = ex["adapted_step_size"]
    assert isinstance(adapted, float) and np.isfinite(adapted) and adapted > 0 and adapted != 0.03
    assert args.step_size == adapted
    assert 0.0 < ex["adapt_acceptance"] <= 1.0
    algo = hmc(dist.logprob, 0.03, 4)
    _, info = algo.step.warmup(jr.split(ex["key_gen"], 4)[3], algo.init(eng.local(dist.init_params)), 20, 0.8)
    assert info.pooled_step_size == adapted
    assert ex["adapt_acceptance"] == pytest.approx(info.acceptance_rate[:eng.n_valid].mean().item(), rel=1e-12)
    eng.close()

    starts.append([])
    args0 = loop.default_args(adapt_steps=0, **kw)
    _, _, ex0 = E.run(D.PhiFour(64), args0, None, log_every=1000, return_extras=True)
    assert "adapted_step_size" not in ex0 and args0.step_size == 0.03
    ex0["engine"].close()
    assert len(starts[0]) == 3 and len(starts[1]) == 3
    for a, b in zip(*starts):
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
