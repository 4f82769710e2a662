"""GPU tests of ``mfm_pt_run`` / ``mfm_pt_exchange`` (mfm_amd/csrc/pt.hip) and of the Python layers on them.

Every case of tests/pt_cases.py runs ONCE (``_record``): the control run without exchange, the run itself, and its replay by the host loop
of the two pieces -- per round one ``mfm_hmc_run`` / ``mfm_mala_run`` of the whole batch per temperature at the scalars
``(beta_k, eps_k)`` on the round's key, rows ``k::K`` taken, then ``mfm_pt_exchange`` on the round's sweep key -- during which every sweep is
predicted exactly from the device state.  The tests share that record and leave it unchanged:

* local moves: with ``exchange = 0`` every chain has the bits of the scalar launches and the tallies are their sums over rounds;
* sweep, exact: candidates from ``Context.mala_init`` on the partner-swapped positions at each ``beta_k``, ``delta`` and ``p`` from those
  doubles in numpy, ``u`` from ``oracle/prng``; no ``|u - p| < 1e-6``; every decision as predicted; accepted pairs hold exactly the
  swapped rows and the candidate values; every other row bit-unchanged (unpaired slots, rows from ``K R`` on); ``replica`` permuted to
  match; the swap tallies;
* replay: ``mfm_pt_run`` is bit-identical with that loop, and its slot-0 trajectory equals the loop's slot-0 rows;
* end to end: against tests/pt_ref.py within ``pt_cases.TOLERANCE``, with identical decisions.

Then the sampling property on the device, the refusals, and the Python API and ``--do_pt``."""
import functools

import numpy as np
import pytest

from oracle import prng
from tests import pt_cases as pc, pt_ref as pr

pytestmark = pytest.mark.gpu


def _ctx(case):
    import torch
    from mfm_amd import _lib
    from tests import gpu_util as gu
    c = pc.CASES[case]
    B = pc.n_chains(case)
    if c["target"] == "gmm4":
        args, dist, *_ = gu.gmm4_setup(B=B)
    else:
        args, dist, *_ = gu.phi4_setup(d=c["d"], B=B, hidden=32, F=16)
    ctx = gu.make_ctx(dist, args)
    if pc.block(case) is not None:
        ctx.set_target(_lib.PHI4, pc.block(case))
    return ctx, torch.as_tensor(pc.start_state(case)).cuda()


def _init_slots(ctx, pos0, betas, KR):
    """Every slot at its own beta; the rows from K R on at beta = 1 (any finite values: they must come back untouched)."""
    import torch
    K = len(betas)
    pos = pos0.clone()
    logp = torch.empty(pos.shape[0], dtype=torch.float64, device="cuda"); grad = torch.empty_like(pos)
    ctx.mala_init(pos, 1.0, logp, grad)
    lp_k, g_k = torch.empty_like(logp), torch.empty_like(grad)
    for k, b in enumerate(betas):
        ctx.mala_init(pos, float(b), lp_k, g_k)
        logp[k:KR:K] = lp_k[k:KR:K]; grad[k:KR:K] = g_k[k:KR:K]
    return pos, logp, grad


def _scalar_round(ctx, c, betas, eps, key, state, KR, tallies=None):
    """One round's local moves by the EXISTING entry points: per temperature the whole batch at the scalars, rows k::K taken."""
    import torch
    K = len(betas)
    pos, logp, grad = state
    out = [t.clone() for t in state]
    B = pos.shape[0]
    for k in range(K):
        p, l, g = pos.clone(), logp.clone(), grad.clone()
        n_acc = torch.empty(B, dtype=torch.int32, device="cuda"); acc_sum = torch.empty(B, dtype=torch.float64, device="cuda")
        if c["kernel"] == "hmc":
            ctx.hmc_run(key, float(betas[k]), float(eps[k]), c["L"], c["n_local"], p, l, g, n_acc=n_acc, acc_sum=acc_sum)
        else:
            ctx.mala_run(key, float(betas[k]), float(eps[k]), c["n_local"], p, l, g, n_acc=n_acc, acc_sum=acc_sum, textbook=True)
        for dst, src in zip(out, (p, l, g)):
            dst[k:KR:K] = src[k:KR:K]
        if tallies is not None:
            tallies[0][k:KR:K] += n_acc[k:KR:K]
            tallies[1][k:KR:K] = tallies[1][k:KR:K] + acc_sum[k:KR:K]
    return tuple(out)


def _predict_sweep(ctx, betas, key, parity, state, K, R, n_total):
    """The sweep from the device state: ``(lower slots, u, p, decisions, candidate logp, candidate grad)`` -- candidates from
    ``Context.mala_init`` on the partner-swapped positions at each beta, delta and p in numpy, u from oracle/prng."""
    import torch
    pos, logp, grad = state
    KR = K * R
    lower = np.array([r * K + k for k in range(parity, K - 1, 2) for r in range(R)], dtype=np.int64)
    swapped = pos.clone()
    if lower.size:
        li = torch.as_tensor(lower).cuda()
        swapped[li], swapped[li + 1] = pos[li + 1], pos[li]
    cand_lp, cand_g = logp.clone(), grad.clone()
    lp_k, g_k = torch.empty_like(logp), torch.empty_like(grad)
    for k, b in enumerate(betas):
        ctx.mala_init(swapped, float(b), lp_k, g_k)
        cand_lp[k:KR:K] = lp_k[k:KR:K]; cand_g[k:KR:K] = g_k[k:KR:K]
    c_lp, lp = cand_lp.cpu().numpy(), logp.cpu().numpy()
    delta = (c_lp[lower] + c_lp[lower + 1]) - (lp[lower] + lp[lower + 1])
    delta = np.where(np.isnan(delta), -np.inf, delta)
    with np.errstate(over="ignore"):
        p = np.minimum(np.exp(delta), 1.0)
    u = prng.uniform_rows(prng.split(key, n_total)[lower]) if lower.size else np.zeros(0)
    return lower, u, p, u < p, swapped, cand_lp, cand_g


def _checked_sweep(ctx, case, betas, key, parity, state, replica, swap_acc, swap_prob, K, R):
    """``mfm_pt_exchange`` in place, checked against its exact prediction; returns the margin and the decisions."""
    import torch
    pos, logp, grad = state
    n_total = pos.shape[0]
    lower, u, p, dec, swapped, cand_lp, cand_g = _predict_sweep(ctx, betas, key, parity, state, K, R, n_total)
    margin = float(np.abs(u - p).min()) if lower.size else np.inf
    assert margin >= 1e-6, (case, parity, margin)                        # the margin first
    before = [t.clone() for t in (pos, logp, grad, replica, swap_acc, swap_prob)]
    ctx.pt_exchange(key, betas, R, parity, pos, logp, grad, replica=replica, swap_accepted=swap_acc, swap_prob=swap_prob)
    want = [t.clone() for t in before[:4]]
    acc_rows = lower[dec]
    if acc_rows.size:
        a = torch.as_tensor(np.concatenate([acc_rows, acc_rows + 1])).cuda()
        want[0][a] = swapped[a]; want[1][a] = cand_lp[a]; want[2][a] = cand_g[a]
        ai = torch.as_tensor(acc_rows).cuda()
        want[3][ai], want[3][ai + 1] = before[3][ai + 1], before[3][ai]
    moved = (pos != before[0]).any(1).cpu().numpy()
    got_dec = moved[lower] if lower.size else np.zeros(0, bool)
    np.testing.assert_array_equal(got_dec, dec, err_msg=f"{case}: decisions of parity {parity}")
    for name, g_, w_ in zip(("pos", "logp", "grad", "replica"), (pos, logp, grad, replica), want):
        assert torch.equal(g_, w_), (case, parity, name)                 # accepted pairs exactly swapped, every other row bit-unchanged
    w_acc, w_prob = before[4].cpu().numpy().copy(), before[5].cpu().numpy().copy()
    w_acc[lower // K, lower % K] += dec
    w_prob[lower // K, lower % K] += p
    np.testing.assert_array_equal(swap_acc.cpu().numpy(), w_acc)
    np.testing.assert_allclose(swap_prob.cpu().numpy(), w_prob, rtol=1e-12, atol=0)        # (exp of the device's libm against numpy's)
    touched = np.zeros((R, K - 1), bool); touched[lower // K, lower % K] = True
    np.testing.assert_array_equal(swap_prob.cpu().numpy()[~touched], before[5].cpu().numpy()[~touched])
    return margin, dec


def _pt_run(ctx, case, state, exchange, thin=1):
    import torch
    c = pc.CASES[case]
    K, R, d = c["K"], c["R"], c["d"]
    KR = K * R
    pos, logp, grad = (t.clone() for t in state)
    i32 = dict(dtype=torch.int32, device="cuda"); f64 = dict(dtype=torch.float64, device="cuda")
    n_acc = torch.full((KR,), -7, **i32); acc_sum = torch.full((KR,), -7.0, **f64)               # (the call zeroes its tallies)
    replica = torch.arange(KR, **i32)
    swap_acc = torch.full((R, K - 1), -7, **i32); swap_prob = torch.full((R, K - 1), -7.0, **f64)
    n_keep = c["n_rounds"] // thin if thin else 0
    tp = torch.zeros(n_keep, R, d, device="cuda") if thin else None
    tl = torch.zeros(n_keep, R, **f64) if thin else None
    ctx.pt_run(pc.key(case), pc.betas(case), pc.step_sizes(case), R, c["n_local"], c["n_rounds"], pos, logp, grad, kernel=c["kernel"], num_steps=c["L"],
               textbook=True, exchange=exchange, thin=thin, n_acc=n_acc, acc_sum=acc_sum, replica=replica, swap_accepted=swap_acc, swap_prob=swap_prob,
               traj_pos=tp, traj_logp=tl)
    names = ("pos", "logp", "grad", "n_acc", "acc_sum", "replica", "swap_accepted", "swap_prob", "traj_pos", "traj_logp")
    return {k: (None if t is None else t.cpu().numpy()) for k, t in zip(names, (pos, logp, grad, n_acc, acc_sum, replica, swap_acc, swap_prob, tp, tl))}


@functools.lru_cache(maxsize=None)
def _record(case):
    import torch
    c = pc.CASES[case]
    K, R = c["K"], c["R"]
    KR = K * R
    betas, eps = pc.betas(case), pc.step_sizes(case)
    ctx, pos0 = _ctx(case)
    state0 = _init_slots(ctx, pos0, betas, KR)
    out = dict(state0=[t.cpu().numpy() for t in state0])
    out["control"] = _pt_run(ctx, case, state0, exchange=False, thin=0)
    out["run"] = _pt_run(ctx, case, state0, exchange=True, thin=1)
    i32 = dict(dtype=torch.int32, device="cuda"); f64 = dict(dtype=torch.float64, device="cuda")
    # the control by the existing entry points
    st = tuple(t.clone() for t in state0)
    tallies = (torch.zeros(pos0.shape[0], **i32), torch.zeros(pos0.shape[0], **f64))
    for t in range(c["n_rounds"]):
        st = _scalar_round(ctx, c, betas, eps, pr.round_keys(pc.key(case), c["n_rounds"], t)[0], st, KR, tallies)
    out["control_loop"] = dict(pos=st[0].cpu().numpy(), logp=st[1].cpu().numpy(), grad=st[2].cpu().numpy(),
                               n_acc=tallies[0][:KR].cpu().numpy(), acc_sum=tallies[1][:KR].cpu().numpy())
    # the replay of the run: the two pieces in a host loop, every sweep checked exactly
    st = tuple(t.clone() for t in state0)
    replica = torch.arange(KR, **i32)
    swap_acc = torch.zeros(R, K - 1, **i32); swap_prob = torch.zeros(R, K - 1, **f64)
    tallies = (torch.zeros(pos0.shape[0], **i32), torch.zeros(pos0.shape[0], **f64))
    margins, decisions, tp, tl = [], [], [], []
    for t in range(c["n_rounds"]):
        km, ks = pr.round_keys(pc.key(case), c["n_rounds"], t)
        st = _scalar_round(ctx, c, betas, eps, km, st, KR, tallies)
        m, dec = _checked_sweep(ctx, case, betas, ks, t % 2, st, replica, swap_acc, swap_prob, K, R)
        margins.append(m); decisions.append(dec)
        tp.append(st[0][0:KR:K].cpu().numpy().copy()); tl.append(st[1][0:KR:K].cpu().numpy().copy())
    # the other parity of the last state as well: both parities of every case see a sweep
    extra = tuple(t.clone() for t in st)
    m, dec = _checked_sweep(ctx, case, betas, prng.PRNGKey(77), c["n_rounds"] % 2, extra, replica.clone(), swap_acc.clone(), swap_prob.clone(), K, R)
    margins.append(m)
    out["replay"] = dict(pos=st[0].cpu().numpy(), logp=st[1].cpu().numpy(), grad=st[2].cpu().numpy(), n_acc=tallies[0][:KR].cpu().numpy(),
                         acc_sum=tallies[1][:KR].cpu().numpy(), replica=replica.cpu().numpy(), swap_accepted=swap_acc.cpu().numpy(),
                         swap_prob=swap_prob.cpu().numpy(), traj_pos=np.stack(tp), traj_logp=np.stack(tl))
    out["margins"], out["decisions"] = margins, decisions
    ctx.close()
    return out


@pytest.mark.parametrize("case", list(pc.CASES))
def test_local_moves_have_the_bits_of_the_scalar_launches(case):
    c = pc.CASES[case]
    r = _record(case)
    a, b = r["control"], r["control_loop"]
    for name in ("pos", "logp", "grad"):
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)                # (all n_chain_local rows: the padding rows untouched by both)
    np.testing.assert_array_equal(a["n_acc"], b["n_acc"])
    np.testing.assert_array_equal(a["acc_sum"], b["acc_sum"])
    KR = c["K"] * c["R"]
    print(case, "accepted local steps", int(a["n_acc"].sum()), "of", KR * c["n_local"] * c["n_rounds"])
    assert 0 < a["n_acc"].sum() < KR * c["n_local"] * c["n_rounds"]
    assert (a["swap_accepted"] == 0).all() and (a["swap_prob"] == 0).all() and (a["replica"] == np.arange(KR)).all()
    np.testing.assert_array_equal(a["pos"][KR:], r["state0"][0][KR:])
    np.testing.assert_array_equal(a["logp"][KR:], r["state0"][1][KR:])


@pytest.mark.parametrize("case", list(pc.CASES))
def test_every_sweep_is_exactly_the_prediction(case):
    """The assertions ran inside ``_record`` (``_checked_sweep``); here: both decisions occurred and the K = 2 odd sweeps were no-ops."""
    c = pc.CASES[case]
    r = _record(case)
    dec = np.concatenate(r["decisions"])
    print(case, "smallest |u - p|", min(r["margins"]), "accepted swaps", int(dec.sum()), "of", dec.size)
    assert dec.any()
    if c["K"] == 2:
        assert all(d.size == 0 for d in r["decisions"][1::2])


@pytest.mark.parametrize("case", list(pc.CASES))
def test_run_is_bit_identical_with_the_host_loop(case):
    r = _record(case)
    a, b = r["run"], r["replay"]
    for name in ("pos", "logp", "grad", "n_acc", "acc_sum", "replica", "swap_accepted", "traj_pos", "traj_logp"):
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
    np.testing.assert_array_equal(a["swap_prob"], b["swap_prob"])
    assert (a["replica"] != np.arange(a["replica"].size)).any()


@pytest.mark.parametrize("case", list(pc.CASES))
def test_end_to_end_against_the_restatement(case):
    c = pc.CASES[case]
    KR = c["K"] * c["R"]
    r, ref = _record(case)["run"], pc.reference(case)
    np.testing.assert_array_equal(r["n_acc"], ref["n_acc"])
    np.testing.assert_array_equal(r["swap_accepted"], ref["swap_accepted"])
    np.testing.assert_array_equal(r["replica"], ref["replica"])
    dev = dict(state=(r["pos"][:KR], r["logp"][:KR], r["grad"][:KR]), acc_sum=r["acc_sum"], swap_prob=r["swap_prob"])
    got, want = pc.quantities(dev), pc.quantities(ref)
    errs = {q: float(np.max(np.abs(got[q] - want[q]) / np.maximum(1.0, np.abs(want[q])))) for q in pc.QUANTITIES}
    for q, tol in zip(pc.QUANTITIES, pc.TOLERANCE[case]):
        print(f"{case}: {q}: largest difference {errs[q]:.3g} (tolerance {tol:.3g})")
    for q, tol in zip(pc.QUANTITIES, pc.TOLERANCE[case]):
        assert errs[q] <= tol, (q, errs[q], tol)
    np.testing.assert_allclose(r["traj_logp"][-1], ref["traj_logp"][-1], rtol=0, atol=pc.TOLERANCE[case][1] * max(1.0, np.abs(ref["traj_logp"]).max()))


def test_sampling_on_the_device():
    """tests/test_pt_ref.py's configuration: slot 0's share of each mode over the last 100 rounds in [0.10, 0.40]; without exchange the
    share of mode 0 exceeds 0.99."""
    import torch
    from tests import gpu_util as gu
    s = pc.SAMPLING
    d_, betas, eps, x0, key = pc.sampling_setup()
    K, R = s["K"], s["R"]
    args, dist, *_ = gu.gmm4_setup(B=K * R)
    ctx = gu.make_ctx(dist, args)
    state0 = _init_slots(ctx, torch.as_tensor(x0).cuda(), betas, K * R)
    shares = {}
    for exchange in (True, False):
        pos, logp, grad = (t.clone() for t in state0)
        tp = torch.empty(s["n_rounds"], R, 2, device="cuda")
        sw = torch.empty(R, K - 1, dtype=torch.int32, device="cuda")
        ctx.pt_run(key, betas, eps, R, s["n_local"], s["n_rounds"], pos, logp, grad, kernel="hmc", num_steps=s["L"], exchange=exchange, thin=1,
                   swap_accepted=sw, traj_pos=tp)
        shares[exchange] = pc.mode_shares(tp[-s["last"]:].cpu().numpy(), d_.modes)
        print("exchange", exchange, "shares", shares[exchange], "swap rates", (sw.sum(0).double() / (R * s["n_rounds"] / 2)).cpu().numpy().round(2))
    ctx.close()
    assert ((shares[True] >= 0.10) & (shares[True] <= 0.40)).all(), shares[True]
    assert shares[False][0] > 0.99


def test_refusals_name_the_argument_and_touch_nothing():
    import torch
    from mfm_amd import _lib
    from tests import gpu_util as gu
    case = "padded"
    c = pc.CASES[case]
    ctx, pos0 = _ctx(case)
    betas, eps = pc.betas(case), pc.step_sizes(case)
    pos, logp, grad = _init_slots(ctx, pos0, betas, 9)
    B = pos.shape[0]
    key = prng.PRNGKey(1)
    tp = torch.full((4, 8, 64), -1.0, device="cuda")
    before = [t.clone() for t in (pos, logp, grad, tp)]

    def refused(match, betas_=betas, eps_=eps, R=3, n_local=2, n_rounds=4, **kw):
        with pytest.raises(_lib.MfmError, match=match):
            ctx.pt_run(key, betas_, eps_, R, n_local, n_rounds, pos, logp, grad, **dict(dict(thin=1, traj_pos=tp), **kw))

    refused("kernel", kernel=2)
    refused("num_steps", num_steps=0)
    refused("n_temps", betas_=[1.0], eps_=[0.1])
    refused("n_temps", betas_=np.ones(65), eps_=np.ones(65))
    refused("n_ladders", R=0)
    refused("n_chain_local", R=6)
    refused(r"betas\[1\]", betas_=[1.0, 0.0, 0.5])
    refused(r"betas\[2\]", betas_=[1.0, 0.5, np.inf])
    refused(r"step_sizes\[0\]", eps_=[-1.0, 0.1, 0.1])
    refused("n_local", n_local=0)
    refused("n_rounds", n_rounds=0)
    refused("exchange", exchange=2)
    refused("thin .* n_steps", thin=3)
    refused("d_traj_pos", traj_pos=None)
    with pytest.raises(_lib.MfmError, match="null device pointer"):
        ctx.pt_run(key, betas, eps, 3, 2, 4, None, logp, grad)
    with pytest.raises(_lib.MfmError, match="parity"):
        ctx.pt_exchange(key, betas, 3, 2, pos, logp, grad)
    with pytest.raises(_lib.MfmError, match="n_chain_local"):
        ctx.pt_exchange(key, betas, 6, 0, pos, logp, grad)
    ctx.set_inverse_mass(np.full(64, 2.0))
    refused("unit mass")
    with pytest.raises(_lib.MfmError, match="unit mass"):
        ctx.pt_exchange(key, betas, 3, 0, pos, logp, grad)
    ctx.set_inverse_mass(None)
    ctx.sync()
    for t, b in zip((pos, logp, grad, tp), before):
        assert torch.equal(t, b)                                               # a rejected call touches nothing
    ctx.close()
    args, dist, *_ = gu.phi4_setup(d=64, B=16, hidden=32, F=16)
    shard = gu.make_ctx(dist, args, n_local=16, n_total=32, offset=16)
    with pytest.raises(_lib.MfmError, match="n_chain_total"):
        shard.pt_run(key, betas, eps, 3, 2, 4, pos, logp, grad)
    shard.close()
    aargs, adist, *_ = gu.lgcp_setup(n=4, B=16)
    cox = gu.make_ctx(adist, aargs)
    cpos = torch.as_tensor(adist.init_params.astype(np.float32)).cuda()
    clogp = torch.empty(16, dtype=torch.float64, device="cuda"); cgrad = torch.empty_like(cpos)
    cox.mala_init(cpos, 1.0, clogp, cgrad)
    with pytest.raises(_lib.MfmError, match="phi-four and mixture targets"):
        cox.pt_run(key, betas, eps, 3, 2, 4, cpos, clogp, cgrad)
    cox.close()


def test_python_step_equals_step_run_and_the_context_call():
    import torch
    from mfm_amd import distributions as D, random as jr
    from mfm_amd.bblackjax.mcmc.parallel_tempering import PTInfo, PTState, parallel_tempering
    from mfm_amd.engine import Engine
    from tests import gpu_util as gu
    B, K = 16, 4
    args, odist, k, model, state = gu.gmm4_setup(B=B)
    dist = D.GaussianMixture(odist.modes, odist.covs, odist.weights)
    args.ot_cond_flow = False
    eng = Engine(dist, args, model.f)
    try:
        betas = pc.betas("gmm4")
        pos0 = torch.as_tensor(pc.start_state("gmm4")).cuda()
        algo = parallel_tempering(dist.logprior, dist.loglik, betas, mcmc="hmc", step_size=0.6, num_integration_steps=3, num_mcmc_steps=2)
        st0 = algo.init(pos0)
        assert isinstance(st0, PTState) and st0.replica.tolist() == list(range(B))
        want = _init_slots(eng.ctx, pos0, betas, B)
        for a, b in zip(st0[:3], want):
            assert torch.equal(a, b)                                           # every slot initialised at its own beta
        key = jr.PRNGKey(6)
        one, info1 = algo.step(key, st0)
        run1, _ = algo.step.run(key, st0, 1)
        for a, b in zip(one, run1):
            assert torch.equal(a, b)
        assert (st0.position == pos0).all()                                    # functional: the input state is not modified
        new, info = algo.step.run(key, st0, 6, thin=2)
        assert isinstance(info, PTInfo) and info.swap_acceptance_rate.shape == (K - 1,) and info.swap_accepted.shape == (B // K, K - 1)
        assert info.acceptance_rate.shape == (B,) and info.positions.shape == (3, B // K, 2) and info.logdensities.shape == (3, B // K)
        assert info1.positions is None and info1.logdensities is None
        pos, logp, grad = (t.clone() for t in st0[:3])
        rep = torch.arange(B, dtype=torch.int32, device="cuda")
        sw = torch.empty(B // K, K - 1, dtype=torch.int32, device="cuda")
        eng.ctx.pt_run(key, betas, 0.6 / np.sqrt(betas), B // K, 2, 6, pos, logp, grad, kernel="hmc", num_steps=3, replica=rep, swap_accepted=sw)
        for a, b in zip(new, (pos, logp, grad, rep)):
            assert torch.equal(a, b)
        assert torch.equal(info.swap_accepted, sw)
        np.testing.assert_allclose(info.swap_acceptance_rate.cpu().numpy(), sw.sum(0).cpu().numpy() / (4 * 3.0))
        none, ninfo = parallel_tempering(dist.logprior, dist.loglik, betas, step_size=0.6, num_integration_steps=3, num_mcmc_steps=2,
                                         exchange="none").step.run(key, st0, 6)
        assert ninfo.swap_accepted.sum().item() == 0 and none.replica.tolist() == list(range(B))
    finally:
        eng.close()


def test_do_pt_end_to_end_on_the_four_mode_example(caplog):
    import logging
    from mfm_amd import exe_others as X, multi_modal as M
    from mfm_amd.distributions import GaussianMixture
    args = M.build_parser().parse_args(["--example", "4-mode", "--num_chain", "64", "--learning_iter", "40", "--eval_iter", "8", "--seed", "1",
                                        "--do_pt", "--mcmc_kernel", "hmc", "--hmc_steps", "4"])
    args.dim, args.lim, args.levels, args.step_size = 2, [-16, 16], 20, 0.2                  # multi_modal.main: the 4-mode example
    dist = GaussianMixture(8. * np.array([[1, 1], [1, -1], [-1, 1], [-1, -1]]), np.ones((4, 2)), np.ones(4) / 4)
    with caplog.at_level(logging.INFO, logger="mfm_amd.exe_others"):
        res, res_, extras = X.run(dist, args, dist.sample_model, return_extras=True)
    try:
        print("do_pt: res", res, "swap rates", extras["swap_rates"], "stats", extras["stats"])
        assert res.shape == (5,) and np.isfinite(res).all() and np.array_equal(res, res_)
        assert extras["samples"].shape == (8 * 8, 2) and extras["swap_rates"].shape == (7,)
        assert np.isfinite(extras["swap_rates"]).all() and (extras["swap_rates"] > 0).all()
        assert np.isfinite(extras["stats"]["rhat_max"]) and extras["stats"]["pt_barrier"] >= 0
        assert any("Swap acceptance rate per pair" in m for m in caplog.messages) and any("Communication barrier" in m for m in caplog.messages)
    finally:
        extras["engine"].close()
