"""GPU tests of ``mfm_chees_warmup`` and ``mfm_hmc_run_lengths`` (mfm_amd/csrc/chees.hip) and of the Python layers on them.

Every case of tests/chees_cases.py runs ONCE (16 or 32 chains, 5 to 12 iterations), followed by its replay with single-step launches;
the tests share that record and leave it unchanged.  The cases reach every (MAXIT, BCRT, MASS) instance of ``chees_step_kernel``
(tests/row_matrix.py), up to d = 2048:

* replay: from the recorded ``(eps_t, L_t)``, ``n_iter`` launches of ``mfm_hmc_step`` / ``mfm_hmc_step_keys`` on the run's step keys
  give the final state bit for bit;
* statistic: from the replay's ``x`` before the last step and the device's ``x'``, ``v'``, ``alpha`` of the last iteration, a float64
  recomputation gives that iteration's ``hm`` and ``ghat`` within a bound propagated from float64 reassociation alone (the inputs are
  exact): every sum of n terms is taken to be off by at most n 2^-52 sum |term|, through the means, the centred norms, the products
  and the pooled quotient;
* recursion: from the recorded ``hm_t`` and ``ghat_t`` the restatement's update lines alone reproduce ``eps_{t+1}``, ``T_{t+1}`` to
  1e-12 relative (a few ulp of exp, log, sqrt), ``L_{t+1}`` exactly, and the four results;
* end to end: the traces agree with tests/chees_ref.py on the same keys within the case's tolerance (tests/chees_cases.py).

The MAXIT 32 instances (d = 1025 and d = 2048, unit and non-unit mass) are also replayed from the start states of
tests/row_instance_cases.py.  Then ``mfm_hmc_run_lengths`` against single steps and against ``mfm_hmc_run`` on the same grid of instances
(``RUN_LENGTHS``), the refusals, and the Python API and CLI."""
import functools

import numpy as np
import pytest

from oracle import prng
from tests import chees_cases as cc, chees_ref as cr

pytestmark = pytest.mark.gpu

U = 2.0 ** -52


def _ctx(case):
    """A context on the case's target with its mass installed, and the start state on the device."""
    import torch
    from mfm_amd import _lib
    from tests import gpu_util as gu
    c = cc.CASES[case]
    if c["target"] == "gmm4":
        args, dist, *_ = gu.gmm4_setup(B=c["B"])
    else:
        args, dist, *_ = gu.phi4_setup(d=c["d"], B=c["B"], hidden=32, F=16)
    ctx = gu.make_ctx(dist, args)
    if cc.block(case) is not None:
        ctx.set_target(_lib.PHI4, cc.block(case))
    ctx.set_inverse_mass(cc.inverse_mass(case))
    return ctx, torch.as_tensor(cc.start_state(case)).cuda()


def _init(ctx, pos0, beta=1.0):
    import torch
    pos = pos0.clone()
    logp = torch.empty(pos.shape[0], dtype=torch.float64, device="cuda"); grad = torch.empty_like(pos)
    ctx.mala_init(pos, beta, logp, grad)
    return pos, logp, grad


def _keys_dev(keys):
    import torch
    return torch.as_tensor(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32)).cuda()


def _single_step(ctx, key, per_chain, n_steps, j, beta, eps, L, pos, logp, grad):
    """The launch of step j of a run of n_steps steps on ``key``: mfm_hmc_step_keys (chain-major) or mfm_hmc_step (step-major)."""
    if per_chain:
        ctx.hmc_step_keys(_keys_dev(prng.split_rows(key, n_steps)[:, j]), beta, eps, L, pos, logp, grad)
    else:
        ctx.hmc_step(prng.split(key, n_steps)[j], beta, eps, L, pos, logp, grad)


@functools.lru_cache(maxsize=None)
def _record(case):
    """The device's run of the case and its replay, as numpy arrays."""
    import torch
    c = cc.CASES[case]
    B, d, n = c["B"], c["d"], c["n_iter"]
    ctx, pos0 = _ctx(case)
    state0 = _init(ctx, pos0)
    pos, logp, grad = (t.clone() for t in state0)
    trace = torch.zeros(n, 7, dtype=torch.float64, device="cuda")
    prop = torch.zeros(B, d, device="cuda"); vel = torch.zeros(B, d, dtype=torch.float64, device="cuda")
    alpha = torch.zeros(B, dtype=torch.float64, device="cuda")
    key = cc.key(case)
    results = ctx.chees_warmup(_keys_dev(key) if c["key_mode"] else key, 1.0, c["eps"], n, pos, logp, grad, traj0=c["T"], n_valid=c["n_valid"],
                               target_accept=cc.TARGET_ACCEPT, learning_rate=c["lr"], max_leapfrog=c["max_leapfrog"], decay=cc.DECAY,
                               divergence_threshold=cc.DIVERGENCE_THRESHOLD, trace=trace, prop=prop, vel=vel, alpha=alpha)
    out = dict(results=results, trace=trace.cpu().numpy(), prop=prop.cpu().numpy(), vel=vel.cpu().numpy(), alpha=alpha.cpu().numpy(),
               pos=pos.cpu().numpy(), logp=logp.cpu().numpy(), grad=grad.cpu().numpy())
    rp, rl, rg = (t.clone() for t in state0)
    for j in range(n):
        if j == n - 1:
            out["x_last"] = rp.cpu().numpy().copy()
        _single_step(ctx, key, bool(c["key_mode"]), n, j, 1.0, float(out["trace"][j, 0]), int(out["trace"][j, 2]), rp, rl, rg)
    out.update(replay_pos=rp.cpu().numpy(), replay_logp=rl.cpu().numpy(), replay_grad=rg.cpu().numpy())
    ctx.close()
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@pytest.mark.parametrize("case", list(cc.CASES))
def test_replay_with_single_step_launches_is_bit_identical(case):
    r = _record(case)
    print(case, "L", r["trace"][:, 2].astype(int).tolist(), "eps", r["trace"][:, 0].tolist())
    for name in ("pos", "logp", "grad"):
        np.testing.assert_array_equal(r[name], r["replay_" + name], err_msg=name)
    assert np.abs(r["pos"] - cc.start_state(case)).max() > 0                # the chains moved


@pytest.mark.parametrize("mass", [False, True])
@pytest.mark.parametrize("case", ["d1025_d0", "d2048_pbc"])
def test_replay_on_the_maxit_32_instances(case, mass):
    """The largest instances (1024 < d <= 2048; BCRT false and true, unit and non-unit mass) from the start states and step sizes of
    tests/row_instance_cases.py: five iterations, replayed by single-step launches bit for bit."""
    import torch
    from mfm_amd import _lib
    from tests import gpu_util as gu, row_instance_cases as rc
    d = rc.CASES[case][0]
    args, dist0, *_ = gu.phi4_setup(d=d, B=rc.N_CHAINS, hidden=32, F=16)
    ctx = gu.make_ctx(dist0, args)
    if rc.block(case) is not None:
        ctx.set_target(_lib.PHI4, rc.block(case))
    ctx.set_inverse_mass(np.exp(np.linspace(np.log(0.5), np.log(2.0), d)) if mass else None)
    state0 = _init(ctx, torch.as_tensor(rc.start_state(case)).cuda())
    pos, logp, grad = (t.clone() for t in state0)
    eps, n, key = 0.5 * rc.STEP_SIZES[case]["hmc"]["b1"], 5, prng.PRNGKey(5)
    trace = torch.zeros(n, 7, dtype=torch.float64, device="cuda")
    ctx.chees_warmup(key, 1.0, eps, n, pos, logp, grad, traj0=6 * eps, trace=trace)
    tr = trace.cpu().numpy()
    rp, rl, rg = (t.clone() for t in state0)
    for j in range(n):
        _single_step(ctx, key, False, n, j, 1.0, float(tr[j, 0]), int(tr[j, 2]), rp, rl, rg)
    print(case, "L", tr[:, 2].astype(int).tolist(), "hm", np.round(tr[:, 3], 3).tolist())
    assert tr[0, 2] == 3 and len(set(tr[:, 2])) >= 3 and (pos != state0[0]).any()
    for a, b in ((pos, rp), (logp, rl), (grad, rg)):
        assert torch.equal(a, b)
    ctx.close()


def _sum_bound(terms, axis=None):
    """What reassociating a float64 sum of these terms can change: n 2^-52 sum |term|."""
    n = terms.size if axis is None else terms.shape[axis]
    return n * U * np.abs(terms).sum(axis)


def _statistic_with_bound(x, prop, vel, alpha, div, tau):
    """``(ghat, hm)`` as tests/chees_ref.py computes them, each with the propagated reassociation bound (module docstring)."""
    x, prop = x.astype(np.float64), prop.astype(np.float64)
    n = x.shape[0]
    ok = ~div
    m0, m1 = x.mean(0), prop.mean(0)
    e_m0, e_m1 = _sum_bound(x, 0) / n + U * np.abs(m0), _sum_bound(prop, 0) / n + U * np.abs(m1)
    dx0, dx1 = x - m0, prop - m1
    e_dx0, e_dx1 = e_m0 + U * np.abs(dx0), e_m1 + U * np.abs(dx1)
    a, b, c = (dx1 * dx1).sum(1), (dx0 * dx0).sum(1), (dx1 * vel).sum(1)
    e_a = (2 * np.abs(dx1) * e_dx1 + e_dx1 ** 2).sum(1) + _sum_bound(dx1 * dx1, 1) + U * a
    e_b = (2 * np.abs(dx0) * e_dx0 + e_dx0 ** 2).sum(1) + _sum_bound(dx0 * dx0, 1) + U * b
    e_c = (np.abs(vel) * e_dx1).sum(1) + _sum_bound(dx1 * vel, 1) + 2 * U * np.abs(dx1 * vel).sum(1)
    g = tau * (a - b) * c
    e_g = tau * (np.abs(a - b) * e_c + np.abs(c) * (e_a + e_b) + (e_a + e_b) * e_c) + 4 * U * np.abs(g)
    al, gk, e_gk = alpha[ok], g[ok], e_g[ok]
    num, den = (al * gk).sum(), (al + 1e-20).sum()
    e_num = (al * e_gk).sum() + _sum_bound(al * gk) + 2 * U * np.abs(al * gk).sum()
    e_den = _sum_bound(al + 1e-20) + U * den
    ghat = num / den
    e_ghat = (e_num + abs(ghat) * e_den) / (den - e_den) + 2 * U * abs(ghat)
    inv = (1.0 / al).sum()
    hm = ok.sum() / inv
    e_hm = hm * (_sum_bound(1.0 / al) + 2 * U * inv) / inv + 2 * U * hm
    return ghat, e_ghat, hm, e_hm


@pytest.mark.parametrize("case", list(cc.CASES))
def test_statistic_of_the_last_iteration(case):
    c = cc.CASES[case]
    r, ref = _record(case), cc.reference(case)
    nv, t = c["n_valid"], c["n_iter"]
    row = r["trace"][-1]
    div = ref["records"][-1].div[:nv]           # the device keeps no flag array: the restatement's, which the counts confirm
    assert int(row[5]) == int(div.sum())
    assert np.isfinite(r["prop"][:nv]).all() and not div.all()
    tau = cr.radical_inverse(t) * row[1]
    ghat, e_ghat, hm, e_hm = _statistic_with_bound(r["x_last"][:nv], r["prop"][:nv], r["vel"][:nv], r["alpha"][:nv], div, tau)
    print(f"{case}: hm {row[3]!r} recomputed {hm!r} (bound {e_hm:.3g}); ghat {row[4]!r} recomputed {ghat!r} (bound {e_ghat:.3g})")
    assert abs(row[3] - hm) <= e_hm
    assert abs(row[4] - ghat) <= e_ghat
    # and through the restatement's own lines
    g2, h2, nd2, ma2 = cr.statistic(r["x_last"], r["prop"], r["vel"], r["alpha"], np.concatenate([div, np.zeros(c["B"] - nv, bool)]), tau, nv)
    assert abs(g2 - ghat) <= e_ghat and abs(h2 - hm) <= e_hm
    np.testing.assert_allclose(row[6], ma2, rtol=nv * U)


@pytest.mark.parametrize("case", list(cc.CASES))
def test_recursion_from_the_recorded_statistics(case):
    c = cc.CASES[case]
    r = _record(case)
    rs = cr.Recursion(c["eps"], c["T"], c["lr"], c["max_leapfrog"], cc.DECAY, cc.TARGET_ACCEPT)
    for t, row in enumerate(r["trace"]):
        np.testing.assert_allclose(row[0], rs.eps, rtol=1e-12, err_msg=f"eps_{t + 1}")
        np.testing.assert_allclose(row[1], rs.T, rtol=1e-12, err_msg=f"T_{t + 1}")
        assert int(row[2]) == rs.L, (t + 1, row[2], rs.L)
        rs.advance(row[3], row[4])
    np.testing.assert_allclose(r["results"], rs.results, rtol=1e-12)
    assert r["trace"][0, 0] == c["eps"] and r["trace"][0, 1] == c["T"]      # eps_1 and T_1 are the caller's values themselves


@pytest.mark.parametrize("case", list(cc.CASES))
def test_traces_match_the_restatement(case):
    """Measured on MI355X, largest difference / tolerance over the seven trace columns: phi4_d65_mass 0.20, phi4_d65_pbc 0.13, phi4_d320
    0.25, phi4_d320_pbc 0.37, phi4_d1025 0.29, phi4_d2048_pbc_mass 0.27, phi4_d64_mass 0.41, phi4_d64_pbc_mass 0.13, phi4_d100_pbc_mass
    0.59, phi4_d320_pbc_mass 0.41, phi4_d1025_mass 0.26, phi4_d1100_pbc 0.44 (the first seven cases: 0.22 to 0.91)."""
    r, ref = _record(case), cc.reference(case)
    dev, want = r["trace"], ref["trace"]
    with np.errstate(invalid="ignore"):
        err = np.abs(dev - want) / np.maximum(1.0, np.abs(want))
    for j, name in enumerate(cr.TRACE_FIELDS):
        print(f"{case}: {name}: largest difference {np.nanmax(err[:, j]):.3g} (tolerance {cc.TOLERANCE[case][j]:.3g})")
    np.testing.assert_array_equal(np.isnan(dev), np.isnan(want))
    np.testing.assert_array_equal(dev[:, 2], want[:, 2])
    np.testing.assert_array_equal(dev[:, 5], want[:, 5])
    for j, name in enumerate(cr.TRACE_FIELDS):
        assert not (err[:, j] > cc.TOLERANCE[case][j]).any(), (name, np.nanmax(err[:, j]), cc.TOLERANCE[case][j])


# ---- mfm_hmc_run_lengths ------------------------------------------------------------------------------------------------------------
LENGTHS = [3, 1, 3, 2]              # three lengths, 1 among them, one repeated


def _run_lengths(ctx, state0, key, eps, lengths, thin):
    import torch
    pos, logp, grad = (t.clone() for t in state0)
    n, d = pos.shape
    ns = len(lengths)
    acc = torch.empty(n, device="cuda"); isacc = torch.empty(n, dtype=torch.uint8, device="cuda")
    n_acc = torch.empty(n, dtype=torch.int32, device="cuda"); acc_sum = torch.empty(n, dtype=torch.float64, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    tp = torch.empty(ns // thin, n, d, device="cuda") if thin else None
    tl = torch.empty(ns // thin, n, dtype=torch.float64, device="cuda") if thin else None
    ctx.hmc_run_lengths(_keys_dev(key) if np.ndim(key) == 2 else key, 1.0, eps, torch.as_tensor(lengths, dtype=torch.int32).cuda(), pos, logp, grad,
                        thin=thin, n_acc=n_acc, acc_sum=acc_sum, acc=acc, is_acc=isacc, traj_pos=tp, traj_logp=tl, total_leapfrog=total)
    names = ("pos", "logp", "grad", "acc", "isacc", "n_acc", "acc_sum", "total", "traj_pos", "traj_logp")
    return {k: (None if t is None else t.cpu().numpy()) for k, t in zip(names, (pos, logp, grad, acc, isacc, n_acc, acc_sum, total, tp, tl))}


# case of tests/chees_cases.py: (chain-major keys, step size) -- the mixture and every (MAXIT, BCRT) instance of the run kernel at unit
# mass and under the case's mass (tests/row_matrix.py has the grid).  Step sizes at which the restatement's four steps hold accepted and
# rejected trajectories; accepted of 16 chains per step in the comment
RUN_LENGTHS = {
    "phi4_d64": (False, 0.03),              # 3 / 10 / 6 / 5
    "phi4_d65": (True, 0.03),               # 4 / 9 / 7 / 7
    "gmm4": (True, 1.4),                    # 12 / 12 / 10 / 16
    "phi4_d320_mass": (False, 0.006),       # 6 / 11 / 8 / 8
    "phi4_d320": (True, 0.007),             # 4 / 13 / 6 / 6
    "phi4_d1025": (False, 0.002),           # 9 / 15 / 12 / 14
    "phi4_d64_pbc": (False, 0.025),         # 6 / 12 / 6 / 8
    "phi4_d65_pbc": (True, 0.03),           # 4 / 9 / 7 / 7
    "phi4_d320_pbc": (True, 0.006),         # 6 / 15 / 10 / 13
    "phi4_d1100_pbc": (False, 0.0022),      # 7 / 14 / 7 / 11
    "phi4_d64_mass": (True, 0.025),         # 5 / 12 / 8 / 8
    "phi4_d65_mass": (False, 0.025),        # 5 / 12 / 7 / 7
    "phi4_d1025_mass": (True, 0.002),       # 7 / 15 / 13 / 13
    "phi4_d64_pbc_mass": (False, 0.025),    # 5 / 12 / 7 / 7
    "phi4_d100_pbc_mass": (True, 0.016),    # 6 / 13 / 9 / 12
    "phi4_d320_pbc_mass": (False, 0.006),   # 6 / 11 / 8 / 8
    "phi4_d2048_pbc_mass": (True, 0.001),   # 12 / 15 / 15 / 15
}


@pytest.mark.parametrize("case,per_chain", [(c, v[0]) for c, v in RUN_LENGTHS.items()])
def test_run_lengths_is_bit_identical_with_single_steps(case, per_chain):
    import torch
    c = cc.CASES[case]
    B = c["B"]
    eps = RUN_LENGTHS[case][1]
    ctx, pos0 = _ctx(case)
    state0 = _init(ctx, pos0)
    key = prng.split(prng.PRNGKey(33), B) if per_chain else prng.PRNGKey(21)
    pos, logp, grad = (t.clone() for t in state0)
    steps = dict(pos=[], logp=[], moved=[])
    for j, L in enumerate(LENGTHS):
        before = pos.clone()
        _single_step(ctx, key, per_chain, len(LENGTHS), j, 1.0, eps, L, pos, logp, grad)
        steps["pos"].append(pos.cpu().numpy().copy()); steps["logp"].append(logp.cpu().numpy().copy())
        steps["moved"].append(((pos != before).any(1)).cpu().numpy())
    run = _run_lengths(ctx, state0, key, eps, LENGTHS, 1)
    moved = np.stack(steps["moved"])
    print(f"{case}: accepted {moved.sum()} of {moved.size}")
    assert 0 < moved.sum() < moved.size
    np.testing.assert_array_equal(run["pos"], pos.cpu().numpy())
    np.testing.assert_array_equal(run["logp"], logp.cpu().numpy())
    np.testing.assert_array_equal(run["grad"], grad.cpu().numpy())
    np.testing.assert_array_equal(run["traj_pos"], np.stack(steps["pos"]))
    np.testing.assert_array_equal(run["traj_logp"], np.stack(steps["logp"]))
    np.testing.assert_array_equal(run["n_acc"], moved.sum(0))
    assert run["total"].item() == sum(LENGTHS)
    thinned = _run_lengths(ctx, state0, key, eps, LENGTHS, 2)
    np.testing.assert_array_equal(thinned["traj_pos"], run["traj_pos"][[1, 3]])
    np.testing.assert_array_equal(thinned["traj_logp"], run["traj_logp"][[1, 3]])
    none = _run_lengths(ctx, state0, key, eps, LENGTHS, 0)
    for other in (thinned, none):
        for name in ("pos", "logp", "grad", "n_acc", "acc_sum", "acc", "isacc", "total"):
            np.testing.assert_array_equal(other[name], run[name], err_msg=name)
    # all lengths equal: mfm_hmc_run
    same = _run_lengths(ctx, state0, key, eps, [3] * 4, 1)
    p2, l2, g2 = (t.clone() for t in state0)
    n_acc = torch.empty(B, dtype=torch.int32, device="cuda"); acc_sum = torch.empty(B, dtype=torch.float64, device="cuda")
    acc = torch.empty(B, device="cuda"); isacc = torch.empty(B, dtype=torch.uint8, device="cuda")
    tp = torch.empty(4, B, c["d"], device="cuda")
    ctx.hmc_run(_keys_dev(key) if per_chain else key, 1.0, eps, 3, 4, p2, l2, g2, thin=1, n_acc=n_acc, acc_sum=acc_sum, acc=acc, is_acc=isacc, traj_pos=tp)
    for name, t in (("pos", p2), ("logp", l2), ("grad", g2), ("n_acc", n_acc), ("acc_sum", acc_sum), ("acc", acc), ("isacc", isacc), ("traj_pos", tp)):
        np.testing.assert_array_equal(same[name], t.cpu().numpy(), err_msg=name)
    assert same["total"].item() == 12
    ctx.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_touch_nothing():
    import torch
    from mfm_amd import _lib
    from tests import gpu_util as gu
    ctx, pos0 = _ctx("phi4_d64")
    pos, logp, grad = _init(ctx, pos0)
    B = pos.shape[0]
    key = prng.PRNGKey(1)
    trace = torch.full((4, 7), -1.0, dtype=torch.float64, device="cuda")
    before = [t.clone() for t in (pos, logp, grad, trace)]
    ok = dict(traj0=0.1, n_valid=B, trace=trace)

    def refused(match, key_=key, eps=0.01, n_iter=4, **kw):
        with pytest.raises(_lib.MfmError, match=match):
            ctx.chees_warmup(key_, 1.0, eps, n_iter, pos, logp, grad, **dict(ok, **kw))

    refused("step_size", eps=0.0)
    refused("key_mode", key_mode=2)
    refused("d_keys", key_mode=1)
    refused("n_steps", n_iter=0)
    refused("n_valid", n_valid=1)
    refused("n_valid", n_valid=B + 1)
    refused("trajectory_length", traj0=0.0)
    refused("learning_rate", learning_rate=0.0)
    refused("decay", decay=1.0)
    refused("decay", decay=-0.1)
    refused("max_leapfrog", max_leapfrog=0)
    refused("max_leapfrog", max_leapfrog=100001)
    refused("target_accept", target_accept=1.0)
    refused("divergence_threshold", divergence_threshold=0.0)
    with pytest.raises(_lib.MfmError, match="null device pointer"):
        ctx.chees_warmup(key, 1.0, 0.01, 4, None, logp, grad, **ok)
    lengths = torch.ones(4, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.MfmError, match="d_num_steps"):
        ctx.hmc_run_lengths(key, 1.0, 0.01, None, pos, logp, grad)
    with pytest.raises(_lib.MfmError, match="step_size"):
        ctx.hmc_run_lengths(key, 1.0, 0.0, lengths, pos, logp, grad)
    with pytest.raises(_lib.MfmError, match="thin .* n_steps"):
        ctx.hmc_run_lengths(key, 1.0, 0.01, lengths, pos, logp, grad, thin=3, traj_pos=torch.empty(4, B, 64, device="cuda"))
    with pytest.raises(_lib.MfmError, match="d_traj_pos"):
        ctx.hmc_run_lengths(key, 1.0, 0.01, lengths, pos, logp, grad, thin=2)
    with pytest.raises(_lib.MfmError, match="d_keys"):
        ctx.hmc_run_lengths(key, 1.0, 0.01, lengths, pos, logp, grad, key_mode=1)
    ctx.sync()
    for t, b in zip((pos, logp, grad, trace), before):
        assert torch.equal(t, b)                                               # a rejected call touches nothing
    ctx.close()
    # more than one rank: the means would need an all-reduce
    args, dist, *_ = gu.phi4_setup(d=64, B=16, hidden=32, F=16)
    shard = gu.make_ctx(dist, args, n_local=16, n_total=32, offset=16)
    spos, slogp, sgrad = _init(shard, pos0)
    with pytest.raises(_lib.MfmError, match="n_chain_total"):
        shard.chees_warmup(key, 1.0, 0.01, 4, spos, slogp, sgrad)
    shard.hmc_run_lengths(key, 1.0, 0.01, lengths, spos, slogp, sgrad)        # (the run itself serves a shard, as mfm_hmc_run)
    shard.close()
    aargs, adist, *_ = gu.lgcp_setup(n=4, B=16)
    cox = gu.make_ctx(adist, aargs)
    cpos, clogp, cgrad = _init(cox, torch.as_tensor(adist.init_params.astype(np.float32)).cuda())
    with pytest.raises(_lib.MfmError, match="the HMC step serves the phi-four and mixture targets"):
        cox.chees_warmup(key, 1.0, 0.01, 4, cpos, clogp, cgrad)
    with pytest.raises(_lib.MfmError, match="the HMC step serves the phi-four and mixture targets"):
        cox.hmc_run_lengths(key, 1.0, 0.01, lengths, cpos, clogp, cgrad)
    cox.close()


# ---- Python -------------------------------------------------------------------------------------------------------------------------
def test_python_api_equals_the_context_calls():
    import torch
    from mfm_amd import distributions as D, random as jr
    from mfm_amd.bblackjax.adaptation.chees_adaptation import CheesAdaptationInfo, chees_adaptation, integration_steps
    from mfm_amd.bblackjax.mcmc.hmc import HMCRunInfo, hmc
    from mfm_amd.bblackjax.optimizers import adam
    from mfm_amd.engine import Engine
    from tests import gpu_util as gu
    B, n = 16, 8
    args, odist, k, model, state = gu.gmm4_setup(B=B)
    dist = D.GaussianMixture(odist.modes, odist.covs, odist.weights)
    args.ot_cond_flow = False
    eng = Engine(dist, args, model.f)
    pos0 = torch.as_tensor(cc.start_state("gmm4")).cuda()
    algo = hmc(dist.logprob, 0.5, 1)
    state = algo.init(pos0)
    key = jr.PRNGKey(6)
    (last, params), info = chees_adaptation(dist.logprob, B).run(key, state, 0.5, adam(0.05), n, trajectory_length=1.5)
    assert isinstance(info, CheesAdaptationInfo) and info.step_size.shape == (n,)
    assert (state.position == pos0).all()                                      # functional: the input state is not modified
    pos, logp, grad = (t.clone() for t in state)
    trace = torch.zeros(n, 7, dtype=torch.float64, device="cuda")
    res = eng.ctx.chees_warmup(key, 1.0, 0.5, n, pos, logp, grad, traj0=1.5, n_valid=B, learning_rate=0.05, trace=trace)
    assert (params["step_size"], params["trajectory_length"]) == res[:2]
    np.testing.assert_array_equal(torch.stack(list(info), 1).numpy(), trace.cpu().numpy())
    for a, b in zip(last, (pos, logp, grad)):
        assert torch.equal(a, b)
    np.testing.assert_array_equal(params["inverse_mass_matrix"], np.ones(2))
    fn = params["integration_steps_fn"]
    assert [fn(i) for i in range(6)] == [integration_steps(i, res[0], res[1], 1000) for i in range(6)]
    assert fn(0) == max(1, int(np.ceil(0.5 * res[1] / res[0])))
    # the sampler: step.run with one leapfrog count per step
    lengths = [fn(i) for i in range(6)]
    sampler = hmc(dist.logprob, params["step_size"], 1, params["inverse_mass_matrix"])
    new, rinfo = sampler.step.run(key, last, 6, thin=1, num_integration_steps_per_step=fn)
    new2, rinfo2 = sampler.step.run(key, last, 6, thin=1, num_integration_steps_per_step=lengths)
    assert isinstance(rinfo, HMCRunInfo) and rinfo.num_leapfrog == sum(lengths) == rinfo2.num_leapfrog
    p2, l2, g2 = (t.clone() for t in last)
    tp = torch.empty(6, B, 2, device="cuda")
    eng.ctx.set_inverse_mass(np.ones(2))
    eng.ctx.hmc_run_lengths(key, 1.0, params["step_size"], torch.as_tensor(lengths, dtype=torch.int32).cuda(), p2, l2, g2, thin=1, traj_pos=tp)
    eng.ctx.set_inverse_mass(None)
    for got in (new, new2):
        assert torch.equal(got.position, p2) and torch.equal(got.logdensity, l2)
    assert torch.equal(rinfo.positions, tp)
    assert sampler.step.run(key, last, 6)[1].num_leapfrog is None             # absent: nothing changes
    with pytest.raises(ValueError, match="num_integration_steps_per_step"):
        sampler.step.run(key, last, 6, num_integration_steps_per_step=[1, 2])
    eng.close()


def test_training_run_with_hmc_adapt_chees():
    from mfm_amd import distributions as D, exe_flow_matching as E
    from mfm_amd.bblackjax.adaptation.chees_adaptation import integration_steps
    from oracle import loop
    kw = dict(example="phi-four", dim=64, num_chain=32, learning_iter=5, mcmc_per_flow_steps=4.0, hutchs=True, fourier_dim=16, seed=7, eval_iter=1,
              step_size=0.02, hidden_x=[32, 32], hidden_t=[32, 32], hidden_xt=[32, 32], ess_steps=16)
    args = loop.default_args(mcmc_kernel="hmc", hmc_adapt="chees", adapt_steps=8, adapt_target=0.651, **kw)
    _, _, ex = E.run(D.PhiFour(64), args, None, log_every=1000, return_extras=True)
    for name in ("adapted_step_size", "adapted_trajectory_length", "adapt_acceptance", "adapt_mean_leapfrog"):
        assert isinstance(ex[name], float) and np.isfinite(ex[name]) and ex[name] > 0, name
    assert args.step_size == ex["adapted_step_size"] and args.hmc_trajectory_length == ex["adapted_trajectory_length"]
    mean_l = np.mean([integration_steps(i, args.step_size, args.hmc_trajectory_length) for i in range(16)])
    assert ex["hmc_mean_leapfrog"] == mean_l
    for name in ("min", "median", "mean"):
        assert ex["ess_per_grad_" + name] == ex["ess_per_step_" + name] / mean_l
    ex["engine"].close()
