"""GPU tests of HMC for the Cox process on the 16-chain GEMM tile (csrc/lgcp_hmc.hip: mfm_cox_hmc_step / _step_keys / _run / _warmup)
against the float64 oracle (oracle/hmc.py on targets.Tempered(dist, beta)) on the shared cases of tests/cox_hmc_cases.py: every kernel
instance, a ragged grid, three tiles, two temperatures.

What a float32 kernel may legitimately do differently is decide ``u < pa`` the other way where ``|u - pa|`` lies below its own error of
``pa``.  That error is MEASURED: cox_hmc_cases.OBSERVED holds the largest figures seen against the oracle and TOLERANCE eight times
that; chains inside the tolerance at any step are left out of the decisions' comparison, at most 10 % of a case.  Every test prints
what it observes before it asserts."""
import functools

import numpy as np
import pytest

from oracle import hmc, loop, mala, prng, targets
from tests import cox_hmc_cases as cc
from tests import warmup_ref as wr

pytestmark = pytest.mark.gpu


def _dev(x, dtype=None):
    import torch
    return torch.as_tensor(np.array(x, copy=True), dtype=dtype).cuda()


def _keys_dev(keys):
    return _dev(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32))


def _ctx(n, B, n_total=None, offset=0, example="pines", dist=None):
    from tests import gpu_util as gu
    dist = cc.dist_of(n) if dist is None else dist
    args = loop.default_args(example=example, dim=dist.dim, num_chain=B, hutchs=True, step_size=0.01, seed=1, fourier_dim=16, **gu.hidden_lists(32))
    return gu.make_ctx(dist, args, n_local=B, n_total=n_total, offset=offset)


def _state(ctx, x0, beta):
    import torch
    pos = _dev(x0, torch.float32)
    logp = torch.empty(pos.shape[0], dtype=torch.float64, device="cuda")
    grad = torch.empty_like(pos)
    ctx.mala_init(pos, beta, logp, grad)
    return pos, logp, grad


def _info(B):
    import torch
    return torch.empty(B, dtype=torch.float32, device="cuda"), torch.empty(B, dtype=torch.uint8, device="cuda")


def _host(*ts):
    return tuple(t.cpu().numpy() for t in ts)


# ---- 1. step parity ----
@functools.lru_cache(maxsize=None)
def _parity(name):
    """The case's steps on the device beside the oracle on the same keys (tests/test_gpu_hmc.py's protocol: both sides continue from the
    KERNEL's decisions, and the oracle restarts from the device's float32 state after each step): the observed figures."""
    c = cc.BY_NAME[name]
    vg = cc.value_and_grad_of(c)
    ctx = _ctx(c.n, c.B)
    try:
        pos, logp, grad = _state(ctx, cc.start_of(name), c.beta)
        acc, isacc = _info(c.B)
        rows = []
        for j in range(c.n_steps):
            st = mala.MALAState(pos.cpu().numpy().astype(np.float64), logp.cpu().numpy(), grad.cpu().numpy().astype(np.float64))
            key = cc.key_of(c, j)
            ctx.cox_hmc_step(key, c.beta, c.eps, c.L, pos, logp, grad, acc, isacc)
            _, info, u = hmc.kernel(prng.split(key, c.B), st, vg, c.eps, c.L)
            pa_g, ia_g, pos_g, logp_g = _host(acc, isacc, pos, logp)
            rows.append(dict(st=st, info=info, u=u, pa=pa_g.astype(np.float64), acc=ia_g.astype(bool), pos=pos_g.astype(np.float64), logp=logp_g,
                             lp_end=vg(info.proposed_position)[0]))
        return tuple(rows)
    finally:
        ctx.close()


def _figures(rows):
    e_pa = e_pos = e_lp = 0.0
    for r in rows:
        s_lp = max(1.0, np.abs(r["st"].logdensity).max())
        s_x = max(1.0, np.abs(r["st"].position).max())
        e_pa = max(e_pa, np.abs(np.log(np.maximum(r["pa"], 1e-30)) - np.log(np.maximum(r["info"].acceptance_rate, 1e-30))).max() / s_lp)
        a = r["acc"]
        if a.any():
            e_pos = max(e_pos, np.abs(r["pos"][a] - r["info"].proposed_position[a]).max() / s_x)
            e_lp = max(e_lp, np.abs(r["logp"][a] - r["lp_end"][a]).max() / s_lp)
    return dict(log_pa=e_pa, position=e_pos, logp=e_lp)


@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_step_matches_oracle(name):
    rows = _parity(name)
    obs = _figures(rows)
    print("cox_hmc parity", name, " ".join(f"{k}={v:.4e}" for k, v in obs.items()))
    assert all(v is not None for v in cc.TOLERANCE.values()), "tests/cox_hmc_cases.py: TOLERANCE has not been measured"
    for k, v in obs.items():
        assert v <= cc.TOLERANCE[k], (name, k, v)
    left_out = np.zeros(len(rows[0]["u"]), dtype=bool)
    for r in rows:
        pa_o = r["info"].acceptance_rate
        s_lp = max(1.0, np.abs(r["st"].logdensity).max())
        border = np.abs(r["u"] - pa_o) <= cc.TOLERANCE["log_pa"] * s_lp * np.maximum(pa_o, 1e-30) + 2.0 ** -24      # (+ the float32 info array)
        assert (r["acc"] == r["info"].is_accepted)[~border].all(), name
        left_out |= border
        # a rejected row keeps its state bit for bit
        assert np.array_equal(r["pos"][~r["acc"]], r["st"].position[~r["acc"]]) and np.array_equal(r["logp"][~r["acc"]], r["st"].logdensity[~r["acc"]])
    assert left_out.mean() <= cc.MAX_SHARE, (name, left_out.mean())


def test_both_decisions_are_seen():
    seen = set()
    for c in cc.CASES:
        for r in _parity(c.name):
            seen |= set(r["acc"].tolist())
    assert seen == {True, False}


# ---- 2. keys ----
@pytest.mark.parametrize("name", ["10x10", "16x16"])
def test_step_equals_step_keys(name):
    c = cc.BY_NAME[name]
    ctx = _ctx(c.n, c.B)
    try:
        key = cc.key_of(c, 0)
        out = []
        for per_chain in (False, True):
            pos, logp, grad = _state(ctx, cc.start_of(name), c.beta)
            acc, isacc = _info(c.B)
            if per_chain:
                ctx.cox_hmc_step_keys(_keys_dev(prng.split(key, c.B)), c.beta, c.eps, c.L, pos, logp, grad, acc, isacc)
            else:
                ctx.cox_hmc_step(key, c.beta, c.eps, c.L, pos, logp, grad, acc, isacc)
            out.append(_host(pos, logp, grad, acc, isacc))
        for a, b in zip(*out):
            assert np.array_equal(a, b)
        assert out[0][4].any()
    finally:
        ctx.close()


# ---- 3. run ----
def _run_vs_steps(name, key_mode, thin):
    import torch
    c = cc.BY_NAME[name]
    n = 4 if thin else c.n_steps
    ctx = _ctx(c.n, c.B)
    try:
        key = cc.key_of(c, 7)
        keys = prng.split(prng.PRNGKey(77 + c.seed), c.B)
        pos, logp, grad = _state(ctx, cc.start_of(name), c.beta)
        acc, isacc = _info(c.B)
        n_acc = torch.empty(c.B, dtype=torch.int32, device="cuda"); acc_sum = torch.empty(c.B, dtype=torch.float64, device="cuda")
        tp = torch.empty(n // thin, c.B, c.d, device="cuda") if thin else None
        tl = torch.empty(n // thin, c.B, dtype=torch.float64, device="cuda") if thin else None
        ctx.cox_hmc_run(_keys_dev(keys) if key_mode else key, c.beta, c.eps, c.L, n, pos, logp, grad, thin=thin, n_acc=n_acc, acc_sum=acc_sum, acc=acc,
                        is_acc=isacc, traj_pos=tp, traj_logp=tl)
        run = _host(pos, logp, grad, acc, isacc, n_acc, acc_sum)
        traj = _host(tp, tl) if thin else None
        pos, logp, grad = _state(ctx, cc.start_of(name), c.beta)
        acc, isacc = _info(c.B)
        tally, psum, kept = np.zeros(c.B, dtype=np.int32), np.zeros(c.B), []
        for j in range(n):
            kj = np.stack([prng.split(keys[b], n)[j] for b in range(c.B)]) if key_mode else prng.split(prng.split(key, n)[j], c.B)
            ctx.cox_hmc_step_keys(_keys_dev(kj), c.beta, c.eps, c.L, pos, logp, grad, acc, isacc)
            a, ia = _host(acc, isacc)
            tally += ia.astype(np.int32); psum += a.astype(np.float64)
            if thin and (j + 1) % thin == 0:
                kept.append(_host(pos, logp))
        steps = _host(pos, logp, grad, acc, isacc)
        for a, b in zip(run[:5], steps):
            assert np.array_equal(a, b), (name, key_mode)
        assert np.array_equal(run[5], tally) and 0 < tally.sum()
        np.testing.assert_allclose(run[6], psum, rtol=2.0 ** -24 + n * 2.0 ** -52, atol=n * 2.0 ** -150)      # (the info array is float32: tests/test_gpu_hmc_run.py)
        if thin:
            assert np.array_equal(traj[0], np.stack([k[0] for k in kept])) and np.array_equal(traj[1], np.stack([k[1] for k in kept]))
            assert not np.array_equal(traj[0][0], traj[0][-1])
    finally:
        ctx.close()


@pytest.mark.parametrize("key_mode", [0, 1])
@pytest.mark.parametrize("name", ["10x10", "16x16", "32x32"])
def test_run_equals_single_steps(name, key_mode):
    _run_vs_steps(name, key_mode, 0)


def test_run_thinned_rows_are_those_steps_states():
    _run_vs_steps("10x10", 0, 2)


# ---- 4. warmup ----
@pytest.mark.parametrize("name", ["4x4", "16x16"])
def test_warmup_steps_and_recursion(name):
    import torch
    c = cc.BY_NAME[name]
    n, target = 8, 0.7
    ctx = _ctx(c.n, c.B)
    try:
        key = cc.key_of(c, 9)
        pos, logp, grad = _state(ctx, cc.start_of(name), c.beta)
        f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device="cuda")
        step_avg, step_last, acc_sum, traj = f64(c.B), f64(c.B), f64(c.B), f64(n, c.B)
        n_acc = torch.empty(c.B, dtype=torch.int32, device="cuda")
        ctx.cox_hmc_warmup(key, c.beta, c.eps, c.L, n, target, pos, logp, grad, step_avg, step_last=step_last, n_acc=n_acc, acc_sum=acc_sum, step_traj=traj)
        w_pos, w_logp, w_grad, w_avg, w_last, w_sum, w_traj, w_nacc = _host(pos, logp, grad, step_avg, step_last, acc_sum, traj, n_acc)
        assert np.array_equal(w_traj[0], np.full(c.B, c.eps)) and (w_traj[1:] != c.eps).any()
        # step m of chain b = a single-step launch at the scalar step size step_traj[m, b]: one chain per tile at a time, the others' rows aside
        tiles = c.B // 16
        pa = np.zeros((n, c.B))
        tally = np.zeros(c.B, dtype=np.int32)
        acc, isacc = _info(c.B)
        for r in (0, 5, 15):
            rows = np.array([16 * t + r for t in range(tiles)])
            pos, logp, grad = _state(ctx, cc.start_of(name), c.beta)
            for m in range(n):
                kj = _keys_dev(prng.split(prng.split(key, n)[m], c.B))
                nxt = [t.clone() for t in (pos, logp, grad)]
                for b in rows:                                   # (tiles may differ in step size: one launch each, its row kept)
                    trial = [t.clone() for t in (pos, logp, grad)]
                    ctx.cox_hmc_step_keys(kj, c.beta, float(w_traj[m, b]), c.L, *trial, acc, isacc)
                    for dst, src in zip(nxt, trial):
                        dst[b] = src[b]
                    pa[m, b] = float(acc[b]); tally[b] += int(isacc[b])
                pos, logp, grad = nxt
            got = _host(pos, logp, grad)
            for a, b in zip(got, (w_pos, w_logp, w_grad)):
                assert np.array_equal(a[rows], b[rows]), (name, r)
            assert np.array_equal(tally[rows], w_nacc[rows])
        # the recursion of tests/warmup_ref.py from the device's own acceptance probabilities (float32 info arrays: their rounding moves
        # x_m by sqrt(m) / gamma / (m + t0) * 2^-24 at most, tests/test_gpu_warmup.py's bound)
        rows = np.array(sorted(16 * t + r for t in range(tiles) for r in (0, 5, 15)))
        t_ref, last_ref, avg_ref = wr.replay(pa[:, rows], c.eps, target)
        print("cox_hmc warmup", name, "max rel err step_traj", np.abs(w_traj[:, rows] / t_ref - 1).max(), "step_avg", np.abs(w_avg[rows] / avg_ref - 1).max())
        rtol = 2 * (np.sqrt(n) / wr.GAMMA) * 2.0 ** -24 + 1e-12      # tests/test_gpu_warmup.py's: the rounding of p to float32, amplified by the recursion
        np.testing.assert_allclose(w_traj[:, rows], t_ref, rtol=rtol, atol=0)
        np.testing.assert_allclose(w_last[rows], last_ref, rtol=rtol, atol=0)
        np.testing.assert_allclose(w_avg[rows], avg_ref, rtol=rtol, atol=0)
        np.testing.assert_allclose(w_sum[rows], pa[:, rows].sum(0), rtol=2.0 ** -24 + n * 2.0 ** -52, atol=n * 2.0 ** -150)
    finally:
        ctx.close()


# ---- 5. shard invariance ----
def test_shard_reproduces_its_chains():
    """A context holding chains [16, 48) of 64 reproduces those chains of the one-context run bit for bit: step, run and warmup (4 x 4)."""
    import torch
    c = cc.BY_NAME["4x4"]
    xi = prng.normal_rows(prng.split(prng.PRNGKey(611), 64), c.d)
    dist = cc.dist_of(c.n)
    x0 = (dist.mu + xi @ dist.chol.T).astype(np.float32)
    key = cc.key_of(c, 11)

    def go(ctx, x):
        B = x.shape[0]
        out = []
        pos, logp, grad = _state(ctx, x, c.beta)
        acc, isacc = _info(B)
        ctx.cox_hmc_step(key, c.beta, c.eps, c.L, pos, logp, grad, acc, isacc)
        out += _host(pos, logp, grad, acc, isacc)
        n_acc = torch.empty(B, dtype=torch.int32, device="cuda"); acc_sum = torch.empty(B, dtype=torch.float64, device="cuda")
        ctx.cox_hmc_run(key, c.beta, c.eps, c.L, 3, pos, logp, grad, n_acc=n_acc, acc_sum=acc_sum, acc=acc, is_acc=isacc)
        out += _host(pos, logp, grad, acc, isacc, n_acc, acc_sum)
        avg, last, traj = (torch.empty(s, dtype=torch.float64, device="cuda") for s in ((B,), (B,), (4, B)))
        ctx.cox_hmc_warmup(key, c.beta, c.eps, c.L, 4, 0.7, pos, logp, grad, avg, step_last=last, n_acc=n_acc, acc_sum=acc_sum, step_traj=traj)
        out += _host(pos, logp, grad, avg, last, n_acc, acc_sum) + (traj.cpu().numpy().T,)
        return out

    full = _ctx(c.n, 64)
    try:
        whole = go(full, x0)
    finally:
        full.close()
    shard = _ctx(c.n, 32, n_total=64, offset=16)
    try:
        part = go(shard, x0[16:48])
    finally:
        shard.close()
    for a, b in zip(whole, part):
        assert np.array_equal(a[16:48], b)


# ---- 6. errors ----
def test_refusals_touch_nothing():
    import torch
    from mfm_amd import _lib
    from tests import gpu_util as gu
    c = cc.BY_NAME["4x4"]
    ctx = _ctx(c.n, c.B)
    try:
        pos, logp, grad = _state(ctx, cc.start_of("4x4"), 1.0)
        before = _host(pos, logp, grad)
        keys = _keys_dev(prng.split(prng.PRNGKey(1), c.B))
        key = prng.PRNGKey(2)
        avg = torch.empty(c.B, dtype=torch.float64, device="cuda")
        tp = torch.empty(2, c.B, c.d, device="cuda")

        def refused(msg, fn, *a, **kw):
            with pytest.raises(_lib.MfmError, match=msg):
                fn(*a, **kw)
            ctx.sync()
            for x, y in zip(before, _host(pos, logp, grad)):
                assert np.array_equal(x, y), msg

        refused("step_size must be positive", ctx.cox_hmc_step, key, 1.0, 0.0, 3, pos, logp, grad)
        refused("null device pointer", ctx.cox_hmc_step, key, 1.0, 0.1, 3, pos, None, grad)
        refused("num_steps", ctx.cox_hmc_step, key, 1.0, 0.1, 0, pos, logp, grad)
        refused("num_steps", ctx.cox_hmc_step_keys, keys, 1.0, 0.1, 100001, pos, logp, grad)
        refused("null key array", ctx.cox_hmc_step_keys, None, 1.0, 0.1, 3, pos, logp, grad)
        refused("num_steps", ctx.cox_hmc_run, key, 1.0, 0.1, 0, 4, pos, logp, grad)
        refused("n_steps must be at least 1", ctx.cox_hmc_run, key, 1.0, 0.1, 3, 0, pos, logp, grad)
        refused("key_mode", ctx.cox_hmc_run, key, 1.0, 0.1, 3, 4, pos, logp, grad, key_mode=2)
        refused("key_mode 1 needs d_keys", ctx.cox_hmc_run, key, 1.0, 0.1, 3, 4, pos, logp, grad, key_mode=1)
        refused("must divide n_steps", ctx.cox_hmc_run, key, 1.0, 0.1, 3, 4, pos, logp, grad, thin=3, traj_pos=tp)
        refused("thin > 0 needs", ctx.cox_hmc_run, key, 1.0, 0.1, 3, 4, pos, logp, grad, thin=2)
        refused("target_accept", ctx.cox_hmc_warmup, key, 1.0, 0.1, 3, 4, 1.0, pos, logp, grad, avg)
        refused("num_steps", ctx.cox_hmc_warmup, key, 1.0, 0.1, 0, 4, 0.8, pos, logp, grad, avg)
        # an installed inverse mass: as mfm_pt_run
        ctx.set_inverse_mass(np.full(c.d, 2.0))
        for fn, a in ((ctx.cox_hmc_step, (key, 1.0, 0.1, 3, pos, logp, grad)), (ctx.cox_hmc_step_keys, (keys, 1.0, 0.1, 3, pos, logp, grad)),
                      (ctx.cox_hmc_run, (key, 1.0, 0.1, 3, 4, pos, logp, grad)), (ctx.cox_hmc_warmup, (key, 1.0, 0.1, 3, 4, 0.8, pos, logp, grad, avg))):
            refused("unit mass: remove the installed inverse mass", fn, *a)
        ctx.set_inverse_mass(None)
        acc, isacc = _info(c.B)
        ctx.cox_hmc_step(key, 1.0, c.eps, c.L, pos, logp, grad, acc, isacc)      # and the context still serves
        assert isacc.any().item()
    finally:
        ctx.close()
    # another target: the call to use is named
    args, dist, k, model, state = gu.phi4_setup(d=64, B=16, hidden=32, F=16)
    ctx = gu.make_ctx(dist, args)
    try:
        pos, logp, grad = _state(ctx, dist.init_params.astype(np.float32), 1.0)
        before = _host(pos, logp, grad)
        avg = torch.empty(16, dtype=torch.float64, device="cuda")
        for fn, a in ((ctx.cox_hmc_step, (key, 1.0, 1e-4, 3, pos, logp, grad)), (ctx.cox_hmc_step_keys, (keys, 1.0, 1e-4, 3, pos, logp, grad)),
                      (ctx.cox_hmc_run, (key, 1.0, 1e-4, 3, 4, pos, logp, grad)), (ctx.cox_hmc_warmup, (key, 1.0, 1e-4, 3, 4, 0.8, pos, logp, grad, avg))):
            with pytest.raises(_lib.MfmError, match=r"use mfm_hmc_\*"):
                fn(*a)
        ctx.sync()
        for x, y in zip(before, _host(pos, logp, grad)):
            assert np.array_equal(x, y)
    finally:
        ctx.close()


def test_shape_beyond_the_instances_is_too_large():
    """A 33 x 33 grid (dim 1089 > 1024): MFM_ETOOLARGE from every entry point, positions unchanged (the context is the wide family's
    where the tile family declines the shape)."""
    import torch
    from mfm_amd import _lib
    from tests import gpu_util as gu
    n, B = 33, 16
    d = n * n
    counts = np.random.default_rng(5).poisson(126.0 / d, d).astype(np.float64)
    dist = targets.LogGaussianCoxPines(d, counts)
    args = loop.default_args(example="pines", dim=d, num_chain=B, hutchs=True, step_size=0.01, seed=1, fourier_dim=16, **gu.hidden_lists(32))
    try:
        ctx = gu.make_ctx(dist, args, n_local=B)
    except _lib.MfmError as e:
        assert "does not fit" in str(e), str(e)
        ctx = gu.make_ctx(dist, args, n_local=B, family=_lib.FAMILY_WIDE)
    try:
        x0 = np.full((B, d), float(dist.mu), dtype=np.float32)
        pos, logp, grad = _state(ctx, x0, 1.0)
        before = _host(pos, logp, grad)
        avg = torch.empty(B, dtype=torch.float64, device="cuda")
        key = prng.PRNGKey(3)
        keys = _keys_dev(prng.split(key, B))
        for fn, a in ((ctx.cox_hmc_step, (key, 1.0, 0.1, 3, pos, logp, grad)), (ctx.cox_hmc_step_keys, (keys, 1.0, 0.1, 3, pos, logp, grad)),
                      (ctx.cox_hmc_run, (key, 1.0, 0.1, 3, 4, pos, logp, grad)), (ctx.cox_hmc_warmup, (key, 1.0, 0.1, 3, 4, 0.8, pos, logp, grad, avg))):
            with pytest.raises(_lib.MfmError, match="too large for the Cox process HMC kernel"):
                fn(*a)
        ctx.sync()
        for x, y in zip(before, _host(pos, logp, grad)):
            assert np.array_equal(x, y)
    finally:
        ctx.close()


# ---- 7. Python ----
def test_python_kernel_on_the_cox_process():
    import torch
    from mfm_amd import distributions as D, random as jr
    from mfm_amd.bblackjax.mcmc import hmc as H
    from mfm_amd.engine import Engine
    from mfm_amd.mcmc_utils import inference_loop0
    B, d, eps, L = 32, 64, 0.3, 4
    dist = D.LogGaussianCoxPines(d)
    from tests import gpu_util as gu
    args = loop.default_args(example="pines", dim=d, num_chain=B, hutchs=True, fourier_dim=16, **gu.hidden_lists(32))
    dist.initialize_model(jr.PRNGKey(3), B)
    eng = Engine(dist, args, None)
    try:
        x0 = eng.local(dist.init_params)
        alg = H.hmc(dist.logprob, eps, L)
        st = alg.init(x0)
        keep = [t.clone() for t in st]
        key = jr.PRNGKey(4)

        def fresh():
            return [t.clone() for t in keep]

        # step
        st2, info = alg.step(key, st)
        pos, logp, grad = fresh(); acc, isacc = _info(B)
        eng.ctx.cox_hmc_step(key, 1.0, eps, L, pos, logp, grad, acc, isacc)
        assert torch.equal(st2.position, pos) and torch.equal(st2.logdensity, logp) and torch.equal(st2.logdensity_grad, grad)
        assert torch.equal(info.acceptance_rate, acc) and torch.equal(info.is_accepted, isacc.bool()) and info.is_accepted.any()
        assert all(torch.equal(a, b) for a, b in zip(st, keep))                        # states are values: the input is untouched
        assert torch.equal((st2.position != st.position).any(1), info.is_accepted)
        # the caller's own keys
        keys = np.asarray(jr.split(key, B))
        st3, info3 = alg.step(keys, st)
        assert torch.equal(st3.position, st2.position) and torch.equal(info3.acceptance_rate, info.acceptance_rate)
        # run
        st4, rinfo = alg.step.run(key, st, 4, thin=2)
        pos, logp, grad = fresh()
        n_acc = torch.empty(B, dtype=torch.int32, device="cuda"); acc_sum = torch.empty(B, dtype=torch.float64, device="cuda")
        eng.ctx.cox_hmc_run(key, 1.0, eps, L, 4, pos, logp, grad, n_acc=n_acc, acc_sum=acc_sum)
        assert torch.equal(st4.position, pos) and torch.equal(st4.logdensity, logp) and torch.equal(rinfo.num_accepted, n_acc)
        assert torch.equal(rinfo.acceptance_rate, acc_sum / 4) and rinfo.positions.shape == (2, B, d) and torch.equal(rinfo.positions[-1], pos)
        assert isinstance(rinfo, H.HMCRunInfo) and all(torch.equal(a, b) for a, b in zip(st, keep))
        # warmup
        st5, winfo = alg.step.warmup(key, st, 6, 0.7, keep_step_sizes=True)
        pos, logp, grad = fresh()
        avg = torch.empty(B, dtype=torch.float64, device="cuda"); last = torch.empty_like(avg)
        eng.ctx.cox_hmc_warmup(key, 1.0, eps, L, 6, 0.7, pos, logp, grad, avg, step_last=last)
        assert torch.equal(st5.position, pos) and torch.equal(winfo.step_size, avg) and torch.equal(winfo.last_step_size, last)
        assert isinstance(winfo, H.HMCWarmupInfo) and winfo.step_sizes.shape == (6, B)
        assert abs(winfo.pooled_step_size - float(torch.exp(avg.log().mean()))) < 1e-12 * winfo.pooled_step_size
        assert all(torch.equal(a, b) for a, b in zip(st, keep))
        # inference_loop0 picks .run up: stacked states from one call
        states, linfo = inference_loop0(key, st, alg.step, 4)
        assert states.position.shape == (4, B, d) and torch.equal(states.position[-1], st4.position) and torch.equal(states.position[1], rinfo.positions[0])
        with pytest.raises(ValueError, match="inverse_mass_matrix is not served on the Cox process"):
            H.hmc(dist.logprob, eps, L, inverse_mass_matrix=np.ones(d))
        with pytest.raises(ValueError, match="num_integration_steps_per_step"):
            alg.step.run(key, st, 4, num_integration_steps_per_step=[1, 2, 3, 4])
    finally:
        eng.close()


# ---- 8. loop ----
LOOP = dict(example="pines", dim=64, num_chain=32, learning_iter=5, mcmc_per_flow_steps=8.0, hutchs=True, fourier_dim=16, seed=7, eval_iter=1,
            step_size=0.3, hidden_x=[32, 32], hidden_t=[32, 32], hidden_xt=[32, 32], mcmc_kernel="hmc", hmc_steps=4)


def test_loop_with_the_hmc_kernel_on_pines_matches_the_oracle_loop():
    """--example pines --mcmc_kernel hmc --hmc_steps 4 on an 8 x 8 grid, fewer iterations than mcmc_per_flow_steps (only iteration 0 takes
    a flow step): losses and acceptance against oracle.loop.run in the same mode (oracle/flow.py takes any target with mcmc_kernel="hmc")."""
    from mfm_amd import distributions as D, exe_flow_matching as E
    dg = D.LogGaussianCoxPines(64)
    out = loop.run(targets.LogGaussianCoxPines(64, dg.counts), loop.default_args(**LOOP))
    res, res_, ex = E.run(dg, loop.default_args(**LOOP), None, log_every=1000, return_extras=True)
    try:
        lg, lo = ex["metrics"][:, 0], np.asarray(out["trace"]["loss"])
        ag, ao = ex["metrics"][:, 1], np.asarray(out["trace"]["acc_mean"])
        print("cox_hmc loop: loss", lg, lo, "acceptance", ag, ao)
        np.testing.assert_allclose(lg, lo, rtol=2e-5)
        np.testing.assert_allclose(ag[1:], ao[1:], atol=1.5 / 32)          # (a borderline decision moves the mean by 1 / 32)
        assert (ag[1:] > 0.3).all(), ag
    finally:
        ex["engine"].close()


def test_loop_adapts_and_measures_ess_on_pines():
    from mfm_amd import distributions as D, exe_flow_matching as E
    kw = dict(LOOP, learning_iter=2, adapt_steps=8, adapt_target=0.7, ess_steps=16)
    res, res_, ex = E.run(D.LogGaussianCoxPines(64), loop.default_args(**kw), None, log_every=1000, return_extras=True)
    try:
        assert np.isfinite(ex["adapted_step_size"]) and ex["adapted_step_size"] > 0 and ex["adapted_step_size"] != LOOP["step_size"]
        assert 0 < ex["adapt_acceptance"] <= 1
        for name in ("ess_per_step_min", "ess_per_step_mean", "ess_per_grad_mean", "rhat_max", "ess_multichain_per_step_mean", "ess_multichain_per_grad_mean"):
            assert np.isfinite(ex[name]), name
        assert ex["ess_per_grad_mean"] == pytest.approx(ex["ess_per_step_mean"] / 4)
    finally:
        ex["engine"].close()
