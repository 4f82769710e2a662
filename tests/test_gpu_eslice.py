"""GPU tests of elliptical slice sampling for the Cox process (csrc/eslice.hip: mfm_eslice_init / _step / _step_keys / _run) against the
float64 restatement tests/eslice_ref.py, on the shared cases of tests/eslice_cases.py (every kernel instance, a ragged grid, three
tiles, two temperatures).

What a float32 kernel may legitimately do differently is decide a comparison whose margin ``|beta ll(x') - log y|`` lies below its own
log-likelihood error.  That error is MEASURED: eslice_cases.OBSERVED holds the largest difference seen against the restatement and
TOLERANCE eight times that; chains of the restatement with a margin below TOLERANCE["loglik"] are left out of a comparison, at most 10 %
of a case, and every other chain must make the restatement's decisions.  Every test prints what it observes before it asserts."""
import functools

import numpy as np
import pytest

from oracle import loop, prng, targets
from tests import eslice_cases as ec
from tests import eslice_ref as er

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24      # float32 unit roundoff


def _dev(x, dtype=None):
    import torch
    return torch.as_tensor(np.array(x, copy=True), dtype=dtype).cuda()


def _keys_dev(keys):
    return _dev(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32))


def _args(d, B, example="pines"):
    from tests import gpu_util as gu
    return loop.default_args(example=example, dim=d, num_chain=B, hutchs=True, step_size=0.01, seed=1, fourier_dim=16, **gu.hidden_lists(32))


def _ctx(n, B, n_total=None, offset=0, chol=True):
    """A context on the n x n Cox process with B local chains (the wide family where the tile family declines the shape)."""
    from mfm_amd import _lib
    from tests import gpu_util as gu
    dist = ec.dist_of(n)
    args = _args(n * n, B)
    try:
        ctx = gu.make_ctx(dist, args, n_local=B, n_total=n_total, offset=offset)
    except _lib.MfmError as e:
        assert "does not fit" in str(e), str(e)
        ctx = gu.make_ctx(dist, args, n_local=B, n_total=n_total, offset=offset, family=_lib.FAMILY_WIDE)
    if chol:
        ctx.set_lgcp_chol(dist.chol)
    return ctx


def _state(ctx, x0):
    import torch
    pos = _dev(x0, torch.float32)
    ll = torch.empty(pos.shape[0], dtype=torch.float64, device="cuda")
    ctx.eslice_init(pos, ll)
    return pos, ll


def _info_bufs(B, d):
    import torch
    return (torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.float64, device="cuda"),
            torch.empty(B, d, dtype=torch.float32, device="cuda"))


def _tol(kind):
    t = ec.TOLERANCE[kind]
    assert t is not None, "tests/eslice_cases.py: TOLERANCE has not been measured"
    return t


def _compared(name, infos):
    """The chains of a case that are compared: the restatement's margin is at least the measured tolerance in every decision."""
    keep = er.min_margin(infos) >= _tol("loglik")
    assert (~keep).mean() <= ec.MAX_SHARE, (name, (~keep).mean())
    return keep


@functools.lru_cache(maxsize=None)
def _device_run(name):
    """The case's end-to-end run on the device, once: init, then ``n_steps`` transitions in one launch with ``thin = 1``."""
    import torch
    c = ec.BY_NAME[name]
    ctx = _ctx(c.n, c.B)
    try:
        pos, ll = _state(ctx, ec.start_of(name))
        ll0 = ll.cpu().numpy()
        sub_sum = torch.empty(c.B, dtype=torch.int32, device="cuda")
        capped, sub_max = torch.empty_like(sub_sum), torch.empty_like(sub_sum)
        tx = torch.empty(c.n_steps, c.B, c.d, dtype=torch.float32, device="cuda")
        tl = torch.empty(c.n_steps, c.B, dtype=torch.float64, device="cuda")
        sub, theta, mom = _info_bufs(c.B, c.d)
        ctx.eslice_run(ec.key_of(c), c.beta, c.n_steps, pos, ll, thin=1, subiter_sum=sub_sum, n_capped=capped, traj_pos=tx, traj_loglik=tl,
                       subiter=sub, theta=theta, momentum=mom, subiter_max=sub_max)
        ctx.sync()
        return dict(ll0=ll0, pos=pos.cpu().numpy(), ll=ll.cpu().numpy(), sub_sum=sub_sum.cpu().numpy(), capped=capped.cpu().numpy(),
                    sub_max=sub_max.cpu().numpy(), tx=tx.cpu().numpy(), tl=tl.cpu().numpy(), sub=sub.cpu().numpy(), theta=theta.cpu().numpy(),
                    mom=mom.cpu().numpy())
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def _device_step(name, beta=None):
    """The case's FIRST transition as a single-step launch on split(key, n_steps)[0] (what the run's first transition uses)."""
    c = ec.BY_NAME[name]
    ctx = _ctx(c.n, c.B)
    try:
        pos, ll = _state(ctx, ec.start_of(name))
        sub, theta, mom = _info_bufs(c.B, c.d)
        ctx.eslice_step(prng.split(ec.key_of(c), c.n_steps)[0], c.beta if beta is None else beta, pos, ll, sub, theta, mom)
        ctx.sync()
        return dict(pos=pos.cpu().numpy(), ll=ll.cpu().numpy(), sub=sub.cpu().numpy(), theta=theta.cpu().numpy(), mom=mom.cpu().numpy())
    finally:
        ctx.close()


NAMES = [c.name for c in ec.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_init_is_the_loglikelihood_of_every_row(name):
    """mfm_eslice_init against the float64 sum: float32 expf (about an ulp) and float64 accumulation, so per row at most
    4 u sum_i |x_i c_i| + |a e^x_i| -- no measured number."""
    c = ec.BY_NAME[name]
    dist = ec.dist_of(c.n)
    x = ec.start_of(name).astype(np.float64)
    got, want = _device_run(name)["ll0"], er.loglik(dist, x)
    bound = 4 * U32 * (np.abs(x * dist.counts[None]) + dist.poisson_a * np.exp(x)).sum(1)
    print(f"{name}: init |dll| max {np.abs(got - want).max():.3e}, bound min {bound.min():.3e}")
    assert (np.abs(got - want) <= bound).all()


@pytest.mark.parametrize("name", NAMES)
def test_momentum_is_L_n(name):
    """d_momentum against L n in float64, per element within the rigorous float32 dot-product bound d 2^-24 sum_k |L_jk| |n_k|."""
    c = ec.BY_NAME[name]
    dist = ec.dist_of(c.n)
    info = ec.reference_of(name)[2][0]
    got = _device_step(name)["mom"].astype(np.float64)
    bound = c.d * U32 * (np.abs(info.normals) @ np.abs(dist.chol).T)
    err = np.abs(got - info.momentum)
    print(f"{name}: momentum max err / bound {np.max(err / bound):.3e}, max err {err.max():.3e}")
    assert (err <= bound).all()


@pytest.mark.parametrize("name", ["4x4", "10x10", "16x16", "40x40"])
def test_beta_zero_accepts_the_first_proposal(name):
    """beta = 0: subiter == 1 everywhere, and x' is the ellipse point of the RETURNED theta and momentum to float32 rounding: the head
    x - mu is rounded (u), cos and sin come from float32 functions (2 ulp = 4 u each) and the two fused multiply-adds round once each,
    so per element at most 8 u (|mu| + |x - mu| + |nu|)."""
    c = ec.BY_NAME[name]
    dist = ec.dist_of(c.n)
    x0 = ec.start_of(name).astype(np.float64)
    out = _device_step(name, 0.0)
    assert (out["sub"] == 1).all()
    nu, th = out["mom"].astype(np.float64), out["theta"]
    want = dist.mu + (x0 - dist.mu) * np.cos(th)[:, None] + nu * np.sin(th)[:, None]
    bound = 8 * U32 * (abs(dist.mu) + np.abs(x0 - dist.mu) + np.abs(nu))
    err = np.abs(out["pos"] - want)
    print(f"{name}: beta 0 max err / bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()
    ref_theta = er.TWO_PI * prng.uniform_rows(prng.split_rows(er.chain_keys(prng.split(ec.key_of(c), c.n_steps)[0], c.B), 4)[:, 2])
    np.testing.assert_allclose(th, ref_theta, rtol=4e-16, atol=0)
    np.testing.assert_allclose(out["ll"], er.loglik(dist, out["pos"]), rtol=0, atol=_tol("loglik"))


@pytest.mark.parametrize("name", NAMES)
def test_one_transition_against_the_restatement(name):
    c = ec.BY_NAME[name]
    x, ll, infos, tx, tl = ec.reference_of(name)
    info = infos[0]
    out = _device_step(name)
    keep = _compared(name, infos[:1])
    dl, dx = np.abs(out["ll"] - tl[0])[keep].max(), np.abs(out["pos"] - tx[0])[keep].max()
    print(f"{name}: one transition, compared {keep.sum()}/{c.B}, |dll| {dl:.3e}, |dx| {dx:.3e}, evaluations {info.subiter.tolist()}")
    np.testing.assert_array_equal(out["sub"][keep], info.subiter[keep])          # identical subiter: identical decisions
    np.testing.assert_allclose(out["theta"][keep], info.theta[keep], rtol=0, atol=8 * 2.0 ** -53 * er.TWO_PI)
    assert dl <= _tol("loglik") and dx <= _tol("position")


@pytest.mark.parametrize("name", NAMES)
def test_run_against_the_restatement(name):
    """End to end: every kept state of the run, the evaluation counts and the cap tally, under the same exclusion rule."""
    c = ec.BY_NAME[name]
    x, ll, infos, tx, tl = ec.reference_of(name)
    out = _device_run(name)
    keep = _compared(name, infos)
    sub = np.stack([i.subiter for i in infos])
    dl, dx = np.abs(out["tl"] - tl)[:, keep].max(), np.abs(out["tx"] - tx)[:, keep].max()
    print(f"{name}: run of {c.n_steps}, compared {keep.sum()}/{c.B}, |dll| {dl:.3e}, |dx| {dx:.3e}, mean evaluations {sub.mean():.2f}")
    np.testing.assert_array_equal(out["sub_sum"][keep], sub.sum(0)[keep])
    np.testing.assert_array_equal(out["sub_max"][keep], sub.max(0)[keep])
    np.testing.assert_array_equal(out["sub"][keep], sub[-1][keep])
    assert (out["capped"] == 0).all()
    assert dl <= _tol("loglik") and dx <= _tol("position")
    np.testing.assert_array_equal(out["pos"], out["tx"][-1])
    np.testing.assert_array_equal(out["ll"], out["tl"][-1])
    np.testing.assert_allclose(out["theta"][keep], infos[-1].theta[keep], rtol=0, atol=8 * 2.0 ** -53 * er.TWO_PI)


@pytest.mark.parametrize("name", ["4x4", "10x10", "16x16", "20x20", "32x32", "40x40"])
def test_run_replays_the_single_steps_bit_for_bit(name):
    """mfm_eslice_run == n_steps mfm_eslice_step launches on split(key, n)[j] (key_mode 0) and == mfm_eslice_step_keys launches on
    split(keys[b], n)[j] (key_mode 1); the thinned trajectory is the loop's states; subiter_sum is the sum of the steps' subiter."""
    import torch
    c = ec.BY_NAME[name]
    n_steps = 4                                              # (its own count: thin = 2 keeps the states after steps 2 and 4)
    key = ec.key_of(c)
    ckeys = prng.split(prng.PRNGKey(900 + c.seed), c.B)
    ctx = _ctx(c.n, c.B)
    try:
        for mode in (0, 1):
            pos, ll = _state(ctx, ec.start_of(name))
            rpos, rll = pos.clone(), ll.clone()
            sub, theta, mom = _info_bufs(c.B, c.d)
            total = torch.zeros(c.B, dtype=torch.int32, device="cuda")
            states = []
            for j in range(n_steps):
                if mode == 0:
                    ctx.eslice_step(prng.split(key, n_steps)[j], c.beta, pos, ll, sub, theta, mom)
                else:
                    ctx.eslice_step_keys(_keys_dev(prng.split_rows(ckeys, n_steps)[:, j]), c.beta, pos, ll, sub, theta, mom)
                total += sub
                states.append((pos.clone(), ll.clone()))
            sub_sum, capped = torch.empty_like(total), torch.empty_like(total)
            tx = torch.empty(n_steps // 2, c.B, c.d, dtype=torch.float32, device="cuda")
            tl = torch.empty(n_steps // 2, c.B, dtype=torch.float64, device="cuda")
            rsub, rtheta, rmom = _info_bufs(c.B, c.d)
            ctx.eslice_run(key if mode == 0 else _keys_dev(ckeys), c.beta, n_steps, rpos, rll, thin=2, subiter_sum=sub_sum, n_capped=capped,
                           traj_pos=tx, traj_loglik=tl, subiter=rsub, theta=rtheta, momentum=rmom)
            assert torch.equal(rpos, pos) and torch.equal(rll, ll), (name, mode)
            assert torch.equal(sub_sum, total) and capped.sum().item() == 0
            assert torch.equal(rsub, sub) and torch.equal(rtheta, theta) and torch.equal(rmom, mom)
            for k in range(n_steps // 2):
                assert torch.equal(tx[k], states[2 * k + 1][0]) and torch.equal(tl[k], states[2 * k + 1][1])
    finally:
        ctx.close()


def test_a_shard_equals_its_rows_of_the_full_run():
    """(n_local, n_total, chain_offset) = (16, 48, 16) and (32, 48, 16): the chains are independent, draws are indexed by the global id."""
    import torch
    c = ec.BY_NAME["16x16"]
    full = _device_run("16x16")
    for n_local, off in ((16, 16), (32, 16)):
        ctx = _ctx(c.n, n_local, n_total=c.B, offset=off)
        try:
            pos, ll = _state(ctx, ec.start_of("16x16")[off:off + n_local])
            sub_sum = torch.empty(n_local, dtype=torch.int32, device="cuda")
            ctx.eslice_run(ec.key_of(c), c.beta, c.n_steps, pos, ll, subiter_sum=sub_sum)
            np.testing.assert_array_equal(pos.cpu().numpy(), full["pos"][off:off + n_local])
            np.testing.assert_array_equal(ll.cpu().numpy(), full["ll"][off:off + n_local])
            np.testing.assert_array_equal(sub_sum.cpu().numpy(), full["sub_sum"][off:off + n_local])
        finally:
            ctx.close()


def test_a_nan_row_ends_at_the_cap_and_disturbs_nobody():
    """An ordinary input check: a state with a NaN row returns normally, reports n_capped == n_steps for that row and leaves it
    unchanged; every other row -- of its own tile and of the other tiles -- has the bits of the run without the NaN row."""
    import torch
    from mfm_amd import _lib
    c = ec.BY_NAME["16x16"]
    bad = 5
    clean = _device_run("16x16")
    x0 = ec.start_of("16x16").copy()
    x0[bad, 3] = np.nan
    ctx = _ctx(c.n, c.B)
    try:
        pos, ll = _state(ctx, x0)
        ll[bad] = -123.25                                     # (init gives NaN there; any value must come back untouched)
        before = pos.clone()
        sub_sum = torch.empty(c.B, dtype=torch.int32, device="cuda")
        capped, sub_max = torch.empty_like(sub_sum), torch.empty_like(sub_sum)
        ctx.eslice_run(ec.key_of(c), c.beta, c.n_steps, pos, ll, subiter_sum=sub_sum, n_capped=capped, subiter_max=sub_max)
        ctx.sync()
        others = np.arange(c.B) != bad
        assert capped[bad].item() == c.n_steps and sub_sum[bad].item() == c.n_steps * _lib.ESLICE_MAX_SUBITER and sub_max[bad].item() == _lib.ESLICE_MAX_SUBITER
        assert torch.equal(pos[bad].view(torch.int32), before[bad].view(torch.int32)) and ll[bad].item() == -123.25
        assert (capped.cpu().numpy()[others] == 0).all()
        np.testing.assert_array_equal(pos.cpu().numpy()[others], clean["pos"][others])
        np.testing.assert_array_equal(ll.cpu().numpy()[others], clean["ll"][others])
        np.testing.assert_array_equal(sub_sum.cpu().numpy()[others], clean["sub_sum"][others])
    finally:
        ctx.close()


def _unchanged(bufs, snaps):
    import torch
    return all(torch.equal(b.view(torch.int32), s.view(torch.int32)) for b, s in zip(bufs, snaps))


def test_refusals_touch_nothing():
    import torch
    from mfm_amd import _lib
    from tests import gpu_util as gu
    c = ec.BY_NAME["4x4"]
    key = ec.key_of(c)
    x0 = ec.start_of("4x4")

    def attempt(ctx, code, match, call):
        pos = _dev(x0, torch.float32)
        ll = torch.full((c.B,), 1.5, dtype=torch.float64, device="cuda")
        extra = (torch.full((c.B,), 7, dtype=torch.int32, device="cuda"), torch.full((2, c.B, c.d), 3.0, dtype=torch.float32, device="cuda"))
        snaps = [t.clone() for t in (pos, ll) + extra]
        with pytest.raises(_lib.MfmError, match=match) as e:
            call(ctx, pos, ll, *extra)
        assert f"error {code}:" in str(e.value), str(e.value)
        ctx.sync()
        assert _unchanged((pos, ll) + extra, snaps)

    step = lambda ctx, pos, ll, s, t: ctx.eslice_step(key, 1.0, pos, ll, s)
    run = lambda **kw: (lambda ctx, pos, ll, s, t: ctx.eslice_run(key, kw.get("beta", 1.0), kw.get("n", 4), pos, ll, thin=kw.get("thin", 0), subiter_sum=s,
                                                                  traj_pos=t if kw.get("thin", 0) else None))
    phi = gu.make_ctx(targets.PhiFour(16), _args(16, c.B, "phi-four"))
    try:
        attempt(phi, -2, "no Gaussian prior factor", step)
        attempt(phi, -2, "no Gaussian prior factor", run())
        attempt(phi, -2, "no Gaussian prior factor", lambda ctx, pos, ll, s, t: ctx.eslice_init(pos, ll))
        with pytest.raises(_lib.MfmError, match="no Gaussian prior factor"):
            phi.set_lgcp_chol(np.eye(16))
    finally:
        phi.close()
    bare = _ctx(c.n, c.B, chol=False)
    try:
        attempt(bare, -5, "mfm_set_lgcp_chol has not been called", step)
        attempt(bare, -5, "mfm_set_lgcp_chol has not been called", run())
        L = ec.dist_of(c.n).chol.copy()
        for edit, match in (((3, 2, np.inf), "finite"), ((2, 3, 1e-3), "lower triangular"), ((0, 0, np.nan), "finite")):
            Lb = L.copy()
            Lb[edit[0], edit[1]] = edit[2]
            with pytest.raises(_lib.MfmError, match=match):
                bare.set_lgcp_chol(Lb)
        attempt(bare, -5, "mfm_set_lgcp_chol has not been called", step)          # a refused factor installs nothing
        bare.set_lgcp_chol(L)
        attempt(bare, -1, "beta must be finite and not negative", run(beta=-0.5))
        attempt(bare, -1, "beta must be finite and not negative", run(beta=float("nan")))
        attempt(bare, -1, "beta must be finite and not negative", lambda ctx, pos, ll, s, t: ctx.eslice_step(key, float("inf"), pos, ll, s))
        attempt(bare, -1, "must divide n_steps", run(n=4, thin=3))
        attempt(bare, -1, "n_steps must be at least 1", run(n=0))
        attempt(bare, -1, "key_mode 1 needs d_keys", lambda ctx, pos, ll, s, t: ctx.eslice_run(None, 1.0, 4, pos, ll, subiter_sum=s, key_mode=1))
        attempt(bare, -1, "null device pointer", lambda ctx, pos, ll, s, t: ctx.eslice_run(key, 1.0, 4, pos, None, subiter_sum=s))
        pos, ll = _state(bare, x0)
        bare.eslice_run(key, 1.0, 2, pos, ll)                                       # ... and the context still serves
        bare.set_target(_lib.LGCP, gu.target_block(ec.dist_of(c.n))[1])            # a new target removes the factor
        attempt(bare, -5, "mfm_set_lgcp_chol has not been called", step)
    finally:
        bare.close()
    # n_chain_local % 16: no such context exists -- mfm_create refuses it, so the tile kernels never see a partial tile
    with pytest.raises(_lib.MfmError, match="multiple of 16"):
        gu.make_ctx(ec.dist_of(c.n), _args(c.d, 24), n_local=24)


def test_python_layers():
    """elliptical_slice(...).step, .step.run, inference_loop0 on it: the same bits as the context calls."""
    import torch
    from mfm_amd import distributions as D, mcmc_utils, random as jr
    from mfm_amd.bblackjax.mcmc.elliptical_slice import EllipSliceInfo, EllipSliceRunInfo, EllipSliceState, elliptical_slice
    from mfm_amd.engine import Engine
    c = ec.BY_NAME["4x4"]
    args = _args(c.d, c.B)
    args.ot_cond_flow = False
    dist = D.LogGaussianCoxPines(c.d)
    eng = Engine(dist, args, None)
    try:
        beta = 0.5
        algo = elliptical_slice(lambda x: beta * dist.loglik(x))
        pos0 = _dev(ec.start_of("4x4"), torch.float32)
        st0 = algo.init(pos0)
        assert isinstance(st0, EllipSliceState) and st0.logdensity.dtype == torch.float64 and st0.logdensity_grad is None
        key = jr.PRNGKey(31)
        st1, info1 = algo.step(key, st0)
        assert isinstance(info1, EllipSliceInfo) and info1.momentum.shape == (c.B, c.d) and info1.theta.shape == (c.B,) and (info1.subiter >= 1).all()
        assert torch.equal(st0.position, pos0)                                  # functional: the input state is not modified
        pos, ll = pos0.clone(), st0.logdensity.clone()
        eng.ctx.eslice_step(key, beta, pos, ll)
        assert torch.equal(st1.position, pos) and torch.equal(st1.logdensity, ll)
        ckeys = np.asarray(jr.split(jr.PRNGKey(32), c.B))
        stk, _ = algo.step(ckeys, st0)
        pos, ll = pos0.clone(), st0.logdensity.clone()
        eng.ctx.eslice_step_keys(_keys_dev(ckeys), beta, pos, ll)
        assert torch.equal(stk.position, pos)
        new, info = algo.step.run(key, st0, 6, thin=2)
        assert isinstance(info, EllipSliceRunInfo) and info.positions.shape == (3, c.B, c.d) and info.logdensities.shape == (3, c.B)
        assert info.mean_subiter.shape == (c.B,) and (info.mean_subiter >= 1).all() and info.num_capped.sum().item() == 0
        assert isinstance(info.last, EllipSliceInfo) and (info.max_subiter >= info.last.subiter).all()
        st = st0
        for j in range(6):
            st, last = algo.step(jr.split(key, 6)[j], st)
        assert torch.equal(new.position, st.position) and torch.equal(new.logdensity, st.logdensity) and torch.equal(info.last.subiter, last.subiter)
        assert torch.equal(info.positions[-1], new.position)
        states, linfo = mcmc_utils.inference_loop0(key, st0, algo.step, 6)       # picks up .run
        assert isinstance(states, EllipSliceState) and states.position.shape == (6, c.B, c.d) and states.logdensity_grad is None
        assert torch.equal(states.position[-1], new.position) and torch.equal(states.position[1], info.positions[0])
        assert torch.equal(linfo.num_capped, info.num_capped)
    finally:
        eng.close()


def test_do_eslice_end_to_end_on_the_8x8_grid(caplog):
    import logging
    from mfm_amd import exe_others as X, multi_modal as M, wandb_shim
    from mfm_amd.distributions import LogGaussianCoxPines
    args = M.build_parser().parse_args(["--example", "pines", "--num_chain", "32", "--learning_iter", "6", "--eval_iter", "4", "--seed", "1",
                                        "--do_eslice", "--hidden_x", "32", "32", "--hidden_t", "32", "32", "--hidden_xt", "32", "32", "--fourier_dim", "16"])
    args.dim, args.lim, args.step_size = 64, None, 0.01                        # multi_modal.main: the pines example at --force_dim 64
    dist = LogGaussianCoxPines(64)
    logged = {}
    orig = wandb_shim.log
    wandb_shim.log = lambda d, *a, **k: logged.update(d)
    try:
        with caplog.at_level(logging.INFO, logger="mfm_amd.exe_others"):
            res, res_, extras = X.run(dist, args, None, return_extras=True)
    finally:
        wandb_shim.log = orig
    try:
        print("do_eslice: res", res, "stats", extras["stats"])
        assert res.shape == (5,) and np.isfinite(res).all() and np.array_equal(res, res_)
        assert extras["samples"].shape == (4 * 32, 64)
        for k in ("eslice_mean_subiter", "eslice_max_subiter", "eslice_capped", "rhat_max", "ess_multichain_per_step_min", "ess_multichain_per_step_median",
                  "ess_multichain_per_step_mean", "ess_multichain_per_eval_min", "ess_multichain_per_eval_median", "ess_multichain_per_eval_mean",
                  "train_time", "logpdf"):
            assert k in logged, k
        assert logged["eslice_capped"] == 0 and 1.0 <= logged["eslice_mean_subiter"] <= logged["eslice_max_subiter"] < 64
        assert any("Likelihood evaluations per transition" in m for m in caplog.messages)
    finally:
        extras["engine"].close()
