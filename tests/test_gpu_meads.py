"""GPU tests of ``mfm_meads_warmup`` (mfm_amd/csrc/ghmc.hip), ``bblackjax.meads_adaptation`` and ``--mcmc_kernel ghmc --adapt_steps``.

A warmup is ONE call, so the states between its iterations are not seen.  They are recovered by REPLAY: from the same start, iteration
t is one ``mfm_ghmc_step_keys`` launch per fold on the run's keys with the eps / alpha / delta / minv the trace says that fold used; the
replayed state after the last iteration must equal the warmup's bit for bit (and so must every fold's mean acceptance rate up to its
float32 storage).  That proves the transition and the bookkeeping (folds, roll, keys, shuffles, padding rows).  The statistics are then
checked against tests/meads_ref.py on the replayed states -- each iteration's from the device's own state before it -- within
``meads_cases.TOLERANCE``."""
import numpy as np
import pytest

from oracle import prng
from tests import ghmc_cases as gc
from tests import meads_cases as mc
from tests import meads_ref as ref

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _keys_dev(keys):
    return _dev(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32))


def _ctx(case, n_total=None):
    from mfm_amd import _lib
    from tests import gpu_util as gu
    tc, B = mc.target(case), mc.shape(case)[0]
    ctx = _lib.Context(dim=mc.dim(case), n_chain_local=B, n_chain_total=n_total or B, fourier_dim=16, hidden_t=(16, 16), hidden_x=(16, 16),
                       hidden_xt=(16, 16))
    if tc == "gmm4":
        ctx.set_target(*gu.target_block(gc.oracle_dist(tc)))
    else:
        ctx.set_target(_lib.PHI4, gc.block(tc) or [gc.A, gc.TBETA])
    return ctx


def _start(ctx, case):
    import torch
    pos = _dev(mc.start_state(case))
    B, d = pos.shape
    logp = torch.empty(B, dtype=torch.float64, device="cuda"); grad = torch.empty_like(pos)
    mom = torch.empty(B, d, dtype=torch.float64, device="cuda"); s = torch.empty(B, dtype=torch.float64, device="cuda")
    ctx.mala_init(pos, 1.0, logp, grad)
    ctx.ghmc_init(mc.init_key(case), mom, s)
    return pos, logp, grad, mom, s


def _warmup(ctx, case, state0, key=None):
    import torch
    B, n_valid, K, S, n_iter, step0, alpha0 = mc.shape(case)
    st = tuple(t.clone() for t in state0)
    d = st[0].shape[1]
    perms = mc.permutations(case)
    trace = torch.full((n_iter, K, 6), float("nan"), dtype=torch.float64, device="cuda")
    mass = torch.full((n_iter, K, d), float("nan"), dtype=torch.float64, device="cuda")
    minv = torch.empty(d, dtype=torch.float64, device="cuda")
    res = ctx.meads_warmup(mc.run_key(case) if key is None else key, 1.0, step0, alpha0, n_iter, *st, n_folds=K, n_valid=n_valid, shuffle_every=S,
                           perms=_dev(perms) if len(perms) else None, inverse_mass_out=minv, trace=trace, mass_trace=mass)
    return st, res, minv.cpu().numpy(), trace.cpu().numpy(), mass.cpu().numpy()


def _replay(ctx, case, state0, trace, mass, key=None):
    """Iteration by iteration with ``mfm_ghmc_step_keys`` and the traced parameters: the states before every iteration (numpy tuples, and
    the one after the last) and every iteration's per-chain acceptance rate."""
    import torch
    B, n_valid, K, S, n_iter, step0, alpha0 = mc.shape(case)
    m = n_valid // K
    perms = mc.permutations(case)
    key = mc.run_key(case) if key is None else key
    per_chain = np.ndim(key) == 2
    st = tuple(t.clone() for t in state0)
    acc = torch.empty(B, device="cuda")
    before, rates = [], []
    for t in range(1, n_iter + 1):
        before.append(tuple(x.cpu().numpy().copy() for x in st))
        perm = ref.perm_at(perms, t, S, n_valid)
        fold_of = np.zeros(B, np.int64)
        fold_of[perm] = np.arange(n_valid) // m
        keys = _keys_dev(prng.split_rows(key, n_iter)[:, t - 1] if per_chain else ref.step_keys(key, n_iter, t, B))
        new = tuple(x.clone() for x in st)
        rate = torch.empty(B, device="cuda")
        for f in range(K):
            tmp = tuple(x.clone() for x in st)
            ctx.ghmc_step_keys(keys, 1.0, trace[t - 1, f, 0], trace[t - 1, f, 1], trace[t - 1, f, 2], *tmp, _dev(mass[t - 1, f]), acc)
            rows = torch.as_tensor(np.flatnonzero(fold_of == f), device="cuda")
            for dst, src in zip(new, tmp):
                dst[rows] = src[rows]
            rate[rows] = acc[rows]
        st = new
        rates.append(rate.cpu().numpy().astype(np.float64))
    before.append(tuple(x.cpu().numpy().copy() for x in st))
    return before, np.stack(rates)


def _check_against_the_restatement(case, before, trace, mass, res, minv_out):
    """Every iteration's statistics from the device's own state before it."""
    B, n_valid, K, S, n_iter, step0, alpha0 = mc.shape(case)
    m = n_valid // K
    perms = mc.permutations(case)
    rz, ry, _ = mc.TOLERANCE[case]
    te, ta, td = mc.param_tolerance(case)
    par = ref.initial_params(K, mc.dim(case), step0, alpha0)
    worst = np.zeros(5)
    for t in range(1, n_iter + 1):
        x, _, g = (before[t - 1][q].astype(np.float64) for q in range(3))
        perm = ref.perm_at(perms, t, S, n_valid)
        with np.errstate(all="ignore"):
            stats = [ref.fold_stats(x[perm[f * m:(f + 1) * m]], g[perm[f * m:(f + 1) * m]], t) for f in range(K)]
        par = ref.roll(par, stats)
        for f in range(K):
            r = (f + 1) % K
            lz, ly = trace[t - 1, f, 3], trace[t - 1, f, 4]
            if not stats[f].usable:
                assert (case, t, r) in mc.KEPT and not (np.isfinite(lz) and np.isfinite(ly)), (case, t, f, lz, ly)
                prev = (step0, alpha0, alpha0 / 2) if t == 1 else tuple(trace[t - 2, r, :3])
                assert tuple(trace[t - 1, r, :3]) == prev                          # kept bit for bit
                np.testing.assert_array_equal(mass[t - 1, r], np.ones(mc.dim(case)) if t == 1 else mass[t - 2, r])
                continue
            err = np.array([abs(lz - stats[f].lam_z) / stats[f].lam_z, abs(ly - stats[f].lam_y) / stats[f].lam_y,
                            abs(trace[t - 1, r, 0] - par.eps[r]) / par.eps[r], abs(trace[t - 1, r, 1] - par.alpha[r]),
                            np.abs(mass[t - 1, r] / par.minv[r] - 1.0).max()])
            worst = np.maximum(worst, err)
            assert err[0] <= rz and err[1] <= ry and err[2] <= te and err[3] <= ta, (case, t, f, err, (rz, ry, te, ta))
            assert abs(trace[t - 1, r, 2] - par.delta[r]) <= td and trace[t - 1, r, 2] == trace[t - 1, r, 1] / 2
            assert err[4] <= 1e-12                                                  # sd^2: float64 sums of float32 positions
        # the reference continues from the device's parameters, not its own (a kept fold aside, they agree within the tolerance)
        par = ref.Params(trace[t - 1, :, 0].copy(), trace[t - 1, :, 1].copy(), trace[t - 1, :, 2].copy(), mass[t - 1].copy())
    x, _, g = (before[n_iter][q].astype(np.float64) for q in range(3))
    last = ref.fold_stats(x[:n_valid], g[:n_valid], n_iter + 1)
    print(f"{case}: worst rel lam_z {worst[0]:.3g} (tol {rz:.3g}), lam_y {worst[1]:.3g} (tol {ry:.3g}), eps {worst[2]:.3g} (tol {te:.3g}), "
          f"|alpha| {worst[3]:.3g} (tol {ta:.3g}), minv {worst[4]:.3g}; closing eps {res[0]:.6g} (ref {last.eps:.6g}), alpha {res[1]:.6g} (ref {last.alpha:.6g})")
    assert abs(res[0] - last.eps) <= te * last.eps and abs(res[1] - last.alpha) <= ta and res[2] == res[1] / 2
    np.testing.assert_allclose(minv_out, last.minv, rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", mc.CASES)
def test_warmup_replays_bit_for_bit_and_matches_the_restatement(case):
    """Measured on MI355X, worst relative error of lam(Z) / lam(Y) over iterations and folds (tolerances in tests/meads_cases.py):
    d320_k4 4.2e-7 / 2.6e-7; d1100_k4 9.8e-7 / 3.4e-7; d64_pbc_k4 1.5e-7 / 7.4e-8; d65_pbc_k4 1.3e-7 / 8.3e-8; 32x32_k4 4.4e-7 / 3.5e-7;
    d1025_pbc_k4 6.1e-7 / 2.6e-7; k6 1.9e-7 / 9.1e-8 -- 1e-4 to 5e-3 of the tolerances, which carry the worst-case float32 dot-product
    bound; inverse mass within 1e-12 and the replay bit for bit in every case."""
    B, n_valid, K, S, n_iter, step0, alpha0 = mc.shape(case)
    ctx = _ctx(case)
    state0 = _start(ctx, case)
    st, res, minv_out, trace, mass = _warmup(ctx, case, state0)
    assert np.isfinite(trace[:, :, :3]).all() and np.isfinite(trace[:, :, 5]).all() and np.isfinite(mass).all()
    before, rates = _replay(ctx, case, state0, trace, mass)
    for name, a, b in zip(("pos", "logp", "grad", "mom", "slice"), st, before[-1]):
        a = a.cpu().numpy()
        np.testing.assert_array_equal(a, b, err_msg=name)                          # (rows from n_valid on included: fold 0's parameters)
    assert not np.array_equal(before[0][0][:n_valid], before[-1][0][:n_valid])      # the chains moved
    m = n_valid // K
    perms = mc.permutations(case)
    for t in range(1, n_iter + 1):
        perm = ref.perm_at(perms, t, S, n_valid)
        for f in range(K):
            want = rates[t - 1][perm[f * m:(f + 1) * m]].mean()
            assert abs(trace[t - 1, f, 5] - want) <= 2.0 ** -23, (case, t, f)
    _check_against_the_restatement(case, before, trace, mass, res, minv_out)
    if case == "unstable":                                                          # fold 1 keeps step0 = 1 at t = 1 and rejects everything ...
        assert trace[0, 1, 0] == 1.0 and trace[0, 1, 5] == 0.0
        np.testing.assert_array_equal(before[1][0][8:], before[0][0][8:])
        assert trace[1, 1, 0] < 1.0 and trace[1:, 1, 5].min() > 0.5                # ... then recovers
    if case == "gmm4_k2":                                                           # alpha left the floor's value 1 - exp(-2 / t)
        t = n_iter
        assert np.abs(trace[t - 1, :, 1] - (1.0 - np.exp(-2.0 / t))).min() > 1e-3
        assert abs(trace[0, 0, 1] - (1.0 - np.exp(-2.0))) < 1e-12
    if case == "shuffle":
        assert len(perms) == 2
    ctx.close()


def test_chain_major_keys_no_trace_and_no_host_wait():
    """key_mode 1 replays with the chains' own keys; without trace buffers and ``read_result=False`` the state is the same bits."""
    import torch
    case = "k2"
    B, n_valid, K, S, n_iter, step0, alpha0 = mc.shape(case)
    ctx = _ctx(case)
    state0 = _start(ctx, case)
    keys = prng.split(prng.PRNGKey(77), B)
    st, res, minv_out, trace, mass = _warmup(ctx, case, state0, key=_keys_dev(keys))
    before, _ = _replay(ctx, case, state0, trace, mass, key=keys)
    for a, b in zip(st, before[-1]):
        np.testing.assert_array_equal(a.cpu().numpy(), b)
    bare = tuple(t.clone() for t in state0)
    minv = torch.empty(mc.dim(case), dtype=torch.float64, device="cuda")
    out = ctx.meads_warmup(_keys_dev(keys), 1.0, step0, alpha0, n_iter, *bare, n_folds=K, inverse_mass_out=minv, read_result=False)
    assert out is None
    for a, b in zip(bare, st):
        assert torch.equal(a, b)
    np.testing.assert_array_equal(minv.cpu().numpy(), minv_out)
    ctx.close()


def test_the_plan_and_the_gram_of_the_two_tile_case():
    """m = 80: two tiles per side, three tile pairs per fold and matrix; the off-diagonal pair must count twice -- the restatement's
    lam on the start state is met within the tolerance only if it does (half the cross terms would lose ~ (48 / 80) of the sum)."""
    from mfm_amd import _lib
    assert _lib.meads_plan(320, 4, 64) == (80, 128, 64, 2 * 4 * 3)
    assert _lib.meads_plan(32, 4, 65) == (8, 64, 96, 2 * 4 * 1)
    assert _lib.meads_plan(4096, 4, 256) == (1024, 1024, 256, 2 * 4 * 136)
    for bad in ((320, 1, 64), (321, 4, 64), (4, 4, 64), (320, 4, 0)):
        with pytest.raises(_lib.MfmError):
            _lib.meads_plan(*bad)


def test_refusals_and_their_order():
    import torch
    from mfm_amd import _lib
    from tests import gpu_util as gu
    case = "k2"
    B, n_valid, K, S, n_iter, step0, alpha0 = mc.shape(case)
    ctx = _ctx(case)
    state = _start(ctx, case)
    before = tuple(t.clone() for t in state)
    key = prng.PRNGKey(1)
    w = lambda *a, **k: ctx.meads_warmup(*a, **k)
    bad_calls = [
        ("null device pointer", lambda: w(key, 1.0, 0.1, 0.5, 4, state[0], state[1], state[2], None, state[4])),
        ("n_steps", lambda: w(key, 1.0, 0.1, 0.5, 0, *state)),
        ("d_keys", lambda: w(key, 1.0, 0.1, 0.5, 4, *state, key_mode=1)),
        ("step_size", lambda: w(key, 1.0, 0.0, 0.5, 4, *state)),
        ("alpha", lambda: w(key, 1.0, 0.1, 0.0, 4, *state)),
        ("alpha", lambda: w(key, 1.0, 0.1, 1.5, 4, *state)),
        ("n_folds", lambda: w(key, 1.0, 0.1, 0.5, 4, *state, n_folds=1)),
        ("multiple of n_folds", lambda: w(key, 1.0, 0.1, 0.5, 4, *state, n_folds=3)),
        ("multiple of n_folds", lambda: w(key, 1.0, 0.1, 0.5, 4, *state, n_folds=16)),          # m = 1
        ("multiple of n_folds", lambda: w(key, 1.0, 0.1, 0.5, 4, *state, n_folds=2, n_valid=32)),  # above n_chain_local
        ("shuffle_every", lambda: w(key, 1.0, 0.1, 0.5, 4, *state, n_folds=2, shuffle_every=-1)),
        ("d_perms", lambda: w(key, 1.0, 0.1, 0.5, 4, *state, n_folds=2, shuffle_every=2)),
        # the order: step_size before alpha before the folds
        ("step_size", lambda: w(key, 1.0, -1.0, 2.0, 4, *state, n_folds=1)),
        ("alpha", lambda: w(key, 1.0, 0.1, 2.0, 4, *state, n_folds=1)),
        ("n_folds", lambda: w(key, 1.0, 0.1, 0.5, 4, *state, n_folds=1, shuffle_every=-1)),
    ]
    for pattern, call in bad_calls:
        with pytest.raises(_lib.MfmError, match=pattern):
            call()
    for t, b in zip(state, before):
        assert torch.equal(t, b)                                                    # a rejected call touches nothing
    w(key, 1.0, 0.1, 0.5, 2, *state, n_folds=2, shuffle_every=2)                    # no shuffle falls inside 2 iterations: no buffer needed
    assert not torch.equal(state[3], before[3])
    ctx.close()
    shard = _ctx(case, n_total=2 * B)                                               # a shard is refused, after the parameter checks
    sstate = _start(shard, case)
    with pytest.raises(_lib.MfmError, match="alpha"):
        shard.meads_warmup(key, 1.0, 0.1, 0.0, 4, *sstate, n_folds=2)
    with pytest.raises(_lib.MfmError, match="error -?[0-9]+: the MEADS warmup serves one rank"):      # ... and ahead of the fold checks
        shard.meads_warmup(key, 1.0, 0.1, 0.5, 4, *sstate, n_folds=1)
    shard.close()
    args, dist, *_ = gu.lgcp_setup(n=4, B=16)
    cox = gu.make_ctx(dist, args)
    cstate = (_dev(dist.init_params.astype(np.float32)), torch.zeros(16, dtype=torch.float64, device="cuda"), torch.zeros(16, 16, device="cuda"),
              torch.zeros(16, 16, dtype=torch.float64, device="cuda"), torch.zeros(16, dtype=torch.float64, device="cuda"))
    with pytest.raises(_lib.MfmError, match="the HMC step serves the phi-four and mixture targets"):
        cox.meads_warmup(key, 1.0, 0.0, 0.5, 4, *cstate, n_folds=1)
    cox.close()


def test_meads_adaptation_and_ghmc_with_its_parameters():
    import torch
    from mfm_amd import distributions as D, random as jr
    from mfm_amd.bblackjax import ghmc, meads_adaptation
    from mfm_amd.bblackjax.mcmc.ghmc import GHMCState
    from mfm_amd.engine import Engine
    from tests import gpu_util as gu
    case = "shuffle"
    B, n_valid, K, S, n_iter, step0, alpha0 = mc.shape(case)
    args, odist, k, model, state = gu.phi4_setup(d=64, B=B, hidden=32, F=16)
    dist = D.PhiFour(64)
    args.ot_cond_flow = False
    eng = Engine(dist, args, model.f)
    warm = meads_adaptation(dist.logprob, num_folds=K, shuffle_every=S, initial_step_size=step0, initial_alpha=alpha0)
    key = jr.PRNGKey(5)
    pos = _dev(mc.start_state(case))
    (st, par), info = warm.run(key, pos, n_iter, keep_inverse_mass=True)
    assert isinstance(st, GHMCState) and set(par) == {"step_size", "alpha", "delta", "momentum_inverse_scale"}
    assert info.step_size.shape == (n_iter, K) and info.inverse_mass.shape == (n_iter, K, 64)
    # the same call on the context, with the driver's key split and its host-drawn permutations
    k_init, k_run, k_shuffle = jr.split(key, 3)
    raw = list(ghmc(dist.logprob, 0.1, 0.5).init(pos.clone(), k_init))
    raw = [raw[0].clone(), raw[2].clone(), raw[3].clone(), raw[1].clone(), raw[4].clone()]
    perms = _dev(ref.permutations(np.asarray(k_shuffle), n_iter, S, B))
    minv = torch.empty(64, dtype=torch.float64, device="cuda")
    res = eng.ctx.meads_warmup(k_run, 1.0, step0, alpha0, n_iter, *raw, n_folds=K, shuffle_every=S, perms=perms, inverse_mass_out=minv)
    assert (par["step_size"], par["alpha"], par["delta"]) == res
    assert torch.equal(st.position, raw[0]) and torch.equal(st.momentum, raw[3]) and torch.equal(par["momentum_inverse_scale"], minv.sqrt())
    algo = ghmc(dist.logprob, **par)
    s2, rinfo = algo.step.run(jr.PRNGKey(6), st, 50)
    rate = rinfo.acceptance_rate.mean().item()
    print(f"adapted step size {res[0]:.4g}, alpha {res[1]:.4g}; acceptance of 50 transitions with them {rate:.3f}")
    assert 0.3 < rate <= 1.0 and torch.isfinite(s2.position).all()
    with pytest.raises(ValueError, match="num_folds"):
        meads_adaptation(dist.logprob, num_folds=1)
    with pytest.raises(ValueError, match="multiple of num_folds"):
        meads_adaptation(dist.logprob, num_chains=18, num_folds=4)
    eng.close()


def test_training_loop_with_the_ghmc_kernel_and_the_meads_warmup():
    from mfm_amd import distributions as D, exe_flow_matching as E
    from oracle import loop
    kw = dict(example="phi-four", dim=64, num_chain=32, learning_iter=5, mcmc_per_flow_steps=4.0, hutchs=True, fourier_dim=16, seed=7, eval_iter=1,
              step_size=0.02, hidden_x=[32, 32], hidden_t=[32, 32], hidden_xt=[32, 32], ess_steps=16, adapt_steps=20)
    args = loop.default_args(mcmc_kernel="ghmc", ghmc_alpha=0.5, meads_folds=4, meads_shuffle=8, **kw)
    _, _, ex = E.run(D.PhiFour(64), args, None, log_every=1000, return_extras=True)
    for k in ("adapted_step_size", "adapted_alpha", "adapted_inverse_mass_min", "adapted_inverse_mass_max", "adapt_acceptance"):
        assert isinstance(ex[k], float) and np.isfinite(ex[k]), (k, ex.get(k))
    assert 0 < ex["adapted_step_size"] <= 1 and 0 < ex["adapted_alpha"] <= 1 and 0 < ex["adapted_inverse_mass_min"] <= ex["adapted_inverse_mass_max"]
    assert args.step_size == ex["adapted_step_size"] and args.ghmc_alpha == ex["adapted_alpha"] and args.ghmc_delta == args.ghmc_alpha / 2
    for s in ("min", "median", "mean"):
        assert np.isfinite(ex[f"ess_per_step_{s}"]) and ex[f"ess_per_grad_{s}"] == ex[f"ess_per_step_{s}"]      # one gradient per transition
    eng = ex["engine"]
    assert eng.ghmc_momentum is not None and eng.ghmc_momentum.shape == (eng.n_local, 64) and eng.ghmc_slice.abs().max().item() <= 1.0
    eng.close()
