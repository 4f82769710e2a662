"""GPU parity of the wide family's layer GEMM (mfm_amd/csrc/wide.hip: launch_gemm) on EVERY instance its dispatch can choose, at the
shapes where each instance's guards, clamps and forks are live (case table and what each network is for: tests/wide_gemm_cases.py).

Every case asserts through mfm_wide_gemm_tally -- a host-side count kept where launch_gemm launches -- that the instances it is named
for ran, and pins the plan of the shapes it exists for through mfm_wide_gemm_plan (the function launch_gemm launches from): a case
that stops reaching its instance fails.  All comparisons are float32 kernels against the float64 oracle on the same float32-rounded
inputs, at the project's own tolerances for the same quantities:

    loss 2e-5 relative; every gradient tensor 3e-4 of its maximum; field and JVP 3e-5 of the maximum (tests/test_gpu_wide.py,
    tests/test_gpu_activations.py); fixed-step solves: tests/test_gpu_fixed_families.py; prescribed-step solves: tests/test_gpu_depth.py;
    the Cox process MALA: tests/test_gpu_lgcp_ragged.py.

Measured maxima (MI355X) are recorded at the assertions.  No kernel change was needed: every instance met every bound, and the
switch arms agree bit for bit.

Sensitivity, measured once on an MI355X with two libraries built for the purpose, each with one planted error that keeps every access
in bounds: (1) gemm_lds_kernel accumulates the tangent over all K steps instead of the first NST (`tt = DUAL`): 17 of the 40 cases fail
-- every parity case whose joint layer runs the dual LDS kernel (Q, A, X, M4 from 528 rows, W), JVP off by 2.1e-4 .. 2.0e-3 against
the bound of 3e-5; the four bit-equality cases with an LDS arm (up to 129,023 differing JVP words); the W time batch and the compacting
A solve through their log-dets.  (2) gemm_kernel's one-block path multiplies the tangent for every K block instead of the first KBT: 14
cases fail -- all eight R cases and both M cases (JVP off by 1.2e-3 .. 2.8e-3), the three R time batches and the compacting R solve;
the R bit-equality case passes, as it must: every arm then runs the same wrong path, which is why equality is asserted beside parity
and not instead of it."""
import functools

import numpy as np
import pytest

from oracle import fm, mala, ode, prng, targets
from tests.wide_gemm_cases import ALL_SWITCHES, ARMS, EQUALITY, NETS, PARITY, TALL

pytestmark = pytest.mark.gpu


def _dev(x, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def _relerr(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


@functools.lru_cache(maxsize=4)
def _net(name, B, act, **kw):
    """(args, dist, model) of a case's phi-four network: computed once per shape and left unchanged."""
    from tests import gpu_util as gu
    d, F, hidden = NETS[name]
    args, dist, k, model, state = gu.phi4_setup(d=d, B=B, hidden=hidden, F=F, non_linearity=act, **dict(kw))
    return args, dist, model


def _wide_ctx(dist, args, model, params, monkeypatch=None, switches=()):
    """A FAMILY_WIDE context under exactly the named development switches (latched at mfm_create)."""
    from mfm_amd import _lib
    from tests import gpu_util as gu
    if monkeypatch is not None:
        for s in ALL_SWITCHES:
            monkeypatch.delenv(s, raising=False)
        for s in switches:
            monkeypatch.setenv(s, "1")
    ctx = gu.make_ctx(dist, args, fourier=model.f, params=params, family=_lib.FAMILY_WIDE)
    assert ctx.cfg.kernel_family == _lib.FAMILY_WIDE
    assert not any(ctx.wide_gemm_tally().values())                  # a fresh context has launched nothing
    return ctx


def _ran(tally):
    return {k for k, v in tally.items() if v > 0}


def _inputs(dist, B, d):
    rng = np.random.default_rng(1)
    x32 = dist.init_params.astype(np.float32)
    return x32, rng.uniform(0, 1, B).astype(np.float32), rng.standard_normal((B, d)).astype(np.float32)


def _device_results(ctx, x32, t, z, key):
    """Field without a tangent, field + JVP, loss + gradient: the three calls of a parity case, with the tally of each."""
    import torch
    B, d = x32.shape
    out = {}
    v2 = torch.full((B, d), float("nan"), device="cuda")
    ctx.wide_gemm_tally(reset=True)
    ctx.vf_apply(_dev(x32), _dev(t), v2)
    out["tally_field"] = ctx.wide_gemm_tally(reset=True)
    v = torch.full((B, d), float("nan"), device="cuda"); jv = torch.full((B, d), float("nan"), device="cuda")
    ctx.vf_apply(_dev(x32), _dev(t), v, _dev(z), jv)
    out["tally_jvp"] = ctx.wide_gemm_tally(reset=True)
    loss = torch.zeros(1, dtype=torch.float64, device="cuda"); grads = torch.full((ctx.n_params,), float("nan"), device="cuda")
    ctx.fm_loss_grad(key, _dev(x32), loss, grads)
    out["tally_grad"] = ctx.wide_gemm_tally(reset=True)
    out.update(v2=v2.cpu().numpy(), v=v.cpu().numpy(), jv=jv.cpu().numpy(), loss=loss.item(), grads=grads.cpu().numpy())
    return out


@pytest.mark.parametrize("name,rows,act,named,pins", PARITY, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in PARITY])
def test_every_instance_matches_the_oracle_at_its_boundary_shapes(monkeypatch, name, rows, act, named, pins):
    """Field (non-dual forward GEMMs), field + JVP (dual GEMMs, the TS path of x1), loss and every gradient tensor (backward GEMMs with
    mask / add, the pre-activation copy P, wide::wgrad_kernel) at `rows` rows.

    Measured over the 24 cases (MI355X), against bounds of 3e-5 / 3e-5 / 2e-5 / 3e-4: field <= 6.9e-7 (Q, d = 192 > 128 with the clipped
    target gradient: 3.3e-6 .. 5.7e-6), JVP <= 7.6e-7, loss <= 1.1e-7, worst gradient tensor <= 1.5e-6 (W at 16384 rows: 4.9e-6)."""
    from mfm_amd import _lib
    from tests import gpu_util as gu
    for shape, want in pins:
        assert _lib.wide_gemm_plan(*shape)[:3] == want, (shape, _lib.wide_gemm_plan(*shape))
    args, dist, model = _net(name, rows, act)
    d = args.dim
    params = gu.rand_params(model, seed=3)
    ctx = _wide_ctx(dist, args, model, params, monkeypatch)
    x32, t, z = _inputs(dist, rows, d)
    key = prng.PRNGKey(11)
    r = _device_results(ctx, x32, t, z, key)
    ctx.close()
    # the instances the case is named for ran: non-dual ones without a tangent and in the training pass, dual ones with the tangent
    ran = _ran(r["tally_field"]) | _ran(r["tally_jvp"]) | _ran(r["tally_grad"])
    print(f"{name} rows={rows} {act}: field {r['tally_field']}, jvp {r['tally_jvp']}, grad {r['tally_grad']}")
    assert set(named) <= ran, (named, ran)
    assert not any(k.endswith("_dual") for k in _ran(r["tally_field"]) | _ran(r["tally_grad"]))
    assert {k for k in named if k.endswith("_dual")} <= _ran(r["tally_jvp"])
    assert {k for k in named if not k.endswith("_dual")} <= _ran(r["tally_grad"]) & _ran(r["tally_field"])
    assert not ran & {"22_ring8", "22_ring8_dual", "lds_wm1", "lds_wm1_dual"}           # those run only under their switches
    if rows <= 256:
        assert ran <= {"11", "11_dual"}
    elif rows <= 512:
        assert ran <= {"12", "12_dual"}
    else:
        assert not ran & {"11", "11_dual", "12", "12_dual"}
    # oracle
    v_o, jv_o = model.forward(params, x32.astype(np.float64), t.astype(np.float64), tangent=z.astype(np.float64))
    loss_o, grads_o = fm.loss_and_grad(model, params, key, x32.astype(np.float64), args.sigma)
    g = gu.unflat_params(model, r["grads"])
    e_g = [(_relerr(gg[kk], go[kk].astype(np.float64)), i, kk) for i, (gg, go) in enumerate(zip(g, grads_o)) for kk in ("kernel", "bias")]
    e_v2, e_v, e_jv, e_l = _relerr(r["v2"], v_o), _relerr(r["v"], v_o), _relerr(r["jv"], jv_o), abs(r["loss"] - loss_o) / abs(loss_o)
    print(f"   field alone {e_v2:.2e}, field {e_v:.2e}, JVP {e_jv:.2e}, loss {e_l:.2e}, worst gradient tensor {max(e_g)[0]:.2e} (layer {max(e_g)[1]} {max(e_g)[2]})")
    assert np.isfinite(r["v2"]).all() and np.isfinite(r["v"]).all() and np.isfinite(r["jv"]).all()      # every element is written
    assert np.isfinite(r["grads"]).all()
    assert e_v2 < 3e-5 and e_v < 3e-5, (e_v2, e_v)             # measured <= 5.7e-6
    assert e_jv < 3e-5, e_jv                                   # measured <= 7.6e-7
    assert e_l <= 2e-5, (r["loss"], loss_o)                    # measured <= 1.1e-7
    assert max(e_g)[0] < 3e-4, max(e_g)                        # measured <= 4.9e-6


@pytest.mark.parametrize("name,rows,act,min_distinct", EQUALITY, ids=[f"{c[0]}-{c[1]}" for c in EQUALITY])
def test_all_instances_give_bit_identical_results(monkeypatch, name, rows, act, min_distinct):
    """Every instance accumulates an output element in ONE MFMA chain, K blocks ascending and the four k-sub-steps of a block ascending,
    from a zero accumulator, and the epilogue is shared code: read from the kernels, the same inputs give the same bits whatever instance
    runs.  One context per switch arm; field, JVP, loss and gradient must be equal bit for bit, and the tallies must show that the arms
    ran different instances.  Measured (MI355X): equal in every bit on all five shapes and all six arms."""
    from tests import gpu_util as gu
    args, dist, model = _net(name, rows, act)
    params = gu.rand_params(model, seed=3)
    x32, t, z = _inputs(dist, rows, args.dim)
    res = {}
    for arm, switches in ARMS.items():
        ctx = _wide_ctx(dist, args, model, params, monkeypatch, switches)
        res[arm] = _device_results(ctx, x32, t, z, prng.PRNGKey(11))
        ctx.close()
    ran = {arm: frozenset(_ran(r["tally_field"]) | _ran(r["tally_jvp"]) | _ran(r["tally_grad"])) for arm, r in res.items()}
    for arm in ARMS:
        print(f"{name} rows={rows} arm {arm}: {sorted(ran[arm])}")
    base = res["default"]
    assert np.isfinite(base["grads"]).all() and np.abs(base["jv"]).max() > 0
    for arm, r in res.items():
        for q in ("v2", "v", "jv", "grads"):
            a, b = base[q].view(np.uint32), r[q].view(np.uint32)
            assert np.array_equal(a, b), (arm, q, int((a != b).sum()), float(np.abs(base[q] - r[q]).max()))
        assert r["loss"] == base["loss"], (arm, r["loss"], base["loss"])
    # the arms ran what they are named for
    lds_any = {"lds", "lds_dual", "lds_wm1", "lds_wm1_dual"}
    for arm in ("nolds", "nolds_no_small", "nolds_ring8"):
        assert not ran[arm] & lds_any, (arm, ran[arm])
    assert not ran["wm1"] & {"lds", "lds_dual"}
    assert {k.replace("lds", "lds_wm1") for k in ran["default"] & {"lds", "lds_dual"}} <= ran["wm1"]
    for arm in ARMS:
        if arm != "nolds_ring8":
            assert not ran[arm] & {"22_ring8", "22_ring8_dual"}, (arm, ran[arm])
        if arm != "wm1":
            assert not ran[arm] & {"lds_wm1", "lds_wm1_dual"}, (arm, ran[arm])
    if rows <= 512:
        assert ran["default"] <= {"11", "11_dual", "12", "12_dual"} and ran["no_small"] <= {"22", "22_dual"}
    if name in ("Q", "A", "X"):
        assert "22_ring8" in ran["nolds_ring8"] and ran["default"] & {"lds", "lds_dual"}
    if name in ("A", "X"):
        assert "22_ring8_dual" in ran["nolds_ring8"] and "lds_wm1_dual" in ran["wm1"]
    assert len(set(ran.values())) >= min_distinct, ran


# ---- the tall time batch of the solvers: 5 x rows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,named", TALL, ids=[f"{c[0]}-{c[1]}" for c in TALL])
def test_the_tall_time_batch_of_a_fixed_step_solve(monkeypatch, name, B, named):
    """Four RK4 steps in both directions: a launch sequence known in advance and no controller.  The time branch (t1, t2, gate) runs on 5 B
    rows -- 240 (<1,1>), 320 (<1,2>), 560 (<2,2> one block at a time; the LDS kernel with a 48-row last tile) and 16400 ("big": MT = 1025, the
    last workgroup row holds one tile of eight) -- while the x branch runs on B.  Bounds: tests/test_gpu_fixed_families.py (outputs 3e-5, log-det
    q90 2e-5 and max 1e-3 with ReLU / 5e-5 with tanh, of max(1, |l|)).  Measured (MI355X): |dy| <= 2.9e-7, |dl| q90 <= 6.1e-7, max <= 1.5e-6 at
    |l| 1.5 .. 6.5."""
    from mfm_amd import _lib
    from tests.test_gpu_fixed_families import _check_transforms, _tamed
    act = "relu" if 5 * B <= 560 else "tanh"
    args, dist, model = _net(name, B, act, ode_method="rk4", ode_steps=4)
    params = _tamed(model, 9, 0.5, 1e-3)
    ctx = _wide_ctx(dist, args, model, params, monkeypatch)
    d, F, hidden = NETS[name]
    h = hidden if isinstance(hidden, int) else hidden[1][0]
    plan_t1 = _lib.wide_gemm_plan(5 * B, (2 * F + 15) // 16, (h + 15) // 16)
    assert plan_t1[0] == named[0], plan_t1
    try:
        _check_transforms(ctx, model, params, dist.init_params.astype(np.float32), True, "rk4", 4, f"tall time batch {name} B = {B}", kink=(act == "relu"))
        tally = ctx.wide_gemm_tally()
    finally:
        ctx.close()
    ran = _ran(tally)
    print(f"tall time batch {name} B = {B}: {tally}")
    assert set(named) <= ran, (named, ran)
    if 5 * B <= 256:
        assert ran <= {"11", "11_dual"}, ran                     # 240 rows stay on the 32 x 32 tile


# ---- compaction: a solve whose live row count shrinks through 512 and 256 ------------------------------------------------------------------
COMPACT_KEY = {"R": 21, "A": 21}


def _live_rows(n_att):
    """Rows of attempt j's evaluations: every row until the first chain has finished, then ceil16 of the chains still integrating."""
    B = len(n_att)
    live = [int((n_att > j).sum()) for j in range(int(n_att.max()))]
    return [B if l == B else (l + 15) // 16 * 16 for l in live]


@pytest.mark.parametrize("name", ["R", "A"])
def test_a_compacting_solve_walks_through_the_row_thresholds(monkeypatch, name):
    """One adaptive transform of 528 chains on the oracle's step sequence (tests/test_gpu_depth.py: test_transform_on_prescribed_steps_matches_
    oracle): the chains end after different numbers of attempts, the evaluations run on ceil16(live) rows, and the x branch passes from
    the large branch (<2,2> for R, the LDS kernel for A) through <1,2> to <1,1> inside one solve.  Attempt counts exact; outputs and
    log-det at that test's bounds (3e-5 of max(1, |y|), 1e-4 of max(1, |l|)).  The oracle alone: 15 .. 60 (R) and 14 .. 60 (A) attempts per
    chain, so the evaluations run on 528, then 512 .. 272, then 256 .. 16 rows.  Measured (MI355X): |dy| 3.5e-6 / 4.0e-6, |dl| 2.3e-6 of |l| 2.8 /
    7.4e-6 of |l| 7.9."""
    import torch
    from tests.test_gpu_fixed_families import _tamed
    from tests.test_gpu_replay import _replay_arrays
    B = 528
    args, dist, model = _net(name, B, "relu")
    d = args.dim
    params = _tamed(model, 9, 0.5, 1e-3)
    x64 = dist.init_params.astype(np.float32).astype(np.float64)
    keys = prng.split(prng.PRNGKey(COMPACT_KEY[name]), B)
    o = (True, args.rtol, args.atol, args.mxstep)
    st = {}
    ode.transform_and_logdet(model, params, keys, x64, *o, stats=st)
    rows_seen = _live_rows(st["n_attempted"])
    print(f"compaction {name}: attempts {st['n_attempted'].min()} .. {st['n_attempted'].max()}, rows per attempt {rows_seen}")
    # from the oracle alone: the solve passes through all three row classes
    assert rows_seen[0] == B and any(256 < r <= 512 for r in rows_seen) and any(0 < r <= 256 for r in rows_seen), rows_seen
    dt, acc = _replay_arrays([st])
    st_o = {}
    y_o, l_o = ode.transform_and_logdet(model, params, keys, x64, *o, stats=st_o, replay=dict(dt=dt[0].astype(np.float64), acc=acc[0]))
    ctx = _wide_ctx(dist, args, model, params, monkeypatch)
    ratio = torch.zeros(dt[0].shape, device="cuda"); own = torch.zeros(dt[0].shape, device="cuda")
    ctx.debug_replay(_dev(dt[0]), _dev(acc[0]), ratio, own)
    out = torch.empty(B, d, device="cuda"); ldj = torch.empty(B, device="cuda"); ns = torch.empty(B, dtype=torch.int32, device="cuda")
    ctx.ode_transform(1, _dev(x64.astype(np.float32)), out, ldj, keys=_dev(keys.astype(np.uint32).view(np.int32)), nsteps=ns)
    y, l, n = out.cpu().numpy(), ldj.cpu().numpy(), ns.cpu().numpy()
    tally = ctx.wide_gemm_tally()
    ctx.close()
    ey, el, ls = np.abs(y - y_o).max(), np.abs(l - l_o), max(1.0, np.abs(l_o).max())
    print(f"   |dx| {np.abs(y_o - x64).max():.2f}, |dy| {ey:.2e}, |dl| max {el.max():.2e} (|l| {np.abs(l_o).max():.2f}); tally {tally}")
    np.testing.assert_array_equal(n, st["n_attempted"])
    # the dual instances run only in the x branch, on ceil16(live) rows: all three row classes were launched
    big = "22_dual" if name == "R" else "lds_dual"
    assert {big, "12_dual", "11_dual"} <= _ran(tally), tally
    assert st["n_attempted"].mean() > 6 and np.abs(l_o).max() > 0.02
    assert ey < 3e-5 * max(1.0, np.abs(y_o).max()), ey
    assert el.max() < 1e-4 * ls, (el.max(), ls)


# ---- the K^-1 product of the Cox process: KB = NT = 34 ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _lgcp23(B):
    from tests import gpu_util as gu
    return gu.lgcp_setup(n=23, B=B, hidden=32, F=16)


@pytest.mark.parametrize("B,named", [(48, ()), (144, ("11",)), (528, ("22",))])
def test_kinv_gemm_in_the_mala_step_matches_oracle(monkeypatch, B, named):
    """23 x 23 grid (d = 529, dp = 544: KB = NT = 34, the one-block K path, 15 zero pad columns): one MALA init and two steps against the
    oracle at the bounds of tests/test_gpu_lgcp_ragged.py.  From 128 chains on a wide-family context sends the K^-1 contraction through
    launch_gemm (api.hip: lgcp_mala_dispatch): 144 chains on <1,1,false>, 528 on <2,2,false>.  Below 128 chains the dispatch keeps the
    fused tile kernel even in a wide context -- 48 chains launch no GEMM at all, which the tally states.  Measured (MI355X, the three chain
    counts): init |dlogp| <= 7.2e-5 at |logp| ~ 600, |dgrad| <= 3.1e-6; steps |dprop| <= 4.8e-7, |dp| <= 6.8e-5, |dlogp| <= 7.1e-5, |dgrad| <= 6.5e-6."""
    import torch
    from mfm_amd import _lib
    from tests.test_gpu_lgcp_ragged import STEP, _step_keys
    n, d, beta = 23, 529, 1.0
    args, dist, k, model, state = _lgcp23(B)
    ctx = _wide_ctx(dist, args, model, None, monkeypatch)
    if named:
        assert _lib.wide_gemm_plan((B + 15) // 16 * 16, 34, 34)[0] == named[0]
    x32 = dist.init_params.astype(np.float32)
    vg = targets.Tempered(dist, beta).value_and_grad
    st = mala.init(x32.astype(np.float64), vg)
    pos, logp, grad = _dev(x32), torch.empty(B, dtype=torch.float64, device="cuda"), torch.empty(B, d, device="cuda")
    ctx.mala_init(pos, beta, logp, grad)
    lp0, g0 = logp.cpu().numpy(), grad.cpu().numpy()
    print(f"K^-1 B={B}: init |dlogp| {np.abs(lp0 - st.logdensity).max():.2e} (|logp| {np.abs(st.logdensity).max():.0f}), |dgrad| {np.abs(g0 - st.logdensity_grad).max():.2e}")
    np.testing.assert_allclose(lp0, st.logdensity, rtol=2e-6, atol=1e-3)
    np.testing.assert_allclose(g0, st.logdensity_grad, rtol=2e-5, atol=2e-3)
    n_acc = 0
    for j in range(2):
        kj, keys = _step_keys(n, B, j, False)
        st_in = mala.MALAState(pos.cpu().numpy().astype(np.float64), logp.cpu().numpy(), grad.cpu().numpy().astype(np.float64))
        new, info, u = mala.kernel(keys, st_in, vg, STEP[n])
        acc = torch.empty(B, device="cuda"); isacc = torch.empty(B, dtype=torch.uint8, device="cuda"); prop = torch.empty(B, d, device="cuda")
        ctx.mala_step(kj, beta, STEP[n], pos, logp, grad, acc, isacc, prop)
        ia = isacc.cpu().numpy().astype(bool)
        decided = np.abs(u - info.acceptance_rate) > 1e-2
        same = ia == info.is_accepted
        n_acc += int(info.is_accepted.sum())
        print(f"   step {j}: oracle accepts {info.is_accepted.sum()}/{B}, borderline {(~decided).sum()}, |dprop| {np.abs(prop.cpu().numpy() - info.proposed_position).max():.2e}, "
              f"|dp| {np.abs(acc.cpu().numpy() - info.acceptance_rate).max():.2e}, |dlogp| {np.abs(logp.cpu().numpy() - new.logdensity)[same].max():.2e}, "
              f"|dgrad| {np.abs(grad.cpu().numpy() - new.logdensity_grad)[same].max():.2e}")
        np.testing.assert_allclose(prop.cpu().numpy(), info.proposed_position, rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(acc.cpu().numpy(), info.acceptance_rate, rtol=5e-3, atol=5e-3)
        np.testing.assert_array_equal(ia[decided], info.is_accepted[decided])
        assert (~decided).sum() <= 0.1 * B
        np.testing.assert_allclose(pos.cpu().numpy()[same], new.position[same], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(logp.cpu().numpy()[same], new.logdensity[same], rtol=2e-6, atol=2e-3)
        np.testing.assert_allclose(grad.cpu().numpy()[same], new.logdensity_grad[same], rtol=3e-5, atol=3e-3)
    assert 0 < n_acc < 2 * B                                      # both decisions were compared
    tally = ctx.wide_gemm_tally()
    ctx.close()
    print(f"   tally {tally}")
    if named:
        assert _ran(tally) == set(named) and tally[named[0]] == 3, tally          # one K^-1 product per launch: init and two steps
    else:
        assert not _ran(tally), tally


def test_kinv_gemm_on_the_big_tile_matches_oracle(monkeypatch):
    """7712 chains: MT NT = 482 x 34 = 16388 >= 16384 and KB = 34 is no multiple of 8, so the K^-1 product of the init runs on
    gemm_kernel<4,2,false> (the reference's default d = 1600 gets there at 2624 chains): NT = 34 leaves the second wave column of the
    last workgroup column empty, MT = 482 two live tiles of eight in the last workgroup row.  The kernel runs all 7712 chains; the
    float64 oracle (17 MFLOP per chain) checks the first, middle and last 64.  Measured (MI355X): |dlogp| 6.9e-5 at |logp| 607, |dgrad| 3.2e-6
    at |grad| 71."""
    import torch
    from mfm_amd import _lib
    B, d, beta = 7712, 529, 1.0
    assert _lib.wide_gemm_plan(B, 34, 34)[:3] == ("big", 9, 61) and _lib.wide_gemm_plan(B - 16, 34, 34)[0] == "22"
    args, dist, k, model, state = _lgcp23(B)
    ctx = _wide_ctx(dist, args, model, None, monkeypatch)
    x32 = dist.init_params.astype(np.float32)
    pos, logp, grad = _dev(x32), torch.full((B,), float("nan"), dtype=torch.float64, device="cuda"), torch.full((B, d), float("nan"), device="cuda")
    ctx.mala_init(pos, beta, logp, grad)
    lp, g = logp.cpu().numpy(), grad.cpu().numpy()
    tally = ctx.wide_gemm_tally()
    ctx.close()
    assert _ran(tally) == {"big"} and tally["big"] == 1, tally
    assert np.isfinite(lp).all() and np.isfinite(g).all()          # every chain of the 7712 is written
    idx = np.concatenate([np.arange(64), B // 2 - 32 + np.arange(64), B - 64 + np.arange(64)])
    st = mala.init(x32[idx].astype(np.float64), targets.Tempered(dist, beta).value_and_grad)
    print(f"K^-1 big tile: |dlogp| {np.abs(lp[idx] - st.logdensity).max():.2e} (|logp| {np.abs(st.logdensity).max():.0f}), |dgrad| {np.abs(g[idx] - st.logdensity_grad).max():.2e} "
          f"(|grad| {np.abs(st.logdensity_grad).max():.1f})")
    np.testing.assert_allclose(lp[idx], st.logdensity, rtol=2e-6, atol=1e-3)
    np.testing.assert_allclose(g[idx], st.logdensity_grad, rtol=2e-5, atol=2e-3)
