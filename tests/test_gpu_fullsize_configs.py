"""The other BASELINE configurations at their FULL size, live against libmfm_ref (oracle/cref: the float64 C / OpenMP restatement, held to
the numpy oracle in tests/test_oracle_cref.py), as tests/test_gpu_fullsize.py does for the headline:

* configs[1], gaussian-mixture: d = 2, 4096 chains, K = 100, exact trace -- MALA, FM loss and gradient, the flow-MH step with each side's
  own controllers and on prescribed steps, the latter on every d = 2 tile (MFM_D2_TILE = 16 / 4 / 4s) and the automatic choice;
* configs[0], 4-mode: 512 chains, K = 10, n_ts = 5 -- the same four checks (the deterministic bound on the d = 2 solver the end-to-end
  test, tests/test_gpu_e2e.py, bounds only statistically);
* configs[4] per GPU, pines: d = 1024, 1024 chains, hidden 1024, --hutch -- MALA through the fused LGCP tile and FM loss and gradient
  through the wide family, all chains (its flow step stays on the 64-chain slices of tests/test_gpu_rank_slices.py: a float64 solve of
  1024 chains at hidden width 1024 takes the oracle minutes);
* the KSD / MMD pair kernels at configs[0]'s 51,200 samples and, for the KSD, above 131,072 samples (one column chunk per row tile).

Every configuration starts from the network of one full cycle of the product's own loop (tests/gpu_util.py: train_like_bench).  Each
bound is set from the measured error (printed); each test also replays the oracle with ONE PLANTED ERROR (a JVP of the exact trace
dropped, a mixture component dropped, mu of the K^-1 term shifted by 1e-3, the U-statistic without its diagonal removed) and requires
the device to miss it by at least 10x the bound."""
import numpy as np
import pytest

from oracle import fm, prng

pytestmark = pytest.mark.gpu

D2 = {"gaussian-mixture": 4096, "4-mode": 512}


def _dev(x, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


_TRAINED = {}


def _trained(workload):
    from tests import gpu_util as gu
    if workload not in _TRAINED:
        _TRAINED[workload] = gu.train_like_bench(workload)
    return _TRAINED[workload]


@pytest.fixture(scope="module")
def trained_d2():
    return _trained


def _cut_component(dist):
    from oracle.targets import GaussianMixture
    k = int(np.argmax(dist.weights))                      # the heaviest component: the one most chains sit in
    keep = np.arange(len(dist.weights)) != k
    return GaussianMixture(dist.modes[keep], dist.covs[keep], dist.weights[keep])


def _mala_and_loss(tp, planted_target):
    """MALA init + 3 steps of all chains and the FM loss / gradient on the result, device against libmfm_ref; returns the measured errors
    and those against the oracle run on ``planted_target``."""
    import torch
    from oracle import cref, mala
    from oracle.vfield import flat_params
    from tests import gpu_util as gu
    dist, model, args = tp["dist"], tp["model"], tp["args"]
    params = gu.unflat_params(model, tp["params_flat"])
    x32 = tp["pos"]
    B, d = x32.shape
    ctx = gu.make_ctx(dist, args, n_local=B, n_total=B, fourier=model.f, params=params)
    crs = {"ok": cref.CRef(model, params), "planted": cref.CRef(model, params, target=planted_target)}
    pos = _dev(x32); logp = torch.empty(B, dtype=torch.float64, device="cuda"); grad = torch.empty(B, d, device="cuda")
    ctx.mala_init(pos, 1.0, logp, grad)
    x64 = x32.astype(np.float64)
    sts = {k: mala.MALAState(x64, *c.value_and_grad(x64)) for k, c in crs.items()}
    res = {}
    lp0, g0 = logp.cpu().numpy(), grad.cpu().numpy().astype(np.float64)
    for k, st in sts.items():
        res[f"init_lp_{k}"] = np.abs(lp0 - st.logdensity).max() / np.abs(st.logdensity).max()
        res[f"init_g_{k}"] = np.abs(g0 - st.logdensity_grad).max() / np.abs(st.logdensity_grad).max()
    acc = torch.empty(B, device="cuda"); isacc = torch.empty(B, dtype=torch.uint8, device="cuda")
    ok = np.ones(B, bool)
    moved = 0
    for it in range(3):
        k = prng.split(prng.PRNGKey(77), 3)[it]
        ctx.mala_step(k, 1.0, args.step_size, pos, logp, grad, acc, isacc)
        outs = {n: c.mala_kernel(prng.split(k, B), sts[n], args.step_size) for n, c in crs.items()}
        sts = {n: o[0] for n, o in outs.items()}
        info = outs["ok"][1]
        pg = acc.cpu().numpy().astype(np.float64)
        ig = isacc.cpu().numpy().astype(bool)
        # decisions: equal wherever u is clear of p by more than float32 rounding of p (the uniforms are the oracle's own draws)
        u = prng.uniform_rows(prng.split_rows(prng.split(k, B), 2)[:, 1])
        clear = np.abs(u - info.acceptance_rate) > 1e-4 * np.maximum(info.acceptance_rate, 1e-30) + 1e-6
        res.setdefault("flips_clear", 0); res["flips_clear"] += int((ig != info.is_accepted)[clear & ok].sum())
        ok &= ig == info.is_accepted
        moved += int(info.is_accepted.sum())
        po = info.acceptance_rate[ok]
        res.setdefault("p_err", 0.0); res["p_err"] = max(res["p_err"], float(np.abs(pg[ok] - po).max()))
    res["moved"], res["ok_frac"] = moved, ok.mean()
    xg = pos.cpu().numpy().astype(np.float64)
    sc = max(1.0, np.abs(sts["ok"].position).max())
    for n, st in sts.items():
        res[f"x_{n}"] = np.abs(xg - st.position)[ok].max() / sc
        res[f"lp_{n}"] = (np.abs(logp.cpu().numpy() - st.logdensity)[ok] / np.maximum(1.0, np.abs(st.logdensity[ok]))).max()
    # ---- loss and gradient on the oracle's positions (float32-rounded: what the kernel is given) ----
    xk = sts["ok"].position.astype(np.float32)
    key = prng.PRNGKey(123)
    loss = torch.zeros(1, dtype=torch.float64, device="cuda"); g = torch.zeros(ctx.n_params, device="cuda")
    ctx.fm_loss_grad(key, _dev(xk), loss, g)
    gg = g.cpu().numpy().astype(np.float64)
    batch = fm.cond_flow_batch(key, xk.astype(np.float64), args.sigma)
    for n, c in crs.items():
        lo, go = c.fm_loss_grad(*batch)
        gof = flat_params(go).astype(np.float64)
        res[f"loss_{n}"] = abs(loss.item() - lo) / abs(lo)
        res[f"grad_{n}"] = np.linalg.norm(gg - gof) / np.linalg.norm(gof)
    ctx.close()
    return res


def _check_mala_and_loss(name, r, bounds, p_bound):
    print(f"{name}: mala_init logp rel {r['init_lp_ok']:.1e} (planted {r['init_lp_planted']:.1e}), grad rel {r['init_g_ok']:.1e} "
          f"(planted {r['init_g_planted']:.1e}); 3 MALA steps: {r['moved']} accepted moves, decisions kept {r['ok_frac']:.4f}, flips where "
          f"|u - p| is clear {r['flips_clear']}, |dp| {r['p_err']:.1e}, |dx| {r['x_ok']:.1e} (planted {r['x_planted']:.1e}), logp {r['lp_ok']:.1e} "
          f"(planted {r['lp_planted']:.1e}); loss rel {r['loss_ok']:.1e} (planted {r['loss_planted']:.1e}), grad rel L2 {r['grad_ok']:.1e} "
          f"(planted {r['grad_planted']:.1e})")
    assert r["flips_clear"] == 0 and r["ok_frac"] > 0.995 and r["moved"] > 0
    assert r["p_err"] < p_bound
    for k, b in bounds.items():
        assert r[f"{k}_ok"] < b, (k, r[f"{k}_ok"], b)
    # sensitivity: the device misses the planted oracle by at least 10x the bound on the quantity that sees the error
    assert max(r[f"{k}_planted"] / b for k, b in bounds.items()) > 10.0, {k: r[f"{k}_planted"] for k in bounds}


@pytest.mark.parametrize("workload", list(D2))
def test_d2_mala_steps_loss_and_gradient_all_chains_against_libmfm_ref(trained_d2, workload):
    tp = trained_d2(workload)
    assert tp["pos"].shape == (D2[workload], 2)
    r = _mala_and_loss(tp, _cut_component(tp["dist"]))
    # measured (gaussian-mixture / 4-mode): init log p 1.6e-7 / 7.7e-8, init grad 5.1e-7 / 5.2e-7, |dp| 1.9e-6 / 4.0e-6, |dx| 1.1e-7 / 1.0e-7,
    # log p 4.0e-7 / 3.6e-7, loss 2.2e-11 / 1.6e-9, gradient 4.6e-7 / 1.1e-7; the planted oracle (heaviest component dropped) 0.2 - 1
    _check_mala_and_loss(workload, r, dict(init_lp=1e-6, init_g=3e-6, x=1e-6, lp=2e-6, loss=1e-8, grad=3e-6), p_bound=2e-5)


def _natural_and_replay(tp, tiles):
    """One flow-MH step of all chains: the device and the oracle with their own controllers, then the oracle's recorded sequences on both
    sides (mfm_debug_replay), once per d = 2 tile in ``tiles`` (None: the automatic choice)."""
    import time
    import torch
    from mfm_amd import _lib
    from oracle import cref, mala
    from tests import gpu_util as gu
    dist, model, args = tp["dist"], tp["model"], tp["args"]
    params = gu.unflat_params(model, tp["params_flat"])
    x32 = tp["pos"]
    B, d = x32.shape
    key = prng.PRNGKey(4243)
    keys = prng.split(key, B)
    cr = cref.CRef(model, params)
    st0 = mala.MALAState(x32.astype(np.float64), *cr.value_and_grad(x32.astype(np.float64)))
    out = {}
    t0 = time.perf_counter()
    nat = {}
    _, info_n = cr.rwmh_step(keys, st0, args, stats=nat, record=1001)
    out["t_natural"] = time.perf_counter() - t0
    out["nat"], out["info_nat"] = nat, info_n
    amax = int(max(nat["n_att_inv"].max(), nat["n_att_fwd"].max()))
    cap = amax + 2
    dt = np.zeros((2, B, cap), np.float32); ac = np.zeros((2, B, cap), np.uint8)
    for s_, k_ in enumerate(("inv", "fwd")):
        dt[s_] = nat[k_]["dt_seq"][:, :cap].astype(np.float32); ac[s_] = nat[k_]["acc_seq"][:, :cap]
    rp = dict(inv=dict(dt=dt[0].astype(np.float64), acc=ac[0]), fwd=dict(dt=dt[1].astype(np.float64), acc=ac[1]))
    t0 = time.perf_counter()
    so = {}
    _, info_r = cr.rwmh_step(keys, st0, args, stats=so, replay=rp)
    out["t_replay"] = time.perf_counter() - t0
    out["rep"], out["info_rep"] = so, info_r
    sp = {}
    _, info_p = cr.rwmh_step(keys, st0, args, stats=sp, replay=rp, drop_jvp=1)      # PLANTED: the exact trace without its second JVP
    out["planted"], out["info_planted"] = sp, info_p
    dev = {}
    import os
    for tile in tiles:
        if tile in (None, "natural"):
            os.environ.pop("MFM_D2_TILE", None)
        else:
            os.environ["MFM_D2_TILE"] = tile
        try:
            ctx = gu.make_ctx(dist, args, n_local=B, n_total=B, fourier=model.f, params=params)
        finally:
            os.environ.pop("MFM_D2_TILE", None)
        pos = _dev(x32); logp = torch.empty(B, dtype=torch.float64, device="cuda"); grad = torch.empty(B, d, device="cuda")
        ctx.mala_init(pos, 1.0, logp, grad)
        a = torch.empty(B, device="cuda"); isacc = torch.empty(B, dtype=torch.uint8, device="cuda")
        prop = torch.empty(B, d, device="cuda"); ns = torch.empty(B, dtype=torch.int32, device="cuda")
        if tile == "natural":
            ctx.flow_step(_lib.FLOW_RWMH, key, 1.0, pos.clone(), logp.clone(), grad.clone(), a, isacc, prop, ns)
        else:
            ratio = torch.zeros(dt.shape, device="cuda"); own = torch.zeros(dt.shape, device="cuda")
            diag = torch.zeros(B, 4, dtype=torch.float64, device="cuda")
            ctx.debug_replay(_dev(dt), _dev(ac), ratio, own, diag)
            ctx.flow_step(_lib.FLOW_RWMH, key, 1.0, pos.clone(), logp.clone(), grad.clone(), a, isacc, prop, ns)
        with np.errstate(divide="ignore"):
            la = np.log(a.cpu().numpy().astype(np.float64))
        dev[tile] = dict(n=ns.cpu().numpy().astype(np.int64), prop=prop.cpu().numpy().astype(np.float64), acc=isacc.cpu().numpy().astype(bool),
                         la=la, diag=None if tile == "natural" else diag.cpu().numpy())
        ctx.close()
    out["dev"] = dev
    return out


_FLOW = {}


def _flow(trained_d2, workload):
    if workload not in _FLOW:
        _FLOW[workload] = _natural_and_replay(trained_d2(workload), ["natural", "16", "4", "4s", None])
    return _FLOW[workload]


@pytest.mark.parametrize("workload", list(D2))
def test_d2_flow_step_all_chains_natural_controllers_against_libmfm_ref(trained_d2, workload):
    """Two adaptive solves (float32 kernel, float64 oracle) of the trained exact-trace flow: chain by chain their controllers part ways at
    borderline decisions; over all chains the statistics agree -- attempt counts, proposals, log acceptance ratios, decisions."""
    r = _flow(trained_d2, workload)
    nat, info = r["nat"], r["info_nat"]
    g = r["dev"]["natural"]
    n_o = nat["n_att_inv"] + nat["n_att_fwd"]
    B = n_o.shape[0]
    qs = [0.1, 0.5, 0.9, 0.99]
    ep = np.abs(g["prop"] - info.proposed_position).max(1)
    la_o = nat["log_alpha"]
    fin = np.isfinite(g["la"]) & np.isfinite(la_o)
    ea = np.abs(g["la"] - la_o)[fin]
    print(f"{workload} natural flow step ({B} chains, oracle {r['t_natural']:.1f} s + replay {r['t_replay']:.1f} s): attempts gpu {g['n'].mean():.2f} "
          f"oracle {n_o.mean():.2f} (quantiles {np.quantile(g['n'], qs)} vs {np.quantile(n_o, qs)}), equal for {(g['n'] == n_o).mean():.1%}; "
          f"|dx'| median {np.median(ep):.1e} p90 {np.quantile(ep, 0.9):.1e} max {ep.max():.1e}; |d log alpha| median {np.median(ea):.1e} "
          f"p90 {np.quantile(ea, 0.9):.1e}; decisions differ {(g['acc'] != info.is_accepted).sum()}")
    # measured (gaussian-mixture / 4-mode): mean attempts 72.43 vs 72.46 / 33.08 vs 33.08, quantiles equal but 51.89 vs 52; |dx'| median
    # 5.9e-4 / 1.8e-4, p90 2.2e-3 / 1.1e-3; |d log alpha| median 3.4e-3 / 1.3e-3, p90 1.2e-2 / 6.8e-3; no decision differs
    assert n_o.mean() > 20
    assert abs(g["n"].mean() - n_o.mean()) < 0.005 * n_o.mean()
    assert np.abs(np.quantile(g["n"], qs) / np.quantile(n_o, qs) - 1.0).max() < 0.02
    assert np.median(ep) < 2e-3 and np.quantile(ep, 0.9) < 1e-2
    assert np.median(ea) < 1e-2 and np.quantile(ea, 0.9) < 5e-2
    assert (g["acc"] != info.is_accepted).sum() <= B // 1000


@pytest.mark.parametrize("workload", list(D2))
def test_d2_flow_step_all_chains_on_prescribed_steps_every_tile_against_libmfm_ref(trained_d2, workload):
    """The oracle's recorded step sequences on both sides, once per d = 2 tile: attempt counts of all 2 B solves EXACT; proposals,
    log-determinants and log acceptance ratios by median and quantiles; the automatic tile choice is bit-identical to one of the three.
    PLANTED: the oracle without the second JVP of its exact trace -- the device must miss it by 10x the bound."""
    r = _flow(trained_d2, workload)
    so, info = r["rep"], r["info_rep"]
    sp = r["planted"]
    n_o = so["n_att_inv"] + so["n_att_fwd"]
    q = lambda v: np.quantile(v, [0.5, 0.9, 0.99, 1.0])
    # measured over the three tiles (gaussian-mixture / 4-mode): |dx'| median 2.4e-6 / 1.6e-6, 99 % 2.3e-5 / 1.4e-5, max 9.1e-5 / 2.6e-5;
    # |d vol| median 6.9e-7 / 5.1e-7, 99 % 1.4e-5 / 1.1e-3, max 1.9e-3 / 2.6e-3; |d log alpha| median 3.4e-6 / 5.5e-6, 99 % 2.1e-4 / 1.1e-3;
    # the planted oracle (second JVP dropped): |d vol| median 1.2 / 0.22
    BND = dict(p50=1e-5, p99=1e-4, pmax=5e-4, v50=3e-6, v99=5e-3, vmax=1e-2, a50=3e-5, a99=5e-3)
    for tile in ("16", "4", "4s"):
        g = r["dev"][tile]
        np.testing.assert_array_equal(g["n"], n_o)                                      # every chain, both solves
        ep = np.abs(g["prop"] - info.proposed_position).max(1)
        ev = np.maximum(np.abs(g["diag"][:, 0] - so["vol0"]), np.abs(g["diag"][:, 1] - so["volp"]))
        ea = np.abs(g["diag"][:, 3] - so["log_alpha"])
        evp = np.maximum(np.abs(g["diag"][:, 0] - sp["vol0"]), np.abs(g["diag"][:, 1] - sp["volp"]))
        print(f"{workload} tile {tile}: attempts {n_o.mean():.1f} (max {n_o.max()}) all equal; |dx'| 50/90/99/100 % {q(ep)}; |d vol| {q(ev)}; "
              f"|d log alpha| {q(ea)}; vs the planted oracle |d vol| median {np.median(evp):.1e}")
        assert np.median(ep) < BND["p50"] and np.quantile(ep, 0.99) < BND["p99"] and ep.max() < BND["pmax"]
        assert np.median(ev) < BND["v50"] and np.quantile(ev, 0.99) < BND["v99"] and ev.max() < BND["vmax"]
        assert np.median(ea) < BND["a50"] and np.quantile(ea, 0.99) < BND["a99"]
        assert np.median(evp) > 10 * BND["v50"], np.median(evp)
        sure = np.abs(so["log_alpha"]) > 0.05
        assert (g["acc"] != info.is_accepted)[sure].sum() == 0
    auto = r["dev"][None]
    same = [t for t in ("16", "4", "4s") if all(np.array_equal(auto[k], r["dev"][t][k]) for k in ("n", "prop", "acc", "diag"))]
    print(f"{workload}: the automatic choice is tile {same}")
    assert len(same) >= 1


# ---- pines: configs[4] per GPU ----------------------------------------------------------------------------------------------------------

def test_pines_mala_steps_loss_and_gradient_all_1024_chains_against_libmfm_ref():
    """MALA through the fused LGCP tile (K^-1 streamed once per 16 chains) and the FM loss / gradient through the wide family (split-K
    weight-gradient combine over 1024 chains), all chains.  PLANTED: mu of the K^-1 term shifted by 1e-3."""
    import copy
    tp = _trained("pines")
    assert tp["pos"].shape == (1024, 1024)
    sh = copy.copy(tp["dist"]); sh.mu = tp["dist"].mu + 1e-3
    r = _mala_and_loss(tp, sh)
    # measured: init log p 1.4e-7, init grad 6.0e-7, |dp| 9.8e-5, |dx| 1.2e-7, log p 1.5e-7, loss 2.7e-9, gradient 5.0e-6; the planted oracle
    # (mu + 1e-3) 2.1e-5, 3.5e-5, -, 9.8e-7, 2.3e-5, 2.9e-6, 1.9e-3
    _check_mala_and_loss("pines", r, dict(init_lp=5e-7, init_g=2e-6, x=5e-7, lp=5e-7, loss=2e-8, grad=2e-5), p_bound=5e-4)


# ---- metrics -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [51200, 140000])
def test_stein_and_mmd_pair_kernels_at_full_size_against_libmfm_ref(n):
    """The all-pairs tile kernel (metrics.hip) at configs[0]'s 51,200 samples (several column chunks per row tile) and at 140,000 > 131,072
    (more than 2048 row tiles: one column chunk per row tile) on samples drawn from the 16-mode target, where the Stein sum cancels: the
    stated 1e-5 relative tolerance, on U against V's scale.  PLANTED: the U-statistic without its diagonal removed.  MMD: at 51,200
    only (three float64 exp sums of 1.3e10 pairs each at the larger size take the oracle minutes)."""
    import time
    from oracle import cref
    from oracle.targets import GaussianMixture
    from mfm_amd.multi_modal import gmm16_parameters
    from tests import gpu_util as gu
    m, c, w = gmm16_parameters()
    dist = GaussianMixture(m, c, w)
    keys = prng.split(prng.PRNGKey(n), n)
    x32 = dist.sample_model_rows(keys).astype(np.float32)
    g32 = dist.grad_logprob(x32.astype(np.float64)).astype(np.float32)
    args, odist, k, model, state = gu.gmm4_setup(B=64)
    ctx = gu.make_ctx(odist, args, fourier=model.f, params=state.params)
    u, v = ctx.stein_disc(_dev(x32), _dev(g32))
    t0 = time.perf_counter()
    tot, diag = cref.stein_sums(x32.astype(np.float64), g32.astype(np.float64))
    t_s = time.perf_counter() - t0
    uo, vo = (tot - diag) / (n * (n - 1.0)), tot / float(n) ** 2
    u_planted = tot / (n * (n - 1.0))
    eu, ev = abs(u - uo) / abs(vo), abs(v - vo) / abs(vo)
    print(f"KSD n = {n}: U {u:.6e} vs {uo:.6e}, V {v:.6e} vs {vo:.6e} (U / V {uo / vo:.1e}): |dU| / V {eu:.1e}, |dV| / V {ev:.1e}; "
          f"planted |dU| / V {abs(u - u_planted) / abs(vo):.1e}; oracle {t_s:.1f} s")
    # stated tolerance 1e-5 relative (tests/test_gpu_metrics.py), on U against V's scale; measured 3.3e-8 / 3.0e-8 at both sizes (U / V
    # -0.18 and 0.066: the cancellation is real), so bounded at 1e-6; the planted U (diagonal kept) misses by ~1
    assert ev < 1e-6 and eu < 1e-6
    assert abs(u - u_planted) > 10 * 1e-6 * abs(vo)
    if n <= 51200:
        y32 = (dist.sample_model_rows(prng.split(prng.PRNGKey(n + 1), n)) * 1.02).astype(np.float32)
        mmd = ctx.max_mean_disc(_dev(x32), _dev(y32))
        t0 = time.perf_counter()
        mo = cref.max_mean_disc(x32.astype(np.float64), y32.astype(np.float64))
        print(f"MMD n = {n}: {mmd:.6e} vs {mo:.6e} (rel {abs(mmd - mo) / abs(mo):.1e}); oracle {time.perf_counter() - t0:.1f} s")
        assert abs(mmd - mo) < 1e-7 * abs(mo)                  # (measured 5.1e-9)
    ctx.close()
