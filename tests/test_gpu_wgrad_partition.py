"""GPU parity of the weight-gradient kernels at chain counts that split unevenly over their slices.

The stream-K kernel (wgrad_sk.hip) deals U = n_jobs * nbb units to G workgroups; for nbb <= 8 or nbb % 8 == 0 every workgroup
stays inside one 64 x 64 block and every block has min(nbb, 8) contributors.  Any other chain count reaches the second segment of
a workgroup, contributor counts that do not divide a partial block or exceed one read batch, ring stages that straddle a block
boundary and a slice count that differs from the grid -- and the slab kernels (fm.hip) and the wide family's kernel (wide.hip) have
row-count branches of their own.  Every case first asks the library which plan it runs (mfm_wgrad_info / mfm_wsk_plan) and FAILS
if the feature it exists for is absent, so a changed plan cannot quietly stop covering a path.

References: the float64 oracle (oracle.fm.loss_and_grad) under the project's tolerances, and -- element by element -- the sum of the
gradients of shards with trivial plans under the forward-error bound of a float32 dot product (tests/wgrad_cases.py: order_bound;
tests/test_oracle_wgrad_bound.py shows that a dropped or doubled tile exceeds it at least tenfold)."""
import json

import numpy as np
import pytest

from oracle import prng
from tests import wgrad_cases as wc

pytestmark = pytest.mark.gpu

_RUNS = {}


def _dev(x, dtype=None):
    import torch
    return torch.as_tensor(np.array(x), dtype=dtype).cuda()


def _features(info):
    """What the plan this context runs exercises (stream-K: from the very table the context was built from)."""
    from mfm_amd import _lib
    f = dict(info)
    if info["kind"] != _lib.WGRAD_STREAM_K:
        return f
    p = _lib.wsk_plan(info["n_jobs"], info["nbb"], info["G"], info["G"])
    assert (p["G"], p["q"], p["r"]) == (info["G"], info["q"], info["r"]), (p, info)
    j0, bb0, cnt, n0 = p["wg"].astype(np.int64).T
    two = n0 < cnt
    nc = np.bincount(j0, minlength=info["n_jobs"]) + np.bincount(j0[two] + 1, minlength=info["n_jobs"])
    f.update(n_slices=p["n_slices"], two_seg=int(two.sum()), nc=sorted(set(nc.tolist())), max_nc=int(nc.max()),
             units=(int(cnt.min()), int(cnt.max())),
             nc_ragged=bool((wc.PF4 % nc != 0).any()),                    # `per` rounds up: the last slice is shorter
             odd_n0=bool((two & (n0 % 2 == 1)).any()),                    # a two-tile ring stage straddles the block boundary
             ring_wrap_cross=bool((two & (cnt >= 7)).any()),              # the ring wraps in a range that crosses a boundary
             ring_wrap=bool((cnt >= 7).any()), nc_gt_8=bool(nc.max() > 8),      # more than one batch of WSK_NCB = 8 read-backs
             slices_ne_G=p["n_slices"] != info["G"])
    return f


def _need(f, *names, **values):
    """The plan features a case exists for: absent means the case no longer covers its path -- a failure, never a skip."""
    for n in names:
        if not f.get(n):
            pytest.fail(f"the plan no longer has the feature this case exists for: {n} ({f})")
    for n, v in values.items():
        if f.get(n) != v:
            pytest.fail(f"the plan no longer has the feature this case exists for: {n} == {v} ({f})")


def _loss_grad(net, B, n_local=None, offset=0, n_valid=None, family=None, x=None):
    """mfm_fm_loss_grad of chains [offset, offset + n_local) of the case's B on a fresh context -> loss, gradient, plan features."""
    import torch
    from tests import gpu_util as gu
    args, dist, model, params, x32 = wc.setup(net, B)
    n_local = B if n_local is None else n_local
    n_total = B if n_valid is None else n_valid
    ctx = gu.make_ctx(dist, args, n_local=n_local, n_total=n_total, offset=offset, fourier=model.f, params=params, family=family, n_valid=n_valid)
    try:
        f = _features(ctx.wgrad_info())
        loss = torch.zeros(1, dtype=torch.float64, device="cuda"); grads = torch.zeros(ctx.n_params, device="cuda")
        ctx.fm_loss_grad(wc.case_key(net, B), _dev(x32[offset:offset + n_local] if x is None else x), loss, grads)
        return dict(loss=loss.item(), grads=grads.cpu().numpy(), f=f)
    finally:
        ctx.close()


def _run(net, B, mode="default", monkeypatch=None):
    """The whole-batch result of a case under a decomposition `mode`, computed once and shared (read-only)."""
    k = (net, B, mode)
    if k not in _RUNS:
        if mode == "slabs":
            monkeypatch.setenv("MFM_WGRAD_SLABS", "1")
        elif mode != "default":
            monkeypatch.setenv("MFM_WSK_G", str(int(mode)))
        _RUNS[k] = _loss_grad(net, B)
        _RUNS[k]["grads"].setflags(write=False)
        if monkeypatch is not None:
            monkeypatch.delenv("MFM_WGRAD_SLABS", raising=False); monkeypatch.delenv("MFM_WSK_G", raising=False)
    return _RUNS[k]


def _shard_sum(net, B, sizes):
    """Sum (float64) of the gradients and losses of consecutive shards of `sizes` chains, every one on a plan with r == 0."""
    tot, loss, off = 0.0, 0.0, 0
    for n in sizes:
        r = _loss_grad(net, B, n_local=n, offset=off)
        _need(r["f"], r=0, two_seg=0)
        tot = tot + r["grads"].astype(np.float64); loss += r["loss"]; off += n
    assert off == B
    return loss, tot


def _friendly(net, B):
    k = (net, B, "shards")
    if k not in _RUNS:
        _RUNS[k] = _shard_sum(net, B, [min(128, B - o) for o in range(0, B, 128)])
    return _RUNS[k]


def _order_ratio(a, b, B, S):
    """max over the elements of |a - b| / (2 (B + 2) 2^-24 S_e); where S_e == 0 both sides must be exactly equal."""
    err = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    bound = wc.order_bound(B, S)
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max())


def _assert_oracle(net, B, r, o):
    from tests import gpu_util as gu
    args, dist, model, params, x32 = wc.setup(net, B)
    assert abs(r["loss"] - o["loss"]) <= 2e-5 * abs(o["loss"]), (r["loss"], o["loss"])
    worst = 0.0
    for i, (gg, go) in enumerate(zip(gu.unflat_params(model, r["grads"]), o["grads"])):
        for kk in ("kernel", "bias"):
            e = np.abs(gg[kk].astype(np.float64) - go[kk]).max() / (np.abs(go[kk]).max() + 1e-30)
            worst = max(worst, e)
            assert e < 2e-4, (net, B, i, kk, e)
    return worst


# what each chain count of (a) exists for (restated for the headline network in tests/test_wsk_plan_host.py)
FRIENDLY = dict(r=0, two_seg=0)
NEEDS = {
    ("S", 16): FRIENDLY, ("S", 48): FRIENDLY,
    ("S", 144): ("r", "two_seg", "nc_gt_8", "nc_ragged", "odd_n0", "slices_ne_G"),
    ("S", 160): ("r", "nc_gt_8", "nc_ragged"),                       # 10 contributors, no workgroup crosses a boundary
    ("S", 208): ("r", "two_seg", "nc_gt_8", "odd_n0", "slices_ne_G"),
    ("S", 272): ("r", "two_seg", "nc_gt_8", "nc_ragged", "odd_n0", "slices_ne_G"),
    ("S", 912): ("r", "two_seg", "nc_gt_8", "ring_wrap_cross", "slices_ne_G"),
    ("R", 144): ("r", "two_seg", "nc_gt_8", "odd_n0", "slices_ne_G"),
    ("R", 400): ("r", "two_seg", "nc_gt_8", "nc_ragged", "slices_ne_G"),
    ("H", 144): ("r", "two_seg", "nc_gt_8", "nc_ragged", "odd_n0", "slices_ne_G"),
    ("H", 272): ("r", "two_seg", "nc_gt_8", "nc_ragged", "odd_n0", "slices_ne_G"),
    ("H", 912): ("r", "two_seg", "nc_gt_8", "ring_wrap_cross", "slices_ne_G"),
    ("M", 208): ("r", "two_seg", "nc_gt_8", "odd_n0", "slices_ne_G"),
}


@pytest.mark.parametrize("net,B", wc.CASES_A)
def test_loss_and_gradient_match_the_oracle_at_uneven_chain_counts(net, B):
    """mfm_fm_loss_grad against oracle.fm.loss_and_grad under the project's tolerances (loss 2e-5, every parameter tensor 2e-4 of
    its maximum), on the default plan of each chain count, whose features (NEEDS) are asserted first."""
    from mfm_amd import _lib
    r, o = _run(net, B), wc.oracle(net, B)
    f = r["f"]
    _need(f, kind=_lib.WGRAD_STREAM_K)
    need = NEEDS[(net, B)]
    _need(f, **need) if isinstance(need, dict) else _need(f, *need)
    worst = _assert_oracle(net, B, r, o)
    print("WGRAD_A " + json.dumps(dict(case=f"{net}@{B}", G=f["G"], q=f["q"], r=f["r"], two_seg=f["two_seg"], max_nc=f["max_nc"], nc=f["nc"],
                                       n_slices=f["n_slices"], units=f["units"], worst_rel_err_vs_oracle=worst)))


def test_control_two_friendly_shardings_agree_within_the_summation_order_bound():
    """64 + 64 + 16 against 128 + 16 chains of S at 144: both sides are sums over trivial plans.  If THIS failed the tiles would
    not be bit-identical across shardings and the bound would prove nothing about the ragged plans."""
    o = wc.oracle("S", 144)
    la, ga = _shard_sum("S", 144, [64, 64, 16])
    lb, gb = _friendly("S", 144)
    ratio = _order_ratio(ga, gb, 144, o["S"])
    print(f"WGRAD_CONTROL ratio {ratio:.4g}")
    assert ratio <= 1.0
    assert abs(la - lb) <= 1e-12 * abs(lb)


@pytest.mark.parametrize("net,B", wc.CASES_A)
def test_gradient_equals_the_sum_over_friendly_shards_up_to_summation_order(net, B):
    """The draws are indexed by global chain id and a 16-chain tile is processed alike wherever it sits: B chains on one context
    against shards of at most 128 chains (plans with r == 0), element by element within 2 (B + 2) 2^-24 S_e."""
    r, o = _run(net, B), wc.oracle(net, B)
    loss, tot = _friendly(net, B)
    ratio = _order_ratio(r["grads"], tot, B, o["S"])
    print("WGRAD_B " + json.dumps(dict(case=f"{net}@{B}", worst_ratio_to_order_bound=ratio)))
    assert ratio <= 1.0, (net, B, ratio)
    assert abs(r["loss"] - loss) <= 1e-12 * abs(loss)


# ---- (c) one call equals the separate calls ---------------------------------------------------------------------------------

def _train(net, B, one_call, nan_at=None):
    import torch
    from mfm_amd._lib import FLOW_RWMH
    from tests import gpu_util as gu
    args, dist, model, _, x32 = wc.setup(net, B, learning_iter=20)
    params = gu.rand_params(model, seed=3, out_scale=0.05)
    ctx = gu.make_ctx(dist, args, fourier=model.f, params=params)
    f = _features(ctx.wgrad_info())
    pos = torch.from_numpy(x32.copy()).cuda(); logp = torch.empty(B, device="cuda", dtype=torch.float64); grad = torch.empty_like(pos)
    acc = torch.empty(B, device="cuda"); loss = torch.zeros(1, device="cuda", dtype=torch.float64); grads = torch.zeros(ctx.n_params, device="cuda")
    ctx.mala_init(pos, 1.0, logp, grad)
    ks, tr = prng.PRNGKey(5), []
    for count in range(1, 6):
        ks, kg, kt = prng.split(ks, 3)
        if count == nan_at:
            saved = pos[5, 7].item(); pos[5, 7] = float("nan")
        if one_call:
            ctx.train_iter(count, 100, FLOW_RWMH, kg, kt, 1.0, args.step_size, pos, logp, grad, loss, grads, acc=acc)
        else:
            ctx.mala_step(kg, 1.0, args.step_size, pos, logp, grad, acc); ctx.fm_loss_grad(kt, pos, loss, grads); ctx.adamw_step(grads)
        st = ctx.opt_state()
        tr.append(dict(st=st, params=ctx.get_params().copy(), loss=loss.item(), pos=pos.cpu().numpy(), logp=logp.cpu().numpy(),
                       grads=grads.cpu().numpy()))
        if count == nan_at:
            pos[5, 7] = saved
            ctx.mala_init(pos, 1.0, logp, grad)
    ctx.close()
    return f, tr


def _assert_same_trace(a, b):
    for i, (u, v) in enumerate(zip(a, b)):
        assert u["st"] == v["st"], (i, u["st"], v["st"])
        assert (np.isnan(u["loss"]) and np.isnan(v["loss"])) or u["loss"] == v["loss"], (i, u["loss"], v["loss"])
        for kk in ("params", "pos", "logp", "grads"):
            np.testing.assert_array_equal(u[kk], v[kk], err_msg=f"iteration {i + 1}: {kk}")


@pytest.mark.parametrize("net,B", [("H", 144), ("H", 272), ("S", 208)])
def test_train_iter_equals_the_separate_calls_at_uneven_chain_counts(net, B):
    """Five iterations of mfm_train_iter(apply_update = 1) against mfm_mala_step + mfm_fm_loss_grad + mfm_adamw_step: parameters,
    optimizer state (the moments show in the next iteration's parameters), loss, gradient and chains bit for bit."""
    from mfm_amd import _lib
    f, sep = _train(net, B, False)
    _need(f, "r", "two_seg", "slices_ne_G", kind=_lib.WGRAD_STREAM_K)
    _, one = _train(net, B, True)
    _assert_same_trace(sep, one)
    for i, t in enumerate(one):
        assert (t["st"]["step"], t["st"]["count"], t["st"]["notfinite_count"], t["st"]["last_applied"]) == (i + 1, i + 1, 0, 1)
        assert i == 0 or not np.array_equal(t["params"], one[i - 1]["params"])


def test_train_iter_through_the_deferred_decision_commits_every_step_at_an_uneven_chain_count(monkeypatch):
    """H at 144 with every launch forced through the apply-if-finite exchange, whose last ticket is recognised by comparing a
    count with n_slices (422 here, not G = 416): a sum that is off would leave `step` where it was, silently.  A NaN position in
    iteration 3: that update is skipped and counted, the next one applies."""
    from mfm_amd import _lib
    monkeypatch.setenv("MFM_DEBUG_FORCE_EXCHANGE", "1")
    f, sep = _train("H", 144, False, nan_at=3)
    _need(f, "r", "two_seg", "slices_ne_G", kind=_lib.WGRAD_STREAM_K)
    _, one = _train("H", 144, True, nan_at=3)
    want = [(1, 1, 0, 1), (2, 2, 0, 1), (3, 2, 1, 0), (4, 3, 0, 1), (5, 4, 0, 1)]          # step, count, notfinite_count, last_applied
    for tr in (sep, one):
        for t, w in zip(tr, want):
            assert (t["st"]["step"], t["st"]["count"], t["st"]["notfinite_count"], t["st"]["last_applied"]) == w, (t["st"], w)
        np.testing.assert_array_equal(tr[1]["params"], tr[2]["params"])          # the skipped update left the parameters alone
        assert not np.array_equal(tr[2]["params"], tr[3]["params"]) and not np.array_equal(tr[0]["params"], tr[1]["params"])
    _assert_same_trace(sep, one)


# ---- (d) padding rows ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_valid,B", [(150, 160), (200, 208)])
def test_padding_rows_of_an_uneven_shard_contribute_nothing(n_valid, B):
    from mfm_amd import _lib
    args, dist, model, params, x32 = wc.setup("S", B)
    o = wc.oracle("S", B, n_valid=n_valid)
    r = _loss_grad("S", B, n_valid=n_valid)
    _need(r["f"], "r", kind=_lib.WGRAD_STREAM_K)
    _assert_oracle("S", B, r, o)
    flipped = x32.copy(); flipped[n_valid:] = -3.0 * flipped[n_valid:] + 1.0
    r2 = _loss_grad("S", B, n_valid=n_valid, x=flipped)
    assert r2["loss"] == r["loss"]
    np.testing.assert_array_equal(r2["grads"], r["grads"])


# ---- (e) slab kernels, (f) other decompositions --------------------------------------------------------------------------------

@pytest.mark.parametrize("net,B", [("S", 144), ("S", 208), ("H", 272)])
def test_slab_kernels_with_unequal_slices(monkeypatch, net, B):
    from mfm_amd import _lib
    sk, o = _run(net, B), wc.oracle(net, B)
    r = _run(net, B, "slabs", monkeypatch)
    _need(r["f"], "r", kind=_lib.WGRAD_SLABS)          # r = nbb % split: the slices bb_lo = nbb * sp / split are unequal
    _need(sk["f"], kind=_lib.WGRAD_STREAM_K)
    _assert_oracle(net, B, r, o)
    ratio = _order_ratio(r["grads"], sk["grads"], B, o["S"])
    print("WGRAD_E " + json.dumps(dict(case=f"{net}@{B}", worst_ratio_to_order_bound=ratio)))
    assert ratio <= 1.0
    assert r["loss"] == sk["loss"]


@pytest.mark.parametrize("which", ["one_unit_per_workgroup", "one_workgroup_per_block"])
def test_other_decompositions_of_the_same_units(monkeypatch, which):
    from mfm_amd import _lib
    net, B = "S", 208
    d, o = _run(net, B), wc.oracle(net, B)
    n_jobs, nbb = d["f"]["n_jobs"], d["f"]["nbb"]
    G = n_jobs * nbb if which == "one_unit_per_workgroup" else n_jobs
    r = _run(net, B, str(G), monkeypatch)
    _need(r["f"], kind=_lib.WGRAD_STREAM_K, G=G, two_seg=0)
    if which == "one_unit_per_workgroup":
        _need(r["f"], units=(1, 1), nc=[13], max_nc=13)          # 13 contributors: two read batches
    else:
        _need(r["f"], "ring_wrap", units=(13, 13), nc=[1])
    _assert_oracle(net, B, r, o)
    ratio = _order_ratio(r["grads"], d["grads"], B, o["S"])
    print("WGRAD_F " + json.dumps(dict(case=which, worst_ratio_to_order_bound=ratio)))
    assert ratio <= 1.0


# ---- (g) wide family ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("net,B", [("S", 16), ("S", 48), ("S", 80), ("P", 64), ("P", 80)])
def test_wide_family_row_count_branches(net, B):
    """One, three and five 16-row blocks (the odd tail of the two-block loop), the workgroup-per-job tail with one block per wave
    (pines width, 64 rows) and the same width at 80 rows, where the tail is declined."""
    from mfm_amd import _lib
    r = _loss_grad(net, B, family=_lib.FAMILY_WIDE)
    _need(r["f"], kind=_lib.WGRAD_WIDE, nbb=B // 16)
    if (net, B) == ("P", 64):
        _need(r["f"], "q")                                        # q: jobs run a workgroup each
        assert r["f"]["n_jobs"] > 2048 and r["f"]["q"] == r["f"]["n_jobs"] % 2048
    else:
        _need(r["f"], q=0)
        assert (B // 16) % 2 == 1
    _assert_oracle(net, B, r, wc.oracle(net, B))
