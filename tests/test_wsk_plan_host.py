"""CPU tests of the stream-K weight-gradient plan (wgrad_sk.hip: wsk_plan and the tables built from it, through mfm_wsk_plan).

The kernel's workgroups WAIT for the other contributors of their block: a plan whose contributor counts disagree with the ranges
actually dealt out would leave a workgroup polling for a ticket that never comes, and a slice count that is off by one would skip
the deferred optimizer step without any error.  Everything the kernel derives from (q, r) on the device is restated here and
checked against the ranges over the whole parameter space a context can reach -- before anything is launched."""
import numpy as np
import pytest

PF4 = 4 * 4 * 64 + 16          # float4 per partial block (wgrad_sk.hip: WSK_PF4)


def wsk_start(q, r, w):
    return w * q + (w if w < r else r)


def wsk_wg_of(q, r, u):
    big = r * (q + 1)
    return u // (q + 1) if u < big else r + (u - big) // q


def _overrides(n_jobs, nbb, cap):
    U = n_jobs * nbb
    return sorted({0, n_jobs, U, min(U, cap), n_jobs + 1, (n_jobs + U) // 2, 3 * n_jobs, 7 * n_jobs + 3, U - 1})


def _check(n_jobs, nbb, cap, g_req):
    from mfm_amd import _lib
    p = _lib.wsk_plan(n_jobs, nbb, cap, g_req)
    G, q, r, wg = p["G"], p["q"], p["r"], p["wg"].astype(np.int64)
    U = n_jobs * nbb
    tag = (n_jobs, nbb, cap, g_req, G, q, r)
    assert n_jobs <= G <= min(U, cap) and q >= 1 and q * G + r == U and 0 <= r < G, tag
    if n_jobs <= g_req <= min(U, cap):
        assert G == g_req, tag
    j0, bb0, cnt, n0 = wg.T
    w = np.arange(G)
    # the table is what the device functions say: range w starts at unit wsk_start(w) and holds q + (w < r) units
    start = w * q + np.minimum(w, r)
    assert (start == j0 * nbb + bb0).all() and (cnt == q + (w < r)).all(), tag
    assert ((0 <= bb0) & (bb0 < nbb) & (0 <= j0) & (j0 < n_jobs)).all(), tag
    # every unit lies in exactly one range: the ranges are contiguous, in order, and end at U
    assert start[0] == 0 and (start[1:] == start[:-1] + cnt[:-1]).all() and start[-1] + cnt[-1] == U, tag
    # a range is never longer than a block's chain axis, so it touches at most two blocks; n0 is its part of the first
    assert (cnt >= 1).all() and (cnt <= nbb).all(), tag
    last_block = (start + cnt - 1) // nbb
    assert (last_block - j0 <= 1).all() and (last_block < n_jobs).all(), tag
    assert (n0 == np.minimum(cnt, nbb - bb0)).all() and (n0 >= 1).all(), tag
    nseg = 1 + (n0 < cnt)
    assert (nseg == 1 + (last_block - j0)).all(), tag
    # contributors of every block: as counted from the ranges, and as the kernel derives them (nc)
    touched = np.bincount(j0, minlength=n_jobs) + np.bincount(last_block[nseg == 2], minlength=n_jobs)
    blocks = np.arange(n_jobs)
    big = r * (q + 1)

    def wg_of(u):
        return np.where(u < big, u // (q + 1), r + (u - big) // q)
    w_lo, w_hi = wg_of(blocks * nbb), wg_of((blocks + 1) * nbb - 1)
    nc = w_hi - w_lo + 1
    assert (nc == touched).all(), tag
    assert nc.sum() == p["n_slices"] == nseg.sum(), tag
    # the segment select of the combine loop names the segment in which contributor cw holds block j
    # (the contributors [w_lo, w_hi] of a block are exactly the workgroups whose range touches it: each of those lies inside, and
    # the counts agree; for such a pair the select `wsk_start(cw) < j * nbb` must say 0 for the first block of cw, 1 for its second)
    assert ((w_lo[j0] <= w) & (w <= w_hi[j0])).all() and ((w_lo[last_block] <= w) & (w <= w_hi[last_block])).all(), tag
    assert not (start < j0 * nbb).any(), tag
    two = nseg == 2
    assert (start[two] < (j0[two] + 1) * nbb).all() and (cnt[two] - n0[two] >= 1).all(), tag
    j, cw = n_jobs // 2, int(w_lo[n_jobs // 2])          # and once through the scalar restatements
    assert wsk_wg_of(q, r, j * nbb) == cw and j0[cw] + (1 if wsk_start(q, r, cw) < j * nbb else 0) == j, tag
    return set(nc.tolist())


def test_the_scalar_restatements_agree_with_the_vector_forms():
    for q, r in ((1, 0), (1, 52), (2, 52), (7, 45), (32, 0), (3, 1)):
        G = r + 5
        for w in range(G):
            for u in range(wsk_start(q, r, w), wsk_start(q, r, w + 1)):
                assert wsk_wg_of(q, r, u) == w


@pytest.mark.parametrize("cap_kind", ["n_jobs", "256", "512"])
def test_every_plan_covers_every_unit_once_and_counts_its_contributors_as_the_kernel_does(cap_kind):
    """n_jobs 1..64, nbb 1..300: the default G (what every context runs) and a grid half way between its bounds; more overrides
    at a thinner set of nbb in the next test."""
    seen = set()
    for n_jobs in range(1, 65):
        cap = n_jobs if cap_kind == "n_jobs" else int(cap_kind)
        if cap < n_jobs:
            continue
        for nbb in range(1, 301):
            seen |= _check(n_jobs, nbb, cap, 0)
            _check(n_jobs, nbb, cap, (n_jobs + min(n_jobs * nbb, cap)) // 2)
    # the contributor counts that occur cut the 1040 float4 of a partial block into slices that partition it
    assert seen and max(seen) <= 300
    if cap_kind == "512":
        assert {5, 6, 7, 9, 10, 13} <= seen          # the counts of the ragged chain counts the GPU tests run
    for nc in sorted(seen):
        per = (PF4 + nc - 1) // nc
        edges = [(min(i * per, PF4), min(i * per + per, PF4)) for i in range(nc)]
        assert edges[0][0] == 0 and edges[-1][1] == PF4 and all(a[1] == b[0] for a, b in zip(edges, edges[1:])), nc
        assert all(lo <= hi for lo, hi in edges), nc


@pytest.mark.parametrize("cap", [64, 256, 512])
def test_overridden_grids_keep_the_invariants(cap):
    nbbs = sorted(set(range(1, 40)) | {57, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 300})
    for n_jobs in (1, 2, 3, 7, 8, 13, 31, 52, 64):
        for nbb in nbbs:
            for g_req in _overrides(n_jobs, nbb, cap):
                _check(n_jobs, nbb, cap, g_req)


def test_the_headline_network_plans_named_in_the_kernel_header():
    """52 blocks under a cap of 512 resident workgroups: the default is 8 slices of 32 tiles at 4096 chains; ragged chain counts
    give two-segment workgroups, contributor counts that do not divide 1040 or exceed one read batch of 8, and n_slices != G."""
    from mfm_amd import _lib
    rows = {}
    for chains in (64, 4096, 144, 160, 208, 272, 912):
        p = _lib.wsk_plan(52, chains // 16, 512)
        wg = p["wg"]
        nc = np.bincount(wg[:, 0], minlength=52) + np.bincount(wg[wg[:, 3] < wg[:, 2], 0] + 1, minlength=52)
        rows[chains] = (p["G"], p["q"], p["r"], int((wg[:, 3] < wg[:, 2]).sum()), sorted(set(nc.tolist())), p["n_slices"])
    assert rows[64] == (208, 1, 0, 0, [4], 208)
    assert rows[4096] == (416, 32, 0, 0, [8], 416)
    assert rows[144] == (416, 1, 52, 6, [5, 7, 9], 422)
    assert rows[160] == (416, 1, 104, 0, [5, 6, 10], 416)
    assert rows[208] == (416, 1, 260, 20, [7, 13], 436)
    assert rows[272] == (416, 2, 52, 27, [6, 7, 8, 9], 443)
    assert rows[912] == (416, 7, 52, 45, [8, 9], 461)


def test_invalid_plan_requests_are_refused():
    from mfm_amd import _lib
    for bad in ((0, 4, 512), (4, 0, 512), (8, 4, 7)):
        with pytest.raises(_lib.MfmError):
            _lib.wsk_plan(*bad)
