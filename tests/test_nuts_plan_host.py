"""CPU tests of the NUTS launch geometry (nuts.hip: nuts_waves and nuts_smem, through mfm_nuts_launch_plan).

The kernels place wave w's U-turn checkpoints at ``mala_smem(dim) + w * slab`` with ``slab = (max_tree_depth - 1) * 2 * dim`` doubles
(nuts_checkpoints) and the launch asks for ``nuts_smem`` bytes: a plan whose byte count is short of the last slab's end lets a wave
write past the workgroup's LDS, and one whose slabs overlap makes a chain's tree depend on its neighbour's.  The layout is restated here
and held to the plan over every (dim, max_tree_depth) the API accepts -- before anything is launched."""
import pytest

LDS_CU, MAX_WAVES, MAX_DIM, MAX_DEPTH = 163840, 4, 256, 16


def mala_smem(d):
    """mala.hip: MALA_WAVES rows of d + 2 floats and MALA_WAVES x MALA_MAXD_SMALL floats of gradient scratch."""
    return (4 * (d + 2) + 4 * 8) * 4


def slab(d, depth):
    return (depth - 1) * 2 * d * 8


def test_the_plan_over_every_dim_and_depth():
    from mfm_amd import _lib
    seen = {}
    largest = (0, None)
    for d in range(1, MAX_DIM + 1):
        for depth in range(1, MAX_DEPTH + 1):
            waves, lds, per_cu = _lib.nuts_launch_plan(d, depth)
            tag = (d, depth, waves, lds, per_cu)
            assert 1 <= waves <= MAX_WAVES, tag
            assert lds <= LDS_CU and per_cu == LDS_CU // lds and per_cu >= 1, tag
            assert lds == mala_smem(d) + waves * slab(d, depth), tag
            # the slabs as nuts_checkpoints places them: 8-byte aligned, back to back, the last one ending where the request ends
            starts = [mala_smem(d) + w * slab(d, depth) for w in range(waves)]
            assert all(s % 8 == 0 for s in starts), tag
            assert all(starts[w] + slab(d, depth) == starts[w + 1] for w in range(waves - 1)), tag
            assert starts[-1] + slab(d, depth) == lds, tag
            # the rule in nuts.hip's comment: the count that puts the most chains on a CU, the larger count on a tie
            chains = {w: (LDS_CU // (mala_smem(d) + w * slab(d, depth))) * w for w in range(1, MAX_WAVES + 1)
                      if mala_smem(d) + w * slab(d, depth) <= LDS_CU}
            assert all(chains[w] <= chains[waves] for w in chains if w < waves), (tag, chains)
            assert all(chains[w] < chains[waves] for w in chains if w > waves), (tag, chains)
            seen.setdefault(waves, (d, depth))
            largest = max(largest, (lds, (d, depth, waves)))
    print(f"first (dim, depth) of each chain count: {seen}; largest request {largest}")
    assert set(seen) == {1, 2, 3, 4}, seen
    # the largest request of all, 16 B under a CU's LDS: tests/nuts_cases.py's PLACEMENT launches it
    assert largest == (163824, (193, 14, 4)), largest


@pytest.mark.parametrize("d,depth,waves", [(64, 10, 4), (64, 11, 3), (64, 12, 1), (64, 16, 2), (128, 11, 1), (128, 14, 1), (128, 15, 1),
                                           (192, 10, 1), (100, 5, 2), (256, 6, 3), (256, 14, 2), (130, 16, 4), (193, 14, 4)])
def test_the_geometries_the_gpu_tests_name(d, depth, waves):
    from mfm_amd import _lib
    assert _lib.nuts_launch_plan(d, depth)[0] == waves


def test_errors_are_those_of_the_step():
    from mfm_amd import _lib
    for depth in (0, 17, -1):
        with pytest.raises(_lib.MfmError, match=r"max_tree_depth must be in \[1, 16\]"):
            _lib.nuts_launch_plan(64, depth)
    with pytest.raises(_lib.MfmError, match="dim <= 256"):
        _lib.nuts_launch_plan(257, 5)
    with pytest.raises(_lib.MfmError, match="dim"):
        _lib.nuts_launch_plan(0, 5)
    import ctypes as C
    w = C.c_int32()
    assert _lib.load().mfm_nuts_launch_plan(64, 5, C.byref(w), None, C.byref(w)) != 0
