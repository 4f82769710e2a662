"""CPU tests of the wide family's GEMM dispatch (wide.hip: gemm_plan, the function launch_gemm launches from, through
mfm_wide_gemm_plan).

Every network layer of the wide family is one launch of one of thirteen kernel instances on a grid that the same function sizes.  A
grid one workgroup short leaves a band of rows or features unwritten (finite garbage from the last call, not a crash); an instance
chosen outside its precondition reads K blocks that are not there (the LDS kernel consumes K in steps of 8 blocks, ring 8 likewise,
the dual LDS kernel tangent K in steps of 4).  What each kernel assumes is restated here from the kernels themselves and checked
over the whole shape space a context can reach, under every mask of the four development switches -- before anything is launched."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

# 16 x 16 output tiles per workgroup (rows, features) and threads, from the kernels: gemm_kernel<MTW, NTW> is 2 x 2 waves of
# MTW x NTW tiles; gemm_lds_kernel<DUAL, WM> a 64 x 64 tile on 4 WM waves
TILE = {"11": (2, 2, 256), "12": (2, 4, 256), "22": (4, 4, 256), "22_ring8": (4, 4, 256), "big": (8, 4, 256), "lds": (4, 4, 512), "lds_wm1": (4, 4, 256)}
ROWS = sorted(set(range(16, 1041, 16)) | {2624, 5120, 16384})
KBS = list(range(1, 21)) + [64, 100]
NTS = list(range(1, 37)) + [64, 100]


def _plan_fn():
    """mfm_wide_gemm_plan with the output as a plain address: 1.1 million plans per mask go straight into one numpy array."""
    from mfm_amd import _lib
    lib = _lib.load()
    proto = C.CFUNCTYPE(C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_void_p)
    return C.cast(lib.mfm_wide_gemm_plan, proto)


def _shapes():
    out = []
    for KB in KBS:
        for dual, KBT in [(0, 0)] + [(1, k) for k in range(1, KB + 1)]:
            for NT in NTS:
                for rows in ROWS:
                    out.append((rows, KB, NT, dual, KBT))
    return np.array(out, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _shape_lists():
    S = _shapes()
    return S, [c.tolist() for c in S.T]


def _sweep(mask):
    from mfm_amd import _lib
    S, cols = _shape_lists()
    res = np.full((len(S), 4), -1, dtype=np.int32)
    addr = (res.ctypes.data + 16 * np.arange(len(S), dtype=np.int64)).tolist()
    rc = list(map(_plan_fn(), *cols, itertools.repeat(mask), addr))
    assert not any(rc), (S[np.flatnonzero(rc)[0]], mask, _lib.load().mfm_last_error())
    names = np.array(_lib.WGEMM)[res[:, 0]]
    return S, names, res


@pytest.mark.parametrize("mask", range(16))
def test_every_plan_covers_the_output_and_meets_its_kernels_preconditions(mask):
    from mfm_amd import _lib
    SW = _lib.WGEMM_SW
    S, names, res = _sweep(mask)
    rows, KB, NT, dual, KBT = S.T
    MT = rows // 16
    gx, gy, block = res[:, 1].astype(np.int64), res[:, 2].astype(np.int64), res[:, 3]
    assert ((res[:, 0] >= 0) & (res[:, 0] < len(_lib.WGEMM))).all()
    kinds = sorted(TILE)                                             # per instance id: its kernel (the name without "_dual") and whether it is dual
    kind_of = np.array([kinds.index(n[:-5] if n.endswith("_dual") else n) for n in _lib.WGEMM])
    base = np.array(kinds)[kind_of[res[:, 0]]]
    is_dual = np.array([n.endswith("_dual") for n in _lib.WGEMM])[res[:, 0]]
    assert (np.char.add(base, np.where(is_dual, "_dual", "")) == names).all()
    # the tangent GEMM rides along exactly when it was asked for ("big" has no dual form and is never chosen for one)
    assert (is_dual == (dual == 1)).all()
    assert (dual[base == "big"] == 0).all()
    tm, tn, th = np.array([TILE[k] for k in kinds])[kind_of[res[:, 0]]].T
    assert (block == th).all()
    # the grid covers MT x NT tiles with less than one whole workgroup row / column to spare
    assert ((gy * tm >= MT) & ((gy - 1) * tm < MT)).all(), S[~((gy * tm >= MT) & ((gy - 1) * tm < MT))][:5]
    assert ((gx * tn >= NT) & ((gx - 1) * tn < NT)).all(), S[~((gx * tn >= NT) & ((gx - 1) * tn < NT))][:5]
    # LDS staging: K in steps of 8 blocks (two 64-wide steps per loop trip), the tangent's prefix in whole 64-wide steps, at least one
    lds = (base == "lds") | (base == "lds_wm1")
    assert (KB[lds] & 7 == 0).all()
    assert ((KBT[lds & is_dual] & 3 == 0) & (KBT[lds & is_dual] >= 4)).all()
    # the ring of eight: whole rings of K blocks, and of tangent K blocks
    r8 = base == "22_ring8"
    assert (KB[r8] % 8 == 0).all() and (KBT[r8 & is_dual] % 8 == 0).all()
    # the variants behind a switch run only under it; a switch that forbids a kernel is obeyed
    if not mask & SW["MFM_WIDE_RING8"]:
        assert not r8.any()
    if not mask & SW["MFM_WIDE_WM1"]:
        assert not (base == "lds_wm1").any()
    else:
        assert not (base == "lds").any()
    if mask & SW["MFM_WIDE_NOLDS"]:
        assert not lds.any()
    if mask & SW["MFM_WIDE_NO_SMALL_TILES"]:
        assert not ((base == "11") | (base == "12")).any()
    else:
        # the thresholds of the row count: 32 x 32 wave tiles up to 256 rows, 32 x 64 up to 512 (none of the swept shapes is "big" there)
        assert (base[rows <= 256] == "11").all() and (base[(rows > 256) & (rows <= 512)] == "12").all()
        assert not np.isin(base[rows > 512], ("11", "12")).any()
    # "big": only launches of at least 16384 tiles that the LDS kernel does not serve
    big = base == "big"
    assert (MT[big] * NT[big] >= 16384).all()
    want_big = (MT * NT >= 16384) & (dual == 0) & ((KB & 7 != 0) | bool(mask & SW["MFM_WIDE_NOLDS"]))
    assert (big == want_big).all()
    if mask == 0:
        # the default dispatch above 512 rows: the LDS kernel wherever its preconditions hold, else the 64 x 64 register tile
        rest = (rows > 512) & ~big
        can = (KB & 7 == 0) & ((dual == 0) | ((KBT & 3 == 0) & (KBT >= 4)))
        assert (base[rest & can] == "lds").all() and (base[rest & ~can] == "22").all()
        assert {"11", "12", "22", "big", "lds"} == set(base.tolist())


def test_the_switch_arms_reach_every_instance_between_them():
    from mfm_amd import _lib
    seen = set()
    for mask in (0, _lib.WGEMM_SW["MFM_WIDE_WM1"], _lib.WGEMM_SW["MFM_WIDE_NOLDS"] | _lib.WGEMM_SW["MFM_WIDE_RING8"]):
        for rows in (16, 272, 528, 16384):
            for KB in (3, 8):
                for NT in (3, 16):
                    for dual, KBT in ((0, 0), (1, KB)):
                        seen.add(_lib.wide_gemm_plan(rows, KB, NT, dual, KBT, mask)[0])
    assert seen == set(_lib.WGEMM)


def test_the_plans_at_the_pines_shapes():
    """the pines network (hidden 1024) at 1024 chains and d = 1024 runs every layer on the eight-wave LDS kernel, 16
    x 16 workgroups (the XCD remap applies: gridDim.x % 8 == 0 and gridDim.y % 4 == 0); the reference's default d = 1600 at 128 chains has
    KB = 100 on its x1 layer and its K^-1 product and runs everything on the 32 x 32 tile; above 512 chains those two fall to the 64 x 64
    register tile, the K^-1 product from 2624 chains on to the 128 x 64 one."""
    from mfm_amd import _lib
    p = _lib.wide_gemm_plan
    assert p(1024, 64, 64) == ("lds", 16, 16, 512)
    assert p(1024, 64, 64, True, 64) == ("lds_dual", 16, 16, 512)
    assert p(1024, 128, 64, True, 64) == ("lds_dual", 16, 16, 512)          # the joint layer: the tangent spans the sx half
    assert p(5120, 16, 64) == ("lds", 16, 80, 512)                          # the batched time branch (F = 128: K = 256)
    assert p(128, 100, 64) == ("11", 32, 4, 256) and p(128, 100, 100) == ("11", 50, 4, 256)
    assert p(128, 64, 64, True, 64) == ("11_dual", 32, 4, 256)
    assert p(1024, 100, 64) == ("22", 16, 16, 256) and p(1024, 100, 100) == ("22", 25, 16, 256)
    assert p(2608, 100, 100) == ("22", 25, 41, 256) and p(2624, 100, 100) == ("big", 25, 21, 256)
    assert p(1024, 64, 64, switches=_lib.WGEMM_SW["MFM_WIDE_WM1"]) == ("lds_wm1", 16, 16, 256)
    assert p(1024, 64, 64, switches=_lib.WGEMM_SW["MFM_WIDE_NOLDS"] | _lib.WGEMM_SW["MFM_WIDE_RING8"]) == ("22_ring8", 16, 16, 256)


def test_invalid_plan_requests_are_refused():
    from mfm_amd import _lib
    for bad in ((0, 4, 4), (24, 4, 4), (16, 0, 4), (16, 4, 0), (16, 4, 4, True, 0), (16, 4, 4, True, 5), (16, 4, 4, False, 0, 16)):
        with pytest.raises(_lib.MfmError):
            _lib.wide_gemm_plan(*bad)


def test_the_gpu_case_table_pins_what_it_says_and_names_every_instance():
    """tests/wide_gemm_cases.py, checked without a GPU: the plans its cases pin, the instance of each tall time batch, and that the named
    instances of the parity cases plus the switch arms' variants are all thirteen."""
    from mfm_amd import _lib
    from tests.wide_gemm_cases import NETS, PARITY, TALL
    named = set()
    for name, rows, act, insts, pins in PARITY:
        named |= set(insts)
        for shape, want in pins:
            assert shape[0] == rows and _lib.wide_gemm_plan(*shape)[:3] == want, (name, shape, _lib.wide_gemm_plan(*shape))
    assert named == {"11", "11_dual", "12", "12_dual", "22", "22_dual", "big", "lds", "lds_dual"}
    assert named | {"22_ring8", "22_ring8_dual", "lds_wm1", "lds_wm1_dual"} == set(_lib.WGEMM)
    for name, B, insts in TALL:
        d, F, hidden = NETS[name]
        assert isinstance(hidden, int)
        assert _lib.wide_gemm_plan(5 * B, (2 * F + 15) // 16, (hidden + 15) // 16)[0] == insts[0], (name, B)
        assert _lib.wide_gemm_plan(B, (d + 15) // 16, (hidden + 15) // 16)[0] != insts[0] or 5 * B <= 256, (name, B)
