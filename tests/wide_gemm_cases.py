"""Case table of tests/test_gpu_wide_gemm.py: the networks, row counts and switch arms that put every instance of the wide family's GEMM
dispatch (wide.hip: gemm_plan) at its boundary shapes, and what each case exists for.

A layer of K inputs and N outputs is a GEMM of KB = ceil16(K) / 16 K blocks and NT = ceil16(N) / 16 feature tiles.  With hidden widths
(x1, x2) / (t1, t2) / (j1, j2), F Fourier frequencies and dimension d the forward pass launches, per evaluation,

    t1: K = 2F -> t1      t2: t1 -> t2       gate: t2 -> d       x1: d -> x1       x2: x1 -> x2 (dual: KBT = KB)
    j1: x2 + t2 -> j1 (dual: KBT = x2 / 16, the tangent's st half is zero)       j2: j1 -> j2 (dual)       out: j2 -> d (dual)

(x1's tangent comes from a buffer, so x1 is never dual), the backward pass the transposed layers (KB and NT swapped)."""

# name: (d, F, hidden as tests/gpu_util.py: hidden_lists takes it)
NETS = {
    "R": (48, 10, 48),                                       # KB = 2, 3 or 6: never LDS, always the one-block K path; NT = 3
    "Q": (192, 96, 192),                                     # KB = 12 or 24: the ring path of the register kernels, LDS only on the joint layer (NST = 3 < NS = 6)
    "A": (128, 64, 128),                                     # KB = 8 or 16: LDS everywhere, gridDim.x = 2: remap off
    "X": (64, 64, ([64, 64], [64, 64], [512, 512])),         # N = 512: gridDim.x = 8, remap on when gridDim.y % 4 == 0; joint KB = 8, KBT = 4
    "M": (64, 64, ([64, 32], [64, 96], [128, 128])),         # joint KB = 8, KBT = 2: dual LDS refused -> <2,2,true> with KBT < KB, KBT % 4 != 0
    "M4": (64, 64, ([64, 64], [64, 64], [128, 128])),        # joint KB = 8, KBT = 4: dual LDS with NST = 1 < NS = 2
    "W": (48, 10, 256),                                      # NT = 16: "big" at 16384 rows on the K = 20 / K = 48 forward and the two N = 48 backward GEMMs
}

# (network, rows, activation, instances the case is named for, plans it pins: ((rows, KB, NT, dual, KBT), (instance, gridDim.x, gridDim.y)))
# relu up to 528 rows (the production activation); tanh from 1008 on (among > 1e7 float32 pre-activations one within rounding of the ReLU
# kink is expected, and it flips a whole tangent row); gelu twice, so that the pre-activation copy P and the mask_is_pre backward path see
# the register kernel and the LDS kernel
PARITY = [
    ("R", 16, "relu", ("11", "11_dual"), [((16, 6, 3, 1, 3), ("11_dual", 2, 1))]),
    ("R", 48, "relu", ("11", "11_dual"), [((48, 3, 3, 0, 0), ("11", 2, 2))]),                          # MT = 3: the second wave row of the last workgroup is empty
    ("R", 256, "relu", ("11", "11_dual"), [((256, 3, 3, 0, 0), ("11", 2, 8))]),
    ("R", 272, "relu", ("12", "12_dual"), [((272, 3, 3, 1, 3), ("12_dual", 1, 9))]),                   # MT = 17, NT = 3 of the 4 a workgroup holds
    ("R", 512, "relu", ("12", "12_dual"), [((512, 6, 3, 1, 3), ("12_dual", 1, 16))]),
    ("R", 528, "relu", ("22", "22_dual"), [((528, 6, 3, 1, 3), ("22_dual", 1, 9))]),                   # MT = 33: one live tile in the last workgroup row
    ("R", 528, "gelu", ("22", "22_dual"), []),
    ("R", 1008, "tanh", ("22", "22_dual"), [((1008, 3, 3, 0, 0), ("22", 1, 16))]),                     # MT = 63
    ("Q", 272, "relu", ("12", "12_dual"), [((272, 24, 12, 1, 12), ("12_dual", 3, 9))]),                # the ring path of <1,2>, tangent prefix KBT < KB
    ("Q", 528, "relu", ("22", "22_dual", "lds", "lds_dual"), [((528, 12, 12, 1, 12), ("22_dual", 3, 9)), ((528, 24, 12, 1, 12), ("lds_dual", 3, 9))]),
    ("Q", 1024, "tanh", ("22", "22_dual", "lds", "lds_dual"), []),
    ("A", 256, "relu", ("11", "11_dual"), [((256, 16, 8, 1, 8), ("11_dual", 4, 8))]),                  # the ring path of <1,1>
    ("A", 512, "relu", ("12", "12_dual"), []),
    ("A", 528, "relu", ("lds", "lds_dual"), [((528, 8, 8, 0, 0), ("lds", 2, 9))]),                      # the last row tile holds 16 rows; remap off
    ("A", 1008, "gelu", ("lds", "lds_dual"), [((1008, 16, 8, 1, 8), ("lds_dual", 2, 16))]),             # last row tile 48 rows
    ("A", 1024, "tanh", ("lds", "lds_dual"), []),
    ("X", 528, "relu", ("lds", "lds_dual", "22", "22_dual"), [((528, 8, 32, 1, 4), ("lds_dual", 8, 9))]),      # gridDim.x = 8 but gridDim.y = 9: remap off
    ("X", 1008, "tanh", ("lds", "lds_dual", "22", "22_dual"), [((1008, 8, 32, 1, 4), ("lds_dual", 8, 16)), ((1008, 32, 32, 1, 32), ("lds_dual", 8, 16))]),   # remap on, last tile partial
    ("X", 1024, "tanh", ("lds", "lds_dual"), [((1024, 32, 32, 0, 0), ("lds", 8, 16))]),                 # remap on, every tile full
    ("M", 528, "relu", ("22_dual", "lds", "lds_dual"), [((528, 8, 8, 1, 2), ("22_dual", 2, 9)), ((528, 8, 8, 0, 0), ("lds", 2, 9))]),
    ("M", 1008, "tanh", ("22_dual", "lds", "lds_dual"), []),
    ("M4", 528, "relu", ("lds", "lds_dual"), [((528, 8, 8, 1, 4), ("lds_dual", 2, 9))]),
    ("M4", 1008, "tanh", ("lds", "lds_dual"), []),
    ("W", 16384, "tanh", ("big", "lds", "lds_dual"), [((16384, 2, 16, 0, 0), ("big", 4, 128)), ((16384, 3, 16, 0, 0), ("big", 4, 128)), ((16384, 16, 3, 0, 0), ("lds", 1, 256))]),
]

# switch arms of the cross-instance equality test (latched at mfm_create)
ARMS = {
    "default": (),
    "no_small": ("MFM_WIDE_NO_SMALL_TILES",),
    "nolds": ("MFM_WIDE_NOLDS",),
    "nolds_no_small": ("MFM_WIDE_NOLDS", "MFM_WIDE_NO_SMALL_TILES"),
    "nolds_ring8": ("MFM_WIDE_NOLDS", "MFM_WIDE_RING8"),
    "wm1": ("MFM_WIDE_WM1",),
}
ALL_SWITCHES = ("MFM_WIDE_NOLDS", "MFM_WIDE_NO_SMALL_TILES", "MFM_WIDE_WM1", "MFM_WIDE_RING8")
# (network, rows, activation, distinct sets): what the arms differ in at each -- R 272: <1,2> against <2,2>; Q 528: LDS on the joint layer against the rings
# of 4 and of 8 (KB = 24, KBT = 12: ring 8 serves only the non-dual launches); A 528 / A 1008: LDS (8 and 4 waves) against both rings; X 1008:
# the remapped LDS grid against the register tile; last: the number of distinct instance sets the six arms must show
EQUALITY = [("R", 272, "relu", 2), ("Q", 528, "relu", 4), ("A", 528, "relu", 4), ("A", 1008, "tanh", 4), ("X", 1008, "tanh", 4)]

# the tall time batch: (network, chains, instances the 5 B-row time branch must show)
TALL = [("R", 48, ("11",)), ("R", 64, ("12",)), ("R", 112, ("22",)), ("A", 112, ("lds",)), ("W", 3280, ("big",))]
