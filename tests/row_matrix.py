"""Which template instances of the one-wave-per-chain sampler kernels the GPU tests reach.  A helper of tests/test_row_matrix.py, not a
test.

Every such kernel is launched through ``ROW_DISPATCH`` (mala.hip), which picks an instance from MAXIT in {1, 4, 16, 32} (by
ceil(d / 64)), BCRT (false: Dirichlet 0 on the chain, the compiled-in boundary; true: every other phi-four boundary and every lattice)
and, for the kernels that go through ``HMC_MASS_DISPATCH``, MASS (a diagonal inverse mass installed or handed in).  A cell is
``(MAXIT, BCRT, MASS)``.  ``ENTRY_POINTS`` lists every entry point with the case tables its GPU tests parametrize over -- the tables
themselves, imported, so a case added to or taken from one moves this grid with it -- and ``reached(entry)`` derives the cells from each
case's d, boundary, lattice side and mass flag, as ``row_instance_cases.maxit`` / ``bcrt`` do.

The mixtures have d = 2 and no boundary: they exist at MAXIT 1, BCRT false only.  That is the target's shape, not a hole: a mixture
case counts as ``MIXTURE`` (reached or not, per entry point) and never as a cell of the phi-four grid.

``FAMILIES`` are the entry points whose grid is complete: tests/test_row_matrix.py asserts that no cell of theirs is unreached.  For
every other entry point ``OPEN[entry]`` writes out the unreached cells, each with its reason; the test asserts that it is EXACTLY the
set of unreached cells, so a hole can be closed (and must then be struck here) but cannot open unnoticed."""
from tests import chees_cases as cc
from tests import ghmc_cases as gc
from tests import mclmc_cases as mcc
from tests import meads_cases as mc
from tests import pt_cases as pc
from tests import row_instance_cases as rc
from tests import test_gpu_chees, test_gpu_hmc_mass, test_gpu_hmc_run, test_gpu_mala_run, test_gpu_warmup

MAXITS = (1, 4, 16, 32)
MIXTURE = "mixture"


def cell(d, bcrt, mass=False):
    return (rc.maxit(d), bool(bcrt), bool(mass))


def _rc(names, mass=False):
    return [cell(rc.CASES[c][0], rc.bcrt(c), mass) for c in names]


def _run_table(table, names=None, mass=False):
    """The tables of tests/test_gpu_hmc_run.py, test_gpu_mala_run.py and test_gpu_hmc_mass.FAMILIES: (kind, d or row case, block tail, ...)."""
    out = []
    for name in (table if names is None else names):
        kind, d, tail = table[name][:3]
        if kind == "row":
            out += _rc([d], mass)
        elif kind == "phi4":
            out.append(cell(d, tail is not None, mass))          # any block tail is a run-time boundary (periodic, Dirichlet b, a lattice)
        elif kind == "gmm":
            out.append(MIXTURE)
    return out


def _mclmc():
    return [MIXTURE if c == "gmm4" else _rc([c])[0] for c in mcc.CASES]


def _ghmc():
    return [MIXTURE if gc.CASES[c][2] is None else cell(gc.dim(c), gc.lattice(c) > 0 or gc.CASES[c][2] != ("dirichlet", 0.0), m)
            for c in gc.CASES for m in gc.MASSES]


def _meads():
    out = []
    for c in mc.CASES:
        t = mc.target(c)
        out.append(MIXTURE if gc.CASES[t][2] is None else cell(gc.dim(t), gc.lattice(t) > 0 or gc.CASES[t][2] != ("dirichlet", 0.0), True))
    return out


def _chees(names):
    return [MIXTURE if cc.CASES[c]["target"] == "gmm4" else cell(cc.CASES[c]["d"], cc.CASES[c]["target"] != "d0", cc.CASES[c]["mass"]) for c in names]


def _pt(kernel=None):
    out = []
    for name, c in pc.CASES.items():
        if kernel is not None and c["kernel"] != kernel:
            continue
        if c["target"] == "gmm4":
            out.append(MIXTURE)
        elif c["target"] == "rc":
            out += _rc([name])
        else:
            out.append(cell(c["d"], c["target"] != "d0"))
    return out


_WARMUP_HMC = ["phi4_d64", "phi4_d100", "phi4_d256", "phi4_d64_pbc", "gmm4"] + test_gpu_warmup.ROW
_WARMUP_MALA = sorted({c for c, _, _ in test_gpu_warmup.MALA_RUNS}) + [c + "_textbook" for c in test_gpu_warmup.ROW]
# the small phi-four cases of tests/test_gpu_hmc_mass.py::test_mass_step_matches_the_float64_restatement ("phi4-<d>...": Dirichlet 0)
_MASS_STEP_SMALL = [cell(int(c.split("-")[1]), False, True) for c in test_gpu_hmc_mass.STEP_CASES if c.startswith("phi4")]

# entry point: (whether its kernel has MASS instances, the cells and MIXTURE marks of its tables' cases)
ENTRY_POINTS = {
    "mala_init": (False, _rc(rc.CASES)),
    "loglik": (False, _rc(rc.CASES)),
    "mala_step": (False, _rc(rc.CASES)),
    "hmc_step": (True, _rc(rc.CASES) + _rc(rc.MASS_CASES, True) + _MASS_STEP_SMALL),
    "mala_run": (False, _run_table(test_gpu_mala_run.CASES)),
    "hmc_run": (True, _run_table(test_gpu_hmc_run.CASES) + _run_table(test_gpu_hmc_mass.FAMILIES, mass=True)),
    "mala_warmup": (False, _run_table(test_gpu_mala_run.CASES, _WARMUP_MALA)),
    "hmc_warmup": (True, _run_table(test_gpu_hmc_run.CASES, _WARMUP_HMC) + _run_table(test_gpu_hmc_mass.FAMILIES, mass=True)),
    "hmc_warmup_window": (True, _run_table(test_gpu_hmc_mass.FAMILIES, mass=True) + _run_table(test_gpu_hmc_mass.FAMILIES)),
    "mclmc_step": (False, _mclmc()),
    "mclmc_run": (False, _mclmc()),
    "ghmc_step": (True, _ghmc()),
    "ghmc_run": (True, _ghmc()),
    "meads_step": (True, _meads()),
    "chees_step": (True, _chees(cc.CASES)),
    "hmc_run_lengths": (True, _chees(test_gpu_chees.RUN_LENGTHS)),
    "pt_hmc_run": (False, _pt("hmc")),
    "pt_mala_run": (False, _pt("mala")),
    "pt_exchange": (False, _pt()),
}
# HMC with an installed mass, as one family: the step against tests/hmc_mass_ref.py, run / warmup / window as loops of that step
HMC_MASS = sorted({c for e in ("hmc_step", "hmc_run", "hmc_warmup", "hmc_warmup_window") for c in ENTRY_POINTS[e][1] if c != MIXTURE}, key=str)

# the families whose grid is complete.  MEADS is always MASS: ``meads_step_kernel<MAXIT, BCRT>`` has no unit-mass instance
FAMILIES = ("ghmc_step", "ghmc_run", "meads_step", "chees_step", "hmc_run_lengths", "hmc_mass")


def grid(entry):
    """Every cell the entry point's kernel is compiled for (phi-four)."""
    if entry == "meads_step":
        masses = (True,)
    elif entry == "hmc_mass" or ENTRY_POINTS[entry][0]:
        masses = (False, True)
    else:
        masses = (False,)
    return {(m, b, ms) for m in MAXITS for b in (False, True) for ms in masses}


def reached(entry):
    cases = HMC_MASS if entry == "hmc_mass" else ENTRY_POINTS[entry][1]
    return {c for c in cases if c != MIXTURE}


def reaches_the_mixture(entry):
    return entry != "hmc_mass" and MIXTURE in ENTRY_POINTS[entry][1]


def unreached(entry):
    return grid(entry) - reached(entry)


_NOT_YET = "not yet"
_SMALL = "MAXIT 1 and the boundary at d <= 256 are held by tests without a case table (tests/test_gpu_mala.py, test_gpu_hmc.py, test_gpu_phi4_bc.py)"
# entry point: {unreached cell: why}.  Filling these is other work; the set may shrink, and the test fails if it grows
OPEN = {
    "mala_init": {(1, False, False): _SMALL, (1, True, False): _SMALL},
    "loglik": {(1, False, False): _SMALL, (1, True, False): _SMALL},
    "mala_step": {(1, False, False): _SMALL, (1, True, False): _SMALL},
    "hmc_step": {(1, False, False): _SMALL, (1, True, False): _SMALL,
                 (1, True, True): "the periodic d = 64 family holds it to run == single steps only (hmc_run below)"},
    "mala_run": {},
    "hmc_run": {(4, True, True): _NOT_YET, (32, True, True): _NOT_YET},
    "mala_warmup": {},
    "hmc_warmup": {(4, True, True): _NOT_YET, (32, True, True): _NOT_YET},
    "hmc_warmup_window": {(4, True, False): _NOT_YET, (4, True, True): _NOT_YET, (32, True, False): _NOT_YET, (32, True, True): _NOT_YET},
    "mclmc_step": {(1, False, False): _NOT_YET, (1, True, False): _NOT_YET, (4, True, False): _NOT_YET, (16, False, False): _NOT_YET},
    "mclmc_run": {(1, False, False): _NOT_YET, (1, True, False): _NOT_YET, (4, True, False): _NOT_YET, (16, False, False): _NOT_YET},
    "pt_hmc_run": {(1, True, False): _NOT_YET, (4, False, False): _NOT_YET, (16, True, False): _NOT_YET, (32, True, False): _NOT_YET},
    "pt_mala_run": {(1, False, False): _NOT_YET, (1, True, False): _NOT_YET, (4, True, False): _NOT_YET, (16, False, False): _NOT_YET,
                    (16, True, False): _NOT_YET, (32, False, False): _NOT_YET},
    "pt_exchange": {(1, True, False): _NOT_YET, (16, True, False): _NOT_YET},
}
