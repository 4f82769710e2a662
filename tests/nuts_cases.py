"""The (instance, launch geometry) table of the No-U-turn tests: tests/test_nuts_cases.py checks its conditions on the reference alone
(CPU), tests/test_gpu_nuts_instances.py runs the kernel on it.  Not a test.

``nuts.hip`` holds one transition in 24 instances (MAXIT 1 / 2 / 4 by dim, the phi-four boundary read at run time, the mass; step, run
and warmup kernels) and launches 1 to 4 chains per workgroup by ``(dim, max_tree_depth)``.  Each case names the instance and the
geometry it exists for; ``waves`` is the chains per workgroup it is MEANT to run under, asserted through ``mfm_nuts_launch_plan`` so that
a change of the budget cannot silently move it elsewhere.

Every case: 64 chains, the reference's own state after 30 burn-in transitions at limit 6, then 3 transitions under the case's limit
(tests/nuts_util.py: ``burned``).  The table's conditions (tests/test_nuts_cases.py): borderline share <= 0.25 in every transition, no
divergent burn-in, both directions drawn, and per case what it is for.

Findings that shaped it (reference alone):
* with the mass, d >= 192 diverges from the initial draw at a step size of 0.03 or more: d192 runs 0.025 under the mass;
* at d = 256 with the mass and uncut trees the step sizes 0.015, 0.02 and 0.025 all gave borderline shares of 0.25 to 0.39, over the
  cap: d = 256 at the deep limit is unit mass only, and its mass instances at that geometry are covered by the placement test;
* the 12 x 12 periodic lattice at 0.03 (unit) and 0.02 (mass) sat at 0.23 to 0.25, too fragile, and the 16 x 16 lattice at 0.03 reached
  0.30: neither is here.

POSITION BOUND.  The common bound ``3e-6 max(1, |x|max)`` was set for trees of at most 63 leapfrog steps; these run to 700 and more.
Per case and mass ``nuts_util.position_probe`` repeats the reference's pass with every leaf's float32 gradient scaled by ``1 +- 2^-22``
and measures how far the end moves on the chains whose tree is unchanged; the case's bound is ``max(common bound, 4 x that)``, 4 being
the usual margin over a measured figure (the kernel's float32 gradient arithmetic is a few last places from the rounded float64
gradient, not one).  The probe must change no non-borderline chain's depth or leapfrog count.  Measured figures: the table in DESIGN.md
section 4.14."""
from collections import namedtuple

from tests import nuts_util as nu

# tail: what follows {a, beta} in the target block (nuts_util); eps: (unit mass, log_spaced_mass), None where the case does not run;
# limit: max_tree_depth; waves: chains per workgroup; deep: the case that must realize depth >= 9
Case = namedtuple("Case", "d tail eps limit waves deep")
DBC, LAT_DBC, LAT_PBC = (0.0, 0.7), (0.0, 0.7, 2.0), (1.0, 0.0, 2.0)

CASES = {
    # MAXIT 1, slots up to 7 and runs of trailing ones up to 8, k_tree's children 6 to 8: depths 5 to 9, up to 767 leapfrog steps
    "deep": Case(64, None, (0.01, 0.01), 16, 2, True),
    "one-wave": Case(64, None, (0.03, 0.03), 12, 1, False),
    # MAXIT 2: the ragged second row and the full one
    "maxit2-ragged": Case(100, None, (0.03, 0.03), 10, 2, False),
    "maxit2-full": Case(128, None, (0.03, 0.03), 14, 1, False),
    # MAXIT 4 with a dead fourth row (every jj < d guard works), 127,040 B of LDS in one workgroup
    "three-rows": Case(130, None, (0.03, 0.03), 16, 4, False),
    "d192": Case(192, None, (0.04, 0.025), 10, 1, False),
    "d256-two": Case(256, None, (0.04, None), 14, 2, False),
    # the boundary read at run time (BCRT) and the lattice, through row_value_grad<MAXIT, BCRT>
    "dbc-128": Case(128, DBC, (0.03, 0.03), 6, 2, False),
    "lat-36": Case(36, LAT_DBC, (0.03, 0.03), 6, 4, False),
    "lat-144": Case(144, LAT_DBC, (0.03, 0.03), 8, 3, False),
    "lat-144-pbc": Case(144, LAT_PBC, (0.05, 0.05), 8, 3, False),
    # no checkpoint slot at all: a slab of 0 bytes
    "depth-one": Case(64, None, (0.03, 0.03), 1, 4, False),
}
RUNS = [(name, mass) for name, c in CASES.items() for mass in (False, True) if c.eps[mass] is not None]
RUN_IDS = [f"{name}-{'mass' if mass else 'unit'}" for name, mass in RUNS]

# the placement test's geometries (device only): (d, limit, mass, step size, chains per workgroup).  (193, 14) is the largest LDS
# request any (dim, limit) makes, 163,824 B of a CU's 163,840 (tests/test_nuts_plan_host.py).  The last two are there because a slab
# stride that is one slot short makes wave w's LAST slot wave w + 1's first, and only a tree that reaches the limit's last doubling
# stores there: at limits 5 and 6 most trees do (the test asserts it), at 10 and more none does.
PLACEMENT = [(64, 10, False, 0.03, 4), (64, 11, False, 0.03, 3), (64, 12, False, 0.03, 1), (64, 16, False, 0.03, 2),
             (130, 16, True, 0.03, 4), (256, 14, True, 0.02, 2), (193, 14, False, 0.03, 4), (64, 5, False, 0.03, 4), (256, 6, True, 0.02, 3)]
LIMIT_REACHED = 6          # placement geometries with a limit up to this must have trees that reach it


def spec(name, mass):
    """The arguments of ``nuts_util.burned`` / ``position_probe`` for a run of the table."""
    c = CASES[name]
    return ("phi4", c.d, c.tail, c.eps[mass], c.limit, mass)


def position_floor(name, mass):
    """The case's own position bound (module docstring): 4 x the probe's displacement; ``_compare`` takes the larger of it and the
    common bound."""
    return 4.0 * nu.position_probe(*spec(name, mass))[0]
