"""The cases of tests/test_gpu_ghmc.py and tests/test_ghmc_cases.py: ``mfm_ghmc_*`` (mfm_amd/csrc/ghmc.hip) on every dispatch instance,
at the smallest shape that reaches it.

case          chains  instance
gmm4          16      d = 2: MAXIT 1, the mixture path
d64_d0        16      MAXIT 1, a full lane group
d65_d0        16      MAXIT 4, a ragged last lane group (minv in registers with mass)
d256_d0       32      MAXIT 4, its last dimension; eight workgroups
d320_d0       16      MAXIT 16: with mass, minv read from memory at every use
d64_pbc       16      MAXIT 1 with the run-time boundary (BCRT)
d1100_d0      16      MAXIT 32 (draws and exp called out of line); 16 chains: a context takes a multiple of 16
d65_pbc       16      MAXIT 4 with the run-time boundary: the wrap-around neighbours of a ragged last lane group
32x32_db      16      MAXIT 16, its last dimension, with the run-time boundary: a lattice (d = 1024) inside a frame held at 0.5
d1025_pbc     16      MAXIT 32 with the run-time boundary: the last lane group holds one element, whose right neighbour is element 0

The last three (``ROW_CASES``) are cases of tests/row_instance_cases.py: its targets, target blocks and start states.  A finding: on the
smaller framed lattice 17x17_db the step sizes ``scan`` picks (0.032 / 0.026) leave the alpha = 1 transition from the start state with
acceptance rates of at most 0.42 / 0.53 in the restatement (the chains of a framed lattice start from one profile, so their rates lie
close together), and the comparison with HMC at one leapfrog step, whose slice variable is 0.5, would have no chain accepted by both
samplers to compare.  ``scan`` therefore also asks for two such chains (``alpha_one_both``), and the lattice is 32x32_db.

Every case runs at unit metric (``mass`` False) and with the diagonal inverse mass ``inverse_mass(d)`` (True).  The phi-four start states
are tests/row_instance_cases.py's construction (a smooth state near a mode plus (0.5 / d) N(0, 1)); ``gmm4`` is tests/mclmc_cases.py's.

``states(case, mass)``: the ``N_STEPS`` states the transitions start from -- the restatement's own trajectory in the device's number
formats (tests/ghmc_ref.py with ``float32_positions=True`` and the gradient in float32 arithmetic), from ``mfm_ghmc_init``'s momenta and
slice variables.  The GPU test uploads each of them, makes one transition on the device and compares with the float64 restatement from
the SAME state, so what this module checks on a CPU is what the GPU test relies on.

``STEP_SIZES[case][mass]``: chosen by ``scan`` on the restatement so that the case's transitions hold accepted and rejected proposals
and no decision is borderline.  ``TOLERANCE[case][mass]`` = (x, p, logp, dH, s): 4 x the largest difference between the float64
restatement and its ``float32_positions=True`` variant over the case's transitions, each from the same state -- what the device's number
formats cost, whatever the kernel; rounded up to two digits.  Both tables are written by ``measure`` (run this module), not by hand;
tests/test_ghmc_cases.py recomputes them and asserts that no accept decision has ``|s|`` within the dH tolerance of ``exp(-dH)``
(relative: ``| log|s| + dH | > tol``)."""
import functools

import numpy as np

from oracle import prng, targets
from tests import ghmc_ref as ref
from tests import mclmc_cases as mcc
from tests import row_instance_cases as rc
from tests.phi4_bc_oracle import PhiFourBC

A, TBETA = 0.1, 20.0
N_STEPS = 3
ALPHA, DELTA = 0.3, 0.15
# case: (d, chains, boundary)
CASES = {
    "gmm4": (2, 16, None),
    "d64_d0": (64, 16, ("dirichlet", 0.0)),
    "d65_d0": (65, 16, ("dirichlet", 0.0)),
    "d256_d0": (256, 32, ("dirichlet", 0.0)),
    "d320_d0": (320, 16, ("dirichlet", 0.0)),
    "d64_pbc": (64, 16, ("pbc", 0.0)),
    "d1100_d0": (1100, 16, ("dirichlet", 0.0)),
}
ROW_CASES = ("d65_pbc", "32x32_db", "d1025_pbc")       # of tests/row_instance_cases.py
# the seeds count along this order: the cases above by name, then the row cases in the order they were added
SEED_ORDER = sorted(CASES) + list(ROW_CASES)
for _c in ROW_CASES:
    CASES[_c] = (rc.CASES[_c][0], rc.N_CHAINS, rc.BOUNDARIES[rc.CASES[_c][2]])
MASSES = (False, True)

# case: {mass: step size} -- written by ``measure``
STEP_SIZES = {
    "gmm4": {False: 1.0, True: 1.0},
    "d64_d0": {False: 0.032, True: 0.026},
    "d65_d0": {False: 0.032, True: 0.026},
    "d256_d0": {False: 0.0083, True: 0.0083},
    "d320_d0": {False: 0.0083, True: 0.0083},
    "d64_pbc": {False: 0.026, True: 0.022},
    "d1100_d0": {False: 0.0032, True: 0.0032},
    "d65_pbc": {False: 0.026, True: 0.026},
    "32x32_db": {False: 0.015, True: 0.012},
    "d1025_pbc": {False: 0.0032, True: 0.0032},
}

# case: {mass: (x, p, logp, dH, s)} -- written by ``measure``
TOLERANCE = {
    "gmm4": {False: (1.9e-06, 9.5e-07, 3.6e-06, 3.4e-06, 2.1e-06), True: (1.9e-06, 9.5e-07, 3.9e-06, 4.4e-06, 3.9e-06)},
    "d64_d0": {False: (2.6e-07, 2e-06, 1.3e-05, 1.6e-05, 8.9e-06), True: (2.4e-07, 1.9e-06, 2.6e-05, 2.4e-05, 1.2e-05)},
    "d65_d0": {False: (2.6e-07, 1.7e-06, 1.8e-05, 2e-05, 8.4e-06), True: (2.5e-07, 2e-06, 2.4e-05, 2.6e-05, 9.7e-06)},
    "d256_d0": {False: (2.5e-07, 2.4e-06, 4.4e-05, 4.2e-05, 1.5e-05), True: (2.5e-07, 2.4e-06, 5.9e-05, 6.8e-05, 4.5e-05)},
    "d320_d0": {False: (2.5e-07, 2.8e-06, 4.7e-05, 3.7e-05, 2.2e-05), True: (2.4e-07, 2.9e-06, 2.9e-05, 6.6e-05, 1.3e-05)},
    "d64_pbc": {False: (2.5e-07, 1.7e-06, 1.6e-05, 1.4e-05, 7.9e-06), True: (2.6e-07, 1.5e-06, 2.4e-05, 2.9e-05, 7.4e-06)},
    "d1100_d0": {False: (2.4e-07, 3.5e-06, 8.3e-05, 0.00014, 5.7e-05), True: (2.5e-07, 3.5e-06, 8.4e-05, 0.00015, 3.7e-05)},
    "d65_pbc": {False: (2.5e-07, 1.9e-06, 2.9e-05, 2.7e-05, 1.8e-05), True: (2.6e-07, 1.8e-06, 2e-05, 2.7e-05, 8.8e-06)},
    "32x32_db": {False: (2.5e-07, 1.5e-06, 6.9e-05, 5.7e-05, 2.1e-05), True: (2.5e-07, 1.3e-06, 4.4e-05, 4e-05, 2.8e-05)},
    "d1025_pbc": {False: (2.5e-07, 3.9e-06, 0.00012, 0.00017, 5.7e-05), True: (2.5e-07, 3.7e-06, 0.00021, 0.00027, 9.6e-05)},
}


def dim(case):
    return CASES[case][0]


def lattice(case):
    """The lattice side, or 0 on the chain."""
    return rc.CASES[case][1] if case in ROW_CASES else 0


def n_chains(case):
    return CASES[case][1]


def inverse_mass(d):
    """A non-unit diagonal in [0.5, 2] without a period that divides 64."""
    j = np.arange(d)
    return 0.5 + 1.5 * ((7 * j) % 11) / 10.0


def minv(case, mass):
    return inverse_mass(dim(case)) if mass else None


def oracle_dist(case):
    d, _, bc = CASES[case]
    if case in ROW_CASES:
        return rc.oracle_dist(case)
    return mcc.gmm4_dist() if bc is None else PhiFourBC(d, A, TBETA, bc)


def block(case):
    """The target block to hand ``set_target`` after {a, beta}, or None (Dirichlet 0, or the mixture)."""
    if case in ROW_CASES:
        return rc.block(case)
    bc = CASES[case][2]
    return oracle_dist(case).block() if bc is not None and bc[0] == "pbc" else None


@functools.lru_cache(maxsize=None)
def start_state(case):
    """[chains, d] float32."""
    d, n, bc = CASES[case]
    if bc is None:
        return mcc.start_state("gmm4")[:n]
    if case in ROW_CASES:
        return rc.start_state(case)
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[:, None]
    base = sign * np.ones((1, d)) if bc[0] == "pbc" else sign * np.sin(np.pi * (np.arange(d) + 1) / (d + 1))[None]
    noise = prng.normal_rows(prng.split(prng.PRNGKey(4200 + SEED_ORDER.index(case)), n), d)
    return (base + 0.5 / d * noise).astype(np.float32)


def value_and_grad(case):
    return targets.Tempered(oracle_dist(case), 1.0).value_and_grad


def grad32(case, x):
    """The device's phi-four gradient formula on the chain in float32 arithmetic (tests/row_instance_cases.grad32, at beta = 1)."""
    f = np.float32
    if case in ROW_CASES:
        return rc.grad32(case, x, 1.0)
    d, _, bc = CASES[case]
    x = np.asarray(x, f)
    coef = f(A * d)
    if bc[0] == "pbc":
        l, r = np.roll(x, 1, 1), np.roll(x, -1, 1)
    else:
        e = np.full((x.shape[0], 1), f(bc[1]))
        l, r = np.concatenate([e, x[:, :-1]], 1), np.concatenate([x[:, 1:], e], 1)
    lap = f(2) * x - l - r
    return f(1) * (-f(TBETA) * (coef * lap - x * (f(1) - x * x) / coef))


def value_and_grad_f32(case):
    """The target as the device evaluates it at a float32 position: the log-density in float64, the gradient in float32 arithmetic."""
    if case == "gmm4":
        return mcc.value_and_grad_f32("gmm4")
    dist = oracle_dist(case)
    return lambda x: (dist.loglik(x), grad32(case, x.astype(np.float32)).astype(np.float64))


def init_key(case):
    return prng.PRNGKey(5200 + SEED_ORDER.index(case))


def step_key(case, j):
    """The key of transition j and the per-chain keys ``mfm_ghmc_step`` derives from it."""
    key = prng.split(prng.PRNGKey(6200 + SEED_ORDER.index(case)), N_STEPS)[j]
    return key, ref.chain_keys(key, n_chains(case))


def _pair(case, mass, st, j, eps):
    """Transition j from ``st`` (position float32-valued) by the float64 restatement and by its device-format variant."""
    keys = step_key(case, j)[1]
    m = minv(case, mass)
    vg, vg32 = value_and_grad(case), value_and_grad_f32(case)
    lp, g = vg(st.position)
    r64 = ref.step(keys, st._replace(logdensity=lp, logdensity_grad=g), vg, eps, ALPHA, DELTA, m)
    lp32, g32 = vg32(st.position)
    r32 = ref.step(keys, st._replace(logdensity=lp32, logdensity_grad=g32), vg32, eps, ALPHA, DELTA, m, float32_positions=True)
    return r64, r32


def walk(case, mass, eps=None):
    """Per transition: (start state, (state, info) of the float64 restatement, (state, info) of the device-format variant)."""
    eps = STEP_SIZES[case][mass] if eps is None else eps
    st = ref.init(start_state(case).astype(np.float64), value_and_grad(case), init_key(case), minv(case, mass), n_chains(case))
    out = []
    for j in range(N_STEPS):
        r64, r32 = _pair(case, mass, st, j, eps)
        out.append((st, r64, r32))
        st = r32[0]
    return out


def states(case, mass):
    return [w[0] for w in walk(case, mass)]


def distance(case, mass, eps=None):
    """The largest differences (x, p, logp, dH, s) between the two restatements over the case's transitions."""
    out = np.zeros(5)
    for _, (s64, i64), (s32, i32) in walk(case, mass, eps):
        same = i64.is_accepted == i32.is_accepted
        out = np.maximum(out, [np.abs(i64.proposed_position - i32.proposed_position).max(), np.abs(s64.momentum - s32.momentum)[same].max(),
                               np.abs(s64.logdensity - s32.logdensity)[same].max(), np.abs(i64.energy_change - i32.energy_change).max(),
                               np.abs(s64.slice - s32.slice)[same].max()])
    return tuple(out)


def margins(case, mass, eps=None):
    """Per transition ``| log|s| + dH |`` of every chain (the decision's distance from its boundary, on the log scale, float64
    restatement) and the decisions."""
    m, acc = [], []
    for _, (s64, i64), _ in walk(case, mass, eps):
        with np.errstate(divide="ignore"):
            m.append(np.abs(np.log(np.abs(i64.slice_after_drift)) + i64.energy_change))
        acc.append(i64.is_accepted)
    return np.stack(m), np.stack(acc)


def alpha_one_both(case, mass, eps=None):
    """How many chains the alpha = 1 transition from the start state with s = 0 (|s| = 0.5 after the drift) AND HMC at one leapfrog step on
    the same keys both accept, in the restatement: what tests/test_gpu_ghmc.py's comparison of the two has to compare."""
    eps = STEP_SIZES[case][mass] if eps is None else eps
    vg = value_and_grad(case)
    st = ref.init(start_state(case).astype(np.float64), vg, init_key(case), minv(case, mass), n_chains(case))
    keys = step_key(case, 0)[1]
    _, info = ref.step(keys, st._replace(slice=np.zeros(n_chains(case))), vg, eps, 1.0, 0.5, minv(case, mass))
    u = prng.uniform_rows(prng.split_rows(keys, 2)[:, 1])
    return int((info.is_accepted & (u < info.acceptance_rate)).sum())


def _up2(v):
    """v rounded up to two significant digits."""
    if v == 0:
        return 0.0
    e = int(np.floor(np.log10(v))) - 1
    return float(f"{np.ceil(v / 10.0 ** e) * 10.0 ** e:.2g}")


def tolerance(case, mass, eps=None):
    return tuple(_up2(4.0 * v) for v in distance(case, mass, eps))


def scan(case, mass, grid):
    """Of the step sizes of ``grid`` whose decisions are all further than 10 x the dH tolerance from their boundary and at which the
    alpha = 1 transition has at least 2 chains accepted by GHMC and HMC alike: the one with the most even mix of accepted and rejected
    proposals (at least 2 of each), or None."""
    best, best_score = None, 1
    for eps in grid:
        with np.errstate(all="ignore"):
            m, acc = margins(case, mass, eps)
            tol = tolerance(case, mass, eps)[3]
        score = min(acc.sum(), (~acc).sum())
        if score > best_score and np.isfinite(m).all() and m.min() > 10 * tol and alpha_one_both(case, mass, eps) >= 2:
            best, best_score = float(eps), score
    return best


def measure(names=None):
    """Prints the two tables."""
    grid = [float(f"{10.0 ** (-3 + k / 12):.2g}") for k in range(37)]       # 1e-3 .. 1
    names = names or list(CASES)
    sizes = {c: {m: scan(c, m, grid) for m in MASSES} for c in names}
    for c in names:
        print(f'    "{c}": {sizes[c]},', flush=True)
    for c in names:
        print(f'    "{c}": {({m: tolerance(c, m, sizes[c][m]) for m in MASSES})},', flush=True)


if __name__ == "__main__":
    import sys
    measure(sys.argv[1:])
