"""The cases of tests/test_gpu_meads.py and tests/test_meads_ref.py: ``mfm_meads_warmup`` (mfm_amd/csrc/ghmc.hip).

case       d    B    n_valid  K   S  n_iter  what it reaches
d65_k4     65   32   32       4   0  4       MAXIT 4 with a ragged lane group, d_pad > d, one Gram tile per fold
n_valid    64   32   24       4   0  3       n_valid < B: rows 24 .. 31 stepped with fold 0's parameters and never read
k2         64   16   16       2   0  3       two folds: each steers the other
shuffle    64   16   16       4   2  5       the membership redrawn before iterations 3 and 5
m80        64   320  320      4   0  2       m = 80: the Gram spans two tiles per side with a ragged edge, so off-diagonal tiles count twice
unstable   64   16   16       2   0  4       fold 0 starts with all chains at ONE point: its first statistics are not finite, fold 1 keeps
                                             step0 = 1, far beyond the stability limit, and rejects everything at t = 1; then it recovers
gmm4_k2    2    16   16       2   0  24      the mixture path, d = 2 (d_pad = 32); the only case whose iterations outlast the floor
                                             1 / (t eps) of gamma, so that 1 / sqrt(lam(Y)) sets alpha

d320_k4    320  32   32       4   0  3       MAXIT 16: the out-of-line trajectory; d_pad = 320, a Gram K-loop of 10 chunks, 5 column blocks
d1100_k4   1100 32   32       4   0  3       MAXIT 32; d_pad = 1120; the closing pass's inverse mass beyond d = 1024
d65_pbc_k4 65   32   32       4   0  3       the run-time boundary (BCRT) at MAXIT 4: the step kernel's own halo cells wrap around
32x32_k4   1024 32   32       4   0  3       BCRT at MAXIT 16, its last dimension: a lattice inside a frame held at 0.5
k6         64   48   48       6   0  3       six folds of m = 8: waves 0 and 1 of the update kernel own two folds each (f and f + 4), and the roll
                                             carries fold 3's statistics (wave 3) to fold 4 (wave 0's second) and fold 5's (wave 1) to fold 0
d64_pbc_k4 64   32   32       4   0  3       BCRT at MAXIT 1
d1025_pbc_k4 1025 32 32       4   0  4     BCRT at MAXIT 32: the last lane group holds one element, whose right neighbour is element 0

phi-four from tests/ghmc_cases.py's start states after a short walk (``start_state``); ``step0`` / ``alpha0`` are 0.01 / 0.5 except where
stated (d320_k4: 0.005, d1100_k4 and d1025_pbc_k4: 0.002 -- below the targets' stability limits, so that the first iteration moves chains).

``reference(case)``: the restatement's own warmup in the device's number formats (tests/meads_ref.py with ``float32_positions=True`` and
the float32 gradient).  ``TOLERANCE[case]`` = (lam(Z), lam(Y), dH): for the two eigenvalue estimates the RELATIVE tolerance, 4 x the
largest relative difference between the float64 statistic and the one formed from Y, Z rounded to float32 (what the staged tiles hold)
over the reference's iterations and folds, plus the float32 dot-product bound of the Gram entries, e_ij = (d + 8) 2^-23 |x_i| |x_j|
(svgd.hip: any summation order), carried through the sum of squares: sum_{i != j} (2 |S_ij| e_ij + e_ij^2) over the sum itself; for dH
4 x the largest difference between the float64 transition and its device-format variant from the same state.  Written by ``measure``
(run this module); tests/test_meads_ref.py recomputes it.

The parameters follow from the estimates: eps = 0.5 / sqrt(lam_z) has half the relative error of lam_z, and with u = eps gamma,
alpha = 1 - exp(-2 u) moves by 2 u exp(-2 u) <= 1 / e times the relative error of u, which is at most that of lam_z plus that of lam_y
(none where the floor 1 / (t eps) is active: then u = 1 / t exactly).  ``param_tolerance`` states these: relative rel_z for eps,
absolute rel_z + rel_y for alpha, half that for delta."""
import functools

import numpy as np

from oracle import prng
from tests import ghmc_cases as gc
from tests import ghmc_ref
from tests import meads_ref as ref

# case: (target case of ghmc_cases, B, n_valid, K, shuffle_every, n_iter, step0, alpha0)
CASES = {
    "d65_k4": ("d65_d0", 32, 32, 4, 0, 4, 0.01, 0.5),
    "n_valid": ("d64_d0", 32, 24, 4, 0, 3, 0.01, 0.5),
    "k2": ("d64_d0", 16, 16, 2, 0, 3, 0.01, 0.5),
    "shuffle": ("d64_d0", 16, 16, 4, 2, 5, 0.01, 0.5),
    "m80": ("d64_d0", 320, 320, 4, 0, 2, 0.01, 0.5),
    "unstable": ("d64_d0", 16, 16, 2, 0, 4, 1.0, 0.5),
    "gmm4_k2": ("gmm4", 16, 16, 2, 0, 24, 0.5, 0.5),
}
NEW_CASES = {
    "d320_k4": ("d320_d0", 32, 32, 4, 0, 3, 0.005, 0.5),
    "d1100_k4": ("d1100_d0", 32, 32, 4, 0, 3, 0.002, 0.5),
    "d65_pbc_k4": ("d65_pbc", 32, 32, 4, 0, 3, 0.01, 0.5),
    "32x32_k4": ("32x32_db", 32, 32, 4, 0, 3, 0.01, 0.5),
    "k6": ("d64_d0", 48, 48, 6, 0, 3, 0.01, 0.5),
    "d64_pbc_k4": ("d64_pbc", 32, 32, 4, 0, 3, 0.01, 0.5),
    # (4 iterations: over 3 a chain's | log|s| + dH | is 7 x the dH tolerance, short of the 10 x the comparison of decisions needs)
    "d1025_pbc_k4": ("d1025_pbc", 32, 32, 4, 0, 4, 0.002, 0.5),
}
# the seeds count along this order: the first seven cases by name, then the later ones in the order they were added
SEED_ORDER = sorted(CASES) + list(NEW_CASES)
CASES.update(NEW_CASES)
# (case, iteration, receiving fold) whose parameters are KEPT on purpose
KEPT = {("unstable", 1, 1)}

# case: (lam(Z) relative, lam(Y) relative, dH) -- written by ``measure``
TOLERANCE = {
    "d65_k4": (9.9e-05, 2e-05, 3e-05),
    "n_valid": (8.7e-05, 2e-05, 2.8e-05),
    "k2": (8.3e-05, 1.9e-05, 2.3e-05),
    "shuffle": (0.00027, 2.1e-05, 3.9e-05),
    "m80": (8.1e-05, 1.9e-05, 3.2e-05),
    "unstable": (8.6e-05, 8.1e-05, 1.9e-05),
    "gmm4_k2": (3.8e-06, 3.1e-06, 9.1e-06),
    # the float32 dot-product bound (d + 8) 2^-23 per Gram entry is 3.9e-5 at d = 320 and 1.3e-4 at d = 1100, against 8.7e-6 at d = 65
    "d320_k4": (0.00091, 8.3e-05, 9.4e-05),
    "d1100_k4": (0.0052, 0.00028, 0.00047),
    "d65_pbc_k4": (0.00012, 1.8e-05, 4.9e-05),
    "32x32_k4": (0.0052, 0.0017, 0.00016),
    "k6": (0.00011, 2e-05, 2.7e-05),
    "d64_pbc_k4": (0.00011, 1.8e-05, 3.9e-05),
    "d1025_pbc_k4": (0.0066, 0.00025, 0.00063),
}


def target(case):
    return CASES[case][0]


def dim(case):
    return gc.dim(target(case))


def shape(case):
    """(B, n_valid, K, shuffle_every, n_iter, step0, alpha0)."""
    return CASES[case][1:]


def run_key(case):
    return prng.PRNGKey(7200 + SEED_ORDER.index(case))


def shuffle_key(case):
    return prng.PRNGKey(7300 + SEED_ORDER.index(case))


def init_key(case):
    return prng.PRNGKey(7400 + SEED_ORDER.index(case))


# transitions, step size, alpha of the walk that spreads the start states; the step size is the target case's own where that is smaller
THERMALISE = (60, 0.02, 0.3)


@functools.lru_cache(maxsize=None)
def start_state(case):
    """[B, d] float32.  The target case's start states sit AT a mode (gradients near zero, a fold's chains on one line): an ensemble no
    warmup is started from, on which the eigenvalue estimates say nothing of the target.  So they are repeated up to B rows and walked
    ``THERMALISE[0]`` GHMC transitions of the float64 restatement (for the mixture: chain b's mode plus 0.5 N(0, 1) as it is)."""
    tc, B = target(case), CASES[case][1]
    base = gc.start_state(tc)
    x = np.concatenate([base] * -(-B // base.shape[0]))[:B].astype(np.float64)
    seed = 7500 + SEED_ORDER.index(case)
    if tc != "gmm4":
        vg = gc.value_and_grad(tc)
        n, eps, alpha = THERMALISE
        eps = min(eps, gc.STEP_SIZES[tc][False])
        st, _ = ghmc_ref.run(prng.PRNGKey(seed), ghmc_ref.init(x, vg, prng.PRNGKey(seed + 50), None, B), vg, eps, alpha, alpha / 2, n)
        x = st.position
    if case == "unstable":
        m = CASES[case][2] // CASES[case][3]
        x = x.copy()
        x[:m] = x[0]                                     # fold 0: every chain at one point
    return x.astype(np.float32)


def permutations(case):
    B, n_valid, K, S, n_iter, _, _ = shape(case)
    return ref.permutations(shuffle_key(case), n_iter, S, n_valid)


def initial_state(case, vg):
    B = CASES[case][1]
    return ghmc_ref.init(start_state(case).astype(np.float64), vg, init_key(case), None, B)


@functools.lru_cache(maxsize=None)
def reference(case):
    """The restatement's warmup in the device's number formats."""
    B, n_valid, K, S, n_iter, step0, alpha0 = shape(case)
    vg32 = gc.value_and_grad_f32(target(case))
    with np.errstate(all="ignore"):
        return ref.warmup(run_key(case), initial_state(case, vg32), vg32, n_iter, n_valid, K, step0, alpha0, S, shuffle_key(case),
                          float32_positions=True)


def round32(a):
    return a.astype(np.float32).astype(np.float64)


def staged(x, g):
    """(Y, Z) of one fold in float64 and as the staged float32 tiles hold them."""
    mu = x.mean(0)
    sd = np.sqrt(((x - mu) ** 2).mean(0))
    Y, Z = (x - mu) / sd, g * sd
    return (Y, Z), (round32(Y), round32(Z))


def gram_bound(X, d):
    """The relative error the float32 dot products can leave in sum_{i != j} S_ij^2."""
    S = X @ X.T
    nrm = np.sqrt(np.diag(S))
    e = (d + 8) * 2.0 ** -23 * np.outer(nrm, nrm)
    off = ~np.eye(X.shape[0], dtype=bool)
    return float((2.0 * np.abs(S) * e + e * e)[off].sum() / (S * S)[off].sum())


def states_before(case):
    """The state before every iteration of the reference (and after the last), by re-running it with a recording hook."""
    B, n_valid, K, S, n_iter, step0, alpha0 = shape(case)
    vg32 = gc.value_and_grad_f32(target(case))
    seen = []

    def rec(t, st):
        seen.append(st)
        return st
    with np.errstate(all="ignore"):
        res = ref.warmup(run_key(case), initial_state(case, vg32), vg32, n_iter, n_valid, K, step0, alpha0, S, shuffle_key(case),
                         float32_positions=True, restart=rec)
    return seen, res


def tolerance(case):
    B, n_valid, K, S, n_iter, step0, alpha0 = shape(case)
    m, d = n_valid // K, dim(case)
    seen, res = states_before(case)
    perms = permutations(case)
    vg, vg32 = gc.value_and_grad(target(case)), gc.value_and_grad_f32(target(case))
    rel = np.zeros(2)
    bound = np.zeros(2)
    d_h = 0.0
    for t, st in enumerate(seen, start=1):
        perm = ref.perm_at(perms, t, S, n_valid)
        for f in range(K):
            rows = perm[f * m:(f + 1) * m]
            with np.errstate(all="ignore"):
                (Y, Z), (Y32, Z32) = staged(st.position[rows], st.logdensity_grad[rows])
                pairs = ((Z, Z32), (Y, Y32))
                vals = [(ref.lam(a), ref.lam(b)) for a, b in pairs]
            for q, ((a, b), (va, vb)) in enumerate(zip(pairs, vals)):
                if np.isfinite(va) and np.isfinite(vb) and va > 0:
                    rel[q] = max(rel[q], abs(va - vb) / va)
                    bound[q] = max(bound[q], gram_bound(b, d))
        # the transition of this iteration in float64 and in the device's formats, from the same state and parameters
        fold_of = np.zeros(B, np.int64)
        fold_of[perm] = np.arange(n_valid) // m
        keys = ref.step_keys(run_key(case), n_iter, t, B)
        par = [res.trace[t - 1, fold_of, q] for q in range(3)]
        minv = res.mass_trace[t - 1][fold_of]
        lp, g = vg(st.position)
        with np.errstate(all="ignore"):
            _, i64 = ghmc_ref.step(keys, st._replace(logdensity=lp, logdensity_grad=g), vg, par[0], par[1], par[2], minv)
            _, i32 = ghmc_ref.step(keys, st, vg32, par[0], par[1], par[2], minv, float32_positions=True)
        ok = np.isfinite(i64.energy_change) & np.isfinite(i32.energy_change) & (np.abs(i64.energy_change) < 30)
        if ok.any():
            d_h = max(d_h, float(np.abs(i64.energy_change - i32.energy_change)[ok].max()))
    return tuple(gc._up2(v) for v in (4 * rel[0] + bound[0], 4 * rel[1] + bound[1], 4 * d_h))


def param_tolerance(case):
    """(eps relative, alpha absolute, delta absolute) from the eigenvalue tolerances (module docstring)."""
    rz, ry, _ = TOLERANCE[case]
    return rz, rz + ry, 0.5 * (rz + ry)


def clamp_margins(case):
    """Per iteration and PRODUCING fold of the reference: (|0.5 / sqrt(lam_z) - 1|, relative distance of 1 / sqrt(lam_y) from the floor
    1 / (t eps), whether the floor is active); NaN where the statistics are not finite."""
    res = reference(case)
    n_iter, K = res.trace.shape[:2]
    out = np.full((n_iter, K, 3), np.nan)
    for t in range(1, n_iter + 1):
        for f in range(K):
            lz, ly = res.trace[t - 1, f, 3], res.trace[t - 1, f, 4]
            if not (np.isfinite(lz) and np.isfinite(ly)):
                continue
            raw = 0.5 / np.sqrt(lz)
            eps = min(1.0, raw)
            gy, gt = 1.0 / np.sqrt(ly), 1.0 / (t * eps)
            out[t - 1, f] = [abs(raw - 1.0), abs(gy - gt) / max(gy, gt), float(gt >= gy)]
    return out


def decision_margins(case):
    """``| log|s| + dH |`` of every chain and iteration of the reference with a finite energy change, and the decisions."""
    res = reference(case)
    with np.errstate(all="ignore"):
        m = np.abs(np.log(np.abs(res.slices)) + res.energy_changes)
    return np.where(np.isfinite(res.energy_changes), m, np.inf), res.decisions


def measure(names=None):
    for c in names or list(CASES):
        print(f'    "{c}": {tolerance(c)},', flush=True)


if __name__ == "__main__":
    import sys
    measure(sys.argv[1:])
