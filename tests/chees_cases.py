"""The cases of tests/test_gpu_chees.py and tests/test_chees_cases.py: ``mfm_chees_warmup`` on every (MAXIT, BCRT, MASS) instance of its
step kernel (tests/test_row_matrix.py asserts that none is left out), with the float64 restatement (tests/chees_ref.py) of each.  A
helper, not a test.

Start states are smooth states near a mode (as tests/row_instance_cases.py has them, for the reason given there): chain b with sign
s_b = +1, -1, ...; Dirichlet 0 on the chain: s_b sin(pi (j + 1) / (d + 1)); periodic: the constant s_b; each plus (0.5 / d) N(0, 1)
noise, rounded to float32.  The 4-mode mixture starts chain b at mode b % 4 plus N(0, 1) noise.

``TOLERANCE[case]``: the bound of the GPU test's end-to-end comparison of the traces, per trace column the largest difference over
the case's iterations between the restatement and its ``float32_positions=True`` variant, times 4 (the device's libm and summation
order, which the variant does not model), relative to max(1, |value|).  tests/test_chees_cases.py recomputes it and holds the recorded
figures to the recomputation; it also asserts what the GPU test relies on: no accept / reject decision, divergence flag or leapfrog
count of any iteration is near its threshold."""
import functools

import numpy as np

from oracle import prng, targets
from tests import chees_ref as cr
from tests.phi4_bc_oracle import PhiFourBC

A, TBETA = 0.1, 20.0

# name: target ("gmm4" or the phi-four boundary), d, chains, n_valid, iterations, key_mode, eps_1, T_1, max_leapfrog, learning rate,
#       non-unit inverse mass
CASES = {
    # the mixture path (MAXIT 1, gradient scratch), step-major keys.  The step size stays where no chain leaves its mode's
    # neighbourhood: far out the oracle's mixture density (a product of pdfs, then the log) underflows where the kernel's does not
    "gmm4": dict(target="gmm4", d=2, B=16, n_valid=16, n_iter=8, key_mode=0, eps=0.06, T=1.5, max_leapfrog=1000, lr=0.025, mass=False),
    # MAXIT 1; 13 of 16 chains count
    "phi4_d64": dict(target="d0", d=64, B=16, n_valid=13, n_iter=8, key_mode=0, eps=0.05, T=0.21, max_leapfrog=1000, lr=0.025, mass=False),
    # MAXIT 4, a ragged last lane group; chain-major keys
    "phi4_d65": dict(target="d0", d=65, B=16, n_valid=16, n_iter=8, key_mode=1, eps=0.045, T=0.17, max_leapfrog=1000, lr=0.025, mass=False),
    # MAXIT 4, full; the leapfrog count clamped at max_leapfrog = 3
    "phi4_d256": dict(target="d0", d=256, B=32, n_valid=32, n_iter=6, key_mode=0, eps=0.02, T=0.13, max_leapfrog=3, lr=0.025, mass=False),
    # MAXIT 16 on the mass instance: minv read from memory at every use
    "phi4_d320_mass": dict(target="d0", d=320, B=16, n_valid=16, n_iter=6, key_mode=0, eps=0.016, T=0.07, max_leapfrog=1000, lr=0.025, mass=True),
    # the run-time boundary (BCRT), chain-major keys, 12 iterations
    "phi4_d64_pbc": dict(target="pbc", d=64, B=16, n_valid=16, n_iter=12, key_mode=1, eps=0.05, T=0.19, max_leapfrog=1000, lr=0.05, mass=False),
    # a first step size beyond velocity Verlet's stability limit (eps omega_max = 2 at 0.088): divergent chains, then recovery
    "phi4_d64_divergent": dict(target="d0", d=64, B=16, n_valid=16, n_iter=8, key_mode=0, eps=0.13, T=1.7, max_leapfrog=1000, lr=0.025, mass=False),
}
# the instances the first table left out (tests/row_matrix.py has the grid): unit mass and mass, BCRT false and true, at every MAXIT
NEW_CASES = {
    # MAXIT 4 on the mass instance (minv in registers)
    "phi4_d65_mass": dict(target="d0", d=65, B=16, n_valid=16, n_iter=6, key_mode=0, eps=0.04, T=0.17, max_leapfrog=1000, lr=0.025, mass=True),
    # MAXIT 4 with the run-time boundary and a ragged last lane group
    "phi4_d65_pbc": dict(target="pbc", d=65, B=16, n_valid=16, n_iter=6, key_mode=0, eps=0.03, T=0.17, max_leapfrog=1000, lr=0.025, mass=False),
    # MAXIT 16 at unit mass
    "phi4_d320": dict(target="d0", d=320, B=16, n_valid=16, n_iter=6, key_mode=1, eps=0.014, T=0.07, max_leapfrog=1000, lr=0.025, mass=False),
    # MAXIT 16 with the run-time boundary
    "phi4_d320_pbc": dict(target="pbc", d=320, B=16, n_valid=16, n_iter=6, key_mode=0, eps=0.012, T=0.07, max_leapfrog=1000, lr=0.025, mass=False),
    # MAXIT 32: the last lane group holds one element; the cross-chain statistic over 1025 columns
    "phi4_d1025": dict(target="d0", d=1025, B=16, n_valid=16, n_iter=5, key_mode=0, eps=0.004, T=0.022, max_leapfrog=1000, lr=0.025, mass=False),
    # MAXIT 32, its last dimension, with the run-time boundary AND the mass
    "phi4_d2048_pbc_mass": dict(target="pbc", d=2048, B=16, n_valid=16, n_iter=5, key_mode=0, eps=0.002, T=0.011, max_leapfrog=1000, lr=0.025, mass=True),
    # the rest of the grid: each (MAXIT, BCRT) cell on the instance of the other mass.  A finding: the eps and T columns of a trace move
    # little between the two restatements (T by 1e-9 .. 1e-8 over five or six iterations at this learning rate), so their tolerances sit
    # near float64 noise of the recursion's inputs and say little about the formats.  Two first choices for the cells (4, BCRT, mass) and
    # (32, BCRT, unit), d = 65 periodic with the mass at eps_1 = 0.03 and d = 2048 periodic at eps_1 = 0.002, had T and eps tolerances of
    # 2.2e-9 and 2.5e-8; on an MI355X the traces were off by 3.9e-9 and 3.9e-8 there (every other column within 0.6 of its tolerance, the
    # statistic within its reassociation bound and the recursion to 1e-12), so those two cells are held at d = 100 and d = 1100 instead
    "phi4_d64_mass": dict(target="d0", d=64, B=16, n_valid=16, n_iter=6, key_mode=1, eps=0.04, T=0.17, max_leapfrog=1000, lr=0.025, mass=True),
    "phi4_d64_pbc_mass": dict(target="pbc", d=64, B=16, n_valid=16, n_iter=6, key_mode=0, eps=0.03, T=0.17, max_leapfrog=1000, lr=0.025, mass=True),
    "phi4_d100_pbc_mass": dict(target="pbc", d=100, B=16, n_valid=16, n_iter=6, key_mode=1, eps=0.03, T=0.15, max_leapfrog=1000, lr=0.025, mass=True),
    "phi4_d320_pbc_mass": dict(target="pbc", d=320, B=16, n_valid=16, n_iter=6, key_mode=0, eps=0.014, T=0.08, max_leapfrog=1000, lr=0.025, mass=True),
    "phi4_d1025_mass": dict(target="d0", d=1025, B=16, n_valid=16, n_iter=5, key_mode=1, eps=0.004, T=0.022, max_leapfrog=1000, lr=0.025, mass=True),
    "phi4_d1100_pbc": dict(target="pbc", d=1100, B=16, n_valid=16, n_iter=5, key_mode=0, eps=0.003, T=0.02, max_leapfrog=1000, lr=0.025, mass=False),
}
# the seeds count along this order: the first seven cases by name, then the later ones in the order they were added
SEED_ORDER = sorted(CASES) + list(NEW_CASES)
CASES.update(NEW_CASES)

# case: per trace column (chees_ref.TRACE_FIELDS) 4 x the largest |float64 - float32 positions| / max(1, |value|) -- written from
# ``measure`` (run this module), not by hand
TOLERANCE = {
    "gmm4": (9.3e-05, 4.8e-06, 0, 3.3e-05, 0.00014, 0, 1.6e-05),
    "phi4_d64": (6.2e-06, 5e-07, 0, 0.00013, 6.6e-05, 0, 0.00012),
    "phi4_d65": (3.5e-07, 1e-08, 0, 9.6e-06, 1.8e-05, 0, 6.7e-06),
    "phi4_d256": (2.2e-08, 2e-08, 0, 1.8e-06, 4.9e-07, 0, 2e-06),
    "phi4_d320_mass": (6.5e-07, 1.6e-08, 0, 8.7e-05, 4e-05, 0, 6e-05),
    "phi4_d64_pbc": (3.7e-06, 1.7e-07, 0, 6.2e-05, 6.3e-05, 0, 4.9e-05),
    "phi4_d64_divergent": (2.1e-05, 2e-06, 0, 0.00031, 0.0044, 0, 0.00037),
    "phi4_d65_mass": (2.4e-07, 2.6e-07, 0, 4.1e-06, 2.6e-06, 0, 4.5e-06),
    "phi4_d65_pbc": (1.9e-06, 1.1e-08, 0, 1.5e-05, 1.9e-05, 0, 1.3e-05),
    "phi4_d320": (2.3e-07, 1e-08, 0, 6.7e-05, 4.2e-05, 0, 7.3e-05),
    "phi4_d320_pbc": (1.5e-07, 3e-08, 0, 2.7e-05, 0.00011, 0, 1.6e-05),
    "phi4_d1025": (6.4e-08, 6.7e-09, 0, 4.1e-05, 2.2e-05, 0, 4.1e-05),
    "phi4_d2048_pbc_mass": (7.1e-08, 2.4e-08, 0, 0.00021, 0.00014, 0, 0.00022),
    "phi4_d64_mass": (4e-07, 2.4e-07, 0, 8.1e-06, 1.4e-05, 0, 6.1e-06),
    "phi4_d64_pbc_mass": (1.2e-06, 1.5e-08, 0, 2.6e-05, 6e-05, 0, 1.9e-05),
    "phi4_d100_pbc_mass": (3.4e-07, 1.3e-08, 0, 1.6e-05, 1.1e-05, 0, 1.5e-05),
    "phi4_d320_pbc_mass": (3.6e-07, 1.9e-08, 0, 9.5e-05, 0.00011, 0, 9.4e-05),
    "phi4_d1025_mass": (5.4e-08, 4e-09, 0, 4.2e-05, 3.7e-05, 0, 4.2e-05),
    "phi4_d1100_pbc": (8.7e-08, 8.7e-09, 0, 5.6e-05, 0.00012, 0, 3.6e-05),
}

DIVERGENCE_THRESHOLD = 1000.0
TARGET_ACCEPT, DECAY = 0.651, 0.5


def dist(case):
    c = CASES[case]
    if c["target"] == "gmm4":
        return targets.GaussianMixture(8.0 * np.array([[1, 1], [1, -1], [-1, 1], [-1, -1.0]]), np.ones((4, 2)), np.ones(4) / 4)
    return PhiFourBC(c["d"], A, TBETA, ("pbc", 0.0) if c["target"] == "pbc" else ("dirichlet", 0.0))


def block(case):
    """The target block to hand ``set_target`` after the context's default, or None."""
    return dist(case).block() if CASES[case]["target"] == "pbc" else None


def start_state(case):
    """[B, d] float32."""
    c = CASES[case]
    B, d = c["B"], c["d"]
    noise = prng.normal_rows(prng.split(prng.PRNGKey(7000 + SEED_ORDER.index(case)), B), d)
    if c["target"] == "gmm4":
        return (dist(case).modes[np.arange(B) % 4] + noise).astype(np.float32)
    sign = np.where(np.arange(B) % 2 == 0, 1.0, -1.0)[:, None]
    base = sign * (np.ones((1, d)) if c["target"] == "pbc" else np.sin(np.pi * (np.arange(d) + 1) / (d + 1))[None])
    return (base + 0.5 / d * noise).astype(np.float32)


def inverse_mass(case):
    """None, or [d] values log-spaced over [0.5, 2] in a fixed permutation."""
    c = CASES[case]
    if not c["mass"]:
        return None
    return np.exp(np.linspace(np.log(0.5), np.log(2.0), c["d"]))[np.random.RandomState(5).permutation(c["d"])]


def key(case):
    """ONE key (key_mode 0) or the chains' keys [B, 2] (key_mode 1)."""
    c = CASES[case]
    k = prng.PRNGKey(9000 + SEED_ORDER.index(case))
    return prng.split(k, c["B"]) if c["key_mode"] else k


def value_and_grad(case):
    return targets.Tempered(dist(case), 1.0).value_and_grad


@functools.lru_cache(maxsize=None)
def reference(case, float32_positions=False):
    """The restatement's run of the case (computed once per process; the callers leave it unchanged)."""
    c = CASES[case]
    vg = value_and_grad(case)
    x = start_state(case).astype(np.float64)
    lp, g = vg(x)
    return cr.chees_warmup(key(case), cr.State(x, lp, g), vg, c["eps"], c["n_iter"], T1=c["T"], n_valid=c["n_valid"], key_mode=c["key_mode"],
                           inverse_mass=inverse_mass(case), target_accept=TARGET_ACCEPT, learning_rate=c["lr"], max_leapfrog=c["max_leapfrog"],
                           decay=DECAY, divergence_threshold=DIVERGENCE_THRESHOLD, float32_positions=float32_positions)


def measure(case):
    """Per trace column 4 x the largest difference between the two variants over the case, relative to max(1, |value|)."""
    a, b = reference(case, False)["trace"], reference(case, True)["trace"]
    with np.errstate(invalid="ignore"):
        return tuple(float(v) for v in 4.0 * np.nanmax(np.abs(a - b) / np.maximum(1.0, np.abs(a)), axis=0))


def margins(case):
    """What the GPU test relies on, over every iteration and VALID-or-not chain: the smallest |u - alpha|, the smallest
    |dH - threshold| / threshold, the smallest relative distance of tau / eps from an integer."""
    r = reference(case)
    u_gap = min(float(np.abs(rec.u - rec.alpha).min()) for rec in r["records"])
    dh = np.concatenate([rec.energy_change for rec in r["records"]])
    dh_gap = float(np.abs(dh[np.isfinite(dh)] - DIVERGENCE_THRESHOLD).min()) / DIVERGENCE_THRESHOLD      # (a NaN or an infinite change is divergent outright)
    ratio = np.array([cr.radical_inverse(t + 1) * row[1] / row[0] for t, row in enumerate(r["trace"])])
    int_gap = float((np.abs(ratio - np.round(ratio)) / ratio).min())
    return u_gap, dh_gap, int_gap


if __name__ == "__main__":
    import sys
    for name in sys.argv[1:] or CASES:
        r = reference(name)
        tr = r["trace"]
        print(name, "L", tr[:, 2].astype(int).tolist(), "n_div", tr[:, 5].astype(int).tolist(), "hm", np.round(tr[:, 3], 3).tolist())
        print("   eps", np.round(tr[:, 0], 4).tolist(), "T", np.round(tr[:, 1], 4).tolist(), "ghat", ["%.3g" % v for v in tr[:, 4]])
        print("   accepted", [int(rec.accepted.sum()) for rec in r["records"]], "margins (u, dH, integer) %.3g %.3g %.3g" % margins(name))
        print('    "%s": (%s),' % (name, ", ".join("%.2g" % v for v in measure(name))))
