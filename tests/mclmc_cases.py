"""The cases of tests/test_gpu_mclmc.py and tests/test_mclmc_ref.py: ``mfm_mclmc_*`` (mfm_amd/csrc/mclmc.hip) on every dispatch instance.

case                 instance
gmm4 (d = 2)         MAXIT 1, the mixture path and the d - 1 = 1 edge
d65_d0               MAXIT 4, a ragged last lane group
d257_pbc             MAXIT 16 with the run-time boundary
32x32_db             MAXIT 16, lattice with a frame
d1025_d0             MAXIT 32
d2048_pbc            MAXIT 32 with the run-time boundary
d2048_d0_shard       MAXIT 32, chains 48 .. 63 of 64

The phi-four cases are those of tests/row_instance_cases.py (16 chains, its start states near a mode, its boundaries); ``gmm4`` is the
4-mode mixture of tests/gpu_util.gmm4_setup from chain b's mode plus 0.5 N(0, 1).  L = sqrt(d).

``STEP_SIZES[case][integrator]``: chosen on a CPU with the float64 restatement (``scan``: ``SCAN_STEPS`` steps from the start state) so
that the energy-change variance per dimension over the 16 chains is within [0.1, 10] of blackjax's target 5e-4 -- the regime the
sampler is run in; tests/test_mclmc_ref.py asserts it.

``step_f32`` restates a step in the device's number formats as ``row_instance_cases.hmc_step_f32`` does: the position rounded to
float32 after every A, the gradient in float32 arithmetic (``grad32``; the mixture: log-density and gradient as the device's float32
evaluation makes them), everything else float64.  ``F32_DISTANCE[case][integrator]``: the largest differences of (x, u, logp, dE) between that and the float64 restatement over
the case's steps, each step of both from the same state -- what the formats cost, whatever the kernel.  ``f32_distance`` computes it,
tests/test_mclmc_ref.py recomputes it, and the GPU test's tolerance is the larger of the existing HMC tests' form and 4 x this."""
import numpy as np

from oracle import prng, targets
from tests import mclmc_ref as ref
from tests import row_instance_cases as rc

N_CHAINS, N_STEPS, SCAN_STEPS = rc.N_CHAINS, 3, 12
TARGET_VAR = 5e-4
ROW_CASES = ("d65_d0", "d257_pbc", "32x32_db", "d1025_d0", "d2048_pbc", "d2048_d0_shard")
CASES = ("gmm4",) + ROW_CASES
INTEGRATORS = (0, 1)

# case: {integrator: step size} -- written by ``scan`` (run this module), not by hand
STEP_SIZES = {
    "gmm4": {0: 0.75, 1: 1.3},
    "d65_d0": {0: 0.18, 1: 0.42},
    "d257_pbc": {0: 0.13, 1: 0.42},
    "32x32_db": {0: 0.42, 1: 1.0},
    "d1025_d0": {0: 0.1, 1: 0.32},
    "d2048_pbc": {0: 0.1, 1: 0.32},
    "d2048_d0_shard": {0: 0.1, 1: 0.32},
}

# case: {integrator: (x, u, logp, dE)} -- ``f32_distance`` rounded up to two digits (run this module)
F32_DISTANCE = {
    "gmm4": {0: (4.7e-07, 3.2e-07, 1.5e-06, 1.6e-06), 1: (6.3e-07, 6.7e-07, 1.1e-06, 1.8e-06)},
    "d65_d0": {0: (6.1e-08, 4.8e-08, 4.6e-06, 4.3e-06), 1: (1.1e-07, 1.5e-07, 6.3e-06, 8.3e-06)},
    "d257_pbc": {0: (6.1e-08, 3.9e-08, 2.3e-05, 2.2e-05), 1: (1.2e-07, 2.1e-07, 4.6e-05, 4.8e-05)},
    "32x32_db": {0: (6.1e-08, 1.2e-08, 1.8e-05, 1.7e-05), 1: (1.2e-07, 3.5e-08, 6e-05, 5.5e-05)},
    "d1025_d0": {0: (6e-08, 2.8e-08, 4.7e-05, 4.4e-05), 1: (1.2e-07, 1.5e-07, 0.00011, 0.00014)},
    "d2048_pbc": {0: (6.1e-08, 3.3e-08, 0.00022, 0.00018), 1: (1.2e-07, 1.7e-07, 0.00031, 0.00034)},
    "d2048_d0_shard": {0: (6.1e-08, 2.8e-08, 0.00011, 8.9e-05), 1: (1.2e-07, 1.4e-07, 0.00024, 0.00026)},
}


def gmm4_dist():
    return targets.GaussianMixture(8.0 * np.array([[1, 1], [1, -1], [-1, 1], [-1, -1.0]]), np.ones((4, 2)), np.ones(4) / 4)


def dim(case):
    return 2 if case == "gmm4" else rc.CASES[case][0]


def shard(case):
    """(n_chain_total, chain_offset)."""
    return (N_CHAINS, 0) if case == "gmm4" else rc.CASES[case][3:5]


def start_state(case):
    """[N_CHAINS, d] float32."""
    if case != "gmm4":
        return rc.start_state(case)
    d = gmm4_dist()
    noise = prng.normal_rows(prng.split(prng.PRNGKey(4100), N_CHAINS), 2)
    return (d.modes[np.arange(N_CHAINS) % 4] + 0.5 * noise).astype(np.float32)


def value_and_grad(case):
    if case == "gmm4":
        return targets.Tempered(gmm4_dist(), 1.0).value_and_grad
    return rc.value_and_grad(case, "b1")


def value_and_grad_f32(case):
    """The target as the device evaluates it at a float32 position: the log-density in float64, the gradient in float32 arithmetic."""
    if case == "gmm4":                                  # targets.hip.h, gmm_eval_lanes16: everything in float32, the modes summed after the max is taken out
        f32 = np.float32
        dist = gmm4_dist()
        std = np.sqrt(dist.covs)
        logw = (np.log(dist.weights) - (np.log(std) + 0.5 * np.log(2.0 * np.pi)).sum(1)).astype(f32)
        mode, sd = dist.modes.astype(f32), std.astype(f32)

        def f(x):
            dx = x.astype(f32)[:, None, :] - mode[None]
            z = dx / sd[None]
            comp = logw[None] - (f32(0.5) * z * z).sum(2, dtype=f32)
            m = comp.max(1)
            e = np.exp(comp - m[:, None], dtype=f32)
            se = e.sum(1, dtype=f32)
            g = (e[:, :, None] * (-dx / (sd * sd)[None])).sum(1, dtype=f32) * (f32(1) / se)[:, None]
            return m.astype(np.float64) + np.log(se, dtype=f32).astype(np.float64), g.astype(np.float64)
        return f
    dist = rc.oracle_dist(case)

    def f(x):
        return dist.loglik(x), rc.grad32(case, x.astype(np.float32), 1.0).astype(np.float64)
    return f


def momentum_key(case):
    return prng.PRNGKey(5000 + CASES.index(case))


def step_key(case, j, n_steps=N_STEPS):
    """The key of step j and the per-chain keys ``mfm_mclmc_step`` derives from it for the context's chains."""
    n_total, off = shard(case)
    key = prng.split(prng.PRNGKey(6000 + CASES.index(case)), n_steps)[j]
    return key, ref.chain_keys(key, n_total, off, N_CHAINS)


def start(case, vg=None):
    """The float64 restatement's state at the start state with ``mfm_mclmc_init``'s momenta."""
    n_total, off = shard(case)
    return ref.init(start_state(case).astype(np.float64), vg or value_and_grad(case), momentum_key(case), n_total, off)


def round32(x):
    return x.astype(np.float32).astype(np.float64)


def step_f32(case, state, keys, eps, L, integrator):
    """One step in the device's number formats from ``state`` (position float32-valued): (state, info)."""
    vg32 = value_and_grad_f32(case)
    lp, g = vg32(state.position)
    return ref.step(keys, ref.State(state.position, state.momentum, lp, g), vg32, eps, L, integrator, round_position=round32)


def f32_distance(case, integrator, eps=None):
    eps = STEP_SIZES[case][integrator] if eps is None else eps
    vg, L = value_and_grad(case), float(np.sqrt(dim(case)))
    st = start(case)
    out = np.zeros(4)
    for j in range(N_STEPS):
        keys = step_key(case, j)[1]
        lp, g = vg(st.position)
        s64, i64 = ref.step(keys, ref.State(st.position, st.momentum, lp, g), vg, eps, L, integrator)
        s32, i32 = step_f32(case, st, keys, eps, L, integrator)
        out = np.maximum(out, [np.abs(s64.position - s32.position).max(), np.abs(s64.momentum - s32.momentum).max(),
                               np.abs(s64.logdensity - s32.logdensity).max(), np.abs(i64.energy_change - i32.energy_change).max()])
        st = s32
    return tuple(out)


def variance_ratio(case, integrator, eps, n_steps=SCAN_STEPS):
    """v / target of ``n_steps`` float64 steps from the start state at step size eps."""
    vg = value_and_grad(case)
    _, info = ref.run(prng.PRNGKey(7000 + CASES.index(case)), start(case, vg), vg, eps, float(np.sqrt(dim(case))), integrator, n_steps)
    return info.energy_var_per_dim / TARGET_VAR


def scan(case, integrator, grid):
    """The step size of ``grid`` whose ``variance_ratio`` is nearest 1 on the log scale."""
    with np.errstate(all="ignore"):
        r = np.array([variance_ratio(case, integrator, e) for e in grid])
    score = np.where(np.isfinite(r) & (r > 0), np.abs(np.log(np.where(r > 0, r, 1.0))), np.inf)
    return float(grid[int(np.argmin(score))])


def _up2(v):
    """v rounded up to two significant digits."""
    if v == 0:
        return 0.0
    e = int(np.floor(np.log10(v))) - 1
    return float(f"{np.ceil(v / 10.0 ** e) * 10.0 ** e:.2g}")


if __name__ == "__main__":                            # prints the two tables
    import sys
    grid = [float(f"{10.0 ** (-3 + k / 8):.2g}") for k in range(33)]       # 1e-3 .. 10
    names = sys.argv[1:] or list(CASES)
    sizes = {c: {i: scan(c, i, grid) for i in INTEGRATORS} for c in names}
    for c in names:
        print(f'    "{c}": {sizes[c]},', flush=True)
    for c in names:
        row = {i: tuple(_up2(v) for v in f32_distance(c, i, sizes[c][i])) for i in INTEGRATORS}
        print(f'    "{c}": {row},', flush=True)
