"""The case table of tests/test_gpu_shard_invariance.py: which chains the parts hold, the targets with their step sizes, and the
entry points of every family.  Not a test.

THE SCHEME.  B = 64 chains.  The whole run is one context with ``n_chain_local = n_chain_total = 64`` at offset 0; the parts are fresh
contexts with ``n_chain_total = 64`` that hold the chains [0, 16), [16, 48) and [48, 64): uneven, two non-zero offsets, every offset a
multiple of 16 so that a 16-chain (and a 4-chain) tile holds the same chains in both runs.  The CONTROL runs the [16, 48) part in a
context built with offset 0: what it draws must differ from rows 16..47 of the whole run.

Step sizes are those of the existing tables, chosen there with the float64 oracle so that accepted and rejected steps both occur:
tests/test_gpu_mala_run.py (MALA as written and the mixture's textbook step), tests/test_gpu_hmc_run.py (HMC, 3 leapfrog steps),
tests/row_instance_cases.py ``d65_d0`` (d = 65, from a start near a mode as there), tests/test_gpu_nuts.py (NUTS)."""
import numpy as np

from oracle import prng

B = 64
PARTS = ((0, 16), (16, 32), (48, 16))                 # (chain_offset, n_chain_local)
CONTROL = (16, 32)                                    # the part the control runs again at offset 0
CHAIN_AXIS_1 = ("traj_pos", "traj_logp", "step_traj")      # outputs [n_kept or n_steps, n_chain_local, ...]: every other is [n_chain_local, ...]

N_STEPS, THIN, LEAPFROG = 4, 2, 3
LENGTHS = (3, 1, 4, 2)                                # mfm_hmc_run_lengths: leapfrog steps of each HMC step
HMC_TARGET, MALA_TARGET = 0.8, 0.574                  # target acceptance of the warmups (tests/test_gpu_warmup.py)
NUTS_DEPTH, NUTS_TRANSITIONS = 5, 3

# name: target kind, d, where the chains start, and per sampler (beta, step size).  "mala_textbook" is what mfm_mala_warmup takes (it
# refuses the rule as written); d = 65 is the last lane-ragged dimension of the small instances (MAXIT 4: one element in the second row).
TARGETS = {
    "phi4_d64": dict(kind="phi4", d=64, start="init", mala=(1.0, 4e-5), mala_textbook=(1.0, 4e-5), hmc=(1.0, 0.088), nuts=(1.0, 0.03)),
    "phi4_d65": dict(kind="phi4", d=65, start="mode", mala=(1.0, 0.0018), mala_textbook=(0.37, 0.0015), hmc=(1.0, 0.046), nuts=(1.0, 0.03)),
    "gmm4": dict(kind="gmm", d=2, start="init", mala=(1.0, 0.2), mala_textbook=(1.0, 1.5), hmc=(1.0, 1.8), nuts=(1.0, 0.3)),
}

# the resident-chain kernels (resident.hip.h: run_step_key), each in key mode 0 (step-major) and 1 (one key per chain)
RESIDENT = ("mala_run", "hmc_run", "hmc_run_lengths", "mala_warmup", "hmc_warmup_window", "hmc_warmup_window_mass", "nuts_warmup_window")
NUTS = ("nuts_step", "nuts_step_keys", "nuts_run_mode0", "nuts_run_mode1")

# mfm_flow_step: name -> (family, mode, fixed-step (method, steps) or None).  Families: "tile" the generic 16-chain tile (phi-four d = 64,
# hidden 32, F 16); "d2-4" / "d2-4s" / "d2-16" the d = 2 tiles on the 4-mode mixture (MFM_D2_TILE pins the tile for both runs: the library
# picks it by chain count); "fast" the shape-specialised solver (d = 64, hidden 128); "wide" the wide family at the tile's small shape.
FLOW = {
    "tile-rwmh": ("tile", "rwmh", None), "tile-imh": ("tile", "imh", None), "tile-cis": ("tile", "cis", None),
    "d2-4-rwmh": ("d2-4", "rwmh", None), "d2-4-imh": ("d2-4", "imh", None), "d2-4-rk4": ("d2-4", "rwmh", ("rk4", 8)),
    "d2-4s-rwmh": ("d2-4s", "rwmh", None), "d2-4s-imh": ("d2-4s", "imh", None), "d2-4s-rk4": ("d2-4s", "rwmh", ("rk4", 8)),
    "d2-16-rwmh": ("d2-16", "rwmh", None), "d2-16-imh": ("d2-16", "imh", None),
    "fast-rk4": ("fast", "rwmh", ("rk4", 8)),
    "wide-rwmh": ("wide", "rwmh", None), "wide-imh": ("wide", "imh", None), "wide-rk4": ("wide", "rwmh", ("rk4", 8)),
}
# one sensitivity control per key-derivation site: ode.hip, ode_d2.hip, ode_fixed.hip, the wide family's probes in api.hip
FLOW_CONTROLS = ("tile-rwmh", "d2-4-rwmh", "fast-rk4", "wide-rwmh")
CIS_SAMPLES = 3

# mfm_train_iter with the MALA step inside the training kernel (fm.hip: fm_mala_fusable): one column tile per wave, two, and the
# headline's static instance.  (d, hidden, F, MALA step size: tests/test_gpu_mala_run.py's for the rule as written, oracle mean
# acceptance 0.52 at d = 64 and 0.36 at d = 256 -- at the loop's default 1e-4 every d = 256 proposal is rejected with probability 0)
FUSED = {"tpw1": (64, 32, 16, 4e-5), "tpw2": (256, 32, 16, 3e-6), "headline": (256, 128, 128, 3e-6)}
FUSED_K = 3                                           # counts 1 .. 3 are MALA iterations; count 4 would be the flow step


def mode_start(d, n):
    """[n, d] float32: the start of tests/row_instance_cases.py on the Dirichlet-0 chain for n chains -- chain b near the mode of sign
    (-1)^b, plus (0.5 / d) N(0, 1) noise from oracle.prng."""
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[:, None]
    base = sign * np.sin(np.pi * (np.arange(d) + 1) / (d + 1))[None]
    noise = prng.normal_rows(prng.split(prng.PRNGKey(4100 + d), n), d)
    return (base + 0.5 / d * noise).astype(np.float32)


def rows(a, name, off, n):
    """Chains [off, off + n) of the whole run's output ``name``."""
    return a[:, off:off + n] if name in CHAIN_AXIS_1 else a[off:off + n]
