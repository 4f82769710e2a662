"""The cases of tests/test_gpu_row_instances.py and tests/test_row_instance_cases.py: the row kernels (one wave per chain, lane l owns
elements l + 64 it: mala_init / loglik / mala_step in mala.hip, hmc_step in hmc.hip, the run and warmup kernels) on the dispatch
instances above d = 256 -- MAXIT 16 (256 < d <= 1024) and MAXIT 32 (1024 < d <= 2048), BCRT false (Dirichlet 0 on the chain) and
true (every other boundary, every lattice) -- at each instance's first and last dimension, plus d = 65 (the first of MAXIT 4).

Start states.  Not ``dist.init_params``: from that U(-1, 1) start |log pi| is 4.8e4 at d = 257 and 2.9e6 at d = 2048, and tolerances
of the form max(1, |log pi|) would admit anything.  A smooth state near a mode instead, chain b with sign s_b = +1, -1, ...:
Dirichlet b on the chain: b + (s_b - b) sin(pi (j + 1) / (d + 1)); periodic, chain and lattice: the constant s_b; the Dirichlet-b
lattice: b + (1 - b) g(r) g(c) with the boundary layer g(i) = tanh((i + 1) / (a L)) tanh((L - i) / (a L)) for every chain -- the frame
held at b costs a L / 2 (x - b)^2 per edge site, so on a lattice the product of sines has |log pi| = 2.1e3 at 45 x 45 and the -1 side
of the layer as much; each plus (0.5 / d) N(0, 1) noise (oracle.prng draws), rounded to float32.  Float64 oracle at beta = 1:
|log pi| = 24 on the Dirichlet-0 chain at every d, 35 with b = 0.5, 0.5 periodic, 140 ... 430 on the Dirichlet-0.5 lattices.

Step sizes (``STEP_SIZES``): chosen with the float64 oracle on a CPU (``scan`` below) so that the case's three steps hold accepted
and rejected proposals, at most one chain per step lies inside the borderline band the GPU test excludes and none near its edge;
tests/test_row_instance_cases.py asserts the conditions the GPU test relies on (both decisions; at most 1 of 16 chains per step
inside the band).  ``HMC_F32_DISTANCE``: what the device's number formats cost the HMC energies against the oracle (see there).

The sampler ``"hmc_mass"`` is the HMC step under the diagonal inverse mass ``hmc_mass_ref.log_spaced_mass(d)`` (tests/hmc_mass_ref.py
is its float64 restatement), on ``MASS_CASES``: one case per (MAXIT 16 / 32, BCRT false / true) cell and BCRT at MAXIT 4, for
tests/test_gpu_hmc_mass.py.  ``MASS_STEP_SIZES`` and ``HMC_MASS_F32_DISTANCE`` are its two tables, made and checked as the unit-mass ones."""
import numpy as np

from oracle import hmc as ohmc, mala as omala, prng, targets
from tests import hmc_mass_ref
from tests.mcmc_bits_cases import VARIANTS
from tests.phi4_2d_oracle import PhiFour2D
from tests.phi4_bc_oracle import PhiFourBC

N_CHAINS, N_STEPS, HMC_LEAPFROG = 16, 3, 3
A, TBETA = 0.1, 20.0                                  # the phi-four model's own constants (oracle.targets.PhiFour's defaults)
BOUNDARIES = {"d0": ("dirichlet", 0.0), "pbc": ("pbc", 0.0), "db": ("dirichlet", 0.5)}

# name: (d, lattice side L or 0, boundary, n_chain_total, chain_offset)
CASES = {}
for _d in (65, 257, 1024, 1025, 2048):
    for _bc in BOUNDARIES:
        CASES[f"d{_d}_{_bc}"] = (_d, 0, _bc, N_CHAINS, 0)
CASES["d2048_d0_shard"] = (2048, 0, "d0", 64, 48)      # key derivation and row addressing with a non-zero chain offset
for _L in (17, 32, 33, 45):
    for _bc in ("pbc", "db"):
        CASES[f"{_L}x{_L}_{_bc}"] = (_L * _L, _L, _bc, N_CHAINS, 0)

SAMPLERS = ("mala", "hmc")
# MAXIT 16 / 32 x BCRT false / true under a non-unit mass, and BCRT at MAXIT 4 (tests/test_gpu_hmc_mass.py has MAXIT 1 and 4 on Dirichlet 0)
MASS_CASES = ("d65_pbc", "d257_d0", "17x17_db", "d1025_d0", "d2048_pbc")

# case: {sampler: {variant: step size}} -- written by ``scan`` (run this module), not by hand
STEP_SIZES = {
    "d65_d0": {"mala": {"b1": 0.0018, "b037_textbook": 0.0015}, "hmc": {"b1": 0.046, "b037_textbook": 0.038}},
    "d65_pbc": {"mala": {"b1": 0.0018, "b037_textbook": 0.0015}, "hmc": {"b1": 0.026, "b037_textbook": 0.068}},
    "d65_db": {"mala": {"b1": 0.0026, "b037_textbook": 0.0012}, "hmc": {"b1": 0.022, "b037_textbook": 0.038}},
    "d257_d0": {"mala": {"b1": 0.00056, "b037_textbook": 0.00018}, "hmc": {"b1": 0.0083, "b037_textbook": 0.012}},
    "d257_pbc": {"mala": {"b1": 0.00056, "b037_textbook": 0.00015}, "hmc": {"b1": 0.0068, "b037_textbook": 0.01}},
    "d257_db": {"mala": {"b1": 0.00056, "b037_textbook": 0.00015}, "hmc": {"b1": 0.0068, "b037_textbook": 0.012}},
    "d1024_d0": {"mala": {"b1": 0.00015, "b037_textbook": 1.8e-05}, "hmc": {"b1": 0.0022, "b037_textbook": 0.0038}},
    "d1024_pbc": {"mala": {"b1": 0.00015, "b037_textbook": 2.6e-05}, "hmc": {"b1": 0.0022, "b037_textbook": 0.0038}},
    "d1024_db": {"mala": {"b1": 0.00015, "b037_textbook": 2.2e-05}, "hmc": {"b1": 0.0026, "b037_textbook": 0.0038}},
    "d1025_d0": {"mala": {"b1": 0.00015, "b037_textbook": 1.5e-05}, "hmc": {"b1": 0.0022, "b037_textbook": 0.0038}},
    "d1025_pbc": {"mala": {"b1": 0.00012, "b037_textbook": 2.2e-05}, "hmc": {"b1": 0.0022, "b037_textbook": 0.0038}},
    "d1025_db": {"mala": {"b1": 0.00012, "b037_textbook": 2.2e-05}, "hmc": {"b1": 0.0022, "b037_textbook": 0.0038}},
    "d2048_d0": {"mala": {"b1": 6.8e-05, "b037_textbook": 5.6e-06}, "hmc": {"b1": 0.0012, "b037_textbook": 0.0022}},
    "d2048_pbc": {"mala": {"b1": 6.8e-05, "b037_textbook": 6.8e-06}, "hmc": {"b1": 0.0012, "b037_textbook": 0.0022}},
    "d2048_db": {"mala": {"b1": 6.8e-05, "b037_textbook": 6.8e-06}, "hmc": {"b1": 0.0015, "b037_textbook": 0.0022}},
    "d2048_d0_shard": {"mala": {"b1": 6.8e-05, "b037_textbook": 6.8e-06}, "hmc": {"b1": 0.0015, "b037_textbook": 0.0022}},
    "17x17_pbc": {"mala": {"b1": 0.0026, "b037_textbook": 0.0015}, "hmc": {"b1": 0.018, "b037_textbook": 0.032}},
    "17x17_db": {"mala": {"b1": 0.0046, "b037_textbook": 0.0012}, "hmc": {"b1": 0.018, "b037_textbook": 0.032}},
    "32x32_pbc": {"mala": {"b1": 0.0026, "b037_textbook": 0.00026}, "hmc": {"b1": 0.01, "b037_textbook": 0.015}},
    "32x32_db": {"mala": {"b1": 0.0026, "b037_textbook": 0.00026}, "hmc": {"b1": 0.01, "b037_textbook": 0.015}},
    "33x33_pbc": {"mala": {"b1": 0.0026, "b037_textbook": 0.00032}, "hmc": {"b1": 0.01, "b037_textbook": 0.015}},
    "33x33_db": {"mala": {"b1": 0.0026, "b037_textbook": 0.00032}, "hmc": {"b1": 0.0083, "b037_textbook": 0.015}},
    "45x45_pbc": {"mala": {"b1": 0.0018, "b037_textbook": 0.00018}, "hmc": {"b1": 0.0068, "b037_textbook": 0.01}},
    "45x45_db": {"mala": {"b1": 0.0018, "b037_textbook": 0.00015}, "hmc": {"b1": 0.01, "b037_textbook": 0.012}},
}


# case: {variant: step size} of the sampler "hmc_mass" -- written by ``scan`` (run this module with --mass), not by hand
MASS_STEP_SIZES = {
    "d65_pbc": {"b1": 0.022, "b037_textbook": 0.038},
    "d257_d0": {"b1": 0.0056, "b037_textbook": 0.01},
    "17x17_db": {"b1": 0.015, "b037_textbook": 0.026},
    "d1025_d0": {"b1": 0.0018, "b037_textbook": 0.0032},
    "d2048_pbc": {"b1": 0.001, "b037_textbook": 0.0018},
}


def step_size(case, sampler, variant):
    return MASS_STEP_SIZES[case][variant] if sampler == "hmc_mass" else STEP_SIZES[case][sampler][variant]


def inverse_mass(case):
    """The diagonal inverse mass of the sampler "hmc_mass": log-spaced over [0.25, 4] in a fixed permutation."""
    return hmc_mass_ref.log_spaced_mass(CASES[case][0])


def maxit(d):
    """The MAXIT instance MALA_DISPATCH selects for dimension d (mala.hip)."""
    nit = -(-d // 64)
    return next(m for m in (1, 4, 16, 32) if nit <= m)


def bcrt(case):
    """Whether the case runs on the run-time-boundary instances (anything but Dirichlet 0 on the chain)."""
    d, L, bc, _, _ = CASES[case]
    return L > 0 or bc != "d0"


def oracle_dist(case):
    d, L, bc, _, _ = CASES[case]
    return (PhiFour2D if L else PhiFourBC)(d, A, TBETA, BOUNDARIES[bc])


def block(case):
    """The target block to hand ``set_target`` after the context's default {a, beta}, or None (Dirichlet 0 on the chain)."""
    return oracle_dist(case).block() if bcrt(case) else None


def start_state(case):
    """[N_CHAINS, d] float32 (module docstring)."""
    d, L, bc, _, _ = CASES[case]
    kind, b = BOUNDARIES[bc]
    sign = np.where(np.arange(N_CHAINS) % 2 == 0, 1.0, -1.0)[:, None]
    if kind == "pbc":
        base = sign * np.ones((1, d))
    elif L:
        i = np.arange(L)
        g = np.tanh((i + 1) / (A * L)) * np.tanh((L - i) / (A * L))
        base = b + (1.0 - b) * np.outer(g, g).reshape(1, -1) * np.ones((N_CHAINS, 1))
    else:
        base = b + (sign - b) * np.sin(np.pi * (np.arange(d) + 1) / (d + 1))[None]
    noise = prng.normal_rows(prng.split(prng.PRNGKey(4000 + sorted(CASES).index(case)), N_CHAINS), d)
    return (base + 0.5 / d * noise).astype(np.float32)


# (case, sampler): n -- the step keys come from seed 2000 + index + 100 n.  With the default seed one chain of these draws u within a
# quarter band of 0.99, on the edge of the band around p = 1 at every step size; n is the first that admits a step size.
RESEED = {("d257_db", "mala"): 1, ("d2048_d0_shard", "mala"): 1, ("33x33_db", "mala"): 1, ("45x45_pbc", "mala"): 1}


def step_keys(case, j, sampler="mala"):
    """The key of step j and the per-chain keys ``mfm_mala_step`` / ``mfm_hmc_step`` derive from it for the context's chains."""
    _, _, _, n_total, off = CASES[case]
    key = prng.split(prng.PRNGKey(2000 + sorted(CASES).index(case) + 100 * RESEED.get((case, sampler), 0)), N_STEPS)[j]
    return key, prng.split(key, n_total)[off:off + N_CHAINS]


def seam_set(case):
    """Elements where a stencil that drops or misplaces a neighbour goes wrong: both sides of every 64-element seam, the row's
    ends and the elements 64 / 65 from its end; on a lattice also the first and last row and column."""
    d, L, _, _, _ = CASES[case]
    j = np.arange(d)
    m = (j % 64 == 0) | (j % 64 == 63)
    m[[i for i in (0, 63, 64, 65, d - 65, d - 64, d - 1) if 0 <= i < d]] = True
    if L:
        m |= (j < L) | (j >= d - L) | (j % L == 0) | (j % L == L - 1)
    return np.flatnonzero(m)


def where(j):
    """(element, it, lane) of element j, for failure messages."""
    return f"element {int(j)} (it {int(j) // 64}, lane {int(j) % 64})"


def value_and_grad(case, variant):
    return targets.Tempered(oracle_dist(case), VARIANTS[variant][0]).value_and_grad


def oracle_step(sampler, variant, st, vg, keys, eps):
    """One float64 oracle step: (new state, info, u)."""
    if sampler == "hmc":
        return ohmc.kernel(keys, st, vg, eps, HMC_LEAPFROG)
    if sampler == "hmc_mass":
        return hmc_mass_ref.kernel(keys, st, vg, eps, HMC_LEAPFROG, hmc_mass_ref.log_spaced_mass(st.position.shape[1]))
    return omala.kernel(keys, st, vg, eps, textbook=VARIANTS[variant][1])


def band_ratio(sampler, st, info, u):
    """|u - p| in units of the borderline band's half width; the bands are those of the existing tests (MALA: tests/test_gpu_mala.py,
    1e-2; HMC: tests/test_gpu_hmc.py, 10 tol p + 1e-6 with tol = 5e-6 max(1, |log pi|))."""
    p = info.acceptance_rate
    if sampler == "mala":
        return np.abs(u - p) / 1e-2
    tol = 5e-6 * max(1.0, np.abs(st.logdensity).max())
    return np.abs(u - p) / (10 * tol * np.maximum(p, 1e-30) + 1e-6)


def borderline(sampler, st, info, u):
    """The chains left out of the decision comparison."""
    return band_ratio(sampler, st, info, u) <= 1.0


def oracle_run(case, sampler, variant, eps=None):
    """The oracle alone over the case's three steps, restarting each step from the float32-rounded position as the device's state is:
    per step (decisions, |u - p| in units of the band, max |log pi| of the state the step started from)."""
    eps = step_size(case, sampler, variant) if eps is None else eps
    vg = value_and_grad(case, variant)
    st = omala.init(start_state(case).astype(np.float64), vg)
    out = []
    for j in range(N_STEPS):
        new, info, u = oracle_step(sampler, variant, st, vg, step_keys(case, j, sampler)[1], eps)
        out.append((info.is_accepted, band_ratio(sampler, st, info, u), np.abs(st.logdensity).max()))
        st = omala.init(new.position.astype(np.float32).astype(np.float64), vg)
    return out


def grad32(case, x, beta):
    """A numpy float32 restatement of the device's gradient formula, beta * (-tbeta (coef lap - x (1 - x^2) / coef)) with
    lap = cf x - l - r - (u + dn), every operation rounded to float32 (numpy has no fused multiply-add; the device fuses two)."""
    f = np.float32
    d, L, bc, _, _ = CASES[case]
    kind, b = BOUNDARIES[bc]
    x = np.asarray(x, f)
    if L:
        coef = f(A * L)
        fld = x.reshape(-1, L, L)
        if kind == "pbc":
            l, r, u, dn = np.roll(fld, 1, 2), np.roll(fld, -1, 2), np.roll(fld, 1, 1), np.roll(fld, -1, 1)
        else:
            pad = np.pad(fld, ((0, 0), (1, 1), (1, 1)), constant_values=f(b))
            l, r, u, dn = pad[:, 1:-1, :-2], pad[:, 1:-1, 2:], pad[:, :-2, 1:-1], pad[:, 2:, 1:-1]
        lap = (f(4) * fld - l - r - (u + dn)).reshape(x.shape)
    else:
        coef = f(A * d)
        if kind == "pbc":
            l, r = np.roll(x, 1, 1), np.roll(x, -1, 1)
        else:
            e = np.full((x.shape[0], 1), f(b))
            l, r = np.concatenate([e, x[:, :-1]], 1), np.concatenate([x[:, 1:], e], 1)
        lap = f(2) * x - l - r
    return f(beta) * (-f(TBETA) * (coef * lap - x * (f(1) - x * x) / coef))


def hmc_step_f32(case, variant, st, keys, eps, minv=None):
    """The oracle's HMC step (oracle/hmc.py; with ``minv`` tests/hmc_mass_ref.py's) restated with the device's number formats: the
    position rounded to float32 after every drift, the gradient in float32 arithmetic (``grad32``), momentum, energies and the
    log-density (of the float32 position) in float64.  Returns (log acceptance probability, end position, its log-density, its
    gradient)."""
    beta = VARIANTS[variant][0]
    dist = oracle_dist(case)
    x, lp, g = st.position.astype(np.float32), st.logdensity, st.logdensity_grad.astype(np.float32)
    minv = np.ones(x.shape[1]) if minv is None else minv
    p = prng.normal_rows(prng.split_rows(keys, 2)[:, 0], x.shape[1]) / np.sqrt(minv)
    h0 = -lp + 0.5 * (minv * p * p).sum(1)
    for _ in range(HMC_LEAPFROG):
        p = p + 0.5 * eps * g.astype(np.float64)
        x = (x.astype(np.float64) + eps * (minv * p)).astype(np.float32)
        lp, g = beta * dist.loglik(x.astype(np.float64)), grad32(case, x, beta)
        p = p + 0.5 * eps * g.astype(np.float64)
    h1 = -lp + 0.5 * (minv * p * p).sum(1)
    return np.minimum(h0 - h1, 0.0), x, lp, g


def hmc_f32_distance(case, variant, sampler="hmc"):
    """The float32 restatement against the float64 oracle over the case's three steps (the oracle's own trajectory): the largest
    differences of the log acceptance probability and of the end point's log-density."""
    eps = step_size(case, sampler, variant)
    minv = inverse_mass(case) if sampler == "hmc_mass" else None
    vg = value_and_grad(case, variant)
    st = omala.init(start_state(case).astype(np.float64), vg)
    d_p = d_lp = 0.0
    for j in range(N_STEPS):
        keys = step_keys(case, j, sampler)[1]
        new, info, u = oracle_step(sampler, variant, st, vg, keys, eps)
        lpa, x, lp, g = hmc_step_f32(case, variant, st, keys, eps, minv)
        d_p = max(d_p, np.abs(lpa - np.minimum(info.energy_delta, 0.0)).max())
        d_lp = max(d_lp, np.abs(lp - vg(info.proposed_position)[0]).max())
        st = omala.init(new.position.astype(np.float32).astype(np.float64), vg)
    return d_p, d_lp


# case: {variant: (log acceptance probability, end point's log-density)} -- ``hmc_f32_distance`` rounded up to two digits: what float32
# positions and float32 gradient arithmetic cost the HMC step's energies against the float64 oracle, whatever the kernel.  It does not
# scale with |log pi| (it is sum_j g_j dx_j over float32 roundings dx of the trajectory), so near a mode, where |log pi| is 0.5 on a
# periodic chain, it exceeds the forms of tests/test_gpu_hmc.py, 5e-6 max(1, |log pi|) + 1e-5 and 2e-6 max(1, |log pi|).  The GPU
# test takes the larger of that form and 4 x this distance; tests/test_row_instance_cases.py recomputes the table.
HMC_F32_DISTANCE = {
    "d65_d0": {"b1": (9.8e-06, 4.2e-06), "b037_textbook": (7.1e-06, 3.9e-06)},
    "d65_pbc": {"b1": (1.2e-05, 1.3e-05), "b037_textbook": (7.3e-06, 4.5e-06)},
    "d65_db": {"b1": (6.9e-06, 8.4e-06), "b037_textbook": (4.8e-06, 5.1e-06)},
    "d257_d0": {"b1": (3e-05, 2.5e-05), "b037_textbook": (1.8e-05, 1.8e-05)},
    "d257_pbc": {"b1": (3.8e-05, 3.9e-05), "b037_textbook": (2.1e-05, 2.1e-05)},
    "d257_db": {"b1": (2.7e-05, 2.2e-05), "b037_textbook": (1.3e-05, 1.7e-05)},
    "d1024_d0": {"b1": (5.5e-05, 7.7e-05), "b037_textbook": (3.4e-05, 4.1e-05)},
    "d1024_pbc": {"b1": (0.00014, 0.00013), "b037_textbook": (7.1e-05, 9.5e-05)},
    "d1024_db": {"b1": (6.6e-05, 0.0001), "b037_textbook": (3.5e-05, 4.3e-05)},
    "d1025_d0": {"b1": (9e-05, 9.9e-05), "b037_textbook": (4.2e-05, 3.8e-05)},
    "d1025_pbc": {"b1": (0.00014, 0.00019), "b037_textbook": (9.4e-05, 9.2e-05)},
    "d1025_db": {"b1": (6.9e-05, 7.9e-05), "b037_textbook": (4.2e-05, 5.4e-05)},
    "d2048_d0": {"b1": (0.00012, 0.00017), "b037_textbook": (7.2e-05, 9.1e-05)},
    "d2048_pbc": {"b1": (0.00017, 0.00022), "b037_textbook": (0.00015, 0.00018)},
    "d2048_db": {"b1": (0.00018, 0.00017), "b037_textbook": (0.00012, 0.00013)},
    "d2048_d0_shard": {"b1": (8.5e-05, 9.3e-05), "b037_textbook": (8.3e-05, 9.8e-05)},
    "17x17_pbc": {"b1": (1.3e-05, 1.9e-05), "b037_textbook": (8.2e-06, 1e-05)},
    "17x17_db": {"b1": (1.5e-05, 1.5e-05), "b037_textbook": (1.1e-05, 1.4e-05)},
    "32x32_pbc": {"b1": (3.3e-05, 3.6e-05), "b037_textbook": (2.2e-05, 2.1e-05)},
    "32x32_db": {"b1": (2.5e-05, 2.8e-05), "b037_textbook": (1.5e-05, 1.8e-05)},
    "33x33_pbc": {"b1": (3.1e-05, 4.2e-05), "b037_textbook": (1.9e-05, 1.6e-05)},
    "33x33_db": {"b1": (2.8e-05, 3.3e-05), "b037_textbook": (1.5e-05, 1.8e-05)},
    "45x45_pbc": {"b1": (6.5e-05, 4.6e-05), "b037_textbook": (2.3e-05, 2.9e-05)},
    "45x45_db": {"b1": (3.5e-05, 4.9e-05), "b037_textbook": (3.2e-05, 2.9e-05)},
}


# case: {variant: (log acceptance probability, end point's log-density)} under ``inverse_mass(case)``: ``hmc_f32_distance(case, variant,
# "hmc_mass")`` rounded up to two digits.  The mass changes what the formats cost (a drift of eps minv_j p_j rounds a larger step where
# minv_j = 4), so tests/test_gpu_hmc_mass.py takes 4 x THIS distance, not the unit-mass one.
HMC_MASS_F32_DISTANCE = {
    "d65_pbc": {"b1": (1.1e-05, 8.4e-06), "b037_textbook": (7.3e-06, 6.3e-06)},
    "d257_d0": {"b1": (2.2e-05, 2.1e-05), "b037_textbook": (2.5e-05, 2.1e-05)},
    "17x17_db": {"b1": (1.4e-05, 1.4e-05), "b037_textbook": (7e-06, 8.7e-06)},
    "d1025_d0": {"b1": (7.1e-05, 6.2e-05), "b037_textbook": (4.7e-05, 5.1e-05)},
    "d2048_pbc": {"b1": (0.00017, 0.00021), "b037_textbook": (0.00012, 0.00012)},
}


def scan(case, sampler, variant, grid):
    """Of the step sizes of ``grid`` with at most one chain per step inside the band and none within a quarter of its width of its
    edge: the one with the most even mix of accepted and rejected proposals (at least 2 of each), or None."""
    best, best_score = None, 1
    for eps in grid:
        res = oracle_run(case, sampler, variant, eps)
        acc, ratio = np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
        score = min(acc.sum(), (~acc).sum())
        if score > best_score and ((ratio <= 1.0).sum(1) <= 1).all() and not ((ratio > 0.75) & (ratio < 1.25)).any():
            best, best_score = float(eps), score
    return best


def _up2(v):
    """v rounded up to two significant digits."""
    e = int(np.floor(np.log10(v))) - 1
    return float(f"{np.ceil(v / 10.0 ** e) * 10.0 ** e:.2g}")


if __name__ == "__main__":                            # prints the STEP_SIZES table; with --mass, MASS_STEP_SIZES and HMC_MASS_F32_DISTANCE
    import sys
    if sys.argv[1:2] == ["--mass"]:
        grid = [float(f"{10.0 ** (-4 + k / 12):.2g}") for k in range(43)]
        for case in sys.argv[2:] or MASS_CASES:
            MASS_STEP_SIZES[case] = {v: scan(case, "hmc_mass", v, grid) for v in VARIANTS}
            print(f'    "{case}": {MASS_STEP_SIZES[case]},', flush=True)
        for case in sys.argv[2:] or MASS_CASES:
            row = {v: tuple(_up2(x) for x in hmc_f32_distance(case, v, "hmc_mass")) for v in VARIANTS}
            print(f'    "{case}": {row},', flush=True)
        sys.exit(0)
    grids = {"mala": [float(f"{10.0 ** (-7 + k / 12):.2g}") for k in range(73)],      # 1e-7 .. 1e-1
             "hmc": [float(f"{10.0 ** (-4 + k / 12):.2g}") for k in range(43)]}       # 1e-4 .. 0.3
    for case in sys.argv[1:] or list(CASES):
        row = {s: {v: scan(case, s, v, grids[s]) for v in VARIANTS} for s in SAMPLERS}
        print(f'    "{case}": {row},', flush=True)
