"""CPU tests of tests/ghmc_ref.py, the float64 restatement of the GHMC transition (``mfm_ghmc_*``), and of tests/ghmc_cases.py."""
import numpy as np
import pytest

from oracle import hmc as ohmc, prng
from oracle.mala import MALAState
from tests import ghmc_cases as gc
from tests import ghmc_ref as ref

SIGMA = np.array([0.5, 1.0, 2.0])                       # the target: N(0, diag(SIGMA^2)), no correlation
MINV = np.array([0.3, 1.0, 3.0])                        # a non-unit diagonal inverse mass that is NOT the target's covariance


def _gauss_vg(x):
    return -0.5 * ((x / SIGMA) ** 2).sum(1), -x / SIGMA ** 2


def _stationary_start(n, key):
    k = prng.split(key, 3)
    x = prng.normal_rows(prng.split(k[0], n), 3) * SIGMA
    p = prng.normal_rows(prng.split(k[1], n), 3) / np.sqrt(MINV)
    s = 2.0 * prng.uniform_rows(prng.split(k[2], n)) - 1.0
    lp, g = _gauss_vg(x)
    return ref.State(x, p, lp, g, s)


def test_the_transition_leaves_a_gaussian_invariant_under_a_non_unit_mass():
    """n chains start from the invariant law p(x) N(p; 0, M) U(s) and make 300 transitions; every 20th state is a sample of n draws of
    that law if, and only if, the transition leaves it invariant.  For n independent draws the sample variance of a coordinate has
    relative standard deviation sqrt(2 / (n - 1)), the mean of |s| standard deviation sqrt(1 / 12 / n) and the mean of s^2
    sqrt(4 / 45 / n); the average of identically distributed estimates over the kept states varies no more than one of them.  The bound
    is 5 of these standard deviations: 11 %, 0.023 and 0.023 at n = 4096 (a broken rule -- no momentum flip, s not rescaled -- misses by
    far more: at step size 1.3 a third of the proposals are rejected)."""
    n, steps, thin = 4096, 300, 20
    st = _stationary_start(n, prng.PRNGKey(11))
    var, m1, m2, acc = [], [], [], []
    for j, kj in enumerate(prng.split(prng.PRNGKey(12), steps)):
        st, info = ref.step(prng.split(kj, n), st, _gauss_vg, 1.3, 0.4, 0.2, MINV)
        acc.append(info.is_accepted.mean())
        assert (np.abs(st.slice) <= 1.0).all()
        if (j + 1) % thin == 0:
            var.append(st.position.var(0)); m1.append(np.abs(st.slice).mean()); m2.append((st.slice ** 2).mean())
    rate = float(np.mean(acc))
    print(f"acceptance {rate:.3f}; var / sigma^2 {np.mean(var, 0) / SIGMA ** 2}; E|s| {np.mean(m1):.4f}; E s^2 {np.mean(m2):.4f}")
    assert 0.3 < rate < 0.9                                            # the accept test is at work both ways
    assert np.abs(np.mean(var, 0) / SIGMA ** 2 - 1.0).max() <= 5 * np.sqrt(2.0 / (n - 1))
    assert abs(np.mean(m1) - 0.5) <= 5 * np.sqrt(1.0 / 12.0 / n)
    assert abs(np.mean(m2) - 1.0 / 3.0) <= 5 * np.sqrt(4.0 / 45.0 / n)
    pvar = st.momentum.var(0) * MINV                                   # p ~ N(0, 1 / minv)
    assert np.abs(pvar - 1.0).max() <= 5 * np.sqrt(2.0 / (n - 1))


def test_rejection_negates_the_refreshed_momentum_and_keeps_the_rest():
    n = 64
    st = _stationary_start(n, prng.PRNGKey(21))
    keys = prng.split(prng.PRNGKey(22), n)
    new, info = ref.step(keys, st, _gauss_vg, 1.9, 0.3, 0.15, MINV)     # a step near the stability limit: many rejections
    rej = ~info.is_accepted
    assert rej.sum() >= 8 and (~rej).sum() >= 8
    refreshed = ref.refresh(st.momentum, keys, 0.3, MINV)
    np.testing.assert_array_equal(new.momentum[rej], -refreshed[rej])
    np.testing.assert_array_equal(new.position[rej], st.position[rej])
    np.testing.assert_array_equal(new.logdensity[rej], st.logdensity[rej])
    np.testing.assert_array_equal(new.logdensity_grad[rej], st.logdensity_grad[rej])
    drifted = ref.slice_drift(st.slice, 0.15)
    np.testing.assert_array_equal(new.slice[rej], drifted[rej])
    np.testing.assert_array_equal(new.slice[~rej], (drifted * np.exp(info.energy_change))[~rej])
    np.testing.assert_array_equal(new.position[~rej], info.proposed_position[~rej])
    assert (np.abs(new.slice) <= 1.0).all()
    np.testing.assert_array_equal(info.is_accepted, np.abs(drifted) <= np.exp(-info.energy_change))
    np.testing.assert_array_equal(info.acceptance_rate, np.minimum(1.0, np.exp(-info.energy_change)))


def test_a_nan_energy_change_rejects():
    n = 8
    st = _stationary_start(n, prng.PRNGKey(31))

    def vg(x):
        lp, g = _gauss_vg(x)
        return np.where(np.arange(n) % 2 == 0, np.nan, lp), g
    new, info = ref.step(prng.split(prng.PRNGKey(32), n), st._replace(slice=np.zeros(n)), vg, 0.1, 0.5, 0.0, None)
    assert not info.is_accepted[::2].any() and (info.acceptance_rate[::2] == 0).all()
    np.testing.assert_array_equal(new.position[::2], st.position[::2])


def test_the_slice_drift_wraps_into_the_interval():
    s = np.array([-0.99, -0.5, 0.0, 0.5, 0.9, 0.99])
    for delta in (0.0, 0.15, 0.5, 1.0, 2.5):
        out = ref.slice_drift(s, delta)
        assert ((out >= -1.0) & (out < 1.0)).all()
        np.testing.assert_allclose(np.mod(out - s - delta + 1.0, 2.0) - 1.0, 0.0, atol=1e-15)


@pytest.mark.parametrize("mass", [False, True])
def test_alpha_one_is_the_hmc_oracle_at_one_leapfrog_step(mass):
    """alpha = 1: the refresh is 0 p + 1 n, so the proposal and the acceptance probability are those of oracle/hmc.py at one leapfrog
    step on the same keys, bit for bit at unit mass; with a mass the momentum n / sqrt(minv) is handed to the oracle in x' = M^-1/2 x
    coordinates, where the two agree to rounding."""
    case = "d65_d0"
    vg = gc.value_and_grad(case)
    x = gc.start_state(case).astype(np.float64)
    st = ref.init(x, vg, gc.init_key(case), None, gc.n_chains(case))
    keys = gc.step_key(case, 0)[1]
    eps = gc.STEP_SIZES[case][False]
    if not mass:
        new, info = ref.step(keys, st, vg, eps, 1.0, 0.5, None)
        _, oinfo, _ = ohmc.kernel(keys, MALAState(x, st.logdensity, st.logdensity_grad), vg, eps, 1)
        np.testing.assert_array_equal(info.proposed_position, oinfo.proposed_position)
        np.testing.assert_array_equal(info.acceptance_rate, oinfo.acceptance_rate)
        np.testing.assert_array_equal(info.energy_change, -oinfo.energy_delta)
        return
    minv = gc.inverse_mass(gc.dim(case))
    new, info = ref.step(keys, st, vg, eps, 1.0, 0.5, minv)
    # HMC with inverse mass minv on x is unit-mass HMC on y = x / sqrt(minv): value_and_grad in y, momentum n
    sq = np.sqrt(minv)

    def vg_y(y):
        lp, g = vg(y * sq)
        return lp, g * sq
    lp0, g0 = vg_y(x / sq)
    _, oinfo, _ = ohmc.kernel(keys, MALAState(x / sq, lp0, g0), vg_y, eps, 1)
    np.testing.assert_allclose(info.proposed_position, oinfo.proposed_position * sq, rtol=0, atol=1e-14)
    np.testing.assert_allclose(info.acceptance_rate, oinfo.acceptance_rate, rtol=0, atol=1e-10)


def test_unit_inverse_mass_gives_the_unit_form_bits():
    case = "d65_d0"
    vg = gc.value_and_grad(case)
    st = ref.init(gc.start_state(case).astype(np.float64), vg, gc.init_key(case), None, gc.n_chains(case))
    keys = gc.step_key(case, 0)[1]
    a, ia = ref.step(keys, st, vg, 0.03, 0.3, 0.15, None)
    b, ib = ref.step(keys, st, vg, 0.03, 0.3, 0.15, np.ones(gc.dim(case)))
    for u, v in zip(a + ia, b + ib):
        np.testing.assert_array_equal(u, v)


def test_init_draws_from_the_two_halves_of_the_chain_key():
    p, s = ref.init_momentum_slice(prng.PRNGKey(3), 8, 5, np.full(5, 4.0), offset=2, n=4)
    kk = prng.split_rows(prng.split(prng.PRNGKey(3), 8)[2:6], 2)
    np.testing.assert_array_equal(p, prng.normal_rows(kk[:, 0], 5) / 2.0)
    np.testing.assert_array_equal(s, 2.0 * prng.uniform_rows(kk[:, 1]) - 1.0)
    assert ((s >= -1) & (s < 1)).all()


# ---- tests/ghmc_cases.py: what the GPU test relies on, for the restatement alone ---------------------------------------------------------
@pytest.mark.parametrize("mass", gc.MASSES)
@pytest.mark.parametrize("case", gc.CASES)
def test_the_cases_tables_are_what_measure_computes_and_no_decision_is_borderline(case, mass):
    tol = gc.tolerance(case, mass)
    assert tol == gc.TOLERANCE[case][mass], (case, mass, tol)
    assert all(0 < v < 1e-3 for v in tol)                              # the formats cost something, and little
    m, acc = gc.margins(case, mass)
    print(f"{case} mass {mass}: accepted {acc.sum(1)}, of {acc.shape[1]}; smallest | log|s| + dH | {m.min():.3g} (dH tolerance {tol[3]:.3g})")
    assert m.min() > 10 * tol[3]                                       # no |s| within the tolerance of exp(-dH)
    assert acc.sum() >= 2 and (~acc).sum() >= 2                        # both decisions occur
    assert gc.alpha_one_both(case, mass) >= 2                          # the alpha = 1 comparison with HMC has chains to compare
    for _, (s64, i64), (s32, i32) in gc.walk(case, mass):
        np.testing.assert_array_equal(i64.is_accepted, i32.is_accepted)


def test_the_step_size_table_is_what_scan_chooses():
    grid = [float(f"{10.0 ** (-3 + k / 12):.2g}") for k in range(37)]
    for case in ("gmm4", "d64_pbc"):
        for mass in gc.MASSES:
            assert gc.scan(case, mass, grid) == gc.STEP_SIZES[case][mass]
