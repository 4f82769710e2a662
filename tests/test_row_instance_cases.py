"""The conditions tests/test_gpu_row_instances.py relies on, asserted on the float64 oracle alone (no device): with the committed step
sizes every case and variant sees accepted AND rejected proposals within its three steps, and per step at most 1 of the 16 chains
lies inside the borderline band the device comparison leaves out -- so that test cannot pass by excluding the chains that matter.
Also the case table itself: every (MAXIT, BCRT) instance above d = 64 has a case at its first and at its last dimension."""
import numpy as np
import pytest

from tests import row_instance_cases as rc


def test_the_table_covers_every_instance_at_its_boundary_dimensions():
    dims = {}
    for case, (d, L, bc, n_total, off) in rc.CASES.items():
        dims.setdefault((rc.maxit(d), rc.bcrt(case)), set()).add(d)
        assert set(rc.STEP_SIZES[case]) == set(rc.SAMPLERS) and all(set(v) == set(rc.VARIANTS) for v in rc.STEP_SIZES[case].values()), case
    for b in (False, True):
        assert 65 in dims[(4, b)]
        assert {257, 1024} <= dims[(16, b)]
        assert {1025, 2048} <= dims[(32, b)]
    assert {289, 1024, 1089, 2025} <= dims[(16, True)] | dims[(32, True)]                # lattices with L > 16: up / down neighbours in another lane
    assert [rc.maxit(d) for d in (64, 65, 256, 257, 1024, 1025, 2048)] == [1, 4, 4, 16, 16, 32, 32]
    assert any(off > 0 and d == 2048 for d, L, bc, n_total, off in rc.CASES.values())


@pytest.mark.parametrize("variant", list(rc.VARIANTS))
@pytest.mark.parametrize("sampler", rc.SAMPLERS)
@pytest.mark.parametrize("case", list(rc.CASES))
def test_both_decisions_occur_and_the_band_excludes_at_most_one_chain(case, sampler, variant):
    res = rc.oracle_run(case, sampler, variant)
    acc = np.stack([r[0] for r in res])
    assert 0 < acc.sum() < acc.size, (case, sampler, variant, int(acc.sum()))
    for j, (_, ratio, _) in enumerate(res):
        assert (ratio <= 1.0).sum() <= 1, (case, sampler, variant, j, int((ratio <= 1.0).sum()))


def test_the_mass_cases_cover_the_cells_above_d_256_and_the_boundary_at_maxit_4():
    cells = {(rc.maxit(rc.CASES[c][0]), rc.bcrt(c)) for c in rc.MASS_CASES}
    assert cells == {(4, True), (16, False), (16, True), (32, False), (32, True)}
    assert any(rc.CASES[c][1] and rc.CASES[c][2] == "db" for c in rc.MASS_CASES)           # a lattice with a held frame among them
    assert set(rc.MASS_STEP_SIZES) == set(rc.HMC_MASS_F32_DISTANCE) == set(rc.MASS_CASES)
    for c in rc.MASS_CASES:
        m = rc.inverse_mass(c)
        assert m.shape == (rc.CASES[c][0],) and m.min() == 0.25 and abs(m.max() - 4.0) < 1e-12


@pytest.mark.parametrize("variant", list(rc.VARIANTS))
@pytest.mark.parametrize("case", rc.MASS_CASES)
def test_mass_both_decisions_occur_and_the_band_excludes_at_most_one_chain(case, variant):
    """The conditions of the unit-mass cases, for the step under ``inverse_mass(case)``; and none of the chains sits near the band's
    edge (within a quarter of its width), as ``scan`` chose."""
    res = rc.oracle_run(case, "hmc_mass", variant)
    acc = np.stack([r[0] for r in res])
    assert 0 < acc.sum() < acc.size, (case, variant, int(acc.sum()))
    for j, (_, ratio, _) in enumerate(res):
        assert (ratio <= 1.0).sum() <= 1, (case, variant, j, int((ratio <= 1.0).sum()))
        assert not ((ratio > 0.75) & (ratio < 1.25)).any(), (case, variant, j)


@pytest.mark.parametrize("case", rc.MASS_CASES)
def test_the_mass_float32_distance_table_is_the_restatement_against_the_oracle(case):
    for variant in rc.VARIANTS:
        for got, kept in zip(rc.hmc_f32_distance(case, variant, "hmc_mass"), rc.HMC_MASS_F32_DISTANCE[case][variant]):
            assert got <= kept <= 1.11 * got, (case, variant, got, kept)
        # outside the band the device-format restatement makes the float64 restatement's decisions
        from oracle import mala as omala
        vg = rc.value_and_grad(case, variant)
        st = omala.init(rc.start_state(case).astype(np.float64), vg)
        for j in range(rc.N_STEPS):
            keys = rc.step_keys(case, j, "hmc_mass")[1]
            new, info, u = rc.oracle_step("hmc_mass", variant, st, vg, keys, rc.MASS_STEP_SIZES[case][variant])
            lpa = rc.hmc_step_f32(case, variant, st, keys, rc.MASS_STEP_SIZES[case][variant], rc.inverse_mass(case))[0]
            out = ~rc.borderline("hmc_mass", st, info, u)
            np.testing.assert_array_equal((u < np.exp(lpa))[out], info.is_accepted[out])
            st = omala.init(new.position.astype(np.float32).astype(np.float64), vg)
    grid = [float(f"{10.0 ** (-4 + k / 12):.2g}") for k in range(43)]
    assert rc.scan(case, "hmc_mass", "b1", grid) == rc.MASS_STEP_SIZES[case]["b1"]


def test_start_states_are_near_a_mode():
    """|log pi| of the start states at beta = 1: the scale the tolerances of the device test are relative to."""
    from oracle import mala
    worst = {}
    for case in rc.CASES:
        st = mala.init(rc.start_state(case).astype(np.float64), rc.value_and_grad(case, "b1"))
        worst[case] = np.abs(st.logdensity).max()
        d, L, bc, _, _ = rc.CASES[case]
        assert worst[case] < (2.5e3 if L else 50.0), (case, worst[case])


@pytest.mark.parametrize("case", list(rc.CASES))
def test_the_float32_distance_table_is_the_restatement_against_the_oracle(case):
    """``HMC_F32_DISTANCE`` holds what ``hmc_f32_distance`` computes (rounded up to two digits): the wider energy bounds of the device
    test come from the number formats, measured on the oracle, not from a kernel's output."""
    for variant in rc.VARIANTS:
        for got, kept in zip(rc.hmc_f32_distance(case, variant), rc.HMC_F32_DISTANCE[case][variant]):
            assert got <= kept <= 1.11 * got, (case, variant, got, kept)
