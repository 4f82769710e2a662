"""CPU tests of tests/chees_cases.py: on the float64 restatement alone, the conditions tests/test_gpu_chees.py rests on.  No decision of
any case's run is near its threshold -- the device's float32 positions cannot flip an accept / reject, a divergence flag or a leapfrog
count -- the table covers the branches it is meant to cover, and the recorded tolerances are the measured ones."""
import numpy as np
import pytest

from tests import chees_cases as cc, chees_ref as cr


@pytest.mark.parametrize("case", list(cc.CASES))
def test_no_decision_is_near_its_threshold(case):
    u_gap, dh_gap, int_gap = cc.margins(case)
    print(f"{case}: min |u - alpha| {u_gap:.3g}, min |dH - threshold| / threshold {dh_gap:.3g}, min distance of tau / eps from an integer {int_gap:.3g}")
    assert u_gap > 1e-3
    assert dh_gap > 1e-3                 # (the energy change of a chain near the threshold of 1000 moves by far less than 1 with float32 positions)
    assert int_gap > 1e-6
    a, b = cc.reference(case, False), cc.reference(case, True)
    for ra, rb in zip(a["records"], b["records"]):               # and the float32 variant indeed makes the same decisions
        np.testing.assert_array_equal(ra.accepted, rb.accepted)
        np.testing.assert_array_equal(ra.div, rb.div)
    np.testing.assert_array_equal(a["trace"][:, 2], b["trace"][:, 2])


def test_the_table_covers_its_branches():
    traces = {c: cc.reference(c)["trace"] for c in cc.CASES}
    n_div = {c: t[:, 5] for c, t in traces.items()}
    assert any(((v > 0) & (v < cc.CASES[c]["n_valid"])).any() for c, v in n_div.items())        # some chains divergent
    assert any((v == cc.CASES[c]["n_valid"]).any() for c, v in n_div.items())                   # all of them
    clamped = [c for c, t in traces.items()
               if any(np.ceil(cr.radical_inverse(i + 1) * r[1] / r[0]) > cc.CASES[c]["max_leapfrog"] for i, r in enumerate(t))]
    assert clamped
    assert any(v["n_valid"] < v["B"] for v in cc.CASES.values())
    assert {v["key_mode"] for v in cc.CASES.values()} == {0, 1}
    assert any(v["mass"] for v in cc.CASES.values())
    for c, t in traces.items():                                  # every case holds accepted and rejected trajectories and several lengths
        acc = np.concatenate([r.accepted for r in cc.reference(c)["records"]])
        assert 0 < acc.sum() < acc.size, c
        assert len(set(t[:, 2])) >= 3, c


@pytest.mark.parametrize("case", list(cc.CASES))
def test_recorded_tolerances_are_the_measured_ones(case):
    got, rec = cc.measure(case), cc.TOLERANCE[case]
    print(case, ["%.3g" % v for v in got])
    for g, r in zip(got, rec):
        assert (g == 0 and r == 0) or abs(g - r) <= 0.05 * g + 1e-12, (case, got, rec)      # (recorded to two digits)
