"""The conditions of tests/nuts_cases.py, checked on the CPU with the reference alone (tests/nuts_ref.py), so that the GPU comparison of
tests/test_gpu_nuts_instances.py is known to be meaningful before a kernel runs:

* every case launches under the chains per workgroup it names (``mfm_nuts_launch_plan``), and so do the placement test's geometries and
  the deep-limit cases of the run-equals-steps and warmup-replay tables;
* per case and mass, exactly as ``burned`` runs it (64 chains, 30 burn-in transitions at limit 6 on keys 900 + it, 3 transitions under
  the case's limit on keys 50 + it, continued from the reference's own state): no divergent burn-in, the borderline share at most 0.25 in
  every transition (the rule and the cap of tests/test_gpu_nuts.py), both directions drawn, the case marked deep realizes depth >= 9, and
  a case whose limit is 10 or more has at least 8 chain-transitions that stop inside a subtree (the checkpoint walk decided them);
* the position probe (``nuts_util.position_probe``) changes no non-borderline chain's depth or leapfrog count; its displacement gives
  the case's position bound."""
import numpy as np
import pytest

from tests import nuts_cases as nc, nuts_util as nu


def test_every_case_runs_under_the_geometry_it_names():
    from mfm_amd import _lib
    for name, c in nc.CASES.items():
        waves, lds, per_cu = _lib.nuts_launch_plan(c.d, c.limit)
        print(f"{name}: d {c.d} limit {c.limit}: {waves} chains per workgroup, {lds} B, {per_cu} workgroups per CU")
        assert waves == c.waves, (name, waves, c.waves)
    assert _lib.nuts_launch_plan(130, 16)[1] == 127040
    assert {c.waves for c in nc.CASES.values()} == {1, 2, 3, 4}
    assert {(c.d + 63) // 64 for c in nc.CASES.values()} == {1, 2, 3, 4}           # MAXIT 1, 2, and 4 with three and with four rows
    for d, limit, _, _, waves in nc.PLACEMENT:
        assert _lib.nuts_launch_plan(d, limit)[0] == waves, (d, limit)
    assert {w for *_, w in nc.PLACEMENT} == {1, 2, 3, 4}
    # tests/test_gpu_nuts.py: BITS, tests/test_gpu_nuts_warmup.py: REPLAY_CASES
    assert [_lib.nuts_launch_plan(d, limit)[0] for d, limit in ((64, 12), (128, 14), (256, 14))] == [1, 1, 2]


@pytest.mark.parametrize("name,mass", nc.RUNS, ids=nc.RUN_IDS)
def test_the_reference_alone_meets_the_conditions_of_the_comparison(name, mass):
    c = nc.CASES[name]
    ref = nu.burned(*nc.spec(name, mass))
    infos, shares = ref["infos"], ref["shares"]
    hist = np.sum([np.bincount(i.depth, minlength=c.limit + 1) for i in infos], 0)
    in_sub = sum(int(i.stopped_in_subtree.sum()) for i in infos)
    disp, changed = nu.position_probe(*nc.spec(name, mass))
    common = 3e-6 * max(1.0, max(np.abs(st_n.position).max() for _, st_n in ref["states"]))
    print(f"{name} mass={mass}: d {c.d} tail {c.tail} eps {c.eps[mass]} limit {c.limit} chains/WG {c.waves}; borderline shares "
          f"{[round(float(s), 3) for s in shares]}; depths {hist.tolist()}; leapfrog max {max(i.num_leapfrog.max() for i in infos)}; "
          f"stopped in a subtree {in_sub}; divergent burn-in {ref['burn_divergent']}; probe displacement {disp:.2e} "
          f"(changed trees {changed}), position bound max({common:.2e}, {4 * disp:.2e})")
    assert ref["burn_divergent"] == 0
    assert max(shares) <= 0.25, shares
    assert any((i.directions > 0).any() for i in infos) and any((i.directions < 0).any() for i in infos)
    if c.deep:
        assert max(i.depth.max() for i in infos) >= 9
    if c.limit >= 10:
        assert in_sub >= 8, in_sub
    assert changed == 0, changed
    assert np.isfinite(disp) and (disp > 0.0 or c.limit == 1)                     # (one leaf: its position is set by the start's gradient alone)
