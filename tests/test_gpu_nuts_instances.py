"""GPU tests of the No-U-turn kernels on every instance and launch geometry of tests/nuts_cases.py (MAXIT 1 / 2 / 4 with three and four
rows, the run-time boundary and the lattice, the mass; 1, 2, 3 and 4 chains per workgroup; trees to depth 9; ``max_tree_depth`` 1).

REFERENCE PARITY: the loop of tests/test_gpu_nuts.py (``nuts_util._transitions_against_the_reference``) on every run of the table, from
the reference's burned state, over the chains that are not borderline: depth, leapfrog count and both flags exactly, log-density, rate
and energy within that file's bounds, the position within ``max(3e-6 max(1, |x|max), 4 x the case's probe displacement)``
(tests/nuts_cases.py).  The conditions of the comparison are asserted on the reference alone in tests/test_nuts_cases.py.

PLACEMENT INVARIANCE (device only): with per-chain keys a chain's outcome is a function of its key and state alone.  64 chains, burnt
in on the device by 30 transitions at limit 6, are run once; fresh contexts of 16 chains (a context's chain count is a multiple of 16: the smallest there is) get rows and keys picked out of
order from the 64 (the last row, one from the middle of a workgroup, one from a workgroup's last wave, ...), in three orders that move
every row to another workgroup, wave and neighbourhood, and must return every bit: a checkpoint slab shared by two waves, a wrong chain
index, exit guard or pad row makes a chain depend on where it sits and on its neighbours.  (At 3 chains per workgroup both the 64 and
the 16 leave waves of the last workgroup past the end: the ``b >= B`` exit.)"""
import numpy as np
import pytest

from oracle import prng
from tests import hmc_mass_ref as hm, nuts_cases as nc, nuts_util as nu

pytestmark = pytest.mark.gpu

N_PLACE = 2                # transitions per placement run


@pytest.mark.parametrize("name,mass", nc.RUNS, ids=nc.RUN_IDS)
def test_every_instance_and_geometry_matches_the_reference(name, mass):
    from mfm_amd import _lib
    c = nc.CASES[name]
    assert _lib.nuts_launch_plan(c.d, c.limit)[0] == c.waves
    ref = nu.burned(*nc.spec(name, mass))
    floor = nc.position_floor(name, mass)
    print(f"{name} mass={mass}: borderline shares of the reference-only pass {ref['shares']}; position bound floor {floor:.2e}")
    assert max(ref["shares"]) <= 0.25, ref["shares"]
    worst = nu._transitions_against_the_reference("phi4", c.d, c.tail, c.eps[mass], c.limit, ref["minv"], ref["start"], f"{name} mass={mass}", floor)
    print(f"MEASURED {name} {'mass' if mass else 'unit'}: |pos diff| {worst[0]:.2e} |logp diff| {worst[1]:.2e} |rate diff| {worst[2]:.2e}")


N_SMALL = 16               # the smallest chain count a context takes (a multiple of 16)


def _placements(waves):
    """Three orders of 16 distinct rows of the 64: out of order (the last row first, then one from the middle of a workgroup and one
    from a workgroup's last wave), reversed, and rotated by one -- so that every row meets other neighbours, another workgroup and, with
    more than one chain per workgroup, another wave of it."""
    rows = [63, 5 * waves + waves // 2, 9 * waves + waves - 1, 2, 40, 17, 30, 0, 62, 33, 8, 51, 26, 47, 13, 58]
    assert len(set(rows)) == N_SMALL
    return rows, rows[::-1], rows[1:] + rows[:1]


@pytest.mark.parametrize("d,limit,mass,eps,waves", nc.PLACEMENT, ids=[f"d{g[0]}-limit{g[1]}-{g[4]}wave" for g in nc.PLACEMENT])
def test_a_chains_outcome_does_not_depend_on_its_place(d, limit, mass, eps, waves):
    import torch
    from mfm_amd import _lib
    assert _lib.nuts_launch_plan(d, limit)[0] == waves
    minv = hm.log_spaced_mass(d) if mass else None
    ctx, pos0, _ = nu._ctx("phi4", d, None)
    ctx.set_inverse_mass(minv)
    state0 = nu._init(ctx, pos0)
    ctx.nuts_run(prng.PRNGKey(60), 1.0, eps, nu.DEPTH, nu.BURN, *state0)       # (from the initial draw every tree turns by depth 5)
    keys = prng.split(prng.PRNGKey(61), nu.B)
    steps = nu._stepwise(ctx, state0, keys, eps, N_PLACE, limit)
    run = nu._run(ctx, state0, keys, eps, N_PLACE, limit)
    ctx.close()
    print(f"d {d} limit {limit} mass {mass}: depths {np.bincount(steps['depth'].reshape(-1)).tolist()}, leapfrog max {steps['num_leapfrog'].max()}, "
          f"divergent {int(steps['is_divergent'].sum())}")
    assert steps["depth"].max() >= min(3, limit)                               # (checkpoints were stored and walked)
    if limit > nc.LIMIT_REACHED:
        assert len(np.unique(steps["depth"])) >= 3
    else:
        assert (steps["depth"] == limit).mean() >= 0.25                         # (every slab's last slot was)
    for n, rows in enumerate(_placements(waves)):
        idx = torch.as_tensor(rows).cuda()
        small, _, _ = nu._ctx("phi4", d, None, N_SMALL)
        small.set_inverse_mass(minv)
        part0 = tuple(t[idx].contiguous() for t in state0)
        s = nu._stepwise(small, part0, keys[rows], eps, N_PLACE, limit)
        r = nu._run(small, part0, keys[rows], eps, N_PLACE, limit)
        small.close()
        for k in s:                                                             # position, log-density, gradient, the six info fields: [step, chain, ...]
            np.testing.assert_array_equal(s[k], steps[k][:, rows], err_msg=f"steps, placement {n}: {k}")
        for k in r:
            want = run[k][:, rows] if k.startswith("traj_") else run[k][rows]
            np.testing.assert_array_equal(r[k], want, err_msg=f"run, placement {n}: {k}")
