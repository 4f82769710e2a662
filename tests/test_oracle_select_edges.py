"""The oracle's semantics of the CIS categorical selection on degenerate weight tables (vanished, overflowing and NaN weights), pinned
with hard-coded indices, and ``cis_step == cis_select`` on ``cis_step``'s own solves.

PARITY UNPINNED: the expectations rest on numpy's ``searchsorted`` order, in which NaN sorts LAST and equal to itself, so
``searchsorted(table, NaN)`` is the index of the table's first NaN (0 on an all-NaN table) and a finite query stops at the first NaN
entry at the latest.  jax's sort comparators (``jax.random.choice`` -> ``jnp.searchsorted``) share that order; jax cannot be imported
here, so it is restated, not checked."""
import numpy as np
import pytest

from oracle import flow, mala, prng, targets
from tests import select_cases as sc

KEYS = [prng.PRNGKey(s) for s in (0, 1, 7, 55, 2 ** 40 + 3)]


def _choice(key, w):
    """``exe_flow_matching.py:290-292`` on a weight table: normalise by the sum, inverse-CDF draw, gather clamp."""
    w = np.asarray(w, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        norm = w / w.sum()
    return int(np.minimum(prng.choice_p(key, norm), w.size - 1))


@pytest.mark.parametrize("table,expect", [
    ([0, 0, 0, 0, 0, 0], 0),                     # every weight underflows: 0 / 0, the current state is kept
    ([1e-300, 0, np.inf, 0, 3, 0], 2),           # the overflowing entry
    ([np.nan, 1, 1, 1, 1, 1], 0),
    ([1, 1, np.nan, 1, 1, 1], 0),                # a NaN anywhere poisons the sum, hence the whole table
    ([0, 0, 1e-320, 0, 0, 0], 2),
    ([2, 0, 0, 0, 0, 0], 0),
    ([0, 0, 0, 0, 0, 5], 5),
    ([0, np.inf, 0, np.inf, 0, 0], 1),           # the first of two overflowing entries
])
def test_choice_on_degenerate_tables(table, expect):
    """The draw on these tables does not depend on the uniform: one index for every key."""
    assert [_choice(k, table) for k in KEYS] == [expect] * len(KEYS)


def test_searchsorted_orders_nan_last():
    cum = np.array([0.0, 0.5, np.nan, np.nan])
    assert np.searchsorted(cum, np.nan) == 2 and np.searchsorted(cum, 0.7) == 2 and np.searchsorted(cum, 0.5) == 1
    assert np.searchsorted(np.full(4, np.nan), np.nan) == 0 and np.searchsorted(np.full(4, np.nan), 0.3) == 0


def test_cis_select_degenerate_scenarios():
    """The scenarios tests/test_gpu_select_edges.py launches (NaN ``lps`` entry, NaN current ``logp``, only the current state /
    only the last sample / only a middle sample surviving, overflows): hard-coded indices, for several keys."""
    inp = sc.cis_degenerate_inputs()
    B, n_is = inp["pos"].shape[0], 5
    nd = len(sc.DEGENERATE)
    expect = np.array([e for _, _, e in sc.DEGENERATE])
    for key in KEYS:
        state, info, stats, margin = sc.cis_oracle(inp, prng.split_at(key, B, np.arange(B)), n_is, 1.0)
        np.testing.assert_array_equal(stats["choice"][:nd], expect, err_msg=str([n for n, _, _ in sc.DEGENERATE]))
        np.testing.assert_array_equal(info.is_accepted[:nd], expect != 0)
        np.testing.assert_array_equal(sc.choice_from_pos(state.position.astype(np.float32), inp, n_is), stats["choice"])
        # the log-density follows the selection; a rejected NaN / overflowing current value stays
        pick = np.arange(B) * n_is + np.maximum(stats["choice"] - 1, 0)
        np.testing.assert_array_equal(state.logdensity, np.where(stats["choice"] > 0, inp["lps"][pick], inp["logp"]))
        assert np.isfinite(stats["norm"][nd:]).all() and np.isfinite(margin[nd:]).all()
    # weights of the selected entries: 1 where one entry survives, NaN on the poisoned tables
    names = [n for n, _, _ in sc.DEGENERATE]
    w = info.acceptance_rate[:nd]
    assert all(w[names.index(n)] == 1.0 for n in ("only_current", "only_last", "only_middle"))
    assert all(np.isnan(w[names.index(n)]) for n in names if n not in ("only_current", "only_last", "only_middle"))


def test_cis_step_is_cis_select_on_its_own_solves():
    from tests import gpu_util as gu
    B, n_is = 8, 3
    args, dist, k, model, state = gu.gmm4_setup(B=B, hutchs=False, num_importance_samples=n_is)
    params = gu.rand_params(model, seed=9, out_scale=0.3)
    vg = targets.Tempered(dist, 0.9).value_and_grad
    st = mala.init(dist.init_params.astype(np.float32).astype(np.float64), vg)
    keys = prng.split(prng.PRNGKey(55), B)
    stats = {}
    new, info = flow.cis_step(keys, st, vg, model, params, args, stats)
    new2, info2, sel = flow.cis_select(keys, st, stats["u0"], stats["vol0"], stats["refs"], stats["xs"], stats["vols"], stats["lps"],
                                       n_is, targets.REF_VARS[args.ref_dist])
    for a, b in zip(tuple(new) + tuple(info), tuple(new2) + tuple(info2)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(sel["norm"], stats["norm"])
    np.testing.assert_array_equal(sel["choice"], stats["choice"])
    assert set(stats) == {"u0", "vol0", "refs", "xs", "vols", "lps", "norm", "choice"}
    assert info.is_accepted.any() and len(set(stats["choice"])) > 1
