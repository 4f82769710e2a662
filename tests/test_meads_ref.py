"""CPU tests of tests/meads_ref.py, the float64 restatement of the MEADS warmup (``mfm_meads_warmup``), and of tests/meads_cases.py."""
import numpy as np
import pytest

from oracle import prng
from tests import meads_cases as mc
from tests import meads_ref as ref


def _planted(m, lam_true, seed):
    """X [m, d] with X^T X / m = diag(lam_true) EXACTLY (up to rounding): sqrt(m) Q sqrt(diag), Q with orthonormal columns."""
    d = len(lam_true)
    q, _ = np.linalg.qr(prng.normal_rows(prng.split(prng.PRNGKey(seed), m), d))
    return np.sqrt(m) * q * np.sqrt(np.asarray(lam_true))[None]


def test_lam_equals_the_direct_pair_sum():
    X = prng.normal_rows(prng.split(prng.PRNGKey(1), 12), 5) * np.array([3.0, 1.0, 0.5, 0.2, 2.0])
    assert ref.lam(X) == pytest.approx(ref.lam_direct(X), rel=1e-13)
    S = X @ X.T
    m = X.shape[0]
    direct = ((S ** 2).sum() - (np.diag(S) ** 2).sum()) / (m * (m - 1)) / (np.trace(S) / m)
    assert ref.lam(X) == pytest.approx(direct, rel=1e-15)


def test_lam_is_tr_c2_over_tr_c_on_a_planted_spectrum():
    """With C = X^T X / m, sum_ij S_ij^2 = m^2 tr C^2 and sum_i S_ii = m tr C, so
    lam = [m^2 tr C^2 - sum_i |x_i|^4] / (m (m - 1) tr C): tr C^2 / tr C up to the diagonal term, which is O(1 / m)."""
    lam_true = np.array([9.0, 4.0, 1.0, 0.25])
    target = (lam_true ** 2).sum() / lam_true.sum()
    for m in (50, 400, 3200):
        X = _planted(m, lam_true, 7 + m)
        np.testing.assert_allclose(X.T @ X / m, np.diag(lam_true), atol=1e-12)
        r4 = ((X * X).sum(1) ** 2).sum()
        exact = (m * m * (lam_true ** 2).sum() - r4) / (m * (m - 1) * lam_true.sum())
        assert ref.lam(X) == pytest.approx(exact, rel=1e-12)
        # |x_i|^2 <= m max_j q_ij^2 tr-weighted; here simply: the diagonal term's share of the numerator
        assert abs(ref.lam(X) - target) <= target / (m - 1) + r4 / (m * (m - 1) * lam_true.sum())
    assert abs(ref.lam(_planted(3200, lam_true, 1)) - target) < 0.01 * target
    # a rank-one ensemble: the estimate is the one non-zero eigenvalue
    v = np.outer(np.linspace(-1, 1, 9), np.array([1.0, 2.0, 2.0]))
    assert ref.lam(v) == pytest.approx((v * v).sum() / 9 * (1 - ((v * v).sum(1) ** 2).sum() / (v * v).sum() ** 2) * 9 / 8, rel=1e-12)


def _stats(eps, alpha=0.3, ok=True, d=3, minv=None):
    return ref.FoldStats(eps if ok else np.nan, alpha, alpha / 2, np.full(d, 2.0) if minv is None else minv, 1.0, 1.0)


def test_the_fold_roll_and_the_keep_rule():
    par = ref.initial_params(3, 3, 0.1, 0.5)
    np.testing.assert_array_equal(par.delta, [0.25] * 3)
    np.testing.assert_array_equal(par.minv, np.ones((3, 3)))
    new = ref.roll(par, [_stats(0.01), _stats(0.02), _stats(0.03)])
    np.testing.assert_array_equal(new.eps, [0.03, 0.01, 0.02])                      # fold f's statistics steer fold (f + 1) mod K
    np.testing.assert_array_equal(new.minv[1], [2.0] * 3)
    # non-finite eps, eps <= 0, a non-finite alpha, a non-finite minv entry: the receiving fold keeps ALL its previous parameters
    bad = [_stats(0.5, ok=False), _stats(0.0), ref.FoldStats(0.7, np.inf, np.inf, np.full(3, 2.0), 1.0, 1.0)]
    kept = ref.roll(new, bad)
    for a, b in zip(kept, new):
        np.testing.assert_array_equal(a, b)
    one = ref.roll(new, [_stats(0.9), _stats(0.8, minv=np.array([1.0, np.nan, 1.0])), _stats(0.7)])
    np.testing.assert_array_equal(one.eps, [0.7, 0.9, new.eps[2]])
    np.testing.assert_array_equal(one.minv[2], new.minv[2])
    np.testing.assert_array_equal(par.eps, [0.1] * 3)                               # roll does not write into its argument


def test_fold_stats_formulas_the_floor_and_the_clamp():
    x = prng.normal_rows(prng.split(prng.PRNGKey(5), 10), 4) * np.array([1.0, 2.0, 0.5, 3.0]) + 7.0
    g = -(x - 7.0) / np.array([1.0, 4.0, 0.25, 9.0])
    s = ref.fold_stats(x, g, 1)
    sd = x.std(0)
    np.testing.assert_allclose(s.minv, sd ** 2, rtol=1e-14)
    assert s.lam_y == pytest.approx(ref.lam((x - x.mean(0)) / sd), rel=1e-14) and s.lam_z == pytest.approx(ref.lam(g * sd), rel=1e-14)
    assert s.eps == min(1.0, 0.5 / np.sqrt(s.lam_z)) and s.delta == s.alpha / 2
    # t = 1: 1 / (t eps) >= 1 / eps >= 1 dominates 1 / sqrt(lam_y) here, so eps gamma = 1 and alpha = 1 - exp(-2)
    assert 1.0 / s.eps > 1.0 / np.sqrt(s.lam_y) and s.alpha == 1.0 - np.exp(-2.0 * s.eps * (1.0 / (1 * s.eps)))
    late = ref.fold_stats(x, g, 10 ** 6)                                            # the floor has fallen away
    assert late.alpha == 1.0 - np.exp(-2.0 * late.eps / np.sqrt(late.lam_y)) and late.alpha < s.alpha
    flat = ref.fold_stats(x, 1e-3 * g, 1)                                           # tiny gradients: 0.5 / sqrt(lam_z) > 1 is clamped
    assert flat.eps == 1.0 and 0.5 / np.sqrt(flat.lam_z) > 1.0
    same = ref.fold_stats(np.tile(x[:1], (10, 1)), g, 1)                            # a fold at one point: sd = 0, nothing is usable
    assert not same.usable and s.usable and flat.usable


def test_shuffle_bookkeeping():
    key = prng.PRNGKey(9)
    assert ref.n_shuffles(5, 2) == 2 and ref.n_shuffles(3, 2) == 1 and ref.n_shuffles(2, 2) == 0 and ref.n_shuffles(9, 0) == 0
    perms = ref.permutations(key, 5, 2, 16)
    assert perms.shape == (2, 16) and perms.dtype == np.int32
    for p in perms:
        np.testing.assert_array_equal(np.sort(p), np.arange(16))
    assert not np.array_equal(perms[0], perms[1]) and not np.array_equal(perms[0], np.arange(16))
    ident = np.arange(16)
    for t, want in ((1, ident), (2, ident), (3, perms[0]), (4, perms[0]), (5, perms[1])):
        np.testing.assert_array_equal(ref.perm_at(perms, t, 2, 16), want)
    np.testing.assert_array_equal(ref.perm_at(perms, 7, 0, 16), ident)
    from mfm_amd import random as jr                                                # the product's host draw is the same permutation
    from mfm_amd.bblackjax.adaptation.meads_adaptation import shuffle_permutations
    np.testing.assert_array_equal(shuffle_permutations(jr.PRNGKey(9), 5, 2, 16), perms)
    assert shuffle_permutations(jr.PRNGKey(9), 2, 2, 16).shape == (0, 16)


def test_warmup_uses_the_previous_folds_statistics_and_the_run_keys():
    case = "shuffle"
    res = mc.reference(case)
    B, n_valid, K, S, n_iter, step0, alpha0 = mc.shape(case)
    seen, _ = mc.states_before(case)
    perms = mc.permutations(case)
    m = n_valid // K
    for t in (1, 3):
        perm = ref.perm_at(perms, t, S, n_valid)
        for f in range(K):
            rows = perm[f * m:(f + 1) * m]
            s = ref.fold_stats(seen[t - 1].position[rows], seen[t - 1].logdensity_grad[rows], t)
            r = (f + 1) % K
            assert res.trace[t - 1, r, 0] == s.eps and res.trace[t - 1, r, 1] == s.alpha and res.trace[t - 1, r, 2] == s.delta
            assert res.trace[t - 1, f, 3] == s.lam_z and res.trace[t - 1, f, 4] == s.lam_y
            np.testing.assert_array_equal(res.mass_trace[t - 1, r], s.minv)
    np.testing.assert_array_equal(ref.step_keys(mc.run_key(case), n_iter, 2, B), prng.split(prng.split(mc.run_key(case), n_iter)[1], B))


# ---- tests/meads_cases.py: what the GPU test relies on, for the restatement alone -----------------------------------------------------
@pytest.mark.parametrize("case", mc.CASES)
def test_the_cases_table_no_borderline_decision_and_no_parameter_at_its_clamp(case):
    tol = mc.tolerance(case)
    assert tol == mc.TOLERANCE[case], (case, tol)
    # the formats cost something, and little; the eigenvalue tolerances carry the dot-product bound (d + 8) 2^-23 per Gram entry, which
    # at d = 1100 is 15 x what it is at d = 65, so above d = 320 they are held to 1e-2
    assert all(0 < v < 1e-3 for v in tol) or (mc.dim(case) > 320 and all(0 < v < 1e-2 for v in tol[:2]) and 0 < tol[2] < 1e-3)
    res = mc.reference(case)
    B, n_valid, K, S, n_iter, step0, alpha0 = mc.shape(case)
    m, acc = mc.decision_margins(case)
    print(f"{case}: accepted {acc[:, :n_valid].sum()}, rejected {(~acc[:, :n_valid]).sum()}; smallest | log|s| + dH | {m.min():.3g} (dH tolerance {tol[2]:.3g})")
    assert m.min() > 10 * tol[2]                                                  # no |s| within the tolerance of exp(-dH)
    assert acc.any() and (~acc).any()
    cm = mc.clamp_margins(case)
    rz, ry, _ = tol
    for t in range(1, n_iter + 1):
        for f in range(K):
            r = (f + 1) % K
            if np.isnan(cm[t - 1, f, 0]):                                         # statistics not finite: the receiving fold keeps its own
                assert (case, t, r) in mc.KEPT, (case, t, r)
                prev = (step0, alpha0, alpha0 / 2) if t == 1 else tuple(res.trace[t - 2, r, :3])
                assert tuple(res.trace[t - 1, r, :3]) == prev
                continue
            assert (case, t, r) not in mc.KEPT
            assert cm[t - 1, f, 0] > 10 * rz, (case, t, f, "eps at its clamp")     # 0.5 / sqrt(lam_z) is not within the tolerance of 1
            assert cm[t - 1, f, 1] > 10 * (rz + ry), (case, t, f, "gamma at its floor's edge")
    assert np.isfinite([res.eps, res.alpha, res.delta]).all() and np.isfinite(res.minv).all() and (res.minv > 0).all()


def test_the_cases_reach_what_they_are_meant_to():
    un = mc.reference("unstable")
    assert un.trace[0, 1, 0] == 1.0 and un.trace[0, 1, 5] == 0.0 and not un.decisions[0, 8:].any()      # step0 kept, every proposal rejected
    assert un.trace[1:, 1, 5].min() > 0.5 and un.trace[1, 1, 0] < 1.0                                      # ... and it recovers
    floor = mc.clamp_margins("gmm4_k2")[:, :, 2]
    assert floor[0].all() and not floor[-1].any()                                   # both branches of gamma occur
    assert all(mc.clamp_margins(c)[:, :, 2][np.isfinite(mc.clamp_margins(c)[:, :, 2])].all() for c in ("d65_k4", "m80"))
    sh = mc.permutations("shuffle")
    assert sh.shape == (2, 16)
    B, n_valid = mc.shape("n_valid")[:2]
    assert n_valid < B
    B, n_valid, K = mc.shape("k6")[:3]
    assert K > 4 and n_valid // K >= 2                                            # a wave of the update kernel owns two folds
    from tests import row_instance_cases as rc
    assert {rc.maxit(mc.dim(c)) for c in mc.CASES} == {1, 4, 16, 32} and max(mc.dim(c) for c in mc.CASES) > 1024
    assert all(np.isfinite(mc.reference(c).trace[:, :, :5]).all() for c in mc.NEW_CASES)      # their statistics are all usable
    assert mc.reference("n_valid").trace.shape == (3, 4, 6)
