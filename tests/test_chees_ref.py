"""CPU tests of tests/chees_ref.py, the float64 restatement ``mfm_chees_warmup`` is held to: the jitter sequence, the leapfrog count at
its edges, the sign of the ChEES gradient on a Gaussian (the paper's), the trajectory length's clamp and skipped updates, the
all-divergent branch, and the dual-averaging lines against include/mfm.h's recursion typed again here."""
import numpy as np

from oracle import prng
from tests import chees_ref as cr


def test_radical_inverse_first_16_values():
    want = [1 / 2, 1 / 4, 3 / 4, 1 / 8, 5 / 8, 3 / 8, 7 / 8, 1 / 16, 9 / 16, 5 / 16, 13 / 16, 3 / 16, 11 / 16, 7 / 16, 15 / 16, 1 / 32]
    assert [cr.radical_inverse(t) for t in range(1, 17)] == want
    assert all(0.0 < cr.radical_inverse(t) < 1.0 for t in range(1, 5000))


def test_leapfrog_count_at_its_edges():
    assert cr.num_leapfrog(0.75, 0.25, 1000) == 3                # tau / eps an exact integer: no extra step
    assert cr.num_leapfrog(0.75 + 2.0 ** -40, 0.25, 1000) == 4
    assert cr.num_leapfrog(0.01, 0.25, 1000) == 1                # below one step
    assert cr.num_leapfrog(0.25, 0.25, 1000) == 1
    assert cr.num_leapfrog(300.0, 0.25, 1000) == 1000            # above max_leapfrog
    assert cr.num_leapfrog(250.0, 0.25, 1000) == 1000
    assert cr.num_leapfrog(np.nan, 0.25, 1000) == 1
    rs = cr.Recursion(0.25, 1.5, max_leapfrog=1000)              # iteration 1: h = 1/2, tau = 0.75
    assert rs.L == 3 and rs.tau == 0.75


def _gaussian_vg(x):
    return -0.5 * (x * x).sum(1), -x


def _mean_g(T, n=4096, d=8, eps=0.05, seed=3):
    """The mean over n chains at stationarity of g_k / tau for trajectories of length T on a unit Gaussian."""
    x = prng.normal_rows(prng.split(prng.PRNGKey(seed), n), d)
    lp, g = _gaussian_vg(x)
    L = int(round(T / eps))
    _, rec = cr.hmc_step(prng.split(prng.PRNGKey(seed + 1), n), cr.State(x, lp, g), _gaussian_vg, eps, L)
    dx0, dx1 = rec.x - rec.x.mean(0), rec.prop - rec.prop.mean(0)
    gk = ((dx1 * dx1).sum(1) - (dx0 * dx0).sum(1)) * (dx1 * rec.vel).sum(1)
    ghat = cr.statistic(rec.x, rec.prop, rec.vel, rec.alpha, rec.div, T)[0]
    return gk.mean(), ghat


def test_gradient_sign_on_a_unit_gaussian():
    """On a unit Gaussian x' = x cos T + p sin T and v' = -x sin T + p cos T, so with A = |p|^2 - |x|^2 (variance 4 d) and C = <x, p>
    (variance d, uncorrelated with A): |x'|^2 - |x|^2 = A sin^2 T + C sin 2T, <x', v'> = A sin 2T / 2 + C cos 2T, and
    E[g / tau] = d sin 2T (2 sin^2 T + cos 2T) = d sin 2T.  Positive at T = 0.3 (a longer trajectory is better), negative at T = 3
    (past the optimum pi / 2): the paper's signs.  4096 chains, d = 8, fixed seed: d sin 2T = 4.5 and -2.2 against a standard error
    of about 0.2."""
    short, ghat_short = _mean_g(0.3)
    long_, ghat_long = _mean_g(3.0)
    print(f"E[g / tau] at T = 0.3: {short:.3f}; at T = 3: {long_:.3f}; ghat {ghat_short:.3f}, {ghat_long:.3f}")
    assert short > 0 and ghat_short > 0
    assert long_ < 0 and ghat_long < 0


def test_trajectory_length_clamp():
    rs = cr.Recursion(0.1, 0.1, learning_rate=0.025, max_leapfrog=4)
    rs.advance(0.651, -1.0)                                      # T would fall below eps: held at the NEW eps
    assert rs.T == rs.eps and rs.logT == rs.da.x
    rs = cr.Recursion(0.1, 0.4, learning_rate=5.0, max_leapfrog=4)
    rs.advance(0.651, 1.0)                                       # T would exceed max_leapfrog eps
    np.testing.assert_allclose(rs.T, 4 * rs.eps, rtol=1e-15)
    assert rs.L <= 4


def test_non_finite_gradient_leaves_log_T_alone():
    for bad in (np.nan, np.inf, -np.inf):
        rs = cr.Recursion(0.1, 0.3)
        rs.advance(0.651, 0.5)
        before = (rs.logT, rs.m, rs.v, rs.b1t, rs.b2t)
        t = rs.t
        rs.advance(0.651, bad)
        assert (rs.logT, rs.m, rs.v, rs.b1t, rs.b2t) == before and rs.t == t + 1
        assert np.isfinite(rs.T) and np.isfinite(rs.eps)


def test_all_divergent_branch():
    n, d = 8, 3
    r = np.random.RandomState(0)
    x, prop, vel = r.randn(n, d), r.randn(n, d), r.randn(n, d)
    alpha = np.zeros(n)
    ghat, hm, n_div, mean_alpha = cr.statistic(x, prop, vel, alpha, np.ones(n, bool), 0.5)
    assert (ghat, hm, n_div, mean_alpha) == (0.0, 0.0, n, 0.0)
    # an alpha of 0 on a chain that is not divergent: IEEE arithmetic as it falls
    alpha = np.array([0.0] + [0.5] * (n - 1))
    ghat, hm, n_div, _ = cr.statistic(x, prop, vel, alpha, np.zeros(n, bool), 0.5)
    assert hm == 0.0 and n_div == 0 and np.isfinite(ghat)
    # padding rows and divergent chains are left out of the sums, divergent chains stay in the means
    div = np.zeros(n, bool); div[2] = True
    alpha = r.rand(n)
    ghat, hm, n_div, _ = cr.statistic(x, prop, vel, alpha, div, 0.5, n_valid=6)
    ok = [0, 1, 3, 4, 5]
    dx0, dx1 = x[:6] - x[:6].mean(0), prop[:6] - prop[:6].mean(0)
    g = 0.5 * ((dx1 ** 2).sum(1) - (dx0 ** 2).sum(1)) * (dx1 * vel[:6]).sum(1)
    np.testing.assert_allclose(ghat, (alpha[ok] * g[ok]).sum() / (alpha[ok] + 1e-20).sum(), rtol=1e-14)
    np.testing.assert_allclose(hm, 5 / (1 / alpha[ok]).sum(), rtol=1e-14)
    assert n_div == 1


def test_dual_averaging_lines_follow_the_header():
    """include/mfm.h, mfm_hmc_warmup, steps 2 - 5, typed again from the header's text."""
    step0, target = 0.07, 0.651
    ps = [0.0, 0.3, 1.0, 0.9, 0.651, 0.02, 0.8, 0.7]
    t0, gamma, mu = 10.0, 0.05, np.log(10.0 * step0)
    x, hbar, xbar = np.log(step0), 0.0, 0.0
    da = cr.DualAveraging(step0)
    for m, p in enumerate(ps, start=1):
        hbar = (1.0 - 1.0 / (m + t0)) * hbar + (target - p) / (m + t0)
        x = mu - (np.sqrt(m) / gamma) * hbar
        x = min(max(x, np.log(step0) - 23.0), np.log(step0) + 23.0)
        eta = 1.0 / (np.sqrt(m) * np.sqrt(np.sqrt(m)))
        xbar = eta * x + (1.0 - eta) * xbar
        da.update(m, p, target)
        assert (da.x, da.hbar, da.xbar) == (x, hbar, xbar)
    # and the recursion object hands it hm, and takes eps_{t+1} = exp(x_t)
    rs = cr.Recursion(step0, 0.2, target=target)
    for p in ps:
        rs.advance(p, 0.1)
    assert rs.eps == float(np.exp(x)) and rs.results[0] == float(np.exp(xbar))


def test_moving_average_and_results():
    rs = cr.Recursion(0.1, 0.3, decay=0.5)
    ma = np.log(0.3)
    for g in (0.4, -0.2, 0.7):
        rs.advance(0.6, g)
        ma = 0.5 * ma + 0.5 * rs.logT
    assert rs.ma == ma
    assert rs.results == (float(np.exp(rs.da.xbar)), float(np.exp(ma)), rs.eps, rs.T)
