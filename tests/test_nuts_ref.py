"""tests/nuts_ref.py, the float64 restatement of the No-U-turn kernel (mfm_amd/csrc/nuts.hip), checked on the CPU: tree shapes against a
recursive restatement, the single leaf against oracle.hmc.kernel, the prefix property, a Gaussian's moments; and the host surface of the
feature (parser, exports, ctypes signatures)."""
import os
import re

import numpy as np

from oracle import hmc, prng
from oracle.mala import MALAState
from tests import autocorr_oracle as ao, hmc_mass_ref as hm, nuts_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG = np.array([0.5, 1.0, 2.0, 0.7, 1.5])


def gauss_vg(x):
    return -0.5 * (x * x / SIG ** 2).sum(1), -x / SIG ** 2


def gauss_state(seed, B):
    x = (np.random.default_rng(seed).standard_normal((B, SIG.size)) * SIG).astype(np.float32).astype(np.float64)
    lp, g = gauss_vg(x)
    return MALAState(x, lp, g.astype(np.float32).astype(np.float64))


def _recursive_shape(key, state, eps, max_depth, thr=1000.0):
    """(depth, leapfrog count, turning, divergent) of ONE chain's tree by the textbook recursion: a subtree of depth k is two subtrees of
    depth k - 1, turning when (p_first, p_last, p_sum) of its span turn; no proposal is needed for the shape."""
    x0, lp0, g0 = (np.asarray(a, dtype=np.float64) for a in state)
    r32 = lambda a: a.astype(np.float32).astype(np.float64)
    kk = prng.split(key, 2)
    p0 = prng.normal(kk[0], (x0.size,))
    h0 = -lp0 + 0.5 * (p0 * p0).sum()
    count = [0]

    def turn(pa, pb, s):
        return (pa * s).sum() <= 0 or (pb * s).sum() <= 0

    def build(z, e, k):
        """-> (end point, p_first, p_last, p_sum, stopped, turning, divergent)"""
        if k == 0:
            x, p, g = z
            p = p + 0.5 * e * g
            x = r32(x + e * p)
            lp, g = gauss_vg(x[None])
            g = r32(g[0])
            p = p + 0.5 * e * g
            count[0] += 1
            delta = h0 - (-lp[0] + 0.5 * (p * p).sum())
            div = bool(np.isnan(delta) or -delta > thr)
            return (x, p, g), p, p, p.copy(), div, False, div
        za, pf, _, sa, stop, t, dv = build(z, e, k - 1)
        if stop:
            return za, pf, None, sa, True, t, dv
        zb, _, pl, sb, stop, t, dv = build(za, e, k - 1)
        if stop:
            return zb, pf, pl, sa + sb, True, t, dv
        s = sa + sb
        t = turn(pf, pl, s)
        return zb, pf, pl, s, t, t, False

    left = right = (x0, p0, g0)
    psum = p0.copy()
    k_tree = kk[1]
    for j in range(max_depth):
        kd = prng.split(prng.split_at(k_tree, nr.MAX_DOUBLINGS, np.array(j)), 3)
        fwd = prng.uniform(kd[0]) < 0.5
        z, _, _, s, stop, t, dv = build(right if fwd else left, eps if fwd else -eps, j)
        if stop:
            return j, count[0], t, dv
        if fwd:
            right = z
        else:
            left = z
        psum = psum + s
        if turn(left[1], right[1], psum):
            return j + 1, count[0], True, False
    return max_depth, count[0], False, False


def test_tree_shapes_equal_the_recursive_restatement():
    """(a) 4 chains x 60 consecutive transitions (240 trees) of the anisotropic Gaussian: depth, leapfrog count and both flags."""
    B, eps, D = 4, 0.35, 7
    st = gauss_state(1, B)
    depths = []
    for it in range(60):
        keys = prng.split(prng.PRNGKey(100 + it), B)
        st_n, info = nr.kernel(keys, st, gauss_vg, eps, D)
        for b in range(B):
            one = MALAState(st.position[b], st.logdensity[b], st.logdensity_grad[b])
            assert _recursive_shape(keys[b], one, eps, D) == (info.depth[b], info.num_leapfrog[b], bool(info.is_turning[b]), bool(info.is_divergent[b])), (it, b)
        depths += info.depth.tolist()
        st = st_n
    assert min(depths) <= 2 and max(depths) >= 4                    # trees of several depths


def test_depth_one_is_the_oracle_hmc_leapfrog():
    """(b) With max_tree_depth = 1 the tree is the start and ONE leaf: oracle.hmc.kernel's one-leapfrog proposal and energy difference on
    the same key (with -eps when the direction is backward); with a mass, hmc_mass_ref.kernel's."""
    B, eps = 64, 0.4
    st = gauss_state(2, B)
    keys = prng.split(prng.PRNGKey(7), B)
    for minv in (None, hm.log_spaced_mass(SIG.size)):
        st_n, info = nr.kernel(keys, st, gauss_vg, eps, 1, inverse_mass=minv, f32=False)
        fwd = info.directions[:, 0] > 0
        assert fwd.any() and (~fwd).any()
        for sign in (1.0, -1.0):
            o = hmc.kernel(keys, st, gauss_vg, sign * eps, 1)[1] if minv is None else hm.kernel(keys, st, gauss_vg, sign * eps, 1, minv)[1]
            m = fwd if sign > 0 else ~fwd
            np.testing.assert_allclose(info.acceptance_rate[m], o.acceptance_rate[m], rtol=1e-13)
            moved = m & (st_n.position != st.position).any(1)
            assert moved.any()
            np.testing.assert_allclose(st_n.position[moved], o.proposed_position[moved], rtol=1e-14)
            h0 = -st.logdensity + _kinetic(keys, minv)             # the leaf's energy is H0 - energy_delta
            np.testing.assert_allclose(info.energy[moved], (h0 - o.energy_delta)[moved], rtol=1e-12)
        assert (info.num_leapfrog == 1).all() and (info.depth <= 1).all()


def _kinetic(keys, minv):
    p = prng.normal_rows(prng.split_rows(keys, 2)[:, 0], SIG.size)
    return 0.5 * (p * p).sum(1) if minv is None else 0.5 * (minv * (p / np.sqrt(minv)) ** 2).sum(1)


def test_a_tree_under_a_smaller_limit_is_a_prefix():
    """(c) A transition that ends at depth < D under limit D is the same transition under limit D + 1."""
    B, eps = 64, 0.35
    st = gauss_state(3, B)
    keys = prng.split(prng.PRNGKey(11), B)
    seen = set()
    for D in (3, 4, 5):
        sa, ia = nr.kernel(keys, st, gauss_vg, eps, D)
        sb, ib = nr.kernel(keys, st, gauss_vg, eps, D + 1)
        m = ia.depth < D
        seen |= {bool(v) for v in m}
        for a, b in zip(sa, sb):
            np.testing.assert_array_equal(a[m], b[m])
        for f in ("depth", "num_leapfrog", "is_turning", "is_divergent", "acceptance_rate", "energy"):
            np.testing.assert_array_equal(getattr(ia, f)[m], getattr(ib, f)[m])
        assert (ib.num_leapfrog[~m] >= ia.num_leapfrog[~m]).all()
    assert seen == {True, False}                                   # trees that ended early, and trees that the limit cut


def test_gaussian_moments_are_recovered():
    """(d) 16 chains x 400 transitions from exact draws: every mean and variance within 6 standard errors, the standard error from the
    run's own effective sample size (Geyer, tests/autocorr_oracle.py) summed over the chains."""
    B, n, eps = 16, 400, 0.4
    st = gauss_state(4, B)
    traj = np.empty((n, B, SIG.size))
    leap = 0
    for it in range(n):
        st, info = nr.kernel(prng.split(prng.PRNGKey(1000 + it), B), st, gauss_vg, eps, 8)
        traj[it] = st.position
        leap += info.num_leapfrog.sum()
        assert not info.is_divergent.any()
    assert 3 <= leap / (n * B) <= 64
    flat = traj.reshape(n, -1)
    for series, truth in ((flat, np.zeros(SIG.size)), (flat ** 2, SIG ** 2)):
        ess = ao.ess(series, n // 4)[0].reshape(B, SIG.size)
        ess = np.minimum(ess, 4.0 * n).sum(0)                       # (an antithetic series: capped, so the error bar is not understated)
        est = series.reshape(n * B, SIG.size).mean(0)
        se = series.reshape(n * B, SIG.size).std(0) / np.sqrt(ess)
        print("estimate", est, "truth", truth, "standard error", se)
        assert (np.abs(est - truth) < 6 * se).all(), (est, truth, se)


def test_host_surface():
    """(e) Parser flags and defaults, exported names, ctypes signatures and header declarations."""
    from mfm_amd import _lib
    from mfm_amd.bblackjax import mcmc
    from mfm_amd.bblackjax.mcmc import hmc as H, nuts as N
    from mfm_amd.multi_modal import build_parser
    a = build_parser().parse_args([])
    assert (a.mcmc_kernel, a.max_tree_depth) == ("mala", 10)
    a = build_parser().parse_args(["--mcmc_kernel", "nuts", "--max_tree_depth", "6"])
    assert (a.mcmc_kernel, a.max_tree_depth) == ("nuts", 6)
    assert mcmc.nuts is N
    assert {"NUTSState", "NUTSInfo", "NUTSRunInfo", "init", "build_kernel", "nuts"} <= set(N.__all__)
    assert N.NUTSState is H.HMCState
    assert N.NUTSInfo._fields == ("num_trajectory_expansions", "num_integration_steps", "is_turning", "is_divergent", "acceptance_rate", "energy")
    assert callable(N.build_kernel().run)
    hdr = open(os.path.join(ROOT, "include", "mfm.h")).read()
    for name, nargs in (("mfm_nuts_step", 16), ("mfm_nuts_step_keys", 15), ("mfm_nuts_run", 26), ("mfm_nuts_launch_plan", 5)):
        assert name in _lib.EXPORTS and len(_lib._SIGS[name][1]) == nargs
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == nargs, name
    for m in ("nuts_step", "nuts_step_keys", "nuts_run"):
        assert callable(getattr(_lib.Context, m))
    import inspect
    sig = inspect.signature(N.nuts.__new__)
    assert sig.parameters["max_num_doublings"].default == 10 and sig.parameters["divergence_threshold"].default == 1000
    from mfm_amd import exe_flow_matching as E
    from oracle import loop
    assert E.check_adapt_args(loop.default_args(mcmc_kernel="nuts", adapt_steps=5)) == 5
