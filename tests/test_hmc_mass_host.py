"""CPU tests of the diagonal mass matrix's host side: Stan's window schedule, the pooled within-chain variance and its regularisation
(mfm_amd/bblackjax/adaptation/window_adaptation.py), the argument check of ``hmc(..., inverse_mass_matrix=...)``, and the float64
restatement of the mass step (tests/hmc_mass_ref.py) pinned to ``oracle.hmc.kernel``."""
import numpy as np
import pytest

from oracle import hmc as ohmc, mala as omala, prng, targets
from tests import hmc_mass_ref as mr


def _tiles(schedule, n):
    assert schedule[0][1] == 0 and schedule[-1][2] == n
    for (_, _, e), (_, s, _) in zip(schedule, schedule[1:]):
        assert e == s                                                          # no gap, no overlap
    assert all(e > s for _, s, e in schedule)


def test_window_schedule_examples_and_rules():
    from mfm_amd.bblackjax.adaptation.window_adaptation import window_schedule
    assert window_schedule(10) == [("fast", 0, 10)]
    assert window_schedule(19) == [("fast", 0, 19)]
    assert window_schedule(20) == [("fast", 0, 3), ("slow", 3, 18), ("fast", 18, 20)]                  # 15 % / 10 %, one slow window
    assert window_schedule(100) == [("fast", 0, 15), ("slow", 15, 90), ("fast", 90, 100)]
    assert window_schedule(150) == [("fast", 0, 75), ("slow", 75, 100), ("fast", 100, 150)]            # 150 is not below 150: the buffers
    assert window_schedule(300) == [("fast", 0, 75), ("slow", 75, 100), ("slow", 100, 250), ("fast", 250, 300)]
    assert window_schedule(1000) == [("fast", 0, 75), ("slow", 75, 100), ("slow", 100, 150), ("slow", 150, 250), ("slow", 250, 450),
                                     ("slow", 450, 950), ("fast", 950, 1000)]
    for n in (10, 19, 20, 100, 150, 300, 1000, 149, 151, 457):
        sched = window_schedule(n)
        _tiles(sched, n)
        slow = [(s, e) for k, s, e in sched if k == "slow"]
        if n < 20:
            assert not slow
            continue
        assert sched[0][0] == "fast" and sched[-1][0] == "fast" and all(k == "slow" for k, _, _ in sched[1:-1])
        final_start = sched[-1][1]
        if n < 150:
            assert (sched[0][2], n - final_start, len(slow)) == (int(0.15 * n), int(0.1 * n), 1)
        else:
            assert (sched[0][2], n - final_start, slow[0][0]) == (75, 50, 75)
        # lengths double from 25; the last runs up to the final buffer, which its successor would have reached
        for i, (s, e) in enumerate(slow[:-1]):
            assert e - s == 25 * 2 ** i
            assert e + 2 * (e - s) < final_start
        if n >= 150:
            s, e = slow[-1]
            nominal = 25 * 2 ** (len(slow) - 1)
            assert e == final_start and e - s >= nominal and s + nominal + 2 * nominal >= final_start
    with pytest.raises(ValueError):
        window_schedule(0)


def test_pooled_variance_leaves_padding_rows_out():
    import torch
    from mfm_amd.bblackjax.adaptation.window_adaptation import pooled_variance
    rng = np.random.RandomState(0)
    n, n_valid, n_local, d = 37, 21, 32, 5
    x = rng.randn(n, n_local, d) * np.array([0.2, 1.0, 5.0, 0.5, 2.0]) + rng.randn(n_local, d) * 10.0      # chains far apart
    s, q = x.sum(0), (x * x).sum(0)
    s[n_valid:], q[n_valid:] = np.nan, -1e300                                  # padding rows hold garbage
    want = x[:, :n_valid].var(axis=0, ddof=1).mean(0)
    got = pooled_variance(torch.as_tensor(s), torch.as_tensor(q), n, n_valid)
    assert got.dtype == torch.float64 and got.shape == (d,)
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-9)
    np.testing.assert_allclose(pooled_variance(s[:n_valid], q[:n_valid], n).numpy(), want, rtol=1e-9)      # arrays, no padding
    # the WITHIN-chain variance: far below the variance across the chains' means
    assert (got.numpy() < 0.5 * x[:, :n_valid].reshape(-1, d).var(0)).all()
    with pytest.raises(ValueError):
        pooled_variance(s, q, 1)


def test_regularisation_formula():
    from mfm_amd.bblackjax.adaptation.window_adaptation import regularized_inverse_mass
    w = np.array([0.04, 1.0, 25.0])
    for n in (25, 150, 500):
        np.testing.assert_allclose(regularized_inverse_mass(w, n), n / (n + 5) * w + 1e-3 * 5 / (n + 5), rtol=1e-15)
    assert regularized_inverse_mass(np.zeros(2), 25)[0] == pytest.approx(1e-3 / 6)


def test_bad_inverse_mass_matrix_raises_value_error():
    from mfm_amd.bblackjax.mcmc import hmc as H
    from mfm_amd.distributions import PhiFour
    dist = PhiFour(8)
    good = np.linspace(0.5, 2.0, 8)
    H.hmc(dist.logprob, 1e-2, 3, inverse_mass_matrix=good)                     # (no device work at construction)
    H.hmc(dist.logprob, 1e-2, 3)
    for bad in (np.ones(7), np.ones(9), np.ones((8, 8)), np.r_[good[:7], 0.0], np.r_[good[:7], -1.0], np.r_[good[:7], np.nan],
                np.r_[good[:7], np.inf]):
        with pytest.raises(ValueError, match="inverse_mass_matrix"):
            H.hmc(dist.logprob, 1e-2, 3, inverse_mass_matrix=bad)
        with pytest.raises(ValueError, match="inverse_mass_matrix"):           # the kernel checks before it looks for a device
            H.build_kernel()(prng.PRNGKey(0), None, dist.logprob, 1e-2, 3, inverse_mass_matrix=bad)
    assert H.check_inverse_mass(None) is None and H.check_inverse_mass(good, 8).dtype == np.float64


def _phi4_state(d=12, B=6):
    dist = targets.PhiFour(d)
    vg = targets.Tempered(dist, 0.8).value_and_grad
    x = prng.normal_rows(prng.split(prng.PRNGKey(2), B), d) * 0.4
    return vg, omala.init(x, vg)


def test_restated_step_with_unit_mass_is_the_oracle_step():
    vg, st = _phi4_state()
    keys = prng.split(prng.PRNGKey(9), st.position.shape[0])
    for eps in (0.05, 0.12):
        a, ia, ua = ohmc.kernel(keys, st, vg, eps, 5)
        b, ib, ub = mr.kernel(keys, st, vg, eps, 5, np.ones(st.position.shape[1]))
        for u, v in zip(tuple(a) + tuple(ia) + (ua,), tuple(b) + tuple(ib) + (ub,)):
            np.testing.assert_array_equal(u, v)


def test_restated_step_is_the_oracle_step_on_the_rescaled_target():
    """y = x / sqrt(minv): the log-density unchanged, the gradient multiplied by sqrt(minv); unit-mass HMC in y is mass HMC in x."""
    vg, st = _phi4_state()
    B, d = st.position.shape
    minv = mr.log_spaced_mass(d)
    r = np.sqrt(minv)

    def vg_y(y):
        lp, g = vg(y * r)
        return lp, g * r
    keys = prng.split(prng.PRNGKey(9), B)
    seen = set()
    for eps in (0.05, 0.12):               # (the second: 5 of 6 accepted)
        a, ia, _ = mr.kernel(keys, st, vg, eps, 5, minv)
        st_y = omala.MALAState(st.position / r, st.logdensity, st.logdensity_grad * r)
        b, ib, _ = ohmc.kernel(keys, st_y, vg_y, eps, 5)
        np.testing.assert_array_equal(ia.is_accepted, ib.is_accepted)
        np.testing.assert_allclose(ia.energy_delta, ib.energy_delta, rtol=0, atol=1e-12 * max(1.0, np.abs(st.logdensity).max()))
        np.testing.assert_allclose(ia.acceptance_rate, ib.acceptance_rate, rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(ia.proposed_position, ib.proposed_position * r, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(a.position, b.position * r, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(a.logdensity, b.logdensity, rtol=1e-12)
        np.testing.assert_allclose(a.logdensity_grad, b.logdensity_grad / r, rtol=1e-12, atol=1e-12)
        seen |= set(ia.is_accepted.tolist())
    assert seen == {True, False}
    assert np.abs(minv - 1).max() > 1 and minv.min() == pytest.approx(0.25) and minv.max() == pytest.approx(4.0)


def test_restated_window_adaptation_finds_the_scales_of_an_anisotropic_gaussian():
    """A smoke test of the restated driver on a small problem (the device comparison is tests/test_gpu_hmc_mass.py): the adapted inverse
    mass matrix orders the coordinates as the target's variances do and every entry is positive and finite."""
    var = np.array([0.04, 1.0, 25.0, 0.25])
    dist = targets.GaussianMixture(np.zeros((1, 4)), var[None], np.ones(1))
    vg = targets.Tempered(dist, 1.0).value_and_grad
    x0 = prng.normal_rows(prng.split(prng.PRNGKey(1), 64), 4) * np.sqrt(var)
    _, step, minv, steps = mr.window_adaptation(prng.PRNGKey(3), omala.init(x0, vg), vg, 8, 0.05, 150)
    assert len(steps) == 3 and np.isfinite(step) and step > 0
    assert np.isfinite(minv).all() and (minv > 0).all()
    assert list(np.argsort(minv)) == list(np.argsort(var))
