"""The float64 restatement of the elliptical slice transition (tests/eslice_ref.py) against what the sampler must satisfy, on the CPU:
it preserves the prior at beta = 0, it samples the posterior that the oracle's MALA samples, and the shared cases (tests/eslice_cases.py)
leave few chains with a borderline decision."""
import functools

import numpy as np
import pytest

from oracle import mala, prng, targets
from tests import chain_diag_oracle as cdo
from tests import eslice_cases as ec
from tests import eslice_ref as er


def test_beta_zero_is_a_prior_preserving_rotation():
    """beta = 0: log y = log u < 0 = beta ll(x'), so the first proposal is always accepted, and x' - mu = (x - mu) cos + nu sin of two
    independent N(0, K) vectors is N(0, K) again: after many transitions from prior draws the sample mean and covariance are mu and K
    within 5 standard errors (Gaussian: var of a covariance entry = (K_ii K_jj + K_ij^2) / B)."""
    dist = ec.dist_of(4)
    B, d, n_steps = 4096, 16, 8
    xi = prng.normal_rows(prng.split(prng.PRNGKey(11), B), d)
    x = (dist.mu + xi @ dist.chol.T).astype(np.float32).astype(np.float64)
    x, ll, infos, _, _ = er.run(0, prng.PRNGKey(12), None, 0.0, n_steps, x, er.loglik(dist, x), dist)
    for info in infos:
        assert (info.subiter == 1).all() and not info.capped.any()
    np.testing.assert_array_equal(ll, er.loglik(dist, x))
    K = dist.gram
    se_mean = np.sqrt(np.diag(K) / B)
    assert (np.abs(x.mean(0) - dist.mu) <= 5 * se_mean).all(), np.abs(x.mean(0) - dist.mu) / se_mean
    C = np.cov(x.T, bias=True)
    se_cov = np.sqrt((np.outer(np.diag(K), np.diag(K)) + K * K) / B)
    assert (np.abs(C - K) <= 5 * se_cov).all(), (np.abs(C - K) / se_cov).max()


MALA_STEP, MALA_STEPS, ES_STEPS, BURN, POST_B = 0.05, 900, 1200, 200, 256


def _posterior_start(dist, seed):
    """Rows scattered about the likelihood's mode log((c + 1/2) / a): both samplers then spend their burn-in on the prior's pull alone."""
    xi = prng.normal_rows(prng.split(prng.PRNGKey(seed), POST_B), dist.dim)
    return (np.log((dist.counts + 0.5) / dist.poisson_a)[None] + 0.5 * xi).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _posterior_runs():
    """(eslice trajectory, MALA trajectory) on the 4 x 4 grid at beta = 1, each ``[n, B, d + 1]`` with ll as the last coordinate."""
    dist = ec.dist_of(4)
    x = _posterior_start(dist, 21)
    _, _, infos, tx, tl = er.run(0, prng.PRNGKey(22), None, 1.0, ES_STEPS, x, er.loglik(dist, x), dist, thin=1)
    assert not any(i.capped.any() for i in infos)
    es = np.concatenate([tx, tl[:, :, None]], axis=2)[BURN:]
    vg = targets.Tempered(dist, 1.0).value_and_grad
    st = mala.init(_posterior_start(dist, 23), vg)
    keys = prng.split(prng.PRNGKey(24), MALA_STEPS)
    rows = []
    for j in range(MALA_STEPS):
        st, info, _ = mala.kernel(prng.split(keys[j], POST_B), st, vg, MALA_STEP, textbook=True)
        rows.append(np.concatenate([st.position, dist.loglik(st.position)[:, None]], axis=1))
    return es, np.stack(rows)[BURN:]


def test_posterior_agrees_with_the_oracles_mala():
    """Posterior means of x and of ll on the 4 x 4 grid: the restatement against a long run of oracle/mala.py (textbook rule, small step),
    within 4 standard errors of the difference; each standard error from the multi-chain ESS of tests/chain_diag_oracle.py."""
    es, ml = _posterior_runs()
    out = []
    for tr in (es, ml):
        dg = cdo.diag(tr, 200)
        assert np.nanmax(dg["rhat"]) < 1.2, dg["rhat"]      # (the chains have met: the ESS below means something)
        out.append((tr.mean(axis=(0, 1)), np.sqrt(dg["varp"] / dg["ess"]), dg["ess"]))
    (m1, s1, e1), (m2, s2, e2) = out
    z = np.abs(m1 - m2) / np.sqrt(s1 * s1 + s2 * s2)
    print("ESS eslice (min, ll):", e1.min(), e1[-1], " ESS MALA (min, ll):", e2.min(), e2[-1], " max |z|:", z.max())
    assert (z <= 4.0).all(), z


@pytest.mark.parametrize("name", [c.name for c in ec.CASES])
def test_cases_have_few_borderline_chains(name):
    """At most 10 % of a case's chains have any decision margin below 1e-3 (the prototype gives about 3.5 % for 20 transitions); no
    chain of a case reaches the cap (the evaluation counts are printed), and the state's log-likelihood is that of the stored row."""
    c = ec.BY_NAME[name]
    assert c.n_steps <= 20
    x, ll, infos, tx, tl = ec.reference_of(name)
    share = (er.min_margin(infos) < ec.MARGIN).mean()
    sub = np.stack([i.subiter for i in infos])
    print(f"{name}: borderline share {share:.3f}, mean evaluations {sub.mean():.2f}, max {sub.max()}")
    assert share <= ec.MAX_SHARE, share
    assert not any(i.capped.any() for i in infos)
    assert sub.max() < er.MAX_SUBITER
    np.testing.assert_array_equal(ll, er.loglik(ec.dist_of(c.n), x))
