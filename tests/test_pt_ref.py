"""CPU tests of the parallel-tempering restatement (tests/pt_ref.py) and of the cases the GPU test runs (tests/pt_cases.py): the recorded
tolerances against their recomputation, the margins the GPU test relies on, the exchange move's own properties, and the sampling
property on the 4-mode mixture."""
import numpy as np
import pytest

from oracle import prng, targets
from tests import pt_cases as pc, pt_ref as pr


@pytest.mark.parametrize("case", list(pc.CASES))
def test_recorded_tolerance_is_the_recomputation(case):
    got = pc.measure(case)
    print(case, got)
    assert pc.decisions_agree(case)                           # the two variants made the same decisions: the differences are roundings
    for q, a, b in zip(pc.QUANTITIES, pc.TOLERANCE[case], got):
        assert float("%.2g" % b) == a, (q, a, b)
        assert a > 0                                          # every compared quantity moved


@pytest.mark.parametrize("case", list(pc.CASES))
def test_no_decision_is_near_its_threshold(case):
    c = pc.CASES[case]
    loc, sw = pc.margins(case)
    print(case, loc, sw)
    assert loc >= 1e-6 and sw >= 1e-6
    r = pc.reference(case)
    acc = np.stack([rec.accepted for rec in r["local"]])
    assert 0 < acc.sum() < acc.size                           # both local decisions occur
    swaps = np.concatenate([rec.accepted for rec in r["swaps"]])
    assert swaps.any()
    if case not in ("d1025_d0", "d2048_pbc"):                 # (two pairs, one sweep)
        assert not swaps.all()
    # the sweep of round t holds the pairs k % 2 == t % 2 of every ladder and no others
    for t, rec in enumerate(r["swaps"]):
        want = [rr * c["K"] + k for k in range(t % 2, c["K"] - 1, 2) for rr in range(c["R"])]
        assert rec.lower.tolist() == want
    if c["K"] == 2:
        assert all(rec.lower.size == 0 for rec in r["swaps"][1::2])      # odd rounds: no pair at all


def test_layout_and_case_table():
    assert {"gmm4", "phi4_d65", "phi4_d256_pbc", "phi4_d320", "d1025_d0", "d2048_pbc", "padded"} == set(pc.CASES)
    for name, c in pc.CASES.items():
        assert 2 <= c["n_local"] <= 3 and 2 <= c["n_rounds"] <= 6 and c["L"] <= 3
        assert pc.start_state(name).shape == (c["K"] * c["R"] + c["pad"], c["d"]) and pc.n_chains(name) % 16 == 0
    assert pc.CASES["phi4_d65"]["K"] % 2 == 1 and pc.CASES["phi4_d65"]["K"] * pc.CASES["phi4_d65"]["R"] == 15
    assert pc.CASES["padded"]["pad"] > 0


def test_lse_mixture_is_the_oracle_mixture_near_the_modes_and_finite_far_away():
    modes = 8.0 * np.array([[1, 1], [1, -1], [-1, 1], [-1, -1.0]])
    a = pr.LseMixture(modes, np.ones((4, 2)), np.ones(4) / 4)
    b = targets.GaussianMixture(modes, np.ones((4, 2)), np.ones(4) / 4)
    x = modes[np.arange(12) % 4] + prng.normal_rows(prng.split(prng.PRNGKey(1), 12), 2)
    np.testing.assert_allclose(a.loglik(x), b.loglik(x), rtol=1e-12)
    np.testing.assert_allclose(a.grad_loglik(x), b.grad_loglik(x), rtol=1e-10, atol=1e-12)
    far = np.array([[60.0, -70.0], [0.0, 300.0]])
    assert np.isfinite(a.loglik(far)).all() and np.isfinite(a.grad_loglik(far)).all()
    assert not np.isfinite(b.loglik(far)).all()               # the reason this class exists


def test_exchange_is_metropolis_on_the_joint():
    """delta is the log ratio of the joint density after and before the swap; an accepted pair holds the state init would give; the
    pairs of the other parity and the replica bookkeeping."""
    d_ = pc.dist("phi4_d65")
    betas = np.array([1.0, 0.9, 0.8])
    x0 = pc.start_state("phi4_d65")[:15].astype(np.float64)
    st = pr.init(d_, betas, x0)
    key = prng.PRNGKey(3)
    for parity in (0, 1):
        new, rep, rec = pr.exchange(key, st, d_, betas, 5, parity, np.arange(15, dtype=np.int32))
        assert (rec.lower % 3 == parity).all() and rec.lower.size == 5
        joint0 = st.logdensity.sum()
        for i, acc, delta in zip(rec.lower, rec.accepted, rec.delta):
            perm = np.arange(15); perm[[i, i + 1]] = [i + 1, i]
            np.testing.assert_allclose(pr.init(d_, betas, x0[perm]).logdensity.sum() - joint0, delta, atol=1e-9)
            if acc:
                assert rep[i] == i + 1 and rep[i + 1] == i
                np.testing.assert_array_equal(new.position[i], x0[i + 1])
        again = pr.init(d_, betas, new.position)
        np.testing.assert_allclose(new.logdensity, again.logdensity, rtol=1e-13)
        np.testing.assert_allclose(new.logdensity_grad, again.logdensity_grad, rtol=1e-13, atol=1e-13)
        untouched = np.setdiff1d(np.arange(15), np.concatenate([rec.lower[rec.accepted], rec.lower[rec.accepted] + 1]))
        np.testing.assert_array_equal(new.position[untouched], x0[untouched])
        np.testing.assert_array_equal(np.sort(rep), np.arange(15))


def test_run_is_the_loop_of_its_two_pieces():
    c = pc.CASES["gmm4"]
    r = pc.reference("gmm4")
    full = pr.pt_run(pc.key("gmm4"), pc.start_state("gmm4"), pc.dist("gmm4"), pc.betas("gmm4"), pc.step_sizes("gmm4"), c["R"], c["kernel"], c["L"],
                     True, c["n_local"], c["n_rounds"], thin=2)
    np.testing.assert_array_equal(full["state"].position, r["state"].position)
    np.testing.assert_array_equal(full["swap_accepted"], r["swap_accepted"])
    np.testing.assert_array_equal(full["replica"], r["replica"])
    np.testing.assert_array_equal(full["traj_pos"], r["traj_pos"][1::2])
    none = pr.pt_run(pc.key("gmm4"), pc.start_state("gmm4"), pc.dist("gmm4"), pc.betas("gmm4"), pc.step_sizes("gmm4"), c["R"], c["kernel"], c["L"],
                     True, c["n_local"], c["n_rounds"], exchange_moves=False)
    assert none["swap_accepted"].sum() == 0 and (none["replica"] == np.arange(16)).all()
    np.testing.assert_array_equal(none["local"][0].u, r["local"][0].u)          # the first round's local moves do not know of the sweep


def test_sampling_slot_0_visits_every_mode_only_with_exchange():
    """gmm4 (modes 8 (+-1, +-1), unit covariance), K = 8, R = 32, geometric betas from 1 to 0.01, HMC with L = 4 and eps_k = 0.25 /
    sqrt(beta_k), n_local = 4, 200 rounds, every chain from mode 0 + N(0, I): over the last 100 rounds slot 0's share of each mode lies in
    [0.10, 0.40]; without exchange the share of mode 0 exceeds 0.99.  One key here; the module's __main__ runs the five whose shares
    tests/pt_cases.py records."""
    assert pc.SAMPLING == dict(K=8, R=32, beta_min=0.01, L=4, s=0.25, n_local=4, n_rounds=200, last=100)
    shares, rates = pc.sampling(pc.SAMPLING_KEY)
    print("shares", shares, "swap rates", rates)
    assert ((shares >= 0.10) & (shares <= 0.40)).all(), shares
    np.testing.assert_allclose(shares, pc.SAMPLING_SHARES[pc.SAMPLING_KEY], atol=5e-4)
    for seed, sh in pc.SAMPLING_SHARES.items():
        assert all(0.10 <= v <= 0.40 for v in sh), (seed, sh)
    alone, _ = pc.sampling(pc.SAMPLING_KEY, exchange=False)
    assert alone[0] > 0.99
