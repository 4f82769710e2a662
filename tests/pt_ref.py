"""Parallel tempering restated in float64 numpy: the definition ``mfm_pt_run`` / ``mfm_pt_exchange`` (mfm_amd/csrc/pt.hip, include/mfm.h)
are held to.  A helper of tests/test_pt_ref.py, tests/pt_cases.py and tests/test_gpu_pt.py, not a test.

Layout: ``K`` temperatures x ``R`` ladders, chain ``b = r * K + k`` is slot ``k`` of ladder ``r`` at ``betas[k]`` with step size
``step_sizes[k]``.  A round ``t`` is ``n_local`` local steps of every chain (``oracle.hmc.kernel`` / ``oracle.mala.kernel`` on the rows
``k::K`` at the scalars of slot ``k``: the project's own steps) and one sweep of deterministic even-odd parity (Syed, Bouchard-Cote,
Deligiannidis & Doucet 2019, "Non-reversible parallel tempering"): the pairs ``(k, k + 1)`` with ``k % 2 == t % 2``.

The exchange of slots ``(i, j = i + 1)``: ``c_i = logp_{beta_i}(x_j)``, ``c_j = logp_{beta_j}(x_i)``,
``delta = (c_i + c_j) - (lp_i + lp_j)``, ``p = min(1, exp(delta))`` (NaN rejects), accept iff ``u < p``; on accept the positions swap and
each slot takes the candidate value and gradient at its own beta.  Metropolis on the joint density ``prod_k pi_{beta_k}(x_k)``.

Keys (include/mfm.h): ``(k_move, k_swap) = split(key, 2)``; round ``t``'s local step ``s`` of chain ``b`` uses
``split(split(split(k_move, n_rounds)[t], n_local)[s], n_total)[b]`` (``mfm_hmc_run`` in key_mode 0); round ``t``'s pair with lower slot
``i`` draws ``u`` from ``split(split(k_swap, n_rounds)[t], n_total)[i]``.

``float32_positions=True`` holds the positions as the kernels do: HMC rounds the trajectory's position to float32 after every drift
(tests/chees_ref.py's step), MALA holds the proposal in float32 (``mala_step_f32``)."""
from collections import namedtuple

import numpy as np

from oracle import hmc as ohmc, mala as omala, prng
from tests import chees_ref as cr

State = omala.MALAState


class LseMixture:
    """A diagonal Gaussian mixture with the density by log-sum-exp: ``oracle.targets.GaussianMixture`` takes the product of pdfs and
    then the log, which underflows far from the modes, where hot chains go.  Same interface (``loglik`` is the density, no prior)."""

    kind = "gmm"

    def __init__(self, modes, covs, weights):
        self.modes = np.asarray(modes, dtype=np.float64)
        self.covs = np.asarray(covs, dtype=np.float64)
        self.chol_covs = np.sqrt(self.covs)
        self.weights = np.asarray(weights, dtype=np.float64)
        self.dim = self.modes.shape[1]

    def _terms(self, x):
        z = (x[:, None, :] - self.modes[None]) / self.chol_covs[None]
        a = np.log(self.weights)[None] + (-0.5 * z * z - np.log(np.sqrt(2.0 * np.pi) * self.chol_covs[None])).sum(-1)      # [B, K]
        m = a.max(1, keepdims=True)
        lp = m[:, 0] + np.log(np.exp(a - m).sum(1))
        return lp, np.exp(a - lp[:, None]), -z / self.chol_covs[None]

    def loglik(self, x):
        return self._terms(x)[0]

    logprob = loglik

    def logprior(self, x):
        return np.zeros(x.shape[0])

    def grad_loglik(self, x):
        _, r, a = self._terms(x)
        return (r[:, :, None] * a).sum(1)

    grad_logprob = grad_loglik

    def grad_logprior(self, x):
        return np.zeros_like(x)


def value_and_grad(dist, beta):
    """``x -> (beta loglik + logprior, its gradient)``."""
    def vg(x):
        return beta * dist.loglik(x) + dist.logprior(x), beta * dist.grad_loglik(x) + dist.grad_logprior(x)
    return vg


def init(dist, betas, position):
    """Every slot initialised at its own beta: ``[R * K, d] -> State``."""
    x = np.asarray(position, dtype=np.float64)
    K = len(betas)
    lp, g = np.empty(x.shape[0]), np.empty_like(x)
    for k, b in enumerate(betas):
        lp[k::K], g[k::K] = value_and_grad(dist, b)(x[k::K])
    return State(x, lp, g)


def round_keys(key, n_rounds, t):
    """``(the key of round t's local steps, the key of its sweep)``."""
    k_move, k_swap = prng.split(key, 2)
    return prng.split(k_move, n_rounds)[t], prng.split(k_swap, n_rounds)[t]


LocalRecord = namedtuple("LocalRecord", "u p accepted")            # [n_local, B] each
SwapRecord = namedtuple("SwapRecord", "lower u p accepted delta")  # per pair of the sweep (lower: the lower slot's chain index)


def mala_step_f32(keys, state, value_and_grad, step_size, textbook):
    """``oracle.mala.kernel`` with the proposal HELD in float32, as the kernels hold it (mala.hip): the proposal is rounded once, and the
    rounded position is what is evaluated, what the back term ``|x - x' - eps g'|^2`` is taken from and what an accepted chain keeps; the
    forward term is ``2 eps |noise|^2`` from the draws themselves.  (The back term is divided by ``4 eps``: at a step size of 1e-6 the
    rounding of ``x'`` moves the acceptance probability by 1e-4, far more than the evaluation at the rounded point alone.)"""
    x, logp, g = state
    kk = prng.split_rows(keys, 2)
    th = np.sqrt(2.0 * step_size) * prng.normal_rows(kk[:, 0], x.shape[1])
    xn = (x + step_size * g + th).astype(np.float32).astype(np.float64)
    logpn, gn = value_and_grad(xn)
    new_E = -logp + 0.25 * (1.0 / step_size) * (th * th).sum(1)
    prev_E = omala.transition_energy(xn, logpn, gn, x, step_size)
    delta = prev_E - new_E
    if textbook:
        delta = -delta
    delta = np.where(np.isnan(delta), -np.inf, delta)
    with np.errstate(over="ignore"):
        p = np.minimum(np.exp(delta), 1.0)
    u = prng.uniform_rows(kk[:, 1])
    acc = u < p
    m = acc[:, None]
    return State(np.where(m, xn, x), np.where(acc, logpn, logp), np.where(m, gn, g)), u, p, acc


def local_steps(key, state, dist, betas, step_sizes, kernel, num_steps, textbook, n_local, n_total=None, float32_positions=False):
    """``n_local`` steps of every chain on the round's key: ``(state, LocalRecord)``."""
    x, lp, g = (np.array(a, dtype=np.float64) for a in state)
    B, K = x.shape[0], len(betas)
    n_total = B if n_total is None else n_total
    us, ps, accs = np.empty((n_local, B)), np.empty((n_local, B)), np.empty((n_local, B), dtype=bool)
    step_keys = prng.split(key, n_local)
    for s in range(n_local):
        keys = prng.split(step_keys[s], n_total)[:B]
        for k in range(K):
            vg = value_and_grad(dist, betas[k])
            st = State(x[k::K], lp[k::K], g[k::K])
            if kernel == "hmc":
                if float32_positions:
                    new, rec = cr.hmc_step(keys[k::K], cr.State(*st), vg, step_sizes[k], num_steps, float32_positions=True)
                    u, p, acc = rec.u, rec.alpha, rec.accepted
                else:
                    new, info, u = ohmc.kernel(keys[k::K], st, vg, step_sizes[k], num_steps)
                    p, acc = info.acceptance_rate, info.is_accepted
            elif float32_positions:
                new, u, p, acc = mala_step_f32(keys[k::K], st, vg, step_sizes[k], textbook)
            else:
                new, info, u = omala.kernel(keys[k::K], st, vg, step_sizes[k], textbook=textbook)
                p, acc = info.acceptance_rate, info.is_accepted
            x[k::K], lp[k::K], g[k::K] = new
            us[s, k::K], ps[s, k::K], accs[s, k::K] = u, p, acc
    return State(x, lp, g), LocalRecord(us, ps, accs)


def exchange(key, state, dist, betas, n_ladders, parity, replica=None, n_total=None):
    """One sweep on ``key``: ``(state, replica, SwapRecord)``."""
    x, lp, g = (np.array(a, dtype=np.float64) for a in state)
    K, R = len(betas), int(n_ladders)
    n_total = x.shape[0] if n_total is None else n_total
    replica = None if replica is None else np.array(replica)
    keys = prng.split(key, n_total)
    lower, us, ps, accs, deltas = [], [], [], [], []
    for k in range(parity, K - 1, 2):
        i = np.arange(R) * K + k
        j = i + 1
        ci, gi = value_and_grad(dist, betas[k])(x[j])
        cj, gj = value_and_grad(dist, betas[k + 1])(x[i])
        delta = (ci + cj) - (lp[i] + lp[j])
        delta = np.where(np.isnan(delta), -np.inf, delta)
        with np.errstate(over="ignore"):
            p = np.minimum(np.exp(delta), 1.0)
        u = prng.uniform_rows(keys[i])
        acc = u < p
        ia, ja = i[acc], j[acc]
        xi = x[ia].copy()
        x[ia], x[ja] = x[ja], xi
        lp[ia], lp[ja] = ci[acc], cj[acc]
        g[ia], g[ja] = gi[acc], gj[acc]
        if replica is not None:
            ri = replica[ia].copy()
            replica[ia], replica[ja] = replica[ja], ri
        lower.append(i); us.append(u); ps.append(p); accs.append(acc); deltas.append(delta)
    cat = lambda v, dt: np.concatenate(v) if v else np.zeros(0, dtype=dt)
    return State(x, lp, g), replica, SwapRecord(cat(lower, int), cat(us, float), cat(ps, float), cat(accs, bool), cat(deltas, float))


def pt_run(key, position, dist, betas, step_sizes, n_ladders, kernel="hmc", num_steps=10, textbook=True, n_local=1, n_rounds=1,
           exchange_moves=True, thin=0, float32_positions=False, state=None):
    """``mfm_pt_run``: ``dict(state, replica, n_acc, acc_sum, swap_accepted [R, K - 1], swap_prob, traj_pos, traj_logp, local, swaps)``
    from ``position [R * K, d]`` (initialised per slot) or from ``state``; ``local`` / ``swaps`` hold one record per round."""
    betas, step_sizes = np.asarray(betas, dtype=np.float64), np.asarray(step_sizes, dtype=np.float64)
    K, R = len(betas), int(n_ladders)
    st = init(dist, betas, np.asarray(position)[:K * R]) if state is None else State(*state)
    B = st.position.shape[0]
    assert B == K * R
    replica = np.arange(B, dtype=np.int32)
    n_acc, acc_sum = np.zeros(B, dtype=np.int32), np.zeros(B)
    swap_acc, swap_prob = np.zeros((R, K - 1), dtype=np.int32), np.zeros((R, K - 1))
    traj_pos, traj_logp, local, swaps = [], [], [], []
    for t in range(n_rounds):
        km, ks = round_keys(key, n_rounds, t)
        st, rec = local_steps(km, st, dist, betas, step_sizes, kernel, num_steps, textbook, n_local, float32_positions=float32_positions)
        n_acc += rec.accepted.sum(0).astype(np.int32)
        round_sum = np.zeros(B)
        for s in range(n_local):
            round_sum = round_sum + rec.p[s]
        acc_sum = acc_sum + round_sum
        local.append(rec)
        if exchange_moves:
            st, replica, srec = exchange(ks, st, dist, betas, R, t % 2, replica)
            r_, k_ = srec.lower // K, srec.lower % K
            swap_acc[r_, k_] += srec.accepted
            swap_prob[r_, k_] += srec.p
            swaps.append(srec)
        if thin > 0 and (t + 1) % thin == 0:
            traj_pos.append(st.position[::K].copy()); traj_logp.append(st.logdensity[::K].copy())
    return dict(state=st, replica=replica, n_acc=n_acc, acc_sum=acc_sum, swap_accepted=swap_acc, swap_prob=swap_prob,
                traj_pos=np.array(traj_pos), traj_logp=np.array(traj_logp), local=local, swaps=swaps)
