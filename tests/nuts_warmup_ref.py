"""The NUTS warmup (``mfm_nuts_warmup``, mfm_amd/csrc/nuts_warmup.hip.h) restated in float64 numpy: the dual-averaging recursion of
include/mfm.h (``warmup_ref.DualAveraging``) around a No-U-turn transition in which every chain has its own step size and is steered by
its tree's acceptance statistic.  A helper of tests/test_nuts_warmup_host.py and tests/test_gpu_nuts_warmup.py, not a test.

``nuts_ref.kernel`` takes one scalar step size.  ``transition`` is that function restated with ``eps`` of shape ``[B]`` -- the two lines
that form ``eps`` and the signed step ``e`` -- and without the decision margins, on ``nuts_ref``'s own helpers; at one common step size it
gives ``nuts_ref.kernel``'s outputs bit for bit (tests/test_nuts_warmup_host.py), and chains do not interact (a finished chain keeps its
arrays, every reduction runs along a chain's own row).  The key schedule is the step-major one of ``warmup_ref._warmup``: transition j
of chain b draws from ``split(split(key, n_steps)[j], n_chain)[b]``."""
import numpy as np

from oracle import prng
from oracle.mala import MALAState
from tests import nuts_ref as nr, warmup_ref as wr

INFO = ("depth", "num_leapfrog", "is_turning", "is_divergent", "acceptance_rate", "energy")


def transition(keys, state, value_and_grad, step, max_tree_depth=10, inverse_mass=None, divergence_threshold=1000.0, f32=True):
    """One transition of every chain, chain b with the step size ``step[b]``: ``(state, info)`` with ``info`` a dict of the arrays
    ``INFO`` (``nuts_ref.NUTSInfo``'s fields of those names).  Comments: ``nuts_ref.kernel``."""
    x0, lp0, g0 = (np.asarray(a, dtype=np.float64) for a in state)
    B, d = x0.shape
    eps = np.broadcast_to(np.asarray(step, dtype=np.float64), (B,))
    minv = np.ones(d) if inverse_mass is None else np.asarray(inverse_mass, dtype=np.float64)
    r32 = (lambda a: a.astype(np.float32).astype(np.float64)) if f32 else (lambda a: a)
    kk = prng.split_rows(keys, 2)
    k_tree = kk[:, 1]
    p0 = prng.normal_rows(kk[:, 0], d) / np.sqrt(minv)
    h0 = -lp0 + 0.5 * (minv * p0 * p0).sum(1)

    left = [x0.copy(), p0.copy(), g0.copy()]
    right = [x0.copy(), p0.copy(), g0.copy()]
    prop = [x0.copy(), g0.copy(), lp0.copy(), h0.copy()]
    logw = np.zeros(B)
    psum = p0.copy()
    alive = np.ones(B, bool)
    depth = np.zeros(B, np.int64); nleap = np.zeros(B, np.int64)
    turning = np.zeros(B, bool); divergent = np.zeros(B, bool)
    acc_sum = np.zeros(B)
    ck_p = np.zeros((max(max_tree_depth - 1, 1), B, d)); ck_s = np.zeros_like(ck_p)

    for j in range(int(max_tree_depth)):
        if not alive.any():
            break
        k3 = prng.split_rows(nr.split_at_rows(k_tree, nr.MAX_DOUBLINGS, j), 3)
        k_dir, k_leaf, k_merge = k3[:, 0], k3[:, 1], k3[:, 2]
        fwd = prng.uniform_rows(k_dir) < 0.5
        f = fwd[:, None]
        z = [np.where(f, right[0], left[0]), np.where(f, right[1], left[1]), np.where(f, right[2], left[2])]
        e = np.where(fwd, eps, -eps)[:, None]
        n = 1 << j
        run = alive.copy()
        sub = [z[0].copy(), z[2].copy(), lp0.copy(), h0.copy()]
        logw_s = np.full(B, -np.inf)
        psum_s = np.zeros((B, d))
        for i in range(n):
            if not run.any():
                break
            with np.errstate(all="ignore"):
                p = z[1] + 0.5 * e * z[2]
                x = r32(z[0] + e * (minv * p))
                lp, g = value_and_grad(x)
                g = r32(np.asarray(g, dtype=np.float64))
                p = p + 0.5 * e * g
                h = -lp + 0.5 * (minv * p * p).sum(1)
                delta = h0 - h
                nan = np.isnan(delta)
                delta = np.where(nan, -np.inf, delta)
                div = nan | (-delta > divergence_threshold)
                pacc = np.minimum(np.exp(delta), 1.0)
            r = run[:, None]
            z = [np.where(r, x, z[0]), np.where(r, p, z[1]), np.where(r, g, z[2])]
            nleap += run
            acc_sum += np.where(run, pacc, 0.0)
            psum_s = np.where(r, psum_s + p, psum_s)
            logw_n = nr.logaddexp(logw_s, delta)
            if i == 0:
                take = run.copy()
            else:
                u = prng.uniform_rows(nr.split_at_rows(k_leaf, n, i))
                with np.errstate(all="ignore"):
                    take = run & (u < np.exp(delta - logw_n))
            t = take[:, None]
            sub = [np.where(t, x, sub[0]), np.where(t, g, sub[1]), np.where(take, lp, sub[2]), np.where(take, h, sub[3])]
            logw_s = np.where(run, logw_n, logw_s)
            turn_s = np.zeros(B, bool)
            if i % 2 == 0:
                if i + 1 < n:
                    slot = bin(i >> 1).count("1")
                    ck_p[slot] = np.where(r, p, ck_p[slot]); ck_s[slot] = np.where(r, psum_s, ck_s[slot])
            else:
                idx_max = bin(i >> 1).count("1")
                ones = 0
                while (i >> ones) & 1:
                    ones += 1
                for slot in range(idx_max, idx_max - ones, -1):
                    s = psum_s - ck_s[slot] + ck_p[slot]
                    turn_s |= nr._turn(minv, ck_p[slot], s)[0] | nr._turn(minv, p, s)[0]
            stop = run & (div | turn_s)
            divergent |= run & div
            turning |= run & turn_s
            alive &= ~stop
            run &= ~stop
        done = run
        if not done.any():
            continue
        u = prng.uniform_rows(k_merge)
        with np.errstate(all="ignore"):
            take = done & (u < np.minimum(np.exp(logw_s - logw), 1.0))
        t = take[:, None]
        prop = [np.where(t, sub[0], prop[0]), np.where(t, sub[1], prop[1]), np.where(take, sub[2], prop[2]), np.where(take, sub[3], prop[3])]
        logw = np.where(done, nr.logaddexp(logw, logw_s), logw)
        dn = done[:, None]
        psum = np.where(dn, psum + psum_s, psum)
        for q in range(3):
            right[q] = np.where(dn & f, z[q], right[q])
            left[q] = np.where(dn & ~f, z[q], left[q])
        depth += done
        tt = done & (nr._turn(minv, left[1], psum)[0] | nr._turn(minv, right[1], psum)[0])
        turning |= tt
        alive &= ~tt

    info = dict(depth=depth, num_leapfrog=nleap, is_turning=turning, is_divergent=divergent, acceptance_rate=acc_sum / np.maximum(nleap, 1),
                energy=prop[3])
    return MALAState(prop[0], prop[2], prop[1]), info


def nuts_warmup(key, state, value_and_grad, step0, n_steps, target=0.8, max_tree_depth=10, inverse_mass=None, divergence_threshold=1000.0):
    """``warmup_ref._warmup``'s dict (``state``, ``step_avg``, ``step_last``, ``step_traj`` and ``acc`` ``[n_steps, B]``) and per
    transition the trees' ``depth``, ``num_leapfrog``, ``is_divergent`` ``[n_steps, B]`` and the ``positions`` after it."""
    rec = {k: [] for k in ("depth", "num_leapfrog", "is_divergent", "positions")}

    def one_step(keys, st, step):
        st, info = transition(keys, st, value_and_grad, step, max_tree_depth, inverse_mass, divergence_threshold)
        for k in ("depth", "num_leapfrog", "is_divergent"):
            rec[k].append(info[k])
        rec["positions"].append(st.position)
        return st, info["acceptance_rate"]
    out = wr._warmup(one_step, key, state, step0, n_steps, target)
    out.update({k: np.stack(v) for k, v in rec.items()})
    return out
