"""The No-U-turn sampler of mfm_amd/csrc/nuts.hip restated in float64 numpy, batched over chains.  A helper of tests/test_nuts_ref.py and
tests/test_gpu_nuts.py, not a test.

Multinomial NUTS in the iterative, checkpointed form (Betancourt's "Conceptual Introduction", appendix A; the formulation of NumPyro
and blackjax), with the kernel's key schedule and rounding points:

* ``k_mom, k_tree = split(kb, 2)``; momentum ``normal(k_mom, d) / sqrt(minv)`` (``oracle.hmc.kernel``'s draw);
* doubling ``j`` draws from ``kd = split(k_tree, 16)[j]`` -> ``k_dir, k_leaf, k_merge = split(kd, 3)``: forward iff
  ``uniform(k_dir) < 0.5``, leaf ``i`` of the subtree draws ``uniform(split(k_leaf, 2^j)[i])``, the merge ``uniform(k_merge)``;
* leapfrog: half kick, drift (``f32``: position rounded to float32), value and gradient (``f32``: gradient rounded to float32), half
  kick; ``-eps`` backward; ``H = -logp + sum(minv p^2) / 2``; a leaf has ``delta = H0 - H`` (NaN -> -inf), weight ``exp(delta)``, and
  is divergent when ``H - H0 > threshold`` or ``delta`` was NaN;
* subtree: uniform progressive sampling, the U-turn checkpoints by the bits of the leaf index; tree: biased progressive sampling, the
  U-turn test on the whole tree's end points.  A subtree that stops early ends the transition and none of its leaves is proposed.

Every chain of the batch walks the same leaf indices, so one masked loop serves all of them: a chain that has finished keeps its
arrays.  Besides the outcome a transition returns the smallest decision margin each chain met, so that a comparison with float32-fed
arithmetic can set the chains aside whose tree hung on a draw too close to call:

* ``margin_draw``: over the selection and merge draws, ``|log u - log ratio|``;
* ``margin_turn``: over the U-turn tests, ``|dot| / (|v| |s|)``;
* ``margin_div``: over the leaves, ``|(H - H0) - threshold|``."""
from collections import namedtuple

import numpy as np

from oracle import prng
from oracle.mala import MALAState

MAX_DOUBLINGS = 16          # the fan-out of k_tree: fixed, so that a tree under a smaller limit is a prefix of one under a larger limit

NUTSInfo = namedtuple("NUTSInfo", "depth num_leapfrog is_turning is_divergent acceptance_rate energy "
                                  "margin_draw margin_turn margin_div directions stopped_in_subtree")


def split_at_rows(keys, num, idx):
    """``split(keys[b], num)[idx]`` for every row: [B, 2] -> [B, 2]."""
    keys = np.asarray(keys, dtype=np.uint32)
    out = np.empty_like(keys)
    for w in range(2):
        m = 2 * int(idx) + w
        lo = m < num
        c0 = np.full(keys.shape[0], m if lo else m - num, dtype=np.uint32)
        y0, y1 = prng.threefry2x32((keys[:, 0], keys[:, 1]), c0, (c0 + np.uint32(num)).astype(np.uint32))
        out[:, w] = y0 if lo else y1
    return out


def logaddexp(a, b):
    """``log(exp(a) + exp(b))`` as the kernel forms it: ``max + log1p(exp(-|a - b|))``, -inf when both are."""
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.maximum(a, b)
        r = m + np.log1p(np.exp(-np.abs(a - b)))
    return np.where(np.isneginf(m), -np.inf, r)


def _turn(minv, p_end, s):
    """The U-turn test of one end point against the span ``s``: ``(turning, margin)`` per chain."""
    v = minv * p_end
    dot = (v * s).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        marg = np.abs(dot) / (np.sqrt((v * v).sum(1)) * np.sqrt((s * s).sum(1)))
    return dot <= 0, np.where(np.isnan(marg), np.inf, marg)


def _log(u):
    with np.errstate(divide="ignore"):
        return np.log(u)


def _margin(log_u, log_ratio):
    with np.errstate(invalid="ignore"):
        m = np.abs(log_u - log_ratio)
    return np.where(np.isnan(m), np.inf, m)


def kernel(keys, state, value_and_grad, step_size, max_tree_depth=10, inverse_mass=None, divergence_threshold=1000.0, f32=True):
    """One transition of every chain.  ``keys`` [B, 2]: the chains' step keys; ``state``: ``MALAState`` (float64 arrays);
    ``value_and_grad(x [B, d]) -> (logp [B], grad [B, d])``.  Returns ``(state, NUTSInfo)``."""
    x0, lp0, g0 = (np.asarray(a, dtype=np.float64) for a in state)
    B, d = x0.shape
    eps = float(step_size)
    minv = np.ones(d) if inverse_mass is None else np.asarray(inverse_mass, dtype=np.float64)
    r32 = (lambda a: a.astype(np.float32).astype(np.float64)) if f32 else (lambda a: a)
    kk = prng.split_rows(keys, 2)
    k_tree = kk[:, 1]
    p0 = prng.normal_rows(kk[:, 0], d) / np.sqrt(minv)
    h0 = -lp0 + 0.5 * (minv * p0 * p0).sum(1)

    # the two end points (position, momentum, gradient), the tree's proposal and its sums
    left = [x0.copy(), p0.copy(), g0.copy()]
    right = [x0.copy(), p0.copy(), g0.copy()]
    prop = [x0.copy(), g0.copy(), lp0.copy(), h0.copy()]
    logw = np.zeros(B)
    psum = p0.copy()
    alive = np.ones(B, bool)
    depth = np.zeros(B, np.int64); nleap = np.zeros(B, np.int64)
    turning = np.zeros(B, bool); divergent = np.zeros(B, bool); in_sub = np.zeros(B, bool)
    acc_sum = np.zeros(B)
    m_draw = np.full(B, np.inf); m_turn = np.full(B, np.inf); m_div = np.full(B, np.inf)
    dirs = np.zeros((B, max_tree_depth), np.int8)          # +1 forward, -1 backward, 0 not drawn
    ck_p = np.zeros((max(max_tree_depth - 1, 1), B, d)); ck_s = np.zeros_like(ck_p)

    for j in range(int(max_tree_depth)):
        if not alive.any():
            break
        k3 = prng.split_rows(split_at_rows(k_tree, MAX_DOUBLINGS, j), 3)
        k_dir, k_leaf, k_merge = k3[:, 0], k3[:, 1], k3[:, 2]
        fwd = prng.uniform_rows(k_dir) < 0.5
        dirs[alive, j] = np.where(fwd, 1, -1)[alive]
        f = fwd[:, None]
        z = [np.where(f, right[0], left[0]), np.where(f, right[1], left[1]), np.where(f, right[2], left[2])]
        e = np.where(fwd, eps, -eps)[:, None]
        n = 1 << j
        run = alive.copy()                                  # chains still building this subtree
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
                md = np.abs(-delta - divergence_threshold)
            r = run[:, None]
            z = [np.where(r, x, z[0]), np.where(r, p, z[1]), np.where(r, g, z[2])]
            nleap += run
            acc_sum += np.where(run, pacc, 0.0)
            m_div = np.where(run, np.minimum(m_div, np.where(np.isnan(md), np.inf, md)), m_div)
            psum_s = np.where(r, psum_s + p, psum_s)
            logw_n = logaddexp(logw_s, delta)
            if i == 0:
                take = run.copy()
            else:
                u = prng.uniform_rows(split_at_rows(k_leaf, n, i))
                with np.errstate(all="ignore"):
                    lr = delta - logw_n
                    take = run & (u < np.exp(lr))
                m_draw = np.where(run, np.minimum(m_draw, _margin(_log(u), lr)), m_draw)
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
                    ta, ma = _turn(minv, ck_p[slot], s)
                    tb, mb = _turn(minv, p, s)
                    turn_s |= ta | tb
                    m_turn = np.where(run, np.minimum(m_turn, np.minimum(ma, mb)), m_turn)
            stop = run & (div | turn_s)
            divergent |= run & div
            turning |= run & turn_s
            in_sub |= stop
            alive &= ~stop
            run &= ~stop
        # chains whose subtree is complete: the merge, the new end point, the tree's own U-turn test
        done = run
        if not done.any():
            continue
        u = prng.uniform_rows(k_merge)
        with np.errstate(all="ignore"):
            lr = logw_s - logw
            take = done & (u < np.minimum(np.exp(lr), 1.0))
        m_draw = np.where(done, np.minimum(m_draw, _margin(_log(u), lr)), m_draw)
        t = take[:, None]
        prop = [np.where(t, sub[0], prop[0]), np.where(t, sub[1], prop[1]), np.where(take, sub[2], prop[2]), np.where(take, sub[3], prop[3])]
        logw = np.where(done, logaddexp(logw, logw_s), logw)
        dn = done[:, None]
        psum = np.where(dn, psum + psum_s, psum)
        for q in range(3):
            right[q] = np.where(dn & f, z[q], right[q])
            left[q] = np.where(dn & ~f, z[q], left[q])
        depth += done
        ta, ma = _turn(minv, left[1], psum)
        tb, mb = _turn(minv, right[1], psum)
        m_turn = np.where(done, np.minimum(m_turn, np.minimum(ma, mb)), m_turn)
        tt = done & (ta | tb)
        turning |= tt
        alive &= ~tt

    info = NUTSInfo(depth, nleap, turning, divergent, acc_sum / np.maximum(nleap, 1), prop[3], m_draw, m_turn, m_div, dirs, in_sub)
    return MALAState(prop[0], prop[2], prop[1]), info
