"""Synthetic inputs of the selection / resampling kernels (cis.hip, smc.hip, anneal.hip) and the oracle-side DECISION MARGINS of
the same inputs, shared by tests/test_oracle_select_edges.py (CPU) and tests/test_gpu_select_edges.py (GPU).

Every kernel here returns integers or accept / reject flags, so the comparisons are exact.  A float64 device ``exp`` / ``log`` may
differ from numpy's by an ulp, which can only flip a decision whose operands are that close: each margin below is the distance of
the ORACLE's operands from the nearest decision boundary, computed without the device, and the tests assert that it is never
below the stated bound for the seeds they use (no case is left out)."""
import numpy as np

from oracle import flow, prng, smc
from oracle.mala import MALAState
from oracle.targets import IndepGaussian


# ---- conditional importance sampling: mfm_cis_select ----------------------------------------------------------------------------
def cis_inputs(d, n_is, B, ref_var, seed):
    """float32 solves and float64 log-densities of B chains with O(1) log-weights: u0, refs ~ N(0, ref_var), log-dets ~ N(0, 1),
    ``lps = log q0(refs) + vols + N(0, 2^2)`` and likewise ``logp``.  Every row of ``xs`` and ``pos`` is distinct."""
    rng = np.random.default_rng(seed)
    std = np.sqrt(ref_var)
    ref = IndepGaussian(d, var=ref_var)
    f32 = lambda a: a.astype(np.float32)
    u0, refs = f32(std * rng.standard_normal((B, d))), f32(std * rng.standard_normal((B * n_is, d)))
    vol0, vols = f32(rng.standard_normal(B)), f32(rng.standard_normal(B * n_is))
    xs, pos, grad = f32(rng.standard_normal((B * n_is, d))), f32(rng.standard_normal((B, d))), f32(rng.standard_normal((B, d)))
    lps = ref.logprob(refs.astype(np.float64)) + vols + 2.0 * rng.standard_normal(B * n_is)
    logp = ref.logprob(u0.astype(np.float64)) + vol0 + 2.0 * rng.standard_normal(B)
    return dict(u0=u0, vol0=vol0, refs=refs, xs=xs, vols=vols, lps=lps, pos=pos, logp=logp, grad=grad)


def cis_oracle(inp, keys, n_is, ref_var):
    """``oracle.flow.cis_select`` on the float32-rounded arrays, and per chain ``min_i |cum_i - r|`` of its inverse-CDF search
    (NaN where the table is not finite)."""
    f64 = lambda a: a.astype(np.float64)
    prev = MALAState(f64(inp["pos"]), inp["logp"].copy(), f64(inp["grad"]))
    with np.errstate(invalid="ignore", divide="ignore"):
        state, info, stats = flow.cis_select(keys, prev, f64(inp["u0"]), f64(inp["vol0"]), f64(inp["refs"]), f64(inp["xs"]),
                                             f64(inp["vols"]), inp["lps"], n_is, ref_var)
        cum = np.cumsum(stats["norm"], axis=1)
        u = prng.uniform_rows(prng.split_rows(keys, 4)[:, 3])
        margin = np.abs(cum - (cum[:, -1] * (1.0 - u))[:, None]).min(1)
    return state, info, stats, margin


def choice_from_pos(pos_after, inp, n_is):
    """The selected index (0: the current state kept) recovered from the position rows a selection step left behind."""
    B = pos_after.shape[0]
    out = np.full(B, -1)
    for b in range(B):
        if np.array_equal(pos_after[b], inp["pos"][b]):
            out[b] = 0
        for j in range(n_is):
            if np.array_equal(pos_after[b], inp["xs"][b * n_is + j]):
                assert out[b] == -1
                out[b] = j + 1
    return out


BIG = 1e4       # |log-weight| at which exp() vanishes / overflows in float64 whatever the O(100) log q0 and O(1) log-det are

# name, (lps of the chain's 5 samples, logp) with None = keep the regular value, the index the oracle must select
DEGENERATE = [
    ("all_vanish", ([-BIG] * 5, -BIG), 0),                         # 0 / 0: an all-NaN table, NaN query -> 0
    ("only_current", ([-BIG] * 5, None), 0),
    ("only_last", ([-BIG] * 4 + [None], -BIG), 5),
    ("only_middle", ([-BIG, -BIG, None, -BIG, -BIG], -BIG), 3),   # exact zeros on both sides
    ("overflow_first", ([BIG, None, None, None, None], None), 1),  # tot = inf: [0, NaN, NaN ...], NaN query -> the first NaN
    ("overflow_middle", ([None, None, BIG, None, None], None), 3),
    ("overflow_last", ([None, None, None, None, BIG], None), 5),
    ("overflow_current", ([None] * 5, BIG), 0),
    ("nan_lps", ([None, None, np.nan, None, None], None), 0),      # tot = NaN: all-NaN table -> 0
    ("nan_logp", ([None] * 5, np.nan), 0),
]


def cis_degenerate_inputs(seed=11, d=64, B=16):
    """One launch worth of chains at n_is = 5: chain i < len(DEGENERATE) carries scenario i, the rest stay regular."""
    inp = cis_inputs(d, 5, B, 1.0, seed)
    for b, (_, (lps, logp), _) in enumerate(DEGENERATE):
        for j, v in enumerate(lps):
            if v is not None:
                inp["lps"][b * 5 + j] = v
        if logp is not None:
            inp["logp"][b] = logp
    return inp


# ---- inverse-CDF searches: mfm_choice_logw and the resamplers -------------------------------------------------------------------
def search_margin(cum, v):
    """min over the queries v of the distance to the nearest entry of the sorted table cum."""
    v = np.atleast_1d(v)
    i = np.searchsorted(cum, v)
    lo, hi = cum[np.clip(i - 1, 0, cum.size - 1)], cum[np.clip(i, 0, cum.size - 1)]
    return float(np.minimum(np.abs(v - lo), np.abs(v - hi)).min())


def choice_logw_oracle(key, logw, m):
    """``jax.random.choice(key, n, (m,), p = exp(logw - max))`` as tests/test_gpu_gmm16_final.py composes it, and the margin of its
    queries relative to the table's total."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.exp(logw - logw.max())
        idx = prng.choice_p(key, p, (m,))
        cum = np.cumsum(p)
    if not np.isfinite(cum[-1]):
        return idx, np.nan
    return idx, search_margin(cum, cum[-1] * (1.0 - prng.uniform(key, (m,)))) / cum[-1]


def resample_weights(kind, n, rng):
    """The float64 weight vectors of the resampling tests, normalised in numpy."""
    if kind == "softmax":
        w = np.exp(rng.standard_normal(n))
    elif kind == "dominant":            # one weight 1 - 1e-9, the rest share 1e-9
        if n == 1:
            return np.ones(1)
        w = np.full(n, 1e-9 / (n - 1)); w[n // 2] = 1.0 - 1e-9
        return w
    elif kind == "zeros":               # a block of exact zeros in the middle
        w = np.exp(rng.standard_normal(n)); w[n // 3:2 * n // 3 + (n > 2)] = 0.0
    elif kind == "equal":
        return np.full(n, 1.0 / n)
    else:
        raise ValueError(kind)
    return w / w.sum()


def resample_queries(scheme, key, n):
    """The n search queries of ``oracle.smc``'s cumulative-sum schemes."""
    if scheme == "systematic":
        return (np.arange(n, dtype=np.float64) + prng.uniform(key, ())) / n
    if scheme == "stratified":
        return (np.arange(n, dtype=np.float64) + prng.uniform(key, (n,))) / n
    return smc._sorted_uniforms(key, n)


def resample_margin(scheme, key, w):
    """Margin of the scheme's queries on cumsum(w); for ``residual`` that of its inner multinomial draw on the residual weights
    (inf when every particle is an integer copy and the residual draw is discarded)."""
    n = w.shape[0]
    if scheme == "residual":
        nw = n * w
        ip = np.floor(nw)
        if int(ip.sum()) == n:
            return np.inf
        return resample_margin("multinomial", prng.split(key)[0], (nw - ip) / (n - int(ip.sum())))
    return search_margin(np.cumsum(w), resample_queries(scheme, key, n))


# ---- the two bisections -------------------------------------------------------------------------------------------------------
def delta_oracle(ll, target_ess, max_delta):
    """``clip(oracle.smc.ess_solver)`` and the smallest distance of any of its decisions from its boundary: |f| of every evaluation
    (the bracket tests ``f > 0`` and the branch ``f_mid < 0``) and ``|f_a - f_b - eps|`` of every loop test."""
    n = ll.shape[0]
    target_val = np.log(n * target_ess)
    seen = []

    def fun(delta):
        with np.errstate(invalid="ignore", over="ignore"):
            seen.append(smc.log_ess(np.nan_to_num(-delta * ll)) - target_val)
        return seen[-1]
    with np.errstate(invalid="ignore"):
        res = smc.dichotomy(fun, 0.0, 0.0, max_delta)
        out = float(np.clip(res, 0.0, max_delta))
    assert out == float(np.clip(smc.ess_solver(ll, target_ess, max_delta), 0.0, max_delta)) or np.isnan(out)
    f = np.array(seen)
    margins = list(np.abs(f[np.isfinite(f)]))
    if not seen[1] > 0 and seen[0] > 0:                             # the loop test was evaluated: replay it
        f_a, f_b = seen[0], seen[1]
        for f_mid in seen[2:] + [None]:
            if np.isfinite(f_a - f_b):
                margins.append(abs(f_a - f_b - 1e-4))
            if f_mid is None:
                break
            if f_mid < 0:
                f_b = f_mid
            else:
                f_a = f_mid
    return out, float(min(margins)) if margins else np.inf


def beta_oracle(prev, ll, alpha):
    """``oracle.flow.beta_fn`` and the smallest distance of its decisions from their boundaries: |value| of every evaluation
    (``sign`` and ``sign * value > 0``) and ``||value| - tol|`` of every loop test."""
    n = ll.shape[0]
    out = flow.beta_fn(prev, ll, alpha, n)
    f = lambda b: flow.ess_zero(b, prev, ll, alpha, n)
    low, high = float(prev), 1.0
    fl, fh = f(low), f(high)
    sign = 1 if (fl < 0 and fh >= 0) else (-1 if (fl > 0 and fh <= 0) else 0)
    margins = [abs(fl), abs(fh)]
    params, err, it = 0.5 * (low + high), np.inf, 0
    while err > 1e-5 and it < 30:
        params = 0.5 * (high + low)
        value = f(params)
        if sign * value > 0:
            high = params
        else:
            low = params
        err = abs(value)
        margins += [err, abs(err - 1e-5)]
        it += 1
    assert params == out            # the replay above follows beta_fn
    return out, sign, float(min(margins))
