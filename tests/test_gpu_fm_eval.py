"""GPU parity of the forward-only eval-loss kernel (fm.hip: fm_eval_kernel, 32 or 64 samples per workgroup, engaged from 16,384
samples per call) against the float64 oracle -- per kernel instance and resolved to single 16-row tiles.

Every case names the instance it must run and asserts it through ``mfm_fm_eval_instance`` (the function ``launch_fm`` itself calls).
Contexts are created AFTER the switches are set: they are read once per ``mfm_create``.  N = 16,384 is the smallest count that
engages the kernel; ``xs`` has N + 64 rows.  S(a, b) is the oracle's loss of rows [a, b) at global indices off + [a, b) of T (the loss
is a sum: contributions add).  Per case:

1. total: ``fm_loss(xs[:N])`` against S(0, N) at the project's stated 2e-5 relative;
2. tail rows: ``fm_loss(xs[:N + 16 k]) - fm_loss(xs[:N])`` (k = 1 with 32 rows per workgroup, k = 1, 2, 3 with 64) is the partly
   empty last workgroup's partial -- the full workgroups are bit-identical in both calls -- against S(N, N + 16 k);
3. row-tile independence: ``fm_loss(xs[16:16 + N], off + 16) - fm_loss(xs[:N], off)``, where every sample sits in the other row
   tile of its workgroup (or in the next workgroup), against S(N, N + 16) - S(0, 16);
4. the 16-row tile kernel on a second context created under MFM_EVAL16 (query: 0) gives the same totals on N and N + 16 k rows.

Bounds of 2 and 3: nothing fixed in advance.  The yardstick is the 16-row tile kernel every small-n test anchors: ``fm_loss`` on those
16 k rows alone (n < 16,384) at the same global indices.  Its deviation from the oracle on the same quantity is e16; the eval
kernel must be within max(4 e16, 1e-6 |S|) of the oracle (4: the other float32 grouping of <= 16 addends per lane and the vector-ALU
form of the first x layer).  So that the relative floor means something, no compared S may be below 1e-3 of the mean 16-row
contribution (asserted; the seeds below satisfy it).  Bound of 4: AB_REL, four times the largest distance of the two device paths
measured over all cases.  A planted error (the oracle's draws of the last 16 rows taken 16 global indices off) must miss the device
by >= 10 bounds.

Measured on an MI355X (deviations from the oracle and bounds relative to the compared S; the two device paths relative to the total):
case-rows     instance  total rel   tail: eval off / 16-row off / bound (of S, worst k)   shift: eval off / 16-row off / bound (of S)   two paths rel
chain-32      0x0320    1.0e-09     k=1 2.1e-09 / 2.1e-09 / 1.0e-06                          6.5e-08 / 6.5e-08 / 1.0e-06                  1.3e-11
nochain-32    0x0120    1.0e-09     k=1 2.1e-09 / 2.1e-09 / 1.0e-06                          6.5e-08 / 6.5e-08 / 1.0e-06                  1.3e-11
rows64-64     0x0140    1.0e-09     k=3 4.8e-09 / 3.4e-09 / 1.0e-06                          6.5e-08 / 6.5e-08 / 1.0e-06                  1.7e-11
act-tanh-32   0x0020    5.1e-09     k=1 4.8e-08 / 3.2e-08 / 1.0e-06                          7.5e-07 / 9.7e-07 / 3.9e-06                  9.4e-11
act-tanh-64   0x0040    5.1e-09     k=1 4.8e-08 / 3.2e-08 / 1.0e-06                          7.5e-07 / 9.7e-07 / 3.9e-06                  1.1e-10
act-elu-32    0x0020    4.6e-09     k=1 2.7e-08 / 3.4e-08 / 1.0e-06                          3.1e-07 / 6.6e-07 / 2.6e-06                  1.9e-10
act-elu-64    0x0040    4.6e-09     k=1 2.7e-08 / 3.4e-08 / 1.0e-06                          3.1e-07 / 6.6e-07 / 2.6e-06                  2.0e-10
act-gelu-32   0x0020    2.2e-09     k=1 3.4e-08 / 1.9e-08 / 1.0e-06                          1.9e-06 / 1.9e-06 / 7.5e-06                  3.7e-10
act-gelu-64   0x0040    2.2e-09     k=1 3.4e-08 / 1.9e-08 / 1.0e-06                          1.9e-06 / 1.9e-06 / 7.5e-06                  3.7e-10
act-swish-32  0x0020    1.4e-09     k=1 9.7e-09 / 5.5e-09 / 1.0e-06                          5.9e-07 / 5.9e-07 / 2.3e-06                  1.9e-10
act-swish-64  0x0040    1.4e-09     k=3 1.2e-08 / 7.2e-09 / 1.0e-06                          5.9e-07 / 5.9e-07 / 2.3e-06                  1.9e-10
padded-32     0x0120    1.9e-09     k=1 1.1e-08 / 1.1e-08 / 1.0e-06                          4.0e-07 / 7.0e-07 / 2.8e-06                  1.7e-10
k17-32        0x0120    2.3e-10     k=1 5.5e-09 / 2.3e-09 / 1.0e-06                          9.1e-08 / 9.1e-08 / 1.0e-06                  2.1e-10
k17-64        0x0140    2.3e-10     k=3 1.6e-08 / 6.9e-09 / 1.0e-06                          9.1e-08 / 9.1e-08 / 1.0e-06                  2.3e-10
phi4-16-32    0x0120    4.0e-08     k=1 6.7e-08 / 7.3e-08 / 1.0e-06                          2.7e-08 / 8.5e-09 / 1.0e-06                  4.7e-09
phi4-16-64    0x0140    4.0e-08     k=1 6.7e-08 / 7.3e-08 / 1.0e-06                          2.7e-08 / 8.5e-09 / 1.0e-06                  4.7e-09
phi4-8-32     0x0120    1.5e-09     k=1 1.3e-07 / 3.9e-07 / 1.6e-06                          1.8e-07 / 6.5e-07 / 2.6e-06                  2.6e-09
phi4-8-64     0x0140    1.5e-09     k=3 2.0e-07 / 3.0e-07 / 1.2e-06                          1.8e-07 / 6.5e-07 / 2.6e-06                  2.6e-09
uncond-32     0x0120    5.2e-10     k=1 1.4e-08 / 1.4e-08 / 1.0e-06                          3.6e-07 / 3.6e-07 / 1.5e-06                  0.0e+00
widegauss-32  0x0120    1.1e-09     k=1 1.1e-08 / 1.8e-08 / 1.0e-06                          4.2e-08 / 1.2e-07 / 1.0e-06                  4.7e-10
shard-32      0x0120    1.4e-09     k=1 1.3e-09 / 1.2e-08 / 1.0e-06                          3.4e-07 / 1.8e-07 / 1.0e-06                  3.4e-10
largest distance of the two device paths: 4.687e-09 (phi4-16, rows 64) -> AB_REL = 4 x that = 1.875e-08.
Totals: at most 4.0e-8 of the 2e-5 granted.  The planted error misses by 3.99e4 bounds.  phi-four d = 8 (d < dp = 16) is
accepted by mfm_create and runs as listed.
"""
import functools

import numpy as np
import pytest

from oracle import fm, prng, targets

pytestmark = pytest.mark.gpu

N = 16384
AB_REL = 1.88e-8    # 4 x 4.69e-9, the largest measured distance of the two device paths (phi4-16; table above)

RELU, CHAIN = 0x100, 0x200          # _lib.EVAL_RELU, _lib.EVAL_CHAIN (restated: importing _lib needs the built library)

# case -> (setup, setup keywords, switches, {rows: instance})
_GMM4 = dict(hidden=32, F=16)
_ACT = {a: ("gmm4", dict(_GMM4, non_linearity=a), {}, {32: 32, 64: 64}) for a in ("tanh", "elu", "gelu", "swish")}
CASES = {
    "chain": ("gmm16", dict(hidden=128, F=128), {}, {32: 32 | RELU | CHAIN}),
    "nochain": ("gmm16", dict(hidden=128, F=128), {"MFM_EVAL_NO_CHAIN": "1"}, {32: 32 | RELU}),
    "rows64": ("gmm16", dict(hidden=128, F=128), {}, {64: 64 | RELU}),
    **{f"act-{a}": v for a, v in _ACT.items()},
    # widths that are no multiple of 16 (zero pad columns) and divide the workgroup's 512 threads neither as F nor as hx1: the
    # general Fourier and x1 loops
    "padded": ("gmm4", dict(hidden=([100, 100], [100, 100], [100, 100]), F=10), {}, {32: 32 | RELU}),
    "k17": ("gmm17", dict(hidden=32, F=16), {}, {32: 32 | RELU, 64: 64 | RELU}),           # > 16 modes: serial gmm_eval on the last wave
    "phi4-16": ("phi4", dict(d=16, hidden=32, F=16), {}, {32: 32 | RELU, 64: 64 | RELU}),    # 2 R d > 512: the general draw path
    "phi4-8": ("phi4", dict(d=8, hidden=32, F=16), {}, {32: 32 | RELU, 64: 64 | RELU}),      # d < dp; two-thread draws at 32, general at 64
    "uncond": ("gmm4", dict(_GMM4, cond_flow=False), {}, {32: 32 | RELU}),
    "widegauss": ("gmm4", dict(_GMM4, ref_dist="widegauss"), {}, {32: 32 | RELU}),
    "shard": ("gmm4", dict(_GMM4), {}, {32: 32 | RELU}),
}
PARAMS = [(c, r) for c, v in CASES.items() for r in v[3]]


def _dev(x, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


@functools.lru_cache(maxsize=None)
def _case(name):
    """Oracle side of a case, computed once and shared by its row counts: setup, samples and the oracle's sums."""
    from tests import gpu_util as gu
    kind, kw, env, inst = CASES[name]
    if kind == "gmm16":
        args, dist, k, model, state = gu.gmm16_setup(B=64, hutchs=False, **kw)
    elif kind == "gmm4":
        args, dist, k, model, state = gu.gmm4_setup(B=64, **kw)
    elif kind == "gmm17":           # the 17-mode ring of tests/mcmc_bits_cases.py
        from oracle import loop
        ang = 2 * np.pi * np.arange(17) / 17
        dist = targets.GaussianMixture(6.0 * np.stack([np.cos(ang), np.sin(ang)], 1), np.ones((17, 2)), np.ones(17) / 17)
        args = loop.default_args(example="4-mode", dim=2, num_chain=64, step_size=0.2, seed=1, fourier_dim=kw["F"], **gu.hidden_lists(kw["hidden"]))
        k, model, state, _, _, _ = loop.setup(dist, args)
    else:
        args, dist, k, model, state = gu.phi4_setup(B=64, **kw)
    params = gu.rand_params(model, seed=3)
    if dist.kind == "gmm":
        xs = dist.sample_model_rows(prng.split(prng.PRNGKey(21), N + 64)).astype(np.float32)
    else:
        xs = np.random.default_rng(5).uniform(-1, 1, (N + 64, args.dim)).astype(np.float32)
    T, off = (4 * N, 16 * 1001) if name == "shard" else (N + 64, 0)      # shard: global indices, an odd multiple of 16
    key = prng.PRNGKey(12)
    okw = dict(cond_flow=bool(args.cond_flow), need_grad=False)
    if args.cond_flow:
        okw["ref_std"] = float(np.sqrt(targets.REF_VARS[args.ref_dist]))

    def S(a, b, shift=0):
        return fm.loss_and_grad(model, params, key, xs[a:b].astype(np.float64), args.sigma, n_total=T, start=off + a + shift, **okw)[0]

    o = dict(args=args, dist=dist, model=model, params=params, xs=xs, T=T, off=off, key=key, env=env, S=S)
    o["total"] = S(0, N)
    o["head"] = S(0, 16)
    o["tiles"] = [S(N + 16 * j, N + 16 * j + 16) for j in range(3)]            # S(N, N + 16 k) = sum(tiles[:k])
    mean16 = o["total"] / (N // 16)
    for k_ in (1, 2, 3):
        assert sum(o["tiles"][:k_]) > 1e-3 * mean16, (name, k_)
    assert abs(o["tiles"][0] - o["head"]) > 1e-3 * mean16, name                 # else the relative floors below are empty: change the seed
    return o


def _ctx(o, monkeypatch, env):
    from tests import gpu_util as gu
    for k in ("MFM_EVAL_ROWS", "MFM_EVAL_NO_CHAIN", "MFM_EVAL16"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return gu.make_ctx(o["dist"], o["args"], fourier=o["model"].f, params=o["params"], max_eval=N + 64)


def _measure(case, rows, monkeypatch):
    """Every device figure of one (case, rows): dict of floats."""
    import torch
    o = _case(case)
    xs, T, off, key = _dev(o["xs"]), o["T"], o["off"], o["key"]
    out = torch.zeros(1, dtype=torch.float64, device="cuda")

    def loss(ctx, a, b, shift=0):
        ctx.fm_loss(key, xs[a:b], out, n_total=T, offset=off + a + shift)
        return out.item()

    ks = (1,) if rows == 32 else (1, 2, 3)
    ctx = _ctx(o, monkeypatch, dict(o["env"], MFM_EVAL_ROWS=str(rows)))
    want = CASES[case][3][rows]
    m = dict(inst=[ctx.fm_eval_instance(N + 16 * k) for k in (0,) + ks] + [ctx.fm_eval_instance(16 * k) for k in ks], want=want, ks=ks)
    m["total"] = loss(ctx, 0, N)
    m["ext"] = {k: loss(ctx, 0, N + 16 * k) for k in ks}
    m["shifted"] = loss(ctx, 16, 16 + N)
    # the yardstick: the 16-row tile kernel (n < 16,384) on the same rows at the same global indices
    m["y_tail"] = {k: loss(ctx, N, N + 16 * k) for k in ks}
    m["y_head"] = loss(ctx, 0, 16)
    ctx.close()
    c16 = _ctx(o, monkeypatch, dict(o["env"], MFM_EVAL_ROWS=str(rows), MFM_EVAL16="1"))
    m["inst16"] = [c16.fm_eval_instance(N + 16 * k) for k in (0,) + ks]
    m["total16"] = loss(c16, 0, N)
    m["ext16"] = {k: loss(c16, 0, N + 16 * k) for k in ks}
    c16.close()
    return o, m


@pytest.mark.parametrize("case,rows", PARAMS)
def test_eval_kernel_instance_matches_oracle_per_row_tile(case, rows, monkeypatch):
    o, m = _measure(case, rows, monkeypatch)
    ks = m["ks"]
    # the instance each call ran: the eval kernel for every count >= N, the 16-row tile for the yardstick calls and under MFM_EVAL16
    assert m["inst"] == [m["want"]] * (1 + len(ks)) + [0] * len(ks), (m["inst"], m["want"])
    assert m["inst16"] == [0] * (1 + len(ks)), m["inst16"]
    # 1. total
    rel = abs(m["total"] - o["total"]) / abs(o["total"])
    print(f"{case} rows={rows}: total {m['total']:.10g} (oracle {o['total']:.10g}), rel {rel:.2e}")
    assert rel < 2e-5
    worst = 0.0
    # 2. tail rows, resolved
    for k in ks:
        s = sum(o["tiles"][:k])
        e16 = abs(m["y_tail"][k] - s)
        bound = max(4 * e16, 1e-6 * abs(s))
        dev = abs((m["ext"][k] - m["total"]) - s)
        print(f"{case} rows={rows}: tail k={k}: S {s:.8g}, eval kernel off by {dev:.2e}, 16-row tile by {e16:.2e}, bound {bound:.2e} ({dev / bound:.2f} bounds)")
        worst = max(worst, dev / bound)
        assert dev <= bound, (k, dev, bound)
    # 3. row-tile independence
    s = o["tiles"][0] - o["head"]
    e16 = abs((m["y_tail"][1] - m["y_head"]) - s)
    bound = max(4 * e16, 1e-6 * abs(s))
    dev = abs((m["shifted"] - m["total"]) - s)
    print(f"{case} rows={rows}: shift: S {s:.8g}, eval kernel off by {dev:.2e}, 16-row tile by {e16:.2e}, bound {bound:.2e} ({dev / bound:.2f} bounds)")
    worst = max(worst, dev / bound)
    assert dev <= bound, (dev, bound)
    # 4. the honest A/B: the 16-row tile kernel from its own context
    ab = max([abs(m["total"] - m["total16"]) / abs(m["total16"])] + [abs(m["ext"][k] - m["ext16"][k]) / abs(m["ext16"][k]) for k in ks])
    print(f"{case} rows={rows}: eval kernel vs 16-row tile on N and N + 16 k rows: rel {ab:.2e}; worst of 2 and 3: {worst:.2f} bounds")
    assert ab <= AB_REL, (ab, AB_REL)


def test_planted_wrong_global_index_of_the_tail_rows_is_caught(monkeypatch):
    """The oracle with the last 16 rows' draws taken 16 global indices off must miss the device's tail difference by >= 10 of the
    bounds the parity test grants (so a kernel that indexed the partly empty workgroup's draws wrongly would fail it)."""
    o, m = _measure("chain", 32, monkeypatch)
    s = o["tiles"][0]
    bound = max(4 * abs(m["y_tail"][1] - s), 1e-6 * abs(s))
    wrong = o["S"](N, N + 16, shift=16)
    miss = abs((m["ext"][1] - m["total"]) - wrong)
    print(f"planted: S {s:.8g}, with the draws 16 indices off {wrong:.8g}: the device misses it by {miss / bound:.0f} bounds")
    assert miss >= 10 * bound, (miss, bound)
