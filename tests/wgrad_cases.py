"""Cases and float64 references shared by the weight-gradient partition tests (test_gpu_wgrad_partition.py on the GPU,
test_oracle_wgrad_bound.py on the CPU): the four networks, the chain counts, the 64 x 64 block table of the tile family's
weight-gradient kernels restated in canonical coordinates, and the summation-order bound."""
import functools

import numpy as np

from oracle import fm, prng

# name -> (setup, keywords): S small, R ragged widths (clamped tile rows), H the headline network, M the 4-mode mixture
NETS = {
    "S": ("phi4", dict(d=64, hidden=32, F=16)),
    "R": ("phi4", dict(d=40, hidden=48, F=10)),
    "H": ("phi4", dict(d=256, hidden=128, F=128)),
    "M": ("gmm4", dict(hidden=32, F=16)),
    "P": ("lgcp", dict(n=32, hidden=1024, F=128)),          # the pines width (wide family only)
}
CASES_A = [("S", 16), ("S", 48), ("S", 144), ("S", 160), ("S", 208), ("S", 272), ("S", 912),
           ("R", 144), ("R", 400), ("H", 144), ("H", 272), ("H", 912), ("M", 208)]
U32 = 2.0 ** -24       # unit roundoff of float32
# The flow-matching key of every case.  The network is piecewise linear: where a ReLU pre-activation z of the float64 oracle lies
# within float32 rounding of zero, a float32 evaluation may legitimately take the other branch, and the two gradients then differ
# by that chain's whole contribution to the unit (1 / B of the sum, far above 2e-4 of its maximum) -- at 912 chains x 200 - 800
# ReLU units such a unit exists for most keys (key 11 at S-912: z = -1.3e-8 against a row scale of 0.4).  The oracle is a reference
# only where that cannot happen, so each case uses the first key from 11 on (H-912, P: the best of 11..50 / 11..16) whose smallest
# |z| / (sum_k |a_k| |w_kn| + |b_n|) over all ReLU units is at least RELU_MARGIN = 8 u.  A plain numpy float32 evaluation of these
# networks differs from the oracle's z by at most 7.2 u of that scale (measured over S, H and P; the worst-case bound (K + 2) u is
# met by no key at these sizes).  Chosen from the oracle alone; tests/test_oracle_wgrad_bound.py asserts the margin of every case.
RELU_MARGIN = 8 * U32
KEYS = {("S", 208): 12, ("S", 272): 12, ("S", 912): 12, ("H", 272): 14, ("H", 912): 41, ("P", 64): 12, ("P", 80): 16}
ORACLE_CASES = [(n, B, None) for n, B in CASES_A] + [("S", 160, 150), ("S", 208, 200), ("S", 80, None), ("P", 64, None), ("P", 80, None)]


def case_key(net, B):
    return prng.PRNGKey(KEYS.get((net, B), 11))
PF4 = 4 * 4 * 64 + 16  # float4 per partial block of the stream-K kernel (wgrad_sk.hip: WSK_PF4)


@functools.lru_cache(maxsize=None)
def setup(net, B, **kw):
    """(args, dist, model, params, x32) of network ``net`` with ``B`` chains; x32 are the chains' float32 positions."""
    from tests import gpu_util as gu
    kind, k = NETS[net]
    fn = {"phi4": gu.phi4_setup, "gmm4": gu.gmm4_setup, "lgcp": gu.lgcp_setup}[kind]
    args, dist, _, model, _ = fn(B=B, **k, **kw)
    params = gu.rand_params(model, seed=3)
    x32 = np.ascontiguousarray(dist.init_params.astype(np.float32))
    x32.setflags(write=False)
    return args, dist, model, params, x32


def flat64(tree):
    return np.concatenate([np.concatenate([np.asarray(p["kernel"], dtype=np.float64).reshape(-1), np.asarray(p["bias"], dtype=np.float64).reshape(-1)])
                           for p in tree])


@functools.lru_cache(maxsize=None)
def oracle(net, B, n_valid=None, operands=False):
    """Float64 loss, gradient (rounded to float32 by the oracle, flat), absolute-product sums (flat float64) of the first
    ``n_valid`` of ``B`` chains; computed once per case and shared, read-only."""
    args, dist, model, params, x32 = setup(net, B)
    nv = B if n_valid is None else n_valid
    loss, grads, S, ops = fm.loss_and_grad(model, params, case_key(net, B), x32[:nv].astype(np.float64), args.sigma, abs_sums=True, operands=True)
    out = dict(loss=float(loss), grads=grads, flat=flat64(grads), S=flat64(S), ops=ops if operands else None)
    for v in (out["flat"], out["S"]):
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def relu_margin(net, B, n_valid=None):
    """Smallest |z| / (sum_k |a_k| |w_kn| + |b_n|) over the ReLU units of the oracle's forward pass of a case (see KEYS)."""
    args, dist, model, params, x32 = setup(net, B)
    nv = B if n_valid is None else n_valid
    t, cond, _ = fm.cond_flow_batch(case_key(net, B), x32[:nv].astype(np.float64), args.sigma)
    _, (acts_in, pre, _) = model.forward(params, cond, t, cache=True)
    linear = (len(model.hidden_t) + len(model.hidden_x), len(pre) - 1)          # the gate and the output layer have no activation
    m = np.inf
    for l, (a, z) in enumerate(zip(acts_in, pre)):
        if l not in linear:
            scale = np.abs(a) @ np.abs(params[l]["kernel"].astype(np.float64)) + np.abs(params[l]["bias"].astype(np.float64))
            m = min(m, float((np.abs(z) / scale).min()))
    return m


def order_bound(B, S):
    """|float32 sum in one order - float32 sum in another| of B products whose absolute values total S: each side is within
    gamma_{B+1} S <= (B + 2) 2^-24 S of the exact sum (one rounding per product, B - 1 per addition chain; Higham, Accuracy and
    Stability of Numerical Algorithms, section 3.1), hence twice that between the two."""
    return 2.0 * (B + 2) * U32 * S


def r16(n):
    return (n + 15) // 16 * 16


def blocks(model):
    """The 64 x 64 blocks of the tile family's weight-gradient job table (api.hip: for every layer, n-tiles then k-tiles in steps of
    four 16-tiles) as ``(layer, k, n)`` with the CANONICAL kernel rows ``k`` and columns ``n`` each block covers.  The first joint
    layer's input is [x branch | t branch] with the x part padded to 16 (mlp.hip.h: packed_row)."""
    shapes = model.layer_shapes()
    lt, lx = len(model.hidden_t), len(model.hidden_x)
    joint = lt + lx + 1
    out = []
    for l, (K, N) in enumerate(shapes):
        if l == joint:
            hx = shapes[lt + lx - 1][1]
            rows = np.concatenate([np.arange(hx), np.full(r16(hx) - hx, -1), np.arange(hx, K), np.full(r16(K - hx) - (K - hx), -1)])
        else:
            rows = np.concatenate([np.arange(K), np.full(r16(K) - K, -1)])
        for n0 in range(0, r16(N), 64):
            for k0 in range(0, len(rows), 64):
                k = rows[k0:k0 + 64]
                out.append((l, k[k >= 0], np.arange(n0, min(n0 + 64, N))))
    return out


def layer_offsets(model):
    """(offset of the kernel, offset of the bias) of every layer in the canonical flat vector."""
    off, o = [], 0
    for K, N in model.layer_shapes():
        off.append((o, o + K * N)); o += K * N + N
    return off


def block_elements(model):
    """Flat canonical indices of every block of ``blocks`` (its kernel elements, plus its bias elements for the k0 = 0 block)."""
    off = layer_offsets(model)
    shapes = model.layer_shapes()
    out = []
    for l, k, n in blocks(model):
        idx = (off[l][0] + k[:, None] * shapes[l][1] + n[None, :]).reshape(-1)
        if k.size and k[0] == 0:
            idx = np.concatenate([idx, off[l][1] + n])
        out.append(idx)
    return out
