"""Cost of the phi-four boundary on the headline shape: d = 256, 4096 chains, widths 128, --hutch (the shape-specialised solver and
the static training kernel), with the same network, chains and keys for Dirichlet 0 (the default PHI4_BC0 kernels), Dirichlet 1
and periodic (the PHI4_BCRT instances, targets.hip.h), and for the 16 x 16 lattice (dim_phys = 2: the same PHI4_BCRT instances with
four neighbours by index) under periodic and Dirichlet-0 boundaries.  Per row:

  flow step, adaptive Dopri5   (RWMH, two solves per chain; attempted steps per chain printed beside the time)
  flow step, fixed RK4 x 16    (the like-for-like comparison: every boundary does the same number of evaluations)
  training iteration           (mfm_train_iter: the fused MALA step + flow-matching loss / gradient + AdamW)

The rows' contexts exist side by side: each gets `--warmup` untimed calls, then `--reps` rounds time every boundary once,
in rotating order, with HIP events around the call on the default stream after a synchronisation.  The median and the min..max spread
are printed; the raw times go to `--out`.  (The flow step is timed with its chain reset and mala_init, whose own median is subtracted.)

    python tools/phi4_bc_time.py [--reps 15] [--warmup 5] [--out profiles/r08_phi4_2d_time.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

BCS = [("dirichlet-0", None), ("dirichlet-1", [0.0, 1.0]), ("periodic", [1.0, 0.0]),
       ("2d-periodic", [1.0, 0.0, 2.0]), ("2d-dirichlet-0", [0.0, 0.0, 2.0])]


def _ctx(bc_tail, **kw):
    from mfm_amd import _lib
    from tests import gpu_util as gu
    args, dist, k, model, state = gu.phi4_setup(d=256, B=4096, hidden=128, F=128, **kw)
    params = gu.rand_params(model, seed=9, out_scale=2.0)
    params[4]["kernel"] *= 1e-3; params[4]["bias"] *= 1e-3
    ctx = gu.make_ctx(dist, args, fourier=model.f, params=params)
    if bc_tail is not None:
        ctx.set_target(_lib.PHI4, [dist.a, dist.beta] + bc_tail)
    return ctx, dist, args


def _time_once(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _interleaved(calls, reps, warmup):
    """calls: {name: fn}.  `warmup` untimed calls of each, then `reps` rounds that time every boundary once, in rotating order
    (no boundary always runs first or last in a round)."""
    import torch
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    names = list(calls)
    out = {n: [] for n in names}
    for r in range(reps):
        for i in range(len(names)):
            n = names[(r + i) % len(names)]
            out[n].append(_time_once(calls[n]))
    return out


def _flow_call(bc_tail, **kw):
    """(ctx, full call = reset + mala_init + flow step, init-only call, attempts-per-chain reader)"""
    import torch
    from mfm_amd import _lib
    from oracle import prng
    ctx, dist, args = _ctx(bc_tail, **kw)
    B, d, beta = 4096, 256, 0.5
    x0 = torch.as_tensor(dist.init_params.astype(np.float32)).cuda()
    pos = x0.clone(); logp = torch.empty(B, dtype=torch.float64, device="cuda"); grad = torch.empty(B, d, device="cuda")
    ns = torch.empty(B, dtype=torch.int32, device="cuda")

    def init():
        pos.copy_(x0)
        ctx.mala_init(pos, beta, logp, grad)

    def call():
        init()
        ctx.flow_step(_lib.FLOW_RWMH, prng.PRNGKey(3), beta, pos, logp, grad, nsteps=ns)
    return ctx, call, init, lambda: float(ns.float().mean())


def flow(reps, warmup, **kw):
    """flow-step times (init subtracted) and attempts per chain, boundaries interleaved"""
    made = {name: _flow_call(tail, **kw) for name, tail in BCS}
    init_t = _interleaved({n: m[2] for n, m in made.items()}, reps, warmup)
    t = _interleaved({n: m[1] for n, m in made.items()}, reps, warmup)
    res = {}
    for n, (ctx, call, init, att) in made.items():
        base = float(np.median(init_t[n]))
        res[n] = ([x - base for x in t[n]], att())
        ctx.close()
    return res


def train(reps, warmup):
    import torch
    from mfm_amd._lib import FLOW_RWMH
    from oracle import prng
    made, calls = [], {}
    for name, tail in BCS:
        ctx, dist, args = _ctx(tail)
        B, d = 4096, 256
        pos = torch.as_tensor(dist.init_params.astype(np.float32)).cuda()
        logp = torch.empty(B, dtype=torch.float64, device="cuda"); grad = torch.empty(B, d, device="cuda")
        ctx.mala_init(pos, 1.0, logp, grad)
        loss = torch.zeros(1, dtype=torch.float64, device="cuda"); grads = torch.zeros(ctx.n_params, device="cuda")
        # count = 1 with mcmc_per_flow_steps = 100: a MALA iteration (the fused MALA step + training step)
        calls[name] = (lambda c=ctx, p=pos, lp=logp, g=grad, l=loss, gs=grads:
                       c.train_iter(1, 100, FLOW_RWMH, prng.PRNGKey(4), prng.PRNGKey(5), 1.0, 1e-4, p, lp, g, l, gs))
        made.append(ctx)
    t = _interleaved(calls, reps, warmup)
    for ctx in made:
        ctx.close()
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {name: {} for name, _ in BCS}
    for n, (t, att) in flow(a.reps, a.warmup).items():
        res[n]["dopri5_ms"], res[n]["dopri5_attempts_per_chain"] = t, att
    for n, (t, _) in flow(a.reps, a.warmup, ode_method="rk4", ode_steps=16).items():
        res[n]["rk4x16_ms"] = t
    for n, t in train(a.reps, a.warmup).items():
        res[n]["train_iter_ms"] = t
    d0 = res["dirichlet-0"]
    print(f"{'boundary':12s} {'dopri5 flow step ms':>28s} {'att/chain':>9s} {'rk4x16 flow step ms':>28s} {'vs D0':>6s} {'train iter ms':>26s}")
    for name, r in res.items():
        def fmt(v):
            return f"{np.median(v):8.3f} [{min(v):.3f}..{max(v):.3f}]"
        ratio = float(np.median(np.array(r["rk4x16_ms"]) / np.array(d0["rk4x16_ms"])))      # per round (paired: same round, adjacent calls)
        tr = fmt(r["train_iter_ms"])
        print(f"{name:12s} {fmt(r['dopri5_ms']):>28s} {r['dopri5_attempts_per_chain']:9.1f} {fmt(r['rk4x16_ms']):>28s} {ratio:6.3f} {tr:>26s}")
    # the like-for-like cost of the lattice: 2-D periodic against 1-D periodic, RK4 x 16, per round
    r2 = np.array(res["2d-periodic"]["rk4x16_ms"]) / np.array(res["periodic"]["rk4x16_ms"])
    print(f"rk4x16 flow step, 2d-periodic / periodic: median {np.median(r2):.3f} [{r2.min():.3f}..{r2.max():.3f}]")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
