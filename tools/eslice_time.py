"""Elliptical slice sampling of the Cox process (mfm_eslice_run) next to the MALA tile step on the same context.

Per shape (d = 1024 and d = 1600; 64 and 1024 chains), from prior draws after `--burn` transitions:

* one mfm_eslice_run of `--steps` transitions at beta = 1 and at beta = 0 (a single evaluation per transition: the draw of nu, the
  L^T GEMM and one likelihood pass), and `--steps` launches of mfm_mala_step at `--step_size`, each timed `--reps` times with HIP
  events around the call: us per transition / step (median);
* the cost of one shrink evaluation: the launch ends with its slowest tile, and a tile makes as many passes through the shrink loop as
  its slowest row needs, so the slope is (t(beta = 1) - t(beta = 0)) over (the largest per-tile sum of the transitions' maxima of
  subiter over the tile's 16 rows, minus one per transition), counted from `--steps` single-step launches on the same keys;
* at 64 chains: the multi-chain effective sample size (diagnostics.chain_diagnostics, min and median over the coordinates) of `--ess_steps`
  kept transitions, per transition, per likelihood evaluation and per second, next to mfm_mala_run under the textbook rule at
  `--step_size` (the rule as the reference writes it is not a Metropolis rule, so its ESS says nothing).

    python tools/eslice_time.py [--reps 5] [--steps 20] [--ess_steps 200] [--burn 50] [--step_size 0.01] [--out profiles/eslice_time.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

GRIDS = (32, 40)
CHAINS = (64, 1024)


def _timed(fn, reset, reps):
    import torch
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reset()
        torch.cuda.synchronize()
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out))


def shape(n, B, a):
    import torch
    from mfm_amd import _lib, diagnostics, random as jr
    from oracle import loop, prng
    from tests import eslice_cases as ec, gpu_util as gu
    d = n * n
    dist = ec.dist_of(n)
    args = loop.default_args(example="pines", dim=d, num_chain=B, hutchs=True, step_size=a.step_size, seed=1, fourier_dim=16, **gu.hidden_lists(32))
    try:
        ctx = gu.make_ctx(dist, args)
    except _lib.MfmError:
        ctx = gu.make_ctx(dist, args, family=_lib.FAMILY_WIDE)
    ctx.set_lgcp_chol(dist.chol)
    xi = prng.normal_rows(prng.split(prng.PRNGKey(5), B), d)
    pos = torch.as_tensor((dist.mu + xi @ dist.chol.T).astype(np.float32)).cuda()
    ll = torch.empty(B, dtype=torch.float64, device="cuda")
    ctx.eslice_init(pos, ll)
    ctx.eslice_run(jr.PRNGKey(6), 1.0, a.burn, pos, ll)
    torch.cuda.synchronize()
    x0, ll0 = pos.clone(), ll.clone()
    logp = torch.empty(B, dtype=torch.float64, device="cuda"); grad = torch.empty(B, d, device="cuda")
    ctx.mala_init(pos, 1.0, logp, grad)
    lp0, g0 = logp.clone(), grad.clone()
    key = jr.PRNGKey(7)
    step_keys = [(int(p), int(q)) for p, q in jr.split(key, a.steps)]

    def reset():
        pos.copy_(x0); ll.copy_(ll0); logp.copy_(lp0); grad.copy_(g0)

    sub_sum = torch.empty(B, dtype=torch.int32, device="cuda")
    t1 = _timed(lambda: ctx.eslice_run(key, 1.0, a.steps, pos, ll, subiter_sum=sub_sum), reset, a.reps)
    mean_sub = sub_sum.double().mean().item() / a.steps
    t0 = _timed(lambda: ctx.eslice_run(key, 0.0, a.steps, pos, ll), reset, a.reps)
    tm = _timed(lambda: [ctx.mala_step(sk, 1.0, a.step_size, pos, logp, grad) for sk in step_keys], reset, a.reps)
    # passes of the slowest tile through the shrink loop (single steps on the run's keys: the same bits)
    reset()
    sub = torch.empty(B, dtype=torch.int32, device="cuda")
    trips = torch.zeros(B // 16, dtype=torch.int64, device="cuda")
    for sk in step_keys:
        ctx.eslice_step(sk, 1.0, pos, ll, sub)
        trips += sub.view(B // 16, 16).max(dim=1).values
    crit = trips.max().item()
    slope = (t1 - t0) * 1e3 / max(crit - a.steps, 1)
    line = (f"{n}x{n} d={d} B={B}: eslice {t1 * 1e3 / a.steps:8.1f} us/transition at beta 1 ({mean_sub:.2f} evaluations per chain, "
            f"{crit / a.steps:.2f} passes of the slowest tile), {t0 * 1e3 / a.steps:8.1f} us at beta 0 (one pass); "
            f"shrink evaluation {slope:6.2f} us; mala_step {tm * 1e3 / a.steps:8.1f} us/step")
    ess_line = None
    if B == CHAINS[0] and a.ess_steps > 0:
        m = a.ess_steps
        traj = torch.empty(m, B, d, device="cuda")
        reset()
        te = _timed(lambda: ctx.eslice_run(key, 1.0, m, pos, ll, thin=1, subiter_sum=sub_sum, traj_pos=traj), reset, 1)
        evals = sub_sum.double().mean().item() / m
        es = diagnostics.chain_diagnostics(traj, ctx=ctx).ess.double() / (B * m)
        n_acc = torch.empty(B, dtype=torch.int32, device="cuda")
        tml = _timed(lambda: ctx.mala_run(key, 1.0, a.step_size, m, pos, logp, grad, thin=1, n_acc=n_acc, traj_pos=traj, textbook=True), reset, 1)
        ml = diagnostics.chain_diagnostics(traj, ctx=ctx).ess.double() / (B * m)
        ess_line = (f"    ESS per transition and chain (min, median): eslice {es.min().item():.4g}, {es.median().item():.4g}"
                    f" (per evaluation {es.min().item() / evals:.4g}, {es.median().item() / evals:.4g}; per second of {B} chains "
                    f"{es.min().item() * B * m / (te * 1e-3):.4g}, {es.median().item() * B * m / (te * 1e-3):.4g});"
                    f" mala step {a.step_size} textbook {ml.min().item():.4g}, {ml.median().item():.4g}"
                    f" (acceptance {n_acc.double().mean().item() / m:.3f}; per second {ml.min().item() * B * m / (tml * 1e-3):.4g}, "
                    f"{ml.median().item() * B * m / (tml * 1e-3):.4g})")
    ctx.close()
    return [line] + ([ess_line] if ess_line else [])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--ess_steps", type=int, default=200)
    ap.add_argument("--burn", type=int, default=50)
    ap.add_argument("--step_size", type=float, default=0.01)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    lines = []
    for n in GRIDS:
        for B in CHAINS:
            for ln in shape(n, B, a):
                print(ln, flush=True)
                lines.append(ln)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
