"""The NUTS warmup: one mfm_nuts_warmup launch against one mfm_nuts_run launch, and what adapting on the tree buys.

Per shape (phi-four d = 64 and d = 256, 4096 chains, unit mass, from the initial draw): ONE mfm_nuts_warmup of `--steps` transitions from
the step size of tools/nuts_time.py is timed `--reps` times with HIP events, and so is ONE mfm_nuts_run of `--steps` transitions from the
same state at the warmup's pooled step size.  Early warmup transitions at small step sizes build full-depth trees and a launch ends with
its slowest wave, so the ratio is reported, not bounded.  Printed: ms per call (median [min..max]), the mean leapfrog count per
transition of both, the pooled step size, the ratio.

`--ess N`: the reason for the feature -- two runs of the phi-four default (d = 64, 1024 chains, `--step_size 1e-4`; `--learning_iter`
as given here) with `--mcmc_kernel nuts --adapt_steps --ess_steps N`, one under `--nuts_adapt hmc` (the HMC warmup at `--hmc_steps`
10) and one under `--nuts_adapt tree`: adapted step size, warmup acceptance, and `ess_per_step_*` / `ess_per_grad_*`.  `--out` keeps a copy.

    python tools/nuts_warmup_time.py [--reps 3] [--steps 100] [--depth 10] [--ess 400] [--adapt_steps 200] [--learning_iter 100] [--out profiles/nuts_warmup_time.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tools.nuts_time import SHAPES, _timed  # noqa: E402


def shape(d, B, eps, depth, n_steps, reps):
    import torch
    from mfm_amd import mcmc_utils, random as jr
    from tests import gpu_util as gu
    args, dist, *_ = gu.phi4_setup(d=d, B=B, hidden=32, F=16)
    ctx = gu.make_ctx(dist, args)
    pos = torch.as_tensor(dist.init_params.astype(np.float32)).cuda()
    logp = torch.empty(B, dtype=torch.float64, device="cuda"); grad = torch.empty(B, d, device="cuda")
    ctx.mala_init(pos, 1.0, logp, grad)
    torch.cuda.synchronize()
    s0 = (pos.clone(), logp.clone(), grad.clone())
    leap = torch.empty(B, dtype=torch.int64, device="cuda"); asum = torch.empty(B, dtype=torch.float64, device="cuda")
    avg = torch.empty(B, dtype=torch.float64, device="cuda")
    key = jr.PRNGKey(2)

    def reset():
        for t, s in zip((pos, logp, grad), s0):
            t.copy_(s)

    def warmup():
        ctx.nuts_warmup(key, 1.0, eps, depth, n_steps, 0.8, pos, logp, grad, avg, acc_sum=asum, leapfrog_sum=leap)

    reset(); warmup(); torch.cuda.synchronize()
    pooled = mcmc_utils.pooled_step_size(avg, B)
    w_stats = (leap.double().mean().item() / n_steps, asum.mean().item() / n_steps, avg.min().item(), avg.max().item())
    t_w = _timed(warmup, reset, reps)

    def run():
        ctx.nuts_run(key, 1.0, pooled, depth, n_steps, pos, logp, grad, leapfrog_sum=leap, acc_sum=asum)

    reset(); run(); torch.cuda.synchronize()
    r_stats = (leap.double().mean().item() / n_steps, asum.mean().item() / n_steps)
    t_r = _timed(run, reset, reps)
    ctx.close()
    return pooled, w_stats, r_stats, t_w, t_r


def ess_runs(n_ess, adapt_steps, learning_iter, depth):
    from mfm_amd import distributions as D, exe_flow_matching as E
    from oracle import loop
    out = []
    for mode in ("hmc", "tree"):
        args = loop.default_args(example="phi-four", dim=64, num_chain=1024, eval_iter=1, step_size=1e-4, seed=1, learning_iter=learning_iter,
                                 mcmc_kernel="nuts", max_tree_depth=depth, adapt_steps=adapt_steps, adapt_target=0.8, nuts_adapt=mode,
                                 ess_steps=n_ess)
        _, _, ex = E.run(D.PhiFour(64), args, None, log_every=1000, return_extras=True)
        out.append((mode, {k: v for k, v in ex.items() if isinstance(v, (int, float)) and (k.startswith(("ess_per", "adapt", "nuts_")) or k == "rhat_max")}))
        ex["engine"].close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--ess", type=int, default=0)
    ap.add_argument("--adapt_steps", type=int, default=200)
    ap.add_argument("--learning_iter", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fmt = lambda v: f"{np.median(v):9.3f} [{v.min():.3f}..{v.max():.3f}]"
    lines = [f"mfm_nuts_warmup vs mfm_nuts_run: {a.steps} transitions from the initial draw, max_tree_depth {a.depth}, target 0.8, {a.reps} timed calls each; ms, median [min..max]"]
    for title, d, B, eps in SHAPES:
        pooled, ws, rs, tw, tr = shape(d, B, eps, a.depth, a.steps, a.reps)
        lines += [f"{title}, step0 {eps:g}",
                  f"  mfm_nuts_warmup                    {fmt(tw)}   mean leapfrog steps {ws[0]:.1f}, mean acceptance statistic {ws[1]:.3f}, per-chain step sizes {ws[2]:.5f} .. {ws[3]:.5f}, pooled {pooled:.5f}",
                  f"  mfm_nuts_run at the pooled {pooled:.5f} {fmt(tr)}   mean leapfrog steps {rs[0]:.1f}, mean acceptance statistic {rs[1]:.3f}",
                  f"  warmup / run: {np.median(tw) / np.median(tr):.2f} in time, {ws[0] / rs[0]:.2f} in mean leapfrog steps"]
    if a.ess > 0:
        lines.append(f"phi-four default (d = 64, 1024 chains, --step_size 1e-4), --mcmc_kernel nuts --max_tree_depth {a.depth} --adapt_steps {a.adapt_steps} "
                     f"--ess_steps {a.ess}, --learning_iter {a.learning_iter}:")
        for mode, st in ess_runs(a.ess, a.adapt_steps, a.learning_iter, a.depth):
            lines.append(f"  --nuts_adapt {mode}: " + ", ".join(f"{k} {v:.5g}" for k, v in sorted(st.items())))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
