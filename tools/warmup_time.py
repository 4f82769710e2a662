"""The step-size warmup against the run it is built on: ONE mfm_hmc_warmup against ONE mfm_hmc_run (thin = 0) of the same number of
steps, and the same for MALA under the textbook rule (warmup.hip against hmc_run.hip / mala_run.hip).  Shape: phi-four d = 256 with
4096 chains, L = 10 leapfrog steps per HMC step.  The warmup's extra work per step is a handful of wave-uniform float64 operations and
two out-of-line calls (exp; the draws are the run's), against L gradient evaluations.

The protocol of tools/hmc_run_time.py: the same initial state and key serve three calls -- the run, the run AGAIN, the warmup -- after
`--warmup` untimed calls of each; `--reps` rounds time every call once, in rotating order, with HIP events on the default stream after a
synchronisation (the state reset is outside the timed window).  Printed: the median and min..max of each, and the spread of the baseline
against itself next to warmup / run per round -- a difference inside that spread is no difference.  `--out` keeps a copy of the table.

    python tools/warmup_time.py [--reps 20] [--warmup 3] [--steps 100] [--out profiles/warmup_time.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tools.hmc_run_time import _time_once  # noqa: E402

D, B, L = 256, 4096, 10
STEP0 = {"hmc": 0.02, "mala": 3e-4}
TARGET = {"hmc": 0.8, "mala": 0.574}


def sampler(which, n_steps, reps, warmup):
    import torch
    from mfm_amd import random as jr
    from tests import gpu_util as gu
    args, dist, k, model, state = gu.phi4_setup(d=D, B=B, hidden=32, F=16)
    ctx = gu.make_ctx(dist, args)
    x0 = torch.as_tensor(dist.init_params.astype(np.float32)).cuda()
    pos = x0.clone(); logp = torch.empty(B, dtype=torch.float64, device="cuda"); grad = torch.empty(B, D, device="cuda")
    ctx.mala_init(pos, 1.0, logp, grad)
    lp0, g0 = logp.clone(), grad.clone()
    n_acc = torch.empty(B, dtype=torch.int32, device="cuda")
    acc_sum = torch.empty(B, dtype=torch.float64, device="cuda")
    avg = torch.empty(B, dtype=torch.float64, device="cuda")
    key, eps = jr.PRNGKey(2), STEP0[which]

    def reset():
        pos.copy_(x0); logp.copy_(lp0); grad.copy_(g0)

    if which == "hmc":
        run = lambda: ctx.hmc_run(key, 1.0, eps, L, n_steps, pos, logp, grad, n_acc=n_acc, acc_sum=acc_sum)
        adapt = lambda: ctx.hmc_warmup(key, 1.0, eps, L, n_steps, TARGET[which], pos, logp, grad, avg, n_acc=n_acc, acc_sum=acc_sum)
    else:
        run = lambda: ctx.mala_run(key, 1.0, eps, n_steps, pos, logp, grad, n_acc=n_acc, acc_sum=acc_sum, textbook=True)
        adapt = lambda: ctx.mala_warmup(key, 1.0, eps, n_steps, TARGET[which], pos, logp, grad, avg, n_acc=n_acc, acc_sum=acc_sum)
    calls = {"run": run, "run again": run, "warmup": adapt}
    acc = {}
    for name, fn in calls.items():
        for _ in range(warmup):
            reset(); fn()
        torch.cuda.synchronize()
        acc[name] = float(acc_sum.mean()) / n_steps
    pooled = float(avg.log().mean().exp())
    names = list(calls)
    t = {n: [] for n in names}
    for r in range(reps):
        for i in range(len(names)):
            n = names[(r + i) % len(names)]
            t[n].append(_time_once(reset, calls[n]))
    ctx.close()
    return {n: np.array(v) for n, v in t.items()}, acc, pooled


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"{a.steps} steps, phi-four d = {D}, {B} chains: one warmup (dual averaging per chain) vs one run (thin = 0); {a.reps} rounds after {a.warmup} warm-up calls; ms, median [min..max]"]

    def fmt(v):
        return f"{np.median(v):8.3f} [{v.min():.3f}..{v.max():.3f}]"
    for which, title in (("hmc", f"HMC, L = {L}: mfm_hmc_warmup vs mfm_hmc_run"), ("mala", "MALA, textbook rule: mfm_mala_warmup vs mfm_mala_run")):
        t, acc, pooled = sampler(which, a.steps, a.reps, a.warmup)
        lines += [f"{title} (from step size {STEP0[which]:g}: mean acceptance probability {acc['run']:.3f} in the run, {acc['warmup']:.3f} over the warmup towards "
                  f"{TARGET[which]}; pooled adapted step size {pooled:.4g})",
                  f"  run        {fmt(t['run'])}",
                  f"  run again  {fmt(t['run again'])}   / run per round: {fmt(t['run again'] / t['run'])}   <- the baseline's own spread",
                  f"  warmup     {fmt(t['warmup'])}   / run per round: {fmt(t['warmup'] / t['run'])}"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
