"""100 HMC steps two ways: 100 launches of mfm_hmc_step (a host loop over split(key, 100)) against ONE mfm_hmc_run with thin = 0
(hmc_run.hip: the chain stays in registers between the steps).  The protocol and the two shapes of tools/mala_run_time.py -- phi-four
d = 256 with 4096 chains and the 4-mode mixture d = 2 with 512 chains -- each with L = 3 and L = 10 leapfrog steps per HMC step.

Per shape and L the same initial state and key serve three calls -- the launches, the launches AGAIN, the run -- after `--warmup` untimed
calls of each; `--reps` rounds time every call once, in rotating order, with HIP events on the default stream after a synchronisation
(the state reset is outside the timed window).  Printed: the median and min..max of each, the spread of the baseline against itself (the
second series of launches over the first, per round) next to run / launches per round -- a difference inside that spread is no
difference -- and a check that both ways end in the same bits.  `--out` keeps a copy of the table.

    python tools/hmc_run_time.py [--reps 20] [--warmup 3] [--steps 100] [--out profiles/hmc_run_time.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

SHAPES = [("phi-four d=256, 4096 chains", "phi4", 256, 4096, 0.02), ("4-mode d=2, 512 chains", "gmm", 2, 512, 1.0)]
LEAPFROG = (3, 10)


def _time_once(reset, fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reset()
    torch.cuda.synchronize()
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def shape(kind, d, B, eps, L, n_steps, reps, warmup):
    import torch
    from mfm_amd import random as jr
    from tests import gpu_util as gu
    if kind == "phi4":
        args, dist, k, model, state = gu.phi4_setup(d=d, B=B, hidden=32, F=16)
    else:
        args, dist, k, model, state = gu.gmm4_setup(B=B)
    ctx = gu.make_ctx(dist, args)
    x0 = torch.as_tensor(dist.init_params.astype(np.float32)).cuda()
    pos = x0.clone(); logp = torch.empty(B, dtype=torch.float64, device="cuda"); grad = torch.empty(B, d, device="cuda")
    ctx.mala_init(pos, 1.0, logp, grad)
    lp0, g0 = logp.clone(), grad.clone()
    n_acc = torch.empty(B, dtype=torch.int32, device="cuda")
    key = jr.PRNGKey(2)
    step_keys = [(int(a), int(b)) for a, b in jr.split(key, n_steps)]      # (the host-side key split is not part of either timing)

    def reset():
        pos.copy_(x0); logp.copy_(lp0); grad.copy_(g0)

    def launches():
        for sk in step_keys:
            ctx.hmc_step(sk, 1.0, eps, L, pos, logp, grad)

    def run():
        ctx.hmc_run(key, 1.0, eps, L, n_steps, pos, logp, grad, n_acc=n_acc)

    calls = {"launches": launches, "launches again": launches, "run": run}
    ends = {}
    for name, fn in calls.items():
        for _ in range(warmup):
            reset(); fn()
        torch.cuda.synchronize()
        ends[name] = (pos.clone(), logp.clone(), grad.clone())
    same = all(torch.equal(a, b) for a, b in zip(ends["launches"], ends["run"]))
    names = list(calls)
    t = {n: [] for n in names}
    for r in range(reps):
        for i in range(len(names)):
            n = names[(r + i) % len(names)]
            t[n].append(_time_once(reset, calls[n]))
    acc = float(n_acc.float().mean()) / n_steps
    ctx.close()
    return {n: np.array(v) for n, v in t.items()}, same, acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"{a.steps} HMC steps: {a.steps} launches of mfm_hmc_step vs one mfm_hmc_run (thin = 0); {a.reps} rounds after {a.warmup} warm-up calls; ms, median [min..max]"]
    def fmt(v):
        return f"{np.median(v):8.3f} [{v.min():.3f}..{v.max():.3f}]"
    for title, kind, d, B, eps in SHAPES:
        for L in LEAPFROG:
            t, same, acc = shape(kind, d, B, eps, L, a.steps, a.reps, a.warmup)
            self_ratio = t["launches again"] / t["launches"]
            run_ratio = t["run"] / t["launches"]
            lines += [f"{title}, L = {L} (step size {eps:g}, accepted fraction {acc:.2f}, same bits both ways: {same})",
                      f"  launches        {fmt(t['launches'])}",
                      f"  launches again  {fmt(t['launches again'])}   / launches per round: {fmt(self_ratio)}   <- the baseline's own spread",
                      f"  one run         {fmt(t['run'])}   / launches per round: {fmt(run_ratio)}",
                      f"  per step: launches {1e3 * np.median(t['launches']) / a.steps:.2f} us, run {1e3 * np.median(t['run']) / a.steps:.2f} us"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
