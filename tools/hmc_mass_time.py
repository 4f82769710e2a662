"""What the mass instances of the HMC kernels cost (hmc.hip: MASS; mfm_hmc_set_inverse_mass): 100 HMC steps of phi-four d = 256 with
4096 chains, L = 3 and L = 10 leapfrog steps, under unit mass (the unit instances) and with a vector of ONES installed (the mass
instances: the same bits, hence the same accepted fraction and the same work apart from the instances' own instructions).

The protocol of tools/hmc_run_time.py: per L the same initial state and key serve every call -- 100 launches of mfm_hmc_step, one
mfm_hmc_run with thin = 0, one mfm_hmc_warmup, each under unit mass, under unit mass AGAIN (the baseline's own spread) and on the mass
instance, and one mfm_hmc_warmup_window (the mass instance with the sums) -- after `--warmup` untimed calls of each; `--reps` rounds
time every call once, in rotating order, with HIP events on the default stream after a synchronisation (the state reset and the
installation of the mass are outside the timed window).  Printed: median and min..max of each, and per round again / unit next to mass /
unit.  `--out` keeps a copy of the table.

    python tools/hmc_mass_time.py [--reps 20] [--warmup 3] [--steps 100] [--out profiles/hmc_mass_time.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

D, B, EPS = 256, 4096, 0.02
LEAPFROG = (3, 10)


def _time_once(reset, fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reset()
    torch.cuda.synchronize()
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def shape(L, n_steps, reps, warmup):
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
    avg = torch.empty(B, dtype=torch.float64, device="cuda")
    s, q = torch.empty(B, D, dtype=torch.float64, device="cuda"), torch.empty(B, D, dtype=torch.float64, device="cuda")
    key = jr.PRNGKey(2)
    step_keys = [(int(a), int(b)) for a, b in jr.split(key, n_steps)]
    ones = np.ones(D)

    def reset_for(mass):
        def reset():
            ctx.set_inverse_mass(ones if mass else None)      # (no call when nothing changes)
            pos.copy_(x0); logp.copy_(lp0); grad.copy_(g0)
        return reset

    def launches():
        for sk in step_keys:
            ctx.hmc_step(sk, 1.0, EPS, L, pos, logp, grad)

    def run():
        ctx.hmc_run(key, 1.0, EPS, L, n_steps, pos, logp, grad, n_acc=n_acc)

    def warm():
        ctx.hmc_warmup(key, 1.0, EPS, L, n_steps, 0.8, pos, logp, grad, avg)

    def window():
        ctx.hmc_warmup_window(key, 1.0, EPS, L, n_steps, 0.8, pos, logp, grad, avg, s, q)

    calls = {}
    for name, fn in (("launches", launches), ("run", run), ("warmup", warm)):
        calls[name + " unit"] = (reset_for(False), fn)
        calls[name + " unit again"] = (reset_for(False), fn)
        calls[name + " mass"] = (reset_for(True), fn)
    calls["window mass"] = (reset_for(True), window)
    ends = {}
    for name, (reset, fn) in calls.items():
        for _ in range(warmup):
            reset(); fn()
        torch.cuda.synchronize()
        ends[name] = (pos.clone(), logp.clone(), grad.clone())
    same = all(torch.equal(a, b) for kind in ("launches", "run", "warmup") for a, b in zip(ends[kind + " unit"], ends[kind + " mass"]))
    same = same and all(torch.equal(a, b) for a, b in zip(ends["warmup unit"], ends["window mass"]))
    names = list(calls)
    t = {n: [] for n in names}
    for r in range(reps):
        for i in range(len(names)):
            n = names[(r + i) % len(names)]
            t[n].append(_time_once(*calls[n]))
    reset_for(False)()
    run()
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
    lines = [f"{a.steps} HMC steps of phi-four d = {D}, {B} chains, unit instances vs mass instances on a vector of ones; {a.reps} rounds after "
             f"{a.warmup} warm-up calls; ms, median [min..max]"]

    def fmt(v):
        return f"{np.median(v):8.3f} [{v.min():.3f}..{v.max():.3f}]"
    for L in LEAPFROG:
        t, same, acc = shape(L, a.steps, a.reps, a.warmup)
        lines.append(f"L = {L} (step size {EPS:g}, accepted fraction {acc:.2f}, same bits under unit mass and under ones: {same})")
        for kind in ("launches", "run", "warmup"):
            u, again, m = t[kind + " unit"], t[kind + " unit again"], t[kind + " mass"]
            lines += [f"  {kind:9s} unit  {fmt(u)}   again / unit per round: {fmt(again / u)}   <- the baseline's own spread",
                      f"  {kind:9s} mass  {fmt(m)}   mass / unit per round:  {fmt(m / u)}   per step: unit {1e3 * np.median(u) / a.steps:.2f} us, mass {1e3 * np.median(m) / a.steps:.2f} us"]
        w = t["window mass"]
        lines.append(f"  window    mass  {fmt(w)}   window / warmup unit per round: {fmt(w / t['warmup unit'])}   per step: {1e3 * np.median(w) / a.steps:.2f} us")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
