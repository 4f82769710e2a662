"""The No-U-turn run against fixed-length HMC at the same step size: time per leapfrog step and effective sample size per gradient.

Per shape (phi-four d = 64 and d = 256, 4096 chains, unit mass): the chains are burnt in by `--burn` NUTS transitions, then ONE
mfm_nuts_run of `--steps` transitions (thin = 1) is timed `--reps` times from that state with HIP events, and so is ONE mfm_hmc_run of
`--steps` steps with L = the NUTS run's mean leapfrog count per transition, rounded -- the fixed trajectory length nearest to what NUTS
chose.  hmc_run.hip is not touched by nuts.hip, so its figure is the parent's.  Printed: the tree statistics, ms per call (median
[min..max]), the time per leapfrog step of all chains (call time over leapfrog steps per chain), their ratio, and Geyer's ESS per
gradient (min / median over chains and coordinates, mcmc_utils.effective_sample_size over steps x leapfrog steps per step) of both
trajectories; and what the LDS budget leaves at the depth used.  `--out` keeps a copy.

    python tools/nuts_time.py [--reps 5] [--steps 200] [--burn 100] [--depth 10] [--out profiles/nuts_time.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

SHAPES = [("phi-four d=64, 4096 chains", 64, 4096, 0.03), ("phi-four d=256, 4096 chains", 256, 4096, 0.02)]


def lds_budget(d, depth):
    """(chains per workgroup, workgroups per CU, LDS bytes per workgroup): the library's own answer (mfm_nuts_launch_plan)."""
    from mfm_amd import _lib
    w, sm, per_cu = _lib.nuts_launch_plan(d, depth)
    return w, per_cu, sm


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
    return np.array(out)


def shape(d, B, eps, depth, n_steps, burn, reps):
    import torch
    from mfm_amd import mcmc_utils, random as jr
    from tests import gpu_util as gu
    args, dist, *_ = gu.phi4_setup(d=d, B=B, hidden=32, F=16)
    ctx = gu.make_ctx(dist, args)
    pos = torch.as_tensor(dist.init_params.astype(np.float32)).cuda()
    logp = torch.empty(B, dtype=torch.float64, device="cuda"); grad = torch.empty(B, d, device="cuda")
    ctx.mala_init(pos, 1.0, logp, grad)
    ctx.nuts_run(jr.PRNGKey(1), 1.0, eps, depth, burn, pos, logp, grad)
    torch.cuda.synchronize()
    s0 = (pos.clone(), logp.clone(), grad.clone())
    leap = torch.empty(B, dtype=torch.int64, device="cuda"); dsum = torch.empty(B, dtype=torch.int32, device="cuda")
    ndiv = torch.empty(B, dtype=torch.int32, device="cuda"); asum = torch.empty(B, dtype=torch.float64, device="cuda")
    traj = torch.empty(n_steps, B, d, device="cuda")
    key = jr.PRNGKey(2)

    def reset():
        for t, s in zip((pos, logp, grad), s0):
            t.copy_(s)

    def nuts():
        ctx.nuts_run(key, 1.0, eps, depth, n_steps, pos, logp, grad, thin=1, leapfrog_sum=leap, acc_sum=asum, n_divergent=ndiv, depth_sum=dsum, traj_pos=traj)

    reset(); nuts(); torch.cuda.synchronize()
    mean_leap = leap.double().mean().item() / n_steps
    stats = dict(mean_leap=mean_leap, mean_depth=dsum.double().mean().item() / n_steps, divergent=int(ndiv.sum().item()), acc=asum.mean().item() / n_steps)
    ess_n = (mcmc_utils.effective_sample_size(traj, ctx=ctx)[0].double() / (n_steps * mean_leap)).reshape(-1)
    t_nuts = _timed(nuts, reset, reps)
    L = max(1, int(round(mean_leap)))

    def hmc():
        ctx.hmc_run(key, 1.0, eps, L, n_steps, pos, logp, grad, thin=1, traj_pos=traj)

    reset(); hmc(); torch.cuda.synchronize()
    ess_h = (mcmc_utils.effective_sample_size(traj, ctx=ctx)[0].double() / (n_steps * L)).reshape(-1)
    t_hmc = _timed(hmc, reset, reps)
    ctx.close()
    q = lambda e: (e.min().item(), e.median().item())
    return stats, L, t_nuts, t_hmc, q(ess_n), q(ess_h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--burn", type=int, default=100)
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fmt = lambda v: f"{np.median(v):9.3f} [{v.min():.3f}..{v.max():.3f}]"
    lines = [f"mfm_nuts_run vs mfm_hmc_run: {a.steps} transitions after {a.burn} burn-in transitions, max_tree_depth {a.depth}, {a.reps} timed calls each; ms, median [min..max]"]
    for title, d, B, eps in SHAPES:
        st, L, tn, th, en, eh = shape(d, B, eps, a.depth, a.steps, a.burn, a.reps)
        w, per_cu, sm = lds_budget(d, a.depth)
        us_n = 1e3 * np.median(tn) / (a.steps * st["mean_leap"]); us_h = 1e3 * np.median(th) / (a.steps * L)
        lines += [f"{title}, step size {eps:g}",
                  f"  LDS budget at depth {a.depth}: {w} chains per workgroup, {sm} B per workgroup, {per_cu} workgroups = {w * per_cu} waves per CU ({w * per_cu / 4:.2f} per SIMD)",
                  f"  NUTS trees: mean depth {st['mean_depth']:.2f}, mean leapfrog steps {st['mean_leap']:.1f}, mean acceptance rate {st['acc']:.3f}, divergent transitions {st['divergent']}",
                  f"  mfm_nuts_run            {fmt(tn)}   {us_n:.3f} us per leapfrog step of all chains",
                  f"  mfm_hmc_run, L = {L:<4d}  {fmt(th)}   {us_h:.3f} us per leapfrog step of all chains   NUTS / HMC per leapfrog: {us_n / us_h:.2f}",
                  f"  ESS per gradient (min, median): NUTS {en[0]:.4g}, {en[1]:.4g}; HMC L = {L}: {eh[0]:.4g}, {eh[1]:.4g}"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
