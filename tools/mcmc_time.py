"""100 steps of the Cox process and HMC sampler kernels, for comparing two builds of the library (one process per build: `--lib`).

Calls: 100 `mfm_mala_step` launches on the Cox process 16 x 16 grid with 1024 chains, on the tile family (`mala_lgcp_kernel`) and on the
wide family (`lgcp_propose_kernel` / `lgcp_accept_kernel`); one `mfm_mala_run` of 100 steps on the tile family (adds `mala_run_keys_kernel`);
100 `mfm_hmc_step` launches (3 leapfrog steps) on phi-four d = 256 with 4096 chains.  As tools/mala_run_time.py: the same initial state
and keys every time, `--warmup` untimed calls, `--reps` rounds with HIP events in rotating order, every call timed TWICE per round so
that its own round-to-round spread (again / first) stands next to its median.

    python tools/mcmc_time.py [--lib PATH/libmfm_hip.so] [--reps 20] [--warmup 3] [--steps 100] [--out FILE]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.lib:
        os.environ["MFM_LIB"] = os.path.abspath(a.lib)
    import numpy as np
    import torch
    from mfm_amd import _lib, random as jr
    from tests import gpu_util as gu
    from tools.mala_run_time import _time_once

    step_keys = [(int(k0), int(k1)) for k0, k1 in jr.split(jr.PRNGKey(2), a.steps)]
    calls, resets, closers = {}, {}, []

    def state(ctx, dist, beta):
        x0 = torch.as_tensor(dist.init_params.astype(np.float32)).cuda()
        pos = x0.clone(); logp = torch.empty(x0.shape[0], dtype=torch.float64, device="cuda"); grad = torch.empty_like(x0)
        ctx.mala_init(pos, beta, logp, grad)
        lp0, g0 = logp.clone(), grad.clone()
        return pos, logp, grad, lambda: (pos.copy_(x0), logp.copy_(lp0), grad.copy_(g0))

    for fam, name in ((_lib.FAMILY_TILE, "cox tile"), (_lib.FAMILY_WIDE, "cox wide")):
        args, dist, *_ = gu.lgcp_setup(n=16, B=1024)
        ctx = gu.make_ctx(dist, args, family=fam); closers.append(ctx)
        pos, logp, grad, reset = state(ctx, dist, 0.5)
        calls[name + " steps"] = lambda c=ctx, p=pos, l=logp, g=grad: [c.mala_step(k, 0.5, 0.02, p, l, g) for k in step_keys]
        resets[name + " steps"] = reset
        if fam == _lib.FAMILY_TILE:
            calls["cox tile run"] = lambda c=ctx, p=pos, l=logp, g=grad: c.mala_run(jr.PRNGKey(2), 0.5, 0.02, a.steps, p, l, g)
            resets["cox tile run"] = reset
    args, dist, *_ = gu.phi4_setup(d=256, B=4096, hidden=32, F=16)
    ctx = gu.make_ctx(dist, args); closers.append(ctx)
    pos, logp, grad, reset = state(ctx, dist, 1.0)
    calls["hmc steps"] = lambda c=ctx, p=pos, l=logp, g=grad: [c.hmc_step(k, 1.0, 1e-3, 3, p, l, g) for k in step_keys]
    resets["hmc steps"] = reset

    series = [(n, rep) for n in calls for rep in ("", " again")]
    for n in calls:
        for _ in range(a.warmup):
            resets[n](); calls[n]()
    torch.cuda.synchronize()
    t = {n + rep: [] for n, rep in series}
    for r in range(a.reps):
        for i in range(len(series)):
            n, rep = series[(r + i) % len(series)]
            t[n + rep].append(_time_once(resets[n], calls[n]))
    lines = [f"{a.steps} steps per call; {a.reps} rounds after {a.warmup} warm-up calls; ms, median [min..max]; library: {a.lib or 'in-tree'}"]
    for n in calls:
        v, w = np.array(t[n]), np.array(t[n + " again"])
        ratio = w / v
        lines.append(f"  {n:<16} {np.median(v):8.3f} [{v.min():.3f}..{v.max():.3f}]   again {np.median(w):8.3f}   again / first per round: "
                     f"{np.median(ratio):.3f} [{ratio.min():.3f}..{ratio.max():.3f}]")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    for c in closers:
        c.close()


if __name__ == "__main__":
    main()
