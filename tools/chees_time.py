"""ChEES-HMC against the project's other ways of choosing an HMC trajectory: wall time of the warmup, and effective sample size per
gradient and per second of the sampler each warmup leads to.

Per shape (phi-four d = 256 and d = 64, the 4-mode mixture; 1024 and 4096 chains; unit mass; beta = 1), from the same start state:

* mfm_chees_warmup of `--iters` iterations, timed `--reps` times with HIP events around the call (h_result is not asked for, so the
  call only enqueues): ms per call, us per iteration, us per leapfrog step of all chains (call time over the sum of the recorded
  L_t); next to it mfm_hmc_warmup of `--iters` steps at L = the ChEES run's mean leapfrog count, rounded: the per-chain warmup at the
  same work;
* from the state the ChEES warmup leaves: mfm_hmc_run_lengths of `--steps` steps under the adapted (eps, T), thin = 1: ms per call and
  Geyer's ESS (min / median over chains and coordinates, mcmc_utils.effective_sample_size) per gradient evaluation and per second;
* the same for mfm_hmc_run at L = 10 under the pooled step size of mfm_hmc_warmup (`--iters` steps, target 0.8): the CLI's
  `--mcmc_kernel hmc --hmc_steps 10 --adapt_steps N`;
* the same for mfm_nuts_run under the pooled step size of mfm_nuts_warmup (`--iters` transitions, target 0.8, `--depth`): `--nuts_adapt
  tree`.

    python tools/chees_time.py [--reps 5] [--iters 200] [--steps 200] [--depth 10] [--out profiles/chees_time.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

# title, target, d, first step size
SHAPES = [("phi-four d=256", "phi4", 256, 0.01), ("phi-four d=64", "phi4", 64, 0.02), ("4-mode mixture d=2", "gmm4", 2, 0.2)]
CHAINS = (1024, 4096)


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


def shape(kind, d, B, eps0, iters, n_steps, depth, reps):
    import torch
    from mfm_amd import mcmc_utils, random as jr
    from mfm_amd.bblackjax.adaptation.chees_adaptation import integration_steps
    from tests import gpu_util as gu
    if kind == "gmm4":
        args, dist, *_ = gu.gmm4_setup(B=B)
    else:
        args, dist, *_ = gu.phi4_setup(d=d, B=B, hidden=32, F=16)
    ctx = gu.make_ctx(dist, args)
    pos = torch.as_tensor(dist.init_params.astype(np.float32)).cuda()
    logp = torch.empty(B, dtype=torch.float64, device="cuda"); grad = torch.empty(B, d, device="cuda")
    ctx.mala_init(pos, 1.0, logp, grad)
    torch.cuda.synchronize()
    start = (pos.clone(), logp.clone(), grad.clone())
    state = [start]

    def reset():
        for t, s in zip((pos, logp, grad), state[0]):
            t.copy_(s)

    f64 = dict(dtype=torch.float64, device="cuda")
    trace = torch.zeros(iters, 7, **f64)
    step_avg = torch.empty(B, **f64)
    traj = torch.empty(n_steps, B, d, device="cuda")
    out = {}

    # ---- the warmups, each from the start state ----
    def chees(read=False):
        return ctx.chees_warmup(jr.PRNGKey(1), 1.0, eps0, iters, pos, logp, grad, trace=trace, read_result=read)

    reset(); eps, T, _, _ = chees(True)
    after_chees = (pos.clone(), logp.clone(), grad.clone())
    tr = trace.cpu().numpy()
    out["chees"] = dict(eps=eps, T=T, leap=tr[:, 2].sum(), hm=tr[-1, 3], div=tr[:, 5].sum(), t=_timed(chees, reset, reps))
    L_same = max(1, int(round(tr[:, 2].mean())))

    def hmc_warmup(L):
        return lambda: ctx.hmc_warmup(jr.PRNGKey(1), 1.0, eps0, L, iters, 0.8, pos, logp, grad, step_avg)

    reset(); hmc_warmup(L_same)(); torch.cuda.synchronize()
    out["hmc_warmup_same"] = dict(L=L_same, t=_timed(hmc_warmup(L_same), reset, reps))
    reset(); hmc_warmup(10)(); torch.cuda.synchronize()
    eps_dual = mcmc_utils.pooled_step_size(step_avg)
    leap = torch.zeros(B, dtype=torch.int64, device="cuda")
    eps_nuts = None
    if d <= 256:
        reset(); ctx.nuts_warmup(jr.PRNGKey(1), 1.0, eps0, depth, iters, 0.8, pos, logp, grad, step_avg); torch.cuda.synchronize()
        eps_nuts = mcmc_utils.pooled_step_size(step_avg)

    # ---- the samplers, each from the state the ChEES warmup left ----
    state[0] = after_chees
    key = jr.PRNGKey(2)

    def ess_of(grads_per_step, t_ms):
        e = mcmc_utils.effective_sample_size(traj, ctx=ctx)[0].double().reshape(-1)
        per_grad = e / (n_steps * grads_per_step)
        per_sec = e / (np.median(t_ms) * 1e-3)
        return per_grad.min().item(), per_grad.median().item(), per_sec.min().item(), per_sec.median().item()

    lengths = torch.as_tensor([integration_steps(i, eps, T) for i in range(n_steps)], dtype=torch.int32).cuda()
    mean_len = lengths.double().mean().item()

    def run_lengths():
        ctx.hmc_run_lengths(key, 1.0, eps, lengths, pos, logp, grad, thin=1, traj_pos=traj)

    def run_fixed():
        ctx.hmc_run(key, 1.0, eps_dual, 10, n_steps, pos, logp, grad, thin=1, traj_pos=traj)

    def run_nuts():
        ctx.nuts_run(key, 1.0, eps_nuts, depth, n_steps, pos, logp, grad, thin=1, leapfrog_sum=leap, traj_pos=traj)

    t = _timed(run_lengths, reset, reps)
    out["run_lengths"] = dict(eps=eps, mean_leap=mean_len, t=t, ess=ess_of(mean_len, t))
    t = _timed(run_fixed, reset, reps)
    out["run_fixed"] = dict(eps=eps_dual, mean_leap=10.0, t=t, ess=ess_of(10.0, t))
    if eps_nuts is not None:
        t = _timed(run_nuts, reset, reps)
        ml = leap.double().mean().item() / n_steps
        out["run_nuts"] = dict(eps=eps_nuts, mean_leap=ml, t=t, ess=ess_of(ml, t))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fmt = lambda v: f"{np.median(v):9.3f} [{v.min():.3f}..{v.max():.3f}]"
    lines = [f"ChEES-HMC: warmups of {a.iters} iterations, samplers of {a.steps} steps (thin = 1), {a.reps} timed calls each; ms, median [min..max]"]
    for title, kind, d, eps0 in SHAPES:
        for B in CHAINS:
            o = shape(kind, d, B, eps0, a.iters, a.steps, a.depth, a.reps)
            c, w = o["chees"], o["hmc_warmup_same"]
            tc, tw = np.median(c["t"]), np.median(w["t"])
            lines += [f"{title}, {B} chains, first step size {eps0:g}",
                      f"  mfm_chees_warmup        {fmt(c['t'])}   {1e3 * tc / a.iters:8.2f} us per iteration, {1e3 * tc / c['leap']:7.3f} us per leapfrog step of all chains"
                      f"   ({int(c['leap'])} leapfrog steps; adapted eps {c['eps']:.4g}, T {c['T']:.4g}; last hm {c['hm']:.3f}; divergent chain-iterations {int(c['div'])})",
                      f"  mfm_hmc_warmup, L = {w['L']:<4d}{fmt(w['t'])}   {1e3 * tw / a.iters:8.2f} us per step,      {1e3 * tw / (a.iters * w['L']):7.3f} us per leapfrog step of all chains"
                      f"   ChEES / per-chain warmup per leapfrog: {(tc / c['leap']) / (tw / (a.iters * w['L'])):.2f}"]
            for name, label in (("run_lengths", "mfm_hmc_run_lengths (ChEES eps, T)"), ("run_fixed", "mfm_hmc_run, L = 10 (dual averaging)"),
                                ("run_nuts", f"mfm_nuts_run, depth {a.depth} (NUTS warmup)")):
                if name not in o:
                    continue
                r = o[name]
                lines.append(f"  {label:38s}{fmt(r['t'])}   eps {r['eps']:.4g}, mean leapfrog {r['mean_leap']:.1f}; ESS per gradient (min, median) "
                             f"{r['ess'][0]:.4g}, {r['ess'][1]:.4g}; ESS per second {r['ess'][2]:.4g}, {r['ess'][3]:.4g}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
