"""GHMC and the MEADS warmup on the clock, phi-four d = 256, 4096 chains, beta = 1, from one start state:

* mfm_ghmc_run of `--steps` transitions against mfm_hmc_run of `--steps` steps at num_steps = 1 (the same gradient count and the same
  d normal draws per step), `--reps` timed calls each with HIP events around the call, interleaved; us per transition of all chains,
  median and min .. max;
* mfm_meads_warmup of `--steps` iterations (4 folds, no trace, no read-back: the call only enqueues) against mfm_ghmc_run of as many
  transitions: what the statistics launches add to an iteration;
* after that warmup: `--ess` transitions of mfm_ghmc_run under the adapted parameters, thin = 1, Geyer's ESS per gradient (min / median /
  mean over chains and coordinates) and the largest split R-hat.

    python tools/ghmc_time.py [--reps 7] [--steps 200] [--ess 400] [--out profiles/ghmc_time.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--ess", type=int, default=400)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from mfm_amd import _lib, mcmc_utils, random as jr
    d, B, n = a.dim, a.chains, a.steps
    ctx = _lib.Context(dim=d, n_chain_local=B, fourier_dim=16, hidden_t=(16, 16), hidden_x=(16, 16), hidden_xt=(16, 16))
    ctx.set_target(_lib.PHI4, [0.1, 20.0])
    x0 = torch.as_tensor(jr.uniform(jr.PRNGKey(1), (B, d), -1.0, 1.0).astype(np.float32)).cuda()
    pos = x0.clone(); logp = torch.empty(B, dtype=torch.float64, device="cuda"); grad = torch.empty_like(pos)
    mom = torch.empty(B, d, dtype=torch.float64, device="cuda"); s = torch.empty(B, dtype=torch.float64, device="cuda")
    ctx.mala_init(pos, 1.0, logp, grad)
    ctx.ghmc_init(jr.PRNGKey(2), mom, s)
    ctx.ghmc_run(jr.PRNGKey(3), 1.0, 0.005, 0.3, 0.15, 300, pos, logp, grad, mom, s)        # off the U(-1, 1) start
    start = tuple(t.clone() for t in (pos, logp, grad, mom, s))
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def reset():
        for t, t0 in zip((pos, logp, grad, mom, s), start):
            t.copy_(t0)
    key, eps = jr.PRNGKey(4), 0.008
    calls = {"mfm_hmc_run (num_steps 1)": lambda: ctx.hmc_run(key, 1.0, eps, 1, n, pos, logp, grad),
             "mfm_ghmc_run": lambda: ctx.ghmc_run(key, 1.0, eps, 0.3, 0.15, n, pos, logp, grad, mom, s),
             "mfm_meads_warmup (4 folds)": lambda: ctx.meads_warmup(key, 1.0, eps, 0.3, n, pos, logp, grad, mom, s, n_folds=4, read_result=False)}
    for fn in calls.values():                                      # first launches, workspace allocation
        reset(); fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(a.reps):                                        # interleaved: drift of the clock falls on all three alike
        for k, fn in calls.items():
            times[k].append(_timed(fn, reset, 1)[0])
    say(f"phi-four d = {d}, {B} chains, {n} steps per call, {a.reps} calls each (HIP events, interleaved)")
    med = {}
    for k, v in times.items():
        v = np.array(v) * 1e3 / n
        med[k] = np.median(v)
        say(f"  {k:28s} {np.median(v):8.2f} us per step of all chains (min {v.min():.2f}, max {v.max():.2f})")
    h, g, m = (med[k] for k in calls)
    say(f"  GHMC over HMC at one leapfrog step: {100 * (g / h - 1):+.1f} %; MEADS iteration over GHMC transition: {m / g:.2f} x "
        f"(statistics launches: {100 * (1 - g / m):.1f} % of an iteration)")
    # ESS per gradient after a MEADS warmup
    reset()
    minv = torch.empty(d, dtype=torch.float64, device="cuda")
    e, al, de = ctx.meads_warmup(jr.PRNGKey(5), 1.0, eps, 0.3, n, pos, logp, grad, mom, s, n_folds=4, inverse_mass_out=minv)
    traj = torch.empty(a.ess, B, d, device="cuda")
    n_acc = torch.empty(B, dtype=torch.int32, device="cuda")
    ctx.ghmc_run(jr.PRNGKey(6), 1.0, e, al, de, a.ess, pos, logp, grad, mom, s, minv, thin=1, n_acc=n_acc, traj_pos=traj)
    ess, _ = mcmc_utils.effective_sample_size(traj, ctx=ctx)
    per = (ess.double() / a.ess).reshape(-1)
    from mfm_amd import diagnostics
    cd = diagnostics.chain_diagnostics(traj, n_valid=B, ctx=ctx)
    say(f"after {n} MEADS iterations: step size {e:.4g}, alpha {al:.4g}, inverse mass in [{minv.min().item():.3g}, {minv.max().item():.3g}], "
        f"acceptance {n_acc.double().mean().item() / a.ess:.3f}")
    say(f"  ESS per gradient over {a.ess} transitions (min / median / mean): {per.min().item():.4g} / {per.median().item():.4g} / {per.mean().item():.4g}"
        + f"; split R-hat max {cd.rhat.max().item():.4g}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
