"""Parallel tempering: what one round costs, and what the per-chain parameters and the exchange sweep add to the local steps.

phi-four d = 256, 4096 chains = 512 ladders x K = 8 temperatures (geometric, 1 to 0.01), HMC with L = 10 leapfrog steps, n_local = 4,
step size --eps / sqrt(beta_k).  Timed with HIP events around each call, `--reps` calls of `--rounds` rounds each, from the same start
state (every slot initialised at its own beta):

* mfm_hmc_run of n_local = 4 steps at a SCALAR beta = 1 and step size --eps: the launch the round's local steps replace, one per round;
* mfm_pt_run with exchange = 0: the same steps with beta and the step size read per wave from the ladder;
* mfm_pt_run with exchange = 1: the round as it is run, and the difference to the line above, the sweep;
* mfm_pt_exchange alone, both parities.

    python tools/pt_time.py [--reps 5] [--rounds 50] [--eps 0.01] [--out profiles/pt_time.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

D, CHAINS, K, L, N_LOCAL, BETA_MIN = 256, 4096, 8, 10, 4, 0.01


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--eps", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from mfm_amd import random as jr
    from mfm_amd.bblackjax.mcmc.parallel_tempering import geometric_ladder
    from tests import gpu_util as gu
    args, dist, *_ = gu.phi4_setup(d=D, B=CHAINS, hidden=32, F=16)
    ctx = gu.make_ctx(dist, args)
    betas = geometric_ladder(K, BETA_MIN)
    eps = a.eps / np.sqrt(betas)
    R = CHAINS // K
    pos = torch.as_tensor(dist.init_params.astype(np.float32)).cuda()
    logp = torch.empty(CHAINS, dtype=torch.float64, device="cuda"); grad = torch.empty_like(pos)
    lp_k, g_k = torch.empty_like(logp), torch.empty_like(grad)
    for k in range(K):
        ctx.mala_init(pos, float(betas[k]), lp_k, g_k)
        logp[k::K] = lp_k[k::K]; grad[k::K] = g_k[k::K]
    start = (pos.clone(), logp.clone(), grad.clone())
    lp1, g1 = torch.empty_like(logp), torch.empty_like(grad)
    ctx.mala_init(pos, 1.0, lp1, g1)
    start_scalar = (pos.clone(), lp1, g1)
    key = jr.PRNGKey(1)
    sw = torch.zeros(R, K - 1, dtype=torch.int32, device="cuda")

    def reset_to(state):
        def reset():
            for t, s in zip((pos, logp, grad), state):
                t.copy_(s)
        return reset

    def scalar():
        for _ in range(a.rounds):
            ctx.hmc_run(key, 1.0, a.eps, L, N_LOCAL, pos, logp, grad)

    def pt(exchange):
        return lambda: ctx.pt_run(key, betas, eps, R, N_LOCAL, a.rounds, pos, logp, grad, kernel="hmc", num_steps=L, exchange=exchange, swap_accepted=sw)

    def sweeps():
        for t in range(a.rounds):
            ctx.pt_exchange(key, betas, R, t % 2, pos, logp, grad)

    for fn, st in ((scalar, start_scalar), (pt(False), start), (pt(True), start)):      # warm every kernel
        reset_to(st)(); fn(); torch.cuda.synchronize()
    t_scalar = _timed(scalar, reset_to(start_scalar), a.reps) / a.rounds * 1e3
    t_none = _timed(pt(False), reset_to(start), a.reps) / a.rounds * 1e3
    t_full = _timed(pt(True), reset_to(start), a.reps) / a.rounds * 1e3
    rates = sw.sum(0).double().cpu().numpy() / (R * np.array([len(range(k % 2, a.rounds, 2)) for k in range(K - 1)]))
    t_sweep = _timed(sweeps, reset_to(start), a.reps) / a.rounds * 1e3
    ctx.close()
    fmt = lambda v: f"{np.median(v):9.2f} [{v.min():.2f}..{v.max():.2f}]"
    m = np.median
    lines = [f"Parallel tempering, phi-four d = {D}, {CHAINS} chains = {R} ladders x K = {K} (beta 1 .. {BETA_MIN}), HMC L = {L}, n_local = {N_LOCAL}, "
             f"eps = {a.eps:g} / sqrt(beta); us per round, median [min..max] over {a.reps} calls of {a.rounds} rounds",
             f"  mfm_hmc_run, {N_LOCAL} steps, scalar beta = 1 (one launch per round) {fmt(t_scalar)}",
             f"  mfm_pt_run, exchange = 0 (per-chain beta and step size)          {fmt(t_none)}   {m(t_none) / m(t_scalar):.3f} x the scalar launch",
             f"  mfm_pt_run, exchange = 1 (the round)                              {fmt(t_full)}   the sweep adds {m(t_full) - m(t_none):.2f} us, "
             f"{100 * (m(t_full) - m(t_none)) / m(t_full):.1f} % of the round",
             f"  mfm_pt_exchange alone, alternating parities                      {fmt(t_sweep)}",
             "  swap acceptance rate per pair: " + ", ".join(f"{r:.3f}" for r in rates),
             "  (the tempered chains do different work from the scalar ones -- hot chains move further -- but the same number of gradient evaluations)"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
