"""The times of DESIGN section 4.20 (python tools/cox_hmc_time.py): mfm_cox_hmc_run per leapfrog step on the 32 x 32 Cox process with 32 and
1024 chains, per HMC step at num_steps = 1, and one mfm_mala_step on the same context.  HIP events, median / min / max of 7 after one warm call."""
import os, sys, json
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from oracle import loop, prng
from tests import cox_hmc_cases as cc, gpu_util as gu

def ctx_of(n, B):
    dist = cc.dist_of(n)
    args = loop.default_args(example="pines", dim=dist.dim, num_chain=B, hutchs=True, step_size=0.01, seed=1, fourier_dim=16, **gu.hidden_lists(32))
    return dist, gu.make_ctx(dist, args, n_local=B)

def timed(fn, reps):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

out = {}
for B in (32, 1024):
    dist, ctx = ctx_of(32, B)
    d = dist.dim
    xi = prng.normal_rows(prng.split(prng.PRNGKey(5), B), d)
    x0 = torch.as_tensor((dist.mu + xi @ dist.chol.T).astype(np.float32)).cuda()
    pos = x0.clone(); logp = torch.empty(B, dtype=torch.float64, device="cuda"); grad = torch.empty_like(pos)
    ctx.mala_init(pos, 1.0, logp, grad)
    key = prng.PRNGKey(9)
    L, n = 8, 25            # 200 leapfrog steps per call
    t_run = timed(lambda: ctx.cox_hmc_run(key, 1.0, 0.05, L, n, pos, logp, grad), 7)
    L1 = timed(lambda: ctx.cox_hmc_run(key, 1.0, 0.05, 1, n, pos, logp, grad), 7)
    nm = 200
    def malas():
        for _ in range(nm):
            ctx.mala_step(key, 1.0, 0.01, pos, logp, grad)
    t_mala = timed(malas, 7)
    out[B] = dict(hmc_run_ms=t_run, per_leapfrog_us=1e3 * t_run[0] / (L * n), hmc_L1_run_ms=L1, per_step_L1_us=1e3 * L1[0] / n,
                  mala_200_ms=t_mala, per_mala_step_us=1e3 * t_mala[0] / nm)
    print(B, json.dumps(out[B]), flush=True)
    ctx.close()
