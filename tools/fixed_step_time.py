"""Flow-step and final-sampling transform time of the fixed-step mode (--ode_method rk4|euler --ode_steps N) against the adaptive
Dopri5 on the three workloads whose solves run outside the shape-specialised tile:

  pines            1024 chains, d = 1024, hidden 1024, --hutch     wide family (wide.hip: solve / solve_fixed)
  gaussian-mixture 4096 chains, 16 modes, exact trace              d = 2 four-chain tile (ode_d2.hip)
  4-mode            512 chains, exact trace, n_ts = 5               d = 2 four-chain tile

Set up as bench.py's fixed_step_report: one context per integrator, the same chains, parameters and keys on each, the first of
`--reps` repetitions dropped.  The network is a random one with a tamed gate (tests' gpu_util.rand_params), not a trained one: its
Dopri5 attempt counts are printed beside the times.  Per integrator and workload: the flow-MH step (RWMH, two solves per chain) and a
transform of `chains` samples, each as
  wall_ms    host clock around the call and a stream synchronisation,
  enqueue_ms host clock until the call returns: a solve that reads back from the device (the adaptive wide loop: once per attempted
             step) returns only when the GPU is done; a fixed launch sequence returns once it is queued,
  events_ms  HIP events around the call on the context's (default) stream,
and the field evaluations and steps per chain from mfm_get_counters.

    python tools/fixed_step_time.py [--workloads pines,gaussian-mixture,4-mode] [--reps 4] [--out profiles/r06_fixed_step_time.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

INTEGRATORS = [("dopri5", 0), ("rk4", 16), ("rk4", 64), ("euler", 64), ("euler", 256)]
SOLVER = {"pines": "wide", "gaussian-mixture": "d2", "4-mode": "d2"}      # the solver mfm_create picks for each (module docstring)


def _setup(workload, method, steps):
    from tests import gpu_util as gu
    kw = dict(ode_method=method, ode_steps=steps) if steps else {}
    if workload == "pines":
        args, dist, k, model, state = gu.lgcp_setup(n=32, B=1024, hidden=1024, F=128, **kw)
        params = gu.rand_params(model, seed=2, out_scale=0.2)
        params[4]["kernel"] *= 0.02; params[4]["bias"] *= 0.02
        beta = 1.0
    elif workload == "gaussian-mixture":
        args, dist, k, model, state = gu.gmm16_setup(B=4096, hutchs=False, **kw)
        params = gu.rand_params(model, seed=9, out_scale=0.3)
        beta = 1.0
    else:
        args, dist, k, model, state = gu.gmm4_setup(B=512, hidden=128, F=128, hutchs=False, **kw)
        params = gu.rand_params(model, seed=9, out_scale=0.3)
        beta = 1.0
    return gu, args, dist, model, params, beta


def measure(workload, method, steps, reps):
    import torch
    from mfm_amd import _lib
    from oracle import prng
    gu, args, dist, model, params, beta = _setup(workload, method, steps)
    B = args.num_chain
    ctx = gu.make_ctx(dist, args, fourier=model.f, params=params)
    x32 = dist.init_params.astype(np.float32)
    pos0 = torch.as_tensor(x32).cuda()
    logp0 = torch.empty(B, dtype=torch.float64, device="cuda"); grad0 = torch.empty(B, args.dim, device="cuda")
    ctx.mala_init(pos0, beta, logp0, grad0)
    acc = torch.empty(B, device="cuda"); ns = torch.empty(B, dtype=torch.int32, device="cuda")
    out = torch.empty(B, args.dim, device="cuda"); ldj = torch.empty(B, device="cuda")
    key = prng.PRNGKey(31)
    res = {}
    for what in ("flow_step", "transform"):
        wall, enq, ev, evals, att = [], [], [], [], []
        for rep in range(reps):
            p, l, g = pos0.clone(), logp0.clone(), grad0.clone()
            ctx.sync(); torch.cuda.synchronize()
            ctx.reset_counters()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            if what == "flow_step":
                ctx.flow_step(_lib.FLOW_RWMH, key, beta, p, l, g, acc, None, None, ns)
            else:
                ctx.ode_transform(1, p, out, ldj, key=prng.PRNGKey(4), nsteps=ns)
            tq = time.perf_counter()
            e1.record()
            ctx.sync(); torch.cuda.synchronize()
            t1 = time.perf_counter()
            c = ctx.counters()
            if rep:
                wall.append((t1 - t0) * 1e3); enq.append((tq - t0) * 1e3)
                ev.append(e0.elapsed_time(e1))
                evals.append(c["field_evals"] / B); att.append(c["dopri_attempts"] / B)
        assert torch.isfinite(p).all() and torch.isfinite(out).all()
        res[what] = dict(wall_ms=round(float(np.mean(wall)), 3), enqueue_ms=round(float(np.mean(enq)), 3), events_ms=round(float(np.mean(ev)), 3),
                         field_evals_per_chain=round(float(np.mean(evals)), 2), steps_per_chain=round(float(np.mean(att)), 2))
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--workloads", default="pines,gaussian-mixture,4-mode")
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    report = {"note": "random tamed network (not trained); first repetition dropped; times in ms per call", "workloads": {}}
    for wl in a.workloads.split(","):
        rows = {}
        for method, steps in INTEGRATORS:
            name = method if not steps else f"{method}_x{steps}"
            r = measure(wl, method, steps, a.reps)
            rows[name] = r
            f, t = r["flow_step"], r["transform"]
            print(f"{wl:17s} {SOLVER[wl]:4s} {name:10s} flow step {f['events_ms']:9.3f} ms (wall {f['wall_ms']:9.3f}, {f['field_evals_per_chain']:6.1f} evals, "
                  f"{f['steps_per_chain']:5.1f} steps per chain, enqueued in {f['enqueue_ms']:8.3f})   transform {t['events_ms']:9.3f} ms (wall {t['wall_ms']:9.3f}, "
                  f"{t['field_evals_per_chain']:6.1f} evals)", flush=True)
        report["workloads"][wl] = dict(family=SOLVER[wl], **rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(report, fh, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
