"""Time of one SVGD iteration on the device (mfm_svgd_step and its kernels, svgd.hip) against the obvious PyTorch formulation on the same
GPU: exp, two matmuls, the same adagrad update, then centre, x @ x.T and torch.median over the lower triangle of the NEW particles,
whose distances and centred coordinates it carries into the next iteration exactly as mfm_svgd_step does (one x @ x.T per iteration on
both sides).

Shapes: n = 4096, d = 256 on phi-four (the headline shape); n = 4096, d = 2 on the 4-mode mixture; n = 1024, d = 1024 on the Cox process
(pines).  Timed, each by HIP events after a synchronisation, `--warmup` untimed windows first, then `--reps` rounds that time every
variant once in rotating order; a window is `--iters` back-to-back iterations (step, interaction, torch) or `--inner` back-to-back
launches of one piece, so that the small kernels are not timed as one launch and its events; printed: median [min..max] in ms per
iteration or launch.
  step         mfm_svgd_step, n_iter = --iters in one call (target gradient + interaction)
  interaction  mfm_svgd_gradient + mfm_svgd_apply + mfm_svgd_sqdist (new particles) + mfm_svgd_median as four calls on the carried D:
               the work of one iteration without the target gradient, and what `torch` computes
  torch        the PyTorch formulation of the same work (no target gradient either)
  target_grad / sqdist / median / gradient / apply   the pieces
and the share of the 157.3 TFLOP/s f32 matrix peak that 6 n^2 d flops (2 n^2 d distances + 4 n^2 d weighted sums) reach over sqdist +
gradient and over the whole interaction.  `--out` keeps a copy of the table.

    python tools/svgd_time.py [--reps 20] [--warmup 3] [--iters 5] [--inner 20] [--out profiles/svgd_time.txt] [--small]
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

PEAK_F32_MATRIX = 157.3e12
SHAPES = [("phi-four", 4096, 256), ("4-mode", 4096, 2), ("pines", 1024, 1024)]
SMALL = [("phi-four", 64, 64), ("4-mode", 48, 2), ("pines", 32, 64)]          # --small: a rehearsal of the script itself


def _time_once(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def make_engine(example, n, d):
    from mfm_amd import random as jr
    from mfm_amd.distributions import GaussianMixture, LogGaussianCoxPines, PhiFour
    from mfm_amd.engine import Engine
    from mfm_amd.multi_modal import build_parser
    args = build_parser().parse_args(["--example", example, "--num_chain", str(n), "--seed", "1"])
    args.dim = d
    args.hidden_x = args.hidden_t = args.hidden_xt = [32, 32]          # the network plays no part: keep its workspaces small
    args.fourier_dim = 16
    if example == "phi-four":
        dist = PhiFour(d)
    elif example == "4-mode":
        dist = GaussianMixture(8. * np.array([[1, 1], [1, -1], [-1, 1], [-1, -1]]), np.ones((4, 2)), np.ones(4) / 4)
    else:
        dist = LogGaussianCoxPines(d)
    dist.initialize_model(jr.PRNGKey(1), n)
    return Engine(dist, args, None), dist


class TorchSvgd:
    """The PyTorch-ROCm formulation: everything stays on the device, no host synchronisation; the distances and centred coordinates
    of the new particles are kept for the next iteration, so an iteration has ONE x @ x.T, as on the device path."""

    def __init__(self, x, lr=0.1):
        import torch
        self.t, self.n, self.lr = torch, x.shape[0], lr
        self.x, self.acc = x.clone(), torch.full_like(x, 0.1)
        self.ii, self.jj = torch.tril_indices(self.n, self.n, -1, device=x.device)
        self.D, self.xc = self.sqdist(self.x)
        self.h = self.median(self.D)

    def sqdist(self, x):
        xc = x - x.mean(0)
        q = (xc * xc).sum(1)
        return (q[:, None] + q[None, :] - 2.0 * (xc @ xc.T)).clamp_min_(0.0), xc

    def median(self, D):
        med = self.t.median(self.t.sqrt(D[self.ii, self.jj]))
        return med * med / math.log(self.n)

    def iteration(self, g):
        t = self.t
        K = t.exp(-self.D / self.h)
        fg = -(K @ g + (2.0 / self.h) * (K.sum(1, keepdim=True) * self.xc - K @ self.xc)) / self.n
        self.acc += fg * fg
        self.x = self.x - self.lr * fg * t.rsqrt(self.acc + 1e-7)
        self.D, self.xc = self.sqdist(self.x)
        self.h = self.median(self.D)


def shape(example, n, d, reps, warmup, iters, inner):
    import torch
    from mfm_amd.bblackjax import optimizers as O
    eng, dist = make_engine(example, n, d)
    ctx = eng.ctx
    x0 = eng.local(dist.init_params)
    opt = O.adagrad(0.1)
    logp = torch.empty(n, device="cuda", dtype=torch.float64)
    g, fg = torch.empty_like(x0), torch.empty_like(x0)
    D = torch.empty((n, n), device="cuda", dtype=torch.float32)
    ls = torch.ones(1, device="cuda", dtype=torch.float64)
    ctx.mala_init(x0, 1.0, logp, g)
    ctx.svgd_sqdist(x0, D)
    ctx.svgd_median(D, ls)
    ref = TorchSvgd(x0)
    xs, (acc, _) = x0.clone(), opt.init(x0)
    xi, (acci, _) = x0.clone(), opt.init(x0)
    lsi = ls.clone()

    Di = D.clone()                                   # the interaction's carried matrix: always that of xi as it stands
    xa, (acca, _) = x0.clone(), opt.init(x0)

    def interaction():
        ctx.svgd_gradient(xi, g, Di, lsi, fg)
        ctx.svgd_apply(opt.kind, opt.hyper, 0, xi, fg, [acci])
        ctx.svgd_sqdist(xi, Di)
        ctx.svgd_median(Di, lsi)

    def many(fn, k):
        def run():
            for _ in range(k):
                fn()
        return run, k

    calls = {"step": (lambda: ctx.svgd_step(1.0, opt.kind, opt.hyper, 0, iters, xs, [acc], ls.clone()), iters),
             "interaction": many(interaction, iters), "torch": many(lambda: ref.iteration(g), iters),
             "target_grad": many(lambda: ctx.mala_init(x0, 1.0, logp, g), inner), "sqdist": many(lambda: ctx.svgd_sqdist(x0, D), inner),
             "median": many(lambda: ctx.svgd_median(D, ls), inner), "gradient": many(lambda: ctx.svgd_gradient(x0, g, D, ls, fg), inner),
             "apply": many(lambda: ctx.svgd_apply(opt.kind, opt.hyper, 0, xa, fg, [acca]), inner)}
    for fn, _ in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    names = list(calls)
    t = {k: [] for k in names}
    for r in range(reps):
        for i in range(len(names)):
            k = names[(r + i) % len(names)]
            fn, per = calls[k]
            t[k].append(_time_once(fn) / per)
    finite = bool(torch.isfinite(xs).all() and torch.isfinite(xi).all() and torch.isfinite(ref.x).all())
    eng.close()
    return {k: np.array(v) for k, v in t.items()}, finite


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("svgd_time.py measures on the GPU: none is visible")
    from mfm_amd._lib import MfmError
    lines = [f"mfm_svgd_step and its kernels vs the PyTorch formulation (one x @ x.T per iteration on both sides); {a.reps} rounds in rotating order "
             f"after {a.warmup} warm-up windows; HIP events around {a.iters} iterations (step, interaction, torch) or {a.inner} launches (the pieces); "
             "ms per iteration or launch, median [min..max]"]
    for example, n, d in (SMALL if a.small else SHAPES):
        try:
            t, finite = shape(example, n, d, a.reps, a.warmup, a.iters, a.inner)
        except MfmError as err:             # only the library's named refusals of a shape (MFM_EUNSUPPORTED -2, MFM_ETOOLARGE -3) are reported
            if not str(err).startswith(("libmfm_hip error -2:", "libmfm_hip error -3:")):      # and the next shape tried; anything else ends the run
                raise
            lines.append(f"{example}: n = {n}, d = {d}: NOT MEASURED -- {err}")
            print(lines[-1], flush=True)
            continue
        flops = 6.0 * n * n * d
        gemm = np.median(t["sqdist"]) + np.median(t["gradient"])
        lines.append(f"{example}: n = {n}, d = {d} ({flops / 1e9:.2f} GFLOP per iteration; particles finite after the runs: {finite})")
        for k, v in t.items():
            lines.append(f"  {k:12s} {np.median(v):9.4f} [{v.min():.4f}..{v.max():.4f}]")
        lines.append(f"  share of the {PEAK_F32_MATRIX / 1e12:.1f} TFLOP/s f32 matrix peak on 6 n^2 d flops: sqdist + gradient "
                     f"{flops / (gemm * 1e-3) / PEAK_F32_MATRIX:.3f}, interaction {flops / (np.median(t['interaction']) * 1e-3) / PEAK_F32_MATRIX:.3f}; "
                     f"torch / interaction = {np.median(t['torch']) / np.median(t['interaction']):.2f}")
        print("\n".join(lines[-(len(t) + 2):]), flush=True)
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
