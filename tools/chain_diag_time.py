"""Split-R-hat and multi-chain effective sample size of a chain trajectory on the device: mfm_chain_sums + mfm_chain_diag (diag.hip: the lag
sums of mfm_autocorr, summed over the chains inside the kernel) against
  autocorr  mfm_autocorr returning rho [L][S] at the same shape and lag count: the same lag sums WITHOUT the reduction over chains (every
            series keeps its own row of the [L][S] buffer), so the difference is what the reduction costs or saves;
  fft       the same statistic written with torch.fft (split, centre, rfft of the zero-padded sub-chains, squared magnitude, irfft, mean
            over sub-chains, Geyer's sum by a cumulative product), with its peak extra device memory.

Shapes: [1000, 4096, 256] (the headline chains, 3.9 GiB) at max_lag 100 and 500, and [1000, 512, 2] at max_lag 500; split = 1, so
n_sub = 500.  The data are AR(1) series with phi uniform in [0, 0.9] (generated on the device).  `--warmup` untimed calls of each, then
`--reps` rounds that time every variant once, in rotating order, with HIP events after a synchronisation; printed: median [min..max] in
ms and the largest relative difference of rhat / ess between the kernel and the fft route.  `--out` keeps a copy of the table.

    python tools/chain_diag_time.py [--reps 20] [--warmup 3] [--out profiles/chain_diag_time.txt] [--small]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from autocorr_time import _time_once, ar1_device, make_ctx  # noqa: E402  (tools/autocorr_time.py: the same data, timer and context)

SHAPES = [((1000, 4096, 256), 100), ((1000, 4096, 256), 500), ((1000, 512, 2), 500)]
SMALL = [((100, 64, 8), 50), ((100, 64, 70), 10)]          # --small: a rehearsal of the script itself


def fft_chain_diag(x, L):
    """(rhat, ess) [dim] of x [n, B, d] with split halves, through torch.fft."""
    import torch
    n = x.shape[0]
    h = n // 2
    y = torch.cat([x[:h], x[n - h:]], dim=1)
    M = y.shape[1]
    mu = y.mean(dim=0)
    c = y - mu
    f = torch.fft.rfft(c, n=2 * h, dim=0)
    acov = torch.fft.irfft(f * f.conj(), n=2 * h, dim=0)[:L].mean(dim=1) / (h - 1)
    W, Bn = acov[0], mu.var(dim=0, unbiased=True)
    varp = (h - 1) / h * W + Bn
    rho = 1.0 - (W - acov) / varp
    G = rho[0:2 * (L // 2):2] + rho[1:2 * (L // 2):2]
    keep = torch.cumprod((G > 0).to(G.dtype), dim=0)
    tau = -1.0 + 2.0 * (G * keep).sum(dim=0)
    return torch.sqrt(varp / W), M * h / tau


def shape(ctx, dims, L, reps, warmup):
    import torch
    n, B, d = dims
    x = ar1_device(dims, 1).view(n, B, d)
    sums = torch.empty((L + 2, d), device="cuda", dtype=torch.float64)
    rhat, ess, tau = (torch.empty(d, device="cuda") for _ in range(3))
    rho = torch.empty((L, B * d), device="cuda")
    keep = {}

    def ours():
        n_sub, M = ctx.chain_sums(x, sums, split=True)
        ctx.chain_diag(sums, n_sub, M, rhat=rhat, ess=ess, tau=tau)

    calls = {"chain_diag": ours, "autocorr": lambda: ctx.autocorr(x, n_lags=L, rho=rho),
             "fft": lambda: keep.__setitem__("r", fft_chain_diag(x, L))}
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ours()
    err = max(float((rhat / keep["r"][0] - 1).abs().max()), float((ess / keep["r"][1] - 1).abs().max()))
    stats = (float(rhat.max()), float(tau.mean()))
    keep.clear()
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(); torch.cuda.reset_peak_memory_stats()
    calls["fft"](); torch.cuda.synchronize()
    fft_peak = torch.cuda.max_memory_allocated() - base
    keep.clear()
    names = list(calls)
    t = {k: [] for k in names}
    for r in range(reps):
        for i in range(len(names)):
            k = names[(r + i) % len(names)]
            t[k].append(_time_once(calls[k]))
            keep.clear()
    return {k: np.array(v) for k, v in t.items()}, err, fft_peak, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("chain_diag_time.py measures on the GPU: none is visible")
    ctx = make_ctx(False)
    lines = [f"mfm_chain_sums + mfm_chain_diag vs mfm_autocorr (rho) vs torch.fft; {a.reps} rounds in rotating order after {a.warmup} warm-up calls; "
             "HIP events; ms, median [min..max]"]
    for dims, L in (SMALL if a.small else SHAPES):
        t, err, fft_peak, (rhat_max, tau_mean) = shape(ctx, dims, L, a.reps, a.warmup)
        n, S = dims[0], int(np.prod(dims[1:]))
        lines.append(f"trajectory {list(dims)} float32 ({4 * n * S / 2 ** 30:.2f} GiB), split, max_lag = {L}: max rhat {rhat_max:.4f}, mean tau {tau_mean:.2f}, "
                     f"max rel. difference of rhat / ess to the fft route {err:.2g}")
        for k, v in t.items():
            extra = f"   peak extra memory {fft_peak / 2 ** 30:.2f} GiB" if k == "fft" else ""
            lines.append(f"  {k:10s} {np.median(v):9.3f} [{v.min():.3f}..{v.max():.3f}]{extra}")
        print("\n".join(lines[-(len(t) + 1):]), flush=True)
    ctx.close()
    text = "\n".join(lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
