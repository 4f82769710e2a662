"""Autocorrelation of a chain trajectory on the device: mfm_autocorr (diag.hip: direct lag sums, one lane per series) against what a user
would write today with torch.fft (centre, rfft of the zero-padded signal, squared magnitude, irfft, normalise).

Shapes: [1000, 4096, 256] (the headline chains, 4 GB) at L = 1000 and L = 100 lags, and [1000, 512, 2] at L = 1000.  The data are AR(1)
series with phi uniform in [0, 0.9] (generated on the device), so that the tau-only call meets realistic truncation points.  Variants:
  rho      mfm_autocorr returning rho [L][S]
  tau      mfm_autocorr returning tau only (no [L][S] buffer; a wave stops at the lag block where its 64 series have all truncated)
  ... f64  the same two from a context created under MFM_AUTOCORR_F64=1 (lag sums in float64 throughout, not float32 time blocks)
  fft      torch.fft.rfft / irfft of the same quantity, with its peak extra device memory
`--warmup` untimed calls of each, then `--reps` rounds that time every variant once, in rotating order, with HIP events after a
synchronisation; printed: median [min..max] in ms, the rate in lag-sum FMAs (n L - L (L - 1) / 2 per series) for the rho variants,
and the largest |rho - rho_fft|.  `--out` keeps a copy of the table.

    python tools/autocorr_time.py [--reps 20] [--warmup 3] [--out profiles/autocorr_time.txt] [--small]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

SHAPES = [((1000, 4096, 256), 1000), ((1000, 4096, 256), 100), ((1000, 512, 2), 1000)]
SMALL = [((100, 64, 8), 100), ((100, 64, 8), 10)]          # --small: a rehearsal of the script itself


def make_ctx(f64):
    from mfm_amd import _lib
    if f64:
        os.environ["MFM_AUTOCORR_F64"] = "1"
    else:
        os.environ.pop("MFM_AUTOCORR_F64", None)
    try:             # (the switch is read once, at mfm_create, and belongs to that context)
        return _lib.Context(dim=2, n_chain_local=16, fourier_dim=16, hidden_t=(16, 16), hidden_x=(16, 16), hidden_xt=(16, 16))
    finally:
        os.environ.pop("MFM_AUTOCORR_F64", None)


def ar1_device(shape, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    n, S = shape[0], int(np.prod(shape[1:]))
    phi = torch.rand(S, device="cuda", generator=g) * 0.9
    x = torch.empty((n, S), device="cuda")
    x[0] = torch.randn(S, device="cuda", generator=g) / torch.sqrt(1 - phi * phi)
    for t in range(1, n):
        x[t] = phi * x[t - 1] + torch.randn(S, device="cuda", generator=g)
    x += 3.0
    return x


def fft_rho(x, L):
    import torch
    n = x.shape[0]
    c = x - x.mean(dim=0, keepdim=True)
    f = torch.fft.rfft(c, n=2 * n, dim=0)
    a = torch.fft.irfft(f * f.conj(), n=2 * n, dim=0)[:L]
    return a / a[:1]


def _time_once(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def shape(ctxs, dims, L, reps, warmup):
    import torch
    x = ar1_device(dims, 1)
    n, S = x.shape
    rho = torch.empty((L, S), device="cuda")
    tau = torch.empty(S, device="cuda")
    calls = {}
    for tag, c in ctxs.items():
        calls["rho" + tag] = lambda c=c: c.autocorr(x, n_lags=L, rho=rho)
        calls["tau" + tag] = lambda c=c: c.autocorr(x, n_lags=L, tau=tau)
    keep = {}
    calls["fft"] = lambda: keep.__setitem__("r", fft_rho(x, L))
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    calls["rho"]()
    err = float((rho - keep["r"]).abs().max())
    tau_mean = float(tau.mean())
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
    return {k: np.array(v) for k, v in t.items()}, err, fft_peak, tau_mean


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("autocorr_time.py measures on the GPU: none is visible")
    ctxs = {"": make_ctx(False), " f64": make_ctx(True)}
    lines = [f"mfm_autocorr vs torch.fft; {a.reps} rounds in rotating order after {a.warmup} warm-up calls; HIP events; ms, median [min..max]"]
    for dims, L in (SMALL if a.small else SHAPES):
        t, err, fft_peak, tau_mean = shape(ctxs, dims, L, a.reps, a.warmup)
        n, S = dims[0], int(np.prod(dims[1:]))
        fma = S * (n * L - L * (L - 1) / 2)
        lines.append(f"trajectory {list(dims)} float32 ({4 * n * S / 2 ** 30:.2f} GiB), L = {L}: mean tau {tau_mean:.2f}, max |rho - rho_fft| {err:.2g}")
        for k, v in t.items():
            extra = ""
            if k.startswith("rho"):
                extra = f"   {1e-6 * fma / np.median(v):8.1f} GFMA/s"
            if k == "fft":
                extra = f"   peak extra memory {fft_peak / 2 ** 30:.2f} GiB"
            lines.append(f"  {k:8s} {np.median(v):9.3f} [{v.min():.3f}..{v.max():.3f}]{extra}")
        print("\n".join(lines[-(len(t) + 1):]), flush=True)
    for c in ctxs.values():
        c.close()
    text = "\n".join(lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
