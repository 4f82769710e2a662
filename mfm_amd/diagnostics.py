"""Cross-chain convergence diagnostics of a trajectory ``[n, n_chain, dim]``: split-R-hat and the multi-chain ("bulk") effective
sample size of Gelman et al. / Stan, on the device (``mfm_chain_sums`` / ``mfm_chain_diag``, ``csrc/diag.hip``).

``mcmc_utils.effective_sample_size`` looks at every chain by itself: a chain that never leaves one mode of a multi-modal target looks
perfectly mixed to it.  The statistics here compare the chains with each other.  Every chain is split in two halves (``split``), each
half is a sub-chain of ``n_sub`` steps, ``M`` sub-chains in all; per coordinate

* ``W`` the mean within-sub-chain variance, ``B/n`` the variance of the sub-chain means, ``var+ = (n_sub - 1) / n_sub W + B/n``,
* ``rhat = sqrt(var+ / W)`` (1 when the chains agree, well above 1 when they sit in different places),
* ``rho_k = 1 - (W - mean_c A_k,c / (n_sub - 1)) / var+`` from the chain-averaged autocovariance, ``tau`` by Geyer's initial positive
  sequence over the first ``max_lag`` lags (the rule of ``mfm_autocorr``: no monotone smoothing, no clamp), ``ess = M n_sub / tau``.

The kernel reduces the trajectory where ``kernel.run`` left it to ``sums [max_lag + 2, dim]`` (float64), which is additive over chains:
with chains sharded over ranks ``sums`` and the sub-chain count go through ONE all-reduce (``engine.allreduce_sum_``, a no-op on one
rank), and every rank then holds the same result over the chains of all ranks.
"""
from typing import NamedTuple

__all__ = ["ChainDiagnostics", "chain_diagnostics", "potential_scale_reduction"]


class ChainDiagnostics(NamedTuple):
    rhat: object          # [dim] split-R-hat
    ess: object           # [dim] multi-chain effective sample size (of M n_sub draws over all ranks)
    tau: object           # [dim] integrated autocorrelation time, ess = M n_sub / tau


def _reduce(positions, n_lags, split, n_valid, ctx):
    """``(ctx, sums [n_lags + 2, dim] over all ranks, n_sub, M over all ranks, host)`` with ``n_lags = None`` meaning ``n_sub``."""
    import torch
    from . import mcmc_utils
    from .engine import allreduce_sum_
    xs, host = mcmc_utils._device_f32(positions, 0)
    if xs.ndim != 3:
        raise ValueError(f"positions must be [n, n_chain, dim] (got {tuple(xs.shape)})")
    n, n_chain_ld, dim = (int(v) for v in xs.shape)
    n_sub = n // 2 if split else n
    n_lags = n_sub if n_lags is None else int(n_lags)
    ctx = mcmc_utils._diag_ctx(ctx)
    buf = torch.zeros((max(n_lags, 0) + 2) * dim + 1, device=xs.device, dtype=torch.float64)      # sums, then the sub-chain count
    sums = buf[:-1].view(-1, dim)
    _, m_local = ctx.chain_sums(xs, sums, n_chain=n_chain_ld if n_valid is None else int(n_valid), split=split)
    buf[-1] = float(m_local)
    allreduce_sum_(buf)
    return ctx, sums, n_sub, int(round(buf[-1].item())), host


def chain_diagnostics(positions, max_lag=None, split=True, n_valid=None, ctx=None):
    """``ChainDiagnostics(rhat, ess, tau)``, each ``[dim]`` float32, of a trajectory ``positions [n, n_chain, dim]`` (time first): a CUDA
    tensor (used where it lies when float32 and contiguous; CUDA tensors come back) or a numpy array (uploaded; numpy arrays come back).
    ``max_lag``: the number of lags Geyer's sum may use (default ``n_sub``, all of them).  ``split``: the halves of every chain are the
    sub-chains (``n_sub = n // 2``; the middle row of an odd ``n`` is left out), else the whole chains.  ``n_valid``: only chains
    ``0 .. n_valid - 1`` of every row are read (a shard's padding rows; no copy).  With more than one rank the result is over the chains
    of ALL ranks, identical on each.  A coordinate that is constant in every sub-chain, or holds a non-finite value, gives NaN."""
    import torch
    ctx, sums, n_sub, m_total, host = _reduce(positions, max_lag, split, n_valid, ctx)
    rhat, ess, tau = (torch.empty(sums.shape[1], device=sums.device, dtype=torch.float32) for _ in range(3))
    ctx.chain_diag(sums, n_sub, m_total, rhat=rhat, ess=ess, tau=tau)
    if host:
        return ChainDiagnostics(rhat.cpu().numpy(), ess.cpu().numpy(), tau.cpu().numpy())
    return ChainDiagnostics(rhat, ess, tau)


def potential_scale_reduction(positions, split=True, n_valid=None, ctx=None):
    """Split-R-hat ``[dim]`` alone: ``chain_diagnostics`` with a single lag (the variances need no more), same bits as its ``rhat``."""
    import torch
    ctx, sums, n_sub, m_total, host = _reduce(positions, 1, split, n_valid, ctx)
    rhat = torch.empty(sums.shape[1], device=sums.device, dtype=torch.float32)
    ctx.chain_diag(sums, n_sub, m_total, rhat=rhat)
    return rhat.cpu().numpy() if host else rhat
