"""ESS per gradient evaluation of the HMC kernel under unit mass and under the adapted diagonal mass matrix, each at its OWN adapted
step size, on two targets: the anisotropic Gaussian of tests/test_gpu_hmc_mass.py (one mode, d = 4, variances 0.04, 1, 25, 0.25) and
phi-four d = 64.  Both 1024 chains, L leapfrog steps (`--leapfrog`, default 8 and 3), 300 warmup steps from the same start and key:

* unit mass: ``kernel.warmup`` (one launch of dual averaging), the pooled step size;
* adapted mass: ``window_adaptation`` (step size and mass on Stan's schedule);

then `--steps` steps in one launch from the warmed-up chains (``kernel.run``, thin = 1) and Geyer's effective sample size of every
chain and coordinate (``mcmc_utils.effective_sample_size``), over steps x L: min / median / mean, and the mean per coordinate for d = 4.

L = 8 is the setting of the adaptation's test.  On the whitened Gaussian it is also a resonance: the adapted step size (0.79) times 8 is
2 pi, one full period of every coordinate, so a trajectory ends where it began; L = 3 shows the same mass away from it.

    python tools/hmc_mass_ess.py [--steps 1000] [--leapfrog 8 3] [--out profiles/hmc_mass_ess.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

N_CHAIN, N_WARM = 1024, 300
VAR = np.array([0.04, 1.0, 25.0, 0.25])


def target(name):
    from mfm_amd import distributions as D, random as jr
    from oracle import loop
    small = dict(fourier_dim=16, hidden_x=[32, 32], hidden_t=[32, 32], hidden_xt=[32, 32])
    if name == "gauss4":
        dist = D.GaussianMixture(np.zeros((1, 4)), VAR[None], np.ones(1))
        dist.dim = 4
        x0 = (jr.normal_rows(jr.split(jr.PRNGKey(1), N_CHAIN), 4) * np.sqrt(VAR)).astype(np.float32)
        return dist, loop.default_args(example="gaussian-mixture", dim=4, num_chain=N_CHAIN, **small), x0, 0.05
    dist = D.PhiFour(64)
    dist.initialize_model(jr.PRNGKey(3), N_CHAIN)
    return dist, loop.default_args(example="phi-four", dim=64, num_chain=N_CHAIN, hutchs=True, **small), dist.init_params.astype(np.float32), 0.02


def measure(name, n_steps, L):
    import torch
    from mfm_amd import mcmc_utils, random as jr
    from mfm_amd.bblackjax.adaptation.window_adaptation import window_adaptation
    from mfm_amd.bblackjax.mcmc import hmc as H
    from mfm_amd.engine import Engine
    dist, args, x0, step0 = target(name)
    eng = Engine(dist, args, None)
    state = H.init(torch.as_tensor(x0).cuda(), dist.logprob)
    k_warm, k_run = jr.split(jr.PRNGKey(0), 2)
    lines = []
    for mode in ("unit", "adapted"):
        if mode == "unit":
            warm, info = H.hmc(dist.logprob, step0, L).step.warmup(k_warm, state, N_WARM)
            step, minv = info.pooled_step_size, None
        else:
            warm, params, _ = window_adaptation(dist.logprob, L, step0).run(k_warm, state, N_WARM)
            step, minv = params["step_size"], params["inverse_mass_matrix"]
        _, run = H.hmc(dist.logprob, step, L, minv).step.run(k_run, warm, n_steps, thin=1)
        ess, _ = mcmc_utils.effective_sample_size(run.positions[:, :eng.n_valid], ctx=eng.ctx)
        per_grad = ess.double() / (n_steps * L)
        text = (f"  {mode:8s} step size {step:.5f}, mean acceptance {run.acceptance_rate.mean().item():.3f}: ESS per gradient min {per_grad.min().item():.4g}, "
                f"median {per_grad.median().item():.4g}, mean {per_grad.mean().item():.4g}")
        if minv is not None:
            text += f"; inverse mass min {minv.min():.4g}, max {minv.max():.4g}"
        if per_grad.shape[1] <= 8:
            text += "; mean per coordinate " + ", ".join(f"{v:.4g}" for v in per_grad.mean(0).tolist())
            if minv is not None:
                text += "; inverse mass " + ", ".join(f"{v:.4g}" for v in minv)
        lines.append(text)
    eng.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--leapfrog", type=int, nargs="+", default=[8, 3])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"ESS per gradient evaluation, {N_CHAIN} chains, {N_WARM} warmup steps, then {a.steps} steps"]
    for name, title in (("gauss4", "Gaussian d = 4, variances 0.04, 1, 25, 0.25"), ("phi4", "phi-four d = 64")):
        for L in a.leapfrog:
            lines.append(f"{title}, L = {L}")
            lines += measure(name, a.steps, L)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
