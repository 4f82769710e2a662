"""Baseline runners -- drop-in for the reference's ``exe_others.py``, for the baselines that share the MFM hot path:
adaptive tempered SMC on the MALA kernel (``exe_others.py:79-111``) and -- ``--do_svgd``, a build-side
baseline the reference's script does not run -- Stein variational gradient descent on the same particles and target gradients
(``bblackjax/vi/svgd.py``; ``mfm_svgd_step``), parallel tempering (``--do_pt``) and, for the Cox process, elliptical slice
sampling (``--do_eslice``; ``bblackjax/mcmc/elliptical_slice.py``, ``mfm_eslice_run``).  The other baselines (flowMC, pocoMC, DDS, FAB: ``:44-76,114-296``) wrap third-party
samplers outside the scope and raise.

``run(dist, args, target_gn=None) -> (res[5], res_[5])`` as ``exe_others.py:22,376``: logpdf, Stein U / V, MMD, train time
for the collected particles (the reference reports the same MCMC particles as "flow" and "exact" samples, ``:108-109``).
"""
import logging
import time

import numpy as np

from . import random as jr
from . import wandb_shim as wandb
from .bblackjax.mcmc import mala
from .bblackjax.smc import adaptive_tempered, base as smc_base, resampling
from .bblackjax import optimizers
from .bblackjax.vi import svgd as svgd_module
from .engine import Engine, allgather_cat
from .exe_flow_matching import _logprob_any, stein_disc

logger = logging.getLogger(__name__)


def run(dist, args, target_gn=None, return_extras=False):
    import torch
    logging.basicConfig(format="%(asctime)s - %(levelname)s - %(name)s - %(message)s", datefmt="%m/%d/%Y %H:%M:%S", level=logging.INFO)
    if getattr(args, "do_eslice", False):
        return run_eslice(dist, args, target_gn, return_extras)
    if getattr(args, "do_pt", False):
        return run_pt(dist, args, target_gn, return_extras)
    if getattr(args, "do_svgd", False) and not getattr(args, "do_smc", False):
        return run_svgd(dist, args, target_gn, return_extras)
    if not getattr(args, "do_smc", False):
        raise NotImplementedError("only --do_smc (adaptive tempered SMC on the MALA kernel) is built; flowMC / pocoMC / DDS / FAB "
                                  "wrap third-party samplers outside the hot-path scope (SURVEY.md section 2)")
    learning_iter, n_iter, n_chain = args.learning_iter, args.eval_iter, args.num_chain
    key_target, key_sample, key_init, key_dist, key_fourier, key_gen = jr.split(jr.PRNGKey(args.seed), 6)     # :33
    dist.initialize_model(key_dist, n_chain)                                                # :34
    eng = Engine(dist, args, None, max_eval_samples=n_iter * n_chain)
    if eng.n_valid != eng.n_local:
        raise NotImplementedError("the SMC baseline needs num_chain to be a multiple of 16 per GPU (no padding rows among the particles)")
    smc_base.attach(eng)
    real_samples = None
    if target_gn is not None:                                                               # :36-39
        key_gen, key_loss = jr.split(key_target)
        real_samples = torch.as_tensor(np.ascontiguousarray(dist.sample_rows(jr.split(key_gen, n_iter * n_chain)), dtype=np.float32), device=eng.dev)
    logger.info(f"===== Starting training seed {args.seed} w/ {learning_iter} iterations =====")
    logger.info("Adaptive tempered SMC")
    tempered = adaptive_tempered.adaptive_tempered_smc(                                     # :85-94
        dist.logprior, dist.loglik, mala.build_kernel(), mala.init, dict(step_size=args.step_size), resampling.systematic,
        args.alpha, num_mcmc_steps=args.anneal_iter // args.num_anneal_temp)
    keys = jr.split(jr.PRNGKey(args.seed), learning_iter)                                   # :101
    state = tempered.init(eng.local(dist.init_params))                                      # :102
    lmbdas = []
    train_start = time.time()
    for k in keys:                                                                          # :104 (lax.scan of one_step)
        state, info = tempered.step(k, state)
        lmbdas.append(state.lmbda)
    eng.ctx.sync()
    train_time = time.time() - train_start
    logger.info(f"Final temp= {state.lmbda}")
    keys2 = jr.split(keys[0], n_iter)                                                       # :107
    collected = []
    for k in keys2:                                                                         # :108
        state, info = tempered.step(k, state)
        collected.append(allgather_cat(state.particles.contiguous()))                        # (more than one rank: every rank evaluates ALL particles)
    flow_samples = torch.cat(collected)                                                     # :109 "not really flow but MCMC"
    exact_samples = flow_samples                                                            # :110

    logpdf = _logprob_any(eng, flow_samples).mean().item()                                  # :308
    stein = stein_disc(eng, flow_samples)
    logpdf_, stein_ = logpdf, stein                                                         # same particles (:108-109)
    if real_samples is not None:
        mmd = mmd_ = eng.ctx.max_mean_disc(real_samples, flow_samples)
    else:
        mmd = mmd_ = 0.0
    wandb.log({"train_time": train_time, "logpdf": logpdf, "KSD U-stat": stein[0], "KSD V-stat": stein[1]})
    res = np.array([logpdf, stein[0], stein[1], mmd, train_time])
    res_ = np.array([logpdf_, stein_[0], stein_[1], mmd_, train_time])
    wandb.finish()
    if return_extras:
        return res, res_, dict(lmbdas=np.array(lmbdas), state=state, engine=eng, samples=flow_samples)
    eng.close()
    return res, res_


def svgd_optimizer(args):
    """The descriptor ``--svgd_optimizer`` / ``--svgd_step_size`` name (cocob is parameter-free: the step size plays no part)."""
    kind, lr = getattr(args, "svgd_optimizer", "adagrad"), float(getattr(args, "svgd_step_size", 0.1))
    if kind not in ("sgd", "adagrad", "adam", "cocob"):
        raise ValueError(f"--svgd_optimizer must be one of sgd, adagrad, adam, cocob (got {kind!r})")
    return optimizers.cocob.cocob() if kind == "cocob" else getattr(optimizers, kind)(lr)


def run_svgd(dist, args, target_gn=None, return_extras=False):
    """``--do_svgd``: ``learning_iter`` SVGD iterations on the initial particles at beta = 1, in ONE library call (the length scale of
    every iteration comes back with it and is logged every ``--log_every``-th); ``res[5]`` in ``--do_smc``'s shape for the final particles."""
    import torch
    learning_iter, n_chain = int(args.learning_iter), int(args.num_chain)
    key_target, key_sample, key_init, key_dist, key_fourier, key_gen = jr.split(jr.PRNGKey(args.seed), 6)     # :33
    dist.initialize_model(key_dist, n_chain)                                                # :34
    eng = Engine(dist, args, None, max_eval_samples=n_chain)
    if eng.world > 1:
        eng.close()
        raise NotImplementedError("the SVGD baseline runs on one rank (every particle interacts with every other; mfm_svgd_step refuses a sharded context)")
    real_samples = None
    if target_gn is not None:                                                               # :36-39
        key_gen, key_loss = jr.split(key_target)
        real_samples = torch.as_tensor(np.ascontiguousarray(dist.sample_rows(jr.split(key_gen, n_chain)), dtype=np.float32), device=eng.dev)
    logger.info(f"===== Starting training seed {args.seed} w/ {learning_iter} iterations =====")
    logger.info(f"Stein variational gradient descent, optimizer {getattr(args, 'svgd_optimizer', 'adagrad')}")
    algo = svgd_module.svgd(dist.grad_logprob, svgd_optimizer(args))
    state = algo.init(eng.local(dist.init_params))
    train_start = time.time()
    state, length_scales = algo.step.run(state, learning_iter, keep_length_scales=True)
    eng.ctx.sync()
    train_time = time.time() - train_start
    length_scales = length_scales.cpu().numpy()
    log_every = max(1, int(getattr(args, "log_every", 1) or 1))
    for it in range(0, learning_iter, log_every):
        wandb.log({"iteration": it, "length_scale": float(length_scales[it])})
    particles = state.particles[:eng.n_valid].contiguous()
    logpdf = _logprob_any(eng, particles).mean().item()
    stein = stein_disc(eng, particles)
    mmd = eng.ctx.max_mean_disc(real_samples, particles) if real_samples is not None else 0.0
    wandb.log({"train_time": train_time, "logpdf": logpdf, "KSD U-stat": stein[0], "KSD V-stat": stein[1],
               "length_scale": float(state.kernel_parameters["length_scale"].item())})
    res = np.array([logpdf, stein[0], stein[1], mmd, train_time])
    res_ = res.copy()                                                                       # same particles, as the SMC baseline (:108-109)
    wandb.finish()
    if return_extras:
        return res, res_, dict(length_scales=length_scales, state=state, engine=eng, samples=particles)
    eng.close()
    return res, res_


def check_eslice_args(args):
    """``--do_eslice``'s argument checks, before any device work: the chain count."""
    if getattr(args, "example", "pines") != "pines":
        raise ValueError(f"--do_eslice needs --example pines (got {args.example}): elliptical slice sampling needs the Cox process's Gaussian prior factor")
    if getattr(args, "do_smc", False) or getattr(args, "do_svgd", False) or getattr(args, "do_pt", False):
        raise ValueError("--do_eslice runs alone: not with --do_smc, --do_svgd or --do_pt")
    if int(args.num_chain) < 16 or int(args.num_chain) % 16:
        raise ValueError(f"--do_eslice: num_chain ({args.num_chain}) must be a multiple of 16 (the kernel works on tiles of 16 chains)")
    return int(args.num_chain)


def run_eslice(dist, args, target_gn=None, return_extras=False):
    """``--do_eslice``: elliptical slice sampling (``bblackjax/mcmc/elliptical_slice.py``) of the Cox process at beta = 1 from the
    initial chains.  ``learning_iter`` transitions in one launch, timed as the train time, then ``eval_iter`` transitions with
    ``thin=1`` whose draws give ``res[5]`` in ``--do_smc``'s shape.  Logged: the likelihood evaluations per transition, the capped
    transitions, split R-hat and the multi-chain ESS per transition and per likelihood evaluation (the scale of a MALA step)."""
    import torch
    from . import diagnostics
    from .bblackjax.mcmc import elliptical_slice as ES
    n_chain = check_eslice_args(args)
    learning_iter, n_iter = int(args.learning_iter), int(args.eval_iter)
    key_target, key_sample, key_init, key_dist, key_fourier, key_gen = jr.split(jr.PRNGKey(args.seed), 6)     # :33
    dist.initialize_model(key_dist, n_chain)                                                # :34
    eng = Engine(dist, args, None, max_eval_samples=max(n_iter * n_chain, 16))
    if eng.world > 1 or eng.n_valid != eng.n_local:
        eng.close()
        raise NotImplementedError("the elliptical slice baseline runs on one rank with num_chain a multiple of 16")
    real_samples = None
    if target_gn is not None:                                                               # :36-39
        key_gen, key_loss = jr.split(key_target)
        real_samples = torch.as_tensor(np.ascontiguousarray(dist.sample_rows(jr.split(key_gen, n_iter * n_chain)), dtype=np.float32), device=eng.dev)
    logger.info(f"===== Starting training seed {args.seed} w/ {learning_iter} iterations =====")
    logger.info(f"Elliptical slice sampling: {n_chain} chains")
    algo = ES.elliptical_slice(dist.loglik)
    state = algo.init(eng.local(dist.init_params))
    k_train, k_eval = jr.split(key_sample)
    train_start = time.time()
    state, info = algo.step.run(k_train, state, learning_iter)
    eng.ctx.sync()
    train_time = time.time() - train_start
    state, einfo = algo.step.run(k_eval, state, n_iter, thin=1)
    mean_sub = float(einfo.mean_subiter.mean().item())
    stats = {"eslice_mean_subiter": mean_sub, "eslice_max_subiter": int(max(info.max_subiter.max().item(), einfo.max_subiter.max().item())),
             "eslice_capped": int(info.num_capped.sum().item() + einfo.num_capped.sum().item())}
    logger.info(f"Likelihood evaluations per transition (mean over the evaluation run)= {mean_sub:.3f}; capped transitions= {stats['eslice_capped']}")
    if n_iter >= 4:
        cd = diagnostics.chain_diagnostics(einfo.positions, ctx=eng.ctx)
        rhat, multi = cd.rhat.double(), cd.ess.double() / (float(n_chain) * n_iter)
        stats.update(rhat_max=rhat.max().item(), rhat_median=rhat.median().item())
        for scale, div in (("step", 1.0), ("eval", mean_sub)):
            stats.update({f"ess_multichain_per_{scale}_min": multi.min().item() / div, f"ess_multichain_per_{scale}_median": multi.median().item() / div,
                          f"ess_multichain_per_{scale}_mean": multi.mean().item() / div})
        logger.info(f"Split R-hat (max, median over coordinates)= {stats['rhat_max']:.4g}, {stats['rhat_median']:.4g}")
        logger.info("Multi-chain ESS per transition and chain (min, median, mean over coordinates)= "
                    + ", ".join(f"{stats['ess_multichain_per_step_' + k]:.4g}" for k in ("min", "median", "mean")))
    flow_samples = einfo.positions.reshape(-1, einfo.positions.shape[-1]).contiguous()       # ("not really flow but MCMC")
    logpdf = _logprob_any(eng, flow_samples).mean().item()
    stein = stein_disc(eng, flow_samples)
    mmd = eng.ctx.max_mean_disc(real_samples, flow_samples) if real_samples is not None else 0.0
    wandb.log({"train_time": train_time, "logpdf": logpdf, "KSD U-stat": stein[0], "KSD V-stat": stein[1], **stats})
    res = np.array([logpdf, stein[0], stein[1], mmd, train_time])
    res_ = res.copy()                                                                       # same particles, as the SMC baseline (:108-109)
    wandb.finish()
    if return_extras:
        return res, res_, dict(state=state, engine=eng, samples=flow_samples, stats=stats, info=info, eval_info=einfo)
    eng.close()
    return res, res_


def check_pt_args(args):
    """``--do_pt``'s argument checks, before any device work: ``(K, R)``."""
    K = int(getattr(args, "pt_temps", 8))
    if getattr(args, "do_smc", False) or getattr(args, "do_svgd", False):
        raise ValueError("--do_pt runs alone: not with --do_smc or --do_svgd")
    kern = getattr(args, "mcmc_kernel", "mala")
    if kern not in ("mala", "hmc"):
        raise ValueError(f"--do_pt takes --mcmc_kernel mala or hmc as the local move (got {kern}: NUTS and MCLMC are not served)")
    if K < 2 or int(args.num_chain) % K:
        raise ValueError(f"--do_pt: num_chain ({args.num_chain}) must be a multiple of --pt_temps ({K} >= 2): chains are R ladders of K temperatures")
    return K, int(args.num_chain) // K


def run_pt(dist, args, target_gn=None, return_extras=False):
    """``--do_pt``: parallel tempering (``bblackjax/mcmc/parallel_tempering.py``) on ``num_chain = R * K`` chains, ``K = --pt_temps``
    geometric temperatures from 1 to ``--pt_beta_min``, ``--pt_local_steps`` local steps of ``--mcmc_kernel`` (``mala`` under the textbook
    rule, or ``hmc`` with ``--hmc_steps``) per round at ``--step_size / sqrt(beta_k)``.  ``learning_iter`` rounds, timed as the train
    time, then ``eval_iter`` rounds with ``thin=1`` whose slot-0 draws give ``res[5]`` in ``--do_smc``'s shape."""
    import torch
    from . import diagnostics
    from .bblackjax.mcmc import parallel_tempering as PT
    K, R = check_pt_args(args)
    learning_iter, n_iter, n_chain = int(args.learning_iter), int(args.eval_iter), int(args.num_chain)
    key_target, key_sample, key_init, key_dist, key_fourier, key_gen = jr.split(jr.PRNGKey(args.seed), 6)     # :33
    dist.initialize_model(key_dist, n_chain)                                                # :34
    eng = Engine(dist, args, None, max_eval_samples=max(n_iter * R, 16))
    if eng.world > 1 or eng.n_valid != eng.n_local:
        eng.close()
        raise NotImplementedError("the parallel-tempering baseline runs on one rank with num_chain a multiple of 16 (mfm_pt_run refuses a sharded context)")
    real_samples = None
    if target_gn is not None:                                                               # :36-39
        key_gen, key_loss = jr.split(key_target)
        real_samples = torch.as_tensor(np.ascontiguousarray(dist.sample_rows(jr.split(key_gen, n_iter * R)), dtype=np.float32), device=eng.dev)
    betas = PT.geometric_ladder(K, float(getattr(args, "pt_beta_min", 0.01)))
    kern = getattr(args, "mcmc_kernel", "mala")
    logger.info(f"===== Starting training seed {args.seed} w/ {learning_iter} iterations =====")
    logger.info(f"Parallel tempering: {R} ladders of {K} temperatures, beta_min {betas[-1]:g}, local move {kern}")
    algo = PT.parallel_tempering(dist.logprior, dist.loglik, betas, mcmc=kern, step_size=float(args.step_size),
                                 num_integration_steps=int(getattr(args, "hmc_steps", 10)), num_mcmc_steps=int(getattr(args, "pt_local_steps", 4)),
                                 textbook=True)
    state = algo.init(eng.local(dist.init_params))
    k_train, k_eval = jr.split(key_sample)
    train_start = time.time()
    state, info = algo.step.run(k_train, state, learning_iter)
    eng.ctx.sync()
    train_time = time.time() - train_start
    state, einfo = algo.step.run(k_eval, state, n_iter, thin=1)
    rates = einfo.swap_acceptance_rate.cpu().numpy() if n_iter > 1 else info.swap_acceptance_rate.cpu().numpy()
    train_rates = info.swap_acceptance_rate.cpu().numpy()
    barrier = PT.communication_barrier(np.nan_to_num(train_rates, nan=1.0))
    logger.info("Swap acceptance rate per pair (training rounds)= " + ", ".join(f"{r:.3f}" for r in train_rates))
    logger.info(f"Communication barrier= {barrier:.4g}")
    stats = {"pt_barrier": barrier, **{f"pt_swap_rate_{k}": float(r) for k, r in enumerate(train_rates)}}
    if n_iter >= 4:
        cd = diagnostics.chain_diagnostics(einfo.positions, ctx=eng.ctx)
        rhat, multi = cd.rhat.double(), cd.ess.double() / (float(R) * n_iter)
        stats.update(rhat_max=rhat.max().item(), rhat_median=rhat.median().item(), ess_multichain_per_step_min=multi.min().item(),
                     ess_multichain_per_step_median=multi.median().item(), ess_multichain_per_step_mean=multi.mean().item())
        logger.info(f"Split R-hat of slot 0 across ladders (max, median over coordinates)= {stats['rhat_max']:.4g}, {stats['rhat_median']:.4g}")
        logger.info("Multi-chain ESS per round and ladder (min, median, mean over coordinates)= "
                    + ", ".join(f"{stats['ess_multichain_per_step_' + k]:.4g}" for k in ("min", "median", "mean")))
    flow_samples = einfo.positions.reshape(-1, einfo.positions.shape[-1]).contiguous()       # slot 0's draws ("not really flow but MCMC")
    logpdf = _logprob_any(eng, flow_samples).mean().item()
    stein = stein_disc(eng, flow_samples)
    mmd = eng.ctx.max_mean_disc(real_samples, flow_samples) if real_samples is not None else 0.0
    wandb.log({"train_time": train_time, "logpdf": logpdf, "KSD U-stat": stein[0], "KSD V-stat": stein[1], **stats})
    res = np.array([logpdf, stein[0], stein[1], mmd, train_time])
    res_ = res.copy()                                                                       # same particles, as the SMC baseline (:108-109)
    wandb.finish()
    if return_extras:
        return res, res_, dict(state=state, engine=eng, samples=flow_samples, betas=betas, swap_rates=train_rates, eval_swap_rates=rates,
                               acceptance_rate=info.acceptance_rate, stats=stats)
    eng.close()
    return res, res_
