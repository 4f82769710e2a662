"""CLI / experiment driver -- drop-in for the reference's ``multi_modal.py`` (same flags, defaults and per-example
overrides, ``multi_modal.py:21-101,147-220``), running the MFM loop on MI355X.

Additions (defaults leave the reference behaviour untouched): ``--force_dim`` / ``--force_num_chain`` override the
values ``main`` hard-codes per example (needed for BASELINE.json's phi-four d=256 / 4096-chain configuration;
``multi_modal.py:52,55`` fix 64 / 1024), ``--log_every`` sets how often metrics are copied to the host, ``--ess_steps N`` measures the effective sample size per step of the run's ``--mcmc_kernel`` after training (for ``hmc`` and ``nuts`` also per gradient evaluation; ``--mcmc_kernel nuts --max_tree_depth D`` is the No-U-turn sampler),
``--adapt_steps N --adapt_target p`` (with ``--mcmc_kernel hmc``) replaces ``--step_size`` by the result of N dual-averaging warmup steps before training (``--adapt_mass``: those steps also adapt a diagonal mass matrix, in windows; ``--mcmc_kernel nuts --nuts_adapt tree``: the warmup is the No-U-turn sampler's own, on its trees' acceptance statistic; ``--hmc_adapt chees``: the N steps are ChEES-HMC iterations, which adapt the step size and the trajectory length across the chains, and the HMC steps then make a jittered number of leapfrog steps in place of ``--hmc_steps``),
with ``--example pines`` ``--mcmc_kernel hmc``, the ``--hmc_adapt dual`` warmup and ``--ess_steps`` run on the Cox process's own HMC kernel (``mfm_cox_hmc_*``, dim <= 1024: ``--force_dim``); ``--adapt_mass``, ``--hmc_adapt chees``, ``--mcmc_kernel nuts`` and ``--do_pt`` are refused there,
``--mcmc_kernel mclmc --mclmc_L L --mclmc_integrator leapfrog|mclachlan`` takes an unadjusted microcanonical Langevin step (no accept test; ``L`` 0: ``sqrt(dim)``) per non-flow iteration and logs ``energy_var_per_dim``; with it ``--adapt_steps N`` tunes the step size and ``L`` (``mclmc_find_L_and_step_size``: ``adapted_step_size``, ``adapted_L``, ``adapt_energy_var``) and ``--ess_steps`` also divides by the 1 or 2 gradients of a step; ``--example pines``, ``--adapt_mass``, ``--hmc_adapt chees`` and ``--do_pt`` are refused with it,
``--mcmc_kernel ghmc --ghmc_alpha A --ghmc_delta D`` takes one generalized-HMC transition (one leapfrog step, persistent momentum, slice accept; ``D`` not given: ``A / 2``) per non-flow iteration; with it ``--adapt_steps N --meads_folds K --meads_shuffle S`` runs the MEADS warmup (``meads_adaptation``: ``adapted_step_size``, ``adapted_alpha``, ``adapted_inverse_mass_min`` / ``_max``, ``adapt_acceptance``) and ``--ess_steps`` logs ``ess_per_grad_*`` equal to ``ess_per_step_*``; ``--example pines``, ``--adapt_mass``, ``--hmc_adapt chees``, ``--nuts_adapt tree`` and ``--do_pt`` are refused with it,
``--ode_method rk4|euler --ode_steps N`` integrates the flow on N equal steps instead of the reference's adaptive Dopri5.
``--do_smc`` runs the tempered-SMC baseline on the same MALA kernel (``exe_others.py:79-111``); ``--do_svgd`` (with ``--svgd_optimizer sgd|adagrad|adam|cocob --svgd_step_size``) runs Stein variational gradient descent on the initial particles (``bblackjax/vi/svgd.py``, one rank); ``--do_eslice`` (``--example pines``) runs elliptical slice sampling on the Cox process (``bblackjax/mcmc/elliptical_slice.py``, one rank); the other baselines
(``--do_flowmc`` ... ``--do_fab``) wrap third-party samplers outside the hot-path scope and raise.

Multi-GPU: launch with ``python -m torch.distributed.run --nproc-per-node N -m mfm_amd.multi_modal ...``; chains are
sharded over ranks and the flow-matching gradient is all-reduced over RCCL.
"""
import argparse
import os

import numpy as np

from . import random as jr
from . import wandb_shim as wandb
from .distributions import GaussianMixture, LogGaussianCoxPines, PhiFour
from .exe_flow_matching import check_cox_args, run
from .exe_others import run as run_others


def gmm16_parameters(num_modes=16, dim=2, lim=(-16, 16)):
    """(modes, covs, weights) of the `gaussian-mixture` example, multi_modal.py:39-47 (frozen in tests/golden/gmm16_params.npz)."""
    key_mode, key_cov, key_weight = jr.split(jr.PRNGKey(0), 3)
    modes = jr.uniform(key_mode, (num_modes, dim), lim[0] * .8, lim[1] * .8)
    covs = np.exp(.5 * jr.normal(key_cov, (num_modes, dim)))
    weights = jr.dirichlet(key_weight, 4. * np.ones(num_modes))                # :45 (jax's gamma sampler restated: random.py)
    return modes, covs, weights


def main(args):
    if args.example == "gaussian-mixture":                                              # :23-47
        print("Setting up Gaussian mixture density...")
        args.dim, args.num_modes, args.lim, args.levels, args.step_size = 2, 16, [-16, 16], 20, 0.2
        dist = GaussianMixture(*gmm16_parameters(args.num_modes, args.dim, args.lim))
    elif args.example == "phi-four":                                                    # :50-63
        print("Setting up Phi four example density...")
        args.dim = 64
        args.lim, args.num_chain, args.eval_iter, args.step_size = [-1.6, 1.6], 1024, 1, 0.0001
        if args.force_dim:
            args.dim = args.force_dim
        dist = PhiFour(args.dim, bc=(getattr(args, 'phi4_bc', 'dirichlet'), getattr(args, 'phi4_bc_value', 0.0)),
                       dim_phys=getattr(args, 'phi4_dim_phys', 1))      # (a non-square dim with --phi4_dim_phys 2: ValueError)
        dist.sample_model = None
    elif args.example == "4-mode":                                                      # :65-85
        print("Setting up 4-mode Gaussian mixture density...")
        args.dim, args.lim, args.levels, args.step_size = 2, [-16, 16], 20, 0.2
        dist = GaussianMixture(8. * np.array([[1, 1], [1, -1], [-1, 1], [-1, -1]]), np.ones((4, 2)), np.ones(4) / 4)
    elif args.example == "pines":                                                       # :87-98
        print("Setting up Log Gaussian Cox density...")
        args.dim, args.lim, args.num_chain, args.eval_iter, args.step_size = 1600, None, 128, 1, 0.01
        args.hidden_x = args.hidden_t = args.hidden_xt = [1024, 1024]
        if args.force_dim:
            args.dim = args.force_dim
        dist = LogGaussianCoxPines(args.dim)
        dist.sample_model = None
    else:
        raise Exception("Example not found.")
    if args.force_num_chain:
        args.num_chain = args.force_num_chain
    if args.do_flowmc or args.do_pocomc or args.do_dds or args.do_fab:
        raise NotImplementedError("the flowMC / pocoMC / DDS / FAB runners (exe_others.py) wrap third-party samplers outside the "
                                  "hot-path scope (SURVEY.md section 2); --do_smc (tempered SMC on the MALA kernel) is built")

    if "RANK" in os.environ and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import torch
        import torch.distributed as td
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        if not td.is_initialized():
            td.init_process_group("nccl")

    N_PARAM = args.dim
    job_type = "mcmc_per_flow_steps=" + str(args.mcmc_per_flow_steps) + ",learning_iter=" + str(args.learning_iter) + (",hutchs" if args.hutchs else "")
    if getattr(args, "do_eslice", False):
        from .exe_others import check_eslice_args
        check_eslice_args(args)                                                         # (before any device work)
        job_type = "Elliptical slice sampling"
    elif getattr(args, "do_pt", False):
        from .exe_others import check_pt_args
        check_pt_args(args)                                                             # (before any device work)
        job_type = "Parallel tempering"
    elif args.do_smc:
        job_type = "Adaptive tempered SMC"                                              # :110-111
    elif args.do_svgd:
        job_type = "SVGD"
    check_cox_args(dist, args)                                                          # (--example pines: before any device work, after the baselines' own checks)
    seeds = [args.seed] if args.seed else [i ** 10 for i in range(10)]                  # :118
    res, res_ = [], []
    for seed in seeds:
        args.seed = seed
        wandb.init(project=args.example, config=args, group="dim=" + str(N_PARAM), job_type=job_type)
        if args.do_smc or args.do_svgd or getattr(args, "do_pt", False) or getattr(args, "do_eslice", False):
            _res, _res_ = run_others(dist, args, dist.sample_model)                     # :126-127
        else:
            _res, _res_ = run(dist, args, dist.sample_model, log_every=args.log_every)  # :129
        res.append(_res); res_.append(_res_)
    res, res_ = np.array(res), np.array(res_)
    print(job_type)
    print("-" * 100)
    print("logprob\t & stein-u\t & stein-v\t & mmd  \t & time \t")
    print(*[f"{m:.2e} \\pm {s * 1.96:.2e}" for m, s in zip(res.mean(0), res.std(0))], sep="$ & $")
    print(*[f"{m:.2e} \\pm {s * 1.96:.2e}" for m, s in zip(res_.mean(0), res_.std(0))], sep="$ & $")
    print("-" * 100)
    return res, res_


def build_parser():
    parser = argparse.ArgumentParser()                                                  # :148-219, same defaults
    parser.add_argument("--seed", type=int, default=None)
    parser.add_argument('--dim', type=int, default=64)
    parser.add_argument('--num_modes', type=int, default=16)
    parser.add_argument("--example", type=str, default="pines")
    parser.add_argument("--sigma", type=float, default=1e-4)
    parser.add_argument("--fourier_dim", type=int, default=128)
    parser.add_argument("--fourier_std", type=float, default=1.0)
    parser.add_argument('--hutchs', dest='hutchs', action='store_true')
    parser.set_defaults(hutchs=False)
    parser.add_argument("--ref_dist", type=str, default='stdgauss')
    parser.add_argument('--cond_flow', dest='cond_flow', action='store_true')
    parser.set_defaults(cond_flow=True)
    parser.add_argument('--ot_cond_flow', dest='ot_cond_flow', action='store_true')
    parser.set_defaults(ot_cond_flow=False)
    parser.add_argument("--num_importance_samples", type=int, default=0)
    parser.add_argument("--mcmc_per_flow_steps", type=float, default=10)
    parser.add_argument('--num_chain', type=int, default=128)
    parser.add_argument("--learning_iter", type=int, default=400)
    parser.add_argument("--eval_iter", type=int, default=100)
    parser.add_argument("--alpha", type=float, default=0.95)
    parser.add_argument("--anneal_iter", type=int, default=200)
    parser.add_argument('--num_anneal_temp', type=int, default=200)
    parser.add_argument('--non_linearity', type=str, default='relu')
    parser.add_argument('--hidden_x', type=int, nargs='+', default=[128, 128])
    parser.add_argument('--hidden_t', type=int, nargs='+', default=[128, 128])
    parser.add_argument('--hidden_xt', type=int, nargs='+', default=[128, 128])
    parser.add_argument('--step_size', type=float, default=0.2)
    for flag in ("flowmc", "pocomc", "dds", "smc", "fab"):
        parser.add_argument(f'--do_{flag}', dest=f'do_{flag}', action='store_true')
        parser.set_defaults(**{f'do_{flag}': False})
    parser.add_argument('--learning_rate', type=float, default=1e-3)
    parser.add_argument('--weight_decay', type=float, default=0.0001)
    parser.add_argument('--adam_beta1', type=float, default=0.9)
    parser.add_argument('--adam_beta2', type=float, default=0.999)
    parser.add_argument('--adam_epsilon', type=float, default=1e-8)
    parser.add_argument('--gradient_clip', type=float, default=1.0)
    parser.add_argument('--warmup_steps', type=int, default=0)
    parser.add_argument('--rtol', type=float, default=1e-5)
    parser.add_argument('--atol', type=float, default=1e-5)
    parser.add_argument('--mxstep', type=float, default=1_000)
    parser.add_argument('--lim', type=float, nargs=2, default=[-16, 16])
    parser.add_argument('--grid_width', type=int, default=400)
    parser.add_argument('--levels', type=int, default=50)
    parser.add_argument('--check', dest='check', action='store_true')
    parser.set_defaults(check=False)
    # build-side additions
    parser.add_argument('--force_dim', type=int, default=None)
    parser.add_argument('--force_num_chain', type=int, default=None)
    parser.add_argument('--log_every', type=int, default=1)
    # the fixed-step mode of the CNF solver (BASELINE.json's "RK4/Euler ODE integrator"; the reference integrates with the adaptive
    # Dopri5 of jax.experimental.ode.odeint, exe_flow_matching.py:345-349, which stays the default): --ode_method rk4 --ode_steps 64
    parser.add_argument('--ode_method', type=str, default='dopri5', choices=['dopri5', 'rk4', 'euler'])
    parser.add_argument('--ode_steps', type=int, default=0)
    # the MCMC move of a non-flow iteration: the reference's MALA step (exe_flow_matching.py:313), or -- BASELINE.json's "MALA/HMC" step,
    # not in the reference -- an HMC step of --hmc_steps velocity-Verlet steps of size --step_size (mfm_amd/bblackjax/mcmc/hmc.py)
    parser.add_argument('--mcmc_kernel', type=str, default='mala', choices=['mala', 'hmc', 'nuts', 'mclmc', 'ghmc'])
    parser.add_argument('--hmc_steps', type=int, default=10)
    # 'nuts': a No-U-turn transition of step size --step_size whose tree doubles at most --max_tree_depth times (mfm_amd/bblackjax/mcmc/nuts.py)
    parser.add_argument('--max_tree_depth', type=int, default=10)
    # 'mclmc': an unadjusted microcanonical Langevin step of size --step_size (mfm_amd/bblackjax/mcmc/mclmc.py): no accept test; --mclmc_L is
    # the momentum decoherence length (0: sqrt(dim)), --mclmc_integrator the schedule (one or two gradients per step).  --adapt_steps N
    # tunes step size and L (mclmc_find_L_and_step_size); not with --example pines, --adapt_mass, --hmc_adapt chees or --do_pt
    parser.add_argument('--mclmc_L', type=float, default=0.0)
    parser.add_argument('--mclmc_integrator', type=str, default='mclachlan', choices=['leapfrog', 'mclachlan'])
    # 'ghmc': a generalized-HMC transition (mfm_amd/bblackjax/mcmc/ghmc.py): ONE leapfrog step of size --step_size, the momentum refreshed
    # at rate --ghmc_alpha in (0, 1] and kept across transitions, a slice accept drifting by --ghmc_delta (not given: alpha / 2).
    # --adapt_steps N runs the MEADS warmup (meads_adaptation) over --meads_folds folds of the chains, redrawn every --meads_shuffle
    # iterations (0: never); not with --example pines, --adapt_mass, --hmc_adapt chees, --nuts_adapt tree or --do_pt
    parser.add_argument('--ghmc_alpha', type=float, default=0.5)
    parser.add_argument('--ghmc_delta', type=float, default=None)
    parser.add_argument('--meads_folds', type=int, default=4)
    parser.add_argument('--meads_shuffle', type=int, default=0)
    # the phi-four lattice's boundary (distributions.py:114-139; the reference's main script builds Dirichlet 0): both ends held at
    # --phi4_bc_value, or a periodic ring (--phi4_bc pbc; the value is ignored)
    parser.add_argument('--phi4_bc', type=str, default='dirichlet', choices=['dirichlet', 'pbc'])
    parser.add_argument('--phi4_bc_value', type=float, default=0.0)
    # the phi-four field's physical dimension: 1 = the chain of the reference's main script, 2 = an L x L lattice in row-major order
    # (dim = L * L must be a perfect square; coefficient a * L, the boundary on both axes)
    parser.add_argument('--phi4_dim_phys', type=int, default=1, choices=[1, 2])
    # after training: N more MALA steps from the final chains at beta = 1 in one launch, and the effective sample size per step of that
    # trajectory (mcmc_utils.effective_sample_size) logged as ess_per_step_min / _median / _mean; 0: nothing happens
    parser.add_argument('--ess_steps', type=int, default=0)
    # before training (--mcmc_kernel hmc only): N HMC warmup steps on a COPY of the initial chains at beta = 1, every chain adapting its own
    # step size from --step_size by dual averaging towards the acceptance probability --adapt_target; the pooled result replaces
    # --step_size for the rest of the run (exe_flow_matching.adapt_step_size); 0: nothing happens.  (--warmup_steps is the learning rate's.)
    parser.add_argument('--adapt_steps', type=int, default=0)
    parser.add_argument('--adapt_target', type=float, default=0.8)
    # with --adapt_steps N: the N steps run the window adaptation (bblackjax/adaptation/window_adaptation.py) instead of the single warmup --
    # step size AND a diagonal mass matrix, which the training loop's HMC steps and --ess_steps then use
    parser.add_argument('--adapt_mass', action='store_true')
    # with --mcmc_kernel nuts --adapt_steps N: 'hmc' runs the HMC warmup with --hmc_steps leapfrog steps and hands its step size (and mass) to
    # NUTS; 'tree' runs NUTS's own warmup under --max_tree_depth, adapting on the trees' acceptance statistic (--hmc_steps plays no part)
    parser.add_argument('--nuts_adapt', type=str, default='hmc', choices=['hmc', 'tree'])
    # with --mcmc_kernel hmc --adapt_steps N: 'dual' is the per-chain dual-averaging warmup above; 'chees' runs N ChEES-HMC iterations
    # (bblackjax/adaptation/chees_adaptation.py), which adapt the step size AND the trajectory length across the chains: the HMC steps then
    # make a jittered number of leapfrog steps in place of --hmc_steps (not with --adapt_mass)
    parser.add_argument('--hmc_adapt', type=str, default='dual', choices=['dual', 'chees'])
    # the SVGD baseline (exe_others.run_svgd): --learning_iter iterations of Stein variational gradient descent on the initial particles at
    # beta = 1 under the named optimizer (bblackjax/optimizers); cocob is parameter-free and ignores --svgd_step_size
    parser.add_argument('--do_svgd', dest='do_svgd', action='store_true')
    parser.set_defaults(do_svgd=False)
    parser.add_argument('--svgd_optimizer', type=str, default='adagrad', choices=['sgd', 'adagrad', 'adam', 'cocob'])
    parser.add_argument('--svgd_step_size', type=float, default=0.1)
    # the parallel-tempering baseline (exe_others.run_pt): num_chain = R ladders x --pt_temps temperatures, geometric from 1 to --pt_beta_min,
    # --pt_local_steps local steps of --mcmc_kernel mala|hmc (--hmc_steps, --step_size / sqrt(beta)) per round, then one even-odd exchange sweep
    parser.add_argument('--do_pt', dest='do_pt', action='store_true')
    parser.set_defaults(do_pt=False)
    parser.add_argument('--pt_temps', type=int, default=8)
    parser.add_argument('--pt_beta_min', type=float, default=0.01)
    parser.add_argument('--pt_local_steps', type=int, default=4)
    # the elliptical slice baseline (exe_others.run_eslice; --example pines only): --learning_iter transitions of every chain at beta = 1 in one
    # launch, then --eval_iter kept ones; no step size and no gradient (mfm_amd/bblackjax/mcmc/elliptical_slice.py)
    parser.add_argument('--do_eslice', dest='do_eslice', action='store_true')
    parser.set_defaults(do_eslice=False)
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
