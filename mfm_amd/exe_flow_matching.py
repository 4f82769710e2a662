"""MFM training loop and its building blocks -- drop-in for the reference's ``exe_flow_matching.py`` on MI355X.

Keeps the reference's names and call shapes (``VectorFieldNet``, ``create_train_state``, ``create_learning_rate_fn``,
``create_train_data_gn -> (train_data_generator, init_fn, transform_and_logdet)``, ``run(dist, args, target_gn)``;
``exe_flow_matching.py:56-90,93-198,201-318,321-561``) while every array operation of the hot loop (``:432-449``) runs
in hand-written HIP kernels behind the C ABI (``include/mfm.h``).  What changes at the boundary is listed in
INTEGRATION.md: arrays are CUDA tensors batched over chains (the reference batches with ``jax.vmap``), parameters
and optimizer state live on the device (``state.params`` copies them back on demand), and ``jax.random`` keys are
uint32[2] NumPy arrays with the same split conventions.
"""
import logging
import time
from typing import Callable

import numpy as np

from . import random as jr
from . import wandb_shim as wandb
from ._lib import FLOW_IMH, FLOW_RWMH
from .bblackjax.mcmc.mala import MALAInfo, MALAState, build_kernel, init  # noqa: F401  (same import as :28)
from .distributions import IndepGaussian
from .engine import Engine, allgather_cat, allreduce_sum_

logger = logging.getLogger(__name__)

non_lins = {"tanh": "tanh", "elu": "elu", "relu": "relu", "gelu": "gelu", "swish": "swish"}     # :39-45 (names: evaluated in the kernels)
def _dead_ref(name):
    def make(dim):
        raise NotImplementedError(f"ref_dist={name!r} cannot be constructed in the reference either (exe_flow_matching.py:48-54: "
                                  "GaussianMixture(dim) / FlatDistribution.sample_model / PhiFourBase do not fit their call sites)")
    return make


ref_dists = {"stdgauss": lambda dim: IndepGaussian(dim), "widegauss": lambda dim: IndepGaussian(dim, var=5.),      # :48-54
             "bimodal": _dead_ref("bimodal"), "flat": _dead_ref("flat"), "phifour": _dead_ref("phifour")}


# ---- parameters: flax-style pytree <-> canonical flat vector (include/mfm.h) ---------------------------------------
def layer_shapes(dim, fourier_dim, hidden_x, hidden_t, hidden_xt):
    """(in, out) of the Dense layers in flax creation order (``exe_flow_matching.py:74-86``): the time branch, the x branch, the
    gate, the joint branch, the output; the hidden lists have any length >= 1."""
    shapes, prev = [], 2 * fourier_dim
    for h in hidden_t:
        shapes.append((prev, h)); prev = h
    ht, prev = prev, dim
    for h in hidden_x:
        shapes.append((prev, h)); prev = h
    hx = prev
    shapes.append((ht, dim))
    prev = hx + ht
    for h in hidden_xt:
        shapes.append((prev, h)); prev = h
    shapes.append((prev, dim))
    return shapes


def flatten_params(params):
    p = params["params"]
    return np.concatenate([np.concatenate([np.asarray(p[f"Dense_{i}"]["kernel"], np.float32).reshape(-1),
                                           np.asarray(p[f"Dense_{i}"]["bias"], np.float32).reshape(-1)])
                           for i in range(len(p))])


def unflatten_params(flat, shapes):
    out, o = {}, 0
    for i, (fi, fo) in enumerate(shapes):
        W = flat[o:o + fi * fo].reshape(fi, fo); o += fi * fo
        b = flat[o:o + fo]; o += fo
        out[f"Dense_{i}"] = {"kernel": W.copy(), "bias": b.copy()}
    return {"params": out}


class VectorFieldNet:
    """``exe_flow_matching.py:56-90``.  ``grad_logporob`` is ``dist.grad_logprob`` (the reference passes
    ``jax.grad(dist.logprob)``, :351); the gradient is evaluated inside the kernels."""

    def __init__(self, fourier_random, grad_logporob, hidden_x, hidden_t, hidden_xt, act_fn="relu", grad_clip=None):
        if act_fn not in non_lins:
            raise NotImplementedError(f"unknown activation {act_fn!r}")
        self.fourier_random = np.asarray(fourier_random, dtype=np.float64)
        self.dist = getattr(grad_logporob, "__self__", None)
        if self.dist is None:
            raise NotImplementedError("grad_logporob must be dist.grad_logprob of a built target")
        self.hidden_x, self.hidden_t, self.hidden_xt = list(hidden_x), list(hidden_t), list(hidden_xt)
        self.grad_clip = grad_clip
        self.engine = None

    def shapes(self):
        return layer_shapes(self.dist.dim, len(self.fourier_random), self.hidden_x, self.hidden_t, self.hidden_xt)

    def init(self, rng_key, x=None, t=None):
        """flax ``Module.init``: lecun_normal kernels, zero biases, ZERO gate / output kernels (:81,86), float32."""
        shapes = self.shapes()
        keys = jr.split(rng_key, len(shapes))
        out = {}
        gate = len(self.hidden_t) + len(self.hidden_x)
        for i, (fi, fo) in enumerate(shapes):
            if i in (gate, len(shapes) - 1):
                W = np.zeros((fi, fo), np.float32)
            else:
                W = (jr.truncated_normal(keys[i], -2.0, 2.0, (fi, fo)) * np.sqrt(1.0 / fi) / 0.87962566103423978).astype(np.float32)
            out[f"Dense_{i}"] = {"kernel": W, "bias": np.zeros(fo, np.float32)}
        return {"params": out}

    def attach(self, engine):
        self.engine = engine
        return self

    def apply(self, params, x, t):
        """v(x, t) for CUDA tensors x [n, d], t [n] (n multiple of 16)."""
        eng = self.engine
        _maybe_upload(eng, params)
        v = eng.torch.empty_like(x)
        eng.ctx.vf_apply(x, t, v)
        return v


class DeviceParams:
    """Handle for the parameters resident in the device context (what ``state.params`` is during training)."""

    def __init__(self, engine, shapes):
        self.engine, self.shapes = engine, shapes

    def to_host(self):
        return unflatten_params(self.engine.ctx.get_params(), self.shapes)


def _maybe_upload(engine, params):
    if isinstance(params, DeviceParams) or params is None:
        return
    engine.ctx.set_params(flatten_params(params))


def create_learning_rate_fn(num_train_steps, num_warmup_steps: int, learning_rate: float) -> Callable:
    """``exe_flow_matching.py:189-198`` (evaluated on the device by the optimizer kernel; this is the host twin)."""
    def schedule_fn(step):
        step = float(step)
        if num_warmup_steps > 0 and step < num_warmup_steps:
            return learning_rate * step / num_warmup_steps
        ts = num_train_steps - num_warmup_steps
        if ts <= 0:
            return learning_rate
        return learning_rate * (1.0 - min(max(step - num_warmup_steps, 0.0), ts) / ts)
    return schedule_fn


class TrainState:
    """``flax.training.train_state.TrainState`` twin (:101-110,181-186): parameters, AdamW moments and the step
    counters live in the device context; ``apply_gradients`` runs the fused apply_if_finite/AdamW/clip kernel."""

    def __init__(self, engine, apply_fn, shapes):
        self.engine, self.apply_fn = engine, apply_fn
        self.params = DeviceParams(engine, shapes)

    @property
    def step(self):
        return self.engine.ctx.opt_state()["step"]

    def loss_fn(self, rng_key, samples, params=None):
        """flow_matching_loss (:171-178) on CUDA samples [n, d]; returns a 1-element float64 CUDA tensor."""
        _maybe_upload(self.engine, params)
        return self.engine.eval_loss(rng_key, samples)

    def apply_gradients(self, grads):
        self.engine.ctx.adamw_step(grads)
        return self


def create_train_state(vector_field_apply, vector_field_param, learning_rate_fn, args) -> TrainState:
    """``exe_flow_matching.py:93-186``.  The optimizer hyper-parameters were given to the engine with ``args``."""
    model = vector_field_apply.__self__
    eng = model.engine
    eng.ctx.set_params(flatten_params(vector_field_param))
    eng.ctx.reset_optimizer()
    return TrainState(eng, vector_field_apply, model.shapes())


def create_train_data_gn(dist, vector_field_apply, ode_integrator, args):
    """``exe_flow_matching.py:201-318``.  ``ode_integrator`` is accepted for signature parity; the integrator is the
    in-kernel Dopri5 with the reference's rtol / atol / mxstep (given to the engine with ``args``)."""
    model = vector_field_apply.__self__
    eng = model.engine
    t = eng.torch
    n_is = int(args.num_importance_samples)
    mode = FLOW_IMH if n_is < 0 else FLOW_RWMH                                             # :298
    ref_dist = ref_dists[getattr(args, "ref_dist", "stdgauss")](args.dim)                  # :244
    n, d = eng.n_local, eng.dim
    info = dict(acc=t.empty(n, device=eng.dev, dtype=t.float32), isacc=t.empty(n, device=eng.dev, dtype=t.uint8),
                prop=t.empty(n, d, device=eng.dev, dtype=t.float32), w=t.zeros(n, device=eng.dev, dtype=t.float32),
                nsteps=t.zeros(n, device=eng.dev, dtype=t.int32))

    def transform_and_logdet(key, ref_sample, vector_field_param=None):
        """:206-221, batched over samples with ONE shared Hutchinson key (as used at :455)."""
        _maybe_upload(eng, vector_field_param)
        out = t.empty_like(ref_sample)
        ldj = t.empty(ref_sample.shape[0], device=eng.dev, dtype=t.float32)
        eng.ctx.ode_transform(1, ref_sample, out, ldj, key=key)
        return out, ldj

    def _keys_dev(k):
        return t.as_tensor(np.ascontiguousarray(k, dtype=np.uint32).view(np.int32), device=eng.dev)

    def conditional_importance_sampling(rng_key, beta, pos, logp):
        """:280-296.  The solves and target evaluations are the kernels the other flow steps use; the per-chain
        weights, the categorical draw and the state update run in ``mfm_cis_select``."""
        if eng.n_valid != eng.n_local:
            raise NotImplementedError("num_importance_samples > 0 with a chain count that is not a multiple of 16 per GPU")
        keys = jr.split(rng_key, eng.n_total)[eng.offset:eng.offset + n]                   # :303
        kk = jr.split_rows(keys, 4)                                                        # :281
        u0 = t.empty_like(pos); vol0 = t.empty(n, device=eng.dev, dtype=t.float32)
        eng.ctx.ode_transform(-1, pos, u0, vol0, keys=_keys_dev(kk[:, 1]))                  # :282
        ks = jr.split_rows(kk[:, 0], n_is).reshape(n * n_is, 2)                            # :284
        kh = jr.split_rows(kk[:, 2], n_is).reshape(n * n_is, 2)                            # :286
        refs = t.empty(n * n_is, d, device=eng.dev, dtype=t.float32)
        eng.ctx.normal_rows(_keys_dev(ks), refs)                                           # :285
        if ref_dist.std != 1.0 or ref_dist.mean != 0.0:
            refs.mul_(float(ref_dist.std)).add_(float(ref_dist.mean))                      # distributions.py:96-97
        xs = t.empty_like(refs); vols = t.empty(n * n_is, device=eng.dev, dtype=t.float32)
        eng.ctx.ode_transform(1, refs, xs, vols, keys=_keys_dev(kh))                        # :287
        lps = _logprob_any(eng, xs, beta=beta)                                             # :288
        eng.ctx.cis_select(rng_key, n_is, u0, vol0, refs, xs, vols, lps, pos, logp, info["acc"], info["isacc"], info["prop"], info["w"])

    use_hmc = getattr(args, "mcmc_kernel", "mala") == "hmc"
    use_nuts = getattr(args, "mcmc_kernel", "mala") == "nuts"
    hmc_step = eng.ctx.cox_hmc_step if getattr(dist, "kind", None) == "lgcp" else eng.ctx.hmc_step      # (by target, as bblackjax.mcmc.hmc)
    if use_nuts:
        info["nuts_acc"] = t.empty(n, device=eng.dev, dtype=t.float64)
    use_mclmc = getattr(args, "mcmc_kernel", "mala") == "mclmc"
    if use_mclmc:
        from .bblackjax.mcmc.mclmc import integrator_id
        mclmc_integrator = integrator_id(getattr(args, "mclmc_integrator", "mclachlan"))
        info["mclmc_de"] = t.empty(n, device=eng.dev, dtype=t.float64)
        eng.mclmc_momentum = None                      # [n, d] float64 unit momenta, drawn at the first MCLMC step and kept by the engine
        eng.mclmc_energy = t.zeros(2, device=eng.dev, dtype=t.float64)      # sum dE, sum dE^2 over the run's MCLMC steps (this rank's chains)
        eng.mclmc_energy_count = 0                     # ... and how many terms they hold (host: n_valid per step)

    def mclmc_train_step(rng_key, beta, pos, logp, grad):
        """Build-side mode (--mcmc_kernel mclmc): one MCLMC step (mfm_mclmc_step).  It always moves; a flow step between two of them
        replaces x and keeps u, which is valid: the stationary law is p(x) x uniform(u)."""
        if eng.mclmc_momentum is None:
            eng.mclmc_momentum = t.empty(pos.shape, device=eng.dev, dtype=t.float64)
            eng.ctx.mclmc_init(jr.split(rng_key)[1], eng.mclmc_momentum)
        de = info["mclmc_de"]
        eng.ctx.mclmc_step(rng_key, beta, args.step_size, mclmc_L(args), mclmc_integrator, pos, logp, grad, eng.mclmc_momentum, energy_change=de)
        v = de[:eng.n_valid]
        eng.mclmc_energy += t.stack([v.sum(), (v * v).sum()])
        eng.mclmc_energy_count += int(eng.n_valid)
        info["acc"].fill_(1); info["isacc"].fill_(1)

    use_ghmc = getattr(args, "mcmc_kernel", "mala") == "ghmc"
    if use_ghmc:
        info["ghmc_de"] = t.empty(n, device=eng.dev, dtype=t.float64)
        eng.ghmc_momentum = eng.ghmc_slice = None      # [n, d] / [n] float64, drawn at the first GHMC transition and kept by the engine

    def ghmc_train_step(rng_key, beta, pos, logp, grad):
        """Build-side mode (--mcmc_kernel ghmc): one GHMC transition (mfm_ghmc_step) at --step_size / --ghmc_alpha / --ghmc_delta and the
        inverse mass the MEADS warmup left (args.ghmc_inverse_mass; None: unit metric).  The engine keeps p and s; a flow move between
        two transitions replaces x only, which is valid: the stationary law is p(x) N(p; 0, M) uniform(s)."""
        minv = getattr(args, "ghmc_inverse_mass", None)
        if eng.ghmc_momentum is None:
            eng.ghmc_momentum = t.empty(pos.shape, device=eng.dev, dtype=t.float64)
            eng.ghmc_slice = t.empty(pos.shape[0], device=eng.dev, dtype=t.float64)
            eng.ctx.ghmc_init(jr.split(rng_key)[1], eng.ghmc_momentum, eng.ghmc_slice, minv)
        eng.ctx.ghmc_step(rng_key, beta, args.step_size, ghmc_alpha(args), ghmc_delta(args), pos, logp, grad, eng.ghmc_momentum, eng.ghmc_slice, minv,
                          info["acc"], info["isacc"], info["ghmc_de"])

    def train_data_generator(rng_key, states, count, vector_field_param=None, beta=1.0):
        """:300-314.  States are updated IN PLACE (and returned); infos are views of reused device buffers."""
        _maybe_upload(eng, vector_field_param)
        K = args.mcmc_per_flow_steps
        if 0 < K < 1:
            do_flow = count % (int(1 / K) + 1) != 0                                        # :304-309
        else:
            do_flow = count % (int(K) + 1) == 0                                            # :311
        pos, logp, grad = states
        if do_flow and n_is > 0:
            conditional_importance_sampling(rng_key, beta, pos, logp)
        elif do_flow:
            eng.ctx.flow_step(mode, rng_key, beta, pos, logp, grad, info["acc"], info["isacc"], info["prop"], info["nsteps"])
        elif use_hmc:          # build-side mode (--mcmc_kernel hmc): the iteration's MCMC move is an HMC step (mfm_hmc_step; the Cox process: mfm_cox_hmc_step) instead of :313
            hmc_step(rng_key, beta, args.step_size, hmc_num_steps(args, count), pos, logp, grad, info["acc"], info["isacc"])
        elif use_nuts:         # build-side mode (--mcmc_kernel nuts): a No-U-turn transition (mfm_nuts_step); it always takes its tree's proposal
            eng.ctx.nuts_step(rng_key, beta, args.step_size, int(getattr(args, "max_tree_depth", 10)), pos, logp, grad, acceptance_rate=info["nuts_acc"])
            info["acc"].copy_(info["nuts_acc"]); info["isacc"].fill_(1)
        elif use_mclmc:
            mclmc_train_step(rng_key, beta, pos, logp, grad)
        elif use_ghmc:
            ghmc_train_step(rng_key, beta, pos, logp, grad)
        else:
            eng.ctx.mala_step(rng_key, beta, args.step_size, pos, logp, grad, info["acc"], info["isacc"], info["prop"], info["w"])
        return MALAState(pos, logp, grad), MALAInfo(info["acc"], info["isacc"], info["prop"], info["w"])

    def init_fn(init_positions, beta=1.0):
        """:316."""
        pos = init_positions
        logp = t.empty(pos.shape[0], device=eng.dev, dtype=t.float64)
        grad = t.empty_like(pos)
        eng.ctx.mala_init(pos, beta, logp, grad)
        return MALAState(pos, logp, grad)

    train_data_generator.info_buffers = info
    # what run() needs to issue generator + train_step as ONE library call (mfm_train_iter) where that is the same computation
    train_data_generator.flow_mode = mode
    train_data_generator.one_call_ok = n_is <= 0 and args.mcmc_per_flow_steps >= 1 and float(args.mcmc_per_flow_steps).is_integer() and not use_hmc and not use_nuts and not use_mclmc and not use_ghmc
    return train_data_generator, init_fn, transform_and_logdet


def _finish_metric_rows(eng, metrics, lo, hi):
    """Rows [lo, hi) of the per-iteration metrics hold per-rank partial sums (loss, sum acc, sum acc^2, target loss):
    sum them over ranks in one collective (off the per-iteration critical path) and turn the acceptance sums into the
    mean / population std logged at exe_flow_matching.py:442-443."""
    if hi <= lo:
        return
    rows = metrics[lo:hi]
    allreduce_sum_(rows)
    mean = rows[:, 1] / eng.n_total
    rows[:, 2] = (rows[:, 2] / eng.n_total - mean * mean).clamp_min(0).sqrt()
    rows[:, 1] = mean


def final_sampling(eng, dist, args, key_gen, transform_and_logdet, params=None):
    """``exe_flow_matching.py:453-459``: N = eval_iter * num_chain draws of the reference distribution pushed through the flow
    with ONE shared Hutchinson key, self-normalised importance weights against the target, resampling with replacement.

    The transform is per-sample independent: every rank integrates its contiguous slice of the N draws.  The resampling is
    not -- weights are normalised by the GLOBAL maximum and ``jax.random.choice`` searches the GLOBAL cumulative sum with N
    uniforms -- so flow samples, log-densities and log-weights are all-gathered (N x dim floats: small) and every rank draws
    the same N indices from the same key.  Returns tensors over all N samples, identical on every rank."""
    t = eng.torch
    n_final = args.eval_iter * args.num_chain
    if n_final % eng.world:
        raise ValueError(f"eval_iter * num_chain = {n_final} must be a multiple of the world size")
    ref = ref_dists[args.ref_dist](args.dim)                                                # :388
    u_host = ref.sample_rows(jr.split(key_gen, n_final))                                    # :453 (:389)
    key_hutch, key_choice = jr.split(key_gen)                                               # :454
    per = n_final // eng.world
    lo = eng.rank * per
    u = t.as_tensor(np.ascontiguousarray(u_host[lo:lo + per], dtype=np.float32), device=eng.dev)
    if per % 16:                                                                            # (tiles of 16 samples: pad with copies, drop them again)
        u_pad = t.cat([u, u[-1:].expand(16 - per % 16, -1)]).contiguous()
        flow_pad, vols_pad = transform_and_logdet(key_hutch, u_pad, params)
        flow_local, vols = flow_pad[:per].contiguous(), vols_pad[:per].contiguous()
    else:
        flow_local, vols = transform_and_logdet(key_hutch, u, params)                       # :455
    lp_local = _logprob_any(eng, flow_local)                                                # :456
    ref_lp = (-0.5 * (((u.double() - ref.mean) / ref.std) ** 2).sum(1) - args.dim * np.log(ref.std) - 0.5 * args.dim * np.log(2 * np.pi))   # distributions.py:89-90
    logw_local = lp_local - ref_lp - vols.double()                                          # :457
    flow_samples = allgather_cat(flow_local.contiguous())
    samples_logdensity = allgather_cat(lp_local.contiguous())
    log_weights = allgather_cat(logw_local.contiguous())
    idx = t.empty(n_final, device=eng.dev, dtype=t.int32)
    scratch = t.empty(n_final, device=eng.dev, dtype=t.float64)
    eng.ctx.choice_logw(key_choice, log_weights, n_final, scratch, idx)                     # :458-459
    exact_samples = t.empty_like(flow_samples)
    eng.ctx.gather_rows(flow_samples, idx, exact_samples)
    return dict(flow_samples=flow_samples, exact_samples=exact_samples, samples_logdensity=samples_logdensity,
                log_weights=log_weights, idx=idx, vols=vols, u=u)


def run(dist, args, target_gn=None, log_every=1, return_extras=False):
    """``exe_flow_matching.py:321-561``: the hot loop runs entirely on the device; metrics are fetched every
    ``log_every`` iterations (the reference syncs to the host every iteration for wandb, :442-449)."""
    import torch
    logging.basicConfig(format="%(asctime)s - %(levelname)s - %(name)s - %(message)s", datefmt="%m/%d/%Y %H:%M:%S", level=logging.INFO)
    use_real_samples = args.mcmc_per_flow_steps < 0                                        # :328
    if use_real_samples and target_gn is None:
        raise ValueError("mcmc_per_flow_steps < 0 trains on exact samples and needs a target with sample_model (:382-386)")
    check_adapt_args(args)                                                                  # --adapt_steps (build-side addition)
    check_cox_args(dist, args)                                                              # --example pines: what its HMC kernel does not serve
    check_mclmc_args(args)                                                                  # --mcmc_kernel mclmc: --mclmc_L, --mclmc_integrator
    check_ghmc_args(dist, args)                                                             # --mcmc_kernel ghmc: --ghmc_alpha, --ghmc_delta, --meads_folds, --meads_shuffle
    learning_iter = args.learning_iter
    iter_per_temp = args.anneal_iter // args.num_anneal_temp                                # :330
    n_iter, n_chain = args.eval_iter, args.num_chain
    key_target, key_sample, key_init, key_dist, key_fourier, key_gen = jr.split(jr.PRNGKey(args.seed), 6)    # :333
    dist.initialize_model(key_dist, n_chain)                                                # :334
    fourier_random = args.fourier_std * jr.normal(key_fourier, (args.fourier_dim,))         # :350
    model = VectorFieldNet(fourier_random, dist.grad_logprob, args.hidden_x, args.hidden_t, args.hidden_xt,
                           non_lins[args.non_linearity], args.gradient_clip if args.dim > 128 else None)     # :351
    n_eval = n_iter * n_chain if target_gn is not None else 0
    eng = Engine(dist, args, fourier_random, max_eval_samples=-(-max(n_eval, n_iter * n_chain, n_chain * max(int(args.num_importance_samples), 0)) // 16) * 16)
    model.attach(eng)
    vector_field_param = model.init(key_init, dist.init_params[0], 0.0)                     # :353
    learning_rate_fn = create_learning_rate_fn(learning_iter, args.warmup_steps, args.learning_rate)          # :355-359
    state = create_train_state(model.apply, vector_field_param, learning_rate_fn, args)     # :360

    real_samples = None
    if target_gn is not None:                                                               # :370-374
        key_gen, key_loss = jr.split(key_target)
        keys_target = jr.split(key_gen, n_eval)
        real_host = dist.sample_rows(keys_target)
        lo = eng.rank * (n_eval // eng.world)
        real_samples = torch.as_tensor(np.ascontiguousarray(real_host[lo:lo + n_eval // eng.world], dtype=np.float32), device=eng.dev)
        eval_loss = torch.zeros(1, device=eng.dev, dtype=torch.float64)

    logger.info(f"===== Starting training seed {args.seed} w/ {learning_iter} iterations =====")
    train_data_generator, init_fn, transform_and_logdet = create_train_data_gn(dist, model.apply, None, args)  # :380-381
    train_start = time.time()                                                               # :421

    pos0 = eng.local(dist.init_params)
    if use_real_samples:                                                                    # :382-386, :429-430
        def train_data_generator(key, states, count, *_):
            """positions = vmap(target_gn)(split(key, n_chain)); no MCMC state, acceptance is NaN."""
            rows = dist.sample_rows(jr.split(key, n_chain))[eng.offset:eng.offset + eng.n_valid]
            states.position.copy_(torch.as_tensor(eng.pad_rows(rows), device=eng.dev))
            return states, MALAInfo(nan_acc, None, None, None)
        nan_acc = torch.full((eng.n_local,), float("nan"), device=eng.dev, dtype=torch.float32)
        init_fn = lambda positions, *_: MALAState(positions, None, None)
        beta = 1.0
    else:
        beta = eng.ctx.beta_update(0.0, eng.all_logliks(pos0), args.alpha)                  # :426
        logger.info(f"Initial beta= {beta}")
    train_states = init_fn(pos0, beta)                                                      # :431
    adapt_start = time.time()
    adapt_stats = adapt_step_size(eng, dist, args, pos0, key_gen)                           # --adapt_steps ({} at 0): sets args.step_size
    if "adapted_L" in adapt_stats:                                                          # (--mcmc_kernel mclmc)
        logger.info(f"Adapted step size= {adapt_stats['adapted_step_size']}, L= {adapt_stats['adapted_L']} (energy variance per dimension= {adapt_stats['adapt_energy_var']})")
        wandb.log(adapt_stats)
        train_start += time.time() - adapt_start
    elif "adapted_alpha" in adapt_stats:                                                    # (--mcmc_kernel ghmc: the MEADS warmup)
        logger.info(f"Adapted step size= {adapt_stats['adapted_step_size']}, alpha= {adapt_stats['adapted_alpha']}, inverse mass in "
                    f"[{adapt_stats['adapted_inverse_mass_min']:.4g}, {adapt_stats['adapted_inverse_mass_max']:.4g}] "
                    f"(mean acceptance rate of the last warmup iteration= {adapt_stats['adapt_acceptance']})")
        wandb.log(adapt_stats)
        train_start += time.time() - adapt_start
    elif adapt_stats:
        logger.info(f"Adapted step size= {adapt_stats['adapted_step_size']} (mean acceptance probability over the warmup= {adapt_stats['adapt_acceptance']})")
        if "adapted_trajectory_length" in adapt_stats:                                      # (--hmc_adapt chees)
            logger.info(f"Adapted trajectory length= {adapt_stats['adapted_trajectory_length']} (mean leapfrog steps per iteration= {adapt_stats['adapt_mean_leapfrog']:.4g})")
        elif "adapt_mean_leapfrog" in adapt_stats:                                          # (--nuts_adapt tree)
            logger.info(f"NUTS warmup: mean leapfrog steps per transition= {adapt_stats['adapt_mean_leapfrog']:.4g}")
        if "adapted_inverse_mass" in adapt_stats:
            logger.info(f"Adapted inverse mass matrix (diagonal): min= {adapt_stats['adapted_inverse_mass_min']}, max= {adapt_stats['adapted_inverse_mass_max']}")
        wandb.log({k: v for k, v in adapt_stats.items() if k != "adapted_inverse_mass"})
        train_start += time.time() - adapt_start                                            # (train_time stays the training's: the warmup has ended, its result is on the host)
    metrics = torch.zeros(learning_iter, 4, device=eng.dev, dtype=torch.float64)            # loss, acc mean, acc std, target loss
    betas, lrs = [], []
    n_reduced = 0
    import os
    K_int = int(args.mcmc_per_flow_steps) if args.mcmc_per_flow_steps >= 1 else 0
    prefetch = K_int >= 1 and not use_real_samples and args.num_importance_samples <= 0 and not os.environ.get("MFM_NO_PREFETCH")
    # one rank: generator + train_step in one call (more ranks keep them apart: the MALA step overlaps the gradient all-reduce)
    one_call = (not use_real_samples and eng.world == 1 and not eng._split_calls and getattr(train_data_generator, "one_call_ok", False))
    for count in range(1, learning_iter + 1):                                               # :432
        key_sample, key_train_gn, key_train_step = jr.split(key_sample, 3)                  # :433
        if prefetch and count % (K_int + 1) == 0:
            # a flow step comes: let the workgroups of its kernel that finish early produce the random draws of the K
            # MALA + training iterations that follow (noise.hip); their keys are the next K splits of key_sample.  Slot 0 is
            # this iteration's own training batch (its generator key is the flow step's: those MALA draws are never asked for)
            ks, kg, kt = key_sample, [key_train_gn], [key_train_step]
            for _ in range(min(K_int, learning_iter - count)):
                ks, a_, b_ = jr.split(ks, 3)
                kg.append(a_); kt.append(b_)
            if kg:
                prefetch = eng.ctx.noise_prefetch(np.stack(kg), np.stack(kt))               # False: not served for this configuration
        row = metrics[count - 1]                                                            # loss | sum acc | sum acc^2 | target loss
        if one_call:
            # :438-439 as one library call: on a MALA iteration the step runs inside the training kernel's workgroups (fm.hip)
            _maybe_upload(eng, state.params)
            ib = train_data_generator.info_buffers
            eng.train_iter(count, K_int, train_data_generator.flow_mode, key_train_gn, key_train_step, beta, args.step_size,
                           train_states.position, train_states.logdensity, train_states.logdensity_grad, acc=ib["acc"], nsteps=ib["nsteps"],
                           loss_out=row[0:1])
            infos = MALAInfo(ib["acc"], None, None, None)
        else:
            train_states, infos = train_data_generator(key_train_gn, train_states, count, state.params, beta)    # :438
            eng.train_step(key_train_step, train_states.position, loss_out=row[0:1])        # :439 (:362-368)
            eng.reseed_padding(train_states.position, train_states.logdensity, train_states.logdensity_grad)
        lrs.append(learning_rate_fn(count - 1))                                             # :367 (pre-increment step)
        if not use_real_samples and count % iter_per_temp == 0 and beta < 1.0:              # :440-441, :417
            beta = eng.ctx.beta_update(beta, eng.all_logliks(train_states.position), args.alpha)              # :413
            train_states = init_fn(train_states.position, beta)                             # :415
        eng.ctx.acc_stats(infos.acceptance_rate[:eng.n_valid], row[1:3])                    # :442-443, per-rank partial sums (chains only: no padding rows)
        if real_samples is not None:                                                        # :444-446
            eng.eval_loss(key_loss, real_samples, row[3:4], n_total=n_eval, offset=eng.rank * (n_eval // eng.world))
        betas.append(beta)
        if count % log_every == 0 or count == learning_iter:
            _finish_metric_rows(eng, metrics, n_reduced, count); n_reduced = count          # ONE collective per log interval
            row = metrics[count - 1].tolist()                                               # host sync
            wandb.log({"loss": row[0], "learning_rate": lrs[-1], "acceptance avg.": row[1], "acceptance std.": row[2],
                       "target_loss": row[3], "train_time": time.time() - train_start})     # :447-449
    eng.ctx.sync()
    train_time = time.time() - train_start
    logger.info(f"Final beta= {beta}")

    # ---- final flow samples + importance resampling (:453-459), over ALL N samples on every rank --------------------
    fin = final_sampling(eng, dist, args, key_gen, transform_and_logdet, state.params)
    flow_samples, exact_samples, samples_logdensity = fin["flow_samples"], fin["exact_samples"], fin["samples_logdensity"]
    if getattr(args, "check", False) and real_samples is not None:                          # :462-467 (--check: the exact samples' own scores)
        real_chk = allgather_cat(real_samples)
        logger.info(f"Logpdf of real samples= {_logprob_any(eng, real_chk).mean().item()}")
        stein_chk = stein_disc(eng, real_chk)
        logger.info(f"Stein U, V disc of real samples= {stein_chk[0]}, {stein_chk[1]}")
        logger.info(f"Max mean disc of NF+MCMC samples= {eng.ctx.max_mean_disc(real_chk, real_chk)}")       # (the reference's label)
    logpdf = samples_logdensity.mean().item()                                               # :469
    logger.info(f"Logpdf of flow samples= {logpdf}")
    stein = stein_disc(eng, flow_samples)                                                   # :471 (mcmc_utils.py:28-85)
    logger.info(f"Stein U, V disc of flow samples= {stein[0]}, {stein[1]}")
    logpdf_ = _logprob_any(eng, exact_samples).mean().item()                                # :473
    logger.info(f"Logpdf of exact samples= {logpdf_}")
    stein_ = stein_disc(eng, exact_samples)                                                 # :475
    logger.info(f"Stein U, V disc of exact samples= {stein_[0]}, {stein_[1]}")
    if target_gn is not None:                                                               # :480-487 (mcmc_utils.py:88-111)
        real_all = allgather_cat(real_samples)                                              # every rank holds a slice of the exact samples
        mmd = eng.ctx.max_mean_disc(real_all, flow_samples)
        logger.info(f"Max mean disc of flow samples= {mmd}")
        mmd_ = eng.ctx.max_mean_disc(real_all, exact_samples)
        logger.info(f"Max mean disc of exact samples= {mmd_}")
    else:
        mmd = mmd_ = 0.0                                                                    # :490
    mclmc_stats = {}
    if getattr(args, "mcmc_kernel", "mala") == "mclmc" and not use_real_samples:            # the energy error of the run's own MCLMC steps
        from .engine import allreduce_sum_
        count = torch.tensor([float(eng.mclmc_energy_count)], device=eng.dev, dtype=torch.float64)      # (once, after the loop)
        e = allreduce_sum_(torch.cat([eng.mclmc_energy, count]))[0].tolist()
        m = e[0] / e[2] if e[2] else float("nan")
        mclmc_stats = dict(energy_var_per_dim=(e[1] / e[2] - m * m) / args.dim if e[2] else float("nan"))
        logger.info(f"MCLMC energy variance per dimension over the run= {mclmc_stats['energy_var_per_dim']:.4g}")
        wandb.log(mclmc_stats)
    ess_stats = chain_ess_per_step(eng, dist, args, train_states, key_gen)                  # --ess_steps (build-side addition; {} at 0)
    if ess_stats and getattr(args, "mcmc_kernel", "mala") == "mclmc":
        logger.info("ESS per MCLMC step (min, median, mean over chains and coordinates)= "
                    + ", ".join(f"{ess_stats[k]:.4g}" for k in ("ess_per_step_min", "ess_per_step_median", "ess_per_step_mean")))
        logger.info("ESS per gradient evaluation of the MCLMC kernel (min, median, mean)= "
                    + ", ".join(f"{ess_stats[k]:.4g}" for k in ("ess_per_grad_min", "ess_per_grad_median", "ess_per_grad_mean")))
        logger.info(f"Split R-hat across chains (max, median over coordinates)= {ess_stats['rhat_max']:.4g}, {ess_stats['rhat_median']:.4g}")
        logger.info("Multi-chain ESS per gradient evaluation of the MCLMC kernel and chain (min, median, mean)= "
                    + ", ".join(f"{ess_stats['ess_multichain_per_grad_' + k]:.4g}" for k in ("min", "median", "mean")))
        wandb.log(ess_stats)
    elif ess_stats:
        use_hmc = getattr(args, "mcmc_kernel", "mala") == "hmc"
        use_nuts = getattr(args, "mcmc_kernel", "mala") == "nuts"
        step_name = (f"HMC step ({ess_stats['hmc_mean_leapfrog']:.4g} leapfrog steps on average)" if "hmc_mean_leapfrog" in ess_stats
                     else f"HMC step ({int(args.hmc_steps)} leapfrog steps)") if use_hmc else "NUTS transition" if use_nuts else "MALA step"
        logger.info(f"ESS per {step_name} (min, median, mean over chains and coordinates)= "
                    + ", ".join(f"{ess_stats[k]:.4g}" for k in ("ess_per_step_min", "ess_per_step_median", "ess_per_step_mean")))
        if use_nuts:
            logger.info(f"NUTS trees over the run: mean depth= {ess_stats['nuts_mean_depth']:.4g}, mean leapfrog steps= {ess_stats['nuts_mean_leapfrog']:.4g}, "
                        f"divergent transitions= {ess_stats['nuts_divergent']}")
        if use_hmc or use_nuts:
            logger.info(f"ESS per gradient evaluation of the {'HMC' if use_hmc else 'NUTS'} kernel (min, median, mean)= "
                        + ", ".join(f"{ess_stats[k]:.4g}" for k in ("ess_per_grad_min", "ess_per_grad_median", "ess_per_grad_mean")))
        logger.info(f"Split R-hat across chains (max, median over coordinates)= {ess_stats['rhat_max']:.4g}, {ess_stats['rhat_median']:.4g}")
        logger.info(f"Multi-chain ESS per {step_name} and chain (min, median, mean over coordinates)= "
                    + ", ".join(f"{ess_stats['ess_multichain_per_step_' + k]:.4g}" for k in ("min", "median", "mean")))
        if use_hmc or use_nuts:
            logger.info(f"Multi-chain ESS per gradient evaluation of the {'HMC' if use_hmc else 'NUTS'} kernel and chain (min, median, mean)= "
                        + ", ".join(f"{ess_stats['ess_multichain_per_grad_' + k]:.4g}" for k in ("min", "median", "mean")))
        wandb.log(ess_stats)
    res = np.array([logpdf, stein[0], stein[1], mmd, train_time])                           # :561
    res_ = np.array([logpdf_, stein_[0], stein_[1], mmd_, train_time])
    wandb.finish()
    if return_extras:
        return res, res_, dict(metrics=metrics.cpu().numpy(), betas=np.array(betas), lrs=np.array(lrs), states=train_states,
                               engine=eng, state=state, flow_samples=flow_samples, exact_samples=exact_samples, model=model,
                               final=fin, key_gen=key_gen, **ess_stats, **adapt_stats, **mclmc_stats)
    eng.close()
    return res, res_


def check_adapt_args(args):
    """``--adapt_steps`` needs ``--mcmc_kernel hmc`` (or ``nuts``, which runs the HMC warmup, or with ``--nuts_adapt tree`` its own) and a run
    that takes MCMC steps; ``--nuts_adapt tree`` needs ``--mcmc_kernel nuts``: raised before any device work."""
    n_steps = int(getattr(args, "adapt_steps", 0) or 0)
    if n_steps < 0:
        raise ValueError(f"--adapt_steps must not be negative (got {n_steps})")
    if n_steps == 0 and getattr(args, "adapt_mass", False):
        raise ValueError("--adapt_mass adapts the mass matrix during the --adapt_steps N warmup steps: give N > 0")
    if n_steps > 0 and args.mcmc_per_flow_steps < 0:
        raise ValueError("--adapt_steps has nothing to adapt with mcmc_per_flow_steps < 0: that run trains on exact samples and takes no MCMC step")
    kern = getattr(args, "mcmc_kernel", "mala")
    if kern == "mclmc" and getattr(args, "adapt_mass", False):
        raise ValueError("--adapt_mass is not served with --mcmc_kernel mclmc: the MCLMC kernel (mfm_mclmc_*) runs at unit metric")
    if n_steps > 0 and kern not in ("hmc", "nuts", "mclmc", "ghmc"):
        raise ValueError("--adapt_steps needs --mcmc_kernel hmc: the training loop's MALA step uses the acceptance rule AS WRITTEN, which accepts "
                         "with min(1, 1 / alpha); its acceptance does not fall as the step grows, so dual averaging has nothing to steer by")
    hmc_adapt = getattr(args, "hmc_adapt", "dual")
    if hmc_adapt not in ("dual", "chees"):
        raise ValueError(f"--hmc_adapt must be dual or chees (got {hmc_adapt!r})")
    if hmc_adapt == "chees":
        if getattr(args, "mcmc_kernel", "mala") != "hmc":
            raise ValueError("--hmc_adapt chees adapts the HMC kernel's step size and trajectory length: it needs --mcmc_kernel hmc")
        if n_steps == 0:
            raise ValueError("--hmc_adapt chees runs its iterations during the --adapt_steps N warmup: give N > 0")
        if getattr(args, "adapt_mass", False):
            raise ValueError("--hmc_adapt chees uses the mass matrix as given: it does not go with --adapt_mass")
    nuts_adapt = getattr(args, "nuts_adapt", "hmc")
    if nuts_adapt not in ("hmc", "tree"):
        raise ValueError(f"--nuts_adapt must be hmc or tree (got {nuts_adapt!r})")
    if nuts_adapt == "tree" and getattr(args, "mcmc_kernel", "mala") != "nuts":
        raise ValueError("--nuts_adapt tree adapts on the No-U-turn sampler's own trees: it needs --mcmc_kernel nuts")
    return n_steps


def check_cox_args(dist, args):
    """``--example pines``: the gradient samplers reach the Cox process through ``mfm_cox_hmc_*`` alone (``--mcmc_kernel hmc``, its
    ``--adapt_steps`` dual-averaging warmup, ``--ess_steps``); what has no Cox kernel is named here, before any device work."""
    if getattr(dist, "kind", None) != "lgcp" or any(getattr(args, f, False) for f in ("do_eslice", "do_smc", "do_svgd")):
        return                                      # (those baselines do not read --mcmc_kernel or the adaptation flags)
    kern = getattr(args, "mcmc_kernel", "mala")
    if getattr(args, "do_pt", False):
        raise ValueError("--do_pt is not served with --example pines: parallel tempering (mfm_pt_run) has no local move for the Cox process")
    if kern == "mclmc":
        raise ValueError("--mcmc_kernel mclmc is not served with --example pines: MCLMC (mfm_mclmc_*) has no Cox process kernel (use --mcmc_kernel hmc)")
    if kern == "ghmc":
        raise ValueError("--mcmc_kernel ghmc is not served with --example pines: GHMC (mfm_ghmc_*) has no Cox process kernel (use --mcmc_kernel hmc)")
    if kern == "nuts":
        raise ValueError("--mcmc_kernel nuts is not served with --example pines: the No-U-turn sampler has no Cox process kernel (use --mcmc_kernel hmc)")
    if getattr(args, "adapt_mass", False):
        raise ValueError("--adapt_mass is not served with --example pines: the Cox process's HMC kernel (mfm_cox_hmc_*) runs at unit mass")
    if getattr(args, "hmc_adapt", "dual") == "chees":
        raise ValueError("--hmc_adapt chees is not served with --example pines: ChEES (mfm_chees_warmup, mfm_hmc_run_lengths) has no Cox process kernel "
                         "(use the default --hmc_adapt dual)")
    if kern == "hmc" and int(getattr(dist, "dim", 0)) > 1024:
        raise ValueError(f"--mcmc_kernel hmc with --example pines serves dim <= 1024, a 32 x 32 grid (got {dist.dim}): give --force_dim")


def check_mclmc_args(args):
    """``--mcmc_kernel mclmc``'s own flags, before any device work: ``--mclmc_L`` (0 or positive) and ``--mclmc_integrator``."""
    if getattr(args, "mcmc_kernel", "mala") != "mclmc":
        return
    if float(getattr(args, "mclmc_L", 0.0) or 0.0) < 0:
        raise ValueError(f"--mclmc_L must be positive, or 0 for sqrt(dim) (got {args.mclmc_L})")
    from .bblackjax.mcmc.mclmc import integrator_id
    integrator_id(getattr(args, "mclmc_integrator", "mclachlan"))


def check_ghmc_args(dist, args):
    """``--mcmc_kernel ghmc``'s own flags and what does not go with it, before any device work."""
    if getattr(args, "mcmc_kernel", "mala") != "ghmc":
        return
    from .bblackjax.adaptation.meads_adaptation import check_folds
    from .bblackjax.mcmc.ghmc import check_parameters
    if getattr(dist, "kind", None) == "lgcp":
        raise ValueError("--mcmc_kernel ghmc is not served with --example pines: GHMC (mfm_ghmc_*) has no Cox process kernel (use --mcmc_kernel hmc)")
    if getattr(args, "adapt_mass", False):
        raise ValueError("--adapt_mass is not served with --mcmc_kernel ghmc: its --adapt_steps warmup is MEADS, which sets the mass itself")
    if getattr(args, "hmc_adapt", "dual") == "chees":
        raise ValueError("--hmc_adapt chees is not served with --mcmc_kernel ghmc: a GHMC transition has no trajectory length to adapt")
    if getattr(args, "nuts_adapt", "hmc") == "tree":
        raise ValueError("--nuts_adapt tree is not served with --mcmc_kernel ghmc: it adapts on the No-U-turn sampler's trees")
    if getattr(args, "do_pt", False):
        raise ValueError("--do_pt is not served with --mcmc_kernel ghmc: parallel tempering takes mala or hmc as its local move")
    check_parameters(args.step_size, getattr(args, "ghmc_alpha", 0.5), getattr(args, "ghmc_delta", None))
    if int(getattr(args, "meads_shuffle", 0) or 0) < 0:
        raise ValueError(f"--meads_shuffle must not be negative (got {args.meads_shuffle})")
    if int(getattr(args, "adapt_steps", 0) or 0) > 0:
        try:
            check_folds(int(args.num_chain), int(getattr(args, "meads_folds", 4)))
        except ValueError as e:
            raise ValueError(f"--mcmc_kernel ghmc --adapt_steps: num_chain ({args.num_chain}) must be a multiple of --meads_folds "
                             f"({getattr(args, 'meads_folds', 4)} >= 2) with at least 2 chains per fold") from e


def ghmc_delta(args):
    """``--ghmc_delta``: the slice drift of ``--mcmc_kernel ghmc``; not given: ``--ghmc_alpha / 2``."""
    delta = getattr(args, "ghmc_delta", None)
    return ghmc_alpha(args) / 2.0 if delta is None else float(delta)


def ghmc_alpha(args):
    """``--ghmc_alpha``: the momentum refresh rate of ``--mcmc_kernel ghmc`` (default 0.5)."""
    return float(getattr(args, "ghmc_alpha", 0.5))


def mclmc_L(args):
    """``--mclmc_L``: the momentum decoherence length of ``--mcmc_kernel mclmc``; 0 (the default) means ``sqrt(dim)``."""
    L = float(getattr(args, "mclmc_L", 0.0) or 0.0)
    return L if L > 0 else float(np.sqrt(args.dim))


def hmc_num_steps(args, i):
    """The leapfrog steps of the HMC step of training iteration / sampling step ``i``: ``--hmc_steps``, or under ``--hmc_adapt chees`` the
    jittered count ``integration_steps_fn(i)`` of the adapted ``(step_size, hmc_trajectory_length)``."""
    T = getattr(args, "hmc_trajectory_length", None)
    if T is None:
        return int(args.hmc_steps)
    from .bblackjax.adaptation.chees_adaptation import integration_steps
    return integration_steps(i, args.step_size, T)


def adapt_step_size(eng, dist, args, pos0, key_gen):
    """``--adapt_steps N`` (with ``--mcmc_kernel hmc``): N HMC warmup steps of ``--hmc_steps`` leapfrog steps in one launch
    (``kernel.warmup``, ``mfm_hmc_warmup``) on a COPY of the initial chains ``pos0`` at beta = 1, every chain adapting its own step size
    from ``--step_size`` by dual averaging towards the acceptance probability ``--adapt_target``.  ``args.step_size`` becomes the pooled
    value (geometric mean over the chains of all ranks) for the rest of the run, ``--ess_steps`` included; ``pos0``, the chains the
    training starts from, is not moved.  Returns ``adapted_step_size`` and ``adapt_acceptance``, the mean acceptance probability over
    the warmup's steps and chains.  The key is a child of ``key_gen`` that nothing else draws (``split(key_gen, 4)[3]``: the final
    sampling uses ``split(key_gen)`` and ``split(key_gen, n_final)``, ``--ess_steps`` ``split(key_gen, 3)[2]``).

    ``--adapt_mass``: the N steps run ``window_adaptation`` (``bblackjax/adaptation/window_adaptation.py``) instead, on the same key and
    copy: step size and a diagonal mass matrix together.  The inverse mass matrix is installed on the engine's context, where the
    training loop's ``hmc_step`` calls find it, and kept as ``args.inverse_mass_matrix`` for ``--ess_steps``; besides the two figures
    above (``adapt_acceptance``: of the last segment) the result carries ``adapted_inverse_mass`` (the vector) and its ``_min`` / ``_max``.

    ``--mcmc_kernel nuts``: the same HMC warmup with ``--hmc_steps`` leapfrog steps, whose step size and mass NUTS then samples with -- the
    integrator and the metric are the same; it approximates adapting on the tree's own acceptance statistic.  With ``--nuts_adapt tree``
    the warmup is NUTS's own instead: N transitions under ``--max_tree_depth`` in one launch (``nuts(...).step.warmup``,
    ``mfm_nuts_warmup``), every chain adapting on the mean over its tree's leaves of ``min(1, exp(H0 - H))``; with ``--adapt_mass``
    ``nuts_window_adaptation``.  ``--hmc_steps`` plays no part, and the result also carries ``adapt_mean_leapfrog``, the mean number
    of leapfrog steps per transition over the warmup (with ``--adapt_mass``: of the last segment).

    ``--hmc_adapt chees``: the N steps are N ChEES-HMC iterations (``chees_adaptation``, ``mfm_chees_warmup``) on the same key and copy: the
    chains adapt ONE step size (towards the harmonic-mean acceptance ``--adapt_target``) and ONE trajectory length together.  ``args.step_size`` and ``args.hmc_trajectory_length`` are set, and the
    HMC step of training iteration i and of ``--ess_steps`` then makes ``hmc_num_steps(args, i)`` leapfrog steps in place of ``--hmc_steps``.
    The result carries ``adapted_step_size``, ``adapted_trajectory_length``, ``adapt_acceptance`` (the last iteration's harmonic-mean
    acceptance) and ``adapt_mean_leapfrog`` (the mean leapfrog count over the iterations)."""
    n_steps = check_adapt_args(args)
    if n_steps <= 0:
        return {}
    if getattr(args, "mcmc_kernel", "mala") == "mclmc":
        # --mcmc_kernel mclmc: mclmc_find_L_and_step_size over N steps on the copy, from --step_size; args.step_size and args.mclmc_L are set
        from .bblackjax.adaptation.mclmc_adaptation import mclmc_find_L_and_step_size
        from .bblackjax.mcmc.mclmc import mclmc
        integ = getattr(args, "mclmc_integrator", "mclachlan")
        make = lambda L, eps: mclmc(dist.logprob, L, eps, integ)
        k_init, k_tune = jr.split(jr.split(key_gen, 4)[3])
        history = []
        _, params = mclmc_find_L_and_step_size(make, make(1.0, 1.0).init(pos0.clone(), k_init), k_tune, n_steps, initial_step_size=args.step_size,
                                               n_valid=eng.n_valid, ess_fn=lambda p: mcmc_utils_ess(p, eng), history=history)
        args.step_size, args.mclmc_L = params.step_size, params.L
        # adapt_energy_var: the variance per dimension of the LAST step-size round, the one the returned step size was derived from (at the
        # phase-2 L; the phase-3 run that follows only replaces L)
        return dict(adapted_step_size=params.step_size, adapted_L=params.L, adapt_energy_var=[h for h in history if h[0] != 3][-1][3])
    if getattr(args, "mcmc_kernel", "mala") == "ghmc":
        # --mcmc_kernel ghmc: N MEADS iterations (meads_adaptation, mfm_meads_warmup) on the copy at beta = 1, from --step_size / --ghmc_alpha;
        # args.step_size, args.ghmc_alpha, args.ghmc_delta and args.ghmc_inverse_mass (a float64 device vector) are set
        from .bblackjax.adaptation.meads_adaptation import meads_adaptation
        if eng.world > 1:
            raise ValueError("--mcmc_kernel ghmc --adapt_steps serves one rank: the MEADS fold statistics would need an all-reduce")
        warm = meads_adaptation(dist.logprob, eng.n_valid, int(getattr(args, "meads_folds", 4)), int(getattr(args, "meads_shuffle", 0) or 0),
                                args.step_size, ghmc_alpha(args))
        (_, par), minfo = warm.run(jr.split(key_gen, 4)[3], pos0.clone(), n_steps)
        minv = par["momentum_inverse_scale"] ** 2
        args.step_size, args.ghmc_alpha, args.ghmc_delta, args.ghmc_inverse_mass = par["step_size"], par["alpha"], par["delta"], minv.contiguous()
        return dict(adapted_step_size=par["step_size"], adapted_alpha=par["alpha"], adapted_inverse_mass_min=minv.min().item(),
                    adapted_inverse_mass_max=minv.max().item(), adapt_acceptance=minfo.mean_acceptance[-1].mean().item())
    from .bblackjax.mcmc.hmc import hmc
    from .engine import global_mean_std
    if getattr(args, "hmc_adapt", "dual") == "chees":
        from .bblackjax.adaptation.chees_adaptation import chees_adaptation
        from .bblackjax.optimizers import adam
        algo = hmc(dist.logprob, args.step_size, 1)
        (_, params), info = chees_adaptation(dist.logprob, eng.n_valid, float(getattr(args, "adapt_target", 0.8))).run(
            jr.split(key_gen, 4)[3], algo.init(pos0), args.step_size, adam(0.025), n_steps)
        args.step_size, args.hmc_trajectory_length = params["step_size"], params["trajectory_length"]
        return dict(adapted_step_size=params["step_size"], adapted_trajectory_length=params["trajectory_length"],
                    adapt_acceptance=info.harmonic_mean_acceptance[-1].item(), adapt_mean_leapfrog=info.num_integration_steps.mean().item())
    if getattr(args, "nuts_adapt", "hmc") == "tree":
        from .bblackjax.mcmc.nuts import nuts
        depth, target = int(getattr(args, "max_tree_depth", 10)), float(getattr(args, "adapt_target", 0.8))
        algo = nuts(dist.logprob, args.step_size, depth)
        if getattr(args, "adapt_mass", False):
            from .bblackjax.adaptation.window_adaptation import nuts_window_adaptation
            wa = nuts_window_adaptation(dist.logprob, depth, args.step_size, target)
            _, params, info = wa.run(jr.split(key_gen, 4)[3], algo.init(pos0), n_steps)
            minv = params["inverse_mass_matrix"]
            args.step_size, args.inverse_mass_matrix = params["step_size"], minv
            eng.ctx.set_inverse_mass(minv)
            return dict(adapted_step_size=params["step_size"], adapt_acceptance=info.acceptance_rates[-1],
                        adapt_mean_leapfrog=info.mean_integration_steps[-1], adapted_inverse_mass=minv,
                        adapted_inverse_mass_min=float(minv.min()), adapted_inverse_mass_max=float(minv.max()))
        _, info = algo.step.warmup(jr.split(key_gen, 4)[3], algo.init(pos0), n_steps, target)
        args.step_size = info.pooled_step_size
        acc, _ = global_mean_std(info.acceptance_rate[:eng.n_valid], eng.n_total)
        leap, _ = global_mean_std(info.num_integration_steps[:eng.n_valid].double() / n_steps, eng.n_total)
        return dict(adapted_step_size=info.pooled_step_size, adapt_acceptance=acc.item(), adapt_mean_leapfrog=leap.item())
    if getattr(args, "adapt_mass", False):
        from .bblackjax.adaptation.window_adaptation import window_adaptation
        algo = hmc(dist.logprob, args.step_size, int(args.hmc_steps))
        wa = window_adaptation(dist.logprob, int(args.hmc_steps), args.step_size, float(getattr(args, "adapt_target", 0.8)))
        _, params, info = wa.run(jr.split(key_gen, 4)[3], algo.init(pos0), n_steps)
        minv = params["inverse_mass_matrix"]
        args.step_size, args.inverse_mass_matrix = params["step_size"], minv
        eng.ctx.set_inverse_mass(minv)
        return dict(adapted_step_size=params["step_size"], adapt_acceptance=info.acceptance_rates[-1], adapted_inverse_mass=minv,
                    adapted_inverse_mass_min=float(minv.min()), adapted_inverse_mass_max=float(minv.max()))
    algo = hmc(dist.logprob, args.step_size, int(args.hmc_steps))
    _, info = algo.step.warmup(jr.split(key_gen, 4)[3], algo.init(pos0), n_steps, float(getattr(args, "adapt_target", 0.8)))
    args.step_size = info.pooled_step_size
    acc, _ = global_mean_std(info.acceptance_rate[:eng.n_valid], eng.n_total)
    return dict(adapted_step_size=info.pooled_step_size, adapt_acceptance=acc.item())


def mcmc_utils_ess(positions, eng):
    from . import mcmc_utils
    return mcmc_utils.effective_sample_size(positions, ctx=eng.ctx)


def chain_ess_per_step(eng, dist, args, states, key_gen):
    """``--ess_steps N``: N steps of the kernel the run trained with (``--mcmc_kernel``: MALA steps, or HMC steps of ``--hmc_steps``
    leapfrog steps) at ``--step_size`` from the final chains at beta = 1 in one launch (``kernel.run``, ``thin = 1``) and Geyer's
    effective sample size of every chain and coordinate of that trajectory, over N: ``ess_per_step_min`` / ``_median`` / ``_mean``.
    An HMC step costs ``hmc_steps`` gradient evaluations where a MALA step costs one, so for ``hmc`` the same figures over
    ``hmc_steps`` come along as ``ess_per_grad_min`` / ``_median`` / ``_mean``: the scale on which the two kernels compare (for MALA
    it is ``ess_per_step_*`` itself).  The key is a child of ``key_gen`` that nothing else draws (``split(key_gen, 3)[2]``: the final
    sampling uses ``split(key_gen)`` and ``split(key_gen, n_final)``), and the chains of ``states`` are left as they are.
    From the same trajectory, across the chains of all ranks (``diagnostics.chain_diagnostics``): ``rhat_max`` / ``rhat_median`` over the
    coordinates, and the multi-chain ESS over (all chains x N) as ``ess_multichain_per_step_min`` / ``_median`` / ``_mean`` (for ``hmc`` also
    ``ess_multichain_per_grad_*``).
    ``--mcmc_kernel nuts``: N No-U-turn transitions (``nuts(...).step.run``); a transition costs its tree's leapfrog steps, so ``ess_per_grad_*``
    and ``ess_multichain_per_grad_*`` divide by the MEASURED mean leapfrog count per transition over the run and the chains of all ranks,
    logged as ``nuts_mean_leapfrog`` beside ``nuts_mean_depth`` and ``nuts_divergent`` (the number of divergent transitions).
    ``--mcmc_kernel mclmc``: N MCLMC steps (``mclmc(...).step.run``) at ``--step_size`` / ``--mclmc_L`` from the final chains with fresh unit
    momenta (the key's two halves: momenta, run); a step costs 1 (leapfrog) or 2 (McLachlan) gradient evaluations, which ``ess_per_grad_*`` and
    ``ess_multichain_per_grad_*`` divide by; ``energy_var_per_dim_ess_run`` is that run's energy-change variance per dimension."""
    n_steps = int(getattr(args, "ess_steps", 0) or 0)
    if n_steps <= 0 or states.logdensity is None:                  # (training on exact samples keeps no MCMC state)
        return {}
    import torch
    from . import mcmc_utils
    use_hmc = getattr(args, "mcmc_kernel", "mala") == "hmc"
    use_nuts = getattr(args, "mcmc_kernel", "mala") == "nuts"
    use_mclmc = getattr(args, "mcmc_kernel", "mala") == "mclmc"
    use_ghmc = getattr(args, "mcmc_kernel", "mala") == "ghmc"
    # the kernel, the state it starts from, its key and what a step costs in gradient evaluations ...
    key, run_kw = jr.split(key_gen, 3)[2], {}
    if use_mclmc:          # fresh unit momenta from one half of the key, the run on the other; 1 (leapfrog) or 2 (McLachlan) gradients per step
        from .bblackjax.mcmc.mclmc import integrator_id, mclmc
        integ = integrator_id(getattr(args, "mclmc_integrator", "mclachlan"))
        algo = mclmc(dist.logprob, mclmc_L(args), args.step_size, integ)
        k_init, key = jr.split(key)
        start, grads_per_step = algo.init(states.position, k_init), float(integ + 1)
    elif use_ghmc:         # fresh momenta and slice variables from one half of the key, the run on the other; ONE gradient per transition
        from .bblackjax.mcmc.ghmc import ghmc
        minv = getattr(args, "ghmc_inverse_mass", None)
        algo = ghmc(dist.logprob, args.step_size, ghmc_alpha(args), ghmc_delta(args), None if minv is None else minv.sqrt())
        k_init, key = jr.split(key)
        start, grads_per_step = algo.init(states.position, k_init), 1.0
    elif use_hmc:
        from .bblackjax.mcmc.hmc import hmc
        algo = hmc(dist.logprob, args.step_size, int(args.hmc_steps), getattr(args, "inverse_mass_matrix", None))      # (--adapt_mass)
        start, grads_per_step = algo.init(states.position), float(int(args.hmc_steps))
    elif use_nuts:
        from .bblackjax.mcmc.nuts import nuts
        algo = nuts(dist.logprob, args.step_size, int(getattr(args, "max_tree_depth", 10)), getattr(args, "inverse_mass_matrix", None))
        start, grads_per_step = algo.init(states.position), 1.0      # (replaced by the measured leapfrog count below)
    else:
        from .bblackjax.mcmc.mala import mala
        algo = mala(dist.logprob, args.step_size)
        start, grads_per_step = algo.init(states.position), 1.0
    chees = use_hmc and getattr(args, "hmc_trajectory_length", None) is not None          # (--hmc_adapt chees: the jittered leapfrog counts)
    if chees:
        run_kw["num_integration_steps_per_step"] = lambda i: hmc_num_steps(args, i)
    # ... and the run, the same call for every kernel
    _, info = algo.step.run(key, start, n_steps, thin=1, **run_kw)
    ess, _ = mcmc_utils.effective_sample_size(info.positions[:, :eng.n_valid], ctx=eng.ctx)
    per_step = (ess.double() / n_steps).reshape(-1)
    out = dict(ess_per_step_min=per_step.min().item(), ess_per_step_median=per_step.median().item(), ess_per_step_mean=per_step.mean().item())
    if use_mclmc:
        out["energy_var_per_dim_ess_run"] = info.energy_var_per_dim
    if chees:          # the measured mean leapfrog count per step (the same for every chain), as NUTS
        grads_per_step = info.num_leapfrog / n_steps
        out["hmc_mean_leapfrog"] = grads_per_step
    if use_nuts:       # a transition costs its tree's leapfrog steps: the measured mean over the run's transitions and the chains of all ranks
        from .engine import global_mean_std
        per_chain = torch.stack([info.num_integration_steps.double() / n_steps, info.mean_trajectory_expansions.double(),
                                           info.num_divergent.double()], 1)[:eng.n_valid]
        means = [global_mean_std(per_chain[:, q].contiguous(), eng.n_total)[0].item() for q in range(3)]
        grads_per_step = means[0]
        out.update(nuts_mean_leapfrog=means[0], nuts_mean_depth=means[1], nuts_divergent=int(round(means[2] * eng.n_total)))
    if use_hmc or use_nuts or use_mclmc or use_ghmc:
        for name in ("min", "median", "mean"):
            out["ess_per_grad_" + name] = out["ess_per_step_" + name] / grads_per_step
    # across the chains (of all ranks): split-R-hat and the multi-chain ESS, per step and chain (diagnostics.py; a chain stuck in one
    # mode looks mixed to the per-chain figures above and not to these).  The padding rows past n_valid are skipped without a copy.
    from . import diagnostics
    cd = diagnostics.chain_diagnostics(info.positions, n_valid=eng.n_valid, ctx=eng.ctx)
    rhat, multi = cd.rhat.double(), cd.ess.double() / (float(eng.n_total) * n_steps)
    out.update(rhat_max=rhat.max().item(), rhat_median=rhat.median().item(), ess_multichain_per_step_min=multi.min().item(),
               ess_multichain_per_step_median=multi.median().item(), ess_multichain_per_step_mean=multi.mean().item())
    if use_hmc or use_nuts or use_mclmc or use_ghmc:
        for name in ("min", "median", "mean"):
            out["ess_multichain_per_grad_" + name] = out["ess_multichain_per_step_" + name] / grads_per_step
    return out


def stein_disc(eng, x, beta=-0.5):
    """``mcmc_utils.stein_disc(X, dist.logprob)`` (mcmc_utils.py:28-85) for CUDA samples [n, d] -> (U, V)."""
    _, grad = _logprob_any(eng, x, want_grad=True)
    return eng.ctx.stein_disc(x.contiguous(), grad, beta)


def max_mean_disc(eng, x, y):
    """``mcmc_utils.max_mean_disc`` (mcmc_utils.py:88-111) for CUDA sample sets of equal size."""
    return eng.ctx.max_mean_disc(x.contiguous(), y.contiguous())


def _logprob_any(eng, x, want_grad=False, beta=1.0):
    """vmap(dist.logprob) for any sample count: the MALA init kernel at beta = 1 returns loglik + logprior for every
    built target; samples are processed in chunks of the engine's chain count (zero padded)."""
    t = eng.torch
    out = t.empty(x.shape[0], device=eng.dev, dtype=t.float64)
    gout = t.empty(x.shape[0], x.shape[1], device=eng.dev, dtype=t.float32) if want_grad else None
    n = eng.n_local
    lp = t.empty(n, device=eng.dev, dtype=t.float64)
    gr = t.empty(n, x.shape[1], device=eng.dev, dtype=t.float32)
    for s in range(0, x.shape[0], n):
        chunk = x[s:s + n]
        m = chunk.shape[0]
        if m < n:
            pad = t.zeros(n, x.shape[1], device=eng.dev, dtype=x.dtype); pad[:m] = chunk
            chunk = pad
        eng.ctx.mala_init(chunk.contiguous(), float(beta), lp, gr)
        out[s:s + m] = lp[:m]
        if want_grad:
            gout[s:s + m] = gr[:m]
    return (out, gout) if want_grad else out
