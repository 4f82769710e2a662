"""Shard invariance of every entry point that draws by global chain id.

A multi-GPU run shards the chains contiguously; every rank's context carries ``n_chain_total``, ``chain_offset`` and ``n_chain_local``
and every kernel that draws must derive chain b's key from ``chain_offset + b``, split over ``n_chain_total``.  A kernel that ignored
the offset, or split over the local count, would hand every rank the same stream.  No run with more than one rank has taken place on
hardware, so these one-GPU tests are what stands against that.

The scheme (tests/shard_cases.py): one context holds all 64 chains; fresh contexts with ``n_chain_total = 64`` hold the chains
[0, 16), [16, 48) and [48, 64), start from their rows of the same state (in per-chain-key mode: their rows of the same key array) and
make the same call.  EVERY per-chain output of a part must equal the whole run's rows bit for bit -- proposals, acceptance
probabilities, flags, weights, attempt counts, tallies, step sizes, window sums, tree infos, thinned trajectories, not only the end
state (in the flow step's usual regime nearly every proposal is rejected and end positions say nothing).  A chain's arithmetic depends
on its own row, its own key and the kernel instance only, so bit equality carries the oracle parity that the existing tests establish
for whole contexts over to the shards.  Where the library picks the instance by chain count the case pins it for both runs or says why
64, 32 and 16 chains get the same one.

One sensitivity control per key-derivation site (resident.hip.h, nuts.hip, lgcp.hip / mala_run_keys_kernel, ode.hip, ode_d2.hip,
ode_fixed.hip, the wide family's probes in api.hip, fm.hip) runs the [16, 48) part in a context built with offset 0: what it draws
must differ from rows 16..47 of the whole run, i.e. these tests fail on a kernel that ignores the offset.  Two oracle anchors at an
offset (the No-U-turn step, the generic tile's flow step on prescribed steps) compare chains [48, 64) with the float64 oracle fed
``split_at(key, 64, 48 + arange(16))`` at the tolerances of the tests they come from."""
import functools
import types

import numpy as np
import pytest

from oracle import flow, mala, prng, targets
from tests import shard_cases as sc

pytestmark = pytest.mark.gpu

B = sc.B


# ---- plumbing ---------------------------------------------------------------------------------------------------------------
def _dev(x, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def _keys_dev(keys):
    return _dev(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32))


def _buf(*shape, dtype="float32"):
    import torch
    return torch.empty(*shape, dtype=getattr(torch, dtype), device="cuda")


def _state(ctx, x, beta):
    pos = _dev(x); logp = _buf(pos.shape[0], dtype="float64"); grad = _buf(*pos.shape)
    ctx.mala_init(pos, beta, logp, grad)
    return pos, logp, grad


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def _assert_part_equals_rows(part, whole, off, n):
    assert set(part) == set(whole)
    for name in whole:
        np.testing.assert_array_equal(part[name], sc.rows(whole[name], name, off, n), err_msg=f"{name}, chains [{off}, {off + n})")


def _share_of_chains_that_differ(a, b, name):
    """Of two outputs over the same chains: the share of chains on which they differ anywhere."""
    if name in sc.CHAIN_AXIS_1:
        a, b = np.swapaxes(a, 0, 1), np.swapaxes(b, 0, 1)
    return (a != b).reshape(a.shape[0], -1).any(1).mean()


def _check_shards(open_ctx, call, x0, keys=None, control=()):
    """``open_ctx(n_local, offset)`` builds a context with ``n_chain_total = 64``; ``call(ctx, x rows, key rows or None)`` makes the
    entry point's call from those rows and returns its per-chain outputs as numpy arrays.  ``control``: the outputs that carry the
    draws, compared in the run at the wrong offset (more than half of the chains must differ from the whole run's; with a proposal
    among them every chain does)."""
    sub = (lambda a, off, n: None if a is None else a[off:off + n])
    ctx = open_ctx(B, 0)
    whole = call(ctx, x0, keys)
    ctx.close()
    for off, n in sc.PARTS:
        ctx = open_ctx(n, off)
        part = call(ctx, x0[off:off + n], sub(keys, off, n))
        ctx.close()
        _assert_part_equals_rows(part, whole, off, n)
    if control:
        off, n = sc.CONTROL
        ctx = open_ctx(n, 0)                                                       # the [16, 48) rows in a context that says offset 0
        wrong = call(ctx, x0[off:off + n], sub(keys, off, n))
        ctx.close()
        for name in control:
            share = _share_of_chains_that_differ(wrong[name], sc.rows(whole[name], name, off, n), name)
            print(f"control: {name} differs on {share:.0%} of the chains at the wrong offset")
            assert share > 0.5, (name, share)
    return whole


# ---- 1. the resident-chain kernels and 2. the No-U-turn sampler ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _target(name):
    """(args, dist, start [64, d] float32) of a target of shard_cases.TARGETS."""
    from tests import gpu_util as gu
    t = sc.TARGETS[name]
    if t["kind"] == "phi4":
        args, dist, *_ = gu.phi4_setup(d=t["d"], B=B, hidden=32, F=16)
    else:
        args, dist, *_ = gu.gmm4_setup(B=B)
    x0 = sc.mode_start(t["d"], B) if t["start"] == "mode" else dist.init_params.astype(np.float32)
    return args, dist, x0


def _opener(name, mass=None):
    from tests import gpu_util as gu
    args, dist, _ = _target(name)

    def open_ctx(n_local, offset):
        ctx = gu.make_ctx(dist, args, n_local=n_local, n_total=B, offset=offset)
        if mass is not None:
            ctx.set_inverse_mass(mass)
        return ctx
    return open_ctx


def _mass(d):
    from tests import hmc_mass_ref as hm
    return hm.log_spaced_mass(d)


def _resident_call(entry, tname, key):
    """The call of a resident-chain entry point with every output it offers; ``key``: the step-major key (key rows override it)."""
    t = sc.TARGETS[tname]
    n_steps, thin = sc.N_STEPS, sc.THIN

    def call(ctx, x, keys):
        n, d = x.shape
        k = key if keys is None else _keys_dev(keys)
        f64 = functools.partial(_buf, dtype="float64")
        tally = dict(n_acc=_buf(n, dtype="int32"), acc_sum=f64(n))
        last = dict(acc=_buf(n), is_acc=_buf(n, dtype="uint8"))
        traj = dict(traj_pos=_buf(n_steps // thin, n, d), traj_logp=f64(n_steps // thin, n))
        warm = dict(step_avg=f64(n), step_last=f64(n), step_traj=f64(n_steps, n))
        sums = dict(pos_sum=f64(n, d), pos_sumsq=f64(n, d))
        if entry == "mala_run":
            beta, eps = t["mala"]
            pos, logp, grad = _state(ctx, x, beta)
            out = dict(**tally, **last, **traj, proposed=_buf(n, d), weight=_buf(n))
            ctx.mala_run(k, beta, eps, n_steps, pos, logp, grad, thin=thin, **out)
        elif entry == "hmc_run":
            beta, eps = t["hmc"]
            pos, logp, grad = _state(ctx, x, beta)
            out = dict(**tally, **last, **traj)
            ctx.hmc_run(k, beta, eps, sc.LEAPFROG, n_steps, pos, logp, grad, thin=thin, **out)
        elif entry == "hmc_run_lengths":
            beta, eps = t["hmc"]
            pos, logp, grad = _state(ctx, x, beta)
            out = dict(**tally, **last, **traj)
            ctx.hmc_run_lengths(k, beta, eps, _dev(np.array(sc.LENGTHS, dtype=np.int32)), pos, logp, grad, thin=thin, **out)
        elif entry == "mala_warmup":
            beta, eps = t["mala_textbook"]
            pos, logp, grad = _state(ctx, x, beta)
            out = dict(**tally, **warm)
            avg = out.pop("step_avg")
            ctx.mala_warmup(k, beta, eps, n_steps, sc.MALA_TARGET, pos, logp, grad, avg, **out)
            out["step_avg"] = avg
        elif entry.startswith("hmc_warmup_window"):
            beta, eps = t["hmc"]
            pos, logp, grad = _state(ctx, x, beta)
            out = dict(**tally, **warm)
            avg = out.pop("step_avg")
            ctx.hmc_warmup_window(k, beta, eps, sc.LEAPFROG, n_steps, sc.HMC_TARGET, pos, logp, grad, avg, sums["pos_sum"], sums["pos_sumsq"], **out)
            out.update(step_avg=avg, **sums)
        elif entry == "nuts_warmup_window":
            beta, eps = t["nuts"]
            pos, logp, grad = _state(ctx, x, beta)
            out = dict(step_last=warm["step_last"], step_traj=warm["step_traj"], acc_sum=f64(n), leapfrog_sum=_buf(n, dtype="int64"),
                       n_divergent=_buf(n, dtype="int32"), depth_sum=_buf(n, dtype="int32"))
            ctx.nuts_warmup_window(k, beta, eps, sc.NUTS_DEPTH, n_steps, sc.HMC_TARGET, pos, logp, grad, warm["step_avg"], sums["pos_sum"],
                                   sums["pos_sumsq"], **out)
            out.update(step_avg=warm["step_avg"], **sums)
        else:
            raise KeyError(entry)
        return _np(dict(pos=pos, logp=logp, grad=grad, **out))
    return call


# what carries the draws in the control (resident.hip.h is one site: the control runs on mala_run, whose proposal is an output)
RESIDENT_CONTROL = {("mala_run", "phi4_d64", 0): ("proposed", "acc", "traj_pos")}


@pytest.mark.parametrize("key_mode", [0, 1])
@pytest.mark.parametrize("tname", list(sc.TARGETS))
@pytest.mark.parametrize("entry", sc.RESIDENT)
def test_resident_chain_kernels(entry, tname, key_mode):
    """``mfm_mala_run``, ``mfm_hmc_run``, ``mfm_hmc_run_lengths``, ``mfm_mala_warmup``, ``mfm_hmc_warmup_window`` (unit and installed mass)
    and ``mfm_nuts_warmup_window``: 4 steps, ``thin = 2``, step-major keys (mode 0: ``split(split(key, n_steps)[s], n_total)[offset + b]``)
    and per-chain keys (mode 1).  Instance: one wave per chain, MAXIT by d alone (NUTS: chains per workgroup by d and the depth limit),
    so 64, 32 and 16 chains run the same one."""
    _, _, x0 = _target(tname)
    mass = _mass(sc.TARGETS[tname]["d"]) if entry.endswith("_mass") else None
    key = prng.PRNGKey(21)
    keys = prng.split(prng.PRNGKey(33), B) if key_mode else None
    whole = _check_shards(_opener(tname, mass), _resident_call(entry, tname, key), x0, keys, RESIDENT_CONTROL.get((entry, tname, key_mode), ()))
    if "n_acc" in whole:                                                           # accepted and rejected steps both occur
        print(f"{entry} {tname} mode {key_mode}: accepted {whole['n_acc'].sum()} of {B * sc.N_STEPS}")
        assert 0 < whole["n_acc"].sum() < B * sc.N_STEPS
    # the chains adapt apart -- except from the phi-four d = 64 start, where every chain's p is exactly 1 or 0 in the first steps of the MALA
    # and HMC warmups (float64 restatement: 1, 1, 1, 0 and 1, 0, 0, 1; tests/test_gpu_warmup.py's docstring) and the step sizes part later
    if "step_avg" in whole and (tname != "phi4_d64" or entry == "nuts_warmup_window"):
        assert len(np.unique(whole["step_avg"])) > 1
    assert (whole["pos"] != x0).any()


def _nuts_call(entry, key, eps):
    from tests import nuts_util as nu
    n_tr = sc.NUTS_TRANSITIONS

    def call(ctx, x, keys):
        n, d = x.shape
        pos, logp, grad = _state(ctx, x, 1.0)
        info = nu._dev_info(n)
        if entry.startswith("nuts_run"):
            tot = dict(leapfrog_sum=_buf(n, dtype="int64"), acc_sum=_buf(n, dtype="float64"), n_divergent=_buf(n, dtype="int32"),
                       depth_sum=_buf(n, dtype="int32"), traj_pos=_buf(n_tr, n, d), traj_logp=_buf(n_tr, n, dtype="float64"))
            ctx.nuts_run(key if keys is None else _keys_dev(keys), 1.0, eps, sc.NUTS_DEPTH, n_tr, pos, logp, grad, thin=1, **tot, **info)
            return _np(dict(pos=pos, logp=logp, grad=grad, **tot, **info))
        out = {}
        for j in range(n_tr):                                                      # the single-step calls: every transition's state and info
            if entry == "nuts_step":
                ctx.nuts_step(prng.split(key, n_tr)[j], 1.0, eps, sc.NUTS_DEPTH, pos, logp, grad, **info)
            else:
                ctx.nuts_step_keys(_keys_dev(prng.split_rows(keys, n_tr)[:, j]), 1.0, eps, sc.NUTS_DEPTH, pos, logp, grad, **info)
            out.update({f"{k}_{j}": v for k, v in _np(dict(pos=pos, logp=logp, grad=grad, **info)).items()})
        return out
    return call


@pytest.mark.parametrize("mass", [False, True], ids=["unit", "mass"])
@pytest.mark.parametrize("entry", sc.NUTS)
def test_nuts(entry, mass):
    """``mfm_nuts_step``, ``mfm_nuts_step_keys`` and ``mfm_nuts_run`` (both key modes) on phi-four d = 64 at 0.03 (tests/test_gpu_nuts.py),
    depth limit 5, 3 transitions, unit mass and an installed one: position, log-density, gradient, tree depth, leapfrog count, both
    flags, rate and energy of every transition.  Instance: chains per workgroup follow (d, limit), not the chain count.  The control
    (nuts.hip) runs on ``mfm_nuts_step``."""
    _, _, x0 = _target("phi4_d64")
    per_chain = entry in ("nuts_step_keys", "nuts_run_mode1")
    keys = prng.split(prng.PRNGKey(34), B) if per_chain else None
    control = ("energy_0", "pos_0") if (entry, mass) == ("nuts_step", False) else ()
    whole = _check_shards(_opener("phi4_d64", _mass(64) if mass else None), _nuts_call(entry, prng.PRNGKey(22), sc.TARGETS["phi4_d64"]["nuts"][1]),
                          x0, keys, control)
    depth = whole["depth"] if "depth" in whole else whole["depth_0"]
    assert len(np.unique(depth)) > 1                                               # trees of several depths


# ---- 3. the Cox process on its fused kernel ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cox():
    from tests import gpu_util as gu
    args, dist, *_ = gu.lgcp_setup(n=8, B=B)
    return args, dist, dist.init_params.astype(np.float32)


@pytest.mark.parametrize("textbook", [True, False], ids=["textbook", "as-written"])
@pytest.mark.parametrize("entry", ["mala_step", "mala_run"])
def test_cox_process_on_the_fused_kernel(entry, textbook):
    """``mfm_mala_step`` and ``mfm_mala_run`` (key mode 0: its step keys come from ``mala_run_keys_kernel``) on the 8 x 8 grid, whose
    step is the 16-chain tile of lgcp.hip at every chain count below 128.  The control runs on both (lgcp.hip derives the step's keys,
    ``mala_run_keys_kernel`` the run's)."""
    from tests import gpu_util as gu
    args, dist, x0 = _cox()
    beta, eps, key = 0.45, 0.01, prng.PRNGKey(77)

    def open_ctx(n_local, offset):
        return gu.make_ctx(dist, args, n_local=n_local, n_total=B, offset=offset)

    def call(ctx, x, keys):
        n, d = x.shape
        pos, logp, grad = _state(ctx, x, beta)
        out = dict(acc=_buf(n), is_acc=_buf(n, dtype="uint8"), proposed=_buf(n, d), weight=_buf(n))
        if entry == "mala_step":
            ctx.mala_step(key, beta, eps, pos, logp, grad, out["acc"], out["is_acc"], out["proposed"], out["weight"], textbook=textbook)
        else:
            out.update(n_acc=_buf(n, dtype="int32"), acc_sum=_buf(n, dtype="float64"), traj_pos=_buf(sc.N_STEPS // sc.THIN, n, d),
                       traj_logp=_buf(sc.N_STEPS // sc.THIN, n, dtype="float64"))
            ctx.mala_run(key, beta, eps, sc.N_STEPS, pos, logp, grad, thin=sc.THIN, textbook=textbook, **out)
        return _np(dict(pos=pos, logp=logp, grad=grad, **out))
    whole = _check_shards(open_ctx, call, x0, None, ("proposed",) if textbook else ())
    assert (whole["proposed"] != x0).any()


# ---- 4. the flow step ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _flow_setup(family, mode, fixed):
    """(args, dist, model, params, beta, start) of a flow-step family: the setups and tamed parameters of tests/test_gpu_replay.py,
    tests/test_gpu_d2tile.py, tests/test_gpu_fixed.py and tests/test_gpu_fixed_families.py (attempt counts in the tens)."""
    from tests import gpu_util as gu
    from tests.test_gpu_replay import _tamed
    kw = dict(ode_method=fixed[0], ode_steps=fixed[1]) if fixed else {}
    if mode == "cis":
        kw["num_importance_samples"] = sc.CIS_SAMPLES
    if family.startswith("d2"):
        args, dist, k, model, state = gu.gmm4_setup(B=B, hidden=128, F=128, hutchs=False, **kw)
        params, beta = gu.rand_params(model, seed=9, out_scale=0.3), 0.7
    elif family == "fast":
        args, dist, k, model, state = gu.phi4_setup(d=64, B=B, **kw)
        params, beta = _tamed(model, out_scale=0.05), 1e-3
    else:
        args, dist, k, model, state = gu.phi4_setup(d=64, B=B, hidden=32, F=16, **kw)
        params = _tamed(model, out_scale=0.5) if fixed else _tamed(model, out_scale=2.0)
        # (conditional importance sampling at an early annealing temperature: at 0.8 every weight of a fresh flow sample underflows
        # against the current state's and no chain moves; at 1e-3 the float64 oracle accepts 10 of 16)
        beta = 1e-3 if mode == "cis" else 0.8
    return args, dist, model, params, beta, dist.init_params.astype(np.float32)


def _cis_step(ctx, args, dist, n_total, offset, key, beta, pos, logp):
    """The product's conditional-importance-sampling flow step (exe_flow_matching.create_train_data_gn) on a bare context: the engine
    it asks for is this namespace -- the shard geometry and the context -- and the step is the product's own code, key slicing included."""
    import torch
    from mfm_amd import exe_flow_matching as E
    eng = types.SimpleNamespace(ctx=ctx, torch=torch, dev=pos.device, n_local=pos.shape[0], n_valid=pos.shape[0], n_total=n_total,
                                offset=offset, dim=pos.shape[1])
    gen, _, _ = E.create_train_data_gn(dist, _Bound(eng).apply, None, args)
    grad = torch.zeros_like(pos)
    gen(key, (pos, logp, grad), int(args.mcmc_per_flow_steps) + 1, None, beta)      # count = K + 1: the flow iteration
    b = gen.info_buffers
    return dict(acc=b["acc"], is_acc=b["isacc"], proposed=b["prop"], weight=b["w"])


class _Bound:
    """``create_train_data_gn`` finds the engine through the vector field's bound ``apply``."""

    def __init__(self, engine):
        self.engine = engine

    def apply(self, *a, **kw):
        raise NotImplementedError


@pytest.mark.parametrize("case", list(sc.FLOW))
def test_flow_step(monkeypatch, case):
    """``mfm_flow_step`` on its natural controller (adaptive steps: a deterministic function of row and key, attempt counts compared
    exactly) and in fixed-step mode where the family has one; random-walk, independent and conditional-importance-sampling modes.
    Instances: the generic tile does not depend on the chain count; the d = 2 tile does and is pinned with MFM_D2_TILE; the
    shape-specialised solver's chains per workgroup (2 below 513 chains) is pinned with MFM_FLOW_LIVE all the same.  The wide family is
    left on its own plan, which is NOT the same in both runs: the batched time-branch GEMMs of 64 chains (5 x 64 = 320 rows) take
    ``gemm_kernel<1, 2>`` where 16 and 32 chains take ``gemm_kernel<1, 1>`` (the test prints the tallies).  The two are one kernel
    template whose wave owns one or two 16-wide feature tiles; an output element accumulates its K blocks in the same order in both,
    so the bits agree -- as they must, since a production shard (1,024 rows) and the whole run never share a plan either."""
    from mfm_amd import _lib
    from tests import gpu_util as gu
    family, mode, fixed = sc.FLOW[case]
    if family.startswith("d2"):
        monkeypatch.setenv("MFM_D2_TILE", family[3:])
    if family == "fast":
        monkeypatch.setenv("MFM_FLOW_LIVE", "2")
    args, dist, model, params, beta, x0 = _flow_setup(family, mode, fixed)
    key = prng.PRNGKey(31)
    kw = dict(family=_lib.FAMILY_WIDE) if family == "wide" else {}
    if mode == "cis":
        kw["max_eval"] = B * sc.CIS_SAMPLES

    def open_ctx(n_local, offset):
        ctx = gu.make_ctx(dist, args, n_local=n_local, n_total=B, offset=offset, fourier=model.f, params=params, **kw)
        ctx.shard = (B, offset)
        return ctx

    def call(ctx, x, keys):
        n, d = x.shape
        pos, logp, grad = _state(ctx, x, beta)
        if mode == "cis":
            out = _cis_step(ctx, args, dist, ctx.shard[0], ctx.shard[1], key, beta, pos, logp)
            return _np(dict(pos=pos, logp=logp, **out))
        out = dict(acc=_buf(n), is_acc=_buf(n, dtype="uint8"), proposed=_buf(n, d), nsteps=_buf(n, dtype="int32"))
        ctx.flow_step(_lib.FLOW_IMH if mode == "imh" else _lib.FLOW_RWMH, key, beta, pos, logp, grad, out["acc"], out["is_acc"], out["proposed"], out["nsteps"])
        if family == "wide":
            assert ctx.cfg.kernel_family == _lib.FAMILY_WIDE
            print(f"{case}, {n} chains: GEMM launches {({k: v for k, v in ctx.wide_gemm_tally().items() if v})}")
        return _np(dict(pos=pos, logp=logp, grad=grad, **out))
    whole = _check_shards(open_ctx, call, x0, None, ("proposed",) if case in sc.FLOW_CONTROLS else ())
    if "nsteps" in whole:
        print(f"{case}: attempts mean {whole['nsteps'].mean():.1f} max {whole['nsteps'].max()}, accepted {whole['is_acc'].sum()} of {B}")
        assert (whole["nsteps"] == 2 * fixed[1]).all() if fixed else whole["nsteps"].min() >= 2
    assert (whole["proposed"] != x0).any()


# ---- 5. the fused training iteration -------------------------------------------------------------------------------------------
def _relerr(a, b):
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


@pytest.mark.parametrize("case", list(sc.FUSED))
def test_fused_train_iter(case):
    """``mfm_train_iter`` with its MALA step inside the training kernel (fm.hip: the key of ``m.chain_offset``), the default call of every
    iteration once there is more than one rank, on the three fusable instances: counts 1..3 of K = 3, no optimizer update.  Every part's
    chains equal the whole run's rows bit for bit AND the same part composed from ``mfm_mala_step`` + ``mfm_fm_loss_grad``, losses and
    gradients included; the parts' losses and gradients sum to the whole run's within the bounds of tests/test_gpu_fm.py (1e-9 and 1e-5
    relative: summation order).  Instance: by the network's shape alone.  The control: at the wrong offset the acceptance probabilities
    (the step's draws) and the loss (the batch's draws) both change."""
    from mfm_amd._lib import FLOW_RWMH
    from tests import gpu_util as gu
    d, hidden, F, eps = sc.FUSED[case]
    args, dist, k, model, state = gu.phi4_setup(d=d, B=B, hidden=hidden, F=F)
    params = gu.rand_params(model, seed=3, out_scale=0.05)
    x0 = dist.init_params.astype(np.float32)
    ks, iter_keys = prng.PRNGKey(5), []
    for _ in range(sc.FUSED_K):
        ks, kg, kt = prng.split(ks, 3)
        iter_keys.append((kg, kt))

    def run(n_local, offset, rows_from, fused):
        import torch
        ctx = gu.make_ctx(dist, args, n_local=n_local, n_total=B, offset=offset, fourier=model.f, params=params)
        pos, logp, grad = _state(ctx, x0[rows_from:rows_from + n_local], 1.0)
        acc = _buf(n_local)
        out = {}
        for count, (kg, kt) in enumerate(iter_keys, start=1):
            loss = torch.zeros(1, dtype=torch.float64, device="cuda"); grads = torch.zeros(ctx.n_params, device="cuda")
            if fused:
                ctx.train_iter(count, sc.FUSED_K, FLOW_RWMH, kg, kt, 1.0, eps, pos, logp, grad, loss, grads, acc=acc, apply_update=False)
            else:
                ctx.mala_step(kg, 1.0, eps, pos, logp, grad, acc)
                ctx.fm_loss_grad(kt, pos, loss, grads)
            out.update({f"{k}_{count}": v for k, v in _np(dict(pos=pos, logp=logp, grad=grad, acc=acc, loss=loss, grads=grads)).items()})
        # the step rode in the training kernel: its traffic tally is 4 (4 d + 4) bytes per chain (the proposal never leaves the workgroup),
        # that of mfm_mala_step 4 (5 d + 5) (api.hip)
        assert ctx.counters()["mala_hbm_bytes"] == sc.FUSED_K * n_local * 4 * ((4 if fused else 5) * (d + 1))
        ctx.close()
        return out
    per_chain = [f"{k}_{c}" for k in ("pos", "logp", "grad", "acc") for c in range(1, sc.FUSED_K + 1)]
    whole = run(B, 0, 0, True)
    tot = {k: 0.0 for k in whole if k not in per_chain}
    for off, n in sc.PARTS:
        part, composed = run(n, off, off, True), run(n, off, off, False)
        for name in per_chain:
            np.testing.assert_array_equal(part[name], whole[name][off:off + n], err_msg=f"{name}, chains [{off}, {off + n})")
        for name in part:
            np.testing.assert_array_equal(part[name], composed[name], err_msg=f"{name} against the separate calls, chains [{off}, {off + n})")
        for name in tot:
            tot[name] = tot[name] + part[name].astype(np.float64)
    for c in range(1, sc.FUSED_K + 1):
        full_l, full_g = whole[f"loss_{c}"].item(), whole[f"grads_{c}"].astype(np.float64)
        print(f"{case} count {c}: loss sum rel. diff {abs(tot[f'loss_{c}'].item() - full_l) / abs(full_l):.2e}, gradient {_relerr(tot[f'grads_{c}'], full_g):.2e}; "
              f"mean acceptance {whole[f'acc_{c}'].mean():.3f}")
        assert 0.1 < whole[f"acc_{c}"].mean() < 0.9                                 # proposals are accepted and rejected: the end state is sensitive too
        assert abs(tot[f"loss_{c}"].item() - full_l) < 1e-9 * abs(full_l)
        assert _relerr(tot[f"grads_{c}"], full_g) < 1e-5
    off, n = sc.CONTROL
    wrong = run(n, 0, off, True)
    share = (wrong["acc_1"] != whole["acc_1"][off:off + n]).mean()
    part_loss = run(n, off, off, True)["loss_1"].item()
    print(f"control: acceptance probability differs on {share:.0%} of the chains, loss {wrong['loss_1'].item()} against {part_loss}")
    assert share > 0.5 and wrong["loss_1"].item() != part_loss


# ---- 6. oracle anchors at an offset --------------------------------------------------------------------------------------------
def test_nuts_step_at_an_offset_matches_the_reference():
    """Chains [48, 64) of 64 in their own context, from the reference's burned-in state (tests/nuts_util.py), one ``mfm_nuts_step``
    against tests/nuts_ref.py fed ``split_at(key, 64, 48 + arange(16))``: the borderline rule and the bounds of tests/test_gpu_nuts.py."""
    from tests import gpu_util as gu, nuts_ref as nr, nuts_util as nu
    from tests.test_gpu_nuts import CASES, DEPTH
    kind, d, tail, eps = CASES["phi4-64"]
    off, n = sc.PARTS[2]
    start = nu.burned(kind, d, tail, eps, DEPTH, False)["start"][off:off + n]
    args, dist, odist = nu._setup(kind, d, tail)
    vg = targets.Tempered(odist, 1.0).value_and_grad
    ctx = gu.make_ctx(dist, args, n_local=n, n_total=B, offset=off)
    pos, logp, grad = _state(ctx, start, 1.0)
    st = mala.MALAState(pos.cpu().numpy().astype(np.float64), logp.cpu().numpy(), grad.cpu().numpy().astype(np.float64))
    key, buf = prng.PRNGKey(50), nu._dev_info(n)
    ctx.nuts_step(key, 1.0, eps, DEPTH, pos, logp, grad, **buf)
    st_o, info = nr.kernel(prng.split_at(key, B, off + np.arange(n)), st, vg, eps, DEPTH)
    border = nu._borderline(kind, st.logdensity, info)
    assert border.mean() <= 0.25, border.mean()
    nu._compare(kind, st_o, info, (pos, logp), buf, ~border, "chains [48, 64)")
    ctx.close()


def test_flow_step_at_an_offset_matches_oracle_on_prescribed_steps():
    """Chains [48, 64) of 64 in their own context: the generic tile's random-walk flow step on the oracle's step sequence, the oracle
    fed ``split_at(key, 64, 48 + arange(16))`` -- the comparison and the phi-four bounds of tests/test_gpu_rank_slices.py."""
    import torch
    from mfm_amd import _lib
    from tests import gpu_util as gu
    from tests.test_gpu_replay import _replay_arrays
    args, dist, model, params, beta, x0 = _flow_setup("tile", "rwmh", None)
    off, n = sc.PARTS[2]
    d = x0.shape[1]
    vg = targets.Tempered(dist, beta).value_and_grad
    ctx = gu.make_ctx(dist, args, n_local=n, n_total=B, offset=off, fourier=model.f, params=params)
    pos, logp, grad = _state(ctx, x0[off:off + n], beta)
    st0 = mala.MALAState(x0[off:off + n].astype(np.float64), logp.cpu().numpy(), grad.cpu().numpy().astype(np.float64))
    key = prng.PRNGKey(31)
    keys = prng.split_at(key, B, off + np.arange(n))
    nat = {}
    flow.rwmh_step(keys, st0, vg, model, params, args, nat)
    dt, ac = _replay_arrays([nat["inv"], nat["fwd"]])
    rp = dict(inv=dict(dt=dt[0].astype(np.float64), acc=ac[0]), fwd=dict(dt=dt[1].astype(np.float64), acc=ac[1]))
    so = {}
    new_o, info_o = flow.rwmh_step(keys, st0, vg, model, params, args, so, replay=rp)
    ratio = torch.zeros(dt.shape, device="cuda"); own = torch.zeros(dt.shape, device="cuda"); diag = torch.zeros(n, 4, dtype=torch.float64, device="cuda")
    ctx.debug_replay(_dev(dt), _dev(ac), ratio, own, diag)
    a, ia, pr, ns = _buf(n), _buf(n, dtype="uint8"), _buf(n, d), _buf(n, dtype="int32")
    ctx.flow_step(_lib.FLOW_RWMH, key, beta, pos, logp, grad, a, ia, pr, ns)
    np.testing.assert_array_equal(ns.cpu().numpy(), so["n_att_inv"] + so["n_att_fwd"])      # attempt counts: exact
    dg = diag.cpu().numpy()
    vs = max(1.0, np.abs(so["vol0"]).max(), np.abs(so["volp"]).max())
    e_p = np.abs(pr.cpu().numpy() - info_o.proposed_position).max()
    e_v0, e_vp = np.abs(dg[:, 0] - so["vol0"]), np.abs(dg[:, 1] - so["volp"])
    e_v, e_la = np.maximum(e_v0, e_vp), np.abs(dg[:, 3] - so["log_alpha"])
    print(f"chains [48, 64): attempts {ns.float().mean().item():.0f}, |dx'| {e_p:.2e}, |dvol| q90 {np.quantile(e_v, 0.9):.2e} max {e_v.max():.2e} (scale {vs:.1f}), "
          f"|d log alpha| med {np.median(e_la):.2e} max {e_la.max():.2e}")
    assert e_p < 3e-5 * max(1.0, np.abs(info_o.proposed_position).max())
    assert np.quantile(e_v, 0.9) < 2e-5 * vs and e_v.max() < 2e-3 * vs
    gn = vg(info_o.proposed_position.astype(np.float64))[1]
    dxp = np.linalg.norm(pr.cpu().numpy() - info_o.proposed_position, axis=1)
    bound = 2.0 * np.linalg.norm(gn, axis=1) * dxp + e_v0 + e_vp + 1e-3
    assert (e_la <= bound).all(), (e_la / bound).max()
    same = ia.cpu().numpy().astype(bool) == info_o.is_accepted
    assert same.mean() > 0.9
    np.testing.assert_allclose(pos.cpu().numpy()[same], new_o.position[same], atol=3e-5 * max(1.0, np.abs(new_o.position).max()))
    ctx.close()
