"""GPU parity of every AdamW path against the oracle's TrainState (exe_flow_matching.py:116-137,184-198:
apply_if_finite(chain(adamw(mask = not bias), clip), 10) with a linear warmup + decay schedule), at settings where every term
of the update is visible: weight decay and its mask, the update clip, the warmup branch, the schedule's count against the
step, the bias corrections, epsilon, the 11th consecutive non-finite gradient and mfm_reset_optimizer.

The device paths (api.hip: mfm_adamw_step, mfm_train_iter) and how a case reaches them:
  A  optim.hip adamw_vec_kernel           mfm_adamw_step, every width a multiple of 4, no joint-row remap
  B  optim.hip adamw_kernel               mfm_adamw_step, ragged widths or the joint-row remap (d = 2)
  C  optim.hip finite_decide_kernel + A/B mfm_adamw_step on a buffer mfm_fm_loss_grad did not just check (every synthetic case)
  D  wgrad_sk.hip fused combine + update  mfm_train_iter, tile family, one rank
  E  wgrad_sk.hip deferred update         D with a non-finite partial, or MFM_DEBUG_FORCE_EXCHANGE=1
  F  optim.hip reduce_adamw_kernel        mfm_train_iter with MFM_WGRAD_SLABS=1
Every call hands the oracle the exact float32 gradient the device applied (the caller's buffer, or what mfm_train_iter wrote
to d_grads), so the comparison sees the optimizer alone.

Bound on |w_dev - w_oracle| after n accepted updates (both float32; derived, not fitted):
  * moments: the device forms m = fma(b1, m, (1 - b1) g) and v = fma(b2, v, (1 - b2) g g), the oracle rounds the product
    b1 m (b2 v) before the add: 1 rounding of 2^-24 apart per step, carried with weight b1^k (b2^k).  Summed over the
    history that is < 8 * 2^-24 relative to the terms of m, and |m_hat| / sqrt(v_hat) <= 1.6 for b1^2 < b2 (Cauchy-Schwarz
    over the two geometric weights at b1 = 0.8, b2 = 0.95), so the Adam direction differs by < 2^-20;
  * the two divisions, sqrtf (correctly rounded) and the + eps: 4 roundings, < 2^-22; the decay as fma against
    multiply + add: 2^-24 wd |w|, negligible;
  * so the update lr * (adam + wd w) differs by < 2 lr_peak 2^-20 per step, and w + u is rounded to the nearest float on
    both sides: + 1 ulp(w) per step, with |w| bounded by its final value + n * clip (no step moves it by more than clip).
  |dw| <= n * (ulp(|w| + n clip) + 2 * lr_peak * 2^-20)
The sensitivity self-check then replays the oracle with one planted bug at a time and requires each to land at least 10x
outside that bound on some element: the comparison would catch every one of them."""
import numpy as np
import pytest

from oracle import fm, optim, prng

f32 = np.float32
LR, WD, EPS, B1, B2 = 1e-2, 0.2, 1e-3, 0.8, 0.95
WARM, LITER = 3, 9
N_CALLS, BAD_CALL = 14, 1          # call 1 (during warmup) gets a non-finite gradient: step and count part from there on
K_MCMC = 100                       # mcmc_per_flow_steps of the mfm_train_iter cases: every call a MALA step


def _opt(clip, warmup=WARM, learning_iter=LITER):
    return dict(learning_rate=LR, adam_b1=B1, adam_b2=B2, adam_eps=EPS, weight_decay=WD, update_clip=clip,
                learning_iter=learning_iter, warmup_steps=warmup)


def _bound(w_o, n, clip):
    return n * (np.spacing((np.abs(w_o) + n * clip).astype(f32)).astype(np.float64) + 2 * LR * 2.0 ** -20)


def _decay_mask(model):
    return np.concatenate([np.concatenate([np.ones(fi * fo, bool), np.zeros(fo, bool)]) for fi, fo in model.layer_shapes()])


# ---- the oracle's update restated on flat arrays, with switches that each plant one bug --------------------------------------
MUTANTS = {
    "no weight decay": dict(wd=0.0),
    "decay on biases": dict(bias_decay=True),
    "no update clip": dict(clip=np.inf),
    "warmup ignored": dict(warmup=0),
    "schedule on step": dict(lr_by_step=True),
    "bias correction at count": dict(bc_at_count=True),
    "eps = 0": dict(eps=0.0),
}


def restated(w0, grads, finite, decay, clip, wd=WD, eps=EPS, warmup=WARM, bias_decay=False, lr_by_step=False, bc_at_count=False,
             learning_iter=LITER, max_err=10):
    """oracle.optim.TrainState.apply_gradients element by element (it is elementwise apart from the finite check, which
    `finite[i]` carries for the WHOLE gradient of call i, so a subset of the elements can be replayed).  Returns the parameters
    after every call and, per call, the fraction of decayed elements whose unclipped update exceeds the clip."""
    lr_fn = optim.learning_rate_fn(learning_iter, warmup, LR)
    w = w0.astype(f32).copy()
    m, v = np.zeros_like(w), np.zeros_like(w)
    dec = decay | bias_decay
    b1, b2, epsf, wdf = f32(B1), f32(B2), f32(eps), f32(wd)
    step = count = nf = 0
    out, frac = [], []
    for g, fin in zip(grads, finite):
        nf = 0 if fin else nf + 1
        step += 1
        fr = np.nan
        if fin or nf > max_err:
            c1 = count if bc_at_count else count + 1
            bc1, bc2 = f32(1.0 - B1 ** c1), f32(1.0 - B2 ** c1)
            lr = f32(-lr_fn(step - 1 if lr_by_step else count))
            with np.errstate(all="ignore"):
                m = b1 * m + (f32(1) - b1) * g
                v = b2 * v + (f32(1) - b2) * g * g
                u = (m / bc1) / (np.sqrt(v / bc2) + epsf)
                u = np.where(dec, u + wdf * w, u)
                u = lr * u
                fr = float(np.mean(np.abs(u[decay]) > f32(clip))) if decay.any() else np.nan
                w = (w + np.clip(u, -f32(clip), f32(clip))).astype(f32)
            count = count + 1
        out.append(w.copy())
        frac.append(fr)
    return out, frac


def test_restated_oracle_is_the_oracle():
    """The restatement the sensitivity checks mutate is bit-for-bit the oracle (decay mask, warmup, a rejected update, the
    11th non-finite gradient applied)."""
    rng = np.random.default_rng(1)
    params = [{"kernel": rng.standard_normal((6, 4)).astype(f32), "bias": rng.standard_normal(4).astype(f32)},
              {"kernel": rng.standard_normal((4, 3)).astype(f32), "bias": rng.standard_normal(3).astype(f32)}]
    flat = lambda ps: np.concatenate([np.concatenate([p["kernel"].ravel(), p["bias"]]) for p in ps])
    decay = np.concatenate([np.concatenate([np.ones(p["kernel"].size, bool), np.zeros(p["bias"].size, bool)]) for p in params])
    st = optim.TrainState(params, optim.learning_rate_fn(LITER, WARM, LR), B1, B2, EPS, WD, 5e-3)
    gs, fin, ref = [], [], []
    for i in range(25):
        g = [{k: (rng.standard_normal(v.shape) * 10.0 ** -(2 * j)).astype(f32) for k, v in p.items()} for j, p in enumerate(params)]
        if i == BAD_CALL or i >= 14:
            g[1]["bias"][2] = np.inf
        with np.errstate(all="ignore"):
            st.apply_gradients(g)
        gs.append(flat(g)); fin.append(bool(np.isfinite(gs[-1]).all())); ref.append(flat(st.params))
    got, _ = restated(flat(params), gs, fin, decay, 5e-3)
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a, b)
    assert np.isnan(ref[-1]).sum() == 1 and st.count == 14


# ---- device drivers: one call of a path, returning the float32 gradient it applied --------------------------------------------
def _dev(x, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


class _Driver:
    """`mode`: synth (mfm_adamw_step on a synthetic gradient: C + A/B), sep (mfm_fm_loss_grad + mfm_adamw_step on the same
    buffer: A/B with the decision in line), clone (the same on a copy: C), iter (mfm_train_iter: D/E/F, or A/B behind it with
    MFM_NO_FUSED_OPT=1); an iter call `via_c` runs mfm_train_iter without the update, then mfm_adamw_step on a copy (C)."""

    def __init__(self, ctx, model, dist, mode, seed=0):
        import torch
        self.ctx, self.model, self.mode = ctx, model, mode
        self.rng = np.random.default_rng(seed)
        self.n = ctx.n_params
        L = len(model.layer_shapes())
        # a scale per layer from 1 down to 1e-3: gradients over three decades, the smallest ones at eps
        self.scale = np.concatenate([np.full(fi * fo + fo, 10.0 ** (-3.0 * l / (L - 1))) for l, (fi, fo) in enumerate(model.layer_shapes())])
        self.decay = _decay_mask(model)
        self.bad_idx = (int(np.flatnonzero(self.decay)[self.n // 3]), int(np.flatnonzero(~self.decay)[-5]))
        x = dist.init_params if hasattr(dist, "init_params") else np.random.default_rng(4).normal(size=(ctx.cfg.n_chain_local, dist.dim))
        self.x32 = np.ascontiguousarray(x, dtype=f32)
        self.B, self.d = self.x32.shape
        self.nan_at = (5, min(7, self.d - 1))
        self.keys = prng.PRNGKey(5 + seed)
        self.count = 0
        self.pos = _dev(self.x32)
        self.loss = torch.zeros(1, dtype=torch.float64, device="cuda")
        self.grads = torch.zeros(self.n, device="cuda")
        if mode.startswith("iter"):
            self.logp = torch.empty(self.B, device="cuda", dtype=torch.float64); self.grad = torch.empty_like(self.pos)
            self.acc = torch.empty(self.B, device="cuda")
            ctx.mala_init(self.pos, 1.0, self.logp, self.grad)

    def __call__(self, bad, via_c=False):
        from mfm_amd._lib import FLOW_RWMH
        ctx = self.ctx
        self.count += 1
        self.keys, kg, kt = prng.split(self.keys, 3)
        if self.mode == "synth":
            g = (self.rng.standard_normal(self.n) * self.scale).astype(f32)
            if bad:
                g[list(self.bad_idx)] = np.inf          # one kernel element, one bias element
            ctx.adamw_step(_dev(g))
            return g
        if bad:
            saved = self.pos[self.nan_at].item()
            self.pos[self.nan_at] = float("nan")
        if self.mode in ("sep", "clone"):
            ctx.fm_loss_grad(kt, self.pos, self.loss, self.grads)
            ctx.adamw_step(self.grads if self.mode == "sep" else self.grads.clone())
        else:
            ctx.train_iter(self.count, K_MCMC, FLOW_RWMH, kg, kt, 1.0, 1e-4 if self.d > 2 else 0.2, self.pos, self.logp, self.grad,
                           self.loss, self.grads, acc=self.acc, apply_update=not via_c)
            if via_c:
                ctx.adamw_step(self.grads.clone())
        g = self.grads.cpu().numpy()
        if bad:
            self.pos[self.nan_at] = saved
            if self.mode.startswith("iter"):
                self.ctx.mala_init(self.pos, 1.0, self.logp, self.grad)
        assert np.isfinite(g).all() != bad, (self.count, bad)
        return g


# ---- cases -----------------------------------------------------------------------------------------------------------------
RAGGED = ([20, 50], [30, 24], [100, 36])        # test_gpu_depth.py: widths that are not multiples of 4 / 16, fused tile family
ONE = ([32], [32], [32])
THREE = ([32, 48, 32], [48, 32, 16], [64, 32, 48])

# name: (setup, setup kwargs, family, mode, env, update clip)
CASES = {
    "headline-synth":     ("phi4", dict(d=256, hidden=128, F=128), None, "synth", {}, 5e-3),           # C + A
    "headline-sep":       ("phi4", dict(d=256, hidden=128, F=128), None, "sep", {}, 5e-3),             # A, decision in line
    "headline-clone":     ("phi4", dict(d=256, hidden=128, F=128), None, "clone", {}, 5e-3),           # C + A
    "headline-iter":      ("phi4", dict(d=256, hidden=128, F=128), None, "iter", {}, 5e-3),            # D
    "headline-iter-exch": ("phi4", dict(d=256, hidden=128, F=128), None, "iter", {"MFM_DEBUG_FORCE_EXCHANGE": "1"}, 5e-3),   # E
    "headline-iter-slabs": ("phi4", dict(d=256, hidden=128, F=128), None, "iter", {"MFM_WGRAD_SLABS": "1"}, 5e-3),           # F
    "headline-iter-nofused": ("phi4", dict(d=256, hidden=128, F=128), None, "iter", {"MFM_NO_FUSED_OPT": "1"}, 5e-3),        # A behind train_iter
    "phi4-64-synth":      ("phi4", dict(d=64, hidden=32, F=16), None, "synth", {}, 5e-3),               # C + A
    "phi4-64-iter":       ("phi4", dict(d=64, hidden=32, F=16), None, "iter", {}, 5e-3),                # D
    "phi4-64-iter-slabs": ("phi4", dict(d=64, hidden=32, F=16), None, "iter", {"MFM_WGRAD_SLABS": "1"}, 5e-3),               # F
    "ragged-synth":       ("phi4", dict(d=64, hidden=RAGGED, F=16), "tile", "synth", {}, 5e-3),         # C + B
    "ragged-iter":        ("phi4", dict(d=64, hidden=RAGGED, F=16), "tile", "iter", {}, 5e-3),          # D through the joint-row remap
    "gmm4-synth":         ("gmm", dict(hidden=32, F=16), None, "synth", {}, 5e-3),                      # C + B
    "gmm4-iter":          ("gmm", dict(hidden=32, F=16), None, "iter", {}, 5e-3),                       # D
    "depth-1-1-1-sep":    ("phi4", dict(d=64, hidden=ONE, F=16), "wide", "sep", {}, 5e-3),             # A, wide family
    "depth-3-3-3-sep":    ("phi4", dict(d=64, hidden=THREE, F=16), "wide", "sep", {}, 5e-3),           # A, wide family
}
PINES = ("lgcp", dict(n=32, hidden=1024, F=128), None, "synth", {}, 5e-3)   # 8.65 M parameters: A with the 2048-workgroup grid


def _make(case, monkeypatch, opt, seed=0):
    from mfm_amd import _lib
    from tests import gpu_util as gu
    setup, kw, family, mode, env, clip = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)                 # read at mfm_create
    B = 64
    if setup == "phi4":
        args, dist, k, model, state = gu.phi4_setup(B=B, **kw)
    elif setup == "gmm":
        args, dist, k, model, state = gu.gmm4_setup(B=B, **kw)
    else:
        args, dist, k, model, state = gu.lgcp_setup(B=B, **kw)
    params = gu.rand_params(model, seed=3, out_scale=0.05)
    fam = {None: None, "tile": _lib.FAMILY_TILE, "wide": _lib.FAMILY_WIDE}[family]
    ctx = gu.make_ctx(dist, args, fourier=model.f, params=params, family=fam, opt=opt)
    if family is not None:
        assert ctx.cfg.kernel_family == fam
    return ctx, args, dist, model, params, _Driver(ctx, model, dist, mode, seed)


def _check_call(ctx, st, applied, lr_fn, clip, tag):
    """opt_state against the oracle's counters; master parameters within the bound, NaN exactly where the oracle has NaN."""
    from tests import gpu_util as gu
    s = ctx.opt_state()
    assert (s["step"], s["count"], s["notfinite_count"], s["last_applied"]) == (st.step, st.count, st.notfinite_count, int(applied)), (tag, s)
    assert s["last_lr"] == f32(lr_fn(st.step - 1)), (tag, s["last_lr"], lr_fn(st.step - 1))
    w, w_o = ctx.get_params(), gu.flat_params(st.params)
    nan = np.isnan(w_o)
    bad = np.flatnonzero(np.isnan(w) != nan)
    assert bad.size == 0, (tag, "NaN pattern differs from the oracle's", bad[:8], w[bad[:8]], w_o[bad[:8]])
    err = np.abs(w[~nan].astype(np.float64) - w_o[~nan])
    bnd = _bound(w_o[~nan], st.count, clip)
    i = int(np.argmax(err / bnd)) if err.size else 0
    assert err.size == 0 or err[i] <= bnd[i], (tag, "|dw| above the float32 bound", i, err[i], bnd[i])
    return w


def _run_sequence(ctx, drv, model, params, clip, bads, lr_fn, tag, via_c=()):
    from tests import gpu_util as gu
    st = optim.TrainState(params, lr_fn, B1, B2, EPS, WD, clip)
    gs, fin, devs, counts = [], [], [], []
    for i, bad in enumerate(bads):
        counts.append(st.count)
        g = drv(bad, via_c=i in via_c)
        with np.errstate(all="ignore"):
            applied = st.apply_gradients(gu.unflat_params(model, g))
        devs.append(_check_call(ctx, st, applied, lr_fn, clip, f"{tag} call {i}"))
        gs.append(g); fin.append(bool(np.isfinite(g).all()))
    return st, gs, fin, devs, counts


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES) + ["pines-synth"])
def test_update_matches_oracle_with_every_term_visible(name, monkeypatch):
    """Warmup 3, decay to 0 at count 9 of 13 accepted updates, one rejected update at call 1: per call, the master parameters
    within the derived bound of the oracle fed the device's gradient, and opt_state's counters and logged learning rate equal
    to the oracle's; at the end the packed copies the GEMMs read follow (fm_loss against the oracle on the final parameters).
    Then the same inputs replayed through the oracle with one planted bug at a time must each miss the device by >= 10x the
    bound somewhere, and the clip must bite on 20 - 80 % of the kernel elements on a full-rate step."""
    import torch
    case = PINES if name == "pines-synth" else CASES[name]
    clip = case[5]
    n_calls = 4 if name == "pines-synth" else N_CALLS
    # the pines width: 4 calls with warmup 1 (one full-rate step, count 1) and the rejected update at call 2
    warm, bad_call = (1, 2) if name == "pines-synth" else (WARM, BAD_CALL)
    ctx, args, dist, model, params, drv = _make(case, monkeypatch, _opt(clip, warmup=warm))
    lr_fn = optim.learning_rate_fn(LITER, warm, LR)
    bads = [i == bad_call for i in range(n_calls)]
    st, gs, fin, devs, counts = _run_sequence(ctx, drv, model, params, clip, bads, lr_fn, name)
    assert st.step == n_calls and st.count == n_calls - 1 and (n_calls < N_CALLS or st.count > LITER)
    # packed copies
    key = prng.PRNGKey(1)
    loss = torch.zeros(1, dtype=torch.float64, device="cuda")
    ctx.fm_loss(key, _dev(drv.x32), loss)
    lo, _ = fm.loss_and_grad(model, st.params, key, drv.x32.astype(np.float64), args.sigma, need_grad=False)
    assert abs(loss.item() - lo) < 3e-5 * abs(lo), (loss.item(), lo)
    ctx.close()

    # ---- sensitivity self-check (CPU, the same inputs) ----
    from tests import gpu_util as gu
    w0 = gu.flat_params(params)
    decay = drv.decay
    sub = np.arange(w0.size)
    if w0.size > 200_000:                        # elementwise: a sample of the kernels and every bias is enough
        r = np.random.default_rng(0)
        sub = np.unique(np.concatenate([r.choice(np.flatnonzero(decay), 100_000, replace=False), np.flatnonzero(~decay)]))
    kw = dict(warmup=warm)
    ref, frac = restated(w0[sub], [g[sub] for g in gs], fin, decay[sub], clip, **kw)
    for i, (a, d) in enumerate(zip(ref, devs)):                                     # the unplanted replay: within the bound
        assert (np.abs(a.astype(np.float64) - d[sub]) <= _bound(a, counts[i] + 1, clip)).all(), (name, i)
    full = [i for i, c in enumerate(counts) if lr_fn(c) == LR and fin[i]]
    assert full, name
    assert all(0.2 <= frac[i] <= 0.8 for i in full), (name, "clipped fraction on full-rate steps", [frac[i] for i in full])
    margins = {}
    for mname, mut in MUTANTS.items():
        mkw = dict(kw, **mut)
        mclip = mkw.pop("clip", clip)
        got, _ = restated(w0[sub], [g[sub] for g in gs], fin, decay[sub], mclip, **mkw)
        worst = 0.0
        for i, (a, d) in enumerate(zip(got, devs)):
            bnd = _bound(np.nan_to_num(a, nan=0.0, posinf=0.0, neginf=0.0), counts[i] + 1, clip)
            with np.errstate(invalid="ignore"):
                e = np.abs(a.astype(np.float64) - d[sub])
            e[np.isnan(a) != np.isnan(d[sub])] = np.inf
            worst = max(worst, float(np.nanmax(e / bnd)))
        margins[mname] = worst
    print(name, "mutant margins (x bound):", {k: f"{v:.3g}" for k, v in margins.items()}, "clipped:", [round(frac[i], 3) for i in full])
    missed = {k: v for k, v in margins.items() if not v >= 10}
    assert not missed, (name, "planted bugs the comparison would not catch", missed)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_eleventh_non_finite_gradient_is_applied_like_the_oracle(name, monkeypatch):
    """apply_if_finite(.., 10): ten non-finite gradients in a row leave the parameters alone and count to 10; the 11th is
    applied -- NaN where the oracle's update is NaN (optax.clip propagates it), the count advances."""
    case = CASES[name]
    clip = case[5]
    ctx, args, dist, model, params, drv = _make(case, monkeypatch, _opt(clip, warmup=0, learning_iter=40), seed=1)
    lr_fn = optim.learning_rate_fn(40, 0, LR)
    bads = [False, False] + [True] * 11
    st, gs, fin, devs, counts = _run_sequence(ctx, drv, model, params, clip, bads, lr_fn, name)
    for i in range(2, 12):
        np.testing.assert_array_equal(devs[i], devs[1])
    assert st.notfinite_count == 11 and st.count == 3 and st.step == 13
    nan = np.isnan(devs[-1])
    assert nan.any(), name
    if drv.mode == "synth":
        assert sorted(np.flatnonzero(nan)) == sorted(drv.bad_idx)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,via_c", [("headline-iter", ()), ("headline-iter-slabs", ()), ("headline-iter", (2, 7))])
def test_reset_optimizer_starts_a_fresh_oracle_state(name, via_c, monkeypatch):
    """mfm_reset_optimizer (create_train_state, exe_flow_matching.py:174): five updates, a reset, five more -- the second five
    equal a fresh oracle TrainState started from the device's parameters at the reset.  via_c: those calls update through
    mfm_adamw_step on a copy (C), which moves the count without refreshing D's cached bias corrections (wgrad_sk.hip: bc_for);
    the D call after it must recompute them."""
    case = CASES[name]
    clip = case[5]
    ctx, args, dist, model, params, drv = _make(case, monkeypatch, _opt(clip), seed=2)
    lr_fn = optim.learning_rate_fn(LITER, WARM, LR)
    from tests import gpu_util as gu
    _run_sequence(ctx, drv, model, params, clip, [False] * 5, lr_fn, name + " before", via_c=[i for i in via_c if i < 5])
    ctx.reset_optimizer()
    s = ctx.opt_state()
    assert (s["step"], s["count"], s["notfinite_count"]) == (0, 0, 0)
    p1 = gu.unflat_params(model, ctx.get_params())
    st, *_ = _run_sequence(ctx, drv, model, p1, clip, [False] * 5, lr_fn, name + " after", via_c=[i - 5 for i in via_c if i >= 5])
    assert st.count == 5
    ctx.close()
