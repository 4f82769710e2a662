"""GPU parity of Stein variational gradient descent (``mfm_svgd_*``, ``mfm_amd.bblackjax.vi.svgd``, ``--do_svgd``) against the float64
restatement in ``tests/svgd_ref.py``.  Every bound below is derived from the number formats or is one of the project's stated
tolerances; the measured values are printed before each assertion."""
import math

import numpy as np
import pytest

from tests import svgd_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(18, 2), (37, 2), (100, 25), (100, 64), (257, 64), (130, 256), (48, 1024)]      # 37 / 257: ragged last tile in both directions
CLOUDS = [(0.0, 1.0), (8.0, 1.0), (1000.0, 1.0), (30.0, 0.1)]                            # (offset, spread): the offset cases need centring
U = 2.0 ** -23


@pytest.fixture(scope="module")
def ctx():
    from tests import gpu_util as gu
    args, dist, k, model, state = gu.gmm4_setup(B=16, hidden=16, F=16)
    c = gu.make_ctx(dist, args)
    yield c
    c.close()


def _cloud(n, d, off, scale, seed=0):
    return (off + scale * np.random.default_rng(seed).standard_normal((n, d))).astype(np.float32)


def _dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _qc(x32):
    """Centred squared norms in float64."""
    x = x32.astype(np.float64)
    xc = x - x.mean(0)
    return (xc * xc).sum(1)


def _sqdist_dev(ctx, x32):
    import torch
    n = x32.shape[0]
    D = torch.full((n, n), float("nan"), device="cuda", dtype=torch.float32)
    ctx.svgd_sqdist(_dev(x32), D)
    return D


def _sqdist_bound(x32):
    q = _qc(x32)
    return (x32.shape[1] + 8) * U * (q[:, None] + q[None, :])


# ---- 1. sqdist ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off,scale", CLOUDS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_sqdist_is_within_the_float32_dot_product_bound_of_the_direct_form(ctx, n, d, off, scale):
    """|D_ij - exact| <= (d + 8) 2^-23 (q_i + q_j), q the centred squared norms: the worst case of a float32 dot product of length d
    (any summation order) plus the epilogue's roundings.  Measured on MI355X: the largest |dD| / bound over the 28 cases is 0.24
    (0.20 / 0.22 / 0.24 / 0.19 for the four clouds; an uncentred Gram form fails the offset cases by orders of magnitude)."""
    x = _cloud(n, d, off, scale, seed=n + d)
    D = _sqdist_dev(ctx, x).cpu().numpy()
    ref = R.sqdist(x)
    bound = _sqdist_bound(x)
    ratio = np.abs(D - ref) / np.where(bound > 0, bound, 1.0)
    print(f"sqdist n={n} d={d} off={off} scale={scale}: max |dD| / bound = {ratio.max():.3g}")
    assert np.isfinite(D).all()
    assert (np.diag(D) == 0).all() and (D >= 0).all()
    assert (np.abs(D - ref) <= bound).all()
    assert (D == D.T).all()


# ---- 2. median ----------------------------------------------------------------------------------------------------------------------
def _median_of_device_D(D):
    n = D.shape[0]
    v = np.sort(D[np.tril_indices(n, -1)]).astype(np.float64)          # the float32 squared values
    m = v.size
    a, b = v[(m - 1) // 2], v[m // 2]
    return (0.5 * (math.sqrt(a) + math.sqrt(b))) ** 2 / math.log(n)


def _median_dev(ctx, D):
    import torch
    ls = torch.full((1,), float("nan"), device="cuda", dtype=torch.float64)
    ctx.svgd_median(D, ls)
    return ls.item()


def _decades(n, d, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, d)) * 10.0 ** rng.uniform(-3, 3, size=(n, 1))).astype(np.float32)


def _with_duplicates(n, d, seed):
    x = _cloud(n, d, 0.0, 1.0, seed)
    x[n - 8:] = x[:8]                                                   # 8 duplicated particles: ties at 0 and at every distance to them
    return x


@pytest.mark.parametrize("name,x", [("n16-even", _cloud(16, 3, 0.0, 1.0, 1)), ("n18-odd", _cloud(18, 2, 8.0, 1.0, 2)),
                                    ("n1500-decades", _decades(1500, 3, 3)), ("duplicates", _with_duplicates(40, 5, 4)),
                                    ("n257", _cloud(257, 64, 0.0, 1.0, 5))])
def test_median_is_the_exact_order_statistic_of_the_device_matrix(ctx, name, x):
    """Against numpy on the device's own D: exact selection, so only the float64 square roots, mean, square and log differ (1e-14);
    against the float64 reference on the same particles: an order statistic moves by at most the largest perturbation of its set and
    the squared mean of two square roots by at most twice that, so |dh| <= 4 (d + 8) 2^-23 max_ij (q_i + q_j) / log n."""
    n, d = x.shape
    D = _sqdist_dev(ctx, x)
    h = _median_dev(ctx, D)
    want = _median_of_device_D(D.cpu().numpy())
    h_ref = R.length_scale(R.sqdist(x))
    q = _qc(x)
    bound = 4 * (d + 8) * U * (q[:, None] + q[None, :]).max() / math.log(n)
    print(f"median {name}: device {h!r} numpy-on-device-D {want!r} float64 reference {h_ref!r} |dh| / bound = {abs(h - h_ref) / bound:.3g}")
    assert h == pytest.approx(want, rel=1e-14)
    assert abs(h - h_ref) <= bound


def test_median_of_identical_particles_is_exactly_zero(ctx):
    x = np.tile(np.float32([[3.25, -1.5, 1000.125]]), (33, 1))
    D = _sqdist_dev(ctx, x)
    assert (D.cpu().numpy() == 0).all()
    assert _median_dev(ctx, D) == 0.0


# ---- 3. gradient ----------------------------------------------------------------------------------------------------------------------
def _gradient_dev(ctx, x, g, D, h, i0=0, n_rows=None):
    import torch
    n, d = x.shape
    fg = torch.full((n if n_rows is None else n_rows, d), float("nan"), device="cuda", dtype=torch.float32)
    ctx.svgd_gradient(_dev(x), _dev(g), D, _dev(np.array([h], dtype=np.float64)), fg, i0=i0, n_rows=n_rows)
    return fg.cpu().numpy()


def _gradient_tol(x, g, h, D):
    kg, sx, kx = R.gradient_terms(x, g, h, D)
    return 2e-5 * (kg + (2.0 / h) * (sx + kx)) / x.shape[0]


@pytest.mark.parametrize("which", ["one", "median", "100-median"])
@pytest.mark.parametrize("n,d", SHAPES)
def test_gradient_matches_the_reference_on_the_device_distances(ctx, n, d, which):
    """Only the GEMM exp(-D/h) [G | Xc] and its epilogue are under test: the reference gets the device's own D.  Tolerance: 2e-5 (the
    project's f32-MFMA-chain tolerance against the float64 oracle, docs/HISTORY.md section 2) of the terms' scale
    (max|K G| + (2/h) (max|s xc| + max|K Xc|)) / n.  At h = 1 and d >= 64 the weights underflow to the identity; at 100 medians every
    weight is near 1 and s xc - K Xc cancels.  Measured on MI355X: max |dfg| / tolerance over the 21 cases: 0.0034 at h = 1, 0.030 at the median, 0.048 at 100 medians."""
    x = _cloud(n, d, 8.0, 1.0, seed=3 * n + d)
    g = np.random.default_rng(n * d).standard_normal((n, d)).astype(np.float32)
    D = _sqdist_dev(ctx, x)
    Dh = D.cpu().numpy()
    med = R.length_scale(Dh)
    h = {"one": 1.0, "median": med, "100-median": 100.0 * med}[which]
    fg = _gradient_dev(ctx, x, g, D, h)
    ref = R.functional_gradient(x, g, h, sqdist=Dh)
    tol = _gradient_tol(x, g, h, Dh)
    err = np.abs(fg - ref).max()
    print(f"gradient n={n} d={d} h={which} ({h:.4g}): max |dfg| = {err:.3g}, tolerance {tol:.3g}, ratio {err / tol:.3g}, max |fg| = {np.abs(ref).max():.3g}")
    assert np.isfinite(fg).all()
    assert err <= tol


def test_gradient_of_a_row_range_has_the_bits_of_those_rows_of_the_full_call(ctx):
    n, d = 100, 25
    x = _cloud(n, d, 8.0, 1.0, seed=7)
    g = np.random.default_rng(8).standard_normal((n, d)).astype(np.float32)
    D = _sqdist_dev(ctx, x)
    h = R.length_scale(D.cpu().numpy())
    full = _gradient_dev(ctx, x, g, D, h)
    part = _gradient_dev(ctx, x, g, D, h, i0=16, n_rows=32)
    assert part.shape == (32, d) and np.isfinite(part).all()
    np.testing.assert_array_equal(part.view(np.uint32), full[16:48].view(np.uint32))


# ---- 4. apply --------------------------------------------------------------------------------------------------------------------------
def _opt_pair(kind):
    from mfm_amd.bblackjax import optimizers as O
    return {"sgd": (O.sgd(0.05), R.sgd(0.05)), "adagrad": (O.adagrad(0.1), R.adagrad(0.1)), "adam": (O.adam(0.01), R.adam(0.01)),
            "cocob": (O.cocob.cocob(), R.cocob())}[kind]


@pytest.mark.parametrize("kind", ["sgd", "adagrad", "adam", "cocob"])
def test_apply_matches_the_reference_restarted_from_the_device_state(ctx, kind):
    """Five updates on [37, 25]; before each the float64 reference takes the device's float32 particles and state.  Relative 3e-6, the
    project's AdamW tolerance (the device evaluates in float64 and rounds each stored value once: measured <= 6e-8)."""
    rng = np.random.default_rng(11)
    opt, ref = _opt_pair(kind)
    x = _dev(rng.standard_normal((37, 25)).astype(np.float32))
    *state, count = opt.init(x)
    worst = 0.0
    for it in range(5):
        fg32 = rng.standard_normal((37, 25)).astype(np.float32)
        if it == 2:
            fg32[0, :5] = 0.0
        p = x.cpu().numpy().astype(np.float64)
        st = tuple(s.cpu().numpy().astype(np.float64) for s in state)
        upd, st_new = ref.update(fg32.astype(np.float64), st, p, count)
        ctx.svgd_apply(opt.kind, opt.hyper, count, x, _dev(fg32), state)
        count += 1
        got = x.cpu().numpy()
        np.testing.assert_allclose(got, p + upd, rtol=3e-6, atol=0)
        worst = max(worst, np.abs(got / (p + upd) - 1).max())
        for s, w in zip(state, st_new):
            np.testing.assert_allclose(s.cpu().numpy(), w, rtol=3e-6, atol=0)
        if kind == "cocob" and it == 0:
            np.testing.assert_allclose(got, p - np.sign(fg32) / 100.0, rtol=3e-6, atol=0)        # the first bet: -sign(fg) / alpha
    print(f"apply {kind}: max relative difference {worst:.3g}")


# ---- 5. composite ----------------------------------------------------------------------------------------------------------------------
def _composite_setup(target):
    from tests import gpu_util as gu
    if target == "phi4":
        args, dist, k, model, state = gu.phi4_setup(d=64, B=48, hidden=32, F=16)
        return dist, gu.make_ctx(dist, args, n_local=48, n_valid=40), 40, 0.7
    if target == "gmm4":
        args, dist, k, model, state = gu.gmm4_setup(B=64)
        return dist, gu.make_ctx(dist, args), 64, 1.0
    args, dist, k, model, state = gu.lgcp_setup(n=10, B=32)
    return dist, gu.make_ctx(dist, args), 32, 1.0


def _step_dev(c, beta, opt, count, n_iter, x, state, ls, update_median=True, ls_used=None):
    c.svgd_step(beta, opt.kind, opt.hyper, count, n_iter, x, state, ls, update_median=update_median, ls_used=ls_used)


@pytest.mark.parametrize("target", ["phi4", "gmm4", "lgcp"])
def test_step_matches_the_reference_iteration_by_iteration(target):
    """3 iterations with adagrad(0.1), then 3 with cocob(); before each the reference restarts from the device's particles, optimizer
    state and length scale, with oracle.targets.Tempered's gradient and the device's own D of those particles (mfm_svgd_sqdist: the
    composite's sqdist is the same launch).  New length scale: the bound of the median test, on the device's new particles.  New particles:
    the gradient test's tolerance pushed through the reference's own optimizer update (the larger of the update's change under fg +- that
    tolerance: tolerance x |d update / d fg| to first order) plus 3e-6 relative.  Padding rows keep their bits.  Measured on MI355X over
    the 18 iterations: particle error / allowance <= 0.019, |dh| / bound <= 0.003."""
    import torch
    from oracle import targets
    dist, c, n, beta = _composite_setup(target)
    try:
        x0 = np.ascontiguousarray(dist.init_params, dtype=np.float32)
        B, d = x0.shape
        x = _dev(x0)
        vg = targets.Tempered(dist, beta).value_and_grad
        ls = _dev(np.array([1.0]))
        for kind in ("adagrad", "cocob"):
            opt, ref = _opt_pair(kind)
            *state, count = opt.init(x)
            for it in range(3):
                p32 = x.cpu().numpy()
                p = p32[:n].astype(np.float64)
                h = ls.item()
                st = tuple(s.cpu().numpy()[:n].astype(np.float64) for s in state)
                Dd = torch.empty((n, n), device="cuda", dtype=torch.float32)
                c.svgd_sqdist(x[:n].contiguous(), Dd)
                Dh = Dd.cpu().numpy()
                g = np.asarray(vg(p)[1], dtype=np.float64)
                fg = R.functional_gradient(p, g, h, sqdist=Dh)
                upd, _ = ref.update(fg, st, p, count)
                tol = _gradient_tol(p, g, h, Dh)
                prop = np.maximum(np.abs(ref.update(fg + tol, st, p, count)[0] - upd), np.abs(ref.update(fg - tol, st, p, count)[0] - upd))
                used = torch.empty(1, device="cuda", dtype=torch.float64)
                _step_dev(c, beta, opt, count, 1, x, state, ls, ls_used=used)
                count += 1
                got = x.cpu().numpy()
                assert used.item() == h
                np.testing.assert_array_equal(got[n:].view(np.uint32), p32[n:].view(np.uint32))
                want = p + upd
                err = np.abs(got[:n] - want)
                allow = prop + 3e-6 * np.abs(want)
                q = _qc(got[:n])
                h_new, h_ref = ls.item(), R.length_scale(R.sqdist(got[:n]))
                h_bound = 4 * (d + 8) * U * (q[:, None] + q[None, :]).max() / math.log(n)
                print(f"step {target} {kind} it={it}: h {h:.6g} -> {h_new:.6g} (|dh| / bound {abs(h_new - h_ref) / h_bound:.3g}), "
                      f"max particle error / allowance {np.max(err / allow):.3g}, max |update| {np.abs(upd).max():.3g}")
                assert np.isfinite(got).all()
                assert (err <= allow).all()
                assert abs(h_new - h_ref) <= h_bound
    finally:
        c.close()


def test_step_of_four_iterations_has_the_bits_of_four_single_steps_and_a_fixed_length_scale_stays():
    import torch
    dist, c, n, beta = _composite_setup("phi4")
    try:
        x0 = np.ascontiguousarray(dist.init_params, dtype=np.float32)
        opt, _ = _opt_pair("adam")
        runs = []
        for split in (False, True):
            x = _dev(x0)
            *state, count = opt.init(x)
            ls = _dev(np.array([1.0]))
            used = torch.empty(4, device="cuda", dtype=torch.float64)
            if split:
                for it in range(4):
                    _step_dev(c, beta, opt, count + it, 1, x, state, ls, ls_used=used[it:it + 1])
            else:
                _step_dev(c, beta, opt, count, 4, x, state, ls, ls_used=used)
            runs.append([x.cpu().numpy()] + [s.cpu().numpy() for s in state] + [ls.cpu().numpy(), used.cpu().numpy()])
        for a, b in zip(*runs):
            np.testing.assert_array_equal(a.view(np.uint32 if a.dtype == np.float32 else np.uint64), b.view(np.uint32 if b.dtype == np.float32 else np.uint64))
        assert runs[0][-1][0] == 1.0 and len(set(runs[0][-1])) == 4 and not np.array_equal(runs[0][0], x0)
        x = _dev(x0)
        *state, count = opt.init(x)
        ls = _dev(np.array([0.731]))
        used = torch.empty(3, device="cuda", dtype=torch.float64)
        _step_dev(c, beta, opt, count, 3, x, state, ls, update_median=False, ls_used=used)
        assert ls.item() == 0.731 and (used.cpu().numpy() == 0.731).all() and not np.array_equal(x.cpu().numpy(), x0)
    finally:
        c.close()


# ---- 6. Python API ----------------------------------------------------------------------------------------------------------------------
def _engine(kind, B):
    import torch
    from mfm_amd import distributions as D
    from mfm_amd.engine import Engine
    from tests import gpu_util as gu
    if kind == "phi4":
        args, odist, k, model, state = gu.phi4_setup(d=64, B=B, hidden=32, F=16)
        dist = D.PhiFour(64)
    else:
        args, odist, k, model, state = gu.gmm4_setup(B=B)
        dist = D.GaussianMixture(odist.modes, odist.covs, odist.weights)
    args.ot_cond_flow = False
    eng = Engine(dist, args, model.f)
    return eng, dist, odist, torch.as_tensor(odist.init_params.astype(np.float32)).cuda()


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("kind", ["phi4", "gmm4"])
def test_python_api_states_are_values_and_run_has_the_bits_of_the_steps(kind):
    import torch
    from mfm_amd.bblackjax import optimizers as O
    from mfm_amd.bblackjax.vi import svgd as S
    eng, dist, odist, pos = _engine(kind, 64)
    try:
        beta = 0.6
        for algo in (S.svgd(dist.grad_logprob, O.adagrad(0.1)), S.coin_svgd(dist.grad_logprob),
                     S.svgd(lambda x: beta * dist.loglik(x) + dist.logprior(x), O.adam(0.05)),
                     S.svgd(dist.logprob, O.sgd(0.1), update_kernel_parameters=None)):
            state = algo.init(pos)
            assert state.kernel_parameters == {"length_scale": 1.0} and state.opt_state[-1] == 0
            before = [state.particles.clone()] + [s.clone() for s in state.opt_state[:-1]]
            s1 = algo.step(state)
            for a, b in zip([state.particles] + list(state.opt_state[:-1]), before):          # states are values
                assert torch.equal(a, b)
            assert state.kernel_parameters == {"length_scale": 1.0} and state.opt_state[-1] == 0
            ls1 = s1.kernel_parameters["length_scale"]
            assert ls1.dtype == torch.float64 and ls1.numel() == 1 and ls1.is_cuda and s1.opt_state[-1] == 1
            assert not torch.equal(s1.particles, pos) and torch.isfinite(s1.particles).all()
            st = state
            scales = []
            for _ in range(5):
                scales.append(float(torch.as_tensor(st.kernel_parameters["length_scale"]).item()))
                st = algo.step(st)
            ran, used = algo.step.run(state, 5, keep_length_scales=True)
            plain = algo.step.run(state, 5)
            for a, b, c in zip([st.particles, st.kernel_parameters["length_scale"]] + list(st.opt_state[:-1]),
                               [ran.particles, ran.kernel_parameters["length_scale"]] + list(ran.opt_state[:-1]),
                               [plain.particles, plain.kernel_parameters["length_scale"]] + list(plain.opt_state[:-1])):
                np.testing.assert_array_equal(_bits(a), _bits(b))
                np.testing.assert_array_equal(_bits(a), _bits(c))
            assert ran.opt_state[-1] == 5 and used.cpu().numpy().tolist() == scales
        fixed = S.svgd(dist.logprob, O.sgd(0.1), update_kernel_parameters=None)
        assert fixed.step(fixed.init(pos, {"length_scale": 2.5})).kernel_parameters["length_scale"].item() == 2.5
        # the stand-alone pieces on device tensors
        st = S.update_median_heuristic(S.SVGDState(pos, {"length_scale": 1.0}, ()))
        assert st.kernel_parameters["length_scale"].item() == pytest.approx(R.length_scale(R.sqdist(pos.cpu().numpy())), rel=1e-4)
        k = S.rbf_kernel(pos[0], pos[1], length_scale=2.0).item()
        assert k == pytest.approx(math.exp(-0.5 * float(((pos[0] - pos[1]) ** 2).sum())), rel=1e-5)
    finally:
        eng.close()


def test_library_errors_name_their_argument_and_touch_nothing():
    import torch
    from mfm_amd import _lib
    from tests import gpu_util as gu
    args, dist, k, model, state = gu.gmm4_setup(B=16, hidden=16, F=16)
    hyper, ls = (0.1,), _dev(np.array([1.0]))

    def refused(c, rows, match, n_iter=1, kind="sgd"):
        x = _dev(np.random.default_rng(0).standard_normal((rows, 2)).astype(np.float32))
        keep = x.clone()
        with pytest.raises(_lib.MfmError, match=match):
            c.svgd_step(1.0, kind, hyper, 0, n_iter, x, [], ls)
        torch.cuda.synchronize()
        assert torch.equal(x, keep) and ls.item() == 1.0

    c = gu.make_ctx(dist, args, n_local=16, n_valid=1)
    refused(c, 16, r"error -1: n must be at least 2 \(got 1\)")
    c.close()
    c = gu.make_ctx(dist, args, n_local=16)
    refused(c, 16, r"error -1: n_iter must be at least 1 \(got 0\)", n_iter=0)
    refused(c, 16, r"error -1: d_s0 is null", kind="adagrad")
    with pytest.raises(_lib.MfmError, match="unknown optimizer kind"):
        c.svgd_step(1.0, "lbfgs", hyper, 0, 1, ls, [], ls)
    with pytest.raises(_lib.MfmError, match=r"error -1: row range"):
        c.svgd_gradient(_dev(np.zeros((16, 2), np.float32)), _dev(np.zeros((16, 2), np.float32)), _dev(np.zeros((16, 16), np.float32)), ls,
                        _dev(np.zeros((16, 2), np.float32)), i0=8, n_rows=9)
    c.close()
    c = gu.make_ctx(dist, args, n_local=16, n_total=32)
    refused(c, 16, r"error -2: n_chain_total = 32 differs from n_chain_local = 16")
    c.close()
    c = gu.make_ctx(dist, args, n_local=16400)                          # refused before any allocation (D alone would pass 1 GiB)
    refused(c, 16400, r"error -3: n = 16400 particles exceed 16384")
    c.close()


def test_python_api_refuses_wrong_shapes_and_a_closed_engine():
    """``run`` hands raw pointers to the library, so particles and state arrays that are not float32 ``[n_chain_local, dim]`` raise before
    the call; the stand-alone ``update_median_heuristic`` never launches through a closed engine or on another device's tensor."""
    import torch
    from mfm_amd.bblackjax import optimizers as O
    from mfm_amd.bblackjax.vi import svgd as S
    eng, dist, odist, pos = _engine("gmm4", 64)
    try:
        algo = S.svgd(dist.grad_logprob, O.adagrad(0.1))
        good = algo.init(pos)
        for bad in (algo.init(pos[:48].contiguous()), algo.init(pos.double()),
                    S.SVGDState(pos, good.kernel_parameters, (good.opt_state[0][:32].contiguous(), 0))):
            with pytest.raises(ValueError, match=r"n_chain_local, dim\] = \[64, 2\]"):
                algo.step(bad)
        assert torch.isfinite(algo.step(good).particles).all()
        with pytest.raises(RuntimeError, match="device tensor"):
            S.update_median_heuristic(S.SVGDState(pos.cpu(), {"length_scale": 1.0}, ()))
        assert S.update_median_heuristic(S.SVGDState(pos[:20].contiguous(), {"length_scale": 1.0}, ())).kernel_parameters["length_scale"].item() > 0
    finally:
        eng.close()
    with pytest.raises(RuntimeError, match="has been closed"):
        S.update_median_heuristic(S.SVGDState(pos, {"length_scale": 1.0}, ()))


# ---- 7. behaviour -------------------------------------------------------------------------------------------------------------------------
def test_svgd_covers_the_four_modes():
    """256 particles from the 4-mode example's initial draw, sgd(0.5), 200 iterations in one run.  The float64 reference alone
    (tests/test_svgd_ref.py) takes the V-statistic KSD from 9.20 to 0.082, the second moments to 64.07 / 64.01 and leaves 51 to 71
    particles per quadrant."""
    import torch
    from mfm_amd.bblackjax import optimizers as O
    from mfm_amd.bblackjax.vi import svgd as S
    from mfm_amd.exe_flow_matching import stein_disc
    eng, dist, odist, pos = _engine("gmm4", 256)
    try:
        v0 = stein_disc(eng, pos)[1]
        algo = S.svgd(dist.grad_logprob, O.sgd(0.5))
        out = algo.step.run(algo.init(pos), 200)
        x = out.particles
        v1 = stein_disc(eng, x)[1]
        m2 = (x.double() ** 2).mean(0).cpu().numpy()
        quad = [int((((x[:, 0] > 0) == a) & ((x[:, 1] > 0) == b)).sum()) for a in (True, False) for b in (True, False)]
        print(f"behaviour: KSD-V {v0:.4g} -> {v1:.4g}, second moments {m2}, quadrants {quad}, length scale {out.kernel_parameters['length_scale'].item():.4g}")
        assert torch.isfinite(x).all()
        assert v1 <= v0 / 30
        assert (np.abs(m2 - 65.0) <= 3.0).all()
        assert min(quad) >= 40
    finally:
        eng.close()


# ---- 8. --do_svgd -------------------------------------------------------------------------------------------------------------------------
def test_do_svgd_end_to_end_on_the_four_mode_example():
    """64 chains, 20 iterations, --svgd_optimizer sgd --svgd_step_size 0.5 (the behaviour test's optimizer).  The float64 reference on the
    same initial particles takes the KSD (U, V) from (8.758, 10.07) to (0.234, 0.459).  Under the default adagrad(0.1) twenty iterations
    only carry the particles off the saddle at the origin, where the score is small, and the reference's KSD RISES to (14.816, 15.94) --
    the device gives 14.81586 there too -- so the default is not what this test runs."""
    from mfm_amd import exe_others as X, multi_modal as M
    from mfm_amd.distributions import GaussianMixture
    from mfm_amd.exe_flow_matching import stein_disc

    def setup(flags):
        args = M.build_parser().parse_args(["--example", "4-mode", "--num_chain", "64", "--learning_iter", "20", "--seed", "1", "--log_every", "5"] + flags)
        args.dim, args.lim, args.levels, args.step_size = 2, [-16, 16], 20, 0.2                  # multi_modal.main: the 4-mode example
        return args, GaussianMixture(8. * np.array([[1, 1], [1, -1], [-1, 1], [-1, -1]]), np.ones((4, 2)), np.ones(4) / 4)

    args, dist = setup(["--do_svgd", "--svgd_optimizer", "sgd", "--svgd_step_size", "0.5"])
    res, res_, extras = X.run(dist, args, dist.sample_model, return_extras=True)
    eng = extras["engine"]
    try:
        ksd0 = stein_disc(eng, eng.local(dist.init_params))
        print("do_svgd: res", res, "initial KSD (U, V)", ksd0, "length scales", extras["length_scales"])
        assert res.shape == (5,) and np.isfinite(res).all() and np.array_equal(res, res_)
        assert res[1] < ksd0[0] and res[2] < ksd0[1]
        assert extras["length_scales"].shape == (20,) and extras["length_scales"][0] == 1.0 and np.isfinite(extras["length_scales"]).all()
        assert extras["samples"].shape == (64, 2)
    finally:
        eng.close()
    args, dist = setup([])
    with pytest.raises(NotImplementedError, match="only --do_smc"):
        X.run(dist, args, None)
