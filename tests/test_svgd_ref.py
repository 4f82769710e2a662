"""CPU tests of the SVGD reference (tests/svgd_ref.py) and of the host side of ``mfm_amd.bblackjax.vi.svgd``: no GPU compute."""
import numpy as np
import pytest

from tests import svgd_ref as R


def test_functional_gradient_is_the_literal_double_loop_with_an_autograd_kernel_gradient():
    """svgd.py:74-84 written out: ``phi*(p, p_) = -k(p, p_) g(p) - d/dp k(p, p_)``, mean over p, for every p_."""
    import torch
    rng = np.random.default_rng(0)
    n, d, h = 5, 3, 1.7
    x, g = rng.standard_normal((n, d)), rng.standard_normal((n, d))
    fg = np.zeros((n, d))
    for i in range(n):                       # p_ = x_i
        for j in range(n):                   # p = x_j
            p = torch.tensor(x[j], dtype=torch.float64, requires_grad=True)
            k = torch.exp(-(1 / h) * ((p - torch.tensor(x[i], dtype=torch.float64)) ** 2).sum())      # :94-96
            (gk,) = torch.autograd.grad(k, p)
            fg[i] += (-(k.item() * g[j]) - gk.numpy()) / n
    np.testing.assert_allclose(R.functional_gradient(x, g, h), fg, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(R.functional_gradient(x, g, h, sqdist=R.sqdist(x)), fg, rtol=1e-13, atol=1e-15)


def test_length_scale_is_the_median_of_the_lower_triangle():
    x = np.array([[0.0], [1.0], [3.0], [7.0]])                  # distances 1 3 7 2 6 4 -> median 3.5
    assert R.length_scale(R.sqdist(x)) == pytest.approx(3.5 ** 2 / np.log(4), rel=1e-15)
    assert R.length_scale(R.sqdist(np.ones((6, 2)))) == 0.0


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_sgd_and_adam_match_torch_optim(kind):
    import torch
    rng = np.random.default_rng(1)
    p0 = rng.standard_normal((7, 3))
    grads = rng.standard_normal((5, 7, 3))
    opt = R.sgd(0.05) if kind == "sgd" else R.adam(0.05)
    tp = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    topt = torch.optim.SGD([tp], lr=0.05) if kind == "sgd" else torch.optim.Adam([tp], lr=0.05, betas=(0.9, 0.999), eps=1e-8)
    p, st = p0.copy(), opt.init(p0)
    for c, gr in enumerate(grads):
        upd, st = opt.update(gr, st, p, c)
        p = p + upd
        tp.grad = torch.tensor(gr, dtype=torch.float64)
        topt.step()
        np.testing.assert_allclose(p, tp.detach().numpy(), rtol=1e-12, atol=1e-14)


def test_adagrad_is_the_formula_written_out():
    rng = np.random.default_rng(2)
    p = rng.standard_normal((4, 2))
    opt = R.adagrad(0.1)
    st = opt.init(p)
    acc = np.full((4, 2), 0.1)
    for c in range(4):
        fg = rng.standard_normal((4, 2))
        fg[0, 0] = 0.0
        upd, st = opt.update(fg, st, p, c)
        acc = acc + fg ** 2
        want = np.empty_like(fg)
        for i in range(4):
            for j in range(2):
                want[i, j] = -0.1 * fg[i, j] / np.sqrt(acc[i, j] + 1e-7) if acc[i, j] > 0 else 0.0
        np.testing.assert_allclose(upd, want, rtol=1e-15)
        p = p + upd
    zero = R.adagrad(0.1, initial_accumulator_value=0.0)
    upd, _ = zero.update(np.zeros((2, 2)), zero.init(np.zeros((2, 2))), np.zeros((2, 2)), 0)
    assert (upd == 0).all()                                       # acc == 0: no change, not a division by sqrt(eps)


def test_cocob_first_update_is_minus_sign_over_alpha_and_the_next_three_match_the_transcription():
    rng = np.random.default_rng(3)
    alpha, eps = 100.0, 1e-8
    p = rng.standard_normal((6, 2))
    opt = R.cocob(alpha, eps)
    st = opt.init(p)
    fg = rng.standard_normal((6, 2))
    upd, st_new = opt.update(fg, st, p, 0)
    np.testing.assert_allclose(upd, -np.sign(fg) / alpha, rtol=1e-12)
    # cocob.py:55-81, element by element
    p0, C, L, G, Rw = (a.copy() for a in st)
    q = p.copy()
    st = opt.init(p)
    x = p.copy()
    for c in range(4):
        fg = rng.standard_normal((6, 2))
        upd, st = opt.update(fg, st, x, c)
        for i in range(6):
            for j in range(2):
                cc = fg[i, j]
                L[i, j] = max(L[i, j], abs(cc))
                G[i, j] = G[i, j] + abs(cc)
                Rw[i, j] = max(Rw[i, j] - cc * (q[i, j] - p0[i, j]), 0)
                C[i, j] = C[i, j] - cc
                u = -q[i, j] + (p0[i, j] + C[i, j] / (L[i, j] * max(G[i, j] + L[i, j], alpha * L[i, j])) * (L[i, j] + Rw[i, j]))
                assert upd[i, j] == pytest.approx(u, rel=1e-13, abs=1e-16)
        x = x + upd
        q = x.copy()


def test_reference_svgd_covers_the_four_modes():
    """256 particles from the 4-mode example's initial draw, sgd(0.5), 200 iterations, the float64 reference alone: the V-statistic
    KSD falls from 9.20 to 0.082, the second moments reach 64.07 / 64.01 (the target's: 65) and every quadrant holds 51 to 71 particles."""
    from oracle import metrics
    from tests import gpu_util as gu
    args, dist, k, model, state = gu.gmm4_setup(B=256)
    x = np.asarray(dist.init_params, dtype=np.float64)
    ksd0 = metrics.stein_disc(x, dist.grad_logprob)[1]
    opt = R.sgd(0.5)
    st, h = opt.init(x), 1.0
    for c in range(200):
        x, h, st, _ = R.step(x, dist.grad_logprob, h, opt, st, c)
    ksd1 = metrics.stein_disc(x, dist.grad_logprob)[1]
    print("KSD-V", ksd0, "->", ksd1, "second moments", (x ** 2).mean(0), "quadrants",
          [int(((x[:, 0] > 0) == a).__and__((x[:, 1] > 0) == b).sum()) for a in (True, False) for b in (True, False)])
    assert ksd1 <= ksd0 / 30
    assert (np.abs((x ** 2).mean(0) - 65.0) <= 3.0).all()
    for a in (True, False):
        for b in (True, False):
            assert (((x[:, 0] > 0) == a) & ((x[:, 1] > 0) == b)).sum() >= 40


def test_host_side_errors_are_raised_before_any_device_work():
    from mfm_amd.bblackjax import optimizers
    from mfm_amd.bblackjax.vi import svgd as S
    from mfm_amd.distributions import PhiFour
    d = PhiFour(16)                                              # no engine attached: any device work would raise RuntimeError instead
    with pytest.raises(NotImplementedError, match="rbf_kernel"):
        S.svgd(d.grad_logprob, optimizers.sgd(0.1), kernel=lambda x, y, length_scale=1: 0.0)
    with pytest.raises(TypeError, match="sgd.*adagrad.*adam.*cocob"):
        S.svgd(d.grad_logprob, (lambda p: None, lambda g, s, p: None))
    with pytest.raises(TypeError, match="sgd.*adagrad.*adam.*cocob"):
        S.build_kernel("adam")
    with pytest.raises(NotImplementedError, match="update_median_heuristic or None"):
        S.svgd(d.grad_logprob, optimizers.adam(0.1), update_kernel_parameters=lambda s: s)
    with pytest.raises(NotImplementedError, match="update_median_heuristic or None"):
        S.coin_svgd(d.grad_logprob, update_kernel_parameters=lambda s: s)
    with pytest.raises(NotImplementedError):
        S.svgd(lambda x: x * 2.0, optimizers.sgd(0.1))
    beta = 0.4
    for fn in (d.grad_logprob, d.logprob, lambda x: beta * d.loglik(x) + d.logprior(x)):
        algo = S.svgd(fn, optimizers.adagrad(0.1))               # accepted: nothing runs until init / step
        assert callable(algo.init) and callable(algo.step) and callable(algo.step.run)
    assert S._resolve(lambda x: beta * d.loglik(x) + d.logprior(x)) == (d, beta) and S._resolve(d.grad_logprob) == (d, 1.0)
    assert callable(S.coin_svgd(d.grad_logprob, alpha=50).step.run)
    o = optimizers.cocob.cocob(alpha=50)             # the submodule, as in the reference: optimizers/cocob.py
    assert (o.kind, o.hyper) == ("cocob", (50.0, 1e-8))
    assert optimizers.adagrad(0.1).hyper == (0.1, 0.1, 1e-7) and optimizers.adam(0.2).hyper == (0.2, 0.9, 0.999, 1e-8)


def test_flags_parse_and_the_header_declares_the_five_calls():
    import os
    from mfm_amd import _lib
    from mfm_amd.exe_others import svgd_optimizer
    from mfm_amd.multi_modal import build_parser
    a = build_parser().parse_args([])
    assert (a.do_svgd, a.svgd_optimizer, a.svgd_step_size) == (False, "adagrad", 0.1)
    a = build_parser().parse_args(["--do_svgd", "--svgd_optimizer", "cocob", "--svgd_step_size", "0.5"])
    assert (a.do_svgd, a.do_smc, a.svgd_optimizer, a.svgd_step_size) == (True, False, "cocob", 0.5)
    assert svgd_optimizer(a).kind == "cocob"
    a.svgd_optimizer = "sgd"
    assert svgd_optimizer(a) [:2] == ("sgd", (0.5,))
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--svgd_optimizer", "lbfgs"])
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mfm.h")).read()
    for name, nargs in (("mfm_svgd_sqdist", 5), ("mfm_svgd_median", 4), ("mfm_svgd_gradient", 10), ("mfm_svgd_apply", 13), ("mfm_svgd_step", 15)):
        assert name in _lib.EXPORTS and f"int {name}(" in header and len(_lib._SIGS[name][1]) == nargs
    assert _lib.SVGD_OPTIMIZERS == {"sgd": 0, "adagrad": 1, "adam": 2, "cocob": 3}
