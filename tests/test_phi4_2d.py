"""Phi-four on an L x L lattice (dim_phys = 2): the restated oracle (tests/phi4_2d_oracle.py) against autograd on the scalar
log-density, its bond counts, how far it sits from the chain of the same d and boundary, and the PhiFour constructor, its target
block and the CLI flag.  CPU only."""
import numpy as np
import pytest

from tests.phi4_2d_oracle import PhiFour2D
from tests.phi4_bc_oracle import PhiFourBC

BCS = [("pbc", 0.0), ("dirichlet", 0.0), ("dirichlet", 0.7), ("dirichlet", -1.2)]
SIDES = [3, 6, 16]


def _states(d, n=4, seed=0):
    return np.random.default_rng(seed + d).uniform(-1.5, 1.5, (n, d))


def _torch_logdensity(xt, L, a, beta, bc):
    """-beta (U + V) written with torch on the [B, L, L] field: np.roll by 1 along each axis under pbc, a frame of b otherwise."""
    import torch
    coef = a * L
    f = xt.reshape(xt.shape[0], L, L)
    if bc[0] == "pbc":
        dr, dc = f - torch.roll(f, 1, 1), f - torch.roll(f, 1, 2)
    else:
        p = torch.nn.functional.pad(f, (1, 1, 1, 1), value=float(bc[1]))
        dr = p[:, 1:, 1:-1] - p[:, :-1, 1:-1]
        dc = p[:, 1:-1, 1:] - p[:, 1:-1, :-1]
    U = ((dr ** 2).sum((1, 2)) + (dc ** 2).sum((1, 2))) / 2.0 * coef
    V = ((1.0 - xt ** 2) ** 2).sum(1) / 4.0 / coef
    return -beta * (U + V)


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("L", SIDES)
def test_gradient_and_hvp_match_autograd(L, bc):
    import torch
    d = L * L
    dist = PhiFour2D(d, 0.1, 20.0, bc)
    assert dist.coef == 0.1 * L
    x = _states(d)
    v = np.random.default_rng(7).normal(size=x.shape)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    val = _torch_logdensity(xt, L, 0.1, 20.0, bc)
    g, = torch.autograd.grad(val.sum(), xt, create_graph=True)
    hv, = torch.autograd.grad((g * torch.tensor(v)).sum(), xt)
    np.testing.assert_allclose(dist.loglik(x), val.detach().numpy(), rtol=1e-13, atol=1e-9)
    np.testing.assert_allclose(dist.logprob(x), dist.loglik(x), rtol=0, atol=0)
    np.testing.assert_allclose(dist.grad_logprob(x), g.detach().numpy(), rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(dist.hvp_logprob(x, v), hv.numpy(), rtol=1e-12, atol=1e-9)
    # the exact-trace Hessian diagonal: hvp on the unit vectors
    hd = np.stack([dist.hvp_logprob(x, np.broadcast_to(np.eye(d)[j][None], x.shape))[:, j] for j in range(d)], 1)
    np.testing.assert_allclose(dist.hess_diag(x), hd, rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("L", SIDES)
def test_bond_counts(L):
    d = L * L
    # a constant field at b has no gradient energy under Dirichlet b; any constant field has none under pbc
    for b in (0.0, 0.7, -1.2):
        assert PhiFour2D(d, bc=("dirichlet", b)).bonds(np.full((1, d), b))[0] == 0.0
        assert PhiFour2D(d, bc=("pbc", 0.0)).bonds(np.full((1, d), b))[0] == 0.0
    # every bond of a constant field at b + 1 inside a frame at b has length 1 where it touches the frame: 4 L frame bonds
    assert PhiFour2D(d, bc=("dirichlet", 0.7)).bonds(np.full((1, d), 1.7))[0] == pytest.approx(4 * L, rel=1e-12)
    # bonds in all: a checkerboard has (dx)^2 = 4 on every interior bond (even L: on the wrapped ones too)
    cb = (1.0 - 2.0 * (np.add.outer(np.arange(L), np.arange(L)) % 2)).reshape(1, d)
    if L % 2 == 0:
        assert PhiFour2D(d, bc=("pbc", 0.0)).bonds(cb)[0] == 4.0 * 2 * L * L
    assert PhiFour2D(d, bc=("dirichlet", 0.0)).bonds(cb)[0] == 4.0 * 2 * L * (L - 1) + 4 * L       # + 4 L frame bonds of (1)^2


@pytest.mark.parametrize("bc", [("pbc", 0.0), ("dirichlet", 0.0), ("dirichlet", 0.7)])
@pytest.mark.parametrize("L", [6, 8, 16])
def test_lattice_differs_from_the_chain_of_the_same_d(L, bc):
    """What the GPU tests' sensitivity assertions rely on: on their inputs (uniform in [-1, 1]) value and gradient of the lattice sit
    far from the chain's of the same d and boundary -- the coefficient alone is a L against a L^2."""
    d = L * L
    two, one = PhiFour2D(d, 0.1, 20.0, bc), PhiFourBC(d, 0.1, 20.0, bc)
    x = np.random.default_rng(1).uniform(-1, 1, (8, d))
    v = np.random.default_rng(2).normal(size=x.shape)
    assert (np.abs(two.loglik(x) - one.loglik(x)) / (1e-3 + 2e-6 * np.abs(one.loglik(x)))).min() >= 100
    g1 = one.grad_logprob(x)
    assert (np.abs(two.grad_logprob(x) - g1) / (2e-3 + 2e-5 * np.abs(g1))).max() >= 100
    h1 = one.hvp_logprob(x, v)
    assert np.abs(two.hvp_logprob(x, v) - h1).max() / np.abs(h1).max() >= 100 * 2e-5


# ---- the package's PhiFour, its target block and the CLI ---------------------------------------------------------------------
def test_one_dimensional_blocks_are_unchanged():
    from mfm_amd.distributions import PhiFour
    for kw in ({}, {"dim_phys": 1}):
        assert PhiFour(64, **kw).target_block() == (0, [0.1, 20.0])
        assert PhiFour(64, bc=("dirichlet", 0.0), **kw).target_block() == (0, [0.1, 20.0])
        assert PhiFour(40, a=0.2, beta=10.0, bc=("dirichlet", 1), **kw).target_block() == (0, [0.2, 10.0, 0.0, 1.0])
        assert PhiFour(40, bc=("pbc", 3.0), **kw).target_block() == (0, [0.1, 20.0, 1.0, 0.0])
    assert PhiFour(40).dim_phys == 1 and PhiFour(40).dim_grid == 40


def test_two_dimensional_constructor_and_block():
    from mfm_amd.distributions import PhiFour
    p = PhiFour(64, dim_phys=2)
    assert p.dim == 64 and p.dim_phys == 2 and p.dim_grid == 8
    assert p.target_block() == (0, [0.1, 20.0, 0.0, 0.0, 2.0])
    assert PhiFour(256, a=0.2, beta=10.0, bc=("dirichlet", 0.7), dim_phys=2).target_block() == (0, [0.2, 10.0, 0.0, 0.7, 2.0])
    assert PhiFour(36, bc=("pbc", 3.0), dim_phys=2).target_block() == (0, [0.1, 20.0, 1.0, 0.0, 2.0])
    for dim in (40, 63, 2, 128):
        with pytest.raises(ValueError):
            PhiFour(dim, dim_phys=2)
    for dp in (0, 3, 2.5, None):
        with pytest.raises(ValueError):
            PhiFour(64, dim_phys=dp)
    with pytest.raises(NotImplementedError):
        PhiFour(64, tilt=0.1, dim_phys=2)
    # the oracle class states the same block
    assert PhiFour2D(64, bc=("dirichlet", 0.7)).block() == PhiFour(64, bc=("dirichlet", 0.7), dim_phys=2).target_block()[1]
    assert PhiFour2D(64, bc=("pbc", 0.0)).block() == PhiFour(64, bc=("pbc", 0), dim_phys=2).target_block()[1]
    # initialize_model does not depend on dim_phys
    from mfm_amd import random as jr
    a, b = PhiFour(16), PhiFour(16, dim_phys=2)
    a.initialize_model(jr.PRNGKey(3), 4); b.initialize_model(jr.PRNGKey(3), 4)
    np.testing.assert_array_equal(a.init_params, b.init_params)


def test_cli_flag(monkeypatch):
    from mfm_amd import multi_modal as M
    a = M.build_parser().parse_args([])
    assert a.phi4_dim_phys == 1
    a = M.build_parser().parse_args(["--phi4_dim_phys", "2", "--phi4_bc", "pbc", "--hutch"])
    assert a.phi4_dim_phys == 2 and a.phi4_bc == "pbc" and a.hutchs
    with pytest.raises(SystemExit):
        M.build_parser().parse_args(["--phi4_dim_phys", "3"])
    flags = [o for act in M.build_parser()._actions for o in act.option_strings]
    assert not [f for f in flags if f.startswith("--hutch") and f != "--hutchs"]      # --hutch keeps resolving by prefix
    # main() hands the flag to the constructor: a square --force_dim is built as a lattice, any other is refused before anything runs
    seen = {}

    def fake_run(dist, args, sample_model, log_every=1):
        seen["block"] = dist.target_block()
        return np.zeros(5), np.zeros(5)

    monkeypatch.setattr(M, "run", fake_run)
    M.main(M.build_parser().parse_args(["--example", "phi-four", "--phi4_dim_phys", "2", "--force_dim", "144", "--seed", "1"]))
    assert seen["block"] == (0, [0.1, 20.0, 0.0, 0.0, 2.0])
    M.main(M.build_parser().parse_args(["--example", "phi-four", "--phi4_dim_phys", "2", "--seed", "1"]))      # the default dim = 64 = 8 x 8
    assert seen["block"] == (0, [0.1, 20.0, 0.0, 0.0, 2.0])
    M.main(M.build_parser().parse_args(["--example", "phi-four", "--force_dim", "40", "--seed", "1"]))
    assert seen["block"] == (0, [0.1, 20.0])
    with pytest.raises(ValueError):
        M.main(M.build_parser().parse_args(["--example", "phi-four", "--phi4_dim_phys", "2", "--force_dim", "40", "--seed", "1"]))
