"""Phi-four with periodic and non-zero Dirichlet boundaries: the restated oracle (tests/phi4_bc_oracle.py) against autograd and a
literal NumPy transcription of the reference's energy (distributions.py:144-151), the PhiFour constructor, its target block and
the CLI flags.  CPU only."""
import numpy as np
import pytest

from oracle import targets
from tests.phi4_bc_oracle import PhiFourBC

BCS = [("pbc", 0.0), ("dirichlet", 0.0), ("dirichlet", 1.0), ("dirichlet", -0.7)]
DIMS = [3, 40, 64]


def _ref_U(x, a, bc):
    """The reference's U, transcribed: jnp.pad(x, (1, 0), mode='wrap') for 'pbc', constant pads of b on both sides otherwise."""
    d = x.shape[-1]
    coef = a * d
    if bc[0] == "pbc":
        xp = np.pad(x, ((0, 0), (1, 0)), mode="wrap")
    else:
        xp = np.pad(x, ((0, 0), (1, 1)), mode="constant", constant_values=bc[1])
    diffs = xp[:, 1:] - xp[:, :-1]
    return (diffs ** 2).sum(1) / 2.0 * coef


def _ref_loglik(x, a, beta, bc):
    d = x.shape[-1]
    V = ((1.0 - x ** 2) ** 2).sum(1) / 4.0 / (a * d)
    return -beta * (_ref_U(x, a, bc) + V)


def _states(d, n=5, seed=0):
    return np.random.default_rng(seed + d).uniform(-1.5, 1.5, (n, d))


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("d", DIMS)
def test_value_matches_reference_transcription(d, bc):
    dist = PhiFourBC(d, 0.1, 20.0, bc)
    x = _states(d)
    np.testing.assert_allclose(dist.loglik(x), _ref_loglik(x, 0.1, 20.0, bc), rtol=1e-13, atol=1e-9)
    np.testing.assert_allclose(dist.logprob(x), dist.loglik(x), rtol=0, atol=0)


@pytest.mark.parametrize("bc", BCS)
@pytest.mark.parametrize("d", DIMS)
def test_gradient_and_hvp_match_autograd(d, bc):
    import torch
    dist = PhiFourBC(d, 0.1, 20.0, bc)
    x = _states(d)
    v = np.random.default_rng(7).normal(size=x.shape)
    coef = 0.1 * d

    def U(xt):
        if bc[0] == "pbc":
            xp = torch.cat([xt[:, -1:], xt], 1)
        else:
            e = torch.full((xt.shape[0], 1), bc[1], dtype=torch.float64)
            xp = torch.cat([e, xt, e], 1)
        dd = xp[:, 1:] - xp[:, :-1]
        return -20.0 * ((dd ** 2).sum(1) / 2.0 * coef + ((1.0 - xt ** 2) ** 2).sum(1) / 4.0 / coef)

    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    val = U(xt)
    g, = torch.autograd.grad(val.sum(), xt, create_graph=True)
    hv, = torch.autograd.grad((g * torch.tensor(v)).sum(), xt)
    np.testing.assert_allclose(dist.loglik(x), val.detach().numpy(), rtol=1e-13, atol=1e-9)
    np.testing.assert_allclose(dist.grad_logprob(x), g.detach().numpy(), rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(dist.hvp_logprob(x, v), hv.numpy(), rtol=1e-12, atol=1e-9)
    # the exact-trace Hessian diagonal is the boundary's too: the parent's (unchanged)
    hd = np.stack([dist.hvp_logprob(x, np.broadcast_to(np.eye(d)[j][None], x.shape))[:, j] for j in range(d)], 1)
    np.testing.assert_allclose(dist.hess_diag(x), hd, rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("d", DIMS)
def test_dirichlet_zero_equals_the_existing_oracle(d):
    new, old = PhiFourBC(d, 0.1, 20.0, ("dirichlet", 0)), targets.PhiFour(d, 0.1, 20.0)
    x, v = _states(d), np.random.default_rng(3).normal(size=(5, d))
    np.testing.assert_array_equal(new.loglik(x), old.loglik(x))
    np.testing.assert_array_equal(new.grad_logprob(x), old.grad_logprob(x))
    np.testing.assert_array_equal(new.hvp_logprob(x, v), old.hvp_logprob(x, v))


@pytest.mark.parametrize("bc", [("pbc", 0.0), ("dirichlet", 1.0)])
def test_boundaries_differ_from_dirichlet_zero(bc):
    """The other boundaries move value, gradient and HVP at the ends only (periodic: the HVP too; Dirichlet b: not the HVP)."""
    d = 40
    new, old = PhiFourBC(d, 0.1, 20.0, bc), targets.PhiFour(d)
    x, v = _states(d), np.random.default_rng(3).normal(size=(5, d))
    assert np.abs(new.loglik(x) - old.loglik(x)).min() > 1e-3
    dg = np.abs(new.grad_logprob(x) - old.grad_logprob(x))
    assert dg[:, [0, -1]].min() > 1e-3 and dg[:, 1:-1].max() == 0
    dh = np.abs(new.hvp_logprob(x, v) - old.hvp_logprob(x, v))
    if bc[0] == "pbc":
        assert dh[:, [0, -1]].min() > 1e-3
    else:
        assert dh.max() == 0


# ---- the package's PhiFour, its target block and the CLI ---------------------------------------------------------------------
def test_phifour_constructor_accepts_and_rejects():
    from mfm_amd.distributions import PhiFour
    assert PhiFour(64).target_block() == (0, [0.1, 20.0])
    assert PhiFour(64, bc=("dirichlet", 0)).target_block() == (0, [0.1, 20.0])
    assert PhiFour(64, bc=("dirichlet", 0.0)).target_block() == (0, [0.1, 20.0])
    assert PhiFour(64, a=0.2, beta=10.0, bc=("dirichlet", 1)).target_block() == (0, [0.2, 10.0, 0.0, 1.0])
    assert PhiFour(64, bc=("dirichlet", -0.7)).target_block() == (0, [0.1, 20.0, 0.0, -0.7])
    assert PhiFour(64, bc=("pbc", 3.0)).target_block() == (0, [0.1, 20.0, 1.0, 0.0])
    assert PhiFour(64, bc=("pbc", None)).target_block() == (0, [0.1, 20.0, 1.0, 0.0])
    with pytest.raises(ValueError):
        PhiFour(64, bc=("neumann", 0))
    with pytest.raises(ValueError):
        PhiFour(64, bc=("dirichlet", float("inf")))
    with pytest.raises(ValueError):
        PhiFour(64, bc=("dirichlet", float("nan")))
    with pytest.raises(NotImplementedError):
        PhiFour(64, tilt=0.1)
    with pytest.raises(NotImplementedError):
        PhiFour(64, bc=("pbc", 0), tilt=0.1)


def test_cli_flags():
    from mfm_amd.multi_modal import build_parser
    a = build_parser().parse_args([])
    assert a.phi4_bc == "dirichlet" and a.phi4_bc_value == 0.0
    a = build_parser().parse_args(["--phi4_bc", "pbc", "--phi4_bc_value", "-0.5", "--hutch"])
    assert a.phi4_bc == "pbc" and a.phi4_bc_value == -0.5 and a.hutchs
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--phi4_bc", "neumann"])
    flags = [o for act in build_parser()._actions for o in act.option_strings]
    assert not [f for f in flags if f.startswith("--hutch") and f != "--hutchs"]      # --hutch keeps resolving by prefix
