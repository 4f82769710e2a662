"""CPU tests of the host side of parallel tempering: the surface of ``mfm_pt_run`` / ``mfm_pt_exchange`` (header, ctypes table,
``Context``), the refusals of ``parallel_tempering`` and ``--do_pt`` before any device work, and the ladder helpers."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_TYPES = {"int": "c_int", "int32_t": "c_int", "uint32_t": "c_uint", "double": "c_double"}


def test_c_abi_surface_mirrors_the_header():
    """Argument for argument: a pointer in the header is a pointer in the ctypes table (host pointers typed, device pointers opaque), a
    scalar has the header's type; the header states the key schedule."""
    import ctypes as C
    from mfm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mfm.h")).read()
    for name, nargs in (("mfm_pt_exchange", 13), ("mfm_pt_run", 24)):
        assert name in _lib.EXPORTS
        res, sig = _lib._SIGS[name]
        assert res is C.c_int and len(sig) == nargs
        decl = re.sub(r"/\*.*?\*/", "", re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1), flags=re.S)
        params = [p.strip() for p in decl.split(",")]
        assert len(params) == nargs, name
        for p, ty in zip(params, sig):
            if "*" in p:
                assert ty in (C.c_void_p, C.POINTER(C.c_double)), (name, p, ty)
                assert (ty is C.POINTER(C.c_double)) == p.startswith("const double* h_"), (name, p)
            else:
                want = C_TYPES[p.split()[0]]
                assert ty is getattr(C, want) or (want == "c_int" and ty is C.c_int32) or (want == "c_uint" and ty is C.c_uint32), (name, p, ty)
    run = [p.strip().split()[-1].lstrip("*") for p in re.sub(r"/\*.*?\*/", "", re.search(r"int mfm_pt_run\(([^;]*)\);", hdr).group(1), flags=re.S).split(",")]
    assert run == ["ctx", "kernel", "key0", "key1", "h_betas", "h_step_sizes", "n_temps", "n_ladders", "num_steps", "textbook", "n_local", "n_rounds",
                   "exchange", "thin", "d_pos", "d_logp", "d_grad", "d_n_accepted", "d_acc_sum", "d_replica", "d_swap_accepted", "d_swap_prob",
                   "d_traj_pos", "d_traj_logp"]
    ex = [p.strip().split()[-1].lstrip("*") for p in re.sub(r"/\*.*?\*/", "", re.search(r"int mfm_pt_exchange\(([^;]*)\);", hdr).group(1), flags=re.S).split(",")]
    assert ex == ["ctx", "key0", "key1", "h_betas", "n_temps", "n_ladders", "parity", "d_pos", "d_logp", "d_grad", "d_replica", "d_swap_accepted",
                  "d_swap_prob"]
    for phrase in ("(k_move, k_swap) = split(key, 2)", "split(k_move, n_rounds)[t]", "split(k_swap, n_rounds)[t]", "n_chain_total)[chain_offset + i]"):
        assert phrase in hdr, phrase
    params = list(inspect.signature(_lib.Context.pt_run).parameters)
    assert params[1:10] == ["key", "betas", "step_sizes", "n_ladders", "n_local", "n_rounds", "pos", "logp", "grad"]
    for name in ("kernel", "num_steps", "textbook", "exchange", "thin", "n_acc", "acc_sum", "replica", "swap_accepted", "swap_prob", "traj_pos", "traj_logp"):
        assert name in params, name
    params = list(inspect.signature(_lib.Context.pt_exchange).parameters)
    assert params[1:8] == ["key", "betas", "n_ladders", "parity", "pos", "logp", "grad"] and params[8:] == ["replica", "swap_accepted", "swap_prob"]
    src = open(os.path.join(ROOT, "mfm_amd", "csrc", "api.hip")).read()
    assert '#include "pt.hip"' in src and os.path.exists(os.path.join(ROOT, "mfm_amd", "csrc", "pt.hip"))


def test_ladder_helpers():
    from mfm_amd.bblackjax.mcmc import parallel_tempering as PT
    b = PT.geometric_ladder(8, 0.01)
    assert b[0] == 1.0 and b[-1] == 0.01 and (np.diff(b) < 0).all()
    np.testing.assert_allclose(b[1:] / b[:-1], 0.01 ** (1 / 7), rtol=1e-12)
    for bad in ((1, 0.1), (4, 0.0), (4, 1.0)):
        with pytest.raises(ValueError, match="geometric_ladder"):
            PT.geometric_ladder(*bad)
    assert PT.communication_barrier([0.75, 0.5, 1.0]) == 0.75
    # equal rates: the identity (every pair already rejects equally)
    for b0 in (b, np.array([1.0, 0.6, 0.35, 0.1])):
        np.testing.assert_allclose(PT.adapt_ladder(b0, np.full(b0.size - 1, 0.7)), b0, rtol=1e-12)
    # unequal rates: the end points stay, the ladder stays monotone, and points move towards the pair that rejects most
    rates = np.array([0.9, 0.2, 0.8, 0.6, 0.95, 0.5, 0.7])
    new = PT.adapt_ladder(b, rates)
    assert new[0] == b[0] and new[-1] == b[-1] and (np.diff(new) < 0).all()
    inside = lambda v, k: int(((v < b[k]) & (v > b[k + 1])).sum())
    assert inside(new, 1) > inside(b, 1)
    # a fixed point of the update: the interpolated barrier is cut into equal parts
    cum = np.concatenate([[0.0], np.cumsum(1.0 - rates)])
    lam = np.interp(new[::-1], b[::-1], cum[::-1])[::-1]
    np.testing.assert_allclose(np.diff(lam), cum[-1] / 7, rtol=1e-9)
    assert (np.diff(PT.adapt_ladder(b, np.ones(7))) < 0).all()                 # no rejection anywhere: still a ladder
    with pytest.raises(ValueError, match="adapt_ladder"):
        PT.adapt_ladder(b, rates[:-1])


def test_parallel_tempering_refuses_before_any_device_work():
    from mfm_amd.bblackjax.mcmc import parallel_tempering as PT
    from mfm_amd.distributions import PhiFour
    dist = PhiFour(64)                                                   # (no engine attached: anything past the checks would raise RuntimeError)
    ok = dict(mcmc="hmc", step_size=0.01)
    algo = PT.parallel_tempering(dist.logprior, dist.loglik, [1.0, 0.5], **ok)
    assert callable(algo.step.run)
    assert PT.PTState._fields == ("position", "logdensity", "logdensity_grad", "replica")
    assert PT.PTInfo._fields == ("swap_acceptance_rate", "swap_accepted", "acceptance_rate", "positions", "logdensities")
    sig = inspect.signature(PT.parallel_tempering.__new__).parameters
    assert list(sig)[1:] == ["logprior_fn", "loglikelihood_fn", "betas", "mcmc", "step_size", "num_integration_steps", "num_mcmc_steps", "exchange", "textbook"]
    assert (sig["mcmc"].default, sig["num_integration_steps"].default, sig["num_mcmc_steps"].default, sig["exchange"].default) == ("hmc", 10, 1, "even_odd")
    from mfm_amd.bblackjax.mcmc import mala
    assert sig["textbook"].default == inspect.signature(mala.build_kernel).parameters["textbook"].default
    for kw, match in ((dict(betas=[1.0]), "2 to 64"), (dict(betas=np.ones(65)), "2 to 64"), (dict(betas=[1.0, 0.0]), "finite and positive"),
                      (dict(betas=[1.0, np.nan]), "finite and positive"), (dict(mcmc="nuts"), "NUTS"), (dict(exchange="random"), "even_odd"),
                      (dict(step_size=[0.1, 0.2, 0.3]), "step_size"), (dict(step_size=-1.0), "step_size"), (dict(num_mcmc_steps=0), "at least 1")):
        args = dict(dict(betas=[1.0, 0.5]), **ok)
        args.update(kw)
        betas = args.pop("betas")
        with pytest.raises(ValueError, match=match):
            PT.parallel_tempering(dist.logprior, dist.loglik, betas, **args)
    # a scalar step size s means s / sqrt(beta_k)
    b, s, _, ex = PT.check_arguments([1.0, 0.25], "mala", 0.1, 10, 1, "none")
    np.testing.assert_array_equal(s, [0.1, 0.2])
    assert ex is False and PT.check_arguments([1.0, 0.25], "hmc", [0.3, 0.4], 10, 1, "even_odd")[1].tolist() == [0.3, 0.4]


def _args(**kw):
    from oracle import loop
    a = loop.default_args(**kw)
    for k, v in dict(do_pt=True, pt_temps=8, pt_beta_min=0.01, pt_local_steps=4, do_smc=False, do_svgd=False).items():
        if not hasattr(a, k) or k in kw:
            setattr(a, k, kw.get(k, v))
    return a


def test_do_pt_checks_come_before_any_device_work():
    from mfm_amd import exe_others as X
    from mfm_amd.distributions import PhiFour
    assert X.check_pt_args(_args(num_chain=64, mcmc_kernel="hmc")) == (8, 8)
    assert X.check_pt_args(_args(num_chain=60, pt_temps=4)) == (4, 15)
    with pytest.raises(ValueError, match="multiple of --pt_temps"):
        X.check_pt_args(_args(num_chain=60))
    with pytest.raises(ValueError, match="NUTS"):
        X.check_pt_args(_args(num_chain=64, mcmc_kernel="nuts"))
    with pytest.raises(ValueError, match="--do_smc"):
        X.check_pt_args(_args(num_chain=64, do_smc=True))
    with pytest.raises(ValueError, match="--do_svgd"):
        X.check_pt_args(_args(num_chain=64, do_svgd=True))
    with pytest.raises(ValueError, match="multiple of --pt_temps"):            # X.run raises them first of all (no engine, no GPU)
        X.run(PhiFour(64), _args(num_chain=60))
    from mfm_amd import multi_modal
    a = multi_modal.build_parser().parse_args(["--do_pt"])
    assert (a.do_pt, a.pt_temps, a.pt_beta_min, a.pt_local_steps) == (True, 8, 0.01, 4)
    assert multi_modal.build_parser().parse_args([]).do_pt is False
