"""CPU tests of the host side of ChEES-HMC: the surface of ``mfm_chees_warmup`` / ``mfm_hmc_run_lengths`` (header, ctypes table,
``Context``), ``chees_adaptation``'s refusals before any device work, ``integration_steps_fn``, the per-step leapfrog counts of
``hmc(...).step.run`` and the ``--hmc_adapt`` checks."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import chees_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_TYPES = {"int": "c_int", "int32_t": "c_int", "uint32_t": "c_uint", "double": "c_double"}


def test_c_abi_surface_mirrors_the_header():
    """Argument for argument: a pointer in the header is a pointer in the ctypes table, a scalar has the header's type."""
    import ctypes as C
    from mfm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mfm.h")).read()
    for name, nargs in (("mfm_chees_warmup", 23), ("mfm_hmc_run_lengths", 20)):
        assert name in _lib.EXPORTS
        res, sig = _lib._SIGS[name]
        assert res is C.c_int and len(sig) == nargs
        decl = re.sub(r"/\*.*?\*/", "", re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1), flags=re.S)
        params = [p.strip() for p in decl.split(",")]
        assert len(params) == nargs, name
        for p, ty in zip(params, sig):
            if "*" in p:
                assert ty in (C.c_void_p, C.POINTER(C.c_double)), (name, p, ty)
                assert (ty is C.POINTER(C.c_double)) == p.startswith("double* h_"), (name, p)      # host pointers are typed, device pointers opaque
            else:
                want = C_TYPES[p.split()[0]]
                assert ty is getattr(C, want) or (want == "c_int" and ty is C.c_int32) or (want == "c_uint" and ty is C.c_uint32), (name, p, ty)
    decl = re.search(r"int mfm_hmc_run_lengths\(([^;]*)\);", hdr).group(1)
    run = re.search(r"int mfm_hmc_run\(([^;]*)\);", hdr).group(1)
    assert "const int32_t* d_num_steps" in decl and "int32_t num_steps" in run                      # mfm_hmc_run keeps its scalar
    params = list(inspect.signature(_lib.Context.chees_warmup).parameters)
    assert params[1:8] == ["key", "beta", "step0", "n_iter", "pos", "logp", "grad"]
    sig = inspect.signature(_lib.Context.chees_warmup).parameters
    assert (sig["target_accept"].default, sig["learning_rate"].default, sig["max_leapfrog"].default, sig["decay"].default,
            sig["divergence_threshold"].default, sig["traj0"].default) == (0.651, 0.025, 1000, 0.5, 1000.0, None)
    params = list(inspect.signature(_lib.Context.hmc_run_lengths).parameters)
    assert params[1:8] == ["key", "beta", "step_size", "num_steps", "pos", "logp", "grad"] and "total_leapfrog" in params
    assert list(inspect.signature(_lib.Context.hmc_run).parameters)[1:6] == ["key", "beta", "step_size", "num_steps", "n_steps"]


def test_optimizer_must_be_the_adam_descriptor():
    from mfm_amd.bblackjax.adaptation.chees_adaptation import chees_adaptation
    from mfm_amd.bblackjax.optimizers import adam, sgd
    from mfm_amd.distributions import PhiFour
    wa = chees_adaptation(PhiFour(64).logprob, 16)
    assert (wa.target_acceptance_rate, wa.decay_rate, wa.max_leapfrog, wa.inverse_mass_matrix) == (0.651, 0.5, 1000, None)
    for bad in (sgd(0.1), 0.025, None, lambda g: g, ("adam", 0.025)):
        with pytest.raises(TypeError, match="adam"):
            wa.run(None, None, 0.1, bad, 8)                      # (no state, no key: raised before any of them is looked at)
    with pytest.raises(ValueError, match="b1"):
        wa.run(None, None, 0.1, adam(0.025, b1=0.8), 8)
    with pytest.raises(ValueError, match="inverse_mass_matrix"):
        chees_adaptation(PhiFour(64).logprob, 16, inverse_mass_matrix=np.ones(3))


def test_integration_steps_fn():
    from mfm_amd.bblackjax.adaptation import chees_adaptation as CA
    assert [CA.radical_inverse(t) for t in range(1, 64)] == [cr.radical_inverse(t) for t in range(1, 64)]
    eps, T = 0.03, 0.41
    got = [CA.integration_steps(i, eps, T, 1000) for i in range(32)]
    assert got == [cr.num_leapfrog(cr.radical_inverse(i + 1) * T, eps, 1000) for i in range(32)]
    assert got[0] == 7 and got[1] == 4 and min(got) >= 1                  # h_1 = 1/2: ceil(0.205 / 0.03); h_2 = 1/4
    assert CA.integration_steps(0, 0.03, 0.41, 5) == 5 and CA.integration_steps(0, 1.0, 0.1, 5) == 1
    assert CA.CheesAdaptationInfo._fields == ("step_size", "trajectory_length", "num_integration_steps", "harmonic_mean_acceptance",
                                              "trajectory_gradient", "num_divergent", "mean_acceptance")
    sig = inspect.signature(CA.chees_adaptation.__init__).parameters
    assert list(sig)[1:] == ["logdensity_fn", "num_chains", "target_acceptance_rate", "decay_rate", "max_leapfrog", "inverse_mass_matrix"]
    assert list(inspect.signature(CA.chees_adaptation.run).parameters)[1:6] == ["rng_key", "state", "step_size", "optimizer", "num_steps"]


def test_per_step_leapfrog_counts_of_step_run():
    from mfm_amd.bblackjax.mcmc import hmc as H
    assert H.HMCRunInfo._fields == ("acceptance_rate", "num_accepted", "last", "positions", "logdensities")      # the tuple is MALARunInfo's still
    assert H.HMCRunInfo(1, 2, 3, 4, 5).num_leapfrog is None                 # the count rides beside the tuple: existing callers unchanged
    info = H.HMCRunLengthsInfo(1, 2, 3, 4, 5, 17)
    assert isinstance(info, H.HMCRunInfo) and tuple(info) == (1, 2, 3, 4, 5) and info.num_leapfrog == 17 and info.last == 3
    np.testing.assert_array_equal(H.integration_step_counts([3, 1, 2], 3), np.array([3, 1, 2], dtype=np.int32))
    got = H.integration_step_counts(lambda i: i + 1, 4)
    assert got.dtype == np.int32 and got.tolist() == [1, 2, 3, 4]
    for bad in ([1, 2], [[1, 2, 3]], [1, 0, 2], [1, 2.5, 3], [1, 2, 100001]):
        with pytest.raises(ValueError, match="num_integration_steps_per_step"):
            H.integration_step_counts(bad, 3)
    assert "num_integration_steps_per_step" in inspect.signature(H.build_kernel().run).parameters


def _args(**kw):
    from oracle import loop
    return loop.default_args(**kw)


def test_hmc_adapt_checks_come_before_any_device_work():
    from mfm_amd import exe_flow_matching as E, multi_modal
    ok = _args(mcmc_kernel="hmc", hmc_adapt="chees", adapt_steps=8)
    assert E.check_adapt_args(ok) == 8
    assert E.check_adapt_args(_args(mcmc_kernel="hmc", adapt_steps=8)) == 8           # absent: 'dual', today's behaviour
    assert E.check_adapt_args(_args(mcmc_kernel="hmc", hmc_adapt="dual", adapt_steps=0)) == 0
    with pytest.raises(ValueError, match="--mcmc_kernel hmc"):
        E.check_adapt_args(_args(mcmc_kernel="nuts", hmc_adapt="chees", adapt_steps=8))
    with pytest.raises(ValueError, match="hmc"):
        E.check_adapt_args(_args(mcmc_kernel="mala", hmc_adapt="chees", adapt_steps=8))
    with pytest.raises(ValueError, match="--adapt_steps N"):
        E.check_adapt_args(_args(mcmc_kernel="hmc", hmc_adapt="chees", adapt_steps=0))
    with pytest.raises(ValueError, match="--adapt_mass"):
        E.check_adapt_args(_args(mcmc_kernel="hmc", hmc_adapt="chees", adapt_steps=8, adapt_mass=True))
    with pytest.raises(ValueError, match="dual or chees"):
        E.check_adapt_args(_args(mcmc_kernel="hmc", hmc_adapt="nuts", adapt_steps=8))
    # E.run raises them first of all (no engine, no GPU)
    from mfm_amd.distributions import PhiFour
    with pytest.raises(ValueError, match="--adapt_steps N"):
        E.run(PhiFour(64), _args(mcmc_kernel="hmc", hmc_adapt="chees", adapt_steps=0))
    # the leapfrog count of training iteration i
    a = _args(mcmc_kernel="hmc", hmc_steps=7, step_size=0.03)
    assert E.hmc_num_steps(a, 5) == 7
    a.hmc_trajectory_length = 0.41
    assert [E.hmc_num_steps(a, i) for i in range(4)] == [cr.num_leapfrog(cr.radical_inverse(i + 1) * 0.41, 0.03, 1000) for i in range(4)]
    src = open(os.path.join(ROOT, "mfm_amd", "multi_modal.py")).read()
    assert re.search(r"add_argument\('--hmc_adapt', type=str, default='dual', choices=\['dual', 'chees'\]\)", src)
    assert multi_modal is not None
