"""Host-side tests of the MCLMC surface: the library's exports and signatures, the Python kernel's dispatch against a stub context, the
command line's flags and the refusals raised before any device work (``--mcmc_kernel mclmc``)."""
import numpy as np
import pytest

from oracle import loop


def test_surface():
    import inspect
    from mfm_amd import _lib
    for name in ("mfm_mclmc_init", "mfm_mclmc_step", "mfm_mclmc_step_keys", "mfm_mclmc_run"):
        assert name in _lib.EXPORTS and name in _lib._SIGS, name
    assert len(_lib._SIGS["mfm_mclmc_step"][1]) == 13 and len(_lib._SIGS["mfm_mclmc_step_keys"][1]) == 12 and len(_lib._SIGS["mfm_mclmc_run"][1]) == 21
    run = list(inspect.signature(_lib.Context.mclmc_run).parameters)
    assert run[:11] == ["self", "key", "beta", "step_size", "L", "integrator", "n_steps", "pos", "logp", "grad", "momentum"]
    from mfm_amd import bblackjax
    from mfm_amd.bblackjax.mcmc import mclmc as M
    assert bblackjax.mclmc is M.mclmc and callable(bblackjax.mclmc_find_L_and_step_size)
    assert M.IntegratorState._fields == ("position", "momentum", "logdensity", "logdensity_grad")
    assert M.MCLMCInfo._fields == ("logdensity", "kinetic_change", "energy_change")
    assert [M.integrator_id(v) for v in ("leapfrog", "mclachlan", 0, 1)] == [0, 1, 0, 1]
    for bad in ("verlet", 2, None):
        with pytest.raises(ValueError, match="integrator"):
            M.integrator_id(bad)


def test_the_header_declares_the_entry_points():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mfm.h")).read()
    for name in ("mfm_mclmc_init", "mfm_mclmc_step", "mfm_mclmc_step_keys", "mfm_mclmc_run"):
        assert f"int {name}(" in text, name


# ---- the Python kernel against a stub context that records the calls ----
class _StubCtx:
    def __init__(self, log):
        self.log = log

    def __getattr__(self, name):
        if name not in ("set_inverse_mass", "mala_init", "mclmc_init", "mclmc_step", "mclmc_step_keys", "mclmc_run"):
            raise AttributeError(name)

        def call(*a, **kw):
            self.log.append((name, a, kw))
        return call


class _StubEngine:
    n_valid = 16

    def __init__(self, log):
        import torch
        self.torch = torch
        self.ctx = _StubCtx(log)


def test_kernel_dispatch_and_python_refusals(monkeypatch):
    import torch
    from mfm_amd import random as jr
    from mfm_amd.bblackjax.mcmc import mclmc as M
    from mfm_amd.distributions import LogGaussianCoxPines, PhiFour
    log = []
    eng = _StubEngine(log)
    monkeypatch.setattr(M, "_engine", lambda d: eng)
    monkeypatch.setattr(M, "energy_var_per_dim", lambda *a, **k: 0.0)
    dist = PhiFour(16)
    algo = M.mclmc(dist.logprob, 4.0, 0.1)
    key = jr.PRNGKey(1)
    st = algo.init(torch.zeros(16, 16), key)
    assert [c[0] for c in log] == ["set_inverse_mass", "mala_init", "mclmc_init"] and log[0][1] == (None,)
    assert isinstance(st, M.IntegratorState) and st.momentum.dtype == torch.float64 and st.momentum.shape == (16, 16)
    del log[:]
    algo.step(key, st)
    assert log[-1][0] == "mclmc_step" and log[-1][1][1:5] == (1.0, 0.1, 4.0, 1)          # beta, step size, L, McLachlan
    algo.step(np.asarray(jr.split(key, 16)), st)
    assert log[-1][0] == "mclmc_step_keys"
    _, info = algo.step.run(key, st, 4, thin=2, keep_energy=True)
    assert log[-1][0] == "mclmc_run" and log[-1][1][1:6] == (1.0, 0.1, 4.0, 1, 4)
    assert log[-1][2]["thin"] == 2 and log[-1][2]["traj_pos"].shape == (2, 16, 16) and log[-1][2]["energy_trace"].shape == (4, 16)
    assert isinstance(info, M.MCLMCRunInfo) and info.positions.shape == (2, 16, 16)
    M.mclmc(lambda x: 0.5 * dist.loglik(x) + dist.logprior(x), np.inf, 0.1, "leapfrog").step(key, st)
    assert log[-1][1][1:5] == (0.5, 0.1, np.inf, 0)
    del log[:]
    cox = LogGaussianCoxPines(16)
    with pytest.raises(ValueError, match="mclmc is not served on the Cox process"):
        M.mclmc(cox.logprob, 4.0, 0.1)
    with pytest.raises(ValueError, match="mclmc is not served on the Cox process"):
        M.build_kernel()(key, st, cox.logprob, 4.0, 0.1)
    for L, eps in ((0.0, 0.1), (float("nan"), 0.1), (4.0, 0.0), (4.0, np.inf)):
        with pytest.raises(ValueError, match="mclmc needs L > 0"):
            M.mclmc(dist.logprob, L, eps)
    assert log == []                                            # nothing reached the context


# ---- the command line ----
def _args(*flags, example="phi-four"):
    from mfm_amd import multi_modal as M
    return M.build_parser().parse_args(["--seed", "1", "--example", example, *flags])


def test_flags_parse():
    a = _args("--mcmc_kernel", "mclmc")
    assert (a.mcmc_kernel, a.mclmc_L, a.mclmc_integrator) == ("mclmc", 0.0, "mclachlan")
    a = _args("--mcmc_kernel", "mclmc", "--mclmc_L", "3.5", "--mclmc_integrator", "leapfrog", "--adapt_steps", "100", "--ess_steps", "16")
    assert (a.mclmc_L, a.mclmc_integrator, a.adapt_steps, a.ess_steps) == (3.5, "leapfrog", 100, 16)
    with pytest.raises(SystemExit):
        _args("--mcmc_kernel", "mclmc", "--mclmc_integrator", "verlet")


def test_L_defaults_to_the_square_root_of_the_dimension():
    from mfm_amd import exe_flow_matching as E
    assert E.mclmc_L(loop.default_args(mcmc_kernel="mclmc", dim=64)) == 8.0
    assert E.mclmc_L(loop.default_args(mcmc_kernel="mclmc", dim=64, mclmc_L=0.0)) == 8.0
    assert E.mclmc_L(loop.default_args(mcmc_kernel="mclmc", dim=64, mclmc_L=2.5)) == 2.5


def test_check_adapt_args_serves_and_refuses():
    from mfm_amd import exe_flow_matching as E
    assert E.check_adapt_args(loop.default_args(mcmc_kernel="mclmc")) == 0
    assert E.check_adapt_args(loop.default_args(mcmc_kernel="mclmc", adapt_steps=200, mclmc_integrator="leapfrog")) == 200
    with pytest.raises(ValueError, match="--adapt_mass is not served with --mcmc_kernel mclmc"):
        E.check_adapt_args(loop.default_args(mcmc_kernel="mclmc", adapt_steps=200, adapt_mass=True))
    with pytest.raises(ValueError, match="--hmc_adapt chees .* needs --mcmc_kernel hmc"):
        E.check_adapt_args(loop.default_args(mcmc_kernel="mclmc", adapt_steps=200, hmc_adapt="chees"))
    with pytest.raises(ValueError, match="--mclmc_L must be positive"):
        E.check_mclmc_args(loop.default_args(mcmc_kernel="mclmc", mclmc_L=-1.0))
    with pytest.raises(ValueError, match="integrator"):
        E.check_mclmc_args(loop.default_args(mcmc_kernel="mclmc", mclmc_integrator="verlet"))
    E.check_mclmc_args(loop.default_args(mcmc_kernel="mclmc", mclmc_L=2.0, mclmc_integrator="leapfrog"))
    E.check_mclmc_args(loop.default_args(mcmc_kernel="mala", mclmc_L=-1.0))                # (another kernel does not read the flag)
    with pytest.raises(ValueError, match="--adapt_steps needs --mcmc_kernel hmc"):          # (unchanged for MALA)
        E.check_adapt_args(loop.default_args(mcmc_kernel="mala", adapt_steps=8))


REFUSED = ((["--mcmc_kernel", "mclmc", "--force_dim", "64"], "pines", "--mcmc_kernel mclmc is not served with --example pines"),
           (["--mcmc_kernel", "mclmc", "--adapt_steps", "8", "--adapt_mass"], "phi-four", "--adapt_mass is not served with --mcmc_kernel mclmc"),
           (["--mcmc_kernel", "mclmc", "--adapt_steps", "8", "--hmc_adapt", "chees"], "phi-four", "--hmc_adapt chees .* needs --mcmc_kernel hmc"),
           (["--mcmc_kernel", "mclmc", "--do_pt"], "phi-four",
            r"--do_pt takes --mcmc_kernel mala or hmc as the local move \(got mclmc: NUTS and MCLMC are not served\)"))


@pytest.mark.parametrize("flags,example,msg", REFUSED)
def test_cli_refusals_before_any_device_work(flags, example, msg):
    from mfm_amd import multi_modal as M
    with pytest.raises(ValueError, match=msg):
        M.main(_args(*flags, example=example))


def test_run_refuses_before_any_device_work():
    from mfm_amd import exe_flow_matching as E
    from mfm_amd.distributions import LogGaussianCoxPines, PhiFour
    with pytest.raises(ValueError, match="--mcmc_kernel mclmc is not served with --example pines"):
        E.run(LogGaussianCoxPines(64), _args("--mcmc_kernel", "mclmc", "--force_dim", "64", example="pines"))
    with pytest.raises(ValueError, match="--adapt_mass is not served with --mcmc_kernel mclmc"):
        E.run(PhiFour(64), loop.default_args(mcmc_kernel="mclmc", adapt_steps=8, adapt_mass=True))
    with pytest.raises(ValueError, match="--mclmc_L must be positive"):
        E.run(PhiFour(64), loop.default_args(mcmc_kernel="mclmc", mclmc_L=-1.0))
    E.check_cox_args(PhiFour(64), loop.default_args(mcmc_kernel="mclmc"))


def test_thinned_runs_keep_at_most_kept_states():
    from mfm_amd.bblackjax.adaptation.mclmc_adaptation import KEPT, _thinned
    for n in (1, 31, 32, 33, 63, 64, 200, 1000):
        steps, thin = _thinned(n)
        assert steps % thin == 0 and 1 <= steps // thin <= KEPT and steps <= max(n, thin), (n, steps, thin)
