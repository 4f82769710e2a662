"""CPU tests of the host side of HMC for the Cox process (``mfm_cox_hmc_*``): the shared case table's conditions with the oracle
alone, the launch plan, the refusals of ``bblackjax.mcmc.hmc`` and of the command line before any device work, and the dispatch of
``hmc.build_kernel()`` by target against a stub context that records the call."""
import numpy as np
import pytest

from tests import cox_hmc_cases as cc

MFM_EINVAL, MFM_ETOOLARGE = -1, -3        # include/mfm.h


@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_case_conditions_hold_in_the_oracle(name):
    """The step size puts the mean acceptance probability inside the band; at most 10 % of the chains come within 1e-3 of a decision."""
    c = cc.BY_NAME[name]
    assert 3 <= c.L <= 8 and 1 <= c.n_steps <= 6 and c.B % 16 == 0 and c.d == c.n * c.n
    ref = cc.reference_of(name)
    pa = np.array([info.acceptance_rate for info, _ in ref])
    u = np.array([uu for _, uu in ref])
    print(name, "mean acceptance", pa.mean(), "share within the margin", (np.abs(u - pa) < cc.MARGIN).any(0).mean())
    assert cc.ACC_BAND[0] <= pa.mean() <= cc.ACC_BAND[1], (name, pa.mean())
    assert (np.abs(u - pa) < cc.MARGIN).any(0).mean() <= cc.MAX_SHARE, name


def test_cases_see_both_decisions():
    seen = set()
    for c in cc.CASES:
        for info, _ in cc.reference_of(c.name):
            seen |= set(info.is_accepted.tolist())
    assert seen == {True, False}
    assert max(c.n_steps for c in cc.CASES if c.d >= 400) < max(c.n_steps for c in cc.CASES)      # fewer steps on the largest grids


def test_launch_plan():
    """mfm_cox_hmc_launch_plan (host only): every case's instance and LDS; the thresholds; the refusals."""
    import ctypes as C
    from mfm_amd import _lib
    for c in cc.CASES:
        tpw, sm = _lib.cox_hmc_launch_plan(c.d)
        dp = (c.d + 15) // 16 * 16
        assert tpw == c.tpw, (c.name, tpw)
        # the position tile [16][dp + 4] float32, the row sums [4][8 waves][16] and the warmup's row state [6][16] float64
        assert sm == 16 * (dp + 4) * 4 + (4 * 8 * 16 + 6 * 16) * 8 and sm <= 160 * 1024, (c.name, sm)
    assert {_lib.cox_hmc_launch_plan(d)[0] for d in range(1, 1025)} == {c.tpw for c in cc.CASES} == {1, 2, 4, 8}
    for d, tpw in ((1, 1), (128, 1), (129, 2), (256, 2), (257, 4), (512, 4), (513, 8), (1024, 8)):      # the thresholds
        assert _lib.cox_hmc_launch_plan(d)[0] == tpw, d
    lib = _lib.load()
    tpw, sm = C.c_int32(-1), C.c_int32(-1)
    for bad in (1025, 1600, 1664, 4096):                      # above the largest instance (the 40 x 40 grid is not served)
        assert lib.mfm_cox_hmc_launch_plan(bad, C.byref(tpw), C.byref(sm)) == MFM_ETOOLARGE, bad
        with pytest.raises(_lib.MfmError, match="too large"):
            _lib.cox_hmc_launch_plan(bad)
    for bad in (0, -3):
        assert lib.mfm_cox_hmc_launch_plan(bad, C.byref(tpw), C.byref(sm)) == MFM_EINVAL, bad
    assert lib.mfm_cox_hmc_launch_plan(16, None, C.byref(sm)) == MFM_EINVAL
    assert lib.mfm_cox_hmc_launch_plan(16, C.byref(tpw), None) == MFM_EINVAL
    assert (tpw.value, sm.value) == (-1, -1)                  # a rejected call touches nothing


def test_surface():
    import inspect
    from mfm_amd import _lib
    for name in ("mfm_cox_hmc_step", "mfm_cox_hmc_step_keys", "mfm_cox_hmc_run", "mfm_cox_hmc_warmup", "mfm_cox_hmc_launch_plan"):
        assert name in _lib.EXPORTS, name
    for name in ("step", "step_keys", "run", "warmup"):          # the keyword names of the hmc_* siblings
        assert (list(inspect.signature(getattr(_lib.Context, "cox_hmc_" + name)).parameters)
                == list(inspect.signature(getattr(_lib.Context, "hmc_" + name)).parameters)), name
        assert _lib._SIGS["mfm_cox_hmc_" + name] == _lib._SIGS["mfm_hmc_" + name], name


# ---- the dispatch of the Python kernel by target, against a stub that records the call ----
class _StubCtx:
    def __init__(self, log):
        self.log = log

    def set_inverse_mass(self, v):
        self.log.append(("set_inverse_mass", v))

    def __getattr__(self, name):
        if not (name.startswith("hmc_") or name.startswith("cox_hmc_")):
            raise AttributeError(name)

        def call(*a, **kw):
            self.log.append((name, a, kw))
            for v in kw.values():                                  # the outputs a real call fills
                if hasattr(v, "zero_"):
                    v.zero_()
        return call


class _StubEngine:
    n_valid = 16

    def __init__(self, log):
        import torch
        self.torch = torch
        self.ctx = _StubCtx(log)


def _stub(monkeypatch, dist):
    from mfm_amd.bblackjax.mcmc import hmc as H
    log = []
    eng = _StubEngine(log)
    monkeypatch.setattr(H, "_engine", lambda d: eng)
    import torch
    st = H.HMCState(torch.zeros(16, dist.dim), torch.zeros(16, dtype=torch.float64), torch.zeros(16, dist.dim))
    return H, log, st


@pytest.mark.parametrize("target", ["cox", "phi4"])
def test_build_kernel_dispatches_by_target(monkeypatch, target):
    from mfm_amd import random as jr
    from mfm_amd.distributions import LogGaussianCoxPines, PhiFour
    dist = LogGaussianCoxPines(16) if target == "cox" else PhiFour(16)
    prefix = "cox_hmc_" if target == "cox" else "hmc_"
    H, log, st = _stub(monkeypatch, dist)
    kernel = H.build_kernel()
    key = jr.PRNGKey(1)
    keys = np.asarray(jr.split(key, 16))

    def calls():
        out = [c[0] for c in log if c[0] != "set_inverse_mass"]
        del log[:]
        return out

    fn = lambda x: 0.5 * dist.loglik(x) + dist.logprior(x)
    kernel(key, st, fn, 0.1, 3)
    assert log[-1][0] == prefix + "step" and log[-1][1][1:4] == (0.5, 0.1, 3)      # beta, step size, leapfrog steps
    assert calls() == [prefix + "step"]
    kernel(keys, st, dist.logprob, 0.1, 3)
    assert calls() == [prefix + "step_keys"]
    kernel.run(key, st, dist.logprob, 0.1, 3, 4, thin=2)
    assert log[-1][2]["thin"] == 2 and log[-1][2]["traj_pos"].shape == (2, 16, 16)
    assert calls() == [prefix + "run"]
    _, info = kernel.warmup(key, st, dist.logprob, 0.1, 3, 4, 0.7, keep_step_sizes=True)
    assert log[-1][1][1:6] == (1.0, 0.1, 3, 4, 0.7) and log[-1][2]["step_traj"].shape == (4, 16)
    assert calls() == [prefix + "warmup"]
    assert isinstance(info, H.HMCWarmupInfo) and hasattr(info, "pooled_step_size")
    algo = H.hmc(dist.logprob, 0.1, 3)
    algo.step(key, st)
    algo.step.run(key, st, 2)
    algo.step.warmup(key, st, 2)
    assert calls() == [prefix + "step", prefix + "run", prefix + "warmup"]


def test_python_refusals_before_any_device_work(monkeypatch):
    from mfm_amd import random as jr
    from mfm_amd.distributions import LogGaussianCoxPines
    dist = LogGaussianCoxPines(16)
    H, log, st = _stub(monkeypatch, dist)
    kernel = H.build_kernel()
    key = jr.PRNGKey(1)
    minv = np.ones(16)
    with pytest.raises(ValueError, match="inverse_mass_matrix is not served on the Cox process"):
        H.hmc(dist.logprob, 0.1, 3, inverse_mass_matrix=minv)
    with pytest.raises(ValueError, match="inverse_mass_matrix is not served on the Cox process"):
        kernel(key, st, dist.logprob, 0.1, 3, minv)
    with pytest.raises(ValueError, match="inverse_mass_matrix is not served on the Cox process"):
        kernel.run(key, st, dist.logprob, 0.1, 3, 4, inverse_mass_matrix=minv)
    with pytest.raises(ValueError, match="inverse_mass_matrix is not served on the Cox process"):
        kernel.warmup(key, st, dist.logprob, 0.1, 3, 4, inverse_mass_matrix=minv)
    with pytest.raises(ValueError, match="num_integration_steps_per_step is not served on the Cox process"):
        kernel.run(key, st, dist.logprob, 0.1, 3, 4, num_integration_steps_per_step=[1, 2, 3, 4])
    with pytest.raises(ValueError, match="num_integration_steps_per_step is not served on the Cox process"):
        H.hmc(dist.logprob, 0.1, 3).step.run(key, st, 4, num_integration_steps_per_step=lambda i: 2)
    assert log == []                                            # nothing reached the context


def _args(*flags):
    from mfm_amd import multi_modal as M
    return M.build_parser().parse_args(["--seed", "1", "--example", "pines", "--force_dim", "64", *flags])


REFUSED = ((["--mcmc_kernel", "hmc", "--adapt_steps", "8", "--adapt_mass"], "--adapt_mass is not served with --example pines"),
           (["--mcmc_kernel", "hmc", "--adapt_steps", "8", "--hmc_adapt", "chees"], "--hmc_adapt chees is not served with --example pines"),
           (["--mcmc_kernel", "nuts"], "--mcmc_kernel nuts is not served with --example pines"),
           (["--do_pt"], "--do_pt is not served with --example pines"),
           (["--do_pt", "--mcmc_kernel", "hmc"], "--do_pt is not served with --example pines"))


@pytest.mark.parametrize("flags,msg", REFUSED)
def test_cli_refusals_before_any_device_work(flags, msg):
    from mfm_amd import exe_flow_matching as E
    from mfm_amd import multi_modal as M
    from mfm_amd.distributions import LogGaussianCoxPines, PhiFour
    with pytest.raises(ValueError, match=msg):
        E.check_cox_args(LogGaussianCoxPines(64), _args(*flags))
    E.check_cox_args(PhiFour(64), _args(*flags))                # the other targets are not this check's business
    with pytest.raises(ValueError, match=msg):
        M.main(_args(*flags))
    with pytest.raises(ValueError, match=msg):
        E.run(LogGaussianCoxPines(64), _args(*flags))


def test_cli_serves_hmc_dual_warmup_and_ess_on_pines():
    from mfm_amd import exe_flow_matching as E
    from mfm_amd.distributions import LogGaussianCoxPines
    for flags in (["--mcmc_kernel", "hmc", "--hmc_steps", "4"], ["--mcmc_kernel", "hmc", "--adapt_steps", "8", "--adapt_target", "0.7"],
                  ["--mcmc_kernel", "hmc", "--ess_steps", "16"], []):
        E.check_cox_args(LogGaussianCoxPines(64), _args(*flags))
    with pytest.raises(ValueError, match="dim <= 1024"):        # the 40 x 40 default grid has no instance
        E.check_cox_args(LogGaussianCoxPines(1600), _args("--mcmc_kernel", "hmc"))
    E.check_cox_args(LogGaussianCoxPines(1600), _args())        # (MALA and the flow steps serve it as before)
