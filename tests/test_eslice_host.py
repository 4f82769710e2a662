"""CPU tests of the host side of elliptical slice sampling: the surface of ``mfm_eslice_*`` (header, ctypes table, ``Context``), the
launch plan against the shared case table, and the refusals of ``elliptical_slice`` and ``--do_eslice`` before any device work."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_TYPES = {"int": "c_int", "int32_t": "c_int32", "uint32_t": "c_uint32", "double": "c_double"}
SURFACE = {"mfm_set_lgcp_chol": 2, "mfm_eslice_init": 3, "mfm_eslice_step": 9, "mfm_eslice_step_keys": 8, "mfm_eslice_run": 18,
           "mfm_eslice_launch_plan": 3}


def test_c_abi_surface_mirrors_the_header():
    import ctypes as C
    from mfm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mfm.h")).read()
    for name, nargs in SURFACE.items():
        assert name in _lib.EXPORTS
        res, sig = _lib._SIGS[name]
        assert res is C.c_int and len(sig) == nargs, name
        decl = re.sub(r"/\*.*?\*/", "", re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1), flags=re.S)
        params = [p.strip() for p in decl.split(",")]
        assert len(params) == nargs, name
        for p, ty in zip(params, sig):
            if "*" in p:
                host = p.split()[-1].lstrip("*").startswith("h_")
                assert ty is (C.POINTER(C.c_double) if p.startswith("const double* h_") else C.POINTER(C.c_int32) if host else C.c_void_p), (name, p, ty)
            else:
                assert ty is getattr(C, C_TYPES[p.split()[0]]) or (p.split()[0] == "int32_t" and ty is C.c_int), (name, p, ty)
    run = [p.strip().split()[-1].lstrip("*") for p in re.sub(r"/\*.*?\*/", "", re.search(r"int mfm_eslice_run\(([^;]*)\);", hdr).group(1), flags=re.S).split(",")]
    assert run[:14] == ["ctx", "key_mode", "key0", "key1", "d_keys", "beta", "n_steps", "thin", "d_pos", "d_loglik", "d_subiter_sum", "d_n_capped",
                        "d_traj_pos", "d_traj_loglik"]
    assert run[14:] == ["d_subiter", "d_theta", "d_momentum", "d_subiter_max"]
    assert re.search(r"#define MFM_ESLICE_MAX_SUBITER 64\b", hdr) and _lib.ESLICE_MAX_SUBITER == 64
    for phrase in ("(k_nu, k_u, k_theta, k_shrink) = split(k_b, 4)", "uniform(k_shrink, (MFM_ESLICE_MAX_SUBITER,))[subiter - 1]", "tess.py:42-44"):
        assert phrase in hdr, phrase
    params = list(inspect.signature(_lib.Context.eslice_run).parameters)
    assert params[1:6] == ["key", "beta", "n_steps", "pos", "loglik"]
    for name in ("thin", "subiter_sum", "n_capped", "traj_pos", "traj_loglik", "key_mode"):
        assert name in params, name
    assert list(inspect.signature(_lib.Context.eslice_step).parameters)[1:] == ["key", "beta", "pos", "loglik", "subiter", "theta", "momentum"]
    assert list(inspect.signature(_lib.Context.eslice_step_keys).parameters)[1:] == ["keys", "beta", "pos", "loglik", "subiter", "theta", "momentum"]
    for name in ("set_lgcp_chol", "eslice_init"):
        assert hasattr(_lib.Context, name)
    src = open(os.path.join(ROOT, "mfm_amd", "csrc", "api.hip")).read()
    assert '#include "eslice.hip"' in src and os.path.exists(os.path.join(ROOT, "mfm_amd", "csrc", "eslice.hip"))


def test_cases_cover_every_instance_of_the_launcher():
    """mfm_eslice_launch_plan (host only): the instance of every case is the one its row of the table names; together the cases reach
    every instance the launcher can pick (dim = 1 .. 1664); the LDS of the largest fits a CU; a larger dim is refused."""
    from mfm_amd import _lib
    from tests import eslice_cases as ec
    for c in ec.CASES:
        tpw, sm = _lib.eslice_launch_plan(c.d)
        dp = (c.d + 15) // 16 * 16
        assert tpw == c.tpw, (c.name, tpw)
        assert sm == 16 * (dp + 4) * 4 + 2 * 8 * 16 * 8 and sm <= 160 * 1024, (c.name, sm)
        assert c.B % 16 == 0 and c.n_steps <= 20
    reachable = {_lib.eslice_launch_plan(d)[0] for d in range(1, 1665)}
    assert reachable == {c.tpw for c in ec.CASES} == {1, 2, 4, 8, 13}
    for d, tpw in ((128, 1), (129, 2), (256, 2), (257, 4), (512, 4), (513, 8), (1024, 8), (1025, 13), (1600, 13), (1664, 13)):      # the thresholds
        assert _lib.eslice_launch_plan(d)[0] == tpw, d
    for bad in (0, -3, 1665, 1700, 4096):
        with pytest.raises(_lib.MfmError, match="dim"):
            _lib.eslice_launch_plan(bad)


class _NoPrior:
    has_prior = False
    _engine = None

    def loglik(self, x):
        from mfm_amd.distributions import LogDensityExpr
        return LogDensityExpr(self, 1.0, 0.0)


def test_python_refusals_name_their_reason():
    from mfm_amd.bblackjax.mcmc import elliptical_slice as ES
    from mfm_amd.distributions import LogGaussianCoxPines, PhiFour
    dist = LogGaussianCoxPines(16)
    assert ES.resolve_loglikelihood(dist.loglik) == (dist, 1.0)
    assert ES.resolve_loglikelihood(lambda x: 0.25 * dist.loglik(x)) == (dist, 0.25)
    with pytest.raises(NotImplementedError, match="prior with coefficient 1"):
        ES.elliptical_slice(dist.logprob)
    with pytest.raises(NotImplementedError, match="prior with coefficient 0.5"):
        ES.elliptical_slice(lambda x: dist.loglik(x) + 0.5 * dist.logprior(x))
    with pytest.raises(NotImplementedError, match="PhiFour has none"):
        ES.elliptical_slice(PhiFour(16).loglik)
    with pytest.raises(NotImplementedError, match="_NoPrior has none"):
        ES.elliptical_slice(_NoPrior().loglik)
    with pytest.raises(NotImplementedError, match="must be built from dist.loglik"):
        ES.elliptical_slice(lambda x: 1.0)
    for kw in (dict(mean=np.zeros(16)), dict(cov=np.eye(16)), dict(mean=0.0, cov=1.0)):
        with pytest.raises(NotImplementedError, match="mean and cov must stay None"):
            ES.elliptical_slice(dist.loglik, **kw)
    algo = ES.elliptical_slice(dist.loglik)                    # no device work yet: the distribution is not attached
    assert callable(algo.init) and callable(algo.step) and callable(algo.step.run)
    with pytest.raises(RuntimeError, match="attach the distribution"):
        algo.init(np.zeros((16, 16), dtype=np.float32))
    assert ES.EllipSliceState(1, 2) == (1, 2, None) and ES.EllipSliceInfo._fields == ("momentum", "theta", "subiter")
    assert ES.EllipSliceRunInfo._fields[:5] == ("mean_subiter", "num_capped", "positions", "logdensities", "last")


def _args(*flags):
    from mfm_amd import multi_modal as M
    return M.build_parser().parse_args(["--seed", "1", *flags])


def test_check_eslice_args():
    from mfm_amd import exe_others as E
    a = _args("--do_eslice", "--example", "pines", "--num_chain", "64")
    assert a.do_eslice and E.check_eslice_args(a) == 64
    assert not _args().do_eslice
    for flags, msg in ((["--example", "phi-four"], "needs --example pines"), (["--example", "4-mode"], "needs --example pines"),
                       (["--do_smc"], "runs alone"), (["--do_svgd"], "runs alone"), (["--do_pt"], "runs alone"),
                       (["--num_chain", "40"], "multiple of 16"), (["--num_chain", "8"], "multiple of 16")):
        with pytest.raises(ValueError, match=msg):
            E.check_eslice_args(_args("--do_eslice", *flags))


def test_main_refuses_before_any_device_work():
    """``main`` overrides num_chain per example (pines: 128); ``--force_num_chain`` is what reaches the check."""
    from mfm_amd import multi_modal as M
    with pytest.raises(ValueError, match="needs --example pines"):
        M.main(_args("--do_eslice", "--example", "4-mode"))
    with pytest.raises(ValueError, match="multiple of 16"):
        M.main(_args("--do_eslice", "--example", "pines", "--force_dim", "16", "--force_num_chain", "24"))
    with pytest.raises(ValueError, match="runs alone"):
        M.main(_args("--do_eslice", "--do_pt", "--example", "pines", "--force_dim", "16"))
