"""CPU tests of the NUTS warmup's host side: the float64 restatement (tests/nuts_warmup_ref.py) against ``nuts_ref.kernel`` and
``warmup_ref.replay``, and the surface of ``mfm_nuts_warmup`` / ``mfm_nuts_warmup_window`` -- header, ctypes table, ``Context``, the
Python kernel, ``nuts_window_adaptation`` and ``--nuts_adapt``."""
import inspect
import os
import re

import numpy as np
import pytest

from oracle import prng
from tests import nuts_ref as nr, nuts_warmup_ref as nw, warmup_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, DEPTH = 16, 6


def test_one_common_step_size_gives_the_kernel_bit_for_bit():
    """Per-chain step sizes that are all equal, and two groups of chains at two step sizes against the kernel on each group."""
    _, vg, state = wr.phi4_start(64, B)
    keys = prng.split(prng.PRNGKey(3), B)
    st, info = nw.transition(keys, state, vg, np.full(B, 0.03), DEPTH)
    st_k, info_k = nr.kernel(keys, state, vg, 0.03, DEPTH)
    for a, b in zip(st, st_k):
        np.testing.assert_array_equal(a, b)
    for k in nw.INFO:
        np.testing.assert_array_equal(info[k], getattr(info_k, k), err_msg=k)
    assert len(set(info["depth"].tolist())) > 1
    step = np.where(np.arange(B) % 2 == 0, 0.03, 0.01)
    st2, info2 = nw.transition(keys, state, vg, step, DEPTH)
    st_b, info_b = nr.kernel(keys, state, vg, 0.01, DEPTH)                     # the whole batch at the other step size: rows do not interact
    even = step == 0.03
    np.testing.assert_array_equal(st2.position[even], st_k.position[even])
    np.testing.assert_array_equal(st2.position[~even], st_b.position[~even])
    np.testing.assert_array_equal(info2["acceptance_rate"][~even], info_b.acceptance_rate[~even])
    np.testing.assert_array_equal(info2["num_leapfrog"][even], info_k.num_leapfrog[even])


def test_closed_loop_equals_the_recursion_on_its_recorded_statistics():
    """The restatement fed back its own acceptance statistics is ``warmup_ref.replay``; the first transition runs at ``step0`` itself;
    the chains' step sizes part and the trees reach different depths (what the GPU cases rely on)."""
    _, vg, state = wr.phi4_start(64, B)
    out = nw.nuts_warmup(prng.PRNGKey(21), state, vg, 0.03, 8, 0.8, DEPTH)
    traj, last, avg = wr.replay(out["acc"], 0.03, 0.8)
    np.testing.assert_array_equal(out["step_traj"], traj)
    np.testing.assert_array_equal(out["step_last"], last)
    np.testing.assert_array_equal(out["step_avg"], avg)
    np.testing.assert_array_equal(out["step_traj"][0], 0.03)
    assert out["acc"].shape == out["depth"].shape == out["num_leapfrog"].shape == (8, B) and out["positions"].shape == (8, B, 64)
    assert ((out["acc"] >= 0) & (out["acc"] <= 1)).all()
    assert max(len(np.unique(r)) for r in out["step_traj"][1:]) >= 2
    assert len(np.unique(out["depth"])) >= 3
    np.testing.assert_array_equal(out["positions"][-1], out["state"].position)
    # the step-major key schedule: the first transition is the kernel on split(split(key, n)[0], B)
    st0, info0 = nr.kernel(prng.split(prng.split(prng.PRNGKey(21), 8)[0], B), state, vg, 0.03, DEPTH)
    np.testing.assert_array_equal(out["positions"][0], st0.position)
    np.testing.assert_array_equal(out["acc"][0], info0.acceptance_rate)


def test_c_abi_surface():
    from mfm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mfm.h")).read()
    for name, nargs in (("mfm_nuts_warmup", 21), ("mfm_nuts_warmup_window", 23)):
        assert name in _lib.EXPORTS and len(_lib._SIGS[name][1]) == nargs
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == nargs, name
    for m, lead in (("nuts_warmup", "step_avg"), ("nuts_warmup_window", "pos_sumsq")):
        params = list(inspect.signature(getattr(_lib.Context, m)).parameters)
        assert params[1:10] == ["key", "beta", "step0", "max_tree_depth", "n_steps", "target_accept", "pos", "logp", "grad"] and lead in params
        for opt in ("divergence_threshold", "step_last", "acc_sum", "step_traj", "leapfrog_sum", "n_divergent", "depth_sum", "key_mode"):
            assert opt in params, (m, opt)
    assert "d_n_accepted" not in re.search(r"int mfm_nuts_warmup\(([^;]*)\);", hdr).group(1)      # a transition has no accept / reject


def test_python_surface():
    from mfm_amd.bblackjax.adaptation import window_adaptation as W
    from mfm_amd.bblackjax.mcmc import nuts as N
    assert N.NUTSWarmupInfo._fields == ("step_size", "pooled_step_size", "acceptance_rate", "num_integration_steps", "num_divergent", "mean_depth",
                                        "step_sizes")
    assert "NUTSWarmupInfo" in N.__all__ and callable(N.build_kernel().warmup)
    sig = inspect.signature(N.build_kernel().warmup)
    assert sig.parameters["target_acceptance_rate"].default == 0.8 and sig.parameters["return_step_sizes"].default is False
    assert list(sig.parameters)[:5] == ["rng_key", "state", "logdensity_fn", "step_size", "num_steps"]
    sig = inspect.signature(W.nuts_window_adaptation.__init__)
    assert list(sig.parameters)[1:] == ["logdensity_fn", "max_num_doublings", "initial_step_size", "target_acceptance_rate", "divergence_threshold"]
    assert sig.parameters["target_acceptance_rate"].default == 0.8 and sig.parameters["divergence_threshold"].default == 1000
    assert {"nuts_window_adaptation", "window_adaptation"} <= set(W.__all__)
    # window_adaptation's signature and info stay as they are
    assert list(inspect.signature(W.window_adaptation.__init__).parameters)[1:] == ["logdensity_fn", "num_integration_steps", "initial_step_size",
                                                                                   "target_acceptance_rate"]
    assert W.WindowAdaptationInfo._fields == ("schedule", "step_sizes", "acceptance_rates", "inverse_mass_matrices")
    assert W.NUTSWindowAdaptationInfo._fields == W.WindowAdaptationInfo._fields + ("mean_integration_steps",)


def test_nuts_window_adaptation_uses_window_schedule_unchanged(monkeypatch):
    """Both classes go through the one segment loop, which asks ``window_schedule`` for the segments: a schedule planted there is the
    one both walk, and a key that is not ONE key is refused before anything else."""
    from mfm_amd.bblackjax.adaptation import window_adaptation as W
    seen = []

    class Stop(Exception):
        pass

    def planted(num_steps):
        seen.append(num_steps)
        raise Stop
    monkeypatch.setattr(W, "window_schedule", planted)
    from mfm_amd.distributions import PhiFour
    dist = PhiFour(64)
    for wa in (W.nuts_window_adaptation(dist.logprob, 6, 0.03), W.window_adaptation(dist.logprob, 4, 0.03)):
        with pytest.raises(Stop):
            wa.run(prng.PRNGKey(1), None, 100)
        with pytest.raises(ValueError, match="ONE key"):
            wa.run(prng.split(prng.PRNGKey(1), 4), None, 100)
    assert seen == [100, 100]
    src = inspect.getsource(W.nuts_window_adaptation)
    assert "_run_segments" in src and "_run_segments" in inspect.getsource(W.window_adaptation)


def test_command_line_flag_and_its_check():
    from mfm_amd import exe_flow_matching as E
    from mfm_amd.multi_modal import build_parser
    from oracle import loop
    a = build_parser().parse_args([])
    assert a.nuts_adapt == "hmc"
    a = build_parser().parse_args(["--mcmc_kernel", "nuts", "--adapt_steps", "30", "--nuts_adapt", "tree"])
    assert (a.nuts_adapt, a.adapt_steps) == ("tree", 30)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--nuts_adapt", "leaf"])
    flags = [o for act in build_parser()._actions for o in act.option_strings]
    assert "--nuts_adapt" in flags and not [f for f in flags if f != "--nuts_adapt" and (f.startswith("--nuts_adapt") or "--nuts_adapt".startswith(f))]
    assert E.check_adapt_args(loop.default_args(mcmc_kernel="nuts", adapt_steps=5, nuts_adapt="tree")) == 5
    assert E.check_adapt_args(loop.default_args(mcmc_kernel="nuts", adapt_steps=5)) == 5            # the default: today's HMC warmup
    assert E.check_adapt_args(loop.default_args(mcmc_kernel="hmc", adapt_steps=5, nuts_adapt="hmc")) == 5
    for kernel in ("hmc", "mala"):
        with pytest.raises(ValueError, match="--nuts_adapt tree"):
            E.check_adapt_args(loop.default_args(mcmc_kernel=kernel, adapt_steps=0, nuts_adapt="tree"))
    with pytest.raises(ValueError, match="--nuts_adapt tree"):
        E.check_adapt_args(loop.default_args(mcmc_kernel="hmc", adapt_steps=5, nuts_adapt="tree"))
