"""CPU tests of the pieces around the autocorrelation kernel: ``mcmc_utils.inference_loop``, the ``--ess_steps`` flag and the constants
the binding mirrors from include/mfm.h."""
import os
import re
from typing import NamedTuple

import numpy as np

from mfm_amd import mcmc_utils, random as jr


class State(NamedTuple):
    position: np.ndarray
    count: int


def _kernel0(key, state):
    step = jr.normal(key, state.position.shape)
    return State(state.position + step, state.count + 1), {"step": step, "key": np.asarray(key)}


def _kernel(key, state, param):
    new, info = _kernel0(key, state)
    return State(new.position * param["scale"], new.count), dict(info, seen=param["scale"])


def test_inference_loop_stacks_like_inference_loop0_and_passes_param():
    key, init = jr.PRNGKey(4), State(np.zeros(3), 0)
    states0, infos0 = mcmc_utils.inference_loop0(key, init, _kernel0, 5)
    states, infos = mcmc_utils.inference_loop(key, init, _kernel, 5, {"scale": 1.0})
    assert isinstance(states, State) and states.position.shape == (5, 3)
    np.testing.assert_array_equal(states.position, states0.position)          # scale 1: the same chain from the same keys
    np.testing.assert_array_equal(states.count, np.arange(1, 6))
    np.testing.assert_array_equal(infos["key"], np.asarray(jr.split(key, 5)))
    np.testing.assert_array_equal(infos["step"], infos0["step"])
    np.testing.assert_array_equal(infos["seen"], np.ones(5))
    halved, infos_h = mcmc_utils.inference_loop(key, init, _kernel, 5, {"scale": 0.5})
    np.testing.assert_array_equal(infos_h["seen"], np.full(5, 0.5))           # the same param at every step
    np.testing.assert_allclose(halved.position[0], states.position[0] * 0.5)
    assert not np.allclose(halved.position[-1], states.position[-1])


def test_inference_loop_rejects_an_empty_scan():
    import pytest
    with pytest.raises(ValueError, match="n_iter"):
        mcmc_utils.inference_loop(jr.PRNGKey(0), State(np.zeros(1), 0), _kernel, 0, {"scale": 1.0})


def test_module_exports():
    assert set(mcmc_utils.__all__) == {"inference_loop", "inference_loop0", "autocorrelation", "effective_sample_size"}
    for name in mcmc_utils.__all__:
        assert callable(getattr(mcmc_utils, name))


def test_parser_takes_ess_steps_and_still_resolves_hutch():
    from mfm_amd.multi_modal import build_parser
    p = build_parser()
    assert p.parse_args([]).ess_steps == 0
    assert p.parse_args(["--ess_steps", "256"]).ess_steps == 256
    a = p.parse_args(["--hutch", "--example", "4-mode", "--ess_steps", "8"])   # --hutch: the unambiguous prefix of --hutchs
    assert a.hutchs is True and a.ess_steps == 8 and a.example == "4-mode"


def test_binding_mirrors_the_kernel_constants_and_exports_the_entry():
    from mfm_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mfm.h")).read()
    consts = dict(re.findall(r"#define MFM_AUTOCORR_(\w+) (\d+)", header))
    assert int(consts["LAG_BLOCK"]) == _lib.AUTOCORR_LAG_BLOCK and int(consts["TIME_BLOCK"]) == _lib.AUTOCORR_TIME_BLOCK
    assert _lib.AUTOCORR_LAG_BLOCK % 2 == 0 and _lib.AUTOCORR_TIME_BLOCK % _lib.AUTOCORR_LAG_BLOCK == 0
    assert "mfm_autocorr" in _lib.EXPORTS and "int mfm_autocorr(" in header
    assert callable(_lib.Context.autocorr)
