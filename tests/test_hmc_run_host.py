"""CPU tests around ``mfm_hmc_run``: ``inference_loop0`` takes the one-call path for any kernel that carries ``.run`` and builds the stacked
state from the run info's ``positions`` / ``logdensities`` (``HMCRunInfo`` has ``MALARunInfo``'s fields, so there is no kernel-specific
branch); the HMC module's public names.  (tests/test_host_api.py compares the header with the ctypes table for every symbol.)"""
import numpy as np

from mfm_amd import mcmc_utils
from mfm_amd.bblackjax.mcmc import hmc as H, mala as M


def test_run_info_has_the_fields_of_the_mala_run_info():
    assert H.HMCRunInfo._fields == M.MALARunInfo._fields
    assert H.HMCInfo._fields == ("acceptance_rate", "is_accepted")             # unchanged
    assert H.HMCState is M.MALAState
    assert callable(H.build_kernel().run)
    assert {"HMCRunInfo", "HMCInfo", "HMCState", "hmc", "build_kernel", "init"} <= set(H.__all__)


def test_inference_loop0_takes_the_one_call_path_of_a_kernel_with_run():
    n_iter, n_chain, dim = 5, 3, 2
    calls = []

    def step(key, state):
        raise AssertionError("the host loop must not run for a kernel that carries .run")

    def run(key, state, num_steps, thin=0):
        calls.append((tuple(int(v) for v in key), num_steps, thin))
        pos = np.arange(num_steps * n_chain * dim, dtype=np.float32).reshape(num_steps, n_chain, dim)
        lps = -np.arange(num_steps * n_chain, dtype=np.float64).reshape(num_steps, n_chain)
        info = H.HMCRunInfo(np.full(n_chain, 0.5), np.full(n_chain, 2, np.int32), H.HMCInfo(np.ones(n_chain, np.float32), np.ones(n_chain, bool)),
                            pos, lps)
        return H.HMCState(pos[-1], lps[-1], np.zeros((n_chain, dim), np.float32)), info

    step.run = run
    init = H.HMCState(np.zeros((n_chain, dim), np.float32), np.zeros(n_chain), np.zeros((n_chain, dim), np.float32))
    states, info = mcmc_utils.inference_loop0(np.array([0, 9], dtype=np.uint32), init, step, n_iter)
    assert calls == [((0, 9), n_iter, 1)]                                      # ONE call, every step kept
    assert isinstance(states, H.HMCState) and isinstance(info, H.HMCRunInfo)
    assert states.position is info.positions and states.logdensity is info.logdensities and states.logdensity_grad is None
    assert states.position.shape == (n_iter, n_chain, dim)
