"""CPU tests of ``mfm_amd.mcmc_utils.inference_loop0`` (reference ``mcmc_utils.py:19-25``) on a plain numpy kernel: the host loop over
``split(rng, n_iter)`` and the stacking of states and infos.  No GPU, no library."""
from collections import namedtuple

import numpy as np
import pytest

from mfm_amd import mcmc_utils, random as jr

WalkState = namedtuple("WalkState", "position n_moves")
WalkInfo = namedtuple("WalkInfo", "increment key")


def _walk(key, state):
    """A deterministic random walk keyed by ``mfm_amd.random``: the increment is a pure function of the step's key."""
    inc = jr.normal(key, state.position.shape)
    return WalkState(state.position + inc, state.n_moves + 1), WalkInfo(inc, np.asarray(key))


def test_inference_loop0_loops_over_the_split_keys_and_stacks():
    rng, n_iter = jr.PRNGKey(11), 5
    init = WalkState(np.zeros((3, 2)), np.int64(0))
    calls = []

    def kernel(key, state):
        calls.append(np.asarray(key).copy())
        return _walk(key, state)

    states, info = mcmc_utils.inference_loop0(rng, init, kernel, n_iter)
    keys = jr.split(rng, n_iter)
    assert len(calls) == n_iter
    np.testing.assert_array_equal(np.stack(calls), keys)                      # step j is keyed split(rng, n_iter)[j]
    assert isinstance(states, WalkState) and isinstance(info, WalkInfo)
    assert states.position.shape == (n_iter, 3, 2) and states.n_moves.shape == (n_iter,)
    assert info.increment.shape == (n_iter, 3, 2) and info.key.shape == (n_iter, 2)
    np.testing.assert_array_equal(info.key, keys)
    np.testing.assert_array_equal(states.n_moves, np.arange(1, n_iter + 1))
    incs = np.stack([jr.normal(keys[j], (3, 2)) for j in range(n_iter)])
    np.testing.assert_array_equal(info.increment, incs)
    pos = np.zeros((3, 2))
    for j in range(n_iter):                                                   # states[j] is the state AFTER step j
        pos = pos + incs[j]
        np.testing.assert_array_equal(states.position[j], pos)
    assert init.position.sum() == 0                                           # the initial state is not modified


def test_inference_loop0_stacks_plain_tuples_dicts_and_none():
    def kernel(key, state):
        x = state[0] + 1.0
        return (x, None), {"k0": np.uint32(key[0]), "pair": (x, x * 2)}

    states, info = mcmc_utils.inference_loop0(jr.PRNGKey(0), (np.zeros(4), None), kernel, 3)
    assert isinstance(states, tuple) and states[1] is None
    np.testing.assert_array_equal(states[0], np.array([1.0, 2.0, 3.0])[:, None] * np.ones(4))
    np.testing.assert_array_equal(info["k0"], jr.split(jr.PRNGKey(0), 3)[:, 0])
    assert info["pair"][1].shape == (3, 4)
    with pytest.raises(ValueError, match="n_iter"):
        mcmc_utils.inference_loop0(jr.PRNGKey(0), (np.zeros(4), None), kernel, 0)


def test_inference_loop0_hands_a_kernel_with_run_the_whole_scan():
    """A kernel that carries ``.run`` is called ONCE with the un-split key, ``n_iter`` and ``thin = 1`` (``mfm_mala_run`` on the device)."""
    from mfm_amd.bblackjax.mcmc.mala import MALAInfo, MALARunInfo, MALAState
    seen = []

    def step(key, state):
        raise AssertionError("the per-step kernel must not be called")

    def run(rng_key, state, num_steps, thin=0):
        seen.append((np.asarray(rng_key).copy(), num_steps, thin))
        traj = np.arange(num_steps, dtype=np.float32)[:, None, None] + state.position[None]
        return MALAState(traj[-1], state.logdensity, state.logdensity_grad), MALARunInfo(
            np.full(2, 0.5), np.full(2, 3), MALAInfo(None, None, None, None), traj, traj.sum(-1).astype(np.float64))

    step.run = run
    init = MALAState(np.zeros((2, 3), np.float32), np.zeros(2), np.zeros((2, 3), np.float32))
    states, info = mcmc_utils.inference_loop0(jr.PRNGKey(4), init, step, 6)
    assert len(seen) == 1 and seen[0][1:] == (6, 1)
    np.testing.assert_array_equal(seen[0][0], jr.PRNGKey(4))
    assert isinstance(states, MALAState) and states.position.shape == (6, 2, 3) and states.logdensity.shape == (6, 2)
    assert states.logdensity_grad is None and isinstance(info, MALARunInfo)
