"""CPU tests around the step-size warmup (``mfm_hmc_warmup`` / ``mfm_mala_warmup``): the float64 restatement of the recursion
(tests/warmup_ref.py) finds one step size from starts 100 times apart, ``mcmc_utils.pooled_step_size`` on CPU tensors, and the two
command-line flags.  The device side: tests/test_gpu_warmup.py."""
import numpy as np
import pytest

from oracle import prng
from tests import warmup_ref as wr


def test_restatement_finds_one_step_size_from_starts_a_hundred_times_apart():
    """phi-four d = 64, 16 chains, L = 3, target 0.8, 40 steps, from 0.003 (100 times too small) and from 0.3 (beyond velocity Verlet's
    stability limit): the pooled step sizes agree within 10 % and the mean acceptance probability over the last 10 steps lies in
    [0.7, 0.9]."""
    _, vg, state = wr.phi4_start(64, 16)
    out = {s0: wr.hmc_warmup(prng.PRNGKey(5), state, vg, s0, 3, 40, 0.8) for s0 in (0.003, 0.3)}
    pooled = {s0: wr.pooled(o["step_avg"])[0] for s0, o in out.items()}
    tail = {s0: o["acc"][-10:].mean() for s0, o in out.items()}
    print(f"pooled step sizes {pooled}, mean acceptance over the last 10 steps {tail}")
    assert abs(pooled[0.003] - pooled[0.3]) < 0.1 * min(pooled.values())
    for s0 in out:
        assert 0.7 <= tail[s0] <= 0.9, (s0, tail[s0])
        np.testing.assert_array_equal(out[s0]["step_traj"][0], s0)             # the first step runs at the caller's value itself
        assert np.isfinite(out[s0]["step_avg"]).all() and (out[s0]["step_avg"] > 0).all()


def test_recursion_replay_equals_the_closed_loop():
    """``replay`` on the closed loop's own acceptance probabilities gives the closed loop's step sizes: the GPU tests feed it the
    device's.  (From the common start every chain accepts, then overshoots: the chains part at the tenth step.)"""
    _, vg, state = wr.phi4_start(64, 16)
    o = wr.hmc_warmup(prng.PRNGKey(5), state, vg, 0.02, 3, 12, 0.8)
    traj, last, avg = wr.replay(o["acc"], 0.02, 0.8)
    np.testing.assert_array_equal(traj, o["step_traj"])
    np.testing.assert_array_equal(last, o["step_last"])
    np.testing.assert_array_equal(avg, o["step_avg"])
    assert max(len(np.unique(row)) for row in o["step_traj"][1:]) > 1          # the chains part: the adaptation is per chain


def test_mala_restatement_steers_to_its_target():
    """The MALA step under the textbook rule, one chain at a time: phi-four d = 64, 16 chains, 40 steps towards 0.574 from a step 10
    times too small; the tail acceptance comes down from ~1 towards the target."""
    _, vg, state = wr.phi4_start(64, 16)
    o = wr.mala_warmup(prng.PRNGKey(5), state, vg, 1e-4, 40, 0.574)
    tail = o["acc"][-10:].mean()
    print(f"pooled step size {wr.pooled(o['step_avg'])[0]:.4g}, mean acceptance over the last 10 steps {tail:.3f}, over the first 3 {o['acc'][:3].mean():.3f}")
    assert 0.4 <= tail <= 0.75, tail
    assert wr.pooled(o["step_avg"])[0] > 1e-4


def test_pooled_step_size_on_cpu_tensors_leaves_padding_rows_out():
    import torch
    from mfm_amd import mcmc_utils
    steps = torch.tensor([0.01, 0.04, 0.02, 7.0, 7.0], dtype=torch.float64)     # 3 chains, 2 padding rows
    want = float(np.exp(np.log([0.01, 0.04, 0.02]).mean()))
    assert mcmc_utils.pooled_step_size(steps, 3) == pytest.approx(want, rel=1e-15)
    assert mcmc_utils.pooled_step_size(steps[:3]) == pytest.approx(want, rel=1e-15)
    assert mcmc_utils.pooled_step_size(steps) > want                           # (the padding rows would have counted)


def test_parser_takes_the_flags_and_mala_refuses_adaptation():
    from mfm_amd import exe_flow_matching as E, multi_modal
    p = multi_modal.build_parser()
    a = p.parse_args([])
    assert a.adapt_steps == 0 and a.adapt_target == 0.8
    a = p.parse_args(["--adapt_steps", "5", "--adapt_target", "0.65", "--mcmc_kernel", "hmc"])
    assert a.adapt_steps == 5 and a.adapt_target == 0.65 and a.warmup_steps == 0
    assert E.check_adapt_args(a) == 5
    a = p.parse_args(["--adapt_steps", "5", "--example", "phi-four"])           # the default kernel: MALA
    with pytest.raises(ValueError, match="as written|AS WRITTEN"):
        E.run(None, a)                                                         # raises before it touches the target or a device
    a = p.parse_args(["--adapt_steps", "5", "--mcmc_kernel", "hmc", "--mcmc_per_flow_steps", "-1"])     # exact samples: no MCMC step to adapt
    with pytest.raises(ValueError, match="mcmc_per_flow_steps"):
        E.check_adapt_args(a)
    assert E.check_adapt_args(p.parse_args(["--mcmc_per_flow_steps", "-1"])) == 0
