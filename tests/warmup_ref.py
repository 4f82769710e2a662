"""The step-size warmup (``mfm_hmc_warmup`` / ``mfm_mala_warmup``, mfm_amd/csrc/warmup.hip) restated in float64 numpy: the dual-averaging
recursion of include/mfm.h around the oracle's HMC and MALA steps.  A helper of tests/test_warmup_host.py and tests/test_gpu_warmup.py,
not a test.

``DualAveraging`` is the recursion alone, fed with acceptance probabilities from anywhere (the GPU tests feed it the device's).
``hmc_warmup`` / ``mala_warmup`` close the loop around ``oracle.hmc.kernel`` / ``oracle.mala.kernel`` with the step-major key schedule
of the device (step j of chain b: ``split(split(key, n_steps)[j], n_chain)[b]``).  ``oracle.hmc.kernel`` takes a ``[B, 1]`` step size by
broadcasting; ``oracle.mala.kernel``'s transition energy does not (its ``[B, 1] * [B]`` product would be ``[B, B]``), so the MALA step
is called one chain at a time."""
import numpy as np

from oracle import hmc as ohmc, mala as omala, prng

T0, GAMMA = 10.0, 0.05          # Hoffman & Gelman's constants; kappa = 0.75 is the two square roots of ``eta``
CLAMP = 23.0


class DualAveraging:
    """Per chain: ``x_0 = log step0``, ``Hbar_0 = xbar_0 = 0``; ``update(p)`` takes the acceptance probabilities ``[B]`` of step m and
    returns the step sizes ``exp(x_m)`` of step m + 1.  ``step`` is the size the NEXT step uses (``step0`` itself before any update)."""

    def __init__(self, step0, target, n_chain):
        self.step0, self.target, self.m = float(step0), float(target), 0
        self.mu, self.x0 = np.log(10.0 * self.step0), np.log(self.step0)
        self.hbar, self.xbar = np.zeros(n_chain), np.zeros(n_chain)
        self.step = np.full(n_chain, self.step0)

    def update(self, p):
        self.m += 1
        mt = self.m + T0
        self.hbar = (1.0 - 1.0 / mt) * self.hbar + (self.target - np.asarray(p, dtype=np.float64)) / mt
        rm = np.sqrt(float(self.m))
        x = np.clip(self.mu - rm / GAMMA * self.hbar, self.x0 - CLAMP, self.x0 + CLAMP)
        eta = 1.0 / (rm * np.sqrt(rm))
        self.xbar = eta * x + (1.0 - eta) * self.xbar
        self.step = np.exp(x)
        return self.step

    @property
    def averaged(self):
        return np.exp(self.xbar)


def replay(p, step0, target):
    """The recursion fed with given acceptance probabilities ``p [n_steps, B]``: the step size used at every step ``[n_steps, B]``, the
    last iterate and the averaged step size."""
    da = DualAveraging(step0, target, p.shape[1])
    traj = []
    for row in p:
        traj.append(da.step.copy())
        da.update(row)
    return np.stack(traj), da.step, da.averaged


def pooled(step_avg):
    """``exp(mean(log step_avg))`` and the mean of the logs."""
    m = np.log(step_avg).mean()
    return np.exp(m), m


def _warmup(one_step, key, state, step0, n_steps, target):
    n = state.position.shape[0]
    da = DualAveraging(step0, target, n)
    step_keys = prng.split(key, n_steps)
    traj, acc = [], []
    for j in range(n_steps):
        traj.append(da.step.copy())
        state, p = one_step(prng.split(step_keys[j], n), state, da.step)
        acc.append(p)
        da.update(p)
    return dict(state=state, step_avg=da.averaged, step_last=da.step, step_traj=np.stack(traj), acc=np.stack(acc))


def hmc_warmup(key, state, value_and_grad, step0, num_integration_steps, n_steps, target=0.8):
    def one_step(keys, st, step):
        st, info, _ = ohmc.kernel(keys, st, value_and_grad, step[:, None], num_integration_steps)
        return st, info.acceptance_rate
    return _warmup(one_step, key, state, step0, n_steps, target)


def mala_warmup(key, state, value_and_grad, step0, n_steps, target=0.574):
    def one_step(keys, st, step):
        rows, p = [], []
        for b in range(len(step)):
            sb, info, _ = omala.kernel(keys[b:b + 1], omala.MALAState(*(a[b:b + 1] for a in st)), value_and_grad, float(step[b]), textbook=True)
            rows.append(sb); p.append(info.acceptance_rate[0])
        return omala.MALAState(*(np.concatenate(parts) for parts in zip(*rows))), np.array(p)
    return _warmup(one_step, key, state, step0, n_steps, target)


def phi4_start(d=64, n_chain=16):
    """The phi-four target of the warmup tests and its initial chains as the device holds them (float32 positions; log-density and
    gradient of the oracle at them): ``(dist, value_and_grad, state)``."""
    from oracle import targets
    from tests import gpu_util as gu
    args, dist, k, model, _ = gu.phi4_setup(d=d, B=n_chain, hidden=32, F=16)
    vg = targets.Tempered(dist, 1.0).value_and_grad
    return dist, vg, omala.init(dist.init_params.astype(np.float32).astype(np.float64), vg)
