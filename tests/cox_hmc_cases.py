"""The shared case table of the Cox process HMC tests (tests/test_cox_hmc_host.py on the CPU, tests/test_gpu_cox_hmc.py on the device),
on the grids, targets and starts of tests/eslice_cases.py.

    grid      d     tpw   B    beta      what it adds
    4 x 4     16    1     16   1         a single column tile, seven idle waves
    10 x 10   100   1     16   1         ragged: dp = 112, masked columns
    16 x 16   256   2     48   1, 0.1    three tiles of 16 chains
    20 x 20   400   4     16   1         synthetic counts
    32 x 32   1024  8     32   1         the largest instance
(The 40 x 40 grid, tpw 13, is not served: DESIGN.md section 4.20.)

``L`` leapfrog steps (3 .. 8) per HMC step, at most 6 HMC steps per case.  Every step size was chosen on the CPU with the oracle
(oracle/hmc.py on targets.Tempered(dist, beta)) so that the case's mean acceptance probability lies in [0.4, 0.95], and the seeds so
that at most 10 % of a case's chains have ``|u - pa| < 1e-3`` at any step: those are the chains a float32 kernel may legitimately
decide the other way (tests/test_cox_hmc_host.py asserts both)."""
import functools
from collections import namedtuple

import numpy as np

from oracle import hmc, mala, prng, targets
from tests.eslice_cases import dist_of

Case = namedtuple("Case", "name n d tpw B beta n_steps L eps seed")

CASES = (
    Case("4x4", 4, 16, 1, 16, 1.0, 6, 8, 0.15, 1),
    Case("10x10", 10, 100, 1, 16, 1.0, 6, 5, 0.36, 1),
    Case("16x16", 16, 256, 2, 48, 1.0, 5, 4, 0.4, 1),
    Case("16x16-b0.1", 16, 256, 2, 48, 0.1, 5, 6, 0.48, 2),
    Case("20x20", 20, 400, 4, 16, 1.0, 4, 3, 0.48, 1),
    Case("32x32", 32, 1024, 8, 32, 1.0, 3, 3, 0.48, 1),
)
BY_NAME = {c.name: c for c in CASES}
ACC_BAND = (0.4, 0.95)   # of a case's mean acceptance probability
MARGIN = 1e-3            # |u - pa| of the CPU share test
MAX_SHARE = 0.10         # of a case's chains

# MEASURED on an MI355X (tests/test_gpu_cox_hmc.py::test_step_matches_oracle prints the observed figures before it asserts), over every
# case and step, the oracle restarted from the device's float32 state after each step:
#   log_pa:   the largest |log pa (device) - log pa (oracle)| / max(1, max |logp|): the error of the exponent H_0 - H_end relative to
#             the energies' size (the existing HMC test's form, 5e-6 max|logp|);
#   position: the largest |device position - oracle position| / max(1, max |x|) over the accepted rows;
#   logp:     the largest |device logp - oracle logp| / max(1, max |logp|) over the accepted rows.
# The tolerances are 8 x the observed maxima.  By derivation the exponent's error is of the order of the existing HMC test's
# 5e-6 max|logp| and the position's a few float32 ulps (6e-8 relative each); the observed figures lie below both.
# Observed per case (log_pa | position | logp):
#   4x4 3.5e-7 | 1.6e-7 | 4.6e-8, 10x10 2.7e-7 | 2.6e-7 | 6.9e-8, 16x16 3.5e-7 | 1.6e-7 | 2.6e-7, 16x16 beta 0.1 8.3e-8 | 2.4e-7 | 7.1e-8,
#   20x20 1.2e-7 | 1.8e-7 | 5.8e-8, 32x32 1.4e-7 | 2.3e-7 | 1.0e-7.
OBSERVED = {"log_pa": 3.4904e-07, "position": 2.5759e-07, "logp": 2.5910e-07}
TOLERANCE = {k: 8 * v for k, v in OBSERVED.items()}      # 2.79e-6, 2.06e-6, 2.07e-6


def key_of(case, step):
    return prng.PRNGKey(8200 + 31 * case.seed + case.n + 1000 * step)


@functools.lru_cache(maxsize=None)
def start_of(name):
    """The case's start: prior draws ``mu + L xi`` as float32 rows (eslice_cases.start_of's, at this table's seeds)."""
    c = BY_NAME[name]
    dist = dist_of(c.n)
    xi = prng.normal_rows(prng.split(prng.PRNGKey(600 + c.seed), c.B), c.d)
    x = (dist.mu + xi @ dist.chol.T).astype(np.float32)
    x.setflags(write=False)
    return x


def value_and_grad_of(case):
    return targets.Tempered(dist_of(case.n), case.beta).value_and_grad


@functools.lru_cache(maxsize=None)
def reference_of(name):
    """The oracle's own run of the case (its decisions, float64 throughout), once: per step ``(HMCInfo, u)``; step j on
    ``split(key_of(case, j), B)``."""
    c = BY_NAME[name]
    vg = value_and_grad_of(c)
    x0 = start_of(name).astype(np.float64)
    lp, g = vg(x0)
    st = mala.MALAState(x0, lp, g)
    out = []
    for j in range(c.n_steps):
        st, info, u = hmc.kernel(prng.split(key_of(c, j), c.B), st, vg, c.eps, c.L)
        out.append((info, u))
    return tuple(out)
