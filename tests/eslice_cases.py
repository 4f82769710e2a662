"""The shared case table of the elliptical slice tests (tests/test_eslice_ref.py on the CPU, tests/test_gpu_eslice.py on the device).

    grid      d     tpw   B    beta      what it adds
    4 x 4     16    1     16   1         a single column tile, seven idle waves
    10 x 10   100   1     16   1         ragged: dp = 112, masked columns (counts binned from tests/golden/finpines.csv, as
                                         tests/test_gpu_lgcp_ragged.py builds its grids)
    16 x 16   256   2     48   1, 0.1    three tiles of 16 chains
    20 x 20   400   4     16   1         synthetic counts
    32 x 32   1024  8     32   1
    40 x 40   1600  13    16   1         the reference's default grid, 3 transitions

Every case has at most 20 transitions.  The seeds are chosen so that at most 10 % of a case's chains have a decision margin
``|beta ll(x') - log y|`` below 1e-3 anywhere in the run (tests/test_eslice_ref.py asserts it): those chains are the ones a float32
kernel may legitimately decide the other way, and the GPU tests leave out the chains whose margin is below the measured tolerance."""
import functools
from collections import namedtuple

import numpy as np

from oracle import prng, targets

Case = namedtuple("Case", "name n d tpw B beta n_steps seed")

CASES = (
    Case("4x4", 4, 16, 1, 16, 1.0, 20, 3),
    Case("10x10", 10, 100, 1, 16, 1.0, 20, 1),
    Case("16x16", 16, 256, 2, 48, 1.0, 10, 1),
    Case("16x16-b0.1", 16, 256, 2, 48, 0.1, 10, 2),
    Case("20x20", 20, 400, 4, 16, 1.0, 10, 1),
    Case("32x32", 32, 1024, 8, 32, 1.0, 6, 1),
    Case("40x40", 40, 1600, 13, 16, 1.0, 3, 1),
)
BY_NAME = {c.name: c for c in CASES}
MARGIN = 1e-3            # the margin of the CPU share test
MAX_SHARE = 0.10         # of a case's chains

# MEASURED on an MI355X over every case's end-to-end run (tests/test_gpu_eslice.py prints the observed figures before it asserts):
#   loglik:   the largest |device loglik - restatement loglik| over the accepted points of the chains that are compared;
#   position: the largest |device position - restatement position| over the same chains.
# The tolerances are 8 x the observed maxima.  By derivation delta should be of order 1e-4 or below (float32 expf and products,
# float64 sums, position error about 2.4e-7 per coordinate).
# Observed per case (run of the case | its first transition alone), every chain making the restatement's decisions:
#   4x4 3.7e-5 | 1.3e-5, 10x10 5.2e-5 | 1.9e-5, 16x16 3.3e-5 | 3.3e-5, 16x16 beta 0.1 3.4e-5 | 1.6e-5, 20x20 2.6e-5 | 1.3e-5, 32x32 3.4e-5 | 2.0e-5,
#   40x40 3.5e-5 | 1.2e-5; positions 1.9e-6 | 9.5e-7 (8 | 4 float32 ulps at |x| in [2, 4)) on every grid.
OBSERVED = {"loglik": 5.2395e-05, "position": 1.9073e-06}
TOLERANCE = {"loglik": 8 * 5.2395e-05, "position": 8 * 1.9073e-06}      # 4.19e-4 (below the 1e-3 of the CPU share test) and 1.53e-5


@functools.lru_cache(maxsize=None)
def dist_of(n):
    """The oracle's Cox process on the n x n grid: bundled counts where there are some, the binned point pattern on 10 x 10, Poisson
    counts of the same total intensity on 20 x 20."""
    import os
    d = n * n
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bundled = np.load(os.path.join(root, "mfm_amd", "data", "pines_counts.npz"))
    if n == 20:
        counts = np.random.default_rng(400).poisson(126.0 / d, d).astype(np.float64)
    elif f"counts_{n}" in bundled.files:
        counts = bundled[f"counts_{n}"]
    else:
        from mfm_amd.distributions import LogGaussianCoxPines
        counts = LogGaussianCoxPines(d, file_path=os.path.join(root, "tests", "golden", "finpines.csv")).counts
    return targets.LogGaussianCoxPines(d, counts)


def key_of(case):
    return prng.PRNGKey(7100 + 17 * case.seed + case.n)


@functools.lru_cache(maxsize=None)
def start_of(name):
    """The case's start: prior draws ``mu + L xi`` as float32 rows (distributions.py:313-314)."""
    c = BY_NAME[name]
    dist = dist_of(c.n)
    xi = prng.normal_rows(prng.split(prng.PRNGKey(500 + c.seed), c.B), c.d)
    x = (dist.mu + xi @ dist.chol.T).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference_of(name, key_mode=0):
    """The restatement's run of the case, computed once and shared: ``(x, ll, infos, traj_x, traj_ll)`` with ``thin = 1``."""
    from tests import eslice_ref as er
    c = BY_NAME[name]
    dist = dist_of(c.n)
    x0 = start_of(name).astype(np.float64)
    keys = prng.split(prng.PRNGKey(900 + c.seed), c.B) if key_mode else None
    return er.run(key_mode, key_of(c), keys, c.beta, c.n_steps, x0, er.loglik(dist, x0), dist, thin=1)
