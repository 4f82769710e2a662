"""Host-side binning of the pine-sapling point pattern (mfm_amd/distributions.py: LogGaussianCoxPines(dim, file_path=...)) on
tests/golden/finpines.csv: it reproduces every bundled grid bit for bit, serves the grids that are not bundled (the ones whose
cell count is no multiple of 16: tests/test_gpu_lgcp_ragged.py), and clamps a coordinate of exactly 1.0 into the last bin."""
import os

import numpy as np
import pytest

from mfm_amd.distributions import LogGaussianCoxPines

CSV = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "finpines.csv")
BUNDLED = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mfm_amd", "data", "pines_counts.npz")


def test_fixture_is_the_126_point_pattern():
    pts = np.genfromtxt(CSV, delimiter=",")
    assert pts.shape == (126, 2)
    assert pts.min() >= 0.0 and pts.max() <= 1.0


@pytest.mark.parametrize("n", [4, 8, 16, 32, 40])
def test_binning_the_fixture_equals_the_bundled_counts(n):
    z = np.load(BUNDLED)
    binned = LogGaussianCoxPines(n * n, file_path=CSV).counts
    bundled = LogGaussianCoxPines(n * n).counts
    assert binned.dtype == bundled.dtype == np.float64
    np.testing.assert_array_equal(binned, bundled)
    np.testing.assert_array_equal(binned, z[f"counts_{n}"].astype(np.float64).reshape(-1))


@pytest.mark.parametrize("n", [5, 7, 10, 18, 23, 30, 33])
def test_unbundled_grids_hold_every_point(n):
    with pytest.raises(FileNotFoundError, match="no bundled pine counts"):
        LogGaussianCoxPines(n * n)
    dist = LogGaussianCoxPines(n * n, file_path=CSV)
    assert dist.n == n and dist.dim == n * n and dist.counts.shape == (n * n,)
    assert dist.counts.sum() == 126 and (dist.counts >= 0).all() and (dist.counts == np.round(dist.counts)).all()
    # row-major cells: the marginal over columns is the histogram of the first coordinate
    pts = np.genfromtxt(CSV, delimiter=",")
    rows = np.minimum(np.floor(pts[:, 0] * n).astype(int), n - 1)
    np.testing.assert_array_equal(dist.counts.reshape(n, n).sum(1), np.bincount(rows, minlength=n))


def test_a_coordinate_of_exactly_one_lands_in_the_last_bin(tmp_path):
    path = tmp_path / "two_points.csv"
    path.write_text("1.0,0.25\n0.5,1.0\n")
    for n in (4, 5, 10):
        c = LogGaussianCoxPines(n * n, file_path=str(path)).counts.reshape(n, n)
        assert c.sum() == 2
        assert c[n - 1, int(0.25 * n)] == 1                      # r == n is clamped to n - 1
        assert c[int(0.5 * n), n - 1] == 1                       # c == n is clamped to n - 1


@pytest.mark.parametrize("n", [5, 10])
def test_target_block_layout(n):
    d = n * n
    dist = LogGaussianCoxPines(d, file_path=CSV)
    kind, blk = dist.target_block()
    assert kind == 2 and blk.shape == (3 + d + d * d,)
    assert blk[0] == dist.mu and blk[1] == 1.0 / d and blk[2] == dist.log_norm
    np.testing.assert_array_equal(blk[3:3 + d], dist.counts)
    Kinv = blk[3 + d:].reshape(d, d)
    np.testing.assert_array_equal(Kinv, Kinv.T)                  # symmetrised: exactly symmetric
    np.testing.assert_allclose(Kinv @ dist.gram, np.eye(d), atol=1e-9)
    # the oracle's target on the same counts packs the same block
    from oracle import targets
    o = targets.LogGaussianCoxPines(d, dist.counts)
    np.testing.assert_array_equal(o.Kinv, Kinv)
    assert (o.mu, o.poisson_a, o.log_norm) == (dist.mu, dist.poisson_a, dist.log_norm)
