"""The sampler kernels that share mcmc.hip.h (MALA stand-alone and by keys, the Cox process tile and wide pair with their init, HMC,
the Cox process run) against bits recorded on an MI355X from the commit BEFORE they were moved onto that header
(tools/make_mcmc_bits.py; cases and step sizes: tests/mcmc_bits_cases.py): `==` on the raw bytes of every buffer of three
consecutive steps -- through SHA-256 digests, and on the arrays the fixture keeps.  mala_run_kernel and the training kernel's fused
MALA are pinned to mfm_mala_step bit for bit by tests/test_gpu_mala_run.py and test_fused_mala_train_iter_equals_separate."""
import os

import numpy as np
import pytest

from tests import mcmc_bits_cases as C

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mcmc_bits_parent.npz")


@pytest.fixture(scope="module")
def golden():
    assert os.path.exists(FIXTURE), f"{FIXTURE} is missing: record it from the parent commit with tools/make_mcmc_bits.py"
    return C.unpack(np.load(FIXTURE))


@pytest.mark.parametrize("variant", list(C.VARIANTS))
@pytest.mark.parametrize("case", list(C.CASES))
def test_bits_equal_the_parent_commit(golden, case, variant):
    rec = C.record(case, variant)
    names = [n for n in rec if not n.endswith("/decisions")]
    digests, arrays = golden
    assert {f"{case}/{variant}/{n}" for n in names} == {k for k in digests if k.startswith(f"{case}/{variant}/")}
    bad = []
    for name in names:
        full = f"{case}/{variant}/{name}"
        dig, kept = C.stored(name, rec[name])
        if kept is not None:
            want = arrays[full]
            assert kept.dtype == want.dtype and kept.shape == want.shape, full
            if kept.tobytes() != want.tobytes():
                diff = kept.view(np.uint8).reshape(kept.shape[0], -1) != want.view(np.uint8).reshape(want.shape[0], -1)
                print(f"{full}: {int(diff.any(-1).sum())} of {kept.shape[0]} rows differ; first: got {kept[diff.any(-1)][0]!r} want {want[diff.any(-1)][0]!r}")
                bad.append(full)
        if dig != digests[full]:
            bad.append("sha256:" + full)
    assert not bad, bad
    for name, arr in rec.items():                                  # the shapes still exercise both branches of the accept
        if name.endswith("/decisions"):
            assert 0 < arr.sum() < arr.size, name
