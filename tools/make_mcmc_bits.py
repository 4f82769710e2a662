"""Record tests/golden/mcmc_bits_parent.npz: the bits of every sampler kernel that goes through mcmc.hip.h (tests/mcmc_bits_cases.py),
from a build of the commit BEFORE a change to that header or its call sites -- never from the commit under test.

    git worktree add /tmp/parent <parent commit> && (cd /tmp/parent && python -m mfm_amd.build)
    python tools/make_mcmc_bits.py /tmp/parent/mfm_amd/lib/libmfm_hip.so [--out tests/golden/mcmc_bits_parent.npz]

Needs the GPU.  Asserts that every case's recorded decisions hold both values (the step sizes come from the float64 oracle).
Per buffer `<case>/<variant>/<api>/<step>/<name>`: its SHA-256, and the array itself where tests/mcmc_bits_cases.py keeps it (`pack` there).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib", help="libmfm_hip.so of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mcmc_bits_parent.npz"))
    a = ap.parse_args()
    os.environ["MFM_LIB"] = os.path.abspath(a.lib)                 # read by mfm_amd._lib.load
    import numpy as np
    from tests import mcmc_bits_cases as C
    digests, kept_arrays = {}, {}
    for case in C.CASES:
        for variant in C.VARIANTS:
            rec = C.record(case, variant)
            for name, arr in rec.items():
                full = f"{case}/{variant}/{name}"
                if name.endswith("/decisions"):
                    assert 0 < arr.sum() < arr.size, (full, int(arr.sum()), arr.size)      # both branches of the accept
                    print(f"{full}: accepted {int(arr.sum())} of {arr.size}")
                    continue
                dig, kept = C.stored(name, arr)
                digests[full] = dig
                if kept is not None:
                    kept_arrays[full] = kept
    np.savez_compressed(a.out, **C.pack(digests, kept_arrays))
    print(f"{a.out}: {len(digests)} buffers, {len(kept_arrays)} kept as arrays, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
