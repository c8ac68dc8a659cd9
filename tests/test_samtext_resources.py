"""CPU: register, scratch and LDS use of the SAM text kernels (dev_samtext.h), read from the code object's metadata (tools/isa_resources.py: hipcc -S, no GPU).
The formatter keeps no array in private memory -- digits are written in place, CIGAR records are read through their pointers -- so: no scratch, nothing
spilled, at most 128 VGPRs, and the one staging area of SAM_STAGE = 512 bytes per workgroup in the writing pass (the tree has 35 / 113 VGPRs).  A change that
gives a kernel a private buffer, or that spills, still passes every parity test."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# kernel (as tools/isa_resources.py prints it): (VGPRs at most, scratch bytes per lane at most, spilled VGPRs at most, LDS bytes exactly)
BOUNDS = {
    "k_sam_size": (128, 0, 0, 0),
    "k_sam_write": (128, 0, 0, 512),
    "k_primary_misses": (16, 0, 0, 0),
}


def test_samtext_kernels_do_not_spill():
    import isa_resources
    from bwa_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc is not installed")
    rows = {r[0]: r for r in isa_resources.kernels(os.path.join(build.CSRC, "bwagpu.hip"))}
    missing = [k for k in BOUNDS if k not in rows]
    assert not missing, f"kernels not in the code object (renamed? update BOUNDS): {missing}"
    over = []
    for k, (vgpr, scratch, spill, lds) in BOUNDS.items():
        r = rows[k]
        got = (int(r[1]), int(r[4]), int(r[6]), int(r[5]))
        print(k, "vgpr/scratch/spill/lds", got)
        if got[0] > vgpr or got[1] > scratch or got[2] > spill or got[3] != lds:
            over.append(f"{k}: vgpr/scratch/spill/lds {got} against {(vgpr, scratch, spill, lds)}")
    assert not over, "; ".join(over)
