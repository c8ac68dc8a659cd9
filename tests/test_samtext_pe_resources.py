"""CPU: register, scratch and LDS use of the paired-end SAM text kernels (dev_samtext_pe.h), read from the code object's metadata (tools/isa_resources.py:
hipcc -S, no GPU).  The mate enters the formatter as a few wave-uniform values and two pointers; like the single-end kernels these keep no array in private
memory: no scratch, nothing spilled, and the one staging area of SAM_STAGE = 512 bytes per workgroup in the writing pass.  The tree has 39 VGPRs in
k_sam_pe_size and 120 in k_sam_pe_write; the bounds are those values rounded up to the allocation step of 8 registers (40, 120), so k_sam_pe_write stays
under 128 and leaves the four wavefronts per SIMD (512 / 120) that k_sam_write's 113 -> 120 registers leave.  The single-end kernels are pinned by
test_samtext_resources.py: the mate is a type there (SamNoMate) and they compile to what they were, 35 / 113 VGPRs."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# kernel (as tools/isa_resources.py prints it): (VGPRs at most, scratch bytes per lane at most, spilled VGPRs at most, LDS bytes exactly)
BOUNDS = {
    "k_sam_pe_size": (40, 0, 0, 0),
    "k_sam_pe_write": (120, 0, 0, 512),
}


def test_samtext_pe_kernels_do_not_spill():
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
