"""CPU: register, scratch and LDS use of the kernels of `mem -p` on the device FASTQ reader (dev_fastq_smart.h), read from the cross-compiled
code object's metadata (tools/isa_resources.py: hipcc -S, no GPU), as tests/test_fastq_resources.py does for the reader's own.  No kernel may
spill or use scratch; none uses LDS.  VGPR caps: the counts measured on this tree (profiles/dev_fastq_smart.md: 21, 18, 44) rounded up to the
allocation step of 8."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# kernel: (VGPRs at most, scratch bytes per lane at most, spilled VGPRs at most, LDS bytes exactly)
BOUNDS = {
    "k_fqs_eq": (24, 0, 0, 0),
    "k_fqs_class": (24, 0, 0, 0),
    "k_fqs_emit": (48, 0, 0, 0),
}


def test_fastq_smart_kernels_do_not_spill():
    import isa_resources
    from bwa_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc is not installed")
    rows = {r[0]: r for r in isa_resources.kernels(os.path.join(build.CSRC, "bwagpu_index.hip"))}
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
