"""CPU: register, scratch and LDS use of the FASTA read reader's kernels (dev_fasta_reads.h), read from the cross-compiled code object's
metadata (tools/isa_resources.py: hipcc -S, no GPU), as tests/test_fastq_resources.py does for dev_fastq.h.  No kernel may spill or use
scratch.  VGPR caps: the counts measured on this tree (profiles/dev_fasta_reads.md) rounded up to the allocation step of 8; LDS is exact:
k_fr_index has the block scan's 1024 bytes, k_fr_decide is fq_decide_status like k_fq_decide (its result struct in LDS, 72 bytes per lane
of its wavefront), the others have none."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# kernel: (VGPRs at most, scratch bytes per lane at most, spilled VGPRs at most, LDS bytes exactly)
BOUNDS = {
    "k_fr_index": (48, 0, 0, 1024),
    "k_fr_lines": (16, 0, 0, 0),
    "k_fr_place": (16, 0, 0, 0),
    "k_fr_records": (32, 0, 0, 0),
    "k_fr_cut": (8, 0, 0, 0),
    "k_fr_decide": (24, 0, 0, 4608),
    "k_fr_emit": (56, 0, 0, 0),
}


def test_fasta_read_kernels_do_not_spill():
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
