"""CPU: register, scratch and LDS use of the BGZF writer's kernels (dev_bgzf_out.h), read from the cross-compiled code object's metadata
(tools/isa_resources.py: hipcc -S, no GPU), as tests/test_fasta_reads_resources.py does for dev_fasta_reads.h.  No kernel may spill or use
scratch.  VGPR caps: the counts measured on this tree (profiles/dev_bgzf_out.md: 115 and 2) rounded up to the allocation step of 8; LDS is
exact: k_bo_deflate has BoLds -- the block's text, the hash heads, the tile's matches, counts, codes and the code builder's arrays --,
k_bo_gather has none."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# kernel: (VGPRs at most, scratch bytes per lane at most, spilled VGPRs at most, LDS bytes exactly)
BOUNDS = {
    "k_bo_deflate": (120, 0, 0, 108936),
    "k_bo_gather": (8, 0, 0, 0),
}


def test_bgzf_out_kernels_do_not_spill():
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
