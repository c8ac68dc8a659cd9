"""CPU: register and scratch use of the alignment-list kernels (dev_alns.h), read from the code object's metadata (tools/isa_resources.py: hipcc -S, no GPU),
against bounds a little above what the tree has (43 / 34 VGPRs, no scratch, nothing spilled, no LDS).  The loop of mem_reg2sam keeps two integers per read; a
change that gives the kernels working arrays in private memory, or that spills, still passes every parity test."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# kernel (as tools/isa_resources.py prints it): (VGPRs, scratch bytes per lane, spilled VGPRs, LDS bytes) it may use at most
BOUNDS = {
    "k_alns_lane": (52, 0, 0, 0),
    "k_alns_wave": (44, 0, 0, 0),
}


def test_alns_kernels_do_not_spill():
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
        if got[0] > vgpr or got[1] > scratch or got[2] > spill or got[3] > lds:
            over.append(f"{k}: vgpr/scratch/spill/lds {got} > {(vgpr, scratch, spill, lds)}")
    assert not over, "; ".join(over)
