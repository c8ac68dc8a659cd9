"""CPU: register and scratch use of the kernels that decide a read pair (dev_sampe.h), read from the code object's metadata (tools/isa_resources.py: hipcc -S, no
GPU), against bounds a little above what the tree has.  Measured: k_sampe_lane 78 VGPRs, k_sampe_wave 57, k_alns_pe_lane 50, k_alns_pe_wave 38,
k_sampe_reg_read 26; no scratch, nothing spilled, no LDS in any of them.  The decision is scalar per pair apart from two loops that keep nothing between their
steps; a change that gives the kernels working arrays in private memory or in LDS, or that spills, still passes every parity test."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# kernel (as tools/isa_resources.py prints it): (VGPRs, scratch bytes per lane, spilled VGPRs, LDS bytes) it may use at most
BOUNDS = {
    "k_sampe_lane": (86, 0, 0, 0),
    "k_sampe_wave": (65, 0, 0, 0),
    "k_alns_pe_lane": (58, 0, 0, 0),
    "k_alns_pe_wave": (46, 0, 0, 0),
    "k_sampe_reg_read": (34, 0, 0, 0),
}


def test_sampe_kernels_do_not_spill():
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
