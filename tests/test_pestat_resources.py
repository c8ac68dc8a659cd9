"""CPU: register and scratch use of the insert-size kernels (dev_pestat.h), read from the code object's metadata (tools/isa_resources.py: hipcc -S, no GPU),
against bounds a little above what the tree has (k_pestat_collect 20 VGPRs and no LDS, k_pestat_finish 38 VGPRs and 48 bytes of LDS; no scratch, nothing
spilled).  Both kernels keep their state in registers; a change that indexes the four orientations' values by a lane's value would move them into private
memory and still pass every parity test."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# kernel (as tools/isa_resources.py prints it): (VGPRs, scratch bytes per lane, spilled VGPRs, LDS bytes) it may use at most
BOUNDS = {
    "k_pestat_collect": (24, 0, 0, 0),             # one lane per pair, plain global atomics
    "k_pestat_finish": (44, 0, 0, 64),             # four wavefronts; the four counts and failed flags in LDS
}


def test_pestat_kernels_do_not_spill():
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
