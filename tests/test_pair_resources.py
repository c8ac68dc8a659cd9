"""CPU: register and scratch use of the pairing kernels (dev_pair.h), read from the code object's metadata (tools/isa_resources.py: hipcc -S, no GPU),
against bounds a little above what the tree has (57 / 58 / 62 / 64 VGPRs, no scratch, nothing spilled) and the LDS each form declares.  The working arrays
of a pair live in LDS or in HBM scratch; a change that indexes the windows or the record by a lane's value moves them into private memory and still
passes every parity test."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# kernel (as tools/isa_resources.py prints it): (VGPRs, scratch bytes per lane, spilled VGPRs, LDS bytes) it may use at most
BOUNDS = {
    "k_pair_lane": (64, 0, 0, 16384),              # one lane per pair: 8 words x 4 hits x 128 lanes of LDS
    "k_pair_wave<128>": (64, 0, 0, 4096),
    "k_pair_wave<1024>": (72, 0, 0, 32768),
    "k_pair_wave<0>": (72, 0, 0, 0),               # the arrays in HBM scratch
}


def test_pair_kernels_do_not_spill():
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
