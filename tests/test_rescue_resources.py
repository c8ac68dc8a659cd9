"""CPU: register, scratch and LDS use of the rescue kernels (dev_rescue.h), read from the code object's metadata (tools/isa_resources.py: hipcc -S, no GPU),
against bounds a little above what the tree has (count / scan / lane / wave<256> / wave<0> / pack: 16 / 44 / 119 / 166 / 156 / 28 VGPRs, no scratch, nothing spilled) and the LDS each form declares.  A pair's
working lists live in the arena, the sorts' indices, keys and stack in LDS or HBM scratch; a region held in a local struct (its bit-fields keep it out of
registers) or an introsort with its stack in a local array moves them into private memory and still passes every parity test."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# kernel (as tools/isa_resources.py prints it): (VGPRs, scratch bytes per lane, spilled VGPRs, LDS bytes) it may use at most
BOUNDS = {
    "k_rescue_count": (32, 0, 0, 0),
    "k_rescue_scan": (64, 0, 0, 2048),
    "k_rescue_lane": (128, 0, 0, 4352),              # one lane per pair: 17 index words x 64 lanes of LDS
    "k_rescue_wave<256>": (176, 0, 0, 23024),        # dedup_read_par's arrays for 256 regions (14 KB), the introsort's stack, the alignment's run list (8 KB)
    "k_rescue_wave<0>": (168, 0, 0, 8688),           # the arrays in HBM scratch
    "k_rescue_pack": (32, 0, 0, 0),
    "k_matesw_sw": (96, 0, 0, 32832),                # (shares msw_window and msw_align2 with the rescue kernels)
}


def test_rescue_kernels_do_not_spill():
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
