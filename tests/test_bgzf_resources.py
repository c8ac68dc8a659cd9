"""CPU: register, scratch and LDS use of the BGZF inflate kernel (dev_bgzf.h), read from the cross-compiled code object's metadata
(tools/isa_resources.py: hipcc -S, no GPU).  The kernel keeps a whole block's text in LDS: 70 576 bytes per wavefront, so that two fit the
160 KiB of a CU -- a larger figure silently halves what a CU decodes at once.  VGPR cap: the count measured on this tree
(profiles/dev_bgzf.md) rounded up to the allocation step of 8; nothing in scratch, nothing spilled."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_bgzf_kernel_does_not_spill_and_two_fit_a_cu():
    import isa_resources
    from bwa_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc is not installed")
    rows = {r[0]: r for r in isa_resources.kernels(os.path.join(build.CSRC, "bwagpu_index.hip"))}
    assert "k_bz_inflate" in rows, "kernel not in the code object (renamed?)"
    r = rows["k_bz_inflate"]
    vgpr, scratch, lds, spill = int(r[1]), int(r[4]), int(r[5]), int(r[6])
    print("k_bz_inflate vgpr/scratch/spill/lds", (vgpr, scratch, spill, lds))
    assert vgpr <= 152 and scratch == 0 and spill == 0 and lds == 70576 and 2 * lds <= 160 * 1024
