"""Python binding (ctypes) of the C-ABI in include/bwagpu.h.

This is plumbing for tests and bench.py: every call goes straight into libbwagpu.so, the HIP library built by
`bwa_amd.build`.  There is no CPU implementation behind it; if the library is missing or no GPU is visible the
constructor raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

try:   # torch bundles its own HIP runtime (libamdhip64); loading it first keeps one runtime per process
    import torch  # noqa: F401
except Exception:  # pragma: no cover
    torch = None

from .structs import ALN_DTYPE, ALNREG_DTYPE, PAIR_DTYPE, PESTAT_DTYPE, PESTAT_INFO_DTYPE, PRIMARY_DTYPE, RESCUE_DTYPE, SAMPE_DTYPE, MemOpt, PeOut, SamIn, SamOut

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(HERE, "csrc", "libbwagpu.so")

INTV3_DTYPE = np.dtype([("x0", "<u8"), ("x2", "<u8"), ("info", "<u8")])
GCHAIN_DTYPE = np.dtype([("n_seeds", "<i4"), ("rid", "<i4"), ("w", "<i4"), ("kept", "<i4"), ("is_alt", "<i4"),
                         ("frac_rep", "<f4"), ("pos", "<i8")])
GSEED_DTYPE = np.dtype([("rbeg", "<i8"), ("qbeg", "<i4"), ("len", "<i4"), ("score", "<i4"), ("_pad", "<i4")])
assert GCHAIN_DTYPE.itemsize == 32 and GSEED_DTYPE.itemsize == 24


MATESW_DTYPE = np.dtype([("read", "<i4"), ("r", "<i4"), ("anchor_rb", "<i8"), ("anchor_rid", "<i4"), ("score", "<i4"), ("te", "<i4"), ("qe", "<i4"),
                         ("score2", "<i4"), ("te2", "<i4"), ("tb", "<i4"), ("qb", "<i4"), ("pad_", "<i4"), ("pad2_", "<i4")])   # bwagpu_matesw_t (56 bytes with its tail padding)
assert MATESW_DTYPE.itemsize == 56
PES_DTYPE = np.dtype([("low", "<i4"), ("high", "<i4"), ("failed", "<i4"), ("pad_", "<i4")])               # bwagpu_pes_t
CIGAR_DTYPE = np.dtype([("score", "<i4"), ("n_cigar", "<i4"), ("cigar", "<u4", (6,)), ("nm", "<i4"), ("md_len", "<i4"), ("md", "<u8")])   # bwagpu_cigar_t
assert CIGAR_DTYPE.itemsize == 48
DP_CASE_DTYPE = np.dtype([("q_off", "<i4"), ("q_len", "<i4"), ("t_off", "<i4"), ("t_len", "<i4"), ("w", "<i4"), ("h0", "<i4"), ("end_bonus", "<i4"), ("flags", "<i4")])   # bwagpu_dp_case_t
assert DP_CASE_DTYPE.itemsize == 32
SORT_KEY_DTYPE = np.dtype([("a", "<i8"), ("b", "<i4"), ("c", "<i4")])   # bwagpu_sort_key_t
assert SORT_KEY_DTYPE.itemsize == 16


class Stats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in (
        "n_reads", "n_bases", "n_intv", "n_seeds", "n_chains", "n_regs_raw", "n_regs", "n_occ_blocks", "n_lf_steps",
        "n_ext_calls", "n_ext_cells", "n_glb_calls", "n_glb_cells", "ref_bases", "n_sw_calls", "n_sw_cells")] + [
        (n, C.c_float) for n in ("ms_seed", "ms_sa", "ms_chain", "ms_seedsw", "ms_extend", "ms_dedup", "ms_total")] + [
        ("n_retries", C.c_int32), ("ms_publish", C.c_float), ("n_tab_lookups", C.c_int64), ("n_bt_nodes", C.c_int64), ("n_chain_recs", C.c_int64),
        ("n_chain_deferred", C.c_int64), ("n_ext_fast", C.c_int64), ("n_chain_deferred2", C.c_int64),
        ("ms_pack", C.c_float), ("ms_download_copy", C.c_float), ("ms_cigar_kernels", C.c_float), ("ms_cigar_copy", C.c_float),
        ("n_cig_cells", C.c_int64), ("n_cig_dp", C.c_int64), ("retry_mask", C.c_int32), ("reserved_", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved_"}


EXPORTS = [
    "bwagpu_create", "bwagpu_create_from_files", "bwagpu_destroy", "bwagpu_strerror", "bwagpu_last_error", "bwagpu_version",
    "bwagpu_index_info", "bwagpu_densify_sa", "bwagpu_set_stats", "bwagpu_get_stats", "bwagpu_align_bseq", "bwagpu_align_flat",
    "bwagpu_free", "bwagpu_batch_upload", "bwagpu_batch_run", "bwagpu_batch_download", "bwagpu_set_taps", "bwagpu_tap_intervals",
    "bwagpu_tap_chains", "bwagpu_tap_regs_raw", "bwagpu_index_buffers", "bwagpu_index_export", "bwagpu_clone", "bwagpu_index_ready",
    "bwagpu_batch_cigars", "bwagpu_batch_cigar_ops", "bwagpu_debug_phase", "bwagpu_batch_matesw", "bwagpu_clone_to_device", "bwagpu_index_build", "bwagpu_built_free", "bwagpu_abi_sizes", "bwagpu_debug_prof", "bwagpu_debug_hist", "bwagpu_debug_seed_x2", "bwagpu_debug_ptab", "bwagpu_debug_chain_hist", "bwagpu_debug_dp", "bwagpu_debug_sort", "bwagpu_debug_sort_limits", "bwagpu_set_cigar_filter", "bwagpu_batch_reserve", "bwagpu_batch_footprint", "bwagpu_mem_info",
    "bwagpu_batch_primary", "bwagpu_primary_flat", "bwagpu_primary_limits", "bwagpu_batch_pair", "bwagpu_pair_flat", "bwagpu_pair_limits", "bwagpu_batch_rescue", "bwagpu_rescue_flat", "bwagpu_rescue_limits",
    "bwagpu_batch_pestat", "bwagpu_pestat_flat", "bwagpu_batch_pestat_hist", "bwagpu_pestat_finish", "bwagpu_pestat_limits",
    "bwagpu_batch_alns", "bwagpu_alns_flat", "bwagpu_alns_limits", "bwagpu_aln_size",
    "bwagpu_cigars_flat", "bwagpu_cigar_limits", "bwagpu_dedup_flat", "bwagpu_dedup_limits", "bwagpu_ext_limits", "bwagpu_seed_limits",
    "bwagpu_batch_sampe", "bwagpu_sampe_flat", "bwagpu_sampe_limits", "bwagpu_sampe_size",
    "bwagpu_set_contig_names", "bwagpu_batch_sam", "bwagpu_sam_flat", "bwagpu_sam_limits",
    "bwagpu_trim", "bwagpu_set_option", "bwagpu_get_option", "bwagpu_set_default_option", "bwagpu_clear_default_options", "bwagpu_option_name",
]


class IndexDesc(C.Structure):
    _fields_ = [("bwt", C.c_void_p), ("bwt_size", C.c_uint64), ("primary", C.c_uint64), ("L2", C.c_uint64 * 5), ("seq_len", C.c_uint64),
                ("sa", C.c_void_p), ("n_sa", C.c_uint64), ("sa_intv", C.c_int), ("pac", C.c_void_p), ("l_pac", C.c_int64),
                ("n_seqs", C.c_int32), ("ctg_offset", C.c_void_p), ("ctg_len", C.c_void_p), ("ctg_is_alt", C.c_void_p)]


class BwaGpuError(RuntimeError):
    pass


def load_library(path: str | None = None) -> C.CDLL:
    path = path or DEFAULT_LIB
    if not os.path.exists(path):
        raise BwaGpuError(f"{path} not found: build the HIP library first (python -m bwa_amd.build); there is no CPU fallback")
    L = C.CDLL(path)
    L.bwagpu_strerror.restype = C.c_char_p
    L.bwagpu_last_error.restype = C.c_char_p
    L.bwagpu_last_error.argtypes = [C.c_void_p]
    L.bwagpu_version.restype = C.c_char_p
    L.bwagpu_create_from_files.argtypes = [C.POINTER(C.c_void_p), C.c_char_p, C.c_int]
    L.bwagpu_destroy.argtypes = [C.c_void_p]
    L.bwagpu_index_info.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bwagpu_densify_sa.argtypes = [C.c_void_p, C.c_int]
    L.bwagpu_set_stats.argtypes = [C.c_void_p, C.c_int]
    L.bwagpu_set_taps.argtypes = [C.c_void_p, C.c_int]
    L.bwagpu_get_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.bwagpu_align_flat.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bwagpu_batch_upload.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.bwagpu_batch_run.argtypes = [C.c_void_p, C.c_void_p]
    L.bwagpu_batch_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bwagpu_batch_matesw.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bwagpu_batch_cigars.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bwagpu_batch_cigar_ops.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.bwagpu_cigars_flat.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 8
    L.bwagpu_cigar_limits.restype = None
    L.bwagpu_dedup_flat.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 8
    L.bwagpu_dedup_limits.restype = None
    L.bwagpu_ext_limits.restype = None
    L.bwagpu_seed_limits.argtypes = [C.c_void_p, C.c_void_p]
    L.bwagpu_seed_limits.restype = None
    L.bwagpu_tap_intervals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bwagpu_tap_chains.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bwagpu_tap_regs_raw.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bwagpu_free.argtypes = [C.c_void_p]
    L.bwagpu_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int]
    L.bwagpu_clone.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.bwagpu_index_ready.argtypes = [C.c_void_p]
    L.bwagpu_index_buffers.argtypes = [C.c_void_p] + [C.c_void_p] * 6
    L.bwagpu_index_export.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bwagpu_debug_dp.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.bwagpu_debug_sort.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.bwagpu_batch_primary.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bwagpu_primary_flat.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bwagpu_primary_limits.restype = None
    L.bwagpu_batch_pair.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bwagpu_pair_flat.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bwagpu_pair_limits.restype = None
    L.bwagpu_batch_rescue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 9
    L.bwagpu_rescue_flat.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 14
    L.bwagpu_rescue_limits.restype = None
    L.bwagpu_batch_pestat.argtypes = [C.c_void_p] * 5
    L.bwagpu_pestat_flat.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5
    L.bwagpu_batch_pestat_hist.argtypes = [C.c_void_p] * 5
    L.bwagpu_pestat_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bwagpu_pestat_limits.restype = None
    L.bwagpu_batch_alns.argtypes = [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 6
    L.bwagpu_alns_flat.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int64] + [C.c_void_p] * 5
    L.bwagpu_alns_limits.restype = None
    L.bwagpu_batch_sampe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.bwagpu_sampe_flat.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7
    L.bwagpu_sampe_limits.restype = None
    L.bwagpu_set_contig_names.argtypes = [C.c_void_p] * 5
    L.bwagpu_batch_sam.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.bwagpu_sam_flat.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_int64, C.c_void_p, C.c_void_p]
    L.bwagpu_sam_limits.restype = None
    L.bwagpu_batch_sam_pe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4
    L.bwagpu_sam_pe_flat.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 9
    L.bwagpu_sam_pe_limits.restype = None
    L.bwagpu_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_longlong]
    L.bwagpu_get_option.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
    L.bwagpu_set_default_option.argtypes = [C.c_char_p, C.c_longlong]
    L.bwagpu_clear_default_options.restype = None
    L.bwagpu_option_name.argtypes = [C.c_int, C.c_void_p]
    return L


def option_names(L: C.CDLL) -> list:
    """The library's option list (bwa_amd/csrc/bwagpu_config.h), as bwagpu_option_name enumerates it."""
    out, i, p = [], 0, C.c_char_p()
    while L.bwagpu_option_name(i, C.byref(p)) == 0:
        out.append(p.value.decode()); i += 1
    return out


def _ragged_bytes(items):
    """(the items back to back, int64 offsets[len + 1])"""
    off = np.zeros(len(items) + 1, dtype=np.int64)
    if items:
        off[1:] = np.cumsum([len(x) for x in items])
    return b"".join(items), off


import threading
_CREATE_LOCK = threading.Lock()


class BwaGpu:
    """One handle = one GPU with the index resident in HBM."""

    def __init__(self, prefix: str, device: int = 0, lib_path: str | None = None, options: dict | None = None):
        """options: {name: integer} of include/bwagpu.h's option list -- given to the library as defaults for the handle being created (so
        that the ones shaping what is derived from the index at load time -- occ32, occ32_sb_shift, ptab_m -- apply) and forgotten again."""
        self.L = load_library(lib_path)
        self.h = C.c_void_p()
        with _CREATE_LOCK:      # (the defaults are process-wide: two handles created from two threads must not see each other's, or have theirs cleared)
            try:
                for k, v in (options or {}).items():
                    if self.L.bwagpu_set_default_option(k.encode(), int(v)) != 0:
                        raise BwaGpuError(f"unknown option {k!r}")
                rc = self.L.bwagpu_create_from_files(C.byref(self.h), prefix.encode(), device)
            finally:
                if options:
                    self.L.bwagpu_clear_default_options()
        if rc != 0:
            raise BwaGpuError(f"bwagpu_create_from_files({prefix}) failed: {self.L.bwagpu_strerror(rc).decode()}")
        self.set_taps(True)     # the library's default is off (a second region arena per batch); the tests read the stage taps, bench.py turns them off

    @classmethod
    def empty(cls, meta: dict, device: int = 0, lib_path: str | None = None):
        """Receiving side of an index broadcast: allocate the HBM buffers described by `meta` without uploading."""
        self = cls.__new__(cls)
        self.L = load_library(lib_path)
        self.h = C.c_void_p()
        d = IndexDesc()
        for k in ("bwt_size", "primary", "seq_len", "n_sa", "sa_intv", "l_pac", "n_seqs"):
            setattr(d, k, meta[k])
        for i in range(5):
            d.L2[i] = meta["L2"][i]
        off = np.ascontiguousarray(meta["ctg_offset"], dtype=np.int64)
        ln = np.ascontiguousarray(meta["ctg_len"], dtype=np.int32)
        alt = np.ascontiguousarray(meta["ctg_is_alt"], dtype=np.int32)
        d.ctg_offset, d.ctg_len, d.ctg_is_alt = off.ctypes.data, ln.ctypes.data, alt.ctypes.data
        rc = self.L.bwagpu_create(C.byref(self.h), C.byref(d), device)
        if rc != 0:
            raise BwaGpuError(f"bwagpu_create(empty) failed: {self.L.bwagpu_strerror(rc).decode()}")
        return self

    def index_ready(self):
        self._chk(self.L.bwagpu_index_ready(self.h))

    def clone(self):
        """A second handle sharing this one's resident index, with its own stream and arenas (for a second host thread)."""
        other = BwaGpu.__new__(BwaGpu)
        other.L = self.L
        other.h = C.c_void_p()
        self._chk(self.L.bwagpu_clone(self.h, C.byref(other.h)))
        return other

    def index_meta(self) -> dict:
        d = IndexDesc()
        self._chk(self.L.bwagpu_index_export(self.h, C.byref(d), None, None, None))
        off = np.zeros(d.n_seqs, dtype=np.int64); ln = np.zeros(d.n_seqs, dtype=np.int32); alt = np.zeros(d.n_seqs, dtype=np.int32)
        self._chk(self.L.bwagpu_index_export(self.h, C.byref(d), off.ctypes.data, ln.ctypes.data, alt.ctypes.data))
        return {"bwt_size": d.bwt_size, "primary": d.primary, "L2": [int(x) for x in d.L2], "seq_len": d.seq_len, "n_sa": d.n_sa,
                "sa_intv": d.sa_intv, "l_pac": d.l_pac, "n_seqs": d.n_seqs, "ctg_offset": off, "ctg_len": ln, "ctg_is_alt": alt}

    def index_buffers(self):
        """[(device pointer, bytes)] of the BWT/Occ blocks, the SA and the pac -- the payload of the index broadcast."""
        p = [C.c_void_p() for _ in range(3)]
        n = [C.c_uint64() for _ in range(3)]
        self._chk(self.L.bwagpu_index_buffers(self.h, C.byref(p[0]), C.byref(n[0]), C.byref(p[1]), C.byref(n[1]), C.byref(p[2]), C.byref(n[2])))
        return [(p[i].value, n[i].value) for i in range(3)]

    def _chk(self, rc):
        if rc != 0:
            raise BwaGpuError(f"{self.L.bwagpu_strerror(rc).decode()}: {self.L.bwagpu_last_error(self.h).decode()}")

    def close(self):
        if self.h:
            self.L.bwagpu_destroy(self.h)
            self.h = C.c_void_p()

    def set_stats(self, on=True):
        self._chk(self.L.bwagpu_set_stats(self.h, int(on)))

    def set_option(self, name: str, value: int):
        """bwagpu_set_option: one of the handle's tuning / test options (bwa_amd/csrc/bwagpu_config.h), between batches."""
        self._chk(self.L.bwagpu_set_option(self.h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = C.c_longlong()
        self._chk(self.L.bwagpu_get_option(self.h, name.encode(), C.byref(v)))
        return v.value

    def set_taps(self, on=True):
        self._chk(self.L.bwagpu_set_taps(self.h, int(on)))

    def densify_sa(self, intv: int):
        self._chk(self.L.bwagpu_densify_sa(self.h, intv))

    def stats(self) -> dict:
        s = Stats()
        self._chk(self.L.bwagpu_get_stats(self.h, C.byref(s)))
        return s.as_dict()

    # -- hot path -------------------------------------------------------------------------------------------
    def upload(self, seqs: np.ndarray, off: np.ndarray):
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        self._n = off.shape[0] - 1
        self._chk(self.L.bwagpu_batch_upload(self.h, self._n, seqs.ctypes.data, off.ctypes.data))

    def run(self, opt: MemOpt):
        self._chk(self.L.bwagpu_batch_run(self.h, C.byref(opt)))

    def _take(self, ptr, n, dtype):
        out = np.frombuffer(C.string_at(ptr, n * dtype.itemsize), dtype=dtype).copy() if n else np.zeros(0, dtype=dtype)
        self.L.bwagpu_free(ptr)
        return out

    def download(self):
        counts = np.zeros(self._n, dtype=np.int32)
        p = C.c_void_p()
        n = C.c_int64()
        self._chk(self.L.bwagpu_batch_download(self.h, counts.ctypes.data, C.byref(p), C.byref(n)))
        return counts, self._take(p, n.value, ALNREG_DTYPE)

    def cigars(self, opt: MemOpt):
        """bwagpu_batch_cigars: one CIGAR_DTYPE record per region of the last download(), in its order."""
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.bwagpu_batch_cigars(self.h, C.byref(opt), C.byref(p), C.byref(n)))
        return self._take(p, n.value, CIGAR_DTYPE)

    def cigar_ops(self):
        """bwagpu_batch_cigar_ops: the operation array of the last cigars() call (records with 7..64 operations point into it)."""
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.bwagpu_batch_cigar_ops(self.h, C.byref(p), C.byref(n)))
        return self._take(p, n.value, np.dtype("<u4"))

    @staticmethod
    def _flat_reads(seqs, off, n):
        """the reads of a *_flat call: contiguous (seqs uint8, off int64), one offset more than the n reads"""
        seqs, off = np.ascontiguousarray(seqs, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.int64)
        assert off.shape == (n + 1,)
        return seqs, off

    @staticmethod
    def _flat_lists(counts, regs, ids=None):
        """the lists of a *_flat call: contiguous (counts int32, regs ALNREG_DTYPE[, ids int64, one per read]), as many regions as the counts say"""
        counts, regs = np.ascontiguousarray(counts, dtype=np.int32), np.ascontiguousarray(regs, dtype=ALNREG_DTYPE)
        assert int(counts.sum()) == regs.shape[0]
        if ids is None:
            return counts, regs
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        assert ids.shape == counts.shape
        return counts, regs, ids

    def cigars_flat(self, opt: MemOpt, seqs: np.ndarray, off: np.ndarray, counts: np.ndarray, regs: np.ndarray):
        """bwagpu_cigars_flat: the kernels of cigars() on reads (nt4, int64 offsets) and region lists of the caller (read i: counts[i] records of regs)
        -> (CIGAR_DTYPE records in the regions' order, the operation array they point into).  Leaves the last cigars() / cigar_ops() of the handle alone."""
        counts, regs = self._flat_lists(counts, regs)
        seqs, off = self._flat_reads(seqs, off, counts.shape[0])
        assert int(off[-1]) == seqs.shape[0]
        p, n, po, no = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_int64()
        self._chk(self.L.bwagpu_cigars_flat(self.h, C.byref(opt), counts.shape[0], seqs.ctypes.data, off.ctypes.data, counts.ctypes.data, regs.ctypes.data,
                                            C.byref(p), C.byref(n), C.byref(po), C.byref(no)))
        return self._take(p, n.value, CIGAR_DTYPE), self._take(po, no.value, np.dtype("<u4"))

    def cigar_limits(self) -> dict:
        """bwagpu_cigar_limits: the constants of the CIGAR kernels (dev_cigar.h), as compiled."""
        out = (C.c_int32 * 10)()
        self.L.bwagpu_cigar_limits(out)
        return dict(zip(("max_len", "z_small", "z_big", "max_cols", "max_ops", "tmp_ops", "md_cap", "long_max_cols", "long_max_ops", "long_qcap"), list(out)))

    def dedup_flat(self, opt: MemOpt, seqs: np.ndarray, off: np.ndarray, counts: np.ndarray, regs: np.ndarray):
        """bwagpu_dedup_flat: the de-duplication stage of run() on reads (nt4, int64 offsets) and raw region lists of the caller (read i: counts[i] records of regs)
        -> (counts left per read, their ALNREG_DTYPE records read by read, the routine that finished each read: 0 dedup_read, 1 dedup_read_wave, 2 dedup_read_par)."""
        counts, regs = self._flat_lists(counts, regs)
        seqs, off = self._flat_reads(seqs, off, counts.shape[0])
        assert int(off[-1]) == seqs.shape[0]
        left = np.zeros(counts.shape[0], dtype=np.int32)
        form = np.full(counts.shape[0], -1, dtype=np.int32)
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.bwagpu_dedup_flat(self.h, C.byref(opt), counts.shape[0], seqs.ctypes.data, off.ctypes.data, counts.ctypes.data, regs.ctypes.data,
                                           left.ctypes.data, C.byref(p), C.byref(n), form.ctypes.data))
        assert n.value == int(left.sum())
        return left, self._take(p, n.value, ALNREG_DTYPE), form

    def dedup_limits(self) -> dict:
        """bwagpu_dedup_limits: the switch points of the de-duplication stage, as compiled."""
        out = (C.c_int32 * 8)()
        self.L.bwagpu_dedup_limits(out)
        return dict(zip(("heavy", "stage", "net", "keysort_min", "scan_block", "draw", "ring_min", "lds_per_reg"), list(out)))

    def ext_limits(self) -> dict:
        """bwagpu_ext_limits: the switch points of the extension stage (mem_chain2aln on the device), as compiled."""
        out = (C.c_int32 * 6)()
        self.L.bwagpu_ext_limits(out)
        return dict(zip(("sort_lane_max", "kept_short", "kept_ring", "covered_step", "wave_max_len", "ring_max"), list(out)))

    def seed_limits(self) -> dict:
        """bwagpu_seed_limits: the switch points of the seeding stage (mem_collect_intv on the device), as compiled; ptab_depth as in force for this handle's index, lds_ent_run for its last run()."""
        out = (C.c_int32 * 10)()
        self.L.bwagpu_seed_limits(self.h, out)
        return dict(zip(("ptab_max", "ptab_depth", "lds_ent", "rd_lds_max_len", "wave_max_len", "cand_bits", "pub_max", "task_stack_cap", "lane_lds", "lds_ent_run"), list(out)))

    def matesw(self, opt: MemOpt, pes: np.ndarray):
        """bwagpu_batch_matesw: precomputed mate-rescue alignments (MATESW_DTYPE) for the last download(); pes = PES_DTYPE[4]."""
        pes = np.ascontiguousarray(pes, dtype=PES_DTYPE)
        assert pes.shape == (4,)
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.bwagpu_batch_matesw(self.h, C.byref(opt), pes.ctypes.data, C.byref(p), C.byref(n)))
        return self._take(p, n.value, MATESW_DTYPE)

    def primary(self, opt: MemOpt, id0: int = 0):
        """bwagpu_batch_primary: mem_mark_primary_se + mem_approx_mapq_se of every read of the last download() on the device; read i has id id0 + i.
        -> (PRIMARY_DTYPE records, concatenated per read with the download's counts; n_pri int32[n reads]; device time of the kernels in ms)"""
        p, n, ms = C.c_void_p(), C.c_int64(), C.c_float()
        n_pri = np.zeros(self._n, dtype=np.int32)
        self._chk(self.L.bwagpu_batch_primary(self.h, C.byref(opt), int(id0), C.byref(p), C.byref(n), n_pri.ctypes.data, C.byref(ms)))
        return self._take(p, n.value, PRIMARY_DTYPE), n_pri, ms.value

    def primary_flat(self, opt: MemOpt, counts: np.ndarray, regs: np.ndarray, ids: np.ndarray):
        """bwagpu_primary_flat: the same kernels on region lists of the caller (read i: counts[i] records of regs, id ids[i]) -> (records, n_pri, ms)."""
        counts, regs, ids = self._flat_lists(counts, regs, ids)
        p, ms = C.c_void_p(), C.c_float()
        n_pri = np.zeros(counts.shape[0], dtype=np.int32)
        self._chk(self.L.bwagpu_primary_flat(self.h, C.byref(opt), counts.shape[0], counts.ctypes.data, regs.ctypes.data, ids.ctypes.data, C.byref(p), n_pri.ctypes.data, C.byref(ms)))
        return self._take(p, regs.shape[0], PRIMARY_DTYPE), n_pri, ms.value

    def primary_limits(self) -> dict:
        """bwagpu_primary_limits: the region counts at which the marking kernels change their form, as compiled."""
        out = (C.c_int32 * 4)()
        self.L.bwagpu_primary_limits(out)
        return dict(zip(("lane_max", "lds_small", "lds_big", "scan"), list(out)))

    def alns(self, opt: MemOpt, id0: int = 0):
        """bwagpu_batch_alns: after download() and cigars(), mem_reg2aln of every region and mem_reg2sam's list of every read on the device; read i has id
        id0 + i.  -> (ALN_DTYPE records in marked order per read, n_aln int32[n reads], PRIMARY_DTYPE records, n_pri, device time of the kernels in ms)"""
        p, n, pr, ms = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_float()
        n_aln = np.zeros(self._n, dtype=np.int32); n_pri = np.zeros(self._n, dtype=np.int32)
        self._chk(self.L.bwagpu_batch_alns(self.h, C.byref(opt), int(id0), C.byref(p), C.byref(n), n_aln.ctypes.data, C.byref(pr), n_pri.ctypes.data, C.byref(ms)))
        return self._take(p, n.value, ALN_DTYPE), n_aln, self._take(pr, n.value, PRIMARY_DTYPE), n_pri, ms.value

    def alns_flat(self, opt: MemOpt, counts: np.ndarray, regs: np.ndarray, ids: np.ndarray, read_len: np.ndarray, cigs: np.ndarray, ops: np.ndarray):
        """bwagpu_alns_flat: the same kernels on unmarked lists of the caller (read i: counts[i] records of regs, id ids[i], read_len[i] bases) with one CIGAR
        record per region (cigs) and their operation array (ops) -> (records, n_aln, marking records, n_pri, ms)."""
        counts, regs, ids = self._flat_lists(counts, regs, ids)
        read_len = np.ascontiguousarray(read_len, dtype=np.int32)
        cigs = np.ascontiguousarray(cigs, dtype=CIGAR_DTYPE)
        ops = np.ascontiguousarray(ops, dtype=np.uint32)
        assert counts.shape == read_len.shape and regs.shape[0] == cigs.shape[0]
        p, pr, ms = C.c_void_p(), C.c_void_p(), C.c_float()
        n_aln = np.zeros(counts.shape[0], dtype=np.int32); n_pri = np.zeros(counts.shape[0], dtype=np.int32)
        self._chk(self.L.bwagpu_alns_flat(self.h, C.byref(opt), counts.shape[0], counts.ctypes.data, regs.ctypes.data, ids.ctypes.data, read_len.ctypes.data,
                                          cigs.ctypes.data, ops.ctypes.data, ops.shape[0], C.byref(p), n_aln.ctypes.data, C.byref(pr), n_pri.ctypes.data, C.byref(ms)))
        return self._take(p, regs.shape[0], ALN_DTYPE), n_aln, self._take(pr, regs.shape[0], PRIMARY_DTYPE), n_pri, ms.value

    def alns_limits(self) -> dict:
        """bwagpu_alns_limits: the region count up to which one lane makes a read's list, and the regions a wavefront takes per step."""
        out = (C.c_int32 * 2)()
        self.L.bwagpu_alns_limits(out)
        return dict(zip(("lane_max", "step"), list(out)))

    # -- SAM text on the device (single-end) ------------------------------------------------------------------
    def set_contig_names(self, names, annos=None):
        """bwagpu_set_contig_names: the contigs' names (and annotations) of a handle that was not created from index files; str or bytes, one per contig."""
        enc = lambda xs: [x.encode() if isinstance(x, str) else bytes(x) for x in xs]
        nb, no = _ragged_bytes(enc(names))
        ab, ao = _ragged_bytes(enc(annos)) if annos is not None else (None, None)
        self._chk(self.L.bwagpu_set_contig_names(self.h, nb, no.ctypes.data, ab, None if ao is None else ao.ctypes.data))

    def _sam_call(self, n, names, quals, comments, rg_id, extra_flag, call):
        enc = lambda xs: [x.encode() if isinstance(x, str) else bytes(x) for x in xs]
        nb, no = _ragged_bytes(enc(names))
        assert no.shape[0] == n + 1
        cb, co = _ragged_bytes(enc(comments)) if comments is not None else (None, None)
        keep = (nb, no, cb, co, quals, rg_id.encode() if isinstance(rg_id, str) else rg_id)
        sin = SamIn(C.cast(C.c_char_p(nb), C.c_void_p), no.ctypes.data, C.cast(C.c_char_p(quals), C.c_void_p) if quals is not None else None,
                    C.cast(C.c_char_p(cb), C.c_void_p) if cb is not None else None, co.ctypes.data if co is not None else None, keep[5], int(extra_flag))
        out = SamOut()
        self._chk(call(C.byref(sin), C.byref(out)))
        text = C.string_at(out.text, out.n_text)
        self.L.bwagpu_free(out.text)
        res = dict(text=text, off=self._take(out.off, n + 1, np.dtype("<i8")), flags=self._take(out.flags, n, np.dtype("<i4")),
                   n_lines=self._take(out.n_lines, n, np.dtype("<i4")), n_declined=int(out.n_declined), kernel_ms=tuple(out.kernel_ms))
        del keep
        return res

    def sam(self, opt: MemOpt, id0, names, quals=None, comments=None, rg_id=None, extra_flag=0):
        """bwagpu_batch_sam: after download() and cigars(), the SAM text of every read of the batch, written on the device; read i has id id0 + i and the name
        names[i].  quals: bytes, one per base in the reads' order, or None ('*'); comments: one per read ('' prints nothing) or None.
        -> dict(text: bytes, off int64[n + 1]: read i's lines are text[off[i]:off[i + 1]], flags int32[n]: bit 0 = declined (no bytes, the caller formats the
        read), n_lines int32[n], n_declined, kernel_ms: (marking + alignment lists, sizing + prefix sum, writing))"""
        return self._sam_call(self._n, names, quals, comments, rg_id, extra_flag, lambda i, o: self.L.bwagpu_batch_sam(self.h, C.byref(opt), int(id0), i, o))

    def sam_flat(self, opt: MemOpt, seqs, off, counts, regs, ids, cigs, ops, names, quals=None, comments=None, rg_id=None, extra_flag=0):
        """bwagpu_sam_flat: the same kernels on reads (nt4 with n + 1 offsets), unmarked lists, ids, CIGAR records and operation array of the caller -> as sam()."""
        counts, regs, ids = self._flat_lists(counts, regs, ids)
        seqs, off = self._flat_reads(seqs, off, counts.shape[0])
        cigs = np.ascontiguousarray(cigs, dtype=CIGAR_DTYPE)
        ops = np.ascontiguousarray(ops, dtype=np.uint32)
        assert regs.shape[0] == cigs.shape[0]
        return self._sam_call(counts.shape[0], names, quals, comments, rg_id, extra_flag,
                              lambda i, o: self.L.bwagpu_sam_flat(self.h, C.byref(opt), counts.shape[0], seqs.ctypes.data, off.ctypes.data, counts.ctypes.data, regs.ctypes.data,
                                                                  ids.ctypes.data, cigs.ctypes.data, ops.ctypes.data if ops.shape[0] else None, ops.shape[0], i, o))

    def sam_limits(self) -> dict:
        """bwagpu_sam_limits: bytes of a wavefront's staging area (a longer line is flushed in its middle), places of a marked list it takes per step."""
        out = (C.c_int32 * 2)()
        self.L.bwagpu_sam_limits(out)
        return dict(zip(("staging", "step"), list(out)))

    def pair(self, opt: MemOpt, pes: np.ndarray, id0: int = 0):
        """bwagpu_batch_pair: marking, then mem_pair of every pair (reads 2p, 2p + 1) of the last download() on the device; pes = PESTAT_DTYPE[4], read i has
        id id0 + i (id0 even).  -> (PAIR_DTYPE[n pairs], PRIMARY_DTYPE records as primary() returns them, n_pri int32[n reads], device time of the kernels in ms)"""
        pes = np.ascontiguousarray(pes, dtype=PESTAT_DTYPE)
        assert pes.shape == (4,)
        pp, npairs, pr, nr, ms = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_int64(), C.c_float()
        n_pri = np.zeros(self._n, dtype=np.int32)
        self._chk(self.L.bwagpu_batch_pair(self.h, C.byref(opt), pes.ctypes.data, int(id0), C.byref(pp), C.byref(npairs), C.byref(pr), C.byref(nr), n_pri.ctypes.data, C.byref(ms)))
        return self._take(pp, npairs.value, PAIR_DTYPE), self._take(pr, nr.value, PRIMARY_DTYPE), n_pri, ms.value

    def pair_flat(self, opt: MemOpt, pes: np.ndarray, counts: np.ndarray, n_pri: np.ndarray, regs: np.ndarray, ids: np.ndarray):
        """bwagpu_pair_flat: the pairing kernels on marked lists of the caller (reads 2p, 2p + 1: counts[] records of regs each, of which the first n_pri[]
        take part; pair p has id ids[p]) -> (PAIR_DTYPE[n pairs], ms)."""
        pes = np.ascontiguousarray(pes, dtype=PESTAT_DTYPE)
        counts, regs = self._flat_lists(counts, regs)
        n_pri = np.ascontiguousarray(n_pri, dtype=np.int32)
        ids = np.ascontiguousarray(ids, dtype=np.int64)      # (one per pair)
        assert pes.shape == (4,) and counts.shape == n_pri.shape == (2 * ids.shape[0],)
        p, ms = C.c_void_p(), C.c_float()
        self._chk(self.L.bwagpu_pair_flat(self.h, C.byref(opt), pes.ctypes.data, ids.shape[0], counts.ctypes.data, n_pri.ctypes.data, regs.ctypes.data, ids.ctypes.data, C.byref(p), C.byref(ms)))
        return self._take(p, ids.shape[0], PAIR_DTYPE), ms.value

    def pair_limits(self) -> dict:
        """bwagpu_pair_limits: the numbers of hits at which the pairing kernels change their form, as compiled."""
        out = (C.c_int32 * 3)()
        self.L.bwagpu_pair_limits(out)
        return dict(zip(("lane_max", "lds_small", "lds_big"), list(out)))

    def _rescue_out(self, n, counts, pr, ps, nr, prec, ppri, n_pri, ppair, ms, want_pri, want_pairs):
        out = dict(counts=counts, regs=self._take(pr, nr.value, ALNREG_DTYPE), src=self._take(ps, nr.value, np.dtype("<i4")), rescue=self._take(prec, n // 2, RESCUE_DTYPE), ms=ms.value)
        if want_pri:
            out["pri"] = self._take(ppri, nr.value, PRIMARY_DTYPE); out["n_pri"] = n_pri
        if want_pairs:
            out["pairs"] = self._take(ppair, n // 2, PAIR_DTYPE)
        return out

    def rescue(self, opt: MemOpt, pes: np.ndarray, id0: int = 0, pri: bool = True, pairs: bool = True) -> dict:
        """bwagpu_batch_rescue: mem_matesw's decision loop and merge for every pair (reads 2p, 2p + 1) of the last download() on the device, then (pri) the marking of the
        merged lists and (pairs) mem_pair on those records; pes = PESTAT_DTYPE[4], read i has id id0 + i (id0 even).  -> dict: counts int32[n reads], regs (the merged lists),
        src int32 per merged region (index in the downloaded list, or -1 - (j << 2 | r) for a rescued hit), rescue RESCUE_DTYPE[n pairs], ms; pri, n_pri; pairs."""
        pes = np.ascontiguousarray(pes, dtype=PESTAT_DTYPE)
        assert pes.shape == (4,)
        counts, n_pri = np.zeros(self._n, dtype=np.int32), np.zeros(self._n, dtype=np.int32)
        pr, ps, nr, prec, ppri, ppair, ms = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_float()
        self._chk(self.L.bwagpu_batch_rescue(self.h, C.byref(opt), pes.ctypes.data, int(id0), counts.ctypes.data, C.byref(pr), C.byref(ps), C.byref(nr), C.byref(prec),
                                             C.byref(ppri) if pri else None, n_pri.ctypes.data if pri else None, C.byref(ppair) if pairs else None, C.byref(ms)))
        return self._rescue_out(self._n, counts, pr, ps, nr, prec, ppri, n_pri, ppair, ms, pri, pairs)

    def rescue_flat(self, opt: MemOpt, pes: np.ndarray, seqs: np.ndarray, off: np.ndarray, counts_in: np.ndarray, regs_in: np.ndarray, ids=None, pri: bool = True, pairs: bool = True) -> dict:
        """bwagpu_rescue_flat: the same kernels on reads (nt4, read i at seqs[off[i]:off[i + 1]]) and region lists of the caller; ids: one per read (needed for pri / pairs)."""
        pes = np.ascontiguousarray(pes, dtype=PESTAT_DTYPE)
        if ids is None:
            pri = pairs = False
            counts_in, regs_in = self._flat_lists(counts_in, regs_in)
        else:
            counts_in, regs_in, ids = self._flat_lists(counts_in, regs_in, ids)
        n = counts_in.shape[0]
        seqs, off = self._flat_reads(seqs, off, n)
        assert pes.shape == (4,) and n % 2 == 0
        counts, n_pri = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        pr, ps, nr, prec, ppri, ppair, ms = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_float()
        self._chk(self.L.bwagpu_rescue_flat(self.h, C.byref(opt), pes.ctypes.data, n // 2, seqs.ctypes.data, off.ctypes.data, counts_in.ctypes.data, regs_in.ctypes.data,
                                            ids.ctypes.data if ids is not None else None, counts.ctypes.data, C.byref(pr), C.byref(ps), C.byref(nr), C.byref(prec),
                                            C.byref(ppri) if pri else None, n_pri.ctypes.data if pri else None, C.byref(ppair) if pairs else None, C.byref(ms)))
        return self._rescue_out(n, counts, pr, ps, nr, prec, ppri, n_pri, ppair, ms, pri, pairs)

    def rescue_limits(self) -> dict:
        """bwagpu_rescue_limits: the capacities of a pair's larger end at which the rescue kernels change their form, as compiled."""
        out = (C.c_int32 * 4)()
        self.L.bwagpu_rescue_limits(out)
        return dict(zip(("lane_max", "lds_max"), list(out)[:2]))

    def _pe_out(self, n, counts, o):
        m = int(o.n_regs)
        return dict(counts=counts, regs=self._take(C.c_void_p(o.regs), m, ALNREG_DTYPE), src=self._take(C.c_void_p(o.src), m, np.dtype("<i4")), rescue=self._take(C.c_void_p(o.rescue), n // 2, RESCUE_DTYPE),
                    pri=self._take(C.c_void_p(o.pri), m, PRIMARY_DTYPE), n_pri=self._take(C.c_void_p(o.n_pri), n, np.dtype("<i4")), pairs=self._take(C.c_void_p(o.pairs), n // 2, PAIR_DTYPE),
                    sampe=self._take(C.c_void_p(o.sampe), n // 2, SAMPE_DTYPE), cigs=self._take(C.c_void_p(o.cigs), m, CIGAR_DTYPE), ops=self._take(C.c_void_p(o.ops), int(o.n_ops), np.dtype("<u4")),
                    alns=self._take(C.c_void_p(o.alns), m, ALN_DTYPE), n_aln=self._take(C.c_void_p(o.n_aln), n, np.dtype("<i4")), kernel_ms=list(o.kernel_ms), ms=float(sum(o.kernel_ms)))

    def sampe(self, opt: MemOpt, pes: np.ndarray, id0: int = 0) -> dict:
        """bwagpu_batch_sampe: every pair (reads 2p, 2p + 1) of the last download() decided on the device -- rescue(), then the SAMPE_DTYPE record of every pair, the marking
        records as mem_sam_pe leaves the lists, a CIGAR record and an ALN_DTYPE record per merged region.  -> dict: what rescue() returns (pri patched), sampe, cigs, ops, alns,
        n_aln, kernel_ms (six segments), ms (their sum)."""
        pes = np.ascontiguousarray(pes, dtype=PESTAT_DTYPE)
        assert pes.shape == (4,)
        counts, o = np.zeros(self._n, dtype=np.int32), PeOut()
        self._chk(self.L.bwagpu_batch_sampe(self.h, C.byref(opt), pes.ctypes.data, int(id0), counts.ctypes.data, C.byref(o)))
        return self._pe_out(self._n, counts, o)

    def sampe_flat(self, opt: MemOpt, pes: np.ndarray, seqs: np.ndarray, off: np.ndarray, counts_in: np.ndarray, regs_in: np.ndarray, ids: np.ndarray) -> dict:
        """bwagpu_sampe_flat: the same kernels on reads and region lists of the caller (the inputs of rescue_flat; ids: one per read)."""
        pes = np.ascontiguousarray(pes, dtype=PESTAT_DTYPE)
        counts_in, regs_in, ids = self._flat_lists(counts_in, regs_in, ids)
        n = counts_in.shape[0]
        seqs, off = self._flat_reads(seqs, off, n)
        assert pes.shape == (4,) and n % 2 == 0
        counts, o = np.zeros(n, dtype=np.int32), PeOut()
        self._chk(self.L.bwagpu_sampe_flat(self.h, C.byref(opt), pes.ctypes.data, n // 2, seqs.ctypes.data, off.ctypes.data, counts_in.ctypes.data, regs_in.ctypes.data, ids.ctypes.data,
                                           counts.ctypes.data, C.byref(o)))
        return self._pe_out(n, counts, o)

    def sampe_limits(self) -> dict:
        """bwagpu_sampe_limits: the length of a pair's longer list up to which one lane decides the pair, and the places a wavefront takes per step."""
        out = (C.c_int32 * 2)()
        self.L.bwagpu_sampe_limits(out)
        return dict(zip(("lane_max", "step"), list(out)))

    # -- SAM text on the device (paired-end) ------------------------------------------------------------------
    def sam_pe(self, opt: MemOpt, pes: np.ndarray, id0, names, quals=None, comments=None, rg_id=None, extra_flag=0, want_records=False) -> dict:
        """bwagpu_batch_sam_pe: after download(), sampe()'s kernels and then the SAM text of every read of the batch (reads 2p, 2p + 1 are mates and carry one
        name), written on the device from the records those kernels left there.  names, quals, comments: one per READ, as in sam().  A pair is declined as a whole
        (bit 0 of both reads' flag words).  -> the dictionary of sam() (kernel_ms[0]: the sum of sampe()'s six segments), and with want_records the dictionary of
        sampe() under "pe"; without, no alignment or marking record comes to the host."""
        pes = np.ascontiguousarray(pes, dtype=PESTAT_DTYPE)
        assert pes.shape == (4,)
        counts, o = np.zeros(self._n, dtype=np.int32), PeOut()
        res = self._sam_call(self._n, names, quals, comments, rg_id, extra_flag,
                             lambda i, so: self.L.bwagpu_batch_sam_pe(self.h, C.byref(opt), pes.ctypes.data, int(id0), i, counts.ctypes.data, C.byref(o) if want_records else None, so))
        if want_records:
            res["pe"] = self._pe_out(self._n, counts, o)
        return res

    def sam_pe_flat(self, opt: MemOpt, pes: np.ndarray, seqs, off, counts_in, regs_in, ids, names, quals=None, comments=None, rg_id=None, extra_flag=0, want_records=False) -> dict:
        """bwagpu_sam_pe_flat: the same kernels on reads and region lists of the caller (the inputs of sampe_flat) -> as sam_pe()."""
        pes = np.ascontiguousarray(pes, dtype=PESTAT_DTYPE)
        counts_in, regs_in, ids = self._flat_lists(counts_in, regs_in, ids)
        n = counts_in.shape[0]
        seqs, off = self._flat_reads(seqs, off, n)
        assert pes.shape == (4,) and n % 2 == 0
        counts, o = np.zeros(n, dtype=np.int32), PeOut()
        res = self._sam_call(n, names, quals, comments, rg_id, extra_flag,
                             lambda i, so: self.L.bwagpu_sam_pe_flat(self.h, C.byref(opt), pes.ctypes.data, n // 2, seqs.ctypes.data, off.ctypes.data, counts_in.ctypes.data, regs_in.ctypes.data,
                                                                     ids.ctypes.data, i, counts.ctypes.data, C.byref(o) if want_records else None, so))
        if want_records:
            res["pe"] = self._pe_out(n, counts, o)
        return res

    def sam_pe_limits(self) -> dict:
        """bwagpu_sam_pe_limits: as sam_limits()."""
        out = (C.c_int32 * 2)()
        self.L.bwagpu_sam_pe_limits(out)
        return dict(zip(("staging", "step"), list(out)))

    def pestat(self, opt: MemOpt):
        """bwagpu_batch_pestat: mem_pestat of the last download() on the device (reads 2p, 2p + 1 are mates).
        -> (PESTAT_DTYPE[4], byte for byte the reference's mem_pestat_t[4]; one PESTAT_INFO_DTYPE record; device time of the kernels in ms)"""
        pes, info, ms = np.zeros(4, dtype=PESTAT_DTYPE), np.zeros(1, dtype=PESTAT_INFO_DTYPE), C.c_float()
        self._chk(self.L.bwagpu_batch_pestat(self.h, C.byref(opt), pes.ctypes.data, info.ctypes.data, C.byref(ms)))
        return pes, info[0], ms.value

    def pestat_flat(self, opt: MemOpt, counts: np.ndarray, regs: np.ndarray):
        """bwagpu_pestat_flat: the same kernels on region lists of the caller (read i: counts[i] records of regs) -> (pes, info, ms)."""
        counts, regs = self._flat_lists(counts, regs)
        pes, info, ms = np.zeros(4, dtype=PESTAT_DTYPE), np.zeros(1, dtype=PESTAT_INFO_DTYPE), C.c_float()
        self._chk(self.L.bwagpu_pestat_flat(self.h, C.byref(opt), counts.shape[0], counts.ctypes.data, regs.ctypes.data, pes.ctypes.data, info.ctypes.data, C.byref(ms)))
        return pes, info[0], ms.value

    def pestat_hist(self, opt: MemOpt):
        """bwagpu_batch_pestat_hist: the insert-size histogram of the last download(), uint32[4, max_ins + 1] by orientation; histograms of shards add.  -> (hist, ms)"""
        p, n, ms = C.c_void_p(), C.c_int64(), C.c_float()
        self._chk(self.L.bwagpu_batch_pestat_hist(self.h, C.byref(opt), C.byref(p), C.byref(n), C.byref(ms)))
        return self._take(p, n.value, np.dtype("<u4")).reshape(4, -1), ms.value

    def pestat_finish(self, opt: MemOpt, hist: np.ndarray):
        """bwagpu_pestat_finish: the windows from a histogram (of one handle, or the sum of several handles') -> (pes, info, ms)."""
        hist = np.ascontiguousarray(hist, dtype=np.uint32)
        pes, info, ms = np.zeros(4, dtype=PESTAT_DTYPE), np.zeros(1, dtype=PESTAT_INFO_DTYPE), C.c_float()
        self._chk(self.L.bwagpu_pestat_finish(self.h, C.byref(opt), hist.ctypes.data, hist.size, pes.ctypes.data, info.ctypes.data, C.byref(ms)))
        return pes, info[0], ms.value

    def pestat_limits(self) -> dict:
        """bwagpu_pestat_limits: MIN_DIR_CNT and the largest max_ins the device histogram serves, as compiled."""
        out = (C.c_int32 * 2)()
        self.L.bwagpu_pestat_limits(out)
        return dict(zip(("min_dir_cnt", "max_ins"), list(out)))

    def debug_dp(self, opt: MemOpt, kind: int, cases: np.ndarray, seqs: np.ndarray) -> np.ndarray:
        """bwagpu_debug_dp: one wavefront of a device DP routine per case (DP_CASE_DTYPE) -> int32[n_cases, 72]."""
        cases = np.ascontiguousarray(cases, dtype=DP_CASE_DTYPE)
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        out = np.zeros((cases.shape[0], 72), dtype=np.int32)
        self._chk(self.L.bwagpu_debug_dp(self.h, C.byref(opt), kind, cases.shape[0], cases.ctypes.data, seqs.ctypes.data, seqs.shape[0], out.ctypes.data))
        return out

    def debug_sort_limits(self) -> dict:
        """bwagpu_debug_sort_limits: the sizes at which the library's sorts change their method, as compiled."""
        out = (C.c_int32 * 8)()
        self.L.bwagpu_debug_sort_limits(out)
        return dict(zip(("pub_max", "cw_pw_lds", "cw_flt_lds", "dedup_keysort_min", "par_cap_max", "chain_sort_lane_max", "dd_net_default"), list(out)))

    def debug_sort(self, kind: int, keys: np.ndarray, off: np.ndarray, dd_net: int = 129, par_cap: int = 128, chain_flt_lds: int = 256):
        """bwagpu_debug_sort: one of the device's sorts on every case keys[off[k]:off[k + 1]] (SORT_KEY_DTYPE) -> (perm int32[len(keys)], status int32[n_cases])."""
        keys = np.ascontiguousarray(keys, dtype=SORT_KEY_DTYPE)
        off = np.ascontiguousarray(off, dtype=np.int64)
        assert off.shape[0] >= 1 and int(off[-1]) == keys.shape[0]
        perm = np.full(keys.shape[0], -1, dtype=np.int32)
        status = np.full(off.shape[0] - 1, -1, dtype=np.int32)
        self._chk(self.L.bwagpu_debug_sort(self.h, kind, off.shape[0] - 1, keys.ctypes.data, off.ctypes.data, dd_net, par_cap, chain_flt_lds, perm.ctypes.data, status.ctypes.data))
        return perm, status

    def align(self, opt: MemOpt, seqs: np.ndarray, off: np.ndarray):
        self.upload(seqs, off)
        self.run(opt)
        return self.download()

    # -- taps -------------------------------------------------------------------------------------------------
    def tap_intervals(self):
        counts = np.zeros(self._n, dtype=np.int32)
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.bwagpu_tap_intervals(self.h, counts.ctypes.data, C.byref(p), C.byref(n)))
        return counts, self._take(p, n.value, INTV3_DTYPE)

    def tap_chains(self):
        counts = np.zeros(self._n, dtype=np.int32)
        pc, nc, ps, ns = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_int64()
        self._chk(self.L.bwagpu_tap_chains(self.h, counts.ctypes.data, C.byref(pc), C.byref(nc), C.byref(ps), C.byref(ns)))
        return counts, self._take(pc, nc.value, GCHAIN_DTYPE), self._take(ps, ns.value, GSEED_DTYPE)

    def tap_regs_raw(self):
        counts = np.zeros(self._n, dtype=np.int32)
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.bwagpu_tap_regs_raw(self.h, counts.ctypes.data, C.byref(p), C.byref(n)))
        return counts, self._take(p, n.value, ALNREG_DTYPE)


FASTQ_REC_DTYPE = np.dtype([("file", "<i4"), ("has_comment", "<i4"), ("name", "<i4"), ("l_name", "<i4"), ("comment", "<i4"), ("l_comment", "<i4"),
                            ("seq", "<i4"), ("l_seq", "<i4"), ("qual", "<i4"), ("l_qual", "<i4")])   # bwagpu_fastq_rec_t
assert FASTQ_REC_DTYPE.itemsize == 40
FQ_CUT, FQ_END, FQ_MORE, FQ_DECLINED, FQ_DAMAGED = 0, 1, 2, 3, 4


class FastqOut(C.Structure):
    """bwagpu_fastq_out_t"""
    _fields_ = [("status", C.c_int32), ("n_reads", C.c_int32), ("consumed", C.c_int64 * 2), ("declined_file", C.c_int32), ("declined_at", C.c_int64),
                ("seqs", C.c_void_p), ("off", C.c_void_p), ("names", C.c_void_p), ("name_off", C.c_void_p), ("quals", C.c_void_p),
                ("comments", C.c_void_p), ("comment_off", C.c_void_p), ("has_comment", C.c_void_p), ("recs", C.c_void_p), ("kernel_ms", C.c_float * 3)]


class FastqSmart(C.Structure):
    """bwagpu_fastq_smart_t"""
    _fields_ = [("status", C.c_int32), ("n_reads", C.c_int32), ("consumed", C.c_int64), ("declined_at", C.c_int64), ("cls", C.c_void_p),
                ("n_sub", C.c_int32 * 2), ("idx", C.c_void_p * 2), ("sub", FastqOut * 2), ("kernel_ms", C.c_float * 4)]


class BgzfWin(C.Structure):
    """bwagpu_bgzf_win_t"""
    _fields_ = [("comp", C.c_void_p), ("comp_len", C.c_int64), ("skip", C.c_int32), ("eof", C.c_int32)]


class BgzfInfo(C.Structure):
    """bwagpu_bgzf_info_t"""
    _fields_ = [("used_comp", C.c_int64), ("inflated", C.c_int64), ("n_blocks", C.c_int32), ("next_coff", C.c_int64), ("next_uoff", C.c_int32),
                ("damaged_at", C.c_int64), ("inflate_ms", C.c_float)]

    def as_dict(self) -> dict:
        return {k: (float(getattr(self, k)) if k == "inflate_ms" else int(getattr(self, k))) for k, _ in self._fields_}


class BgzfOutInfo(C.Structure):
    """bwagpu_bgzf_out_info_t"""
    _fields_ = [("n_blocks", C.c_int64), ("text_len", C.c_int64), ("comp_len", C.c_int64), ("deflate_ms", C.c_float)]

    def as_dict(self) -> dict:
        return {k: (float(getattr(self, k)) if k == "deflate_ms" else int(getattr(self, k))) for k, _ in self._fields_}


class FastqParser:
    """The device FASTQ reader (bwagpu_fastq_*): windows of FASTQ text in, the batch bseq_read would cut from them out.  It needs no index.
    lib_path selects another build of the library (the CPU tests pass the mock-runtime one); there is no CPU implementation."""

    def __init__(self, device: int = 0, lib_path: str | None = None):
        self.L = L = load_library(lib_path)
        P = C.c_void_p
        L.bwagpu_fastq_begin.argtypes = [C.POINTER(P), C.c_int, C.c_char_p, C.c_size_t]
        L.bwagpu_fastq_reserve.argtypes = [P, C.c_int64]
        L.bwagpu_fastq_batch.argtypes = [P, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]
        L.bwagpu_bgzf_inflate.argtypes = [P, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
        L.bwagpu_fastq_batch_bgzf.argtypes = [P, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.bwagpu_bgzf_deflate.argtypes = [P, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.bwagpu_bgzf_out_limits.argtypes = [C.c_void_p]
        L.bwagpu_bgzf_out_limits.restype = None
        L.bwagpu_fastq_batch_fasta.argtypes = L.bwagpu_fastq_batch.argtypes
        L.bwagpu_fastq_batch_fasta_bgzf.argtypes = L.bwagpu_fastq_batch_bgzf.argtypes
        L.bwagpu_fasta_reads_limits.argtypes = [C.c_void_p]
        L.bwagpu_fasta_reads_limits.restype = None
        L.bwagpu_fastq_batch_smart.argtypes = [P, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]
        L.bwagpu_fastq_batch_smart_bgzf.argtypes = [P, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.bwagpu_fastq_smart_free.argtypes = [C.c_void_p]
        L.bwagpu_fastq_smart_free.restype = None
        L.bwagpu_fastq_out_free.argtypes = [C.c_void_p]
        L.bwagpu_fastq_out_free.restype = None
        L.bwagpu_fastq_end.argtypes = [P]
        L.bwagpu_fastq_end.restype = None
        L.bwagpu_fastq_last_error.argtypes = [P]
        L.bwagpu_fastq_last_error.restype = C.c_char_p
        assert L.bwagpu_fastq_rec_size() == FASTQ_REC_DTYPE.itemsize
        self.h = P()
        err = C.create_string_buffer(512)
        rc = L.bwagpu_fastq_begin(C.byref(self.h), device, err, 512)
        if rc != 0:
            self.h = P()
            raise BwaGpuError(f"bwagpu_fastq_begin failed: {L.bwagpu_strerror(rc).decode()} {err.value.decode()}")

    def _chk(self, rc, what):
        if rc != 0:
            raise BwaGpuError(f"{what} failed ({rc}): {self.L.bwagpu_strerror(rc).decode()} {self.L.bwagpu_fastq_last_error(self.h).decode()}")

    def reserve(self, window_bytes: int):
        self._chk(self.L.bwagpu_fastq_reserve(self.h, int(window_bytes)), "bwagpu_fastq_reserve")

    def batch_rc(self, raw1, len1, eof1, raw2, len2, eof2, chunk_size, out):
        """the bare call (tests of the error paths): returns the library's code"""
        return self.L.bwagpu_fastq_batch(self.h, raw1, len1, eof1, raw2, len2, eof2, chunk_size, out)

    def batch_fasta_rc(self, raw1, len1, eof1, raw2, len2, eof2, chunk_size, out):
        """the bare call (tests of the error paths): returns the library's code"""
        return self.L.bwagpu_fastq_batch_fasta(self.h, raw1, len1, eof1, raw2, len2, eof2, chunk_size, out)

    def batch_fasta(self, raw1, raw2=None, chunk_size: int = 10_000_000, eof=(True, True)) -> dict:
        """batch() for windows of FASTA text, each starting at a '>' (bwagpu_fastq_batch_fasta).  The same dict; quals is None."""
        return self.batch(raw1, raw2, chunk_size, eof, _call="bwagpu_fastq_batch_fasta")

    def fasta_reads_limits(self) -> dict:
        """bwagpu_fasta_reads_limits: the sizes at which the FASTA reader's kernels change their step, as compiled."""
        out = (C.c_int32 * 4)()
        self.L.bwagpu_fasta_reads_limits(out)
        return dict(zip(("tile_bytes", "lane_bytes", "emit_step_bytes"), list(out)))

    def batch(self, raw1, raw2=None, chunk_size: int = 10_000_000, eof=(True, True), _call="bwagpu_fastq_batch") -> dict:
        """raw1 / raw2: bytes-like windows, each starting at a record start (raw2 None: one file).  Returns a dict with status (FQ_*),
        n_reads, consumed, declined_file, declined_at, kernel_ms and -- for FQ_CUT / FQ_END -- copies of the arrays: seqs (nt4), off,
        names, name_off, quals, comments, comment_off, has_comment, recs."""
        b1 = np.frombuffer(raw1, dtype=np.uint8) if len(raw1) else np.zeros(1, dtype=np.uint8)
        b2 = None if raw2 is None else (np.frombuffer(raw2, dtype=np.uint8) if len(raw2) else np.zeros(1, dtype=np.uint8))
        o = FastqOut()
        rc = getattr(self.L, _call)(self.h, b1.ctypes.data, len(raw1), int(bool(eof[0])), None if b2 is None else b2.ctypes.data,
                                    0 if raw2 is None else len(raw2), int(bool(eof[1])), int(chunk_size), C.byref(o))
        self._chk(rc, _call)
        return self._result(o)

    @staticmethod
    def _take(ptr, count, dtype):
        if count == 0:
            return np.zeros(0, dtype=dtype)
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(count * np.dtype(dtype).itemsize,)).view(dtype).copy()

    def _arrays(self, o, r):
        """copies of a FastqOut's arrays into r"""
        n, take = int(o.n_reads), self._take
        for k in ("off", "name_off", "comment_off"):
            r[k] = take(getattr(o, k), n + 1, np.int64)
        r["seqs"] = take(o.seqs, int(r["off"][n]), np.uint8)
        r["quals"] = take(o.quals, int(r["off"][n]), np.uint8).tobytes() if o.quals else None      # (None: FASTA reads)
        r["names"] = take(o.names, int(r["name_off"][n]), np.uint8).tobytes()
        r["comments"] = take(o.comments, int(r["comment_off"][n]), np.uint8).tobytes()
        r["has_comment"] = take(o.has_comment, n, np.uint8)
        r["recs"] = take(o.recs, n, FASTQ_REC_DTYPE)

    def _result(self, o) -> dict:
        """a filled FastqOut as a dict of copies; the library's arrays are released"""
        r = {"status": int(o.status), "n_reads": int(o.n_reads), "consumed": (int(o.consumed[0]), int(o.consumed[1])),
             "declined_file": int(o.declined_file), "declined_at": int(o.declined_at), "kernel_ms": tuple(float(x) for x in o.kernel_ms)}
        try:
            if o.status in (FQ_CUT, FQ_END):
                self._arrays(o, r)
        finally:
            self.L.bwagpu_fastq_out_free(C.byref(o))
        return r

    def _result_smart(self, o) -> dict:
        """a filled FastqSmart as a dict of copies; the library's arrays are released"""
        r = {"status": int(o.status), "n_reads": int(o.n_reads), "consumed": int(o.consumed), "declined_at": int(o.declined_at),
             "kernel_ms": tuple(float(x) for x in o.kernel_ms)}
        try:
            if o.status in (FQ_CUT, FQ_END):
                r["cls"] = self._take(o.cls, int(o.n_reads), np.uint8)
                r["n_sub"] = (int(o.n_sub[0]), int(o.n_sub[1]))
                r["idx"] = [self._take(o.idx[k], int(o.n_sub[k]), np.int32) for k in range(2)]
                r["sub"] = []
                for k in range(2):
                    d = {"n_reads": int(o.sub[k].n_reads)}
                    self._arrays(o.sub[k], d)
                    r["sub"].append(d)
        finally:
            self.L.bwagpu_fastq_smart_free(C.byref(o))
        return r

    def batch_smart_rc(self, raw, length, eof, chunk_size, out):
        """the bare call (tests of the error paths): returns the library's code"""
        return self.L.bwagpu_fastq_batch_smart(self.h, raw, length, eof, chunk_size, out)

    def batch_smart(self, raw, chunk_size: int = 10_000_000, eof: bool = True) -> dict:
        """raw: a bytes-like window of ONE file of interleaved reads (`mem -p`), starting at a record start.  Returns a dict with the whole
        batch's status (FQ_*), n_reads, consumed, declined_at, kernel_ms and -- for FQ_CUT / FQ_END -- cls (0 single, 1 first of a pair,
        2 second), n_sub, idx (per sub-batch: the reads' places in the batch) and sub: two dicts (single reads, pairs) with n_reads and
        batch()'s arrays."""
        b = np.frombuffer(raw, dtype=np.uint8) if len(raw) else np.zeros(1, dtype=np.uint8)
        o = FastqSmart()
        self._chk(self.L.bwagpu_fastq_batch_smart(self.h, b.ctypes.data, len(raw), int(bool(eof)), int(chunk_size), C.byref(o)), "bwagpu_fastq_batch_smart")
        return self._result_smart(o)

    def batch_smart_bgzf_rc(self, w, chunk_size, out, info):
        """the bare call (tests of the error paths): returns the library's code"""
        return self.L.bwagpu_fastq_batch_smart_bgzf(self.h, w, chunk_size, out, info)

    def batch_smart_bgzf(self, comp, skip: int = 0, chunk_size: int = 10_000_000, eof: bool = True) -> dict:
        """comp: a bytes-like window of BGZF data that starts at a block start; skip: bytes of its first block's text that earlier batches
        consumed.  Returns batch_smart()'s dict plus "bgzf": the window's info dict (bwagpu_bgzf_info_t's fields)."""
        b = np.frombuffer(comp, dtype=np.uint8) if len(comp) else np.zeros(1, dtype=np.uint8)
        w = BgzfWin(b.ctypes.data, len(comp), int(skip), int(bool(eof)))
        o = FastqSmart()
        info = BgzfInfo()
        self._chk(self.L.bwagpu_fastq_batch_smart_bgzf(self.h, C.byref(w), int(chunk_size), C.byref(o), C.byref(info)), "bwagpu_fastq_batch_smart_bgzf")
        r = self._result_smart(o)
        r["bgzf"] = info.as_dict()
        return r

    def inflate_bgzf(self, data, eof: bool = True):
        """data: BGZF bytes that start at a block start.  Returns (text of the whole blocks taken, info dict); the text is None when a block
        is damaged (info["damaged_at"] >= 0).  info has bwagpu_bgzf_info_t's fields."""
        b = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
        total = 0
        info = BgzfInfo()
        dst = np.zeros(1, dtype=np.uint8)
        for _ in range(2):      # (the first call may only say how much text there is: BWAGPU_EINVAL, inflated set)
            rc = self.L.bwagpu_bgzf_inflate(self.h, b.ctypes.data, len(data), int(bool(eof)), dst.ctypes.data, total, C.byref(info))
            if rc == -2 and info.inflated > total:
                total = int(info.inflated)
                dst = np.zeros(total, dtype=np.uint8)
                continue
            break
        self._chk(rc, "bwagpu_bgzf_inflate")
        d = info.as_dict()
        return (None if d["damaged_at"] >= 0 else dst[:d["inflated"]].tobytes()), d

    def deflate_bgzf_rc(self, text, text_len, block_size, eof_marker, comp, info):
        """the bare call (tests of the error paths): returns the library's code"""
        return self.L.bwagpu_bgzf_deflate(self.h, text, text_len, block_size, eof_marker, comp, info)

    def deflate_bgzf(self, text, block_size: int = 0, eof_marker: bool = True):
        """text: bytes-like.  Returns (the text as a BGZF stream of blocks of block_size text bytes -- 0: 0xff00 --, with bgzip's end-of-file
        block behind them if eof_marker; info dict with bwagpu_bgzf_out_info_t's fields).  The bytes depend on text and block_size alone."""
        b = np.frombuffer(text, dtype=np.uint8) if len(text) else np.zeros(1, dtype=np.uint8)
        comp = C.c_void_p()
        info = BgzfOutInfo()
        self._chk(self.L.bwagpu_bgzf_deflate(self.h, b.ctypes.data, len(text), int(block_size), int(bool(eof_marker)), C.byref(comp), C.byref(info)), "bwagpu_bgzf_deflate")
        try:
            data = C.string_at(comp.value, info.comp_len) if info.comp_len else b""
        finally:
            self.L.bwagpu_free(comp)
        return data, info.as_dict()

    def bgzf_out_limits(self) -> dict:
        """what dev_bgzf_out.h's kernel uses: the largest block text, the shortest and longest match, the largest distance"""
        v = (C.c_int32 * 4)()
        self.L.bwagpu_bgzf_out_limits(v)
        return {"max_block_text": v[0], "min_match": v[1], "max_match": v[2], "max_dist": v[3]}

    def batch_bgzf_rc(self, w1, w2, chunk_size, out, info):
        """the bare call (tests of the error paths): returns the library's code"""
        return self.L.bwagpu_fastq_batch_bgzf(self.h, w1, w2, chunk_size, out, info)

    def batch_fasta_bgzf_rc(self, w1, w2, chunk_size, out, info):
        """the bare call (tests of the error paths): returns the library's code"""
        return self.L.bwagpu_fastq_batch_fasta_bgzf(self.h, w1, w2, chunk_size, out, info)

    def batch_fasta_bgzf(self, c1, c2=None, skip=(0, 0), chunk_size: int = 10_000_000, eof=(True, True)) -> dict:
        """batch_bgzf() for BGZF windows of FASTA text (bwagpu_fastq_batch_fasta_bgzf).  The same dict; quals is None."""
        return self.batch_bgzf(c1, c2, skip, chunk_size, eof, _call="bwagpu_fastq_batch_fasta_bgzf")

    def batch_bgzf(self, c1, c2=None, skip=(0, 0), chunk_size: int = 10_000_000, eof=(True, True), _call="bwagpu_fastq_batch_bgzf") -> dict:
        """c1 / c2: bytes-like windows of BGZF data, each starting at a block start (c2 None: one file); skip[k]: bytes of window k's first
        block's text that earlier batches consumed.  Returns batch()'s dict plus "bgzf": one info dict per window (bwagpu_bgzf_info_t's
        fields).  consumed, declined_at and recs refer to the text window, which exists on the device only."""
        keep, wins = [], []
        for k, c in enumerate((c1, c2)):
            if c is None:
                wins.append(None)
                continue
            b = np.frombuffer(c, dtype=np.uint8) if len(c) else np.zeros(1, dtype=np.uint8)
            keep.append(b)
            wins.append(BgzfWin(b.ctypes.data, len(c), int(skip[k]), int(bool(eof[k]))))
        o = FastqOut()
        info = (BgzfInfo * 2)()
        rc = getattr(self.L, _call)(self.h, C.byref(wins[0]), None if wins[1] is None else C.byref(wins[1]), int(chunk_size), C.byref(o), info)
        self._chk(rc, _call)
        r = self._result(o)
        r["bgzf"] = [info[k].as_dict() for k in range(1 if c2 is None else 2)]
        return r

    def close(self):
        if self.h:
            self.L.bwagpu_fastq_end(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
