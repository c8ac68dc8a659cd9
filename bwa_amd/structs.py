"""Plain-C struct mirrors of the reference's boundary types (ctypes + numpy views).

These are the exact layouts the C-ABI in include/bwagpu.h exchanges; they replicate
mem_opt_t (bwamem.h:52-84, 168 B), mem_alnreg_t (bwamem.h:86-104, 88 B), bwtintv_t (bwt.h:62, 32 B),
mem_pestat_t (bwamem.h:108-112, 32 B).  Sizes are asserted against the compiled reference in tests.
"""
import ctypes as C
import numpy as np


class MemOpt(C.Structure):
    _fields_ = [
        ("a", C.c_int), ("b", C.c_int),
        ("o_del", C.c_int), ("e_del", C.c_int), ("o_ins", C.c_int), ("e_ins", C.c_int),
        ("pen_unpaired", C.c_int), ("pen_clip5", C.c_int), ("pen_clip3", C.c_int),
        ("w", C.c_int), ("zdrop", C.c_int),
        ("max_mem_intv", C.c_uint64),
        ("T", C.c_int), ("flag", C.c_int), ("min_seed_len", C.c_int), ("min_chain_weight", C.c_int),
        ("max_chain_extend", C.c_int), ("split_factor", C.c_float), ("split_width", C.c_int),
        ("max_occ", C.c_int), ("max_chain_gap", C.c_int), ("n_threads", C.c_int), ("chunk_size", C.c_int),
        ("mask_level", C.c_float), ("drop_ratio", C.c_float), ("XA_drop_ratio", C.c_float),
        ("mask_level_redun", C.c_float), ("mapQ_coef_len", C.c_float), ("mapQ_coef_fac", C.c_int),
        ("max_ins", C.c_int), ("max_matesw", C.c_int), ("max_XA_hits", C.c_int), ("max_XA_hits_alt", C.c_int),
        ("mat", C.c_int8 * 25),
    ]


assert C.sizeof(MemOpt) == 168

MEM_F_PE = 0x2

ALNREG_DTYPE = np.dtype([
    ("rb", "<i8"), ("re", "<i8"), ("qb", "<i4"), ("qe", "<i4"), ("rid", "<i4"), ("score", "<i4"),
    ("truesc", "<i4"), ("sub", "<i4"), ("alt_sc", "<i4"), ("csub", "<i4"), ("sub_n", "<i4"), ("w", "<i4"),
    ("seedcov", "<i4"), ("secondary", "<i4"), ("secondary_all", "<i4"), ("seedlen0", "<i4"),
    ("ncomp_isalt", "<u4"),  # n_comp:30 (low bits), is_alt:2 (high bits)
    ("frac_rep", "<f4"), ("hash", "<u8"),
])
assert ALNREG_DTYPE.itemsize == 88

# bwagpu_primary_t: one region as mem_mark_primary_se + mem_approx_mapq_se leave it (bwagpu_batch_primary / bwagpu_primary_flat)
PRIMARY_DTYPE = np.dtype([("src", "<i4"), ("secondary", "<i4"), ("secondary_all", "<i4"), ("sub", "<i4"), ("alt_sc", "<i4"), ("sub_n", "<i4"),
                          ("mapq", "<i4"), ("flags", "<i4")])
assert PRIMARY_DTYPE.itemsize == 32

# bwagpu_aln_t: one region as mem_reg2aln returns it and as mem_reg2sam's loop lists it (bwagpu_batch_alns / bwagpu_alns_flat)
ALN_DTYPE = np.dtype([("pos", "<i8"), ("rid", "<i4"), ("flag", "<i4"), ("mapq", "<i4"), ("mapq_out", "<i4"), ("nm", "<i4"), ("n_cigar", "<i4"), ("score", "<i4"),
                      ("sub", "<i4"), ("alt_sc", "<i4"), ("sel", "<i4"), ("clip5", "<i4"), ("clip3", "<i4"), ("flags", "<i4"), ("pad_", "<i4")])
assert ALN_DTYPE.itemsize == 64
ALN_NOCIGAR, ALN_REV, ALN_ALT, ALN_DEL5, ALN_DEL3 = 0x1, 0x2, 0x4, 0x8, 0x10      # bits of `flags` (BWAGPU_ALN_*)

# bwagpu_pestat_t == mem_pestat_t (4 bytes of padding before the doubles), bwagpu_pair_t: mem_pair's results for one pair (bwagpu_batch_pair / bwagpu_pair_flat)
PESTAT_DTYPE = np.dtype({"names": ["low", "high", "failed", "avg", "std"], "formats": ["<i4", "<i4", "<i4", "<f8", "<f8"], "offsets": [0, 4, 8, 16, 24], "itemsize": 32})
PAIR_DTYPE = np.dtype([("score", "<i4"), ("sub", "<i4"), ("n_sub", "<i4"), ("z", "<i4", (2,)), ("flags", "<i4"), ("n_cand", "<i8")])
assert PESTAT_DTYPE.itemsize == 32 and PAIR_DTYPE.itemsize == 32
# bwagpu_rescue_t: what the merge of mate-rescue hits did with one pair (bwagpu_batch_rescue / bwagpu_rescue_flat)
RESCUE_DTYPE = np.dtype([("n_aligned", "<i4"), ("n_inline", "<i4"), ("flags", "<i4"), ("pad_", "<i4")])
assert RESCUE_DTYPE.itemsize == 16
# bwagpu_sampe_t: a read pair as mem_sam_pe decides it (bwagpu_batch_sampe / bwagpu_sampe_flat); PeOut: bwagpu_pe_out_t, what those calls return
SAMPE_DTYPE = np.dtype([("path", "<i4"), ("why", "<i4"), ("extra_flag", "<i4"), ("z", "<i4", (2,)), ("q_se", "<i4", (2,)), ("alt", "<i4", (2,)), ("n_aa", "<i4", (2,)),
                        ("q_pe", "<i4"), ("paired", "<i4"), ("flags", "<i4"), ("pad_", "<i4", (2,))])
assert SAMPE_DTYPE.itemsize == 64


class PeOut(C.Structure):
    _fields_ = [("regs", C.c_void_p), ("src", C.c_void_p), ("n_regs", C.c_int64), ("rescue", C.c_void_p), ("pri", C.c_void_p), ("n_pri", C.c_void_p), ("pairs", C.c_void_p),
                ("sampe", C.c_void_p), ("cigs", C.c_void_p), ("ops", C.c_void_p), ("n_ops", C.c_int64), ("alns", C.c_void_p), ("n_aln", C.c_void_p), ("kernel_ms", C.c_float * 6)]


INTV_DTYPE = np.dtype([("x0", "<u8"), ("x1", "<u8"), ("x2", "<u8"), ("info", "<u8")])
SEED_DTYPE = np.dtype([("rbeg", "<i8"), ("qbeg", "<i4"), ("len", "<i4"), ("score", "<i4"), ("_pad", "<i4")])
CHAIN_HDR_DTYPE = np.dtype([("n", "<i4"), ("rid", "<i4"), ("w", "<i4"), ("kept", "<i4"), ("is_alt", "<i4"),
                            ("first", "<i4"), ("frac_rep", "<f4"), ("seed_off", "<i4"), ("pos", "<i8")])
assert SEED_DTYPE.itemsize == 24 and CHAIN_HDR_DTYPE.itemsize == 40


class MemPestat(C.Structure):
    _fields_ = [("low", C.c_int), ("high", C.c_int), ("failed", C.c_int), ("avg", C.c_double), ("std", C.c_double)]


assert C.sizeof(MemPestat) == 32 == PESTAT_DTYPE.itemsize and MemPestat.avg.offset == 16

# bwagpu_pestat_info_t: what mem_pestat prints and what its scalars were made from, per orientation
PESTAT_INFO_DTYPE = np.dtype([("n", "<i8", (4,)), ("p25", "<i4", (4,)), ("p50", "<i4", (4,)), ("p75", "<i4", (4,)), ("lo_out", "<i4", (4,)), ("hi_out", "<i4", (4,)),
                              ("x", "<i8", (4,)), ("sum", "<f8", (4,)), ("sumsq", "<f8", (4,))])
assert PESTAT_INFO_DTYPE.itemsize == 208


def default_opt() -> MemOpt:
    """mem_opt_init() defaults (bwamem.c:74-110) incl. bwa_fill_scmat (bwa.c:136-145)."""
    o = MemOpt()
    o.a, o.b = 1, 4
    o.o_del = o.o_ins = 6
    o.e_del = o.e_ins = 1
    o.w, o.T, o.zdrop = 100, 30, 100
    o.pen_unpaired = 17
    o.pen_clip5 = o.pen_clip3 = 5
    o.max_mem_intv = 20
    o.min_seed_len, o.split_width, o.max_occ = 19, 10, 500
    o.max_chain_gap = o.max_ins = 10000
    o.mask_level = o.drop_ratio = 0.5
    o.XA_drop_ratio, o.split_factor = 0.8, 1.5
    o.chunk_size, o.n_threads = 10000000, 1
    o.max_XA_hits, o.max_XA_hits_alt, o.max_matesw = 5, 200, 50
    o.mask_level_redun = 0.95
    o.min_chain_weight, o.max_chain_extend = 0, 1 << 30
    o.mapQ_coef_len, o.mapQ_coef_fac = 50.0, 3
    fill_scmat(o)
    return o


def fill_scmat(o: MemOpt):
    k = 0
    for i in range(4):
        for j in range(4):
            o.mat[k] = o.a if i == j else -o.b
            k += 1
        o.mat[k] = -1
        k += 1
    for _ in range(5):
        o.mat[k] = -1
        k += 1


def pacbio_opt() -> MemOpt:
    """`-x pacbio` preset (fastmap.c:337-345) followed by update_a with a == 1 (no rescale)."""
    o = default_opt()
    o.o_del = o.o_ins = 1
    o.e_del = o.e_ins = 1
    o.b = 1
    o.split_factor = 10.0
    o.pen_clip5 = o.pen_clip3 = 0
    o.min_seed_len = 17
    o.min_chain_weight = 40
    fill_scmat(o)
    return o


# bwagpu_sam_in_t / bwagpu_sam_out_t: bwagpu_batch_sam / bwagpu_sam_flat (SAM text written on the device)
class SamIn(C.Structure):
    _fields_ = [("names", C.c_void_p), ("name_off", C.c_void_p), ("quals", C.c_void_p), ("comments", C.c_void_p), ("comment_off", C.c_void_p), ("rg_id", C.c_char_p),
                ("extra_flag", C.c_int32)]


class SamOut(C.Structure):
    _fields_ = [("text", C.c_void_p), ("n_text", C.c_int64), ("off", C.c_void_p), ("flags", C.c_void_p), ("n_lines", C.c_void_p), ("n_declined", C.c_int64),
                ("kernel_ms", C.c_float * 3)]


assert C.sizeof(SamIn) == 56 and C.sizeof(SamOut) == 64
