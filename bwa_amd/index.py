"""Index construction on the device: writes <prefix>.{bwt,sa,pac,ann,amb} byte-identical to what the
reference's `bwa index` produces (bwtindex.c:255-323), in seconds instead of ~0.5-0.7 s/Mbp.

The work is done by `bwagpu_index_build` (include/bwagpu.h, bwa_amd/csrc/bwagpu_index.hip): a suffix sort of the
forward + reverse-complement text in HBM (bucketed 64-bit radix sort of 32-mers, then prefix doubling restricted to the
still-unsorted suffixes), followed by streaming kernels that lay out the BWT, its Occ checkpoints and the sampled SA the way
bwt_bwtupdate_core / bwt_cal_sa leave them.  This module is the ctypes binding plus the writers of the reference's on-disk
formats:
  .bwt  primary, L2[1..4], then bwt_t::bwt (bwt_dump_bwt, bwt.c:385-393)
  .sa   primary, L2[1..4], sa_intv, seq_len, then SA[k] for k = sa_intv, 2 sa_intv, ... (bwt_dump_sa, bwt.c:396-407)
  .pac  2 bits per base of the forward strand, tail bytes as bns_fasta2bntseq writes them (bntseq.c:314-323)
  .ann / .amb  text (bns_dump, bntseq.c:65-95)
There is no CPU implementation: without libbwagpu.so and a GPU the call raises (the CPU test-suite runs the same HIP source
under the mock runtime of tests/hostsim by passing its library as `lib_path`).
Equality with `bwa index` output is asserted in tests/test_index_build.py (CPU, mock runtime) and tests/test_gpu_index.py.
"""
from __future__ import annotations

import ctypes as C
import gzip
import os

import numpy as np

from .api import BwaGpuError, load_library


class Built(C.Structure):
    """bwagpu_built_t"""
    _fields_ = [("bwt", C.POINTER(C.c_uint32)), ("bwt_size", C.c_uint64), ("sa", C.POINTER(C.c_uint64)), ("n_sa", C.c_uint64),
                ("sa_intv", C.c_int), ("primary", C.c_uint64), ("L2", C.c_uint64 * 5), ("seq_len", C.c_uint64), ("build_ms", C.c_float)]


def pack_pac(codes: np.ndarray) -> np.ndarray:
    """2-bit packing of the forward strand, base l in byte l >> 2 at bits (3 - l % 4) * 2 (bntseq.c:229); l_pac/4 + 1 bytes."""
    l_pac = int(codes.shape[0])
    # an ambiguity code left in the array would be OR-ed into its neighbours' bits: the caller replaces Ns first (bns_fasta2bntseq
    # does, bntseq.c:266,295-296) and lists them as holes
    if l_pac and int(codes.max()) > 3:
        raise ValueError("pack_pac: base codes must be 0..3 (replace ambiguity codes first and pass them to write_pac_ann_amb as holes)")
    out = np.zeros(l_pac // 4 + 1, dtype=np.uint8)
    full = l_pac // 4 * 4
    if full:
        c4 = codes[:full].reshape(-1, 4)
        out[: full // 4] = (c4[:, 0] << 6) | (c4[:, 1] << 4) | (c4[:, 2] << 2) | c4[:, 3]
    for k in range(full, l_pac):
        out[k >> 2] |= int(codes[k]) << ((3 - (k & 3)) * 2)
    return out


def build_arrays(pac: np.ndarray, l_pac: int, sa_intv: int = 32, device: int = 0, lib_path: str | None = None):
    """Run the device builder; returns (Built struct, library) -- the caller frees with L.bwagpu_built_free."""
    L = load_library(lib_path)
    L.bwagpu_index_build.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_char_p, C.c_size_t]
    L.bwagpu_built_free.argtypes = [C.c_void_p]
    pac = np.ascontiguousarray(pac, dtype=np.uint8)
    assert pac.shape[0] >= l_pac // 4 + 1
    b = Built()
    err = C.create_string_buffer(512)
    rc = L.bwagpu_index_build(pac.ctypes.data, l_pac, sa_intv, device, C.byref(b), err, 512)
    if rc != 0:
        raise BwaGpuError(f"bwagpu_index_build failed: {L.bwagpu_strerror(rc).decode()} {err.value.decode()}")
    return b, L


def write_pac_ann_amb(prefix: str, codes_or_pac: np.ndarray, l_pac: int, contigs, packed: bool = False, holes=(), annos=None):
    """annos: per-contig comments as bns_dump writes them (bntseq.c:72-75: none -> "(null)"); names and annos may be str or bytes."""
    pac = codes_or_pac if packed else pack_pac(codes_or_pac)
    with open(prefix + ".pac", "wb") as f:          # file length is l_pac/4 + 1 (+1 when l_pac % 4 == 0) + the count byte (bntseq.c:314-323)
        f.write(pac[: (l_pac + 3) // 4].tobytes())
        if l_pac % 4 == 0:
            f.write(b"\0")
        f.write(bytes([l_pac % 4]))
    hole_offs = np.sort(np.array([int(h[0]) for h in holes], dtype=np.int64))
    enc = lambda x: x if isinstance(x, bytes) else str(x).encode()
    with open(prefix + ".ann", "wb") as f:
        f.write(f"{l_pac} {len(contigs)} 11\n".encode())
        off = 0
        for i, (name, ln) in enumerate(contigs):
            n_amb = int(np.searchsorted(hole_offs, off + int(ln)) - np.searchsorted(hole_offs, off))
            anno = b"(null)" if annos is None else enc(annos[i])
            f.write(b"0 " + enc(name) + (b" " + anno if anno else b"") + f"\n{off} {int(ln)} {n_amb}\n".encode())
            off += int(ln)
    with open(prefix + ".amb", "wb") as f:
        f.write(f"{l_pac} {len(contigs)} {len(holes)}\n".encode())
        for o, ln, ch in holes:
            f.write(f"{o} {ln} ".encode() + enc(ch) + b"\n")


def _write_bwt_sa(prefix: str, b: Built):
    hdr = np.array([b.primary, b.L2[1], b.L2[2], b.L2[3], b.L2[4]], dtype=np.uint64)
    with open(prefix + ".bwt", "wb") as f:
        f.write(hdr.tobytes())
        np.ctypeslib.as_array(b.bwt, shape=(int(b.bwt_size),)).tofile(f)
    with open(prefix + ".sa", "wb") as f:
        f.write(hdr.tobytes())
        f.write(np.array([b.sa_intv, b.seq_len], dtype=np.uint64).tobytes())
        np.ctypeslib.as_array(b.sa, shape=(int(b.n_sa),))[1:].tofile(f)       # sa[0] = -1 is not stored (bwt.c:404)


def build_index(prefix: str, codes: np.ndarray, contigs, device: int = 0, sa_intv: int = 32, lib_path: str | None = None) -> dict:
    """codes: uint8 array of the whole genome (values 0..3, contigs concatenated); contigs: [(name, length), ...]."""
    l_pac = int(codes.shape[0])
    assert sum(int(l) for _, l in contigs) == l_pac
    pac = pack_pac(codes)
    b, L = build_arrays(pac, l_pac, sa_intv, device, lib_path)
    try:
        _write_bwt_sa(prefix, b)
        info = {"l_pac": l_pac, "seq_len": int(b.seq_len), "primary": int(b.primary), "n_sa": int(b.n_sa), "build_ms": float(b.build_ms)}
    finally:
        L.bwagpu_built_free(C.byref(b))
    write_pac_ann_amb(prefix, pac, l_pac, contigs, packed=True)
    return info


class FastaResult(C.Structure):
    """bwagpu_fasta_t"""
    _fields_ = [("pac", C.POINTER(C.c_uint8)), ("l_pac", C.c_int64), ("n_seqs", C.c_int32), ("seq_offset", C.POINTER(C.c_int64)),
                ("seq_len", C.POINTER(C.c_int32)), ("seq_n_ambs", C.POINTER(C.c_int32)), ("names", C.POINTER(C.c_char)), ("names_bytes", C.c_int64),
                ("n_holes", C.c_int64), ("hole_offset", C.POINTER(C.c_int64)), ("hole_len", C.POINTER(C.c_int32)), ("hole_amb", C.POINTER(C.c_char)),
                ("parse_ms", C.c_float)]


def _open_fasta(fasta):
    """plain or gzip (by its magic bytes, as gzopen decides; BGZF is gzip), or an open binary file object"""
    if hasattr(fasta, "read"):
        return fasta, False
    with open(fasta, "rb") as f:
        magic = f.read(2)
    return (gzip.open(fasta, "rb") if magic == b"\x1f\x8b" else open(fasta, "rb")), True


def parse_fasta(fasta, device: int = 0, lib_path: str | None = None, chunk_bytes: int | None = None, piece_bytes: int = 64 << 20):
    """Run the device FASTA parser (bwagpu_fasta_*) over a file; returns (pac, l_pac, contigs [(name, len)], annos, holes
    [(offset, len, char)], parse_ms) with names, annos and hole characters as bytes.  piece_bytes: size of each feed call."""
    L = load_library(lib_path)
    P = C.c_void_p
    L.bwagpu_fasta_begin.argtypes = [C.POINTER(P), C.c_int, C.c_int64, C.c_char_p, C.c_size_t]
    L.bwagpu_fasta_feed.argtypes = [P, C.c_void_p, C.c_int64, C.c_char_p, C.c_size_t]
    L.bwagpu_fasta_end.argtypes = [P, C.c_void_p, C.c_char_p, C.c_size_t]
    L.bwagpu_fasta_free.argtypes = [C.c_void_p]
    err = C.create_string_buffer(512)
    h = P()

    def check(rc, what):
        if rc != 0:
            raise BwaGpuError(f"{what} failed: {L.bwagpu_strerror(rc).decode()} {err.value.decode(errors='replace')}")

    check(L.bwagpu_fasta_begin(C.byref(h), device, int(chunk_bytes or 0), err, 512), "bwagpu_fasta_begin")
    f, own = _open_fasta(fasta)
    res = FastaResult()
    try:
        try:
            while True:
                piece = f.read(piece_bytes)
                if not piece:
                    break
                rc = L.bwagpu_fasta_feed(h, piece, len(piece), err, 512)
                if rc != 0:
                    break
        finally:
            if own:
                f.close()
            rc = L.bwagpu_fasta_end(h, C.byref(res), err, 512)      # (always releases the parser; reports a feed error again)
        check(rc, "FASTA parse")
        l_pac = int(res.l_pac)
        pac = np.ctypeslib.as_array(res.pac, shape=(l_pac // 4 + 1,)).copy()
        lens = np.ctypeslib.as_array(res.seq_len, shape=(res.n_seqs,)).tolist()
        blob = C.string_at(res.names, res.names_bytes).split(b"\0")
        names, annos = blob[0:2 * res.n_seqs:2], blob[1:2 * res.n_seqs:2]
        nh = int(res.n_holes)
        if nh:
            ho = np.ctypeslib.as_array(res.hole_offset, shape=(nh,)).tolist()
            hl = np.ctypeslib.as_array(res.hole_len, shape=(nh,)).tolist()
            ha = C.string_at(res.hole_amb, nh)
            holes = [(o, ln, ha[i:i + 1]) for i, (o, ln) in enumerate(zip(ho, hl))]
        else:
            holes = []
        return pac, l_pac, list(zip(names, lens)), annos, holes, float(res.parse_ms)
    finally:
        L.bwagpu_fasta_free(C.byref(res))


def build_index_from_fasta(fasta, prefix: str, device: int = 0, lib_path: str | None = None, chunk_bytes: int | None = None) -> dict:
    """`bwa index` on the device: <prefix>.{pac,ann,amb,bwt,sa} from a FASTA file (plain or gzip), byte-identical to the reference's
    (ambiguity codes replaced and listed as holes as bns_fasta2bntseq does).  No file is written when the input is rejected."""
    pac, l_pac, contigs, annos, holes, parse_ms = parse_fasta(fasta, device, lib_path, chunk_bytes)
    b, L = build_arrays(pac, l_pac, 32, device, lib_path)
    try:
        _write_bwt_sa(prefix, b)
        build_ms = float(b.build_ms)
    finally:
        L.bwagpu_built_free(C.byref(b))
    write_pac_ann_amb(prefix, pac, l_pac, contigs, packed=True, holes=holes, annos=annos)
    return {"l_pac": l_pac, "n_seqs": len(contigs), "n_holes": len(holes), "parse_ms": parse_ms, "build_ms": build_ms}
