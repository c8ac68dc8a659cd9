"""The alignment list of a read on the device (bwagpu_batch_alns, bwagpu_alns_flat; bwa_amd/csrc/dev_alns.h) against the compiled reference: per region
mem_reg2aln (bwamem.c:1119-1189) of the list mem_mark_primary_se leaves, called through ctypes on oracle/_ref/libbwaref.so (it returns mem_aln_t by value),
and per read the SAM text of mem_reg2sam (refapi.RefIndex.regs2sam) -- line j of a read is the record with sel == j.  Every field must be equal, exactly.

1. a fuzz of bwagpu_alns_flat over region counts around the switch point of the kernels and more than one step of the wavefront form, with lists crafted from
   the genome (CIGAR records from hostapi.region_cigars, which other tests pin to the device and to the reference);
2. real batches with chimeric reads: run -> download -> cigars -> alns(opt, id0);
3. `bwa-amd mem` with BWAGPU_CLI_ALNS=1 against `bwa mem`;
4. error paths.
CPU: on the mock runtime (tests/hostsim), thinned.  -m gpu: everything, several seeds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hostapi
import refapi
import testdata
from bwa_amd import simdata
from bwa_amd.api import CIGAR_DTYPE, BwaGpu
from bwa_amd.structs import ALN_DEL3, ALN_DEL5, ALN_DTYPE, ALN_NOCIGAR, ALN_REV, ALN_ALT, ALNREG_DTYPE
from test_primary import alt_prefix, batch_reads, ref_opt

pytestmark = pytest.mark.skipif(not refapi.have_ref(), reason="oracle/_ref not built")

LANE_MAX, STEP = 4, 64      # where the kernels change their form (dev_alns.h); checked against the library under test
SIZES = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 2500)
FAMILIES = ("same", "disjoint", "del", "edge", "low", "none")
ALT_MODES = ("none", "all", "mixed")
F_ALL, F_NO_MULTI, F_SOFTCLIP, F_PRIMARY5, F_KEEP_SUPP_MAPQ = 0x8, 0x10, 0x200, 0x800, 0x1000
REGION_FIELDS = ("pos", "rid", "mapq", "nm", "n_cigar", "score", "alt_sc")
NAMES = ("chr1", "chr2", "chr3")


def check_limits(dev):
    assert dev.alns_limits() == dict(lane_max=LANE_MAX, step=STEP), "a switch point of the library moved: aim the cases at it"
    for n in (LANE_MAX, STEP, 2 * STEP):
        assert {n - 1, n, n + 1} <= set(SIZES), n
    assert max(SIZES) > 2 * STEP


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------------------
class RefAln(C.Structure):      # mem_aln_t (bwamem.h:114-127)
    _fields_ = [("pos", C.c_int64), ("rid", C.c_int), ("flag", C.c_int), ("is_rev", C.c_uint32, 1), ("is_alt", C.c_uint32, 1), ("mapq", C.c_uint32, 8), ("NM", C.c_uint32, 22),
                ("n_cigar", C.c_int), ("cigar", C.c_void_p), ("XA", C.c_void_p), ("score", C.c_int), ("sub", C.c_int), ("alt_sc", C.c_int)]


assert C.sizeof(RefAln) == 56


def ref_alns(idx, opt, counts, regs, ids, seqs, off):
    """mem_mark_primary_se on every list, then mem_reg2aln of every marked region -> (ALN_DTYPE records without the fields of mem_reg2sam's loop: sel -1,
    mapq_out = mapq, sub as mem_reg2aln leaves it; the final CIGAR of every region as a tuple; src: the region's index in the list as given)."""
    L = refapi.lib()
    L.mem_mark_primary_se.restype = C.c_int
    L.mem_mark_primary_se.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    L.mem_reg2aln.restype = RefAln
    L.mem_reg2aln.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    bns, pac = L.refshim_idx_bns(idx.h), L.refshim_idx_pac(idx.h)
    a = np.ascontiguousarray(regs, dtype=ALNREG_DTYPE).copy()
    seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
    out = np.zeros(a.shape[0], dtype=ALN_DTYPE)
    src = np.zeros(a.shape[0], dtype=np.int32)
    cigars = []
    lo = 0
    for i, c in enumerate(counts):
        c = int(c)
        a["seedlen0"][lo:lo + c] = np.arange(c)      # (read by neither function)
        L.mem_mark_primary_se(C.byref(opt), c, a.ctypes.data + lo * ALNREG_DTYPE.itemsize, int(ids[i]))
        lq, q = int(off[i + 1] - off[i]), seqs.ctypes.data + int(off[i])
        for k in range(lo, lo + c):
            r = L.mem_reg2aln(C.byref(opt), bns, pac, lq, q, a.ctypes.data + k * ALNREG_DTYPE.itemsize)
            o = out[k]
            o["pos"], o["rid"], o["flag"], o["mapq"], o["mapq_out"], o["n_cigar"], o["score"], o["sub"], o["alt_sc"], o["sel"] = \
                r.pos, r.rid, r.flag, r.mapq, r.mapq, r.n_cigar, r.score, r.sub, r.alt_sc, -1
            o["nm"] = r.NM if r.NM != 0x3fffff else -1
            o["flags"] = (ALN_REV if r.is_rev else 0) | (ALN_ALT if r.is_alt else 0)
            cigars.append(tuple((C.c_uint32 * r.n_cigar).from_address(r.cigar)) if r.n_cigar > 0 and r.cigar else ())
            if r.cigar:
                L.refshim_free(r.cigar)
        src[lo:lo + c] = a["seedlen0"][lo:lo + c]
        lo += c
    return out, cigars, src


def final_cigar(rec, cig, ops):
    """the CIGAR a caller writes from a record and the region's CIGAR record: clip5, the record's operations without the dropped deletion, clip3"""
    n = int(cig["n_cigar"])
    if n > 6:
        at = int(cig["cigar"][1]) << 32 | int(cig["cigar"][0])
        body = [int(x) for x in ops[at:at + n]]
    else:
        body = [int(x) for x in cig["cigar"][:max(n, 0)]]
    fl = int(rec["flags"])
    if fl & ALN_DEL5:
        assert body[0] & 0xf == 2
        body = body[1:]
    if fl & ALN_DEL3:
        assert body[-1] & 0xf == 2
        body = body[:-1]
    assert not (fl & ALN_DEL5 and fl & ALN_DEL3)
    c5, c3 = int(rec["clip5"]), int(rec["clip3"])
    return tuple(([c5 << 4 | 3] if c5 else []) + body + ([c3 << 4 | 3] if c3 else []))


def sam_by_read(sam, n):
    """[[fields of line 0, ...] per read] of single-end SAM text whose reads are named r0, r1, ..."""
    out = [[] for _ in range(n)]
    for ln in sam.decode().split("\n"):
        if ln and not ln.startswith("@"):
            f = ln.split("\t")
            out[int(f[0][1:])].append(f)
    return out


def check_against_reference(dev_out, idx, opt, counts, regs, ids, seqs, off, cigs, ops, what, region_ref=None):
    """every record of one call against mem_reg2aln, every read against its SAM lines.  -> (records, cover: what the call exercised)"""
    got, n_aln, pri, n_pri, ms = dev_out
    assert ms >= 0 and got.shape[0] == int(counts.sum()) == pri.shape[0]
    want, want_cig, src = region_ref if region_ref is not None else ref_alns(idx, opt, counts, regs, ids, seqs, off)
    assert np.array_equal(pri["src"], src), f"{what}: the marking records differ from mem_mark_primary_se's order"
    base = np.repeat(np.cumsum(counts) - counts, counts)
    cig_of = cigs[base + src] if got.shape[0] else cigs[:0]      # the CIGAR record of every place of the marked lists
    nocig = (got["flags"] & ALN_NOCIGAR) != 0
    assert np.array_equal(nocig, cig_of["n_cigar"] == -1), f"{what}: bit 0 of flags does not follow the CIGAR records' n_cigar == -1"
    computed = ~nocig
    assert not (nocig & (got["score"] >= opt.T)).any(), f"{what}: a region that reaches T has no CIGAR record: the comparison would leave it out"
    assert not got["pad_"].any()
    for f in ("rid", "mapq", "score", "alt_sc"):      # (final whether or not the CIGAR record was computed)
        bad = got[f] != want[f]
        assert not bad.any(), f"{what}: {f} differs at records {np.nonzero(bad)[0][:8].tolist()}: device {got[f][bad][:8]}, reference {want[f][bad][:8]}"
    for f in REGION_FIELDS:
        bad = (got[f] != want[f]) & computed
        assert not bad.any(), f"{what}: {f} differs at records {np.nonzero(bad)[0][:8].tolist()}: device {got[f][bad][:8]}, reference {want[f][bad][:8]}"
    for bit in (ALN_REV, ALN_ALT):
        assert np.array_equal(got["flags"] & bit, want["flags"] & bit), f"{what}: flags bit {bit:#x}"
    assert np.array_equal(got["flag"] & 0x104, want["flag"]), f"{what}: mem_reg2aln's flag"
    printed = got["sel"] >= 0
    unsel = ~printed
    assert np.array_equal(got["sub"][unsel], want["sub"][unsel]) and np.array_equal(got["mapq_out"][unsel], got["mapq"][unsel]) and not (got["flag"][unsel] & ~0x104).any(), what
    for k in np.nonzero(computed)[0]:
        assert final_cigar(got[k], cig_of[k], ops) == want_cig[k], f"{what}: record {k}: the CIGAR from the record differs from mem_reg2aln's"
        assert int(got["n_cigar"][k]) == len(want_cig[k])
    # mem_reg2sam: the lines of every read
    n = counts.shape[0]
    names = [f"r{i}" for i in range(n)]
    assert len(set(int(x) for x in np.diff(ids))) <= 1 and (n < 2 or int(ids[1] - ids[0]) == 1)
    sam = idx.regs2sam(opt, names, np.ascontiguousarray(seqs).tobytes(), None, off, counts, regs, n_processed=int(ids[0]) if n else 0)
    lines = sam_by_read(sam, n)
    cover = dict(sel_max=int(got["sel"].max()) if got.shape[0] else -1, supp=0, capped=0, sec_printed=0, hard=0, unmapped=0)
    lo = 0
    for i in range(n):
        c = int(counts[i])
        recs, cg = got[lo:lo + c], cig_of[lo:lo + c]
        sel = recs["sel"]
        kept = np.nonzero(sel >= 0)[0]
        assert int(n_aln[i]) == kept.shape[0] and sorted(sel[kept].tolist()) == list(range(kept.shape[0])), f"{what}: read {i}: sel {sel.tolist()[:20]}, n_aln {int(n_aln[i])}"
        assert np.all(np.diff(sel[kept]) > 0), f"{what}: read {i}: sel is not in the list's order"
        if kept.shape[0] == 0:
            assert len(lines[i]) == 1 and int(lines[i][0][1]) & 0x4, f"{what}: read {i}: no record kept, but the reference prints {len(lines[i])} lines"
            cover["unmapped"] += 1
        else:
            assert len(lines[i]) == kept.shape[0], f"{what}: read {i}: {kept.shape[0]} records kept, the reference prints {len(lines[i])} lines"
        for j, k in enumerate(kept):
            r, f = recs[k], lines[i][j]
            assert not int(r["flags"]) & ALN_NOCIGAR
            fl = int(r["flag"])
            flag = (fl & 0xffff) | (0x100 if fl & 0x10000 else 0) | (0x10 if int(r["flags"]) & ALN_REV else 0)
            soft = bool(opt.flag & F_SOFTCLIP) or bool(int(r["flags"]) & ALN_ALT) or j == 0
            text = "".join(f"{x >> 4}{'MIDSH'[(x & 0xf) if soft or (x & 0xf) < 3 else 4]}" for x in final_cigar(r, cg[k], ops))
            tags = dict(t.split(":", 2)[::2] for t in f[11:])
            mine = (flag, NAMES[int(r["rid"])], int(r["pos"]) + 1, int(r["mapq_out"]), text, int(r["nm"]), int(r["score"]), int(r["sub"]) if int(r["sub"]) >= 0 else None)
            theirs = (int(f[1]), f[2], int(f[3]), int(f[4]), f[5], int(tags["NM"]), int(tags["AS"]), int(tags["XS"]) if "XS" in tags else None)
            assert mine == theirs, f"{what}: read {i}, line {j} (record {k}):\n device    {mine}\n reference {theirs}"
            cover["supp"] += bool(fl & 0x10800); cover["capped"] += int(r["mapq_out"]) != int(r["mapq"]); cover["sec_printed"] += bool(fl & 0x100); cover["hard"] += "H" in text
        lo += c
    cover.update(del5=int(((got["flags"] & ALN_DEL5) != 0).sum()), del3=int(((got["flags"] & ALN_DEL3) != 0).sum()),
                 del_ops=int((((got["flags"] & (ALN_DEL5 | ALN_DEL3)) != 0) & (cig_of["n_cigar"] > 6)).sum()), rev=int(((got["flags"] & ALN_REV) != 0).sum()),
                 clip_none=int(((got["clip5"] == 0) & (got["clip3"] == 0) & computed).sum()), clip_one=int((((got["clip5"] == 0) != (got["clip3"] == 0)) & computed).sum()),
                 clip_both=int(((got["clip5"] != 0) & (got["clip3"] != 0)).sum()))
    return got, cover


# ---- crafted region lists -----------------------------------------------------------------------------------------------------------------------------------
def mutate(rng, piece, want_len, n_indel):
    """a copy of `piece` with substitutions and n_indel insertions or deletions of one to three bases, want_len bases long (the piece is cut or padded to fit)"""
    s = piece.copy()
    m = rng.random(s.shape[0]) < 0.03
    s[m] = (s[m] + rng.integers(1, 4, int(m.sum()))) & 3
    s = s.tolist()
    for _ in range(n_indel):
        at, ln = int(rng.integers(12, max(13, len(s) - 12))), int(rng.integers(1, 4))
        if rng.random() < 0.5:
            del s[at:at + ln]
        else:
            s[at:at] = rng.integers(0, 4, ln).tolist()
    s = s[:want_len] + rng.integers(0, 4, max(0, want_len - len(s))).tolist()
    return np.array(s, dtype=np.uint8)


def make_read(rng, g, ctg, n, family, alt_mode, T):
    """(read, regions): n regions of one read of 100 .. 150 bases.  A region's query interval holds a mutated copy of its reference piece where no earlier
    region has written the interval; the others align whatever is there (any pair of sequences has a global alignment: the reference computes it too)."""
    l_pac = int(ctg[-1][0] + ctg[-1][1])
    lq = int(rng.integers(100, 151))
    read = rng.integers(0, 4, lq).astype(np.uint8)
    a = np.zeros(n, dtype=ALNREG_DTYPE)
    if n == 0:
        return read, a
    if family in ("disjoint", "del", "edge"):
        n_slot = min(n, int(rng.integers(2, 5)))
        cuts = [0] + sorted((rng.choice(np.arange(1, lq // 25), n_slot - 1, replace=False) * 25).tolist()) + [lq] if n_slot > 1 else [0, lq]
        slots = [(cuts[k], cuts[k + 1]) for k in range(n_slot)]
        if family == "del" and n_slot > 1 and rng.random() < 0.5:
            slots[0] = (int(rng.integers(1, 9)), slots[0][1])      # (a clip in front of a region with a deletion rule)
    else:
        qb = int(rng.choice([0, 0, rng.integers(1, 30)])); qe = int(rng.choice([lq, lq, lq - rng.integers(1, 30)]))
        slots = [(qb, qe)]
    written = set()
    for k in range(n):
        qb, qe = slots[k % len(slots)]
        ql = qe - qb
        c = {"none": int(rng.integers(0, 2)), "all": 2, "mixed": int(rng.integers(0, 3))}[alt_mode]
        if family == "edge":
            c = k % 3
        c_off, c_len = ctg[c]
        rev = bool(rng.integers(0, 2))
        n_indel = int(rng.integers(0, 4))
        e5 = e3 = 0
        if family == "del":      # the reference span longer than the query at the lower or the upper end (or both: the leading rule wins)
            e5, e3 = [(5, 0), (0, 5), (7, 3), (0, 0)][int(rng.integers(0, 4))]
            n_indel = [0, 3, 3, 2][k % 4]
        span = ql + int(rng.integers(-2, 3)) if n_indel else ql
        if family == "edge" and k % 2 == 0:
            tb = c_off + e5
        elif family == "edge":
            tb = c_off + c_len - span - e3
        else:
            tb = int(rng.integers(c_off + 10, c_off + c_len - span - 10))
        te = tb + span
        fb, fe = tb - e5, te + e3
        assert c_off <= fb and fe <= c_off + c_len
        if (qb, qe) not in written:
            seg = mutate(rng, g[tb:te], ql, n_indel)
            read[qb:qe] = (3 - seg)[::-1] if rev else seg
            written.add((qb, qe))
        r = a[k]
        r["rb"], r["re"] = (2 * l_pac - fe, 2 * l_pac - fb) if rev else (fb, fe)
        r["qb"], r["qe"], r["rid"] = qb, qe, c
        if family == "none" or (family == "low" and rng.random() < 0.5):
            r["score"] = int(rng.integers(0, T))
        elif family == "same":
            r["score"] = int(rng.integers(T, T + 40)) if rng.random() < 0.5 else int(rng.integers(T, max(T, ql) + 1))      # (close scores: both sides of the drop_ratio test)
        else:
            r["score"] = int(rng.integers(T, max(T, ql) + 1))
        r["truesc"] = r["score"]
        r["csub"] = 0 if rng.random() < 0.6 else int(rng.integers(0, max(1, int(r["score"]))))
        r["w"], r["seedcov"], r["secondary"], r["secondary_all"] = 100, ql // 2 + 1, -1, -1
        r["frac_rep"] = np.float32(0.0 if rng.random() < 0.7 else rng.random() * 0.6)
        r["ncomp_isalt"] = (np.uint32(c == 2) << np.uint32(30)) | np.uint32(1)
    return read, a


def fuzz_cells(thin, rot):
    """(size, family, ALT mode): every family at every size with the ALT modes rotating, or (thin) every family for the sizes one lane handles and a rotating
    two for the others"""
    cells = []
    for si, n in enumerate(SIZES):
        fams = list(FAMILIES)
        if n == max(SIZES):
            fams = [FAMILIES[(rot + si) % 3]]      # (one read: the issue's budget; "same", "disjoint" or "del")
        elif thin and n > LANE_MAX + 1:
            fams = [FAMILIES[(rot + si * 5 + j * 3) % len(FAMILIES)] for j in range(2)]
        for j, f in enumerate(fams):
            cells.append((n, f, ALT_MODES[(si + j + rot) % 3]))
    return cells


def opt_variants():
    out = []
    for name, kw in (("default", {}), ("-a", dict(flag=F_ALL)), ("-M", dict(flag=F_NO_MULTI)), ("-q", dict(flag=F_KEEP_SUPP_MAPQ)), ("-Y", dict(flag=F_SOFTCLIP)),
                     ("drop0.9", dict(drop_ratio=0.9, flag=F_ALL))):
        o = ref_opt()
        for k, v in kw.items():
            setattr(o, k, v)
        out.append((name, o))
    return out


class World:
    """the index with chr3 flagged ALT, as the device, the reference and the host code see it"""
    def __init__(self, tmp, lib_path=None, options=None):
        prefix, self.g = testdata.small_index()
        lens = testdata.small_genome()[1]
        self.ctg = [(sum(lens[:i]), lens[i]) for i in range(len(lens))]
        self.prefix = alt_prefix(tmp, prefix, ["chr3"])
        self.dev = BwaGpu(self.prefix, lib_path=lib_path, options=options)
        self.idx = refapi.RefIndex(self.prefix)
        self.host = hostapi.HostFinalize(self.prefix)
        self.host.set_alt(2)

    def close(self):
        self.dev.close(); self.idx.close(); self.host.close()


def run_fuzz(W, seed, thin):
    dev = W.dev
    check_limits(dev)
    rng = np.random.default_rng(seed)
    base = ref_opt()
    cells = fuzz_cells(thin, seed)
    made = [make_read(rng, W.g, W.ctg, n, f, m, base.T) for n, f, m in cells]
    counts = np.array([c[0] for c in cells], dtype=np.int32)
    assert set(counts.tolist()) == set(SIZES)
    regs = np.concatenate([m[1] for m in made])
    seqs, off = testdata.ragged([m[0] for m in made])
    read_len = np.diff(off).astype(np.int32)
    ids = (1 << 33) + 7 * seed + np.arange(len(cells), dtype=np.int64)
    cigs, ops = W.host.region_cigars(base, seqs, off, counts, regs, with_ops=True)
    region_ref = ref_alns(W.idx, base, counts, regs, ids, seqs, off)      # (mem_reg2aln reads no flag and no drop_ratio: one reference for every option set)
    total = {}
    for name, opt in opt_variants():
        out = dev.alns_flat(opt, counts, regs, ids, read_len, cigs, ops)
        got, cover = check_against_reference(out, W.idx, opt, counts, regs, ids, seqs, off, cigs, ops, f"fuzz seed {seed}, options {name}", region_ref)
        total[name] = cover
    d = total["default"]
    assert d["sel_max"] >= 2 and d["supp"] > 0 and d["capped"] > 0 and d["unmapped"] > 0 and d["hard"] > 0, d
    assert d["del5"] > 0 and d["del3"] > 0 and d["del_ops"] > 0 and d["rev"] > 0 and d["clip_none"] > 0 and d["clip_one"] > 0 and d["clip_both"] > 0, d
    assert total["-a"]["sec_printed"] > total["drop0.9"]["sec_printed"] > 0, (total["-a"], total["drop0.9"])      # (the drop_ratio test decides both ways)
    assert total["-q"]["capped"] == 0 and total["-Y"]["hard"] == 0 and total["-M"]["supp"] == d["supp"]
    # a printed region whose CIGAR record is withheld: flagged, and the read's list is the same
    got = dev.alns_flat(base, counts, regs, ids, read_len, cigs, ops)[0]
    k = int(np.nonzero((got["sel"] == 0) & (np.repeat(counts, counts) > LANE_MAX))[0][0])
    lo = np.repeat(np.cumsum(counts) - counts, counts)
    pri = dev.alns_flat(base, counts, regs, ids, read_len, cigs, ops)[2]
    cigs2 = cigs.copy()
    cigs2["n_cigar"][lo[k] + pri["src"][k]] = -1
    got2, n_aln2, _, _, _ = dev.alns_flat(base, counts, regs, ids, read_len, cigs2, ops)
    assert int(got2["flags"][k]) & ALN_NOCIGAR and int(((got2["flags"] & ALN_NOCIGAR) != 0).sum()) == int(((got["flags"] & ALN_NOCIGAR) != 0).sum()) + 1
    for f in ("sel", "rid", "mapq", "mapq_out", "flag", "score", "sub", "clip5", "clip3"):
        assert np.array_equal(got2[f], got[f]), f
    return total


# ---- real batches ---------------------------------------------------------------------------------------------------------------------------------------
def run_batches(W, reads, id0s):
    opt = ref_opt()
    dev = W.dev
    seqs, off = testdata.flat(reads)
    dev.upload(seqs, off); dev.run(opt)
    counts, regs = dev.download()
    cigs = dev.cigars(opt); ops = dev.cigar_ops()
    assert int(counts.max()) > LANE_MAX, "no read for the wavefront form"
    sel_max = 0
    for id0 in id0s:
        ids = id0 + np.arange(counts.shape[0], dtype=np.int64)
        out = dev.alns(opt, id0)
        got, cover = check_against_reference(out, W.idx, opt, counts, regs, ids, seqs, off, cigs, ops, f"batch of {counts.shape[0]} reads, id0 {id0}")
        sel_max = max(sel_max, cover["sel_max"])
        assert cover["supp"] > 0
    assert sel_max > 0, "no read with a second line: the chimeric reads did not split"


# ---- the command line -----------------------------------------------------------------------------------------------------------------------------------
TRACE = "reads finalized from device alignment records"


def run_cli(cli, prefix, fq, K, env):
    """single-end SAM of `cli` with BWAGPU_CLI_ALNS=1 against `bwa mem`, byte for byte, for four option sets; the trace line counts the reads finalized from
    the records: all of them, or (-5: the host path) none"""
    body = lambda t: b"\n".join(l for l in t.split(b"\n") if not l.startswith(b"@PG"))
    n_reads = sum(1 for _ in open(fq)) // 4
    seen = b""
    for extra in ([], ["-a"], ["-M", "-Y"], ["-5"]):
        args = ["mem", "-K", str(K), "-t", "2"] + extra
        p = subprocess.run([refapi.REF_BWA] + args + [prefix, fq], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()[-1000:]
        want = body(p.stdout)
        p = subprocess.run([cli] + args + [prefix, fq], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(env, BWAGPU_CLI_TRACE="1", BWAGPU_CLI_ALNS="1"))
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert body(p.stdout) == want, f"BWAGPU_CLI_ALNS=1 {extra}: SAM differs from bwa mem"
        line = [l for l in p.stderr.decode().split("\n") if TRACE in l]
        assert len(line) == 1 and int(line[0].split("]")[1].split()[0]) == (0 if extra == ["-5"] else n_reads), (extra, p.stderr.decode()[-1500:])
        seen += want
    assert b"SA:Z:" in seen      # (supplementary lines)
    p = subprocess.run([cli, "mem", "-K", str(K), "-t", "2", prefix, fq], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(env, BWAGPU_CLI_TRACE="1"))
    assert p.returncode == 0 and TRACE not in p.stderr.decode(), "the switch is off by default"
    return seen


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    import hostsim_build
    w = World(tmp_path_factory.mktemp("alns_sim"), lib_path=hostsim_build.build(), options={"ptab_m": 6})
    yield w
    w.close()


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    w = World(tmp_path_factory.mktemp("alns_gpu"))
    yield w
    w.close()


def test_struct_and_limits(sim):
    assert ALN_DTYPE.itemsize == sim.dev.L.bwagpu_aln_size() == 64
    check_limits(sim.dev)


def test_reference_entry(sim):
    """the symbol is exported, the by-value return works, and a region whose reference span is 5 bases longer than its query comes back squeezed"""
    opt = ref_opt()
    read = sim.g[1000:1100].copy()
    for rb, re in ((995, 1100), (1000, 1105)):
        a = np.zeros(1, dtype=ALNREG_DTYPE)
        a["rb"], a["re"], a["qb"], a["qe"], a["score"], a["truesc"], a["w"], a["seedcov"], a["secondary"] = rb, re, 0, 100, 100, 100, 100, 50, -1
        want, cig, _ = ref_alns(sim.idx, opt, np.array([1]), a, np.array([0]), read, np.array([0, 100]))
        assert (int(want["pos"][0]), int(want["rid"][0]), cig[0]) == (1000, 0, (100 << 4,)), (want, cig)


def test_sim_alns_flat_fuzz(sim):
    run_fuzz(sim, 31, thin=True)


def test_sim_alns_on_batches(sim):
    lens = testdata.small_genome()[1]
    run_batches(sim, batch_reads(sim.g, lens, 60, 521), (7, (1 << 33) + 12345))


def test_sim_cli_alns(sim, tmp_path):
    import test_cli
    lens = testdata.small_genome()[1]
    fq = str(tmp_path / "se.fq")
    simdata.write_fastq(fq, batch_reads(sim.g, lens, 20, 531))
    env = dict(os.environ, BWAGPU_CLI_STREAMS="2", BWAGPU_CLI_SERIALIZE="1", BWAGPU_PTAB_M="6")
    run_cli(test_cli._sim_cli(), sim.prefix, fq, 1500, env)      # (ten reads per batch: id0 > 0 from the second batch on)


def test_error_paths(sim):
    opt = ref_opt()
    dev = sim.dev
    L, h = dev.L, dev.h
    p, n, ms = C.c_void_p(), C.c_int64(), C.c_float()
    reads = simdata.make_reads_se(sim.g, 4, seed=3)
    seqs, off = testdata.flat(reads)
    dev.upload(seqs, off)
    call = lambda *a: L.bwagpu_batch_alns(*a)
    ok_args = (h, C.byref(opt), 0, C.byref(p), C.byref(n), None, None, None, None)
    assert call(*ok_args) == -2, "before a run"
    dev.run(opt)
    assert call(*ok_args) == -2, "before a download"
    counts, regs = dev.download()
    assert call(*ok_args) == -2, "without the CIGAR call"
    cigs = dev.cigars(opt); ops = dev.cigar_ops()
    for args in ((None,) + ok_args[1:], (h, None) + ok_args[2:], ok_args[:3] + (None,) + ok_args[4:], ok_args[:4] + (None,) + ok_args[5:]):
        assert call(*args) == -2
    o5 = ref_opt(); o5.flag |= F_PRIMARY5
    assert call(h, C.byref(o5), *ok_args[2:]) == -2, "MEM_F_PRIMARY5"
    assert call(*ok_args) == 0 and n.value == int(counts.sum())      # n_aln, pri, n_pri and kernel_ms may be NULL
    L.bwagpu_free(p)
    dev.download()
    assert call(*ok_args) == -2, "the CIGAR records of an earlier download"
    dev.cigars(opt)
    # bwagpu_alns_flat
    ids = np.arange(4, dtype=np.int64); rl = np.diff(off).astype(np.int32)
    assert int(counts.sum()) > 0
    def flat(counts=counts, regs=regs, ids=ids, rl=rl, cigs=cigs, ops=ops, n_ops=None, hh=h, oo=opt, out=C.byref(p), n_reads=4):
        ptr = lambda x: None if x is None else x.ctypes.data
        return L.bwagpu_alns_flat(hh, None if oo is None else C.byref(oo), n_reads, ptr(counts), ptr(regs), ptr(ids), ptr(rl), ptr(cigs), ptr(ops) if ops is not None and ops.shape[0] else None,
                                  (ops.shape[0] if ops is not None else 0) if n_ops is None else n_ops, out, None, None, None, None)
    assert flat() == 0
    L.bwagpu_free(p)
    for kw in (dict(hh=None), dict(oo=None), dict(out=None), dict(counts=None), dict(regs=None), dict(ids=None), dict(rl=None), dict(cigs=None), dict(n_reads=-1), dict(n_ops=-1), dict(oo=o5)):
        assert flat(**kw) == -2, kw
    bad = regs.copy(); bad["rid"][0] = 3
    assert flat(regs=bad) == -2, "a rid outside the index"
    bad = regs.copy(); bad["rid"][-1] = -1
    assert flat(regs=bad) == -2
    for v in (-2, 32769):
        bad = cigs.copy(); bad["n_cigar"][0] = v
        assert flat(cigs=bad) == -2, v
    bad = cigs.copy(); bad["n_cigar"][0] = 7; bad["cigar"][0][0] = max(0, ops.shape[0] - 6); bad["cigar"][0][1] = 0
    assert flat(cigs=bad) == -2, "operations past the end of the array"
    bad["cigar"][0][1] = 1
    assert flat(cigs=bad) == -2
    assert flat(rl=np.array([150, -1, 150, 150], dtype=np.int32)) == -2
    # no reads; reads without regions
    assert L.bwagpu_alns_flat(h, C.byref(opt), 0, None, None, None, None, None, None, 0, C.byref(p), None, None, None, None) == 0
    L.bwagpu_free(p)
    got, n_aln, pri, n_pri, _ = dev.alns_flat(opt, np.zeros(3, dtype=np.int32), np.zeros(0, dtype=ALNREG_DTYPE), np.arange(3), np.full(3, 100), np.zeros(0, dtype=CIGAR_DTYPE), np.zeros(0, dtype=np.uint32))
    assert got.shape[0] == 0 and n_aln.tolist() == [0, 0, 0] and n_pri.tolist() == [0, 0, 0]


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed", [31, 32, 33])
def test_gpu_alns_flat_fuzz(gpu, seed):
    run_fuzz(gpu, seed, thin=False)


@pytest.mark.gpu
def test_gpu_alns_on_batches(gpu):
    lens = testdata.small_genome()[1]
    run_batches(gpu, batch_reads(gpu.g, lens, 1500, 621), (7, (1 << 35) + 7771))


@pytest.mark.gpu
def test_gpu_cli_alns(gpu, tmp_path):
    from bwa_amd import build as b
    _, cli = b.build_host(verbose=False)
    lens = testdata.small_genome()[1]
    fq = str(tmp_path / "se.fq")
    simdata.write_fastq(fq, batch_reads(gpu.g, lens, 1200, 631))
    seen = run_cli(cli, gpu.prefix, fq, 150000, dict(os.environ))      # (1000 reads per batch)
    assert seen.count(b"\n") >= 4 * 3000 and b"XA:Z:" in seen and b"\tpa:f:" in seen      # (XA entries from the records, ALT hits)
