"""Paired-end SAM text written on the device (bwagpu_batch_sam_pe, bwagpu_sam_pe_flat; bwa_amd/csrc/dev_samtext_pe.h) against the compiled reference's own
mem_sam_pe (bwamem_pair.c:276-419), called as test_sampe.RefSampe.sam_pe calls it but with every read's name, qualities and comment: the two `sam` strings of a
pair are compared byte for byte with the device's slices.  -R's id is not a field of bseq1_t: RG:Z: is spliced into the reference's lines as
test_samtext.test_xr_and_comments does.

1. a fuzz of bwagpu_sam_pe_flat over test_sampe's pair kinds, option sets (and test_samtext's XA / XB settings) and SIZES, with and without qualities, with and
   without MEM_F_NO_RESCUE.  The set of declined pairs must EQUAL the rule of the header, computed here from the reference's lists and the returned CIGAR records:
   the pair record has flags & 1 or path < 0; an end prints a region, or lists one in a printed XA, without a CIGAR record; an end's mate place has none.  The kinds
   whose path-0 form prints a hit below T ("lowT", "which_npri": no CIGAR record is due for such a hit) are kept to one small call of crafted NOCIGAR pairs; in
   every other call the rule's set is at most a tenth of the pairs;
2. crafted mate cases, each with a coverage counter over the WRITTEN text: TLEN of either sign and with p0 == p1, a reverse mate with an insertion / a deletion /
   a dropped leading deletion, RNEXT as a name, one end unmapped beside a forward and beside a reverse mate, both unmapped, MC with H on a supplementary line and S
   on line 0 of the same read, MC staying S because the mate is ALT, MEM_F_SOFTCLIP, SA on both lines of a path-0 end, path 1 with which == n_pri.  The test index
   is 200 kb: a contig position above 2^31 is not reachable here, the int64 path of POS / PNEXT / TLEN is covered by test_cli's large index only;
3. the writer's boundaries: names and reads around 64 and 512 bytes, a line that MC + SA + XA together make longer than the staging area;
4. real batches: run -> download -> sam_pe(opt, pes, id0), with the records (they equal sampe()'s) and without (the same text); cigars() / alns() / sampe() /
   sam() give afterwards what they gave before;
5. error paths; 6. the command line with BWAGPU_CLI_SAMTEXT=1 on paired-end input.
CPU: on the mock runtime (tests/hostsim), thinned.  -m gpu: everything, several seeds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hostapi
import refapi
import testdata
import test_pair as tpair
import test_primary as tp
import test_rescue as tr
import test_sampe as ts
import test_samtext as tx
from bwa_amd import simdata
from bwa_amd.structs import ALN_ALT, ALN_NOCIGAR, ALN_REV, ALNREG_DTYPE, PeOut, SamIn, SamOut
from test_sampe import F_ALL, F_NO_RESCUE, F_PRIMARY5, F_SOFTCLIP, REG

pytestmark = pytest.mark.skipif(not refapi.have_ref(), reason="oracle/_ref not built")

STAGING, STEP = 512, 64      # bytes of a wavefront's staging area, places of a list per step (dev_samtext.h); checked against the library under test
ALN_DEL5 = 0x8


def check_limits(dev):
    assert dev.sam_pe_limits() == dict(staging=STAGING, step=STEP), "a switch point of the library moved: aim the cases at it"
    ts.check_limits(dev)


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------------------
class RefSamPe(ts.RefSampe):
    def sam_text(self, opt, pes, seqs, off, counts, regs, ids, names, quals=None, comments=None):
        """mem_sam_pe of every pair with the reads' own names, qualities (bytes at the reads' offsets, or None) and comments ('' is none, as bseq_read leaves it)
        -> (the text of every read, the list of every read as mem_sam_pe leaves it)"""
        regs = np.ascontiguousarray(regs, dtype=ALNREG_DTYPE)
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        ends = np.concatenate([[0], np.cumsum(counts)])
        text, lists = [], []
        for p in range(len(counts) // 2):
            v = (tpair.AlnV * 2)()
            s = (ts.BSeq * 2)()
            keep = []
            for i in range(2):
                r = 2 * p + i
                a = regs[ends[r]:ends[r + 1]]
                v[i].a = self.libc.malloc(max(1, a.shape[0]) * REG)
                v[i].n = v[i].m = a.shape[0]
                if a.shape[0]:
                    C.memmove(v[i].a, a.ctypes.data, a.shape[0] * REG)
                q = np.ascontiguousarray(seqs[int(off[r]):int(off[r + 1])]).copy()
                keep.append(q)
                s[i].l_seq = q.shape[0]; s[i].id = r; s[i].name = names[r].encode(); s[i].seq = q.ctypes.data
                if quals is not None:
                    s[i].qual = quals[int(off[r]):int(off[r + 1])]
                if comments is not None and comments[r]:
                    s[i].comment = comments[r].encode()
            assert names[2 * p] == names[2 * p + 1]      # (the reference exits on a pair of two names)
            self.L.mem_sam_pe(C.byref(opt), self.bns, self.pac, pes.ctypes.data, int(ids[2 * p]) >> 1, s, v)
            for i in range(2):
                lists.append(np.frombuffer(C.string_at(v[i].a, v[i].n * REG), dtype=ALNREG_DTYPE).copy())
                self.L.refshim_free(v[i].a)
                text.append(C.string_at(s[i].sam))
                self.L.refshim_free(s[i].sam)
        return text, lists


class World(ts.World):
    def __init__(self, tmp, lib_path=None, options=None):
        super().__init__(tmp, lib_path, options)
        self.ref.close()
        self.ref = RefSamPe(self.prefix)


def expect_declined(opt, pe, lists):
    """the header's rule per PAIR, from the lists as the reference left them (marked order: what mem_gen_alt reads) and the call's CIGAR records"""
    counts, alns, cigs, pri, s = pe["counts"], pe["alns"], pe["cigs"], pe["pri"], pe["sampe"]
    e = np.concatenate([[0], np.cumsum(counts)])
    n = counts.shape[0]
    bad = np.zeros(n, dtype=bool)
    for r in range(n):
        lo, hi = int(e[r]), int(e[r + 1])
        a = lists[r]
        assert a.shape[0] == hi - lo
        nocig = cigs["n_cigar"][lo + pri["src"][lo:hi]] == -1
        printed = np.nonzero(alns["sel"][lo:hi] >= 0)[0]
        bad[r] = bool(nocig[printed].any())
        if not opt.flag & F_ALL:
            for k in printed:
                listed, shown = tx.xa_of(opt, a, int(k))
                if shown:
                    bad[r] |= bool(nocig[listed].any())
        z = int(s["z"][r >> 1][r & 1])      # this read's place as its mate's mate
        if 0 <= z < hi - lo:
            bad[r] |= bool(nocig[z])
    return ((s["flags"] & 1) != 0) | (s["path"] < 0) | bad[0::2] | bad[1::2]


def splice(text, rg, extra_flag):
    """the reference's lines with -R's id behind AS / XS and extra_flag in the flag"""
    out = []
    for ln in text.split(b"\n")[:-1]:
        f = ln.split(b"\t")
        f[1] = str(int(f[1]) | extra_flag).encode()
        if rg:
            k = max(i for i, t in enumerate(f) if i >= 11 and t.startswith((b"AS:i:", b"XS:i:")))
            f.insert(k + 1, b"RG:Z:" + rg.encode())
        out.append(b"\t".join(f) + b"\n")
    return b"".join(out)


COUNTERS = ("tlen_pos", "tlen_neg", "tlen_same", "mate_rev_ins", "mate_rev_del", "rev_del5", "mate_rev_del5", "rnext_name", "unmapped_mate_fwd", "unmapped_mate_rev", "both_unmapped",
            "mate_unmapped", "mc_hard_supp", "mc_soft_alt_mate", "softclip_supp", "softclip_mc", "path0_alt_sa", "which_npri", "mq", "xa", "sa", "path0", "path1")


def tag_of(f, name):
    for t in f[11:]:
        if t.startswith(name):
            return t[len(name):]
    return None


def pe_cover(cover, opt, out, pe):
    """what the WRITTEN text of a call exercised; the columns every line owes its mate are checked on the way"""
    off, s, counts, alns = out["off"], pe["sampe"], pe["counts"], pe["alns"]
    e = np.concatenate([[0], np.cumsum(counts)])
    for r in range(counts.shape[0]):
        text = out["text"][int(off[r]):int(off[r + 1])]
        if not text:
            continue
        p, i = r >> 1, r & 1
        lines = [ln.split(b"\t") for ln in text.split(b"\n")[:-1]]
        mc = [tag_of(f, b"MC:Z:") for f in lines]
        zm = int(s["z"][p][1 - i])
        mate = alns[int(e[r ^ 1]) + zm] if zm >= 0 else None
        mine = alns[int(e[r]):int(e[r + 1])]
        printed = mine[mine["sel"] >= 0][np.argsort(mine["sel"][mine["sel"] >= 0], kind="stable")]
        cover["path0" if s["path"][p] == 0 else "path1"] += 1
        cover["which_npri"] += int(s["path"][p] == 1 and zm > 0 and zm == int(pe["n_pri"][r ^ 1]))
        cover["path0_alt_sa"] += int(s["path"][p] == 0 and len(lines) == 2 and all(tag_of(f, b"SA:Z:") for f in lines))
        for j, f in enumerate(lines):
            fl, tlen = int(f[1]), int(f[8])
            assert fl & 0x1 and fl & (0x40 << i) and tag_of(f, b"MQ:i:") == str(int(s["q_se"][p][1 - i])).encode(), (r, f)
            cover["mq"] += 1
            cover["xa"] += int(bool(tag_of(f, b"XA:Z:") or tag_of(f, b"XB:Z:"))); cover["sa"] += int(bool(tag_of(f, b"SA:Z:")))
            both = f[6] == b"=" and f[5] != b"*" and mc[j] is not None
            cover["tlen_pos"] += int(tlen > 0); cover["tlen_neg"] += int(tlen < 0); cover["tlen_same"] += int(both and tlen == 0)
            if both and fl & 0x20:
                cover["mate_rev_ins"] += int(b"I" in mc[j]); cover["mate_rev_del"] += int(b"D" in mc[j])
                cover["mate_rev_del5"] += int(bool(int(mate["flags"]) & ALN_DEL5))
            if both and fl & 0x10 and j < printed.shape[0]:
                cover["rev_del5"] += int(bool(int(printed[j]["flags"]) & ALN_DEL5))
            cover["rnext_name"] += int(f[6] not in (b"=", b"*"))
            if fl & 0x4 and not fl & 0x8:      # copy mate to alignment: the mate's coordinates, no CIGAR, no NM / MD, the mate's strand
                assert f[2] != b"*" and f[3] == f[7] and f[5] == b"*" and f[6] == b"=" and tlen == 0 and tag_of(f, b"NM:i:") is None and bool(fl & 0x10) == bool(fl & 0x20), f
                cover["unmapped_mate_rev" if fl & 0x10 else "unmapped_mate_fwd"] += 1
            if fl & 0x4 and fl & 0x8:
                assert f[2:9] == [b"*", b"0", b"0", b"*", b"*", b"0", b"0"] and mc[j] is None, f
                cover["both_unmapped"] += 1
            if not fl & 0x4 and fl & 0x8:      # copy alignment to mate
                assert f[6] == b"=" and f[7] == f[3] and tlen == 0 and mc[j] is None and bool(fl & 0x10) == bool(fl & 0x20), f
                cover["mate_unmapped"] += 1
            if j > 0 and mc[j] and mc[0]:
                cover["mc_hard_supp"] += int(b"H" in mc[j] and b"S" in mc[0] and b"H" not in mc[0])
                cover["mc_soft_alt_mate"] += int(b"S" in mc[j] and not opt.flag & F_SOFTCLIP and bool(int(mate["flags"]) & ALN_ALT))
                cover["softclip_mc"] += int(b"S" in mc[j] and bool(opt.flag & F_SOFTCLIP) and not int(mate["flags"]) & ALN_ALT)
            cover["softclip_supp"] += int(j > 0 and bool(fl & 0x800) and b"S" in f[5] and bool(opt.flag & F_SOFTCLIP))


def names_of(n_pairs, tag="q"):
    return [f"{tag}{r >> 1}" for r in range(2 * n_pairs)]


def check_call(W, opt, pes, seqs, off, counts, regs, ids, names, what, cover, quals=None, comments=None, rg=None, extra_flag=0, max_declined=None):
    """one bwagpu_sam_pe_flat call with the records wanted: the declined set against the rule, every byte of the rest against the reference -> (result, declined pairs)"""
    want, lists = W.ref.sam_text(opt, pes, seqs, off, counts, regs, ids, names, quals, comments)
    if rg or extra_flag:
        want = [splice(t, rg, extra_flag) for t in want]
    out = W.dev.sam_pe_flat(opt, pes, seqs, off, counts, regs, ids, names, quals=quals, comments=comments, rg_id=rg, extra_flag=extra_flag, want_records=True)
    pe = out["pe"]
    assert [a.shape[0] for a in lists] == pe["counts"].tolist(), f"{what}: the merged lists' lengths"
    dec = expect_declined(opt, pe, lists)
    if max_declined is not None:
        assert int(dec.sum()) <= max_declined, f"{what}: the rule declines {int(dec.sum())} of {dec.shape[0]} pairs: {np.nonzero(dec)[0].tolist()}"
    tx.check_text(out, want, np.repeat(dec, 2), what, dict.fromkeys(tx.COUNTERS, 0))
    pe_cover(cover, opt, out, pe)
    assert len(out["kernel_ms"]) == 3 and min(out["kernel_ms"]) >= 0 and abs(out["kernel_ms"][0] - sum(pe["kernel_ms"])) <= 1e-3 * (1 + sum(pe["kernel_ms"]))
    return out, dec


# ---- 1. the fuzz --------------------------------------------------------------------------------------------------------------------------------------------
def option_sets():
    """test_sampe's sets and the XA / XB settings of test_samtext.sam_variants()"""
    sets = ts.opt_sets()
    have = {name for name, _ in sets}
    for name, o in tx.sam_variants():
        if name in ("XB", "xa1/3") and name not in have:
            o.max_matesw = 3
            sets.append((name, o))
    assert {"XB", "xa1/3", "-a", "-Y", "-M"} <= {name for name, _ in sets}
    return sets


BELOW_T = ("lowT", "which_npri")      # kinds whose path-0 form prints a hit below T, for which no CIGAR record is due: the rule declines them (run_nocigar)


def fuzz_cells(thin, seed, nopairing):
    """test_sampe's cells without the kinds that print a hit below T; under MEM_F_NOPAIRING, where nothing below T is printed, "which_npri" stays: which == n_pri.
    Every size stays."""
    cells = [c for c in ts.fuzz_cells(thin, seed) if c[0] not in BELOW_T or (nopairing and c[0] == "which_npri")]
    seen = {(a, b) for _, a, b in cells}
    cells += [("proper", a, b) for a, b in ts.SIZES if (a, b) not in seen]
    return cells


def run_fuzz(W, seed, thin):
    dev = W.dev
    check_limits(dev)
    meta = dev.index_meta()
    rng = np.random.default_rng(seed)
    cover = dict.fromkeys(COUNTERS, 0)
    sets = option_sets()
    n_calls = 0
    for oi, (name, opt) in enumerate(sets):
        cells = fuzz_cells(thin, seed, bool(opt.flag & ts.F_NOPAIRING))
        assert {(a, b) for _, a, b in cells} == set(ts.SIZES)
        sub = cells if not thin or oi == 0 else cells[oi::len(sets)]
        for rescue in (False, True):
            o = tp.ref_opt()
            C.memmove(C.byref(o), C.byref(opt), C.sizeof(o))
            if not rescue:
                o.flag |= F_NO_RESCUE
            use = sub if not rescue or not thin else sub[::3]
            if rescue and not thin:
                use = sub[oi % 2::2]      # (the rescue's own kernels are test_rescue's: half the cells, alternating between the option sets)
            pes = tr.fuzz_pes("one")
            seqs, off, counts, regs, tags = ts.build_call(rng, W.g, meta, o, use)
            n_pairs = len(use)
            ids = int(rng.integers(0, 1 << 20)) * 2 + np.arange(2 * n_pairs, dtype=np.int64) + ((1 << 35) if oi == 2 else 0)
            names = names_of(n_pairs)
            quals = tx.quals_of(rng, int(off[-1]))
            for q in ((quals, None) if name in ("default", "XB") and not rescue else (quals,)):
                what = f"fuzz seed {seed}, options {name}, rescue {rescue}, {'with' if q else 'without'} qualities"
                check_call(W, o, pes, seqs, off, counts, regs, ids, names, what, cover, quals=q, max_declined=n_pairs // 10)
                n_calls += 1
    need = ("tlen_pos", "tlen_neg", "rnext_name", "unmapped_mate_fwd", "both_unmapped", "mate_unmapped", "mc_hard_supp", "softclip_supp", "path0_alt_sa", "which_npri", "mq", "xa", "sa", "path0", "path1")
    zero = [k for k in need if cover[k] == 0]
    assert not zero, f"the fuzz never wrote {zero}: {cover}"
    return cover, n_calls


def run_nocigar(W):
    """the one call of crafted NOCIGAR pairs: hits below T that path 0 prints (no CIGAR record is due for them), a region below T listed in a printed XA, and
    ordinary pairs beside them, which are written"""
    dev = W.dev
    meta = dev.index_meta()
    rng = np.random.default_rng(17)
    opt = tp.ref_opt(); opt.flag |= F_NO_RESCUE
    pes = tr.fuzz_pes("one")
    cells = [("lowT", 3, 3), ("proper", 3, 3), ("lowT", 5, 2), ("multi01", 4, 4), ("which_npri", 2, 70), ("empty1", 2, 0)]
    reads, lists = [], []
    for kind, n0, n1 in cells:
        r, l = ts.make_pair(rng, W.g, meta, opt, kind, n0, n1)
        reads += r; lists += l
    # a printed hit of score 34 whose XA lists a hit of score 28 < T on the same interval of the read
    E0, E1 = ts.End(W.g, meta, 0, 30000, 120, False), ts.End(W.g, meta, 0, 30000 + 401 - 130, 130, True)
    reads += [E0.read, E1.read]
    lists += [np.concatenate([E0.true(0, 120, 34), E0.foreign(meta, 1, 7000, 0, 33, 28)]), E1.true(0, 130, 130)]
    seqs, off = testdata.ragged(reads)
    counts = np.array([a.shape[0] for a in lists], dtype=np.int32)
    regs = np.concatenate(lists)
    n_pairs = counts.shape[0] // 2
    ids = 64 + np.arange(2 * n_pairs, dtype=np.int64)
    cover = dict.fromkeys(COUNTERS, 0)
    out, dec = check_call(W, opt, pes, seqs, off, counts, regs, ids, names_of(n_pairs), "crafted NOCIGAR pairs", cover, quals=tx.quals_of(rng, int(off[-1])))
    assert dec.tolist() == [True, False, True, False, True, False, True], dec.tolist()
    pe = out["pe"]
    e = np.concatenate([[0], np.cumsum(pe["counts"])])
    last = pe["alns"][int(e[-3]):int(e[-2])]      # end 0 of the XA pair: its printed place has a CIGAR record, the listed one has none
    assert not int(last["flags"][last["sel"] == 0][0]) & ALN_NOCIGAR and (last["flags"] & ALN_NOCIGAR).any()
    assert out["n_declined"] == 8 and cover["mq"] >= 6


# ---- 2. crafted mate cases ----------------------------------------------------------------------------------------------------------------------------------
def indel_end(g, meta, c, x, L, rev, kind):
    """a read cut from [x, x + L) of contig c and its one region: with two bases inserted in its middle ("ins"), three removed ("del"), or as it is under a
    region that begins five reference bases early ("lead": the CIGAR's leading deletion is dropped and the position moves) -> (read, region)"""
    l_pac = int(meta["l_pac"])
    b = int(meta["ctg_offset"][c]) + x
    fwd = g[b:b + L].copy()
    if kind == "ins":
        fwd = np.concatenate([fwd[:L // 2], (fwd[L // 2:L // 2 + 2] + 1) & 3, fwd[L // 2:]])
    elif kind == "del":
        fwd = np.concatenate([fwd[:L // 2], fwd[L // 2 + 3:]])
    fb, fe = (b - 5 if kind == "lead" else b), b + L
    a = ts.region(c, 2 * l_pac - fe if rev else fb, 1, fwd.shape[0] - 12, 0, int(meta["ctg_is_alt"][c]))
    a["re"] = a["rb"] + (fe - fb); a["qe"] = fwd.shape[0]; a["seedcov"] = fwd.shape[0] // 2
    return (tr.revcomp(fwd) if rev else fwd).astype(np.uint8), a


def crafted_pairs(W, opt, rng):
    g, meta = W.g, W.dev.index_meta()
    reads, lists, tags = [], [], []
    def add(tag, r, l):
        reads.extend(r); lists.extend(l); tags.append(tag)
    if opt.flag & ts.F_NOPAIRING:      # (path 1: place 0 is below T and is not printed, `which` is the ALT hit at place n_pri)
        for n0, n1 in ((2, 3), (5, 70)):
            add("which_npri", *ts.make_pair(rng, g, meta, opt, "which_npri", n0, n1))
    for kind, n0, n1 in (("proper", 2, 3), ("other_ctg", 1, 1), ("empty1", 2, 0), ("empty01", 0, 0), ("multi01", 3, 4), ("multi0", 5, 2), ("alt_print", 2, 3), ("zsec", 2, 4),
                         ("unpaired", 1, 2), ("far", 2, 2), ("alt_only", 2, 2)):
        r, l = ts.make_pair(rng, g, meta, opt, kind, n0, n1)
        add(kind, r, l)
    x = 52000
    # both ends forward at one position: p0 == p1, TLEN 0 between two aligned ends of one contig
    E = ts.End(g, meta, 0, x, 120, False)
    add("same_pos", [E.read, E.read.copy()], [E.true(0, 120, 120), E.true(0, 120, 120)])
    # a reverse mate whose CIGAR has an insertion / a deletion / a dropped leading deletion: its rlen is not its read length
    for k, kind in enumerate(("ins", "del", "lead")):
        E0 = ts.End(g, meta, 0, x + 3000 * (k + 1), 125, False)
        r1, a1 = indel_end(g, meta, 0, x + 3000 * (k + 1) + 400 - 130, 130, True, kind)
        add("rev_" + kind, [E0.read, r1], [E0.true(0, 125, 125), a1])
    # ... and the same three as the forward end beside a reverse mate (the line's own rlen does not enter: its strand is forward; the mate's does)
    r0, a0 = indel_end(g, meta, 0, x + 13000, 128, False, "lead")
    E1 = ts.End(g, meta, 0, x + 13000 + 380 - 120, 120, True)
    add("fwd_lead", [r0, E1.read], [a0, E1.true(0, 120, 120)])
    # end 0 unmapped beside a reverse mate
    E1 = ts.End(g, meta, 1, 20000, 140, True)
    add("unmapped_rev_mate", [rng.integers(0, 4, 101).astype(np.uint8), E1.read], [np.zeros(0, dtype=ALNREG_DTYPE), E1.true(0, 140, 140)])
    # a chimeric end 0 (two lines) beside a clipped mate on the ALT contig: MC keeps S on the supplementary line
    E0 = ts.End(g, meta, 0, x + 17000, 140, False)
    E1 = ts.End(g, meta, 2, 3000, 130, True)
    add("alt_mate", [E0.read, E1.read], [np.concatenate([E0.true(0, 100, 100), E0.foreign(meta, 1, 15000, 106, 140, 34)]), E1.true(0, 90, 90)])
    seqs, off = testdata.ragged(reads)
    counts = np.array([a.shape[0] for a in lists], dtype=np.int32)
    return seqs, off, counts, np.concatenate(lists), tags


def run_crafted(W):
    dev = W.dev
    check_limits(dev)
    cover = dict.fromkeys(COUNTERS, 0)
    pes = tr.fuzz_pes("one")
    for name, fl in (("default", 0), ("-Y", F_SOFTCLIP), ("nopairing", ts.F_NOPAIRING)):
        rng = np.random.default_rng(23)
        opt = tp.ref_opt(); opt.flag |= fl | F_NO_RESCUE
        seqs, off, counts, regs, tags = crafted_pairs(W, opt, rng)
        n_pairs = len(tags)
        ids = 1000 + np.arange(2 * n_pairs, dtype=np.int64)
        quals = tx.quals_of(rng, int(off[-1]))
        out, dec = check_call(W, opt, pes, seqs, off, counts, regs, ids, names_of(n_pairs), f"crafted mate cases, options {name}", cover, quals=quals)
        assert not dec.any(), [tags[p] for p in np.nonzero(dec)[0]]
    zero = [k for k in COUNTERS if cover[k] == 0]
    assert not zero, f"no written line covers {zero}: {cover}"
    # comments, -R's id and extra_flag
    rng = np.random.default_rng(29)
    opt = tp.ref_opt(); opt.flag |= F_NO_RESCUE
    seqs, off, counts, regs, tags = crafted_pairs(W, opt, rng)
    n_pairs = len(tags)
    comments = [("BC:Z:ACGT x%d" % r) if r % 3 else "" for r in range(2 * n_pairs)]
    check_call(W, opt, pes, seqs, off, counts, regs, 6 + np.arange(2 * n_pairs, dtype=np.int64), names_of(n_pairs), "comments, RG and extra_flag", dict.fromkeys(COUNTERS, 0),
               comments=comments, rg="grp1", extra_flag=0x200)


# ---- 3. the writer's boundaries -----------------------------------------------------------------------------------------------------------------------------
def run_boundaries(W):
    dev = W.dev
    check_limits(dev)
    g, meta = W.g, dev.index_meta()
    rng = np.random.default_rng(5)
    opt = tp.ref_opt(); opt.flag |= F_NO_RESCUE
    pes = tr.fuzz_pes("one")
    reads, lists, names = [], [], []
    lens = [63, 64, 65, STAGING - 1, STAGING, STAGING + 1]
    name_lens = [1, 63, 64, 65, STAGING - 1, STAGING, STAGING + 1, 255]
    for j, L in enumerate(lens + [100, 100]):      # exact matches, FR, 380 between the first bases; the names around the wavefront width and the staging area
        x = 2000 + 2500 * j
        E0, E1 = ts.End(g, meta, 0, x, L, False), ts.End(g, meta, 0, x + 380, L, True)
        reads += [E0.read, E1.read]; lists += [E0.true(0, L, L), E1.true(0, L, L)]
        nm = ("n%d_" % j).ljust(name_lens[j], "x")[:name_lens[j]]
        names += [nm, nm]
    # a line that MC, SA and XA together make longer than the staging area: a 150-base chimera with four more hits of nearly its score on its first part
    E0 = ts.End(g, meta, 0, 60000, 150, False)
    E1 = ts.End(g, meta, 0, 60000 + 420 - 140, 140, True)
    first = [E0.true(0, 100, 100)] + [E0.foreign(meta, 1, 3000 + 900 * k, 0, 100, 96 - k) for k in range(4)] + [E0.foreign(meta, 1, 30000, 104, 150, 40)]
    reads += [E0.read, E1.read]; lists += [np.concatenate(first), E1.true(0, 120, 120)]
    names += ["chimera", "chimera"]
    seqs, off = testdata.ragged(reads)
    counts = np.array([a.shape[0] for a in lists], dtype=np.int32)
    regs = np.concatenate(lists)
    n_pairs = len(names) // 2
    ids = 22 + np.arange(2 * n_pairs, dtype=np.int64)
    quals = tx.quals_of(rng, int(off[-1]))
    cover = dict.fromkeys(COUNTERS, 0)
    for q in (None, quals):
        out, dec = check_call(W, opt, pes, seqs, off, counts, regs, ids, names, f"boundaries, {'with' if q else 'without'} qualities", cover, quals=q)
        assert not dec.any()
    r = names.index("chimera")      # (of the call with qualities)
    line0 = out["text"][int(out["off"][r]):int(out["off"][r + 1])].split(b"\n")[0]
    f = line0.split(b"\t")
    extra = sum(len(t) + 1 for t in f[11:] if t.startswith((b"MC:Z:", b"SA:Z:", b"XA:Z:")))
    assert all(tag_of(f, t) for t in (b"MC:Z:", b"SA:Z:", b"XA:Z:")) and len(line0) + 1 > STAGING > len(line0) + 1 - extra, (len(line0), extra)


# ---- 4. real batches ----------------------------------------------------------------------------------------------------------------------------------------
def same_pe(a, b, what):
    for k in ("counts", "regs", "src", "rescue", "pri", "n_pri", "pairs", "sampe", "alns", "n_aln"):
        assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k}"
    assert hostapi.decode_cigars(a["cigs"], a["ops"]) == hostapi.decode_cigars(b["cigs"], b["ops"]), f"{what}: CIGAR records"      # (the operation array's order varies between calls)


def run_batches(W, n_pairs, n_foreign, seed, id0s):
    opt = tp.ref_opt()
    dev = W.dev
    rng = np.random.default_rng(9)
    reads, _, _ = tpair.pe_reads(W.g, n_pairs, n_foreign, seed)
    seqs, off = testdata.flat(reads)
    dev.upload(seqs, off); dev.run(opt)
    counts, regs = dev.download()
    pes = W.ref.pestat(opt, counts, regs)
    assert not pes["failed"].all(), "mem_pestat found no orientation: the batch is too small"
    n = counts.shape[0]
    names = [f"pair{r >> 1}/x" for r in range(n)]
    quals = tx.quals_of(rng, int(off[-1]))
    cover = dict.fromkeys(COUNTERS, 0)
    # what the other calls give before
    cig0 = hostapi.decode_cigars(dev.cigars(opt), dev.cigar_ops())
    aln0 = dev.alns(opt, id0s[0])
    se0 = dev.sam(opt, id0s[0], names, quals=quals)
    for id0 in id0s:
        ids = id0 + np.arange(n, dtype=np.int64)
        pe0 = dev.sampe(opt, pes, id0)
        want, lists = W.ref.sam_text(opt, pes, seqs, off, counts, regs, ids, names, quals)
        out = dev.sam_pe(opt, pes, id0, names, quals=quals, want_records=True)
        same_pe(out["pe"], pe0, f"id0 {id0}: the records of sam_pe() against sampe()'s")
        dec = expect_declined(opt, out["pe"], lists)
        assert int(dec.sum()) * 10 <= dec.shape[0]
        tx.check_text(out, want, np.repeat(dec, 2), f"batch of {n // 2} pairs, id0 {id0}", dict.fromkeys(tx.COUNTERS, 0))
        pe_cover(cover, opt, out, out["pe"])
        bare = dev.sam_pe(opt, pes, id0, names, quals=quals)
        assert "pe" not in bare and bare["text"] == out["text"] and np.array_equal(bare["off"], out["off"]) and np.array_equal(bare["flags"], out["flags"]) and np.array_equal(bare["n_lines"], out["n_lines"])
        same_pe(dev.sampe(opt, pes, id0), pe0, f"id0 {id0}: sampe() after sam_pe()")
    assert cover["tlen_pos"] > 0 and cover["tlen_neg"] > 0 and cover["path0"] > n // 4 and cover["sa"] > 0, cover
    # ... and after
    aln1 = dev.alns(opt, id0s[0])
    for x, y in zip(aln0[:4], aln1[:4]):
        assert np.array_equal(x, y), "bwagpu_batch_alns returns something else after bwagpu_batch_sam_pe"
    se1 = dev.sam(opt, id0s[0], names, quals=quals)
    assert se1["text"] == se0["text"] and np.array_equal(se1["flags"], se0["flags"]), "bwagpu_batch_sam returns something else after bwagpu_batch_sam_pe"
    assert hostapi.decode_cigars(dev.cigars(opt), dev.cigar_ops()) == cig0, "bwagpu_batch_cigars returns something else after bwagpu_batch_sam_pe"
    # a table of logarithms too small for any pair: records travel to the host and back -- the same text
    dev.set_option("pri_log_cap", 2)
    try:
        again = dev.sam_pe(opt, pes, id0s[-1], names, quals=quals)
    finally:
        dev.set_option("pri_log_cap", 0)
    assert again["text"] == out["text"] and np.array_equal(again["flags"], out["flags"])
    return cover, out


# ---- 5. error paths -----------------------------------------------------------------------------------------------------------------------------------------
def run_error_paths(W):
    opt = tp.ref_opt()
    dev = W.dev
    L, h = dev.L, dev.h
    pes = tpair.make_pes("one")
    P = pes.ctypes.data
    reads, _, _ = tpair.pe_reads(W.g, 3, 0, 5)
    cnt = np.zeros(6, dtype=np.int32)
    names = np.frombuffer(b"aabbcc", dtype=np.uint8).copy()
    name_off = np.arange(7, dtype=np.int64)
    sin = SamIn(names.ctypes.data, name_off.ctypes.data, None, None, None, None, 0)
    o, so = PeOut(), SamOut()

    def free(so, o=None):
        for p in (so.text, so.off, so.flags, so.n_lines):
            assert p
            L.bwagpu_free(p)
        if o is not None:
            for f in ("regs", "src", "rescue", "pri", "n_pri", "pairs", "sampe", "cigs", "ops", "alns", "n_aln"):
                assert getattr(o, f)
                L.bwagpu_free(C.c_void_p(getattr(o, f)))
    dev.upload(*testdata.flat(reads))
    call = lambda *a: L.bwagpu_batch_sam_pe(*a)
    ok = lambda: [h, C.byref(opt), P, 0, C.byref(sin), cnt.ctypes.data, C.byref(o), C.byref(so)]
    assert call(*ok()) == -2, "before a run"
    dev.run(opt)
    assert call(*ok()) == -2, "before a download"
    dev.download()
    for k in (0, 1, 2, 4, 5, 7):      # NULL h, opt, pes, in, counts, out
        a = ok(); a[k] = None
        assert call(*a) == -2, k
    a = ok(); a[3] = 7
    assert call(*a) == -2, "odd id0"
    o5 = tp.ref_opt(); o5.flag |= F_PRIMARY5
    a = ok(); a[1] = C.byref(o5)
    assert call(*a) == -2 and not o.regs and not so.text, "MEM_F_PRIMARY5"
    for bad_in in (SamIn(None, name_off.ctypes.data, None, None, None, None, 0), SamIn(names.ctypes.data, None, None, None, None, None, 0),
                   SamIn(names.ctypes.data, name_off.ctypes.data, None, names.ctypes.data, None, None, 0)):
        a = ok(); a[4] = C.byref(bad_in)
        assert call(*a) == -2
    bad = np.array([0, 1, 2, 4, 3, 5, 6], dtype=np.int64)
    a = ok(); a[4] = C.byref(SamIn(names.ctypes.data, bad.ctypes.data, None, None, None, None, 0))
    assert call(*a) == -2 and b"ascend" in L.bwagpu_last_error(h)
    other = np.frombuffer(b"aabxcc", dtype=np.uint8).copy()      # pair 1: "b" and "x"
    a = ok(); a[4] = C.byref(SamIn(other.ctypes.data, name_off.ctypes.data, None, None, None, None, 0))
    assert call(*a) == -2 and b"different names (pair 1)" in L.bwagpu_last_error(h), L.bwagpu_last_error(h)
    longer = np.array([0, 1, 2, 3, 5, 5, 6], dtype=np.int64)      # pair 1: "bb" and ""
    a = ok(); a[4] = C.byref(SamIn(names.ctypes.data, longer.ctypes.data, None, None, None, None, 0))
    assert call(*a) == -2 and b"different names (pair 1)" in L.bwagpu_last_error(h)
    assert call(*ok()) == 0 and so.n_text > 0 and o.sampe      # (no bwagpu_batch_cigars call before it)
    free(so, o)
    a = ok(); a[6] = None
    assert call(*a) == 0 and so.n_text > 0
    free(so)
    # a handle without contig names
    bare = type(dev).empty(dev.index_meta(), lib_path=L._name)
    try:
        bare.upload(*testdata.flat(reads[:2]))
        with pytest.raises(Exception, match="contig names"):
            bare.sam_pe_flat(opt, pes, np.zeros(200, dtype=np.uint8), np.array([0, 100, 200]), np.zeros(2, dtype=np.int32), np.zeros(0, dtype=ALNREG_DTYPE), np.arange(2), ["q", "q"])
    finally:
        bare.close()
    dev.upload(*testdata.flat(reads[:3])); dev.run(opt); dev.download()
    a = ok(); a[4] = C.byref(SamIn(names.ctypes.data, name_off.ctypes.data, None, None, None, None, 0))
    assert call(*a) == -2, "an odd number of reads"
    dev.upload(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64)); dev.run(opt); dev.download()
    got = dev.sam_pe(opt, pes, 0, [], want_records=True)
    assert got["text"] == b"" and got["off"].tolist() == [0] and got["pe"]["sampe"].shape[0] == 0
    # bwagpu_sam_pe_flat
    rng = np.random.default_rng(3)
    rd, ls = tr.make_case(rng, W.g, dev.index_meta(), opt, pes, "rescued", 2)
    seqs, off = testdata.ragged(rd)
    c2 = np.array([a.shape[0] for a in ls], dtype=np.int32); r2 = np.concatenate(ls); ids = np.array([4, 5], dtype=np.int64)
    n2 = np.frombuffer(b"zz", dtype=np.uint8).copy(); no2 = np.arange(3, dtype=np.int64)
    sin2 = SamIn(n2.ctypes.data, no2.ctypes.data, None, None, None, None, 0)
    flat = lambda *a: L.bwagpu_sam_pe_flat(*a)
    okf = lambda: [h, C.byref(opt), P, 1, seqs.ctypes.data, off.ctypes.data, c2.ctypes.data, r2.ctypes.data, ids.ctypes.data, C.byref(sin2), cnt.ctypes.data, C.byref(o), C.byref(so)]
    for k in (0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 12):
        a = okf(); a[k] = None
        assert flat(*a) == -2, k
    a = okf(); a[3] = -1
    assert flat(*a) == -2
    a = okf(); a[1] = C.byref(o5)
    assert flat(*a) == -2, "MEM_F_PRIMARY5"
    n3 = np.frombuffer(b"zy", dtype=np.uint8).copy()
    a = okf(); a[9] = C.byref(SamIn(n3.ctypes.data, no2.ctypes.data, None, None, None, None, 0))
    assert flat(*a) == -2 and b"different names (pair 0)" in L.bwagpu_last_error(h)
    a = okf(); a[9] = C.byref(SamIn(n2.ctypes.data, np.array([0, 2, 1], dtype=np.int64).ctypes.data, None, None, None, None, 0))
    assert flat(*a) == -2
    r3 = r2.copy(); r3["rid"][0] = int(dev.index_meta()["n_seqs"])
    a = okf(); a[7] = r3.ctypes.data
    assert flat(*a) == -2, "rid outside the index"
    assert flat(*okf()) == 0 and o.n_regs == int(cnt[:2].sum()) and so.n_text > 0
    free(so, o)
    got = dev.sam_pe_flat(opt, pes, np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=ALNREG_DTYPE), np.zeros(0, dtype=np.int64), [])
    assert got["text"] == b"" and got["n_declined"] == 0
    # two pairs without a single region: two unmapped records each, with the mate's bits
    got = dev.sam_pe_flat(opt, pes, np.zeros(400, dtype=np.uint8), np.arange(5, dtype=np.int64) * 100, np.zeros(4, dtype=np.int32), np.zeros(0, dtype=ALNREG_DTYPE), np.arange(4, dtype=np.int64),
                          ["u0", "u0", "u1", "u1"])
    assert got["n_lines"].tolist() == [1] * 4 and got["n_declined"] == 0
    assert [ln.split(b"\t")[1] for ln in got["text"].split(b"\n")[:-1]] == [b"77", b"141", b"77", b"141"] and got["text"].count(b"\t*\t0\t0\t*\t*\t0\t0\t") == 4 and got["text"].count(b"\tMQ:i:0\t") == 4


# ---- 6. the command line ------------------------------------------------------------------------------------------------------------------------------------
TRACE = "pairs written from device SAM text"


CLI_SETS = ([], ["-a"], ["-M", "-Y"], ["-C"], ["-R", "@RG\\tID:x"])
CLI_SETS_THIN = ([], ["-a", "-C"], ["-M", "-Y", "-R", "@RG\\tID:x"])      # (the mock runtime: every run is the whole hot path on the host)


def run_cli(cli, prefix, tmp_path, g, n_pairs, n_foreign, seed, K, env, sets=CLI_SETS):
    """paired-end SAM of `cli` with BWAGPU_CLI_SAMTEXT=1 against `bwa mem` and against the switch-off run, byte for byte apart from @PG; -v 4 prints the number of
    pairs written from the device's text"""
    _, a, b = tpair.pe_reads(g, n_pairs, n_foreign, seed)
    f = {}
    for tag, suffix in (("", ""), ("c", " BC:Z:ACGT")):
        f[tag] = (str(tmp_path / f"s{tag}_1.fq"), str(tmp_path / f"s{tag}_2.fq"))
        simdata.write_fastq(f[tag][0], a, suffix=suffix); simdata.write_fastq(f[tag][1], b, suffix=suffix)
    body = lambda t: b"\n".join(l for l in t.split(b"\n") if not l.startswith(b"@PG"))
    def run(exe, extra, files, e=None):
        p = subprocess.run([exe, "mem", "-K", str(K), "-t", "2"] + extra + [prefix, *files], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        return body(p.stdout), p.stderr.decode()
    e_off = dict(env); e_off.pop("BWAGPU_CLI_SAMTEXT", None); e_off.pop("BWAGPU_CLI_SAMPE", None)
    e_on = dict(e_off, BWAGPU_CLI_SAMTEXT="1")
    seen = b""
    for extra in sets:
        files = f["c"] if "-C" in extra else f[""]
        want, _ = run(refapi.REF_BWA, extra, files)
        assert want.count(b"\n") >= 2 * (n_pairs + n_foreign)
        on, err_on = run(cli, ["-v", "4"] + extra, files, e_on)
        assert on == want, f"BWAGPU_CLI_SAMTEXT=1 {extra}: SAM differs from bwa mem"
        off_, err_off = run(cli, ["-v", "4"] + extra, files, e_off)
        assert off_ == on and TRACE not in err_off, "the switch is off by default"
        line = [l for l in err_on.split("\n") if TRACE in l]
        assert len(line) == 1, err_on[-1500:]
        n = int(line[0].split("]")[1].split()[0])
        assert 0 < n <= n_pairs + n_foreign and n * 10 >= 9 * (n_pairs + n_foreign), (extra, n)
        seen += want
    assert b"\tBC:Z:ACGT" in seen and b"\tRG:Z:x" in seen and b"\tMC:Z:" in seen
    return seen


# ---- fixtures and tests -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    import hostsim_build
    w = World(tmp_path_factory.mktemp("sam_pe_sim"), lib_path=hostsim_build.build(), options={"ptab_m": 6})
    yield w
    w.close()


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    w = World(tmp_path_factory.mktemp("sam_pe_gpu"))
    yield w
    w.close()


def test_limits(sim):
    check_limits(sim.dev)


def test_sim_sam_pe_flat_fuzz(sim):
    run_fuzz(sim, 51, thin=True)


def test_sim_nocigar_pairs(sim):
    run_nocigar(sim)


def test_sim_crafted_mates(sim):
    run_crafted(sim)


def test_sim_boundaries(sim):
    run_boundaries(sim)


def test_sim_sam_pe_on_batches(sim):
    run_batches(sim, 16, 4, 701, (0, (1 << 35) + 7770))


def test_error_paths(sim):
    run_error_paths(sim)


def test_sim_cli_samtext_pe(sim, tmp_path):
    import test_cli
    env = dict(os.environ, BWAGPU_CLI_STREAMS="2", BWAGPU_CLI_SERIALIZE="1", BWAGPU_PTAB_M="6")
    run_cli(test_cli._sim_cli(), sim.prefix, tmp_path, sim.g, 18, 6, 711, 3600, env, CLI_SETS_THIN)      # (twelve pairs per batch: id0 > 0 in the second)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [51, 52])
def test_gpu_sam_pe_flat_fuzz(gpu, seed):
    cover, n_calls = run_fuzz(gpu, seed, thin=False)
    print(f"sam_pe fuzz: {n_calls} calls; {cover}")


@pytest.mark.gpu
def test_gpu_nocigar_pairs(gpu):
    run_nocigar(gpu)


@pytest.mark.gpu
def test_gpu_crafted_mates(gpu):
    run_crafted(gpu)


@pytest.mark.gpu
def test_gpu_boundaries(gpu):
    run_boundaries(gpu)


@pytest.mark.gpu
def test_gpu_sam_pe_on_batches(gpu):
    cover, out = run_batches(gpu, 1200, 300, 801, (0, (1 << 35) + 7770))
    print(f"sam_pe: {cover}; kernel_ms {['%.3f' % x for x in out['kernel_ms']]}, {len(out['text'])} bytes, {out['n_declined']} reads declined")


@pytest.mark.gpu
def test_gpu_error_paths(gpu):
    run_error_paths(gpu)


@pytest.mark.gpu
def test_gpu_cli_samtext_pe(gpu, tmp_path):
    from bwa_amd import build as b
    _, cli = b.build_host(verbose=False)
    seen = run_cli(cli, gpu.prefix, tmp_path, gpu.g, 480, 120, 811, 150000, dict(os.environ))      # (five hundred pairs per batch)
    assert b"XA:Z:" in seen and b"SA:Z:" in seen
