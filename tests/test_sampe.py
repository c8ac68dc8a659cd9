"""A read pair decided on the device (bwagpu_batch_sampe, bwagpu_sampe_flat; bwa_amd/csrc/dev_sampe.h) against the compiled reference's own mem_sam_pe
(bwamem_pair.c:276-419), called through ctypes on oracle/_ref/libbwaref.so with malloc()ed mem_alnreg_v's (mem_matesw reallocs them) and two bseq1_t of one
name.  mem_sam_pe mutates the lists in place: afterwards they give the merged regions in marked order and every region's secondary, secondary_all and sub; the
two sam strings give, per printed line, flag, contig, position, mapQ, CIGAR, NM, AS, XS, XA and MQ.

What is compared, for every pair the rescue kernels did not decline (none may be declined here: reads are 100-150 bp, windows span at most 1500):
  * the merged lists, byte for byte, against mem_matesw driven as :291-302 drive it (test_rescue.RefRescue, with MEM_F_NO_RESCUE = 0x20 as bwamem.h has it);
  * the patched marking records against the mutated lists; the other fields of the mutated lists against the merged regions in the records' order;
  * path, why, paired, q_pe against a restatement of :309-331 fed from the reference's own mem_mark_primary_se / mem_pair; z against mem_pair's where paired;
  * every printed line rebuilt from (alns, cigs, ops) as test_alns rebuilds it, with 0x40 << i | extra_flag and the mate's bits; MQ against the mate's q_se;
  * every XA entry: a region of the read whose patched secondary_all is the printed place has this contig, strand, position, CIGAR and NM.
g[i]'s third test (:373, !p->is_alt) cannot decide anything behind mem_mark_primary_se: with ALT hits in a list it sorts them behind the others (bwamem.c:561),
so place n_pri is an ALT hit whenever it exists; the counter for it is asserted to stay zero.

1. a fuzz of bwagpu_sampe_flat on crafted pairs, with MEM_F_NO_RESCUE (lists of the test's making) and without, list lengths around the switch point;
2. real batches: run -> download -> sampe(opt, pes, id0);
3. a logarithm outside the table, the rescue kernel's limits, error paths, non-interference with cigars() / alns().
CPU: on the mock runtime (tests/hostsim), thinned.  -m gpu: everything, several seeds."""
import ctypes as C
import math

import numpy as np
import pytest

import hostapi
import refapi
import testdata
import test_alns as ta
import test_pair as tpair
import test_primary as tp
import test_rescue as tr
from bwa_amd.api import BwaGpu
from bwa_amd.structs import ALN_ALT, ALN_NOCIGAR, ALN_REV, ALNREG_DTYPE, SAMPE_DTYPE

pytestmark = pytest.mark.skipif(not refapi.have_ref(), reason="oracle/_ref not built")

LANE_MAX, STEP = 4, 64      # where the decision kernels change their form (dev_sampe.h); checked against the library under test
# (length of end 0's list, of end 1's): limit - 1, limit, limit + 1, the limit against a 1-region mate both ways, 63 / 64 / 65, 129, a few hundred
SIZES = ((3, 3), (4, 4), (5, 5), (4, 1), (1, 4), (5, 1), (1, 5), (63, 2), (2, 64), (65, 65), (129, 3), (3, 300))
F_NOPAIRING, F_ALL, F_NO_MULTI, F_NO_RESCUE, F_SOFTCLIP, F_PRIMARY5, F_KEEP_SUPP_MAPQ, F_XB = 0x4, 0x8, 0x10, 0x20, 0x200, 0x800, 0x1000, 0x2000
KINDS = ("proper", "unpaired", "multi0", "multi1", "multi01", "alt_only", "other_ctg", "far", "zsec", "alt_print", "alt_low", "alt_sec", "empty1", "empty01", "which_npri", "lowT")
STABLE = ("rb", "re", "qb", "qe", "rid", "score", "truesc", "csub", "w", "seedcov", "seedlen0", "ncomp_isalt", "frac_rep")      # what marking and mem_sam_pe leave alone
REG = ALNREG_DTYPE.itemsize
NAMES = ta.NAMES


def check_limits(dev):
    assert dev.sampe_limits() == dict(lane_max=LANE_MAX, step=STEP), "a switch point of the library moved: aim the cases at it"
    big = {max(a, b) for a, b in SIZES}
    assert {LANE_MAX - 1, LANE_MAX, LANE_MAX + 1, STEP - 1, STEP, STEP + 1, 2 * STEP + 1} <= big and max(big) > 4 * STEP
    assert (LANE_MAX, 1) in SIZES and (1, LANE_MAX) in SIZES and (LANE_MAX + 1, 1) in SIZES and (1, LANE_MAX + 1) in SIZES


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------------------
class BSeq(C.Structure):      # bseq1_t (bwa.h:27-30)
    _fields_ = [("l_seq", C.c_int), ("id", C.c_int), ("name", C.c_char_p), ("comment", C.c_char_p), ("seq", C.c_void_p), ("qual", C.c_char_p), ("sam", C.c_void_p)]


class RefSampe(tr.RefRescue):
    def __init__(self, prefix):
        super().__init__(prefix)
        self.L.mem_sam_pe.restype = C.c_int
        self.L.mem_sam_pe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]

    def merged(self, opt, pes, seqs, off, counts, regs):
        """the lists as mem_sam_pe has them when it reaches mem_mark_primary_se (RefRescue.rescue reads bit 0x8 for MEM_F_NO_RESCUE: hand it the bit there)"""
        o = tp.ref_opt()
        C.memmove(C.byref(o), C.byref(opt), C.sizeof(o))
        o.flag = (opt.flag & ~0x8) | (0x8 if opt.flag & F_NO_RESCUE else 0)
        return self.rescue(o, pes, seqs, off, counts, regs)

    def sam_pe(self, opt, pes, seqs, off, counts, regs, ids):
        """mem_sam_pe of every pair (reads 2p, 2p + 1; the pair's id is ids[2p] >> 1) -> per pair (the two lists as it leaves them, n, the lines of the two ends)"""
        regs = np.ascontiguousarray(regs, dtype=ALNREG_DTYPE)
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        ends = np.concatenate([[0], np.cumsum(counts)])
        out = []
        for p in range(len(counts) // 2):
            v = (tpair.AlnV * 2)()
            s = (BSeq * 2)()
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
                s[i].l_seq = q.shape[0]; s[i].id = r; s[i].name = b"q"; s[i].seq = q.ctypes.data
            n = self.L.mem_sam_pe(C.byref(opt), self.bns, self.pac, pes.ctypes.data, int(ids[2 * p]) >> 1, s, v)
            lists, lines = [], []
            for i in range(2):
                lists.append(np.frombuffer(C.string_at(v[i].a, v[i].n * REG), dtype=ALNREG_DTYPE).copy())
                self.L.refshim_free(v[i].a)
                lines.append([ln.split("\t") for ln in C.string_at(s[i].sam).decode().split("\n") if ln])
                self.L.refshim_free(s[i].sam)
            out.append((lists, n, lines))
        return out


def c_int(x):
    return int(x)      # (int) of a double: toward zero


def expect_decision(opt, a, m, n_pri, pr):
    """path, why, paired, q_pe by :309-331 from the reference's own marking (a: the two marked lists, m: their records, n_pri) and mem_pair record"""
    if opt.flag & F_NOPAIRING:
        return 1, 1, 0, 0
    if not n_pri[0] or not n_pri[1]:
        return 1, 2, 0, 0
    if pr["score"] <= 0:
        return 1, 4, 0, 0
    why = 0
    for i in range(2):
        j = np.arange(1, n_pri[i])
        if ((m[i]["secondary"][j] < 0) & (a[i]["score"][j] >= opt.T)).any():
            why |= 8 << i
    if why:
        return 1, why, 0, 0
    o, score_un = int(pr["score"]), int(a[0]["score"][0]) + int(a[1]["score"][0]) - opt.pen_unpaired
    subo = max(int(pr["sub"]), score_un)      # :322-329
    q_pe = c_int(6.02 * (o - subo) / opt.a + .499) - (c_int(4.343 * math.log(int(pr["n_sub"]) + 1) + .499) if pr["n_sub"] > 0 else 0)
    q_pe = c_int(min(60, max(0, q_pe)) * (1. - .5 * float(np.float32(a[0]["frac_rep"][0]) + np.float32(a[1]["frac_rep"][0]))) + .499)
    return 0, 0, int(o > score_un), q_pe


def cigar_text(ops, soft):
    return "".join(f"{x >> 4}{'MIDSH'[(x & 0xf) if soft or (x & 0xf) < 3 else 4]}" for x in ops)


def new_cover():
    return dict(paired=0, unpaired=0, multi0=0, multi1=0, multi01=0, no_pri=0, pair0_ctg=0, pair0_far=0, pair0_failed=0, nopairing=0, z_sec=0, z_sec_group=0, n_sub=0, alt_printed=0, alt_lowT=0,
                alt_sec=0, alt_not_alt=0, p1_proper=0, p1_not_proper=0, p1_one_empty=0, p1_both_empty=0, which_npri=0, below_T=0, switched=0, xa=0, lines=0, nocigar_lines=0, rescued=0, host=0, wave=0, lane=0)


def check_call(ref, opt, pes, seqs, off, counts_in, regs_in, ids, got, what, cover, ctg_off, tags=None):
    """one call's results against the reference (see the head of the file); cover: counters of what the call exercised"""
    np_ = len(counts_in) // 2
    assert got["sampe"].dtype == SAMPE_DTYPE and got["sampe"].shape[0] == np_ and len(got["kernel_ms"]) == 6 and min(got["kernel_ms"]) >= 0
    s_all = got["sampe"]
    assert not (s_all["flags"] & 1).any() and not (got["rescue"]["flags"] & 1).any(), f"{what}: pairs {np.nonzero(s_all['flags'] & 1)[0][:5]} were declined"
    assert not s_all["pad_"].any() and not (s_all["flags"] & ~3).any()
    # the merged lists, the marking before mem_sam_pe's patches, mem_pair
    wc, wr, wn = ref.merged(opt, pes, seqs, off, counts_in, regs_in)
    assert np.array_equal(got["counts"], wc), f"{what}: merged counts differ at reads {np.nonzero(got['counts'] != wc)[0][:5]}"
    assert got["regs"].tobytes() == wr.tobytes(), f"{what}: merged lists differ"
    assert np.array_equal(got["rescue"]["n_aligned"], wn), what
    cover["rescued"] += int((got["src"] < 0).sum())      # (hits the rescue put into the merged lists)
    wpri, wnp = tp.ref_primary(opt, wc, wr, ids)
    assert np.array_equal(got["n_pri"], wnp) and np.array_equal(got["pri"]["src"], wpri["src"]), f"{what}: marking order"
    e = np.concatenate([[0], np.cumsum(wc)])
    marked = wr.copy()
    for i in range(len(wc)):
        marked[e[i]:e[i + 1]] = wr[e[i]:e[i + 1]][wpri["src"][e[i]:e[i + 1]]]
    wpairs = tpair.ref_pairs(ref, opt, pes, ctg_off, wc, wnp, marked, ids[::2] >> 1)
    tpair.assert_pairs_equal(got["pairs"], wpairs, f"{what}: pair records", flags_zero=False)
    # region level: mem_reg2aln of every merged region under the PATCHED marking is checked through the printed lines below; here the fields marking alone decides
    alns, cigs, ops, pri = got["alns"], got["cigs"], got["ops"], got["pri"]
    assert alns.shape[0] == cigs.shape[0] == pri.shape[0] == wr.shape[0]
    base = np.repeat(e[:-1], wc)
    cig_of = cigs[base + pri["src"]] if wr.shape[0] else cigs[:0]
    nocig = (alns["flags"] & ALN_NOCIGAR) != 0
    assert np.array_equal(nocig, cig_of["n_cigar"] == -1), what
    assert not (nocig & (alns["score"] >= opt.T)).any(), f"{what}: a region that reaches T has no CIGAR record: the comparison would leave it out"
    assert np.array_equal(alns["score"], marked["score"]) and not alns["pad_"].any()
    sam = ref.sam_pe(opt, pes, seqs, off, counts_in, regs_in, ids)
    for p in range(np_):
        s = s_all[p]
        lists, n, lines = sam[p]
        assert n == wn[p]
        lo = [int(e[2 * p]), int(e[2 * p + 1])]; hi = [int(e[2 * p + 1]), int(e[2 * p + 2])]
        a = [marked[lo[i]:hi[i]] for i in range(2)]; m0 = [wpri[lo[i]:hi[i]] for i in range(2)]
        npri = [int(wnp[2 * p]), int(wnp[2 * p + 1])]
        tag = f"{what}: pair {p}" + (f" ({tags[p]})" if tags else "")
        # the lists as mem_sam_pe left them
        for i in range(2):
            L, pr_ = lists[i], pri[lo[i]:hi[i]]
            assert L.shape[0] == hi[i] - lo[i], tag
            for f in STABLE:
                assert np.array_equal(L[f], a[i][f]), (tag, i, f)
            for f in ("secondary", "secondary_all", "sub"):
                assert np.array_equal(pr_[f], L[f]), f"{tag}, end {i}: {f}: device {pr_[f][:12].tolist()}, reference {L[f][:12].tolist()}"
            cover["switched"] += int(not np.array_equal(L["secondary_all"], m0[i]["secondary_all"]))
        path, why, paired, q_pe = expect_decision(opt, a, m0, npri, wpairs[p])
        assert (int(s["path"]), int(s["why"]), int(s["paired"]), int(s["q_pe"])) == (path, why, paired, q_pe), f"{tag}: path, why, paired, q_pe: device {s}, expected {(path, why, paired, q_pe)}"
        cover["host"] += int(bool(s["flags"] & 2))
        big = max(hi[0] - lo[0], hi[1] - lo[1])
        cover["wave" if big > LANE_MAX else "lane"] += 1
        recs = [alns[lo[i]:hi[i]] for i in range(2)]
        if path == 0:
            z = [int(wpairs[p]["z"][i]) if paired else 0 for i in range(2)]
            assert s["z"].tolist() == z, f"{tag}: z {s['z']}, mem_pair's {z}"
            cover["paired" if paired else "unpaired"] += 1
            cover["n_sub"] += int(wpairs[p]["n_sub"] > 0)
            for i in range(2):
                fired = paired and m0[i]["secondary"][z[i]] >= 0
                cover["z_sec"] += int(fired)
                if fired:
                    k = int(m0[i]["secondary_all"][z[i]])
                    grp = np.nonzero(m0[i]["secondary_all"] == k)[0]
                    cover["z_sec_group"] += int((grp < z[i]).any() and (grp > z[i]).any())
                    assert lists[i]["secondary"][z[i]] == -2
                sel = recs[i]["sel"]
                assert int(sel[z[i]]) == 0 and int(recs[i]["mapq_out"][z[i]]) == int(s["q_se"][i]), tag
                alt = int(s["alt"][i])
                if npri[i] < a[i].shape[0]:
                    g = a[i][npri[i]]; gs = lists[i]["secondary"][npri[i]]
                    t1, t2, t3 = g["score"] < opt.T, gs >= 0, not (int(g["ncomp_isalt"]) >> 30)
                    cover["alt_lowT"] += int(t1); cover["alt_sec"] += int(not t1 and t2); cover["alt_not_alt"] += int(not t1 and not t2 and t3)
                    cover["alt_printed"] += int(not (t1 or t2 or t3))
                    assert alt == (-1 if (t1 or t2 or t3) else npri[i]), tag
                else:
                    assert alt == -1
                assert int(s["n_aa"][i]) == 1 + (alt >= 0) == int(got["n_aln"][2 * p + i]), tag
                want_sel = np.full(sel.shape[0], -1); want_sel[z[i]] = 0
                if alt >= 0:
                    want_sel[alt] = 1
                assert np.array_equal(sel, want_sel), tag
                cover["below_T"] += int(a[i]["score"][z[i]] < opt.T)
        else:
            cover["nopairing"] += int(why == 1); cover["no_pri"] += int(why == 2)
            cover["multi0"] += int(why == 8); cover["multi1"] += int(why == 16); cover["multi01"] += int(why == 24)
            if why == 4:
                same = a[0]["rid"][0] == a[1]["rid"][0]      # (the best hits: on other contigs, or on one contig outside every window)
                cover["pair0_failed" if pes["failed"].all() else "pair0_far" if same else "pair0_ctg"] += 1
            cover["p1_proper" if s["extra_flag"] == 3 else "p1_not_proper"] += 1
            empty = int(a[0].shape[0] == 0) + int(a[1].shape[0] == 0)
            cover["p1_one_empty"] += int(empty == 1); cover["p1_both_empty"] += int(empty == 2)
            for i in range(2):
                w = int(s["z"][i])
                cover["which_npri"] += int(w > 0 and w == npri[i])
                assert int(s["alt"][i]) == -1 and int(s["n_aa"][i]) == int(got["n_aln"][2 * p + i]), tag
                if w >= 0:
                    assert a[i]["score"][w] >= opt.T and (w == 0 or (w == npri[i] and a[i]["score"][0] < opt.T)), tag
                    assert int(s["q_se"][i]) == int(recs[i]["mapq"][w]), tag
                else:
                    assert int(s["q_se"][i]) == 0 and (a[i].shape[0] == 0 or (a[i]["score"][0] < opt.T and (npri[i] >= a[i].shape[0] or a[i]["score"][npri[i]] < opt.T))), tag
        # the printed lines
        mate = []
        for i in range(2):
            w = int(s["z"][i])
            mate.append(recs[i][w] if w >= 0 and recs[i].shape[0] else None)
        for i in range(2):
            r_all, cg, L = recs[i], cig_of[lo[i]:hi[i]], lines[i]
            kept = np.nonzero(r_all["sel"] >= 0)[0]
            kept = kept[np.argsort(r_all["sel"][kept], kind="stable")]
            assert r_all["sel"][kept].tolist() == list(range(kept.shape[0])), tag
            mt = mate[1 - i]
            m_unmapped = mt is None or int(mt["rid"]) < 0
            pe_bits = 0x1 | (0x40 << i) | int(s["extra_flag"]) | (0x8 if m_unmapped else 0) | (0x20 if (mt is not None and int(mt["flags"]) & ALN_REV) else 0)
            if kept.shape[0] == 0:
                assert len(L) == 1 and int(L[0][1]) & 0x4, f"{tag}, end {i}: no record kept, the reference prints {len(L)} lines"
                rev_copy = 0x10 if (not m_unmapped and int(mt["flags"]) & ALN_REV) else 0      # (an unmapped read takes its mate's strand, bwamem.c:861-864)
                assert int(L[0][1]) == (pe_bits | 0x4 | rev_copy), f"{tag}, end {i}: unmapped line's flag {L[0][1]}, from the records {pe_bits | 0x4 | rev_copy}"
                assert dict(t.split(":", 2)[::2] for t in L[0][11:]).get("MQ") == str(int(s["q_se"][1 - i])), tag
                continue
            assert len(L) == kept.shape[0], f"{tag}, end {i}: {kept.shape[0]} records kept, the reference prints {len(L)} lines"
            for j, k in enumerate(kept):
                r, f = r_all[k], L[j]
                fl = int(r["flag"])
                flag = (fl & 0xffff) | (0x100 if fl & 0x10000 else 0) | (0x10 if int(r["flags"]) & ALN_REV else 0) | pe_bits
                tg = dict(t.split(":", 2)[::2] for t in f[11:])
                assert tg["MQ"] == str(int(s["q_se"][1 - i])), f"{tag}, end {i}, line {j}: MQ {tg['MQ']}, the mate's q_se {int(s['q_se'][1 - i])}"
                cover["lines"] += 1
                if int(r["flags"]) & ALN_NOCIGAR:      # (a hit below T that :311-394 print all the same: the caller runs mem_reg2aln for it)
                    cover["nocigar_lines"] += 1
                    assert (flag, NAMES[int(r["rid"])], int(r["mapq_out"]), int(r["score"])) == (int(f[1]), f[2], int(f[4]), int(tg["AS"])), f"{tag}, end {i}, line {j}"
                    continue
                soft = bool(opt.flag & F_SOFTCLIP) or bool(int(r["flags"]) & ALN_ALT) or j == 0
                text = cigar_text(ta.final_cigar(r, cg[k], ops), soft)
                mine = (flag, NAMES[int(r["rid"])], int(r["pos"]) + 1, int(r["mapq_out"]), text, int(r["nm"]), int(r["score"]), int(r["sub"]) if int(r["sub"]) >= 0 else None)
                theirs = (int(f[1]), f[2], int(f[3]), int(f[4]), f[5], int(tg["NM"]), int(tg["AS"]), int(tg["XS"]) if "XS" in tg else None)
                assert mine == theirs, f"{tag}, end {i}, line {j} (place {k}):\n device    {mine}\n reference {theirs}\n record {s}"
                xa = tg.get("XB" if opt.flag & F_XB else "XA")
                if xa:      # every entry is a region whose patched secondary_all is this place
                    members = np.nonzero(pri[lo[i]:hi[i]]["secondary_all"] == k)[0]
                    have = set()
                    for t in members:
                        q = r_all[t]
                        if int(q["flags"]) & ALN_NOCIGAR:
                            continue
                        have.add((NAMES[int(q["rid"])], ("-" if int(q["flags"]) & ALN_REV else "+") + str(int(q["pos"]) + 1), cigar_text(ta.final_cigar(q, cg[t], ops), True), str(int(q["nm"]))))
                    for ent in xa.rstrip(";").split(";"):
                        assert tuple(ent.split(",")[:4]) in have, f"{tag}, end {i}, line {j}: XA entry {ent} is no region of place {k}'s group: {sorted(have)[:6]}"
                        cover["xa"] += 1
    return cover


# ---- crafted pairs ----------------------------------------------------------------------------------------------------------------------------------------
def region(rid, rb, ln, score, qb, alt=0, rng=None):
    a = tr.reg(rid, rb, ln, score, qb=qb)
    a["ncomp_isalt"] = np.uint32((1 << 30) | 1) if alt else np.uint32(1)
    a["hash"] = 0
    if rng is not None:
        a["frac_rep"] = np.float32((0.0, 0.25, 0.5)[int(rng.integers(3))])
        a["csub"] = 0 if rng.random() < 0.7 else int(rng.integers(0, max(1, score)))
    return a


class End:
    """one read cut from the genome: forward strand at [b, b + L) or the reverse complement of it"""
    def __init__(self, g, meta, c, x, L, rev):
        self.l_pac, self.off, self.c, self.L, self.rev = int(meta["l_pac"]), meta["ctg_offset"], c, L, rev
        self.b = int(self.off[c]) + x
        fwd = g[self.b:self.b + L].copy()
        self.read = tr.revcomp(fwd) if rev else fwd
        self.alt = int(meta["ctg_is_alt"][c])

    def true(self, qb, qe, score, rng=None):
        """the alignment of read[qb:qe] at its own place"""
        rb = 2 * self.l_pac - (self.b + self.L - qb) if self.rev else self.b + qb
        return region(self.c, rb, qe - qb, score, qb, self.alt, rng)

    def foreign(self, meta, c, x, qb, qe, score, rng=None):
        """read[qb:qe] laid on the forward strand somewhere else"""
        return region(c, int(self.off[c]) + x, qe - qb, score, qb, int(meta["ctg_is_alt"][c]), rng)


def make_pair(rng, g, meta, opt, kind, n0, n1):
    """One pair of the given kind with lists of n0 / n1 regions (or as many as the kind needs at least).  Windows: FR with 200 .. 600 between the ends' positions
    (tpair.make_pes('one')), under which a 'proper' pair pairs.  -> (reads, lists)"""
    ln = meta["ctg_len"]
    T = opt.T
    c = 0
    c1 = 1 if kind == "other_ctg" else 2 if kind == "alt_only" else 0
    L0, L1 = int(rng.integers(116, 151)), int(rng.integers(116, 151))
    x = int(rng.integers(3000, min(int(ln[c]), int(ln[c1])) - 9000))
    D = int(rng.integers(330, 470)) if kind != "far" else 5000      # distance of the mate's last base from end 0's first
    E0 = End(g, meta, c, x, L0, False)
    E1 = End(g, meta, c1, x + D + 1 - L1, L1, True)
    far = lambda j: 5000 + 877 * j      # places on contig 1 no window reaches
    assert int(ln[1]) > far(52) + 400 and int(ln[2]) > 2000
    A, B = [E0.true(0, L0, L0, rng)], [E1.true(0, L1, L1, rng)]
    if kind == "unpaired":
        B = [E1.foreign(meta, 1, far(0), 0, 36, 100), E1.true(0, L1, 60)]
    elif kind in ("multi0", "multi1", "multi01"):
        if kind != "multi1":
            A = [E0.true(0, L0 - 40, L0 - 40, rng)]
        if kind != "multi0":
            B = [E1.true(0, L1 - 40, L1 - 40, rng)]
    elif kind == "zsec":      # place 0 elsewhere, its group: two members elsewhere around the one that pairs, all within pen_unpaired of place 0
        B = [E1.foreign(meta, 1, far(0), 0, 36, 100), E1.foreign(meta, 1, far(1), 0, 34, 97), E1.true(0, 40, 96, rng), E1.foreign(meta, 1, far(2), 2, 36, 95)]
    elif kind in ("alt_print", "alt_low", "alt_sec", "which_npri"):
        B = [E1.true(0, L1 - 40, 25 if kind == "which_npri" else L1 - 40, rng)]
    elif kind == "empty1":
        B = []
    elif kind == "empty01":
        A, B = [], []
    elif kind == "lowT":
        A, B = [E0.true(0, L0, 25)], [E1.true(0, L1, 27)]
    # fillers.  hi: pieces of the read at their own place, scores in (34, 60]: secondaries of the list's first hit, ahead of what the kind appends behind them;
    # lo: pieces laid elsewhere with scores below T (no CIGAR is due), overlapping the first hit on the read
    tail_a, tail_b = [], []
    if kind in ("multi0", "multi01"):
        tail_a = [E0.foreign(meta, 1, far(3), L0 - 34, L0, 34)]
    if kind in ("multi1", "multi01"):
        tail_b = [E1.foreign(meta, 1, far(4), L1 - 34, L1, 34)]
    if kind == "alt_print":
        tail_b = [E1.foreign(meta, 2, 1000, L1 - 36, L1, 33)]
    elif kind == "alt_low":
        tail_b = [E1.foreign(meta, 2, 1000, L1 - 36, L1, 20)]
    elif kind == "alt_sec":
        tail_b = [E1.foreign(meta, 2, 1000, 0, 36, 33)]
    elif kind == "which_npri":
        tail_b = [E1.foreign(meta, 2, 1000, L1 - 36, L1, 50)]
    def fill(E, lst, tail, n, span_hi):
        need = n - len(lst) - len(tail)
        if not lst or need <= 0:
            return lst + tail
        first = lst[0]
        top = int(first["score"][0])
        n_hi = need // 2 if top > 62 and kind not in ("unpaired", "zsec") else 0
        out = list(lst)
        for j in range(n_hi):
            qb = int(rng.integers(0, span_hi - 36)); w = int(rng.integers(30, 37))
            out.append(E.true(qb, qb + w, int(rng.integers(35, 61)), rng))
        q0 = int(first["qb"][0])
        for j in range(need - n_hi):
            out.append(E.foreign(meta, 1, far(10 + j % 40) + j, q0 + int(rng.integers(0, 3)), q0 + 32, int(rng.integers(5, T))))
        return out + tail
    A = fill(E0, A, tail_a, n0, L0 - 40)
    B = fill(E1, B, tail_b, n1, L1 - 40)
    pack = lambda lst: np.concatenate(lst)[np.argsort(-np.concatenate(lst)["score"], kind="stable")] if lst else np.zeros(0, dtype=ALNREG_DTYPE)
    return [E0.read, E1.read], [pack(A), pack(B)]


def opt_sets():
    out = []
    for name, fl in (("default", 0), ("nopairing", F_NOPAIRING), ("-a", F_ALL), ("-M", F_NO_MULTI), ("-Y", F_SOFTCLIP), ("XB", F_XB), ("-q", F_KEEP_SUPP_MAPQ)):
        o = tp.ref_opt()
        o.flag |= fl
        o.max_matesw = 3
        out.append((name, o))
    return out


def fuzz_cells(thin, seed):
    """(kind, n0, n1): every kind at every size, or (thin) every kind at two sizes dealt round, every size at least once"""
    cells = []
    for ki, kind in enumerate(KINDS):
        sizes = SIZES if not thin else [SIZES[(ki + seed) % len(SIZES)], SIZES[(ki * 5 + seed + 3) % len(SIZES)]]
        cells += [(kind, a, b) for a, b in sizes]
    if thin:
        seen = {(a, b) for _, a, b in cells}
        cells += [("proper" if j % 2 else "multi01", a, b) for j, (a, b) in enumerate(SIZES) if (a, b) not in seen]
    return cells


def build_call(rng, g, meta, opt, cells):
    reads, lists, tags = [], [], []
    for kind, n0, n1 in cells:
        r, l = make_pair(rng, g, meta, opt, kind, n0, n1)
        reads += r; lists += l; tags.append(f"{kind} {l[0].shape[0]}+{l[1].shape[0]}")
    seqs, off = testdata.ragged(reads)
    counts = np.array([a.shape[0] for a in lists], dtype=np.int32)
    return seqs, off, counts, np.concatenate(lists), tags


class World(ta.World):
    def __init__(self, tmp, lib_path=None, options=None):
        super().__init__(tmp, lib_path, options)
        self.ref = RefSampe(self.prefix)

    def close(self):
        self.ref.close()
        super().close()


def run_fuzz(W, seed, thin):
    dev = W.dev
    check_limits(dev)
    meta = dev.index_meta()
    assert meta["ctg_is_alt"].tolist() == [0, 0, 1]
    rng = np.random.default_rng(seed)
    total = new_cover()
    cells = fuzz_cells(thin, seed)
    assert {(a, b) for _, a, b in cells} == set(SIZES)
    sets = opt_sets()
    for oi, (name, opt) in enumerate(sets):
        if thin and oi and oi != 1 + seed % (len(sets) - 1):      # (thinned: the default set, MEM_F_NOPAIRING... one of the others per seed; the crafted lists again below)
            sub = cells[oi::len(sets)]
        else:
            sub = cells
        for rescue in (False, True):
            for variant in ("one", "failed") if (rescue is False and oi == 0) else ("one",):
                pes = tr.fuzz_pes(variant)
                o = tp.ref_opt()
                C.memmove(C.byref(o), C.byref(opt), C.sizeof(o))
                if not rescue:
                    o.flag |= F_NO_RESCUE
                use = sub if not rescue or not thin else sub[::3]
                seqs, off, counts, regs, tags = build_call(rng, W.g, meta, o, use)
                ids = int(rng.integers(0, 1 << 20)) * 2 + np.arange(counts.shape[0], dtype=np.int64) + ((1 << 35) if oi == 2 else 0)
                got = dev.sampe_flat(o, pes, seqs, off, counts, regs, ids)
                if not rescue:
                    assert np.array_equal(got["counts"], counts) and got["regs"].tobytes() == regs.tobytes() and (got["rescue"]["n_aligned"] == 0).all(), "MEM_F_NO_RESCUE: the lists pass unchanged"
                cover = check_call(W.ref, o, pes, seqs, off, counts, regs, ids, got, f"fuzz seed {seed}, options {name}, rescue {rescue}, windows {variant}", new_cover(), meta["ctg_offset"], tags)
                for k, v in cover.items():
                    total[k] += v
                if name == "nopairing":
                    assert cover["nopairing"] == len(use)
    for k in ("paired", "unpaired", "multi0", "multi1", "multi01", "no_pri", "pair0_ctg", "pair0_far", "pair0_failed", "nopairing", "z_sec", "z_sec_group", "n_sub", "alt_printed", "alt_lowT", "alt_sec",
              "p1_proper", "p1_not_proper", "p1_one_empty", "p1_both_empty", "which_npri", "below_T", "switched", "xa", "lines", "nocigar_lines", "rescued", "wave", "lane"):
        assert total[k] > 0, f"the fuzz never reached case {k}: {total}"
    assert total["alt_not_alt"] == 0      # (see the head of the file)
    assert total["host"] == 0, "a record was left to the host's log() with the default table"
    return total


# ---- real batches -----------------------------------------------------------------------------------------------------------------------------------------
def run_batches(W, n_pairs, n_foreign, seed, id0s):
    opt = tp.ref_opt()
    dev = W.dev
    reads, _, _ = tpair.pe_reads(W.g, n_pairs, n_foreign, seed)
    seqs, off = testdata.flat(reads)
    dev.upload(seqs, off); dev.run(opt)
    counts, regs = dev.download()
    pes = W.ref.pestat(opt, counts, regs)
    assert not pes["failed"].all(), "mem_pestat found no orientation: the batch is too small"
    meta = dev.index_meta()
    total = new_cover()
    for id0 in id0s:
        assert id0 % 2 == 0
        ids = id0 + np.arange(counts.shape[0], dtype=np.int64)
        got = dev.sampe(opt, pes, id0)
        check_call(W.ref, opt, pes, seqs, off, counts, regs, ids, got, f"batch of {n_pairs + n_foreign} pairs, id0 {id0}", total, meta["ctg_offset"])
    assert total["paired"] > 0 and total["rescued"] > 0 and total["lines"] >= 2 * (n_pairs + n_foreign), total
    return got, total


def run_log_cap(W):
    """a table of logarithms too short for log(n_sub + 1): the host side of the call computes the record, and nothing differs"""
    dev = W.dev
    meta = dev.index_meta()
    rng = np.random.default_rng(77)
    opt = tp.ref_opt(); opt.flag |= F_NO_RESCUE
    pes = tr.fuzz_pes("one")
    cells = [("proper", 3, 9), ("proper", 2, 70), ("zsec", 3, 5), ("multi0", 3, 3), ("far", 2, 2)]
    seqs, off, counts, regs, tags = build_call(rng, W.g, meta, opt, cells)
    ids = 40 + np.arange(counts.shape[0], dtype=np.int64)
    want = dev.sampe_flat(opt, pes, seqs, off, counts, regs, ids)
    assert (want["pairs"]["n_sub"][:2] > 0).all() and not (want["sampe"]["flags"] & 2).any()
    dev.set_option("pri_log_cap", 2)
    try:
        got = dev.sampe_flat(opt, pes, seqs, off, counts, regs, ids)
    finally:
        dev.set_option("pri_log_cap", 0)
    assert (got["sampe"]["flags"][:2] & 2).all(), got["sampe"]["flags"]
    for k in ("regs", "pairs", "alns", "n_aln", "n_pri"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert hostapi.decode_cigars(got["cigs"], got["ops"]) == hostapi.decode_cigars(want["cigs"], want["ops"])      # (the operation array's order is the order the waves finish in)
    for f in SAMPE_DTYPE.names:
        if f != "flags":
            assert np.array_equal(got["sampe"][f], want["sampe"][f]), f
    for f in ("src", "secondary", "secondary_all", "sub", "alt_sc", "sub_n", "mapq"):
        assert np.array_equal(got["pri"][f], want["pri"][f]), f
    check_call(W.ref, opt, pes, seqs, off, counts, regs, ids, got, "a two-entry table of logarithms", new_cover(), meta["ctg_offset"], tags)


def run_limits(W):
    """a 600 bp mate: the rescue kernels decline the pair, the record says so and the host route still gives the reference's SAM; the other pairs are decided"""
    dev = W.dev
    meta = dev.index_meta()
    rng = np.random.default_rng(5)
    opt = tp.ref_opt()
    pes = tr.fuzz_pes("one")
    reads, lists = [], []
    for f in ("rescued", "equal", "rescued"):
        r, l = tr.make_case(rng, W.g, meta, opt, pes, f, 3)
        reads += r; lists += l
    fo = int(meta["ctg_offset"][0])
    x = int(lists[2]["rb"][0]) - fo
    reads[3] = tr.revcomp(W.g[fo + x + 100:fo + x + 700])
    seqs, off = testdata.ragged(reads)
    counts = np.array([a.shape[0] for a in lists], dtype=np.int32)
    regs = np.concatenate(lists)
    ids = 10 + np.arange(6, dtype=np.int64)
    got = dev.sampe_flat(opt, pes, seqs, off, counts, regs, ids)
    s = got["sampe"]
    assert (s["flags"] & 1).tolist() == [0, 1, 0] and s["path"].tolist()[1] == -1 and set(s["path"].tolist()[::2]) <= {0, 1}
    for f in SAMPE_DTYPE.names:
        if f not in ("path", "flags"):
            assert not np.asarray(s[f][1]).any(), f
    e = np.concatenate([[0], np.cumsum(got["counts"])]); ein = np.concatenate([[0], np.cumsum(counts)])
    for i in (2, 3):      # the declined pair's lists are the caller's: mem_sam_pe on them is the host route, and the reference itself
        assert got["regs"][e[i]:e[i + 1]].tobytes() == regs[ein[i]:ein[i + 1]].tobytes()
    from bwa_amd.structs import MEM_F_PE
    o = tp.ref_opt(); o.flag |= MEM_F_PE
    pair = slice(int(ein[2]), int(ein[4]))
    s1, o1 = testdata.ragged(reads[2:4])
    sam_host = W.host.regs2sam(o, ["p1", "p1"], s1, None, o1, counts[2:4], regs[pair], n_processed=int(ids[2]), pes0=pes.ctypes.data)
    sam_ref = W.idx.regs2sam(o, ["p1", "p1"], np.ascontiguousarray(s1).tobytes(), None, o1, counts[2:4], regs[pair], n_processed=int(ids[2]), pes0=pes.ctypes.data)
    assert sam_host == sam_ref and sam_ref.count(b"\n") >= 2
    keep = np.array([True, True, False, False, True, True])
    sub_reads = [r for i, r in enumerate(reads) if keep[i]]; sub_lists = [l for i, l in enumerate(lists) if keep[i]]
    s2, o2 = testdata.ragged(sub_reads)
    c2 = np.array([a.shape[0] for a in sub_lists], dtype=np.int32)
    got2 = dev.sampe_flat(opt, pes, s2, o2, c2, np.concatenate(sub_lists), ids[keep])
    check_call(W.ref, opt, pes, s2, o2, c2, np.concatenate(sub_lists), ids[keep], got2, "the pairs beside a declined one", new_cover(), meta["ctg_offset"])
    for f in SAMPE_DTYPE.names:
        assert np.array_equal(s[f][::2], got2["sampe"][f]), f


def run_non_interference(W):
    """A sampe() call leaves the handle's CIGAR records and operation array of an earlier cigars() call alone: the operation array fetched again and alns() give the
    same bytes before and after.  A NEW cigars() call is compared decoded: bwagpu_batch_cigars is not byte-reproducible between two calls on any tree -- records with
    more than six operations, or an MD string of more than eight characters, point into the operation array, whose slots are handed out in the order the waves finish."""
    opt = tp.ref_opt()
    dev = W.dev
    reads, _, _ = tpair.pe_reads(W.g, 12, 4, 91)
    seqs, off = testdata.flat(reads)
    dev.upload(seqs, off); dev.run(opt)
    counts, regs = dev.download()
    pes = W.ref.pestat(opt, counts, regs) if counts.sum() else tr.fuzz_pes("one")
    if pes["failed"].all():
        pes = tr.fuzz_pes("one")
    cig0 = dev.cigars(opt); ops0 = dev.cigar_ops()
    aln0 = dev.alns(opt, 6)
    got = dev.sampe(opt, pes, 6)
    assert got["sampe"].shape[0] == 16
    aln1 = dev.alns(opt, 6)      # (on the CIGAR records of the call before sampe())
    for x, y in zip(aln0[:4], aln1[:4]):
        assert x.tobytes() == y.tobytes()
    assert dev.cigar_ops().tobytes() == ops0.tobytes()      # (the handle's operation array of that call, fetched again: untouched)
    # a new cigars() call: the same records (two calls lay their operation arrays out in the order their waves finish, so the records are compared decoded)
    dec0 = hostapi.decode_cigars(cig0, ops0)
    cig1 = dev.cigars(opt)
    assert hostapi.decode_cigars(cig1, dev.cigar_ops()) == dec0
    for x, y in zip(aln0[:4], dev.alns(opt, 6)[:4]):
        assert x.tobytes() == y.tobytes()
    again = dev.sampe(opt, pes, 6)
    assert again["alns"].tobytes() == got["alns"].tobytes() and again["sampe"].tobytes() == got["sampe"].tobytes() and again["pri"].tobytes() == got["pri"].tobytes()
    assert hostapi.decode_cigars(again["cigs"], again["ops"]) == hostapi.decode_cigars(got["cigs"], got["ops"])


def run_error_paths(W):
    from bwa_amd.structs import PeOut
    opt = tp.ref_opt()
    dev = W.dev
    L, h = dev.L, dev.h
    pes = tpair.make_pes("one")
    P = pes.ctypes.data
    reads, _, _ = tpair.pe_reads(W.g, 3, 0, 5)
    cnt = np.zeros(6, dtype=np.int32)
    o = PeOut()
    dev.upload(*testdata.flat(reads))
    call = lambda *a: L.bwagpu_batch_sampe(*a)
    ok = lambda: [h, C.byref(opt), P, 0, cnt.ctypes.data, C.byref(o)]
    def free(o):
        for f in ("regs", "src", "rescue", "pri", "n_pri", "pairs", "sampe", "cigs", "ops", "alns", "n_aln"):
            assert getattr(o, f)
            L.bwagpu_free(C.c_void_p(getattr(o, f)))
    assert call(*ok()) == -2, "before a run"
    dev.run(opt)
    assert call(*ok()) == -2, "before a download"
    counts, regs = dev.download()
    for k in (0, 1, 2, 4, 5):      # NULL h, opt, pes, counts, out
        a = ok(); a[k] = None
        assert call(*a) == -2, k
    a = ok(); a[3] = 7
    assert call(*a) == -2, "odd id0"
    o5 = tp.ref_opt(); o5.flag |= F_PRIMARY5
    a = ok(); a[1] = C.byref(o5)
    assert call(*a) == -2 and not o.regs and not o.sampe, "MEM_F_PRIMARY5"
    assert call(*ok()) == 0 and o.n_regs >= int(counts.sum())      # (no bwagpu_batch_cigars call before it)
    free(o)
    dev.upload(*testdata.flat(reads[:3])); dev.run(opt); dev.download()
    assert call(*ok()) == -2, "odd number of reads"
    dev.upload(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64)); dev.run(opt); dev.download()
    got = dev.sampe(opt, pes, 0)
    assert got["sampe"].shape[0] == 0 and got["regs"].shape[0] == 0 and got["alns"].shape[0] == 0
    # bwagpu_sampe_flat
    rng = np.random.default_rng(3)
    rd, ls = tr.make_case(rng, W.g, dev.index_meta(), opt, pes, "rescued", 2)
    seqs, off = testdata.ragged(rd)
    c2 = np.array([a.shape[0] for a in ls], dtype=np.int32); r2 = np.concatenate(ls); ids = np.array([4, 5], dtype=np.int64)
    flat = lambda *a: L.bwagpu_sampe_flat(*a)
    okf = lambda: [h, C.byref(opt), P, 1, seqs.ctypes.data, off.ctypes.data, c2.ctypes.data, r2.ctypes.data, ids.ctypes.data, cnt.ctypes.data, C.byref(o)]
    for k in (0, 1, 2, 4, 5, 6, 7, 8, 9, 10):
        a = okf(); a[k] = None
        assert flat(*a) == -2, k
    a = okf(); a[3] = -1
    assert flat(*a) == -2
    a = okf(); a[1] = C.byref(o5)
    assert flat(*a) == -2, "MEM_F_PRIMARY5"
    r3 = r2.copy(); r3["rid"][0] = int(dev.index_meta()["n_seqs"])
    a = okf(); a[7] = r3.ctypes.data
    assert flat(*a) == -2, "rid outside the index"
    assert flat(*okf()) == 0 and o.n_regs == int(cnt[:2].sum())
    free(o)
    got = dev.sampe_flat(opt, pes, np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=ALNREG_DTYPE), np.zeros(0, dtype=np.int64))
    assert got["sampe"].shape[0] == 0 and got["pairs"].shape[0] == 0
    # two pairs without a single region: two unmapped records each
    got = dev.sampe_flat(opt, pes, np.zeros(400, dtype=np.uint8), np.arange(5, dtype=np.int64) * 100, np.zeros(4, dtype=np.int32), np.zeros(0, dtype=ALNREG_DTYPE), np.arange(4, dtype=np.int64))
    assert got["sampe"]["path"].tolist() == [1, 1] and got["sampe"]["why"].tolist() == [2, 2] and got["sampe"]["z"].tolist() == [[-1, -1]] * 2 and got["n_aln"].tolist() == [0] * 4


# ---- the command line -------------------------------------------------------------------------------------------------------------------------------------
TRACE = "pairs finished from the device's pair records (BWAGPU_CLI_SAMPE)"


def run_cli(cli, prefix, f1, f2, K, env, n_pairs):
    """paired-end SAM of `cli` with BWAGPU_CLI_SAMPE=1 against `bwa mem` and against the default run, byte for byte, for several option sets; the trace line
    counts the pairs finished from the records: all of them, or none where the switch is ignored (-5, -P; -S: without mate rescue the windows are not known before the
    finalize stage, the condition BWAGPU_CLI_RESCUE has too)"""
    import subprocess
    body = lambda t: b"\n".join(l for l in t.split(b"\n") if not l.startswith(b"@PG"))
    def run(exe, extra, e=None):
        p = subprocess.run([exe, "mem", "-K", str(K), "-t", "2"] + extra + [prefix, f1, f2], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        return body(p.stdout), p.stderr.decode()
    e_off = dict(env, BWAGPU_CLI_TRACE="1"); e_off.pop("BWAGPU_CLI_SAMPE", None)
    e_on = dict(e_off, BWAGPU_CLI_SAMPE="1")
    seen = b""
    for extra in ([], ["-a"], ["-M", "-Y"], ["-S"], ["-5"], ["-P"]):
        want, _ = run(refapi.REF_BWA, extra)
        assert want.count(b"\n") >= 2 * n_pairs
        on, err_on = run(cli, extra, e_on)
        assert on == want, f"BWAGPU_CLI_SAMPE=1 {extra}: SAM differs from bwa mem"
        line = [l for l in err_on.split("\n") if TRACE in l]
        assert len(line) == 1, err_on[-1500:]
        n = int(line[0].split("]")[1].split()[0])
        assert n == (0 if extra in (["-5"], ["-P"], ["-S"]) else n_pairs), (extra, n, n_pairs)
        if not extra:
            off, err_off = run(cli, extra, e_off)
            assert off == want and TRACE not in err_off, "the switch is off by default"
        seen += want
    return seen


# ---- fixtures and tests -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    import hostsim_build
    w = World(tmp_path_factory.mktemp("sampe_sim"), lib_path=hostsim_build.build(), options={"ptab_m": 6})
    yield w
    w.close()


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    w = World(tmp_path_factory.mktemp("sampe_gpu"))
    yield w
    w.close()


def test_struct_and_limits(sim):
    assert SAMPE_DTYPE.itemsize == sim.dev.L.bwagpu_sampe_size() == 64
    check_limits(sim.dev)


def test_sim_sampe_flat_fuzz(sim):
    run_fuzz(sim, 41, thin=True)


def test_sim_sampe_on_batches(sim):
    run_batches(sim, 28, 8, 701, (0, (1 << 35) + 7770))


def test_sim_sampe_log_cap(sim):
    run_log_cap(sim)


def test_sim_sampe_limits(sim):
    run_limits(sim)


def test_sim_non_interference(sim):
    run_non_interference(sim)


def test_error_paths(sim):
    run_error_paths(sim)


def test_sim_cli_sampe(sim, tmp_path):
    import os
    import test_cli
    f1, f2 = tpair.cli_inputs(tmp_path, sim.g, 32, 8, 711)
    env = dict(os.environ, BWAGPU_CLI_STREAMS="2", BWAGPU_CLI_SERIALIZE="1", BWAGPU_PTAB_M="6")
    run_cli(test_cli._sim_cli(), sim.prefix, f1, f2, 6000, env, 40)      # (twenty pairs per batch: id0 > 0 in the second)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [41, 42])
def test_gpu_sampe_flat_fuzz(gpu, seed):
    run_fuzz(gpu, seed, thin=False)


@pytest.mark.gpu
def test_gpu_sampe_on_batches(gpu):
    got, total = run_batches(gpu, 1600, 400, 801, (0, (1 << 35) + 7770))
    print(f"sampe: {total}; kernel_ms {['%.3f' % x for x in got['kernel_ms']]}")


@pytest.mark.gpu
def test_gpu_sampe_log_cap(gpu):
    run_log_cap(gpu)


@pytest.mark.gpu
def test_gpu_sampe_limits(gpu):
    run_limits(gpu)


@pytest.mark.gpu
def test_gpu_non_interference(gpu):
    run_non_interference(gpu)


@pytest.mark.gpu
def test_gpu_cli_sampe(tmp_path):
    import os
    from bwa_amd import build as b
    _, cli = b.build_host(verbose=False)
    fa, g = testdata.medium_index()
    alt = tp.alt_prefix(tmp_path, fa, ["chr3"])
    f1, f2 = tpair.cli_inputs(tmp_path, g, 1600, 400, 811)
    seen = run_cli(cli, alt, f1, f2, 150000, dict(os.environ), 2000)      # (five hundred pairs per batch)
    assert b"XA:Z:" in seen and b"\tpa:f:" in seen
