"""The merge of mate-rescue hits on the device (bwagpu_batch_rescue, bwagpu_rescue_flat; bwa_amd/csrc/dev_rescue.h) against the compiled reference itself:
mem_sam_pe's rescue loop (bwamem_pair.c:291-302) restated as a plain loop over the reference's own mem_matesw, then its mem_mark_primary_se and mem_pair, all
called through ctypes on oracle/_ref/libbwaref.so with bns / pac of the loaded index.  mem_matesw reallocs ma->a, so the lists live in libc malloc()ed arrays.
The merged lists must be equal byte for byte (all 88 bytes of every record), and so must counts, n_aligned, the marking records and the pair records.

1. a fuzz of bwagpu_rescue_flat on crafted pairs: mates cut from the genome at chosen places, lists written by the test, list sizes around every switch point
   of the kernels (bwagpu_rescue_limits);
2. real batches: run -> download -> rescue(opt, pes, id0) with pes from the reference's mem_pestat;
3. the alignment kernel's limits: a 600 bp mate and a window of more than 2048 columns flag their pair and leave the others alone;
4. error paths.
CPU: on the mock runtime (tests/hostsim), thinned.  -m gpu: everything, three seeds.
Reads are 100-150 bp and windows span at most 1500 in 1, 2: no pair may be flagged there."""
import ctypes as C

import numpy as np
import pytest

import refapi
import testdata
import test_pair as tpair
import test_primary as tp
from bwa_amd.api import BwaGpu
from bwa_amd.structs import ALNREG_DTYPE, PESTAT_DTYPE, RESCUE_DTYPE

pytestmark = pytest.mark.skipif(not refapi.have_ref(), reason="oracle/_ref not built")

# where the kernels change their form (dev_rescue.h): the capacity of a pair's larger end (its regions + 4 per anchor of the other end)
LANE_MAX, LDS_MAX = 16, 256
# regions of the mate's list besides what the family itself puts there (the anchor end has one or two anchors: capacity = these + the family's + 4 or 8)
FILLERS = (0, 1, 11, 12, 13, 150, 251, 252, 253, 300)
FAMILIES = ("rescued", "consistent", "threshold", "anchors", "equal", "identical", "removal", "shared_re", "poor", "edge", "empty", "withN")
REG = ALNREG_DTYPE.itemsize


def form_of(cap):
    return 0 if cap <= LANE_MAX else 1 if cap <= LDS_MAX else 2


def check_limits(dev):
    assert dev.rescue_limits() == dict(lane_max=LANE_MAX, lds_max=LDS_MAX), "a switch point of the library moved: aim the cases at it"


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------------------
class RefRescue(tpair.Ref):
    def __init__(self, prefix):
        super().__init__(prefix)
        L = self.L
        self.pac = L.refshim_idx_pac(self.idx.h)
        L.mem_matesw.restype = C.c_int
        L.mem_matesw.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        self.libc = C.CDLL(None)
        self.libc.malloc.restype = C.c_void_p
        self.libc.malloc.argtypes = [C.c_size_t]

    def rescue(self, opt, pes, seqs, off, counts, regs):
        """mem_sam_pe's rescue loop for every pair -> (merged counts, merged lists, n per pair)"""
        regs = np.ascontiguousarray(regs, dtype=ALNREG_DTYPE)
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        ends = np.concatenate([[0], np.cumsum(counts)])
        out_counts = np.zeros(len(counts), dtype=np.int32)
        out, ns = [], []
        for p in range(len(counts) // 2):
            v = (tpair.AlnV * 2)()
            b = []
            for i in range(2):
                a = regs[ends[2 * p + i]:ends[2 * p + i + 1]]
                v[i].a = self.libc.malloc(max(1, a.shape[0]) * REG)
                v[i].n = v[i].m = a.shape[0]
                if a.shape[0]:
                    C.memmove(v[i].a, a.ctypes.data, a.shape[0] * REG)
                b.append(np.ascontiguousarray(a[a["score"] >= a["score"][0] - opt.pen_unpaired]) if a.shape[0] else a)      # (:291-294: a snapshot)
            n = 0
            if not (opt.flag & 0x8):
                for i in range(2):
                    m = 2 * p + (1 - i)
                    for j in range(min(b[i].shape[0], opt.max_matesw)):
                        n += self.L.mem_matesw(C.byref(opt), self.bns, self.pac, pes.ctypes.data, b[i].ctypes.data + j * REG, int(off[m + 1] - off[m]),
                                               seqs.ctypes.data + int(off[m]), C.byref(v[1 - i]))
            for i in range(2):
                out_counts[2 * p + i] = v[i].n
                out.append(np.frombuffer(C.string_at(v[i].a, v[i].n * REG), dtype=ALNREG_DTYPE).copy())
                self.L.refshim_free(v[i].a)
            ns.append(n)
        return out_counts, (np.concatenate(out) if out else np.zeros(0, dtype=ALNREG_DTYPE)), np.array(ns, dtype=np.int32)


def ref_all(ref, opt, pes, ctg_off, seqs, off, counts, regs, ids):
    wc, wr, wn = ref.rescue(opt, pes, seqs, off, counts, regs)
    wpri, wnp = tp.ref_primary(opt, wc, wr, ids)
    marked = wr.copy()
    ends = np.concatenate([[0], np.cumsum(wc)])
    for i in range(len(wc)):
        lo, hi = int(ends[i]), int(ends[i + 1])
        marked[lo:hi] = wr[lo:hi][wpri["src"][lo:hi]]
    wpairs = tpair.ref_pairs(ref, opt, pes, ctg_off, wc, wnp, marked, ids[::2] >> 1)
    return wc, wr, wn, wpri, wnp, wpairs


def assert_rescue_equal(got, want, counts_in, regs_in, what, with_pairs=True):
    wc, wr, wn, wpri, wnp, wpairs = want
    assert (got["rescue"]["flags"] == 0).all(), f"{what}: flagged pairs {np.nonzero(got['rescue']['flags'])[0][:5]}"
    assert np.array_equal(got["rescue"]["n_aligned"], wn), f"{what}: n_aligned differs at pairs {np.nonzero(got['rescue']['n_aligned'] != wn)[0][:5]}"
    assert np.array_equal(got["counts"], wc), f"{what}: counts differ at reads {np.nonzero(got['counts'] != wc)[0][:5]}"
    g, w = got["regs"].view(np.uint8).reshape(-1, REG), wr.view(np.uint8).reshape(-1, REG)
    if not np.array_equal(g, w):
        k = int(np.nonzero((g != w).any(axis=1))[0][0])
        raise AssertionError(f"{what}: merged lists differ; first at region {k}\n device    {got['regs'][k]}\n reference {wr[k]}")
    assert (got["rescue"]["n_inline"] >= 0).all() and (got["rescue"]["n_inline"] <= got["rescue"]["n_aligned"]).all()
    # src: a permutation-with-gaps of the downloaded list plus the rescued hits
    ein, eout = np.concatenate([[0], np.cumsum(counts_in)]), np.concatenate([[0], np.cumsum(wc)])
    for i in range(len(wc)):
        s = got["src"][eout[i]:eout[i + 1]]
        m = got["regs"][eout[i]:eout[i + 1]]
        old = s >= 0
        assert len(set(s.tolist())) == s.shape[0] and (s[old] < counts_in[i]).all(), (what, i)
        a = regs_in[ein[i]:ein[i + 1]][s[old]]
        for f in ("rb", "re", "qb", "qe", "score", "rid", "hash", "seedlen0", "w"):
            assert np.array_equal(a[f], m[f][old]), (what, i, f)
        new = m[~old]
        assert (new["secondary"] == -1).all() and (new["hash"] == 0).all() and (new["truesc"] == 0).all() and (((-1 - s[~old]) >> 2) < max(1, counts_in[i ^ 1])).all()
    if with_pairs:
        tp.assert_records_equal(got["pri"], got["n_pri"], wpri, wnp, wc, f"{what}: marking records")
        tpair.assert_pairs_equal(got["pairs"], wpairs, f"{what}: pair records")


# ---- crafted pairs ----------------------------------------------------------------------------------------------------------------------------------------
def revcomp(s):
    return np.where(s < 4, 3 - s, 4)[::-1].astype(np.uint8)


def fuzz_pes(variant):
    if variant == "narrow":      # (the removal family needs a window narrower than a read)
        pes = tpair.make_pes("failed")
        pes[1] = (300, 340, 0, 320.0, 10.0)
        return pes
    return tpair.make_pes(variant)      # spans of at most 1500


def reg(rid, rb, ln, score, qb=0, **kw):
    a = np.zeros(1, dtype=ALNREG_DTYPE)
    a["rid"] = rid; a["rb"] = rb; a["re"] = rb + ln; a["qb"] = qb; a["qe"] = qb + ln; a["score"] = score; a["truesc"] = score; a["seedcov"] = ln // 2; a["secondary"] = -1
    a["w"] = 100; a["seedlen0"] = 19; a["sub"] = 0; a["frac_rep"] = 0.25; a["hash"] = 12345
    for k, v in kw.items():
        a[k] = v
    return a


def make_case(rng, g, meta, opt, pes, family, n_fill):
    """One pair: end 0 carries the anchors, end 1 is the mate (FR: the mate lies downstream on the reverse strand).  -> (reads, lists)"""
    l_pac, off, ln = int(meta["l_pac"]), meta["ctg_offset"], meta["ctg_len"]
    c = 0 if family != "edge" else int(rng.integers(len(ln)))
    L0, L1 = int(rng.integers(100, 151)), int(rng.integers(100, 151))
    lo, hi = int(pes["low"][1]), int(pes["high"][1])
    narrow = hi - lo < 100
    x = int(rng.integers(2000, int(ln[c]) - 4000))
    D = hi - 9 if narrow else int(rng.integers(lo + 60, hi - 10))      # distance of the mate's last base from the anchor's first
    if family == "edge":      # windows clipped at the contig's ends / at 0 and 2 l_pac, or straddling a boundary
        x = (5, int(ln[c]) - L0 - 3, int(ln[c]) - 250, 120)[int(rng.integers(4))]
    fo = int(off[c])
    r0 = g[fo + x:fo + x + L0].copy()
    me = min(fo + x + D + 1, int(off[c]) + int(ln[c]))      # forward end of the mate
    mate_fwd = g[me - L1:me].copy()
    if family == "poor":
        mate_fwd = rng.integers(0, 4, L1).astype(np.uint8)
    elif family == "withN":
        mate_fwd[rng.integers(0, L1, 3)] = 4
    elif rng.random() < 0.5:      # a few substitutions, or an indel
        if rng.random() < 0.6:
            k = rng.integers(10, L1 - 10, 2); mate_fwd[k] = (mate_fwd[k] + 1) % 4
        else:
            k = int(rng.integers(30, L1 - 30)); mate_fwd = np.delete(mate_fwd, [k, k + 1])
    r1 = revcomp(mate_fwd); L1 = r1.shape[0]
    hit_rb = 2 * l_pac - me      # the true hit of the mate, reverse strand
    A = [reg(c, fo + x, L0, L0 * opt.a)]
    M = []
    if family == "consistent":
        M.append(reg(c, hit_rb, L1, L1 * opt.a - 7))
    elif family == "threshold":      # a second anchor exactly at best - pen_unpaired, a third one below
        A.append(reg(c, fo + x + 700, L0, L0 * opt.a - opt.pen_unpaired))
        A.append(reg(c, fo + x + 1400, L0, L0 * opt.a - opt.pen_unpaired - 1))
    elif family == "anchors":      # 0, 1, max_matesw or max_matesw + 3 anchors of equal score (max_matesw is 3 in these calls)
        k = (0, 1, opt.max_matesw, opt.max_matesw + 3)[int(rng.integers(4))]
        A = [reg(c, fo + x + 13 * j, L0, L0 * opt.a) for j in range(k)]
    elif family == "equal":      # an unrelated hit of the score the rescue will find: the new one goes behind it
        M.append(reg(c, fo + 1000 + int(rng.integers(100)), L1, L1 * opt.a))
        M.append(reg(c, fo + 1500, L1, L1 * opt.a - 1))
    elif family == "identical":      # a second anchor from which the rescued hit lies left of the window's range but inside the window: found again
        A.append(reg(c, fo + x + (D - lo) + 5, L0, L0 * opt.a))
    elif family == "removal":      # see the issue: a fragment of the true hit that only the first anchor cannot see; the second needs an alignment nobody foresaw
        assert narrow
        A.append(reg(c, fo + x - 10, L0, L0 * opt.a))
        M.append(reg(c, hit_rb + 40, L1 - 40, (L1 - 40) * opt.a - 5, qb=40))
    elif family == "shared_re":      # several regions ending at one place
        for j in range(4):
            M.append(reg(c, fo + 3000 - 20 * j - 7, 20 * j + 27, 20 + j % 2, qb=int(rng.integers(0, 60))))
    elif family == "empty":
        if rng.random() < 0.5:
            A = []
    if family == "edge" and A and rng.random() < 0.5:      # the same place as a reverse-strand anchor: the windows mirror, and those near contig 0's start clip at 2 l_pac
        A[0]["rb"] = 2 * l_pac - (fo + x + L0); A[0]["re"] = A[0]["rb"] + L0
    # fillers: unrelated regions on the forward strand, far from every window, scores below the rescue's
    if n_fill:
        cf = len(ln) - 1 if c != len(ln) - 1 else 0
        step = max(1, (int(ln[cf]) - 400) // n_fill)
        for j in rng.permutation(n_fill):
            far = int(off[cf]) + 100 + int(j) * step
            if cf == c and abs(far - (fo + x)) < 3000:
                far += 5000
            M.append(reg(cf, far, 60, 30 + int(rng.integers(0, 3)), qb=int(rng.integers(0, 30))))
    def pack(lst):
        if not lst:
            return np.zeros(0, dtype=ALNREG_DTYPE)
        a = np.concatenate(lst)
        return a[np.argsort(-a["score"], kind="stable")]      # best first, as every list mem_sam_pe sees
    return [r0, r1], [pack(A), pack(M)]


def fuzz_cells(thin, call):
    """(family, fillers): the full cross product, or (thin) every family once per form, the sizes dealt round"""
    if not thin:
        return [(f, n) for f in FAMILIES for n in FILLERS]
    cells = [("rescued", n) for n in FILLERS]      # (one anchor: capacities 15, 16, 17 and 255, 256, 257 among them)
    for form, sizes in {0: (0, 1, 4), 1: (13, 150, 240), 2: (253, 300)}.items():
        for k, f in enumerate(FAMILIES):
            cells.append((f, sizes[(k + call) % len(sizes)]))
    return cells


def run_fuzz(dev, ref, g, seed, thin):
    check_limits(dev)
    rng = np.random.default_rng(seed)
    meta = dev.index_meta()
    seen, inline = {}, {}
    for vi, (name, opt) in enumerate(tpair.opt_variants()):
        opt.max_matesw = 3 if vi != 1 else 50
        for variant in ("one", "four", "failed", "narrow") if not thin else (("one", "four", "failed")[vi], "narrow"):
            pes = fuzz_pes(variant)
            geom = fuzz_pes("one") if variant == "failed" else pes      # (all four orientations failed: the pairs are laid out as for FR, and nothing may run)
            cells = fuzz_cells(thin, vi)
            if variant == "narrow":
                cells = [(f, n) for f, n in cells if not thin or f in ("removal", "rescued")]
            else:
                cells = [(f, n) for f, n in cells if f != "removal"]
            reads, lists, fams = [], [], []
            for f, n in cells:
                r, l = make_case(rng, g, meta, opt, geom, f, n)
                reads += r; lists += l; fams.append(f)
            seqs, off = testdata.ragged(reads)
            counts = np.array([a.shape[0] for a in lists], dtype=np.int32)
            regs = np.concatenate(lists)
            ids = int(rng.integers(0, 1 << 20)) * 2 + np.arange(len(lists), dtype=np.int64)
            if vi == 2:
                ids += (1 << 35)
            want = ref_all(ref, opt, pes, meta["ctg_offset"], seqs, off, counts, regs, ids)
            got = dev.rescue_flat(opt, pes, seqs, off, counts, regs, ids)
            assert got["ms"] >= 0
            assert_rescue_equal(got, want, counts, regs, f"fuzz seed {seed}, options {name}, windows {variant}")
            if variant == "failed":
                assert (got["rescue"]["n_aligned"] == 0).all() and np.array_equal(got["counts"], counts)
            for p, f in enumerate(fams):
                n_anchor = int(min((lists[2 * p]["score"] >= lists[2 * p]["score"][0] - opt.pen_unpaired).sum(), opt.max_matesw)) if counts[2 * p] else 0
                n_back = int(min((lists[2 * p + 1]["score"] >= lists[2 * p + 1]["score"][0] - opt.pen_unpaired).sum(), opt.max_matesw)) if counts[2 * p + 1] else 0
                cap = max(int(counts[2 * p + 1]) + 4 * n_anchor, int(counts[2 * p]) + 4 * n_back)
                seen.setdefault(form_of(cap), set()).add(f)
                inline[f] = inline.get(f, 0) + int(got["rescue"]["n_inline"][p])
    for form in range(3):
        assert seen.get(form) == set(FAMILIES), (form, set(FAMILIES) - seen.get(form, set()))
    assert inline["removal"] > 0, "no pair of the removal family needed an alignment nobody precomputed"
    assert all(v == 0 for f, v in inline.items() if f != "removal"), inline
    run_mixed(dev, ref, g, seed)


def run_mixed(dev, ref, g, seed):
    """128 consecutive pairs whose capacities run through every form of the kernels within each wavefront, a cycle of seven, so the places shift from one
    wavefront to the next: the lanes' hand-over with both lists live in one ballot and no list taking a whole wavefront.  Mostly pairs that need no alignment
    (a consistent hit is there already, or no anchor): the merge and the hand-over are what is looked at."""
    rng = np.random.default_rng(seed + 1000)
    meta = dev.index_meta()
    opt = tp.ref_opt()
    opt.max_matesw = 3
    pes = fuzz_pes("one")
    fills = (0, LANE_MAX - 3, LDS_MAX - 3, 1, LANE_MAX - 4, LDS_MAX - 4, LANE_MAX)      # capacities (one anchor: these + 4, at least 13): lane, LDS, HBM, lane, lane, LDS, LDS
    reads, lists = [], []
    for i in range(128):
        r, l = make_case(rng, g, meta, opt, pes, "rescued" if i % 16 == 5 else ("consistent", "empty")[i % 2], fills[i % len(fills)])
        reads += r; lists += l
    seqs, off = testdata.ragged(reads)
    counts = np.array([a.shape[0] for a in lists], dtype=np.int32)
    regs = np.concatenate(lists)
    ids = int(rng.integers(0, 1 << 20)) * 2 + np.arange(len(lists), dtype=np.int64)
    want = ref_all(ref, opt, pes, meta["ctg_offset"], seqs, off, counts, regs, ids)
    got = dev.rescue_flat(opt, pes, seqs, off, counts, regs, ids)
    assert_rescue_equal(got, want, counts, regs, f"128 pairs of mixed forms, seed {seed}")


# ---- real batches -----------------------------------------------------------------------------------------------------------------------------------------
def run_batches(dev, ref, g, n_pairs, n_foreign, seed, id0s):
    opt = tp.ref_opt()
    reads, _, _ = tpair.pe_reads(g, n_pairs, n_foreign, seed)
    seqs, off = testdata.flat(reads)
    dev.upload(seqs, off); dev.run(opt)
    counts, regs = dev.download()
    pes = ref.pestat(opt, counts, regs)
    assert not pes["failed"].all(), "mem_pestat found no orientation: the batch is too small"
    meta = dev.index_meta()
    for id0 in id0s:
        ids = id0 + np.arange(counts.shape[0], dtype=np.int64)
        want = ref_all(ref, opt, pes, meta["ctg_offset"], seqs, off, counts, regs, ids)
        got = dev.rescue(opt, pes, id0)
        assert_rescue_equal(got, want, counts, regs, f"batch of {n_pairs + n_foreign} pairs, id0 {id0}")
    wn = want[2]
    grew = (want[0].reshape(-1, 2) > counts.reshape(-1, 2)).any(axis=1)
    assert ((wn > 0) & grew).any() and ((wn > 0) & ~grew).any() and (wn == 0).any(), (int(((wn > 0) & grew).sum()), int(((wn > 0) & ~grew).sum()), int((wn == 0).sum()))
    return got


def run_limits(dev, ref, g):
    """a 600 bp mate, and a window of more than 2048 columns: flagged, returned as downloaded; the other pairs of the call as the reference has them"""
    rng = np.random.default_rng(5)
    meta = dev.index_meta()
    opt = tp.ref_opt()
    for what in ("mate", "window"):
        pes = fuzz_pes("one")
        if what == "window":
            pes[1] = (200, 2400, 0, 1300.0, 400.0)
        reads, lists = [], []
        for f in ("rescued", "equal", "rescued"):
            r, l = make_case(rng, g, meta, opt, fuzz_pes("one"), f, 3)
            reads += r; lists += l
        if what == "mate":
            fo = int(meta["ctg_offset"][0])
            x = int(lists[2]["rb"][0]) - fo
            reads[3] = revcomp(g[fo + x + 100:fo + x + 700])
        seqs, off = testdata.ragged(reads)
        counts = np.array([a.shape[0] for a in lists], dtype=np.int32)
        regs = np.concatenate(lists)
        ids = 10 + np.arange(6, dtype=np.int64)
        got = dev.rescue_flat(opt, pes, seqs, off, counts, regs, ids)
        fl = got["rescue"]["flags"] & 1
        if what == "mate":
            assert fl.tolist() == [0, 1, 0], fl
        else:
            assert fl.all(), fl
        ein, eout = np.concatenate([[0], np.cumsum(counts)]), np.concatenate([[0], np.cumsum(got["counts"])])
        keep = np.ones(6, dtype=bool)
        for p in np.nonzero(fl)[0]:
            assert got["rescue"]["n_aligned"][p] == -1
            for i in (2 * p, 2 * p + 1):
                assert got["counts"][i] == counts[i] and got["regs"][eout[i]:eout[i + 1]].tobytes() == regs[ein[i]:ein[i + 1]].tobytes(), (what, i)
                assert got["src"][eout[i]:eout[i + 1]].tolist() == list(range(counts[i]))
                keep[i] = False
        if keep.any():      # the other pairs: as in a call without the flagged one
            sub_reads = [r for i, r in enumerate(reads) if keep[i]]; sub_lists = [l for i, l in enumerate(lists) if keep[i]]
            s2, o2 = testdata.ragged(sub_reads)
            c2 = np.array([a.shape[0] for a in sub_lists], dtype=np.int32)
            wc, wr, wn = ref.rescue(opt, pes, s2, o2, c2, np.concatenate(sub_lists))
            sel = np.concatenate([np.arange(eout[i], eout[i + 1]) for i in range(6) if keep[i]])
            assert np.array_equal(got["counts"][keep], wc) and got["regs"][sel].tobytes() == wr.tobytes()
            assert np.array_equal(got["rescue"]["n_aligned"][fl == 0], wn) and (wn > 0).any()


def run_short_window(dev, ref, g):
    """Windows clipped at 0 and at 2 l_pac to 10 columns (fewer than min_seed_len = 19: no alignment is due, n does not count it) beside their neighbours of
    exactly 19 columns (due).  Windows "four": with a forward anchor at x on contig 0 orientation 2 has the window [0, x - 100), the other three are long; with a
    reverse anchor at 2 l_pac - 1 - w (contig 0, reversed) orientation 0 has [rb + 1, 2 l_pac), w columns, orientation 1 is empty and the other two are long."""
    meta = dev.index_meta()
    opt = tp.ref_opt()
    assert opt.min_seed_len == 19
    pes = tpair.make_pes("four")
    l_pac = int(meta["l_pac"])
    assert int(meta["ctg_offset"][0]) == 0 and int(meta["ctg_len"][0]) > 4000
    rng = np.random.default_rng(9)
    reads, lists = [], []
    for rid, rb in ((0, 110), (0, 119), (0, 2 * l_pac - 1 - 10), (0, 2 * l_pac - 1 - 19)):      # (the upper end of the coordinate space is contig 0's start, reversed)
        reads += [g[3000:3120].copy(), rng.integers(0, 4, 120).astype(np.uint8)]      # (the mate matches nowhere near: the alignments run and add nothing much)
        lists += [reg(rid, rb, 5, 100), np.zeros(0, dtype=ALNREG_DTYPE)]
    seqs, off = testdata.ragged(reads)
    counts = np.array([a.shape[0] for a in lists], dtype=np.int32)
    regs = np.concatenate(lists)
    ids = 20 + np.arange(8, dtype=np.int64)
    want = ref_all(ref, opt, pes, meta["ctg_offset"], seqs, off, counts, regs, ids)
    assert want[2].tolist() == [3, 4, 2, 3], want[2]      # the reference: the 10-column windows are not aligned, the 19-column ones are
    got = dev.rescue_flat(opt, pes, seqs, off, counts, regs, ids)
    assert_rescue_equal(got, want, counts, regs, "clipped windows of 10 and 19 columns")
    assert got["rescue"]["n_aligned"].tolist() == [3, 4, 2, 3]


# ---- the command line -------------------------------------------------------------------------------------------------------------------------------------
def run_cli(cli, prefix, f1, f2, K, env, n_pairs):
    """paired-end SAM of `cli` with and without BWAGPU_CLI_RESCUE against `bwa mem`, and with the switch and -5 against `bwa mem -5`"""
    import subprocess
    body = lambda t: b"\n".join(l for l in t.split(b"\n") if not l.startswith(b"@PG"))
    def run(exe, extra, e=None):
        p = subprocess.run([exe, "mem", "-K", str(K), "-t", "2"] + extra + [prefix, f1, f2], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        return body(p.stdout), p.stderr.decode()
    want, _ = run(refapi.REF_BWA, [])
    assert want.count(b"\n") >= 2 * n_pairs
    e_off = dict(env, BWAGPU_CLI_TRACE="1"); e_off.pop("BWAGPU_CLI_RESCUE", None)
    e_on = dict(e_off, BWAGPU_CLI_RESCUE="1")
    on, err_on = run(cli, [], e_on)
    off, err_off = run(cli, [], e_off)
    assert on == want, "BWAGPU_CLI_RESCUE=1: SAM differs from bwa mem"
    assert off == want, "switch unset: SAM differs from bwa mem"
    line = [l for l in err_on.split("\n") if "pairs merged on the device (BWAGPU_CLI_RESCUE)" in l]
    assert len(line) == 1, err_on[-1500:]
    w = line[0].split("]")[1].split()
    n, m = int(w[0]), int(w[w.index("(BWAGPU_CLI_RESCUE),") + 1])
    assert n == n_pairs and m > 0, (n, m, n_pairs)
    assert "pairs merged on the device" not in err_off
    want5, _ = run(refapi.REF_BWA, ["-5"])
    on5, err5 = run(cli, ["-5"], e_on)
    assert on5 == want5, "BWAGPU_CLI_RESCUE=1 with -5: SAM differs from bwa mem -5"
    assert "pairs merged on the device" not in err5      # (the switch is ignored)
    print(f"BWAGPU_CLI_RESCUE: {n} pairs merged on the device, {m} with rescue alignments")


# ---- mock runtime -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim():
    import hostsim_build
    prefix, _ = testdata.small_index()
    s = BwaGpu(prefix, lib_path=hostsim_build.build(), options={"ptab_m": 6})
    yield s
    s.close()


@pytest.fixture(scope="module")
def ref_small():
    r = RefRescue(testdata.small_index()[0])
    yield r
    r.close()


def test_structs_and_limits(sim):
    assert RESCUE_DTYPE.itemsize == 16
    check_limits(sim)
    caps = {n + 4 for n in FILLERS}
    for lim in (LANE_MAX, LDS_MAX):
        assert {lim - 1, lim, lim + 1} <= caps | {n + 5 for n in FILLERS}, lim
    assert max(FILLERS) > LDS_MAX


def test_sim_rescue_flat_fuzz(sim, ref_small):
    run_fuzz(sim, ref_small, testdata.small_index()[1], 51, thin=True)


def test_sim_rescue_on_batches(sim, ref_small):
    run_batches(sim, ref_small, testdata.small_index()[1], 28, 8, 701, (0, (1 << 35) + 7770))


def test_sim_rescue_short_window(sim, ref_small):
    run_short_window(sim, ref_small, testdata.small_index()[1])


def test_sim_rescue_limits(sim, ref_small):
    run_limits(sim, ref_small, testdata.small_index()[1])


def test_sim_cli_rescue(tmp_path):
    import os
    import test_cli
    prefix, g = testdata.small_index()
    alt = tp.alt_prefix(tmp_path, prefix, ["chr3"])
    f1, f2 = tpair.cli_inputs(tmp_path, g, 32, 8, 711)
    env = dict(os.environ, BWAGPU_CLI_STREAMS="2", BWAGPU_CLI_SERIALIZE="1", BWAGPU_PTAB_M="6")
    run_cli(test_cli._sim_cli(), alt, f1, f2, 6000, env, 40)      # (twenty pairs per batch: id0 > 0 in the second)


def test_error_paths(sim, ref_small):
    opt = tp.ref_opt()
    L, h = sim.L, sim.h
    pes = tpair.make_pes("one")
    P = pes.ctypes.data
    g = testdata.small_genome()[0]
    reads, _, _ = tpair.pe_reads(g, 3, 0, 5)
    pr, ps, nr, prec, ppri, ppair, ms = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_float()
    cnt = np.zeros(6, dtype=np.int32); npri = np.zeros(6, dtype=np.int32)
    sim.upload(*testdata.flat(reads))
    call = lambda *a: L.bwagpu_batch_rescue(*a)
    ok = lambda: [h, C.byref(opt), P, 0, cnt.ctypes.data, C.byref(pr), C.byref(ps), C.byref(nr), C.byref(prec), None, None, None, None]
    assert call(*ok()) == -2, "before a run"
    sim.run(opt)
    assert call(*ok()) == -2, "before a download"
    counts, regs = sim.download()
    for k in (0, 1, 2, 4, 5, 6, 7, 8):      # NULL h, opt, pes, counts, regs, src, n_regs, rescue
        a = ok(); a[k] = None
        assert call(*a) == -2, k
    a = ok(); a[3] = 7
    assert call(*a) == -2, "odd id0"
    o5 = tp.ref_opt(); o5.flag |= 0x800
    a = ok(); a[1] = C.byref(o5); a[11] = C.byref(ppair)
    assert call(*a) == -2, "MEM_F_PRIMARY5 with pairs"
    a = ok(); a[1] = C.byref(o5)
    assert call(*a) == 0, "MEM_F_PRIMARY5 without pairs"
    for p_ in (pr, ps, prec):
        L.bwagpu_free(p_)
    assert call(*ok()) == 0 and nr.value >= int(counts.sum())      # pri, n_pri, pairs and kernel_ms may be NULL
    for p_ in (pr, ps, prec):
        L.bwagpu_free(p_)
    # MEM_F_NO_RESCUE: the lists come back unchanged
    on = tp.ref_opt(); on.flag |= 0x8
    got = sim.rescue(on, pes, 0)
    assert np.array_equal(got["counts"], counts) and got["regs"].tobytes() == regs.tobytes() and (got["rescue"]["n_aligned"] == 0).all() and (got["rescue"]["flags"] == 0).all()
    pri2, npri2, _ = sim.primary(on, 0)
    assert np.array_equal(got["pri"], pri2) and np.array_equal(got["n_pri"], npri2)
    # an odd number of reads
    sim.upload(*testdata.flat(reads[:3])); sim.run(opt); sim.download()
    assert call(*ok()) == -2, "odd number of reads"
    # zero pairs
    sim.upload(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64)); sim.run(opt); sim.download()
    got = sim.rescue(opt, pes, 0)
    assert got["counts"].shape[0] == 0 and got["regs"].shape[0] == 0 and got["pairs"].shape[0] == 0 and got["rescue"].shape[0] == 0
    # bwagpu_rescue_flat
    rng = np.random.default_rng(3)
    rd, ls = make_case(rng, g, sim.index_meta(), opt, pes, "rescued", 2)
    seqs, off = testdata.ragged(rd)
    c2 = np.array([a.shape[0] for a in ls], dtype=np.int32); r2 = np.concatenate(ls); ids = np.array([4, 5], dtype=np.int64)
    flat = lambda *a: L.bwagpu_rescue_flat(*a)
    okf = lambda: [h, C.byref(opt), P, 1, seqs.ctypes.data, off.ctypes.data, c2.ctypes.data, r2.ctypes.data, None, cnt.ctypes.data, C.byref(pr), C.byref(ps), C.byref(nr), C.byref(prec),
                   None, None, None, None]
    for k in (0, 1, 2, 4, 5, 6, 7, 9, 10, 11, 12, 13):
        a = okf(); a[k] = None
        assert flat(*a) == -2, k
    a = okf(); a[3] = -1
    assert flat(*a) == -2
    a = okf(); a[14] = C.byref(ppri); a[15] = npri.ctypes.data
    assert flat(*a) == -2, "records wanted without ids"
    r3 = r2.copy(); r3["rid"][0] = int(sim.index_meta()["n_seqs"])
    a = okf(); a[7] = r3.ctypes.data
    assert flat(*a) == -2, "rid outside the index"
    assert flat(*okf()) == 0 and nr.value == int(cnt[:2].sum())
    for p_ in (pr, ps, prec):
        L.bwagpu_free(p_)
    got = sim.rescue_flat(opt, pes, np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=ALNREG_DTYPE), np.zeros(0, dtype=np.int64))
    assert got["rescue"].shape[0] == 0 and got["pairs"].shape[0] == 0


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    d = BwaGpu(testdata.small_index()[0])
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [61, 62, 63])
def test_gpu_rescue_flat_fuzz(gpu, ref_small, seed):
    run_fuzz(gpu, ref_small, testdata.small_index()[1], seed, thin=False)


@pytest.mark.gpu
def test_gpu_rescue_short_window(gpu, ref_small):
    run_short_window(gpu, ref_small, testdata.small_index()[1])


@pytest.mark.gpu
def test_gpu_rescue_limits(gpu, ref_small):
    run_limits(gpu, ref_small, testdata.small_index()[1])


@pytest.mark.gpu
def test_gpu_rescue_on_batches():
    fa, g = testdata.medium_index()
    dev, ref = BwaGpu(fa), RefRescue(fa)
    try:
        got = run_batches(dev, ref, g, 6000, 1000, 801, (0, (1 << 35) + 7770))
        r = got["rescue"]
        print(f"rescue: {int((r['n_aligned'] > 0).sum())} of {r.shape[0]} pairs with alignments, {int(r['n_aligned'].sum())} alignments, {int(r['n_inline'].sum())} in place, {got['ms']:.3f} ms")
    finally:
        dev.close(); ref.close()


@pytest.mark.gpu
def test_gpu_cli_rescue(tmp_path):
    import os
    from bwa_amd import build as b
    _, cli = b.build_host(verbose=False)
    fa, g = testdata.medium_index()
    alt = tp.alt_prefix(tmp_path, fa, ["chr3"])
    f1, f2 = tpair.cli_inputs(tmp_path, g, 3200, 800, 811)
    run_cli(cli, alt, f1, f2, 300000, dict(os.environ), 4000)      # (a thousand pairs per batch)
