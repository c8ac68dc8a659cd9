"""The de-duplication stage of the device library (dedup_plan / dedup_launch in bwa_amd/csrc/bwagpu.hip; k_dedup and dedup_read in dev_dedup.h, k_dedup_wave and
dedup_read_wave in dev_dedupw.h, dedup_read_par in dev_dedupp.h) on crafted raw region lists, through bwagpu_dedup_flat, against the compiled reference.

Truth per read: the reference's exported mem_sort_dedup_patch (bwamem.c:463-515), called through ctypes on oracle/_ref/libbwaref.so: the count it returns and the
first `count` 88-byte records, compared byte for byte.  Every input record carries a unique tag in fields the stage only moves (seedlen0, hash), so a wrong
survivor among regions with equal keys shows.  is_alt (bwamem.c:1111-1115) lies outside the reference function; the 200 kb index has no alt contig.

Inputs without a defined truth are not generated, and make_case asserts so: mem_patch_reg reads an uninitialised score when bwa_gen_cigar2 returns early, which
takes a segment that bridges l_pac -- every region here lies within one strand --, and a list whose regions are all dead on arrival (qe == qb) makes the
reference return 1 for a list it has emptied (bwamem.c:509).

Regions are cut from the committed 200 kb genome, on both strands.  Seven families (fam_* below); cover() asserts from the inputs and the reference's results alone
that each produced members on both sides of what it aims at, for every option set.  Every list runs through six configurations of the handle (FORMS), and the
routine that finished each read (form) must be the one predicted from the rules of k_dedup / k_dedup_wave (predict_forms cites the lines).
CPU: on the mock runtime (tests/hostsim), thinned.  -m gpu: everything, three seeds.

What no list can reach: r == (double)0.05f exactly in mem_patch_reg (a quotient of coordinates below 2^19 is never 13421773 / 2^28), and a patch alignment
longer than the query room of the four-columns-per-lane routine: dedup_launch makes q_cap the longest read, rounded up, or 0, and wave_global_score takes that
routine only when q_cap >= l_query.  The case with q_cap == 0 (dedup_blk = 1 served by k_dedup_wave<false>) is run_no_query_room's."""
import ctypes as C

import numpy as np
import pytest

import refapi
import testdata
from bwa_amd.api import BwaGpu
from bwa_amd.structs import ALNREG_DTYPE, default_opt, pacbio_opt

# the switch points the cases are aimed at (bwagpu_dedup_limits)
LIMITS = dict(heavy=3, stage=128, net=129, keysort_min=24, scan_block=64, draw=64, ring_min=256, lds_per_reg=56)
LONG_LEN = 1100          # WAVE_EXT_MAX_LEN (bwagpu.hip): a call with a longer read is a long-read batch
MAXLEN = 400             # the longest read of the short lists (one read of family 7 has it)
GPU_SEEDS = (81, 82, 83)
SIM_SEED = 81
FORMS = (("a", dict(dedup_heavy=0)), ("b1", dict(dedup_wave=1, dedup_blk=1)), ("b0", dict(dedup_wave=1, dedup_blk=0)), ("c", dict()),
         ("d", dict(dedup_heavy=2, dedup_stage=16, dedup_big=32, dedup_net=12)), ("e", dict(dedup_heavy=2, dedup_stage=512, dedup_big=0, dedup_net=4)))


def check_limits(dev):
    assert dev.dedup_limits() == LIMITS, "a switch point moved: aim the cases at it"


def opt_sets():
    """the default, -x pacbio, the asymmetric-gap set of tests/test_dp_fuzz.py::_opts, and a tight set whose band, window and redundancy thresholds 150-base reads reach"""
    a = default_opt()
    a.o_del, a.e_del, a.o_ins, a.e_ins, a.zdrop = 8, 2, 5, 1, 40
    t = default_opt()
    t.w, t.max_chain_gap, t.mask_level_redun = 5, 50, 0.5
    return [("default", default_opt()), ("pacbio", pacbio_opt()), ("asym", a), ("tight", t)]


def room_of(opt, max_len):
    """regions the LDS of the big launch holds next to the ring (dedup_plan, bwagpu.hip) -> (room, ring columns, q_cap)"""
    need = max(8 * opt.w + 4 + 128, max_len // 4 + 132)
    rc = LIMITS["ring_min"]
    while rc < need and rc < 4096:
        rc <<= 1
    q_cap = (max_len + 15) & ~15
    if 8 * rc + 32 + q_cap > 65536:
        q_cap = 0
    return max((65536 - (8 * rc + 32 + q_cap)) // LIMITS["lds_per_reg"], 0), rc, q_cap


def predict_forms(options, opt, max_len, n_raw):
    """the routine that finishes each read: dedup_launch's branch (long-read batch or dedup_wave: k_dedup_wave on every read), k_dedup's hand-over (dev_dedup.h:
    n_raw > dd_stage_cap and >= dd_heavy_min to the big list, >= dd_heavy_min to the other, else dedup_read) and k_dedup_wave<.., LIST>'s choice (dev_dedupw.h:
    dedup_read_par when the read's regions fit par_cap, else dedup_read_wave)"""
    o = lambda k, auto: auto if options.get(k, -1) < 0 else options[k]
    if max_len > LONG_LEN or options.get("dedup_wave", 0):
        return np.ones(len(n_raw), dtype=np.int32)
    heavy = o("dedup_heavy", LIMITS["heavy"])
    if heavy <= 0:
        return np.zeros(len(n_raw), dtype=np.int32)
    room = room_of(opt, max_len)[0]
    cap_m, cap_b = min(o("dedup_stage", LIMITS["stage"]), room), min(o("dedup_big", room), room)
    stage_cap = cap_m if cap_m > 0 else 0x3fffffff
    out = []
    for n in n_raw:
        if n > stage_cap and n >= heavy:
            out.append(2 if n <= cap_b else 1)
        elif n >= heavy:
            out.append(2 if n <= cap_m else 1)
        else:
            out.append(0)
    return np.array(out, dtype=np.int32)


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------------------
class Ref:
    def __init__(self, idx):
        L = refapi.lib()
        L.mem_sort_dedup_patch.restype = C.c_int
        L.mem_sort_dedup_patch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.bwa_gen_cigar2.restype = C.c_void_p
        L.bwa_gen_cigar2.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        self.L, self.bns, self.pac, self.l_pac = L, L.refshim_idx_bns(idx.h), L.refshim_idx_pac(idx.h), idx.l_pac

    def dedup(self, opt, read, regs):
        """mem_sort_dedup_patch on a copy of the list -> the records it leaves"""
        a = np.ascontiguousarray(regs).copy()
        q = np.ascontiguousarray(read, dtype=np.uint8).copy()
        buf = q if q.shape[0] else np.zeros(1, dtype=np.uint8)
        m = self.L.mem_sort_dedup_patch(C.byref(opt), self.bns, self.pac, buf.ctypes.data, int(a.shape[0]), a.ctypes.data if a.shape[0] else None)
        assert 0 <= m <= a.shape[0]
        assert a.shape[0] < 2 or m == 0 or a["qe"][0] > a["qb"][0], "a list the reference empties has no defined truth"
        return a[:m].copy()

    def piece_score(self, read, qb, qe, rb, re):
        """the score of a piece's own global alignment with default options (what an extension would have left in `score`)"""
        opt = default_opt()
        q = np.ascontiguousarray(read[qb:qe], dtype=np.uint8).copy()
        sc, n, nm = C.c_int(0), C.c_int(0), C.c_int(0)
        p = self.L.bwa_gen_cigar2(C.addressof(opt) + type(opt).mat.offset, opt.o_del, opt.e_del, opt.o_ins, opt.e_ins, 400, self.l_pac, self.pac, int(q.shape[0]), q.ctypes.data,
                                  int(rb), int(re), C.byref(sc), C.byref(n), C.byref(nm))
        assert p
        self.L.refshim_free(p)
        return sc.value


class World:
    def __init__(self, lib_path=None, options=None):
        self.prefix, self.g = testdata.small_index()
        lens = testdata.small_genome()[1]
        self.ctg = [(sum(lens[:i]), lens[i]) for i in range(len(lens))]
        self.dev = BwaGpu(self.prefix, lib_path=lib_path, options=options)
        self.idx = refapi.RefIndex(self.prefix)
        self.R = Ref(self.idx)
        self.l_pac = self.idx.l_pac
        assert self.l_pac == self.g.shape[0] == sum(lens) and len(lens) == 3

    def close(self):
        self.dev.close(); self.idx.close()


# ---- crafted lists ------------------------------------------------------------------------------------------------------------------------------------------
class Case:
    __slots__ = ("fam", "tag", "read", "regs", "p", "aim", "info")      # p: the input index of the region the case is about (-1: none); aim: what cover() files it under; info: what it needs to know besides


def revcomp(s):
    s = np.asarray(s, dtype=np.uint8)
    return np.where(s < 4, 3 - s, 4)[::-1].astype(np.uint8)


def reg(rb, re, qb, qe, score, rid=0, w=0):
    r = np.zeros(1, dtype=ALNREG_DTYPE)
    r["rb"], r["re"], r["qb"], r["qe"], r["score"], r["truesc"], r["rid"], r["w"] = rb, re, qb, qe, score, score, rid, w
    return r


def make_case(W, rng, fam, tag, read, regs, p=-1, aim="", info=None):
    c = Case()
    c.fam, c.tag, c.read, c.p, c.aim, c.info = fam, tag, np.ascontiguousarray(read, dtype=np.uint8), p, aim, info
    c.regs = np.concatenate(regs) if len(regs) else np.zeros(0, dtype=ALNREG_DTYPE)
    r, n, L = c.regs, len(regs), W.l_pac
    # what the stage carries along or takes maxima of
    r["sub"], r["csub"], r["seedcov"] = rng.integers(0, 40, n), rng.integers(0, 40, n), rng.integers(10, 120, n)
    r["sub_n"], r["alt_sc"], r["secondary"], r["secondary_all"] = rng.integers(0, 5, n), rng.integers(0, 30, n), -1, rng.integers(0, 3, n)
    r["frac_rep"], r["hash"] = rng.random(n).astype(np.float32), rng.integers(0, 1 << 62, n).astype(np.uint64)
    # a defined truth (see the module's text), and what bwagpu_dedup_flat accepts
    assert ((r["rb"] >= 0) & (r["rb"] < r["re"]) & (r["re"] <= 2 * L) & ((r["rb"] >= L) | (r["re"] <= L))).all(), (fam, tag)
    assert ((r["qb"] >= 0) & (r["qb"] <= r["qe"]) & (r["qe"] <= c.read.shape[0])).all(), (fam, tag)
    assert n < 2 or (r["qe"] > r["qb"]).any(), (fam, tag)
    assert ((r["rid"] >= -1) & (r["rid"] < 3)).all() and (c.read.shape[0] <= MAXLEN or fam == 6), (fam, tag)
    return c


def place(W, rng, span, rev, left=0, ctg=0):
    """B in the doubled coordinates of the strand asked for, with [B - left, B + span) inside contig ctg -> (B, rid)"""
    o, n = W.ctg[ctg]
    if rev:
        o = 2 * W.l_pac - o - n
    return int(rng.integers(o + left + 20, o + n - span - 20)), ctg


def rand_read(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def fam_redundancy(W, rng, thin):
    """1: pairs at the boundary of bwamem.c:481: the overlap on the reference at mask_level_redun * mr, one below and one above it while the query overlap is far
    above its own; the same for the query; p's score below, at and above q's; some with a third region that arrives dead (qe == qb), which the scan skips as q"""
    out = []
    k = 0
    for mlr, lens in ((0.95, (20, 40, 100, 200)), (0.5, (20, 22, 40, 100, 200))):
        for mr in (lens if not thin else lens[:1] + lens[-2:-1]):
            b = int(round(mlr * mr))
            assert float(np.float32(mlr) * np.float32(mr)) == b      # the product is the integer itself: `>` is false at b, true at b + 1
            for dim in ("ref", "qry"):
                for d in (-1, 0, 1):
                    for ds in (-1, 0, 1):
                        k += 1
                        rev = k % 2 == 1
                        B, rid = place(W, rng, 450, rev)
                        lo, sh = (b + d, 99) if dim == "ref" else (99, b + d)      # overlaps on the reference and on the query
                        lr, lq = (mr, 100) if dim == "ref" else (100, mr)           # q's lengths; p is 7 longer
                        q = reg(B, B + lr, 5, 5 + lq, 60, rid)
                        p = reg(B + lr - lo, B + lr - lo + lr + 7, 5 + lq - sh, 5 + lq - sh + lq + 7, 60 + ds, rid)
                        regs = [q, p]
                        if k % 3 == 0:      # dead on arrival; with a score that would beat both
                            regs.insert(k % 2, reg(B + 3, B + lr + 2, 9, 9, 200, rid))
                        out.append(make_case(W, rng, 1, f"mlr{mlr} mr{mr} {dim} {d:+d} score {ds:+d}", rand_read(rng, int(p["qe"][0]) + 5), regs, aim=f"{mlr}"))
    return out


def fillers(B, rid, idx, K, score=40):
    """the region at sorted place idx of a window of K: 20 reference bases ending at B + 30 + 2 idx, one query base at K - 1 - idx -- the later the end, the earlier the
    query: no two of them are redundant (no common query base) or collinear"""
    re = B + 30 + 2 * idx
    return reg(re - 20, re, K - 1 - idx, K - idx, score, rid)


def fam_sequence(W, rng, thin):
    """2: what happens at j depends on the earlier j: two regions redundant with p in either order; a q killed by one p and met by the next; a p that kills a run and then
    loses; windows of up to 190 live regions with the event -- p loses, or the first region that passes mem_patch_reg's tests ahead of its alignment, followed by a
    region p loses to -- 1, 63, 64, 65, 127, 128, 129 places from p, dead regions on both sides of the 64-region blocks of dedup_read_par's scan"""
    out = []
    for v in range(4 if thin else 12):
        rev = v % 2 == 1
        B, rid = place(W, rng, 700, rev)
        tie = v % 3 == 2      # p's score equal to the stronger one's: then q dies
        strong, weak, ps = 90, 50, (90 if tie else 70)
        S, Wk, P = reg(B, B + 100, 0, 100, strong, rid), reg(B + 100, B + 200, 100, 200, weak, rid), reg(B, B + 205, 0, 205, ps, rid)
        out.append(make_case(W, rng, 2, f"weak then strong {v}", rand_read(rng, 210), [S, Wk, P], p=2, aim="order"))
        S, Wk = reg(B + 100, B + 200, 100, 200, strong, rid), reg(B, B + 100, 0, 100, weak, rid)
        out.append(make_case(W, rng, 2, f"strong then weak {v}", rand_read(rng, 210), [Wk, S, P], p=2, aim="order"))
        for sc in ((50, 60, 70), (50, 60, 55), (50, 50, 50), (60, 50, 55)):
            regs = [reg(B, B + 100 + 2 * i, 0, 100 + 2 * i, s, rid) for i, s in enumerate(sc)]
            out.append(make_case(W, rng, 2, f"met again {sc} {v}", rand_read(rng, 150), regs, p=2, aim="order"))
        for at in (0, 4, 8, -1):      # nine tiles of p, one of them (at) stronger than p
            tiles = [reg(B + 30 * i, B + 30 * i + 30, 30 * i, 30 * i + 30, 95 if i == at else 30 + i, rid) for i in range(9)]
            out.append(make_case(W, rng, 2, f"run then loses at {at} {v}", rand_read(rng, 300), tiles + [reg(B, B + 300, 0, 300, 70, rid)], p=9, aim="order"))
    for d in (1, 63, 64, 65, 127, 128, 129):
        for kind in ("lose", "cand", "none"):
            for inner in (False, True):
                if thin and (kind == "none" or inner != (d % 2 == 0)):
                    continue
                rev = (d + inner) % 2 == 1
                K = d + 12 + int(rng.integers(0, 17))         # regions in front of p
                assert K <= 158
                B, rid = place(W, rng, 2 * K + 120, rev, left=1800)
                P = 2 * K + 60
                regs = []
                for idx in range(K):
                    dist = K - idx                            # places from p
                    if dist == d and kind == "lose":          # redundant with p and stronger
                        r = reg(B + 10 + 2 * idx, B + 30 + 2 * idx, 200, 300, 90, rid)
                    elif dist == d and kind == "cand":        # left of p, collinear, |r| < 0.05: an alignment follows -- and fails on a random read
                        o = 30 + 2 * idx
                        if o / (P + 40) <= 0.2:
                            g, qe = 40, 200 + max(1, round(140 * o / (P + 40)))
                        else:
                            g, qe = 5 * o - P, 228
                        r = reg(B - g, B + o, 160, qe, 35, rid)
                    elif dist == d + 1 and kind == "cand":    # ... and behind it the region p loses to
                        r = reg(B + 10 + 2 * idx, B + 30 + 2 * idx, 200, 300, 90, rid)
                    elif dist in (64, 65, 128, 129) and dist != d:      # dead on arrival, either side of a block boundary
                        r = fillers(B, rid, idx, K)
                        r["qe"] = r["qb"]
                    elif inner and dist % 3 == 0:             # inside p's query: redundant with p, weaker: p kills it on its way
                        r = reg(B + 10 + 2 * idx, B + 30 + 2 * idx, 250, 251, 20, rid)
                    else:
                        r = fillers(B, rid, idx, K)
                    regs.append(r)
                regs.append(reg(B, B + P, 200, 300, 70, rid))
                order = rng.permutation(len(regs))           # (the input order is not the sorted one)
                out.append(make_case(W, rng, 2, f"block d{d} {kind} inner{int(inner)}", rand_read(rng, 300), [regs[i] for i in order], p=int(np.nonzero(order == K)[0][0]), aim=f"block {kind}"))
    return out


def fam_equal_keys(W, rng, thin):
    """3: regions that share `re` (the by-end order is the introsort's own), all redundant with each other, the best score held by several: who survives is a matter
    of that order; a second group with another part of the query; groups equal in (score, rb, qb) at the second sort that differ in qe, re and tag, kept apart in
    the scan by alternating rid; two regions that are equal only once a join has moved one's start"""
    out = []
    sizes = (2, 3, 5, 11, 12, 16, 17, 23, 24, 40, 128, 129, 200)
    for n in sizes:
        for groups in (1, 2):
            for rev in (False, True):
                if n < 4 and groups == 2:
                    continue
                B, rid = place(W, rng, 500, rev)
                regs = []
                for k in range(n):
                    g_ = k % groups
                    regs.append(reg(B + 300 - 100 - k % 7, B + 300, 5 + 150 * g_, 105 + 150 * g_ + k % 5, 60 - (k * 7) % 3 if n > 3 else 60, rid))
                out.append(make_case(W, rng, 3, f"same end n{n} groups{groups}", rand_read(rng, 300), regs, aim="end"))
    for run in ((2,), (3,), (20,), (2, 3, 20), (20, 20), (3, 1, 2, 1, 1, 3)):
        for rev in (False, True):
            for rep in range(4):
                B, rid = place(W, rng, 700, rev)
                regs, k = [], 0
                for gi, m in enumerate(run):
                    for _ in range(m):      # the same score, rb, qb; ends that ascend through all groups; neighbours on different contigs
                        regs.append(reg(B + 10 * gi, B + 80 + 3 * k, 7 + gi, 60 + 2 * k, 50 + gi % 2, (0, 1, 2, -1)[k % 4]))
                        k += 1
                order = rng.permutation(len(regs))
                out.append(make_case(W, rng, 3, f"second sort {run} {rep}", rand_read(rng, 250), [regs[i] for i in order], aim="best"))
    for rev in (False, True):      # A + B join without an alignment into (200, A.rb, A.qb); X has those already, on another contig behind them
        for extra in range(1 if thin else 5):
            tb = place(W, rng, 260, False)[0]
            read = W.g[tb:tb + 200 + extra].copy()
            c = flip(W, make_case(W, rng, 3, f"equal after a join {extra}", read, [reg(tb, tb + 100, 0, 100, 100, 0), reg(tb + 100, tb + 200, 100, 200, 100, 0)], aim="join"), rev)
            x = reg(int(c.regs["rb"].min()), int(c.regs["re"].max()) + extra, int(c.regs["qb"].min()), int(c.regs["qe"].max()), 200, 1)
            out.append(make_case(W, rng, 3, c.tag, c.read, [c.regs[:1], c.regs[1:], x], aim="join"))
    return out


def flip(W, c, rev):
    """the case on the reverse strand: the read reverse-complemented, every region mirrored"""
    if not rev:
        return c
    N, L = c.read.shape[0], W.l_pac
    c.read = revcomp(c.read)
    rb, re, qb, qe = (c.regs[f].copy() for f in ("rb", "re", "qb", "qe"))
    c.regs["rb"], c.regs["re"], c.regs["qb"], c.regs["qe"] = 2 * L - re, 2 * L - rb, N - qe, N - qb
    c.tag += " rev"
    return c


def fam_window(W, rng, thin):
    """4: the window's end: two exact pieces of one read g and g - 1 bases apart for g = max_chain_gap of the tight set (inside, they join without an alignment);
    a region on another contig (rid 0, 1, 2, -1 are only compared) in front of one p would lose to -- the scan stops there, also when a[i-1] alone is the
    other one; a join that moves p.rb to the left and brings a third piece into the window"""
    out = []
    for g_ in (48, 49, 50, 51):
        for rev in (False, True):
            for rep in range(1 if thin else 3):
                tb = place(W, rng, 300, False)[0]
                la = int(rng.integers(80, 110))
                read = W.g[tb:tb + 260].copy()
                regs = [reg(tb, tb + la, 0, la, la), reg(tb + la + g_, tb + 260, la + g_, 260, 260 - la - g_)]
                out.append(flip(W, make_case(W, rng, 4, f"gap {g_}", read, regs, aim="gap"), rev))
    for rids in ((0, 1, 0), (0, 2, 0), (0, -1, 0), (1, 0, 1), (-1, 2, -1), (2, 2, 2), (0, 0, 0), (-1, -1, -1)):
        for rev in (False, True):
            for n_between in (1, 2):
                B, _ = place(W, rng, 300, rev)
                X = reg(B, B + 100, 0, 100, 90, rids[0])
                Y = [reg(B + 2 + i, B + 101 + i, 200, 240, 40, rids[1]) for i in range(n_between)]
                P = reg(B + 1, B + 104, 0, 100, 70, rids[2])
                out.append(make_case(W, rng, 4, f"rid {rids} x{n_between}", rand_read(rng, 250), [X] + Y + [P], p=1 + n_between, aim="rid", info=rids))
    for rev in (False, True):
        for rep in range(2 if thin else 6):
            tb = place(W, rng, 300, False)[0]
            read = W.g[tb:tb + 230].copy()
            regs = [reg(tb, tb + 60, 0, 60, 60), reg(tb + 90, tb + 150, 90, 150, 60), reg(tb + 160, tb + 230, 160, 230, 70)]
            out.append(flip(W, make_case(W, rng, 4, f"moved window {rep}", read, regs, aim="moved"), rev))
    return out


def pieces_of(W, rng, tb, ops):
    """a read made from g[tb:] by ("M", n) n bases as they are, ("D", n) n target bases skipped, ("I", n) n random bases added, ("X", n) n bases that all differ
    -> (read, [(t0, t1, q0, q1)] of the M runs)"""
    t, q, pieces = tb, [], []
    for op, n in ops:
        if op == "M":
            pieces.append((t, t + n, len(q), len(q) + n))
            q += W.g[t:t + n].tolist(); t += n
        elif op == "D":
            t += n
        elif op == "I":
            q += rng.integers(0, 4, n).tolist()
        else:
            q += ((W.g[t:t + n] + rng.integers(1, 4, n)) & 3).tolist(); t += n
    return np.array(q, dtype=np.uint8), pieces


def join_case(W, rng, tag, ops, rev, w=(0, 0), aim="join", extra=None, fam=5, ctg=0, scores=None):
    """the pieces of a read as its raw regions, each with its own score (an exact piece: its length); extra(read, regs, tb): further regions"""
    span = sum(n for op, n in ops if op != "I")
    tb = place(W, rng, span + 40, False, ctg=ctg)[0]
    read, pcs = pieces_of(W, rng, tb, ops)
    regs = [reg(t0, t1, q0, q1, (q1 - q0) if scores is None else scores[k], ctg, w[k % len(w)]) for k, (t0, t1, q0, q1) in enumerate(pcs)]
    c = flip(W, make_case(W, rng, fam, tag, read, regs, aim=aim), rev)
    by_end = np.argsort(c.regs["re"], kind="stable")
    c.p = int(by_end[-1])
    if extra is not None:      # (on the strand the case ends up on: a, p are the pieces by end)
        regs = extra([c.regs[k:k + 1] for k in by_end])
        c = make_case(W, rng, fam, c.tag, c.read, regs, p=len(regs) - 1, aim=aim)
    return c


def fam_patch(W, rng, thin):
    """5: mem_patch_reg on collinear pieces of one read: a deletion or insertion of 1 .. 21 bases between exact pieces of three sizes (w at opt.w << 1 and one above
    for the tight set; the 0.90 score ratio on both sides for every set); a cluster of mismatches (the block without DP when both pieces have w == 0); pieces that
    overlap on both sides with up to 30 bases missing from the target (w at opt.w << 2 and above for the tight set, r on both sides of 0.10 for the others); the
    three non-collinear shapes; a on the forward and b on the reverse strand; w + a.w + b.w beyond opt.w << 2; cascades of three and four pieces; a refused join in
    front of an accepted one; a join after which the longer p is redundant with a region it was not; a join 70 places from p"""
    out = []
    sizes = ((70, 80), (150, 150), (100, 190)) if not thin else ((70, 80), (150, 150))
    for la, lb in sizes:
        for d in ((1, 2, 3, 5, 7, 8, 10, 11, 12, 20, 21) if not thin else (1, 2, 3, 7, 10, 11, 21)):
            for kind in ("D", "I"):
                for rev in (False, True):
                    if thin and rev != (kind == "D"):
                        continue
                    out.append(join_case(W, rng, f"{kind}{d} {la}+{lb}", (("M", la), (kind, d), ("M", lb)), rev, aim="gap"))
    for n_x in (1, 2, 3, 6, 12, 20, 30, 40):
        for w in ((0, 0), (3, 4)):
            for rev in (False, True):
                out.append(join_case(W, rng, f"X{n_x} w{w}", (("M", 80), ("X", n_x), ("M", 90)), rev, w=w, aim="mismatches"))
    for d in ((0, 5, 10, 19, 20, 21, 22, 23, 24, 25, 30) if not thin else (0, 20, 21, 24, 25, 30)):
        for rev in (False, True):
            for w in ((0, 0), (2, 1)):
                # A = g[tb, tb + 150) as it is; B claims the query from 110 on against the target d bases further right: they overlap by 40 query bases and 40 - d target bases
                tb = place(W, rng, 330, False)[0]
                read = np.concatenate([W.g[tb:tb + 150], W.g[tb + 150 + d:tb + 250 + d]])
                sb = W.R.piece_score(read, 110, 250, tb + 110 + d, tb + 250 + d)
                regs = [reg(tb, tb + 150, 0, 150, 150, 0, w[0]), reg(tb + 110 + d, tb + 250 + d, 110, 250, max(sb, 1), 0, w[1])]
                out.append(flip(W, make_case(W, rng, 5, f"overlap D{d} w{w}", read, regs, p=1, aim="overlap"), rev))
    for rev in (False, True):
        for rep in range(1 if thin else 3):
            tb = place(W, rng, 300, False)[0]
            g = W.g
            read = np.concatenate([g[tb + 90:tb + 170], rand_read(rng, 20), g[tb:tb + 80]])
            out.append(flip(W, make_case(W, rng, 5, "a.qb >= b.qb", read, [reg(tb, tb + 80, 100, 180, 80), reg(tb + 90, tb + 170, 0, 80, 80)], p=1, aim="shape"), rev))
            read = g[tb:tb + 130].copy()
            out.append(flip(W, make_case(W, rng, 5, "a.qe >= b.qe", read, [reg(tb, tb + 100, 0, 100, 100), reg(tb + 50, tb + 120, 20, 90, 70)], p=1, aim="shape"), rev))
            out.append(flip(W, make_case(W, rng, 5, "a.re >= b.re", read, [reg(tb, tb + 100, 0, 50, 50), reg(tb + 40, tb + 100, 60, 100, 40)], p=1, aim="shape"), rev))
    L = W.l_pac
    for rep in range(2 if thin else 6):      # the last bases of the forward strand and the first of the reverse strand: one contig, two strands
        a0, b1 = int(rng.integers(60, 120)), int(rng.integers(60, 120))
        read = np.concatenate([W.g[L - a0 - 10:L - 10], rand_read(rng, 10), revcomp(W.g[L - b1 - 5:L - 5])])
        regs = [reg(L - a0 - 10, L - 10, 0, a0, a0, 2), reg(L + 5, L + 5 + b1, a0 + 10, a0 + 10 + b1, b1, 2)]
        out.append(make_case(W, rng, 5, f"two strands {rep}", read, regs, p=1, aim="shape"))
    for d in (2, 3):
        for rev in (False, True):
            out.append(join_case(W, rng, f"clipped w D{d}", (("M", 150), ("D", d), ("M", 150)), rev, w=(250, 250), aim="clip"))
            out.append(join_case(W, rng, f"clipped w I{d}", (("M", 150), ("I", d), ("M", 150)), rev, w=(250, 250), aim="clip"))
    for n_p in (3, 4):
        for kind in ("D", "I", "X"):
            for rev in (False, True):
                ops = [("M", 80)]
                for _ in range(n_p - 1):
                    ops += [(kind, 2), ("M", 78 if kind != "D" else 80)]
                out.append(join_case(W, rng, f"cascade {n_p} {kind}", ops, rev, aim=f"cascade{n_p}"))

    def refused_first(regs):      # X between A and p in the by-end order: collinear with p, far too wide a band; p then joins A
        a, p = regs
        x = reg(int(p["rb"][0]) - 5, int(p["re"][0]) - 2, int(a["qb"][0]), int(a["qb"][0]) + 20, 25)
        return [a, x, p]

    def then_redundant(strong):
        def f(regs):      # Z inside A on the reference, inside p on the query: redundant with p only once p begins where A does
            a, p = regs
            z = reg(int(a["rb"][0]) + 50, int(a["rb"][0]) + 100, int(p["qb"][0]) + 50, int(p["qb"][0]) + 100, 400 if strong else 45)
            return [z, a, p]
        return f

    def seventy_between(regs):      # 70 regions inside p on the reference and inside A on the query, between the two in the by-end order
        a, p = regs
        mid = [reg(int(p["rb"][0]) + 5 + i, int(p["rb"][0]) + 25 + i, int(a["qb"][0]) + 100 - i, int(a["qb"][0]) + 101 - i, 30) for i in range(70)]
        return [a] + mid + [p]

    for rev in (False, True):
        for kind in ("D", "I"):
            ops = (("M", 150), (kind, 2), ("M", 150))
            out.append(join_case(W, rng, f"refused then accepted {kind}", ops, rev, extra=refused_first, aim="refused first"))
            for strong in (False, True, False, True):
                out.append(join_case(W, rng, f"join then redundant {kind} strong{int(strong)}", ops, rev, extra=then_redundant(strong), aim="then redundant"))
            out.append(join_case(W, rng, f"join in the second block {kind}", ops, rev, extra=seventy_between, aim="second block"))
    return out


def fam_sizes(W, rng, thin):
    """7: reads with 0 .. 200 raw regions, and as many as the big launch's LDS holds (for every option set's ring) and one more: clusters of near-copies with random
    scores, a few regions on other contigs; one read of MAXLEN bases"""
    sizes = [0, 1, 2, 3, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200]
    rooms = sorted({room_of(o, MAXLEN)[0] for _, o in opt_sets()})
    assert rooms == [1016, 1126], rooms
    for r in rooms:
        sizes += [r, r + 1]
    out = []
    for n in sizes:
        for rev in ((False, True) if n < 300 and not thin else (n % 2 == 1,)):
            B, rid = place(W, rng, 900, rev)
            N = MAXLEN if n == 200 else int(rng.integers(150, MAXLEN))
            centres = [(int(rng.integers(0, 500)), int(rng.integers(20, 120)), int(rng.integers(0, N - 120)), int(rng.integers(10, 100))) for _ in range(max(1, n // 4))]
            regs = []
            for k in range(n):
                r0, rl, q0, ql = centres[int(rng.integers(0, len(centres)))]
                j = rng.integers(0, 4, 4)
                regs.append(reg(B + r0 + j[0], B + r0 + j[0] + rl + j[1], q0 + j[2], q0 + j[2] + ql + j[3], int(rng.integers(20, 100)), rid if rng.random() > 0.05 else int(rng.integers(-1, 3))))
            out.append(make_case(W, rng, 7, f"n{n}", rand_read(rng, N), regs, aim="size"))
    return out


FAMILIES = (fam_redundancy, fam_sequence, fam_equal_keys, fam_window, fam_patch, fam_sizes)
_cases, _truth, _long = {}, {}, {}


def tag_all(cases):
    k = 0
    for c in cases:
        c.regs["seedlen0"] = np.arange(k, k + c.regs.shape[0])
        k += c.regs.shape[0]


def cases_of(W, seed, thin):
    """the crafted list of a seed (made once); every record of it has its own seedlen0"""
    key = (seed, thin)
    if key not in _cases:
        out = []
        for k, f in enumerate(FAMILIES):
            out += f(W, np.random.default_rng([seed, k]), thin)
        tag_all(out)
        assert max(c.read.shape[0] for c in out) == MAXLEN
        _cases[key] = out
    return _cases[key]


def fam_long(W, rng, thin):
    """6: reads of 2 to 4.5 kb, for -x pacbio and the wave-per-read kernel: two exact pieces around a deletion or insertion whose band fits a ring of 256 columns
    (2 w + 132 <= 256) or does not (lane 0 then computes it with its columns in HBM), among them w at opt.w << 1 and one above; a cascade of three; pieces
    max_chain_gap and one less apart on a 10 kb read (thin: left out)"""
    out = []
    for d, la, lb in ((20, 1000, 1200), (59, 1500, 1500), (60, 1500, 1500), (61, 1200, 1500), (150, 1800, 1800), (200, 2100, 2100), (201, 2100, 2150), (300, 2000, 2000)):
        for kind in ("D", "I"):
            for rev in (False, True):
                if thin and (rev != (kind == "D") or d in (59, 150, 201)):
                    continue
                out.append(join_case(W, rng, f"long {kind}{d}", (("M", la), (kind, d), ("M", lb)), rev, fam=6, aim="long"))
    for rev in (False, True):
        out.append(join_case(W, rng, "long cascade", (("M", 800), ("D", 30), ("M", 900), ("I", 70), ("M", 1000)), rev, fam=6, aim="long"))
    if not thin:
        for g_ in (9999, 10000):
            for rev in (False, True):
                tb = place(W, rng, 10400, False)[0]
                read = W.g[tb:tb + 100 + g_ + 150].copy()
                regs = [reg(tb, tb + 100, 0, 100, 100), reg(tb + 100 + g_, tb + 250 + g_, 100 + g_, 250 + g_, 150)]
                out.append(flip(W, make_case(W, rng, 6, f"long gap {g_}", read, regs, p=1, aim="long gap"), rev))
    tag_all(out)
    return out


def long_cases_of(W, seed, thin):
    key = (seed, thin)
    if key not in _long:
        _long[key] = fam_long(W, np.random.default_rng([seed, 60]), thin)
    return _long[key]


def truth_of(W, cases, key, opt):
    """the reference's records for every read of the list under one option set (computed once, shared and left alone)"""
    if key not in _truth:
        _truth[key] = [W.R.dedup(opt, c.read, c.regs) for c in cases]
    return _truth[key]


def cover(W, oname, opt, cases, truth, thin):
    """each family on both sides of what it aims at, from the inputs and the reference's results alone: at least 8 members (or all there are) per side"""
    def both(what, flags):
        flags = list(flags)
        yes, no = sum(1 for f in flags if f), sum(1 for f in flags if not f)
        assert len(flags) >= 16 and yes >= 8 and no >= 8, f"{oname}: {what}: {yes} of {len(flags)}, {no} on the other side"

    def sel(fam, aim=None, at_least=1):      # the members filed under an aim: never none, so that no check below is about nothing
        out = [(c, t) for c, t in zip(cases, truth) if c.fam == fam and (aim is None or c.aim.startswith(aim))]
        assert len(out) >= at_least, f"{oname}: family {fam} has {len(out)} members filed under {aim!r}"
        return out
    tags = lambda t: set(t["seedlen0"].tolist())
    alive = lambda c: int((c.regs["qe"] > c.regs["qb"]).sum())
    p_lives = lambda c, t: int(c.regs["seedlen0"][c.p]) in tags(t)
    joined = lambda t: bool(((t["ncomp_isalt"] & 0x3fffffff) > 1).any())
    tight = oname == "tight"
    # 1: a live region removed or not, among the pairs aimed at this set's mask_level_redun
    both("1: one of the pair is redundant", [t.shape[0] < alive(c) for c, t in sel(1, "0.5" if tight else "0.95")])
    assert any((c.regs["qe"] == c.regs["qb"]).any() for c, t in sel(1))
    # 2: p survives or not; every block case's p falls to the region d places away unless there is none
    both("2: p survives", [p_lives(c, t) for c, t in sel(2, "order")])
    for kind in ("lose", "cand"):
        assert not any(p_lives(c, t) for c, t in sel(2, f"block {kind}")), f"{oname}: 2: a p of the block cases ({kind}) survived in the reference"
    assert all(p_lives(c, t) for c, t in sel(2, "block none", at_least=0 if thin else 14))
    assert {c.tag.split()[1] for c, t in sel(2, "block")} == {f"d{d}" for d in (1, 63, 64, 65, 127, 128, 129)}
    assert max(alive(c) for c, t in sel(2, "block")) > 128 and any(t.shape[0] > 128 for c, t in sel(2, "block"))
    # 3: the survivor of a group of equal keys is the one listed last, or another
    def last(c, t):      # of the regions with the best score in the first group (those that equal the list's first in qb): does the one listed last survive?
        grp = c.regs[(c.regs["qb"] == c.regs["qb"][0]) & (c.regs["rb"] == c.regs["rb"][0]) if c.aim == "best" else c.regs["qb"] == c.regs["qb"][0]]
        top = grp[grp["score"] == grp["score"].max()]
        return int(top["seedlen0"][-1]) in tags(t)
    both("3: same end, the survivor", [last(c, t) for c, t in sel(3, "end")])
    both("3: second sort, the survivor", [last(c, t) for c, t in sel(3, "best")])
    # (X ties with p in `re` where it is no longer than the two pieces: the introsort may then put it between them, and the scan stops at it)
    assert all(t.shape[0] == 1 and joined(t) for c, t in sel(3, "join") if int(c.regs["re"][2]) > int(c.regs["re"][:2].max())) and any(joined(t) for c, t in sel(3, "join", 2)), f"{oname}: 3: equal after a join"
    assert {c.regs.shape[0] for c, t in sel(3, "end")} >= {2, 3, 12, 17, 24, 129} and (thin or {c.regs.shape[0] for c, t in sel(3, "end")} >= {11, 16, 23, 128, 200})
    # 4
    gaps = {int(c.tag.split()[1]): set() for c, t in sel(4, "gap")}
    for c, t in sel(4, "gap"):
        gaps[int(c.tag.split()[1])].add(joined(t))
    assert gaps == ({48: {True}, 49: {True}, 50: {False}, 51: {False}} if tight else {g_: {True} for g_ in (48, 49, 50, 51)}), (oname, gaps)
    both("4: the scan reaches the stronger region", [not p_lives(c, t) for c, t in sel(4, "rid")])
    assert all(p_lives(c, t) == (len(set(c.info)) > 1) for c, t in sel(4, "rid")), oname
    assert all(t.shape[0] == 1 and int(t["ncomp_isalt"][0] & 0x3fffffff) == 5 for c, t in sel(4, "moved", 4)), oname
    # 5
    both("5: pieces around a gap join", [joined(t) for c, t in sel(5, "gap")])
    both("5: overlapping pieces join", [joined(t) for c, t in sel(5, "overlap")])
    both("5: pieces around mismatches join", [joined(t) for c, t in sel(5, "mismatches")])
    assert {int(t["w"][0]) > 0 for c, t in sel(5, "mismatches") if joined(t)} == {False, True}, oname      # (w == 0: the block without DP)
    assert not any(joined(t) for c, t in sel(5, "shape", 8))
    assert all(joined(t) and int(t["w"].max()) == opt.w << 2 for c, t in sel(5, "clip", 8)), oname
    for n_p in (3, 4):
        got = {int(t["ncomp_isalt"][0] & 0x3fffffff) for c, t in sel(5, f"cascade{n_p}", 6)}
        assert got == {2 * n_p - 1}, (oname, n_p, got)
        for c, t in sel(5, f"cascade{n_p}"):
            assert t.shape[0] == 1 and all(int(t[f][0]) == int(c.regs[f].max()) for f in ("seedcov", "sub", "csub")), (oname, c.tag)
    assert all(joined(t) and t.shape[0] == 2 for c, t in sel(5, "refused first", 4)), oname
    assert all(t.shape[0] == 1 and joined(t) == p_lives(c, t) for c, t in sel(5, "then redundant")), oname      # (the joined p, or the region that beat it)
    both("5: the joined p wins", [p_lives(c, t) for c, t in sel(5, "then redundant")])
    assert all(joined(t) and t.shape[0] == 71 for c, t in sel(5, "second block", 4)), oname
    if tight:      # w at opt.w << 1 = 10 | 11 in the branch without overlap, at opt.w << 2 = 20 | 21 in the other
        by_d = lambda aim, d, kinds: {joined(t) for c, t in sel(5, aim) if c.tag.split()[0 if aim == "gap" else 1] in [k + str(d) for k in kinds] and (aim != "gap" or "150+150" in c.tag)}
        assert by_d("gap", 10, "DI") == {True} and by_d("gap", 11, "DI") == {False}, oname
        assert by_d("overlap", 20, "D") == {True} and by_d("overlap", 21, "D") == {False}, oname
    # 7
    want = {0, 1, 2, 3, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 1016, 1017, 1126, 1127}
    assert {c.regs.shape[0] for c, t in sel(7)} == want
    assert sum(1 for c, t in sel(7) if 0 < t.shape[0] < c.regs.shape[0]) >= 8 and sum(1 for c, t in sel(7) if t.shape[0] == c.regs.shape[0]) >= 2


def cover_long(W, cases, truth, thin):
    opt = pacbio_opt()
    joined = lambda t: bool(((t["ncomp_isalt"] & 0x3fffffff) > 1).any())
    gap = lambda c: int(c.tag.split()[1][1:]) if c.aim == "long" and not c.tag.startswith("long cascade") else None      # "long D60 rev" -> 60
    j = [(gap(c) + 3, joined(t)) for c, t in zip(cases, truth) if gap(c) is not None]      # (the band: the length difference + 3, bwa.c:187)
    assert any(2 * w + 4 + 128 <= 256 and y for w, y in j) and any(2 * w + 4 + 128 > 256 and y for w, y in j) and any(not y for w, y in j)
    d_of = lambda d: {joined(t) for c, t in zip(cases, truth) if gap(c) == d}
    assert d_of(200) == {True} and (thin or d_of(201) == {False}) and opt.w << 1 == 200
    assert all(joined(t) for c, t in zip(cases, truth) if c.tag.startswith("long cascade"))
    if not thin:
        assert {(c.tag.split()[2], joined(t)) for c, t in zip(cases, truth) if c.aim == "long gap"} == {("9999", True), ("10000", False)}
    assert all(2000 <= c.read.shape[0] <= 4500 or c.aim == "long gap" for c in cases)


# ---- the device side ------------------------------------------------------------------------------------------------------------------------------------------
def run_list(dev, opt, cases, **options):
    """bwagpu_dedup_flat on the reads of the cases under the handle options given (restored afterwards) -> (counts, records per read, form)"""
    seqs, off = testdata.ragged([c.read for c in cases])
    regs = np.concatenate([c.regs for c in cases]) if cases else np.zeros(0, dtype=ALNREG_DTYPE)
    counts = np.array([c.regs.shape[0] for c in cases], dtype=np.int32)
    old = {k: dev.get_option(k) for k in options}
    try:
        for k, v in options.items():
            dev.set_option(k, v)
        left, got, form = dev.dedup_flat(opt, seqs, off, counts, regs)
    finally:
        for k, v in old.items():
            dev.set_option(k, v)
    at = np.concatenate([[0], np.cumsum(left)])
    return left, [got[at[i]:at[i + 1]] for i in range(len(cases))], form


def check_list(what, cases, truth, got, form, want_form):
    bad = []
    for k, (c, t, g_) in enumerate(zip(cases, truth, got)):
        if g_.shape[0] != t.shape[0] or g_.tobytes() != t.tobytes():
            bad.append(f"{c.fam} {c.tag} (read {k}, {c.regs.shape[0]} regions, form {int(form[k])}): device {g_.shape[0]} records, reference {t.shape[0]}"
                       + ("" if g_.shape[0] != t.shape[0] else f"; first difference at record {next(i for i in range(t.shape[0]) if g_[i].tobytes() != t[i].tobytes())}"))
    assert not bad, f"{what}: {len(bad)} reads differ from mem_sort_dedup_patch (families {sorted({int(x.split()[0]) for x in bad})}):\n  " + "\n  ".join(bad[:12])
    assert np.array_equal(form, want_form), f"{what}: form {form[form != want_form][:8]} at reads {np.nonzero(form != want_form)[0][:8]}, predicted {want_form[form != want_form][:8]}"


def run_families(W, seed, thin):
    dev = W.dev
    check_limits(dev)
    cases = cases_of(W, seed, thin)
    n_raw = [c.regs.shape[0] for c in cases]
    for oname, opt in opt_sets():
        truth = truth_of(W, cases, (seed, thin, oname), opt)
        cover(W, oname, opt, cases, truth, thin)
        for fname, options in FORMS:
            if thin and oname not in ("default", "tight") and fname not in ("c", "d"):      # (the mock runtime's budget)
                continue
            left, got, form = run_list(dev, opt, cases, **options)
            want = predict_forms(options, opt, MAXLEN, n_raw)
            check_list(f"seed {seed}, {oname}, form {fname}", cases, truth, got, form, want)
            if fname in ("c", "d", "e"):
                assert (form == 2).sum() > 0 and (form == 1).sum() > 0, (oname, fname)
            if fname == "c":
                assert (form == 0).sum() > 0
    # calls of 1, 63, 64 and 65 reads (k_dedup draws 64 at a time), from the end of the list where the counts differ most; reads in another order
    opt = default_opt()
    truth = truth_of(W, cases, (seed, thin, "default"), opt)
    for n in (1, 63, 64, 65):
        sub = list(range(len(cases) - n - 4, len(cases) - 4))
        sc, st = [cases[k] for k in sub], [truth[k] for k in sub]
        left, got, form = run_list(dev, opt, sc)
        check_list(f"seed {seed}, a call of {n} reads", sc, st, got, form, predict_forms({}, opt, max(c.read.shape[0] for c in sc), [c.regs.shape[0] for c in sc]))
    perm = np.random.default_rng(seed).permutation(len(cases))[:len(cases) // (4 if thin else 1)]
    sc, st = [cases[k] for k in perm], [truth[k] for k in perm]
    left, got, form = run_list(dev, opt, sc, **dict(FORMS)["d"])
    check_list(f"seed {seed}, a permuted list", sc, st, got, form, predict_forms(dict(FORMS)["d"], opt, max(c.read.shape[0] for c in sc), [c.regs.shape[0] for c in sc]))


def run_long(W, seed, thin):
    opt = pacbio_opt()
    cases = long_cases_of(W, seed, thin)
    truth = truth_of(W, cases, (seed, thin, "long"), opt)
    cover_long(W, cases, truth, thin)
    for blk in (1, 0):
        for ring in (0, 256):
            if thin and blk == 0 and ring == 0:
                continue
            left, got, form = run_list(W.dev, opt, cases, dedup_blk=blk, dedup_ring=ring)
            check_list(f"long reads, seed {seed}, dedup_blk {blk}, dedup_ring {ring}", cases, truth, got, form, np.ones(len(cases), dtype=np.int32))
    # short reads of the same shapes beside them: still a long-read batch
    mixed = cases[:4] + [c for c in cases_of(W, seed, thin) if c.fam == 5][:40]
    mt = [W.R.dedup(opt, c.read, c.regs) for c in mixed]
    left, got, form = run_list(W.dev, opt, mixed, dedup_ring=256)
    check_list(f"long and short reads, seed {seed}", mixed, mt, got, form, np.ones(len(mixed), dtype=np.int32))


def run_no_query_room(W, seed):
    """dedup_blk = 1 without room for the query segment: with a ring of 4096 columns a read of more than 32736 bases leaves none (8 ring + 32 + q_cap > 65536, so
    q_cap = 0 and dedup_launch takes k_dedup_wave<false>); the same list with a ring of 256 has the room (q_cap = the read's length, rounded up)"""
    opt = pacbio_opt()
    rng = np.random.default_rng([seed, 61])
    cases = [join_case(W, rng, f"33 kb {kind}20", (("M", 16000), (kind, 20), ("M", 17000)), rev, fam=6, aim="long") for kind, rev in (("D", False), ("I", True))]
    tag_all(cases)
    assert all(c.read.shape[0] > 32736 and 8 * 4096 + 32 + ((c.read.shape[0] + 15) & ~15) > 65536 for c in cases)
    truth = [W.R.dedup(opt, c.read, c.regs) for c in cases]
    assert all(t.shape[0] == 1 and int(t["ncomp_isalt"][0] & 0x3fffffff) == 3 for t in truth)
    for ring in (4096, 256):
        left, got, form = run_list(W.dev, opt, cases, dedup_blk=1, dedup_ring=ring)
        check_list(f"33 kb reads, seed {seed}, dedup_blk 1, dedup_ring {ring}", cases, truth, got, form, np.ones(len(cases), dtype=np.int32))


def run_edges(W):
    """no reads; reads without regions; a batch on the handle keeps its results; what the entry rejects"""
    dev, opt = W.dev, default_opt()
    L, h = dev.L, dev.h
    left, got, form = dev.dedup_flat(opt, np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=ALNREG_DTYPE))
    assert left.shape[0] == 0 and got.shape[0] == 0
    reads = [rand_read(np.random.default_rng(k), 100 + k) for k in range(5)]
    seqs, off = testdata.ragged(reads)
    left, got, form = dev.dedup_flat(opt, seqs, off, np.zeros(5, dtype=np.int32), np.zeros(0, dtype=ALNREG_DTYPE))
    assert not left.any() and got.shape[0] == 0 and (form == 0).all()
    cases = [c for c in cases_of(W, SIM_SEED, True) if c.fam == 4][:6]
    truth = [W.R.dedup(opt, c.read, c.regs) for c in cases]
    seqs, off = testdata.ragged([c.read for c in cases])
    regs = np.concatenate([c.regs for c in cases])
    counts = np.array([c.regs.shape[0] for c in cases], dtype=np.int32)
    left = np.zeros(6, dtype=np.int32)
    p, n = C.c_void_p(), C.c_int64()

    def call(seqs=seqs, off=off, counts=counts, regs=regs, hh=h, oo=opt, n_reads=6, left=left, outs=(p, n), form=None):
        ptr = lambda x: None if x is None else x.ctypes.data
        return L.bwagpu_dedup_flat(hh, None if oo is None else C.byref(oo), n_reads, ptr(seqs), ptr(off), ptr(counts), ptr(regs), ptr(left), *[None if x is None else C.byref(x) for x in outs], ptr(form))

    def rejected(text, **kw):
        assert call(**kw) == -2, kw.keys()
        assert text in L.bwagpu_last_error(h).decode(), (text, L.bwagpu_last_error(h))
        assert call() == 0      # a valid call still works, without a form array
        got = dev._take(p, n.value, ALNREG_DTYPE)
        assert got.tobytes() == np.concatenate(truth).tobytes() and left.tolist() == [t.shape[0] for t in truth]

    for kw in (dict(hh=None), dict(oo=None), dict(n_reads=-1), dict(counts=None), dict(off=None), dict(regs=None), dict(seqs=None), dict(left=None), dict(outs=(None, n)), dict(outs=(p, None))):
        assert call(**kw) == -2, kw.keys()
    bad = counts.copy(); bad[2] = -1
    rejected("negative count", counts=bad)
    lens = np.diff(off)
    lp = W.l_pac
    for k, f, v, text in ((0, "qb", -1, "qb < 0"), (1, "qe", int(lens[0]) + 1, "qe beyond"), (2, "qe", int(regs["qb"][2]) - 1, "qe < qb"), (3, "rb", -1, "rb < 0"), (3, "re", 2 * lp + 1, "beyond 2 l_pac"),
                          (4, "re", int(regs["rb"][4]), "re <= rb"), (5, "rid", 3, "rid beyond")):
        bad = regs.copy(); bad[f][k] = v
        rejected(text, regs=bad)
    bad = regs.copy(); bad["rb"][0], bad["re"][0] = lp - 10, lp + 10
    rejected("bridges l_pac", regs=bad)
    for f, v in (("e_del", 0), ("e_ins", -1), ("w", -1)):
        o = default_opt(); setattr(o, f, v)
        rejected("must be positive", oo=o)
    bad = seqs.copy(); bad[7] = 5
    rejected("base code", seqs=bad)
    bad = off.copy(); bad[2] = bad[1] - 1
    rejected("ascend", off=bad)
    ok = regs.copy(); ok["rb"][0], ok["re"][0] = lp - 10, lp      # the strand's last bases, and the other strand's first
    ok["rb"][1], ok["re"][1] = lp, lp + 10
    assert call(regs=ok) == 0
    L.bwagpu_free(p)


def run_non_interference(W, n_reads, seed):
    """a batch's regions survive a bwagpu_dedup_flat call on the same handle, and the flat call gives the batch's own lists back"""
    from bwa_amd import simdata
    dev, opt = W.dev, default_opt()
    reads = simdata.make_reads_se(W.g, n_reads, seed=seed, sub=0.02, dele=0.02, ins=0.02)
    seqs, off = testdata.flat(reads)
    dev.set_taps(True)
    try:
        dev.upload(seqs, off); dev.run(opt)
        cases = [c for c in cases_of(W, SIM_SEED, True) if c.fam in (3, 5)][:30]
        truth = [W.R.dedup(opt, c.read, c.regs) for c in cases]
        left, got, form = run_list(dev, opt, cases)
        check_list("beside a batch", cases, truth, got, form, predict_forms({}, opt, max(c.read.shape[0] for c in cases), [c.regs.shape[0] for c in cases]))
        counts, regs = dev.download()
        raw_counts, raw = dev.tap_regs_raw()
    finally:
        dev.set_taps(False)
    dev.upload(seqs, off); dev.run(opt)
    c2, r2 = dev.download()
    assert np.array_equal(counts, c2) and regs.tobytes() == r2.tobytes()
    left, got, form = dev.dedup_flat(opt, seqs, off, raw_counts, raw)
    assert np.array_equal(left, counts) and got.tobytes() == regs.tobytes(), "the batch's raw lists through the flat entry"


# ---- fixtures and tests -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim():
    if not refapi.have_ref():      # (the CPU tests only: the GPU tests' fixture asserts instead)
        pytest.skip("oracle/_ref not built")
    import hostsim_build
    w = World(lib_path=hostsim_build.build(), options={"ptab_m": 6})
    yield w
    w.close()


@pytest.fixture(scope="module")
def gpu():
    # on the GPU box the compiled reference must have travelled with the snapshot: a silent skip would turn this module green with nothing run
    assert refapi.have_ref(), "oracle/_ref (the compiled reference) is missing on the GPU box"
    w = World()
    yield w
    w.close()


def test_limits_and_reference_entry(sim):
    """the limits are the literals the cases are aimed at; mem_sort_dedup_patch is exported and behaves as the cases assume: two exact pieces around a 3-base
    deletion join into one region of score 141, w 3, n_comp 3; around an 8-base deletion the 0.90 score ratio refuses them"""
    check_limits(sim.dev)
    rng = np.random.default_rng(5)
    for d, want in ((3, [(141, 3, 3)]), (8, [(80, 0, 1), (70, 0, 1)])):
        c = join_case(sim, rng, "probe", (("M", 70), ("D", d), ("M", 80)), False)
        t = sim.R.dedup(default_opt(), c.read, c.regs)
        assert [(int(x["score"]), int(x["w"]), int(x["ncomp_isalt"])) for x in t] == want, t


@pytest.mark.parametrize("seed", GPU_SEEDS)
def test_families_cover_their_boundaries(sim, seed):
    """the full lists of the GPU tests, on the reference's side alone"""
    cases = cases_of(sim, seed, False)
    for oname, opt in opt_sets():
        cover(sim, oname, opt, cases, truth_of(sim, cases, (seed, False, oname), opt), False)
    lc = long_cases_of(sim, seed, False)
    cover_long(sim, lc, truth_of(sim, lc, (seed, False, "long"), pacbio_opt()), False)


def test_sim_families(sim):
    run_families(sim, SIM_SEED, thin=True)


def test_sim_long_reads(sim):
    run_long(sim, SIM_SEED, thin=True)


def test_sim_no_query_room(sim):
    run_no_query_room(sim, SIM_SEED)


def test_sim_edges(sim):
    run_edges(sim)


def test_sim_non_interference(sim):
    run_non_interference(sim, 6, 96)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", GPU_SEEDS)
def test_gpu_families(gpu, seed):
    run_families(gpu, seed, thin=False)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", GPU_SEEDS)
def test_gpu_long_reads(gpu, seed):
    run_long(gpu, seed, thin=False)


@pytest.mark.gpu
def test_gpu_no_query_room(gpu):
    run_no_query_room(gpu, GPU_SEEDS[0])


@pytest.mark.gpu
def test_gpu_edges(gpu):
    run_edges(gpu)


@pytest.mark.gpu
def test_gpu_non_interference(gpu):
    run_non_interference(gpu, 400, 96)
