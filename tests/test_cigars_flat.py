"""The CIGAR stage of the device library (bwagpu_batch_cigars' kernels: cigars_run in bwa_amd/csrc/bwagpu.hip; k_cigar<true>, k_cigar<false>, k_cigar_long_plan,
k_cigar_long in bwa_amd/csrc/dev_cigar.h) on crafted region lists, through bwagpu_cigars_flat, against the compiled reference.

Truth per region: the reference's exported bwa_gen_cigar2 (bwa.c:148-234), called through ctypes on oracle/_ref/libbwaref.so inside a restatement of mem_reg2aln's
band loop (bwamem.c:1138-1152; ref_region below cites the lines): score, n_cigar, the operations, NM and the MD string the function leaves behind the operations.
The restatement is pinned to mem_reg2aln itself (bwamem.c:1119-1189) for every region that function accepts (pin_to_reg2aln).  A region for which bwa_gen_cigar2
returns 0 has no truth: the device must flag it (n_cigar -1, reason 2).

Regions are cut from the committed 200 kb genome: a target segment, a query segment made from it, random flanks around the query, on both strands (a
reverse-strand region is rb' = 2 l_pac - re with the read reverse-complemented).  truesc, w and score are inputs both sides only read; the cases set them to aim
at the switch points of the kernels (LIMITS, checked against bwagpu_cigar_limits).  Ten families (fam_* below); cover() asserts from the reference's side alone that
each produced members on both sides of its boundary.

Every served record must equal the truth exactly; the set of unserved records must equal the set predicted from the rules of family 9.  Which tier serves a region
is observed by running a list with cig_tiers = 1 / cig_long = 0, cig_tiers = 2 / cig_long = 0 and the defaults.
CPU: on the mock runtime (tests/hostsim), thinned.  -m gpu: everything, three seeds."""
import ctypes as C

import numpy as np
import pytest

import hostapi
import refapi
import testdata
from bwa_amd import simdata
from bwa_amd.api import CIGAR_DTYPE, BwaGpu
from bwa_amd.structs import ALNREG_DTYPE, MemOpt, default_opt, pacbio_opt

pytestmark = pytest.mark.skipif(not refapi.have_ref(), reason="oracle/_ref not built")

# the constants of dev_cigar.h the cases are aimed at
LIMITS = dict(max_len=320, z_small=6144, z_big=28672, max_cols=192, max_ops=6, tmp_ops=64, md_cap=1024, long_max_cols=1900, long_max_ops=32768, long_qcap=16384)
MAX_LEN, Z_SMALL, Z_BIG, MAX_COLS, MAX_OPS, TMP_OPS, LONG_COLS, LONG_QCAP = (LIMITS[k] for k in ("max_len", "z_small", "z_big", "max_cols", "max_ops", "tmp_ops", "long_max_cols", "long_qcap"))
GPU_SEEDS = (71, 72, 73)
SIM_SEED = 71


def check_limits(dev):
    assert dev.cigar_limits() == LIMITS, "a switch point moved: aim the cases at it"


def opt_sets():
    """the default, -x pacbio, the asymmetric-gap set of tests/test_dp_fuzz.py::_opts (max_ins != max_del, the two infer_bw calls disagree) and the default with
    w = 31 (so that regions whose w is 30 .. 33 lie below, at and above opt->w at bwamem.c:1142)"""
    a = default_opt()
    a.o_del, a.e_del, a.o_ins, a.e_ins = 8, 2, 5, 1
    w = default_opt()
    w.w = 31
    return [("default", default_opt()), ("pacbio", pacbio_opt()), ("asym", a), ("w31", w)]


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------------------
class RefAln(C.Structure):      # mem_aln_t (bwamem.h:114-127)
    _fields_ = [("pos", C.c_int64), ("rid", C.c_int), ("flag", C.c_int), ("is_rev", C.c_uint32, 1), ("is_alt", C.c_uint32, 1), ("mapq", C.c_uint32, 8), ("NM", C.c_uint32, 22),
                ("n_cigar", C.c_int), ("cigar", C.c_void_p), ("XA", C.c_void_p), ("score", C.c_int), ("sub", C.c_int), ("alt_sc", C.c_int)]


class Ref:
    def __init__(self, idx):
        L = refapi.lib()
        L.bwa_gen_cigar2.restype = C.c_void_p
        L.bwa_gen_cigar2.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mem_reg2aln.restype = RefAln
        L.mem_reg2aln.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        self.L, self.bns, self.pac, self.l_pac = L, L.refshim_idx_bns(idx.h), L.refshim_idx_pac(idx.h), idx.l_pac

    def gen(self, opt, w_, query, rb, re):
        """bwa_gen_cigar2 -> (score, n_cigar, operations, NM, MD) or None (it returned 0)"""
        q = np.ascontiguousarray(query, dtype=np.uint8).copy()      # (reversed in place and back for a reverse-strand hit)
        buf = q if q.shape[0] else np.zeros(1, dtype=np.uint8)
        sc, n, nm = C.c_int(0), C.c_int(0), C.c_int(0)
        p = self.L.bwa_gen_cigar2(C.addressof(opt) + MemOpt.mat.offset, opt.o_del, opt.e_del, opt.o_ins, opt.e_ins, int(w_), self.l_pac, self.pac, int(q.shape[0]), buf.ctypes.data,
                                  int(rb), int(re), C.byref(sc), C.byref(n), C.byref(nm))
        if not p:
            return None
        ops = tuple((C.c_uint32 * n.value).from_address(p))
        md = C.string_at(p + 4 * n.value)
        self.L.refshim_free(p)
        return (sc.value, n.value, ops, nm.value, md)


def infer_bw(l1, l2, score, a, q, r):      # bwamem.c:818-825
    if l1 == l2 and l1 * a - score < (q + r - a) << 1:
        return 0
    w = int((min(l1, l2) * a - score - q) / r + 2.)
    return max(w, abs(l1 - l2))


def ref_region(R, opt, read, reg):
    """mem_reg2aln's loop around bwa_gen_cigar2 -> (truth or None, [w2 of every attempt], why the loop ended: "same" score == last_sc, "wmax" w2 == opt->w << 2,
    "cond" the while condition)"""
    qb, qe, rb, re, truesc, aw = (int(reg[f]) for f in ("qb", "qe", "rb", "re", "truesc", "w"))
    tmp = infer_bw(qe - qb, re - rb, truesc, opt.a, opt.o_del, opt.e_del)       # bwamem.c:1138
    w2 = infer_bw(qe - qb, re - rb, truesc, opt.a, opt.o_ins, opt.e_ins)        # :1139
    w2 = max(w2, tmp)                                                           # :1140
    if w2 > opt.w:
        w2 = min(w2, aw)                                                        # :1142
    i, last_sc, tried = 0, -(1 << 30), []
    while True:                                                                 # :1144
        w2 = min(w2, opt.w << 2)                                                # :1146
        t = R.gen(opt, w2, read[qb:qe] if qe > qb else read[:0], rb, re)        # :1147
        tried.append(w2)
        if t is None:
            return None, tried, ""
        if t[0] == last_sc:                                                     # :1149
            return t, tried, "same"
        if w2 == opt.w << 2:
            return t, tried, "wmax"
        last_sc = t[0]                                                          # :1150
        w2 <<= 1                                                                # :1151
        i += 1
        if not (i < 3 and t[0] < truesc - opt.a):                               # :1152
            return t, tried, "cond"


def dp_band(opt, lq, rl, w_):
    """the band ksw_global2 gets from bwa_gen_cigar2 (bwa.c:180-187), None for the block without DP (bwa.c:168); used to classify cases, never as an expected value"""
    if lq == rl and w_ == 0:
        return None
    max_ins = int((((lq + 1) >> 1) * opt.mat[0] - opt.o_ins) / opt.e_ins + 1.)
    max_del = int((((lq + 1) >> 1) * opt.mat[0] - opt.o_del) / opt.e_del + 1.)
    max_gap = max(max_ins, max_del, 1)
    return max(min((max_gap + abs(rl - lq) + 1) >> 1, w_), abs(rl - lq) + 3)


def pin_to_reg2aln(R, opt, c, truth):
    """mem_reg2aln itself on the region: its n_cigar, NM and operations are the restated loop's after the end-deletion squeeze (bwamem.c:1157-1166) and the clips
    (:1167-1181)"""
    a = c.reg.copy()
    read = np.ascontiguousarray(c.read)
    r = R.L.mem_reg2aln(C.byref(opt), R.bns, R.pac, int(read.shape[0]), read.ctypes.data, a.ctypes.data)
    got = tuple((C.c_uint32 * r.n_cigar).from_address(r.cigar))
    R.L.refshim_free(r.cigar)
    want = list(truth[2])
    if want[0] & 0xf == 2:
        want = want[1:]
    elif want[-1] & 0xf == 2:
        want = want[:-1]
    qb, qe, lq = int(a["qb"][0]), int(a["qe"][0]), int(read.shape[0])
    rev = int(a["rb"][0]) >= R.l_pac
    c5, c3 = (lq - qe, qb) if rev else (qb, lq - qe)
    want = ([c5 << 4 | 3] if c5 else []) + want + ([c3 << 4 | 3] if c3 else [])
    assert (r.n_cigar, int(r.NM), got) == (len(want), truth[3], tuple(want)), f"{c.fam} {c.tag}: the restated loop and mem_reg2aln differ"
    assert bool(r.is_rev) == rev


# ---- crafted regions --------------------------------------------------------------------------------------------------------------------------------------
class World:
    def __init__(self, lib_path=None, options=None):
        self.prefix, self.g = testdata.small_index()
        lens = testdata.small_genome()[1]
        self.ctg = [(sum(lens[:i]), lens[i]) for i in range(len(lens))]
        self.dev = BwaGpu(self.prefix, lib_path=lib_path, options=options)
        self.idx = refapi.RefIndex(self.prefix)
        self.R = Ref(self.idx)
        self.l_pac = self.idx.l_pac
        self.T = default_opt().T
        assert self.l_pac == self.g.shape[0] == sum(lens) and len(lens) == 3

    def close(self):
        self.dev.close(); self.idx.close()


class Case:
    __slots__ = ("fam", "tag", "read", "reg", "rule", "legal")


def revcomp(s):
    s = np.asarray(s, dtype=np.uint8)
    return np.where(s < 4, 3 - s, 4)[::-1].astype(np.uint8)


def craft(W, rng, fam, tag, tb, rl, qseg, rev, truesc=None, w=100, score=None, rule=None, flanks=None):
    """a read holding qseg (given as it aligns to the forward strand's g[tb:tb + rl]) between random flanks, and its region on the strand asked for.
    truesc None: the alignment's real score with default options (a band of 4 opt->w).  rule: the (n_cigar, score) pair the region must come back with."""
    qseg = np.asarray(qseg, dtype=np.uint8)
    f5, f3 = flanks if flanks is not None else (int(rng.integers(0, 9)), int(rng.integers(0, 9)))
    read = np.concatenate([rng.integers(0, 4, f5).astype(np.uint8), revcomp(qseg) if rev else qseg, rng.integers(0, 4, f3).astype(np.uint8)])
    te = tb + rl
    c = Case()
    c.fam, c.tag, c.read, c.rule = fam, tag, read, rule
    c.reg = np.zeros(1, dtype=ALNREG_DTYPE)
    r = c.reg[0]
    r["rb"], r["re"] = (2 * W.l_pac - te, 2 * W.l_pac - tb) if rev else (tb, te)
    r["qb"], r["qe"] = f5, f5 + qseg.shape[0]
    rid = [k for k, (o, n) in enumerate(W.ctg) if o <= tb < o + n]
    r["rid"] = rid[0] if rid else 0
    c.legal = bool(rid) and te <= W.ctg[rid[0]][0] + W.ctg[rid[0]][1] and rl > 0 and qseg.shape[0] > 0
    if truesc is None:
        t = W.R.gen(default_opt(), 400, read[f5:f5 + qseg.shape[0]], r["rb"], r["re"])
        truesc = t[0] if t is not None else 0
    r["truesc"], r["w"] = truesc, w
    r["score"] = int(rng.integers(W.T, W.T + 200)) if score is None else score
    r["seedcov"], r["secondary"], r["secondary_all"] = qseg.shape[0] // 2 + 1, 0, 0
    return c


def place(W, rng, rl, margin=40):
    """the start of a target of rl bases inside one contig"""
    k = int(rng.integers(0, 3)) if rl + 2 * margin < W.ctg[2][1] else 0
    o, n = W.ctg[k]
    return int(rng.integers(o + margin, o + n - rl - margin))


def subst(rng, s, n, code=None):
    """n substitutions (or, with code 4, Ns) at distinct places"""
    s = s.copy()
    if n:
        at = rng.choice(s.shape[0], min(n, s.shape[0]), replace=False)
        s[at] = (s[at] + rng.integers(1, 4, at.shape[0])) & 3 if code is None else code
    return s


def one_gap(W, rng, tb, rl, dl, kind, at=None):
    """the query of g[tb:tb + rl] with one gap of dl bases: "del" -- dl target bases missing from the query; "ins" -- dl random bases added to it"""
    t = W.g[tb:tb + rl]
    at = rl // 2 if at is None else at
    if kind == "del":
        return np.concatenate([t[:at], t[at + dl:]])
    return np.concatenate([t[:at], rng.integers(0, 4, dl).astype(np.uint8), t[at:]])


def many_gaps(W, rng, tb, rl, n_gap, gap=9, first=12):
    """alternating one-base insertions and deletions, `gap` matches apart; an inserted base differs from both neighbours so that the gap stays where it is"""
    t = W.g[tb:tb + rl]
    out, i = [], 0
    for k in range(n_gap):
        nxt = first + k * gap
        out.append(t[i:nxt]); i = nxt
        if k % 2 == 0:
            b = [x for x in range(4) if x != int(t[i - 1]) and x != int(t[i])][0]
            out.append(np.array([b], dtype=np.uint8))
        else:
            i += 1
    out.append(t[i:])
    return np.concatenate(out)


def fam_ungapped(W, rng, thin):
    """1: l_query == rlen.  truesc at the real score (a band of 0 only while the mismatches are few) and at the length (a band of 0 whatever the mismatches:
    the block without DP, twice)"""
    out = []
    for L in (1, 2, 63, 64, 65, 128, MAX_LEN, MAX_LEN + 1, 1000):
        for rev in (False, True):
            for v, n_mm in enumerate((0, 1, 2, max(3, L // 10), L // 3)):
                if thin and ((v in (2, 3) and L != 65) or (L == 1000 and v and (v != 4 or rev))):
                    continue
                tb = place(W, rng, L)
                q = subst(rng, W.g[tb:tb + L], n_mm)
                if v == 3:
                    q = subst(rng, q, 1 + L // 20, code=4)
                if not (thin and L == 1000 and v):
                    out.append(craft(W, rng, 1, f"L{L} mm{n_mm} real", tb, L, q, rev))
                out.append(craft(W, rng, 1, f"L{L} mm{n_mm} top", tb, L, q, rev, truesc=L))
    return out


def fam_forms(W, rng, thin):
    """2: bands of 30 .. 33 (2 w + 1 = 61 .. 67: the diag form up to 63, the lds form from 65), reached through dl + 3, through the band inferred from truesc
    and through the clamp min(w2, ar->w)"""
    out = []
    for W_ in (30, 31, 32, 33):
        for rev in (False, True):
            for kind in ("del", "ins"):
                if thin and (rev != (kind == "del")):
                    continue
                dl = W_ - 3
                rl = int(rng.integers(150, 200))
                tb = place(W, rng, rl)
                out.append(craft(W, rng, 2, f"dl w{W_} {kind}", tb, rl, one_gap(W, rng, tb, rl, dl, kind), rev))
            if thin and rev != (W_ % 2 == 0):
                continue
            rl = 200
            tb = place(W, rng, rl)
            q = one_gap(W, rng, tb, rl, 2, "del", at=int(rng.integers(40, 160)))
            out.append(craft(W, rng, 2, f"truesc w{W_}", tb, rl, q, rev, truesc=198 - 6 - (W_ - 2)))
            out.append(craft(W, rng, 2, f"clamp w{W_}", tb, rl, q, rev, truesc=198 - 6 - 300, w=W_))
    return out


def fam_tiers(W, rng, thin):
    """3: the first tier's direction words (diag form, CIG_Z_SMALL), the second tier's nibbles (lds form, CIG_Z_BIG) and its columns (CIG_MAX_COLS), one gap of
    dl bases putting the band at dl + 3 on either side of each; the pairs follow from the limits"""
    out = []
    rows = 152                                                      # padded rows of the diag form: 145 .. 152 target bases
    w_s = max(w for w in range(3, 32) if rows * (2 * w + 1) <= Z_SMALL)      # 152 x 39 <= 6144 < 152 x 41
    w_b = max(w for w in range(32, 200) if MAX_LEN * (2 * w + 1) <= Z_BIG)    # 320 x 89 <= 28672 < 320 x 91
    w_c = (MAX_COLS - 1) // 2                                        # 2 w + 1 = 191 <= 192 < 193
    assert (w_s, w_b, w_c) == (19, 44, 95)
    for rev in (False, True):
        for w in (w_s - 1, w_s, w_s + 1, w_s + 2):
            rl = int(rng.integers(rows - 7, rows + 1))
            tb = place(W, rng, rl)
            out.append(craft(W, rng, 3, f"z_small w{w}", tb, rl, one_gap(W, rng, tb, rl, w - 3, "ins"), rev))
            if not thin:
                rl = int(rng.integers(rows - 7, rows + 1))
                tb = place(W, rng, rl)
                out.append(craft(W, rng, 3, f"z_small w{w} del", tb, rl, one_gap(W, rng, tb, rl, w - 3, "del"), rev))
        for w in (w_b - 1, w_b, w_b + 1, w_b + 2):
            if thin and rev != (w % 2 == 0):
                continue
            tb = place(W, rng, MAX_LEN)
            out.append(craft(W, rng, 3, f"z_big w{w}", tb, MAX_LEN, one_gap(W, rng, tb, MAX_LEN, w - 3, "del"), rev))
        for w in (w_c - 1, w_c, w_c + 1, w_c + 2):
            if thin and rev != (w % 2 == 0):
                continue
            tb = place(W, rng, 100)
            out.append(craft(W, rng, 3, f"max_cols w{w}", tb, 100, one_gap(W, rng, tb, 100, w - 3, "ins"), rev))
    return out


def fam_lengths(W, rng, thin):
    """4: l_query and rlen of 319, 320, 321, independently: with the length difference as the only gap (or one mismatch), and with a one-base insertion and a
    one-base deletion besides (a band the first tier has no room for at this length)"""
    out = []
    for lq in (MAX_LEN - 1, MAX_LEN, MAX_LEN + 1):
        for rl in (MAX_LEN - 1, MAX_LEN, MAX_LEN + 1):
            for rev in (False, True):
                if thin and rev != ((lq + rl) % 2 == 0):
                    continue
                tb = place(W, rng, rl)
                t = W.g[tb:tb + rl]
                fit = lambda q: np.concatenate([q[:230], q[230 + (rl - lq):]]) if lq < rl else np.concatenate([q[:230], rng.integers(0, 4, lq - rl).astype(np.uint8), q[230:]])
                q = t.copy()
                q[40] = (q[40] + 1) & 3
                out.append(craft(W, rng, 4, f"lq{lq} rl{rl} plain", tb, rl, fit(q), rev))
                # a one-base insertion and, 60 bases on, a one-base deletion; then the length difference as a gap of its own
                b = [x for x in range(4) if x != int(t[99]) and x != int(t[100])][0]
                q = fit(np.concatenate([t[:100], [b], t[100:160], t[161:]]).astype(np.uint8))
                assert q.shape[0] == lq
                out.append(craft(W, rng, 4, f"lq{lq} rl{rl} pair", tb, rl, q, rev))
    return out


MD_SHAPES = {7: ((30, 30), 8), 8: ((30, 30), 38), 9: ((30, 30), 138), 10: ((30, 30, 30), 8)}      # MD length: (matches in front of each mismatch, matches behind the last)


def fam_records(W, rng, thin):
    """5: 5, 6, 7, 8 and 63 .. 66 operations (an even count through a deletion at the alignment's first base), with bands for every tier; MD strings of 7 .. 10
    characters with one operation and with seven (three insertions, which MD does not see)"""
    out = []
    for n_ops in (5, 6, 7, 8, 63, 64, 65, 66):
        n_gap, lead = (n_ops - 1) // 2, 2 * (n_ops % 2 == 0)
        for rev in (False, True):
            for w in ((7, 12, 100) if not thin else ((7, 100) if rev else (12,))):
                ql = 12 + n_gap * 9 + 10 + int(rng.integers(0, 4))
                ql = max(ql, 260) if w == 12 else ql          # (25 diagonals: more than CIG_Z_SMALL direction words take 246 rows)
                if n_ops >= 63 and w == 12:
                    ql = MAX_LEN - 4
                tb = place(W, rng, ql + lead)
                q = many_gaps(W, rng, tb + lead, ql, n_gap)
                out.append(craft(W, rng, 5, f"ops{n_ops} w{w}", tb, ql + lead, q, rev, w=w, truesc=-400))
    for md_len, (runs, tail) in MD_SHAPES.items():
        L = sum(runs) + len(runs) + tail
        for rev in (False, True):
            for many in (False, True):
                tb = place(W, rng, L)
                q = W.g[tb:tb + L].copy()
                at = 0
                for r in runs:
                    at += r
                    q[at] = (q[at] + 1 + int(rng.integers(0, 3))) & 3
                    at += 1
                if many:      # three one-base insertions in the runs of matches, well away from the mismatches
                    for p in (45, 19, 8):
                        b = [x for x in range(4) if x != int(q[p - 1]) and x != int(q[p])][0]
                        q = np.concatenate([q[:p], [b], q[p:]]).astype(np.uint8)
                out.append(craft(W, rng, 5, f"md{md_len} {'many' if many else 'few'}", tb, L, q, rev))
    return out


def fam_doubling(W, rng, thin):
    """6: one gap of 20 .. 70 bases with truesc at the real score, above it by a, 2 a and a lot; an insertion and a deletion of g bases each, 40 apart, under a
    truesc that starts the band below g (the score changes when the band doubles); bands that start above opt->w and reach 4 opt->w"""
    out = []
    for gap in ((20, 45, 70) if not thin else (20, 70)):
        for rev in (False, True):
            for kind in ("del", "ins"):
                if thin and rev != (kind == "del"):
                    continue
                rl = int(rng.integers(150, 240))
                tb = place(W, rng, rl)
                q = one_gap(W, rng, tb, rl, gap, kind)
                c = craft(W, rng, 6, f"gap{gap} {kind} +0", tb, rl, q, rev)
                out.append(c)
                real = int(c.reg["truesc"][0])
                for up in (1, 2, 1000):
                    out.append(craft(W, rng, 6, f"gap{gap} {kind} +{up}", tb, rl, q, rev, truesc=real + up))
    for g_ in ((10, 12, 14) if not thin else (12,)):
        for rev in (False, True):
            rl = 200
            tb = place(W, rng, rl)
            t = W.g[tb:tb + rl]
            q = np.concatenate([t[:60], rng.integers(0, 4, g_).astype(np.uint8), t[60:100], t[100 + g_:]])
            for w2 in (8, g_ + 4):       # infer_bw gives w2 for truesc = l - 6 - (w2 - 2): bands of 8 (misses the gaps), 16 (finds them), 32; or wide enough at once
                out.append(craft(W, rng, 6, f"pair{g_} from{w2}", tb, rl, q, rev, truesc=rl - 6 - (w2 - 2)))
            # a query that hardly aligns: the band inferred from truesc lies above opt->w and starts at ar->w; 4 opt->w ends the loop
            q = rng.integers(0, 4, rl).astype(np.uint8)
            for truesc, aw in ((90, 150), (-4, 200), (-210, 400), (-210, 1000)):
                out.append(craft(W, rng, 6, f"junk truesc{truesc} ar_w{aw}", tb, rl, q, rev, truesc=truesc, w=aw))
    if not thin:      # 900 bases (bwa.c:184 allows a band of 223): gaps of 210 that a band of 200 misses and the next, capped at 4 opt->w, finds
        for rev in (False, True):
            tb = place(W, rng, 900)
            t = W.g[tb:tb + 900]
            q = np.concatenate([t[:100], rng.integers(0, 4, 210).astype(np.uint8), t[100:500], t[710:]])
            out.append(craft(W, rng, 6, "pair210 ar_w200", tb, 900, q, rev, truesc=900 - 6 - 198, w=200))
    return out


def find_repeats(g, lo, hi, unit, min_len):
    """starts of runs of period `unit` of at least min_len bases inside g[lo:hi]"""
    same = g[lo + unit:hi] == g[lo:hi - unit]
    out, run = [], 0
    for i, s in enumerate(same.tolist()):
        run = run + 1 if s else 0
        if run == min_len - unit:
            out.append(lo + i + unit + 1 - min_len)
    return out


def fam_repeats(W, rng, thin):
    """7: one unit of a homopolymer run or of a di- / tri-nucleotide repeat of the genome missing from, or doubled in, the read: several places for the gap give
    the same score, the reference puts it leftmost on the forward strand -- on both strands.  Each case as a forward and as a reverse region"""
    out = []
    o, n = W.ctg[0]
    for unit, min_len in ((1, 5), (2, 8), (3, 9)):
        runs = find_repeats(W.g, o + 100, o + n - 100, unit, min_len)
        assert len(runs) >= 4, (unit, len(runs))
        for p in [runs[int(k)] for k in rng.choice(len(runs), 3 if thin else 12, replace=False)]:
            tb, rl = p - int(rng.integers(30, 60)), int(rng.integers(100, 140))
            at = p - tb + unit * int(rng.integers(0, 2))      # (anywhere inside the run)
            t = W.g[tb:tb + rl]
            for kind, q in (("del", np.concatenate([t[:at], t[at + unit:]])), ("ins", np.concatenate([t[:at], t[at:at + unit], t[at:]]))):
                for rev in (False, True):
                    out.append(craft(W, rng, 7, f"unit{unit} {kind} @{p}", tb, rl, q, rev))
    return out


def fam_end_dels(W, rng, thin):
    """8: the target reaches 1 .. 10 bases past the query's first or last base: the alignment opens or closes with a D, which NM and MD ignore (bwa.c:213-214)"""
    out = []
    for ext in ((1, 2, 3, 5, 10) if not thin else (1, 10)):
        for end in (0, 1):
            for rev in (False, True):
                for n_mm in (0, 2):
                    ql = int(rng.integers(60, 150))
                    tb = place(W, rng, ql + ext)
                    lo = tb + ext if end == 0 else tb
                    q = W.g[lo:lo + ql].copy()
                    if n_mm:
                        q[[20, 40]] = (q[[20, 40]] + 1) & 3
                    out.append(craft(W, rng, 8, f"ext{ext} end{end} mm{n_mm}", tb, ql + ext, q, rev))
    return out


def fam_rules(W, rng, thin):
    """9: shapes the kernels classify (reason 2), scores below T (reason 1), a band of more than CIGL_MAX_COLS columns (reason 2) beside one of just fewer"""
    out = []
    L = W.l_pac
    for rev in (False, True):
        tb = place(W, rng, 100)
        q = W.g[tb:tb + 100]
        c = craft(W, rng, 9, "qe == qb", tb, 100, q[:0], rev, truesc=50, rule=(-1, 2)); out.append(c)
        c = craft(W, rng, 9, "rb == re", tb, 0, q, rev, truesc=50, rule=(-1, 2)); out.append(c)
        c = craft(W, rng, 9, "qe < qb", tb, 100, q, rev, truesc=50, rule=(-1, 2)); c.reg["qe"] = c.reg["qb"] - min(3, int(c.reg["qb"][0])); c.legal = False; out.append(c)
        c = craft(W, rng, 9, "rb > re", tb, 100, q, rev, truesc=50, rule=(-1, 2)); c.reg["rb"], c.reg["re"] = c.reg["re"][0], c.reg["rb"][0]; c.legal = False; out.append(c)
        for sc in (0, W.T - 1):
            out.append(craft(W, rng, 9, f"score {sc}", tb, 100, q, rev, score=sc, rule=(-1, 1)))
        out.append(craft(W, rng, 9, "score T", tb, 100, q, rev, score=W.T))
    for lo, hi in ((L - 50, L + 50), (L - 1, L + 1), (L - 100, L + 1), (L - 1, L + 100)):      # rb < l_pac < re
        c = craft(W, rng, 9, f"bridge {lo - L} {hi - L}", lo, hi - lo, W.g[-(hi - lo):], False, truesc=50, rule=(-1, 2)); c.legal = False; out.append(c)
    for lo, hi in ((L - 100, L), (L, L + 100)):      # ... and on either side of it: the last bases of the forward strand, the first of the reverse strand
        rev = lo >= L
        out.append(craft(W, rng, 9, f"edge {lo - L} {hi - L}", L - 100, 100, W.g[L - 100:L], rev))
    o1 = W.ctg[1][0]      # two contigs: the reference computes it, mem_reg2aln would assert on the rid
    for rev in (False, True):
        c = craft(W, rng, 9, "two contigs", o1 - 60, 120, subst(rng, W.g[o1 - 60:o1 + 60], 2), rev); c.legal = False; out.append(c)
    # l_query 2000: 2 w + 1 = 2 (dl + 3) + 1 columns, 1897 for dl 945 (served by the long tier), 1907 for dl 950 (nobody's)
    for dl in ((945, 950) if not thin else (950,)):
        rl = 2000 - dl
        tb = place(W, rng, rl)
        out.append(craft(W, rng, 9, f"band dl{dl}", tb, rl, one_gap(W, rng, tb, rl, dl, "ins"), dl % 2 == 0, truesc=0))
    return out


def fam_long(W, rng, thin):
    """10: the long tier: segments of 400, 1000, 2500 bases with narrow bands; one longer than CIGL_QCAP whose band is dl + 3; a gap of more than 16 columns within 64 rows;
    more than 64 operations on 300 bases -- beside 300-base segments of up to 64 operations with bands for the first and the second tier"""
    out = []
    for L in ((400, 1000, 2500) if not thin else (400, 1000)):
        for rev in (False, True):
            if thin and rev != (L == 400):
                continue
            tb = place(W, rng, L)
            q = subst(rng, many_gaps(W, rng, tb, L, 6, gap=L // 8, first=30), L // 100)
            out.append(craft(W, rng, 10, f"L{L}", tb, L, q, rev))
    if not thin:
        L = LONG_QCAP + 700
        tb = place(W, rng, L + 5)
        q = subst(rng, one_gap(W, rng, tb, L + 5, 5, "del", at=9000), 40)
        out.append(craft(W, rng, 10, "over qcap", tb, L + 5, q, True, truesc=L - 11))      # (the band inferred from a score without the mismatches: 7, so dl + 3)
    for rev in (False, True):
        for gap in (17, 25, 40):
            if thin and rev != (gap == 25):
                continue
            tb = place(W, rng, 400)
            out.append(craft(W, rng, 10, f"tile ins{gap}", tb, 400, one_gap(W, rng, tb, 400, gap, "ins", at=int(rng.integers(100, 300))), rev))
        for n_gap, w in ((33, 100), (34, 7), (30, 7), (30, 12)):
            if thin and rev != (n_gap % 2 == 0):
                continue
            tb = place(W, rng, 300)
            out.append(craft(W, rng, 10, f"300 gaps{n_gap} w{w}", tb, 300, many_gaps(W, rng, tb, 300, n_gap, gap=8), rev, w=w, truesc=-400))
    return out


FAMILIES = (fam_ungapped, fam_forms, fam_tiers, fam_lengths, fam_records, fam_doubling, fam_repeats, fam_end_dels, fam_rules, fam_long)
_cases, _truth = {}, {}


def cases_of(W, seed, thin):
    """the crafted list of a seed (made once)"""
    key = (seed, thin)
    if key not in _cases:
        out = []
        for k, f in enumerate(FAMILIES):
            out += f(W, np.random.default_rng([seed, k]), thin)
        _cases[key] = out
    return _cases[key]


def truth_of(W, seed, thin, oname, opt):
    """[(truth, attempts, why)] of the list under one option set (computed once, shared and left alone), every legal region pinned to mem_reg2aln"""
    key = (seed, thin, oname)
    if key not in _truth:
        out = []
        for c in cases_of(W, seed, thin):
            t = ref_region(W.R, opt, c.read, c.reg[0])
            if c.legal and t[0] is not None:
                pin_to_reg2aln(W.R, opt, c, t[0])
            out.append(t)
        _truth[key] = out
    return _truth[key]


def predicted_rule(opt, c, t):
    """family 9: the (n_cigar, reason) a region must come back with, or None (it must be served)"""
    r = c.reg[0]
    if int(r["score"]) < opt.T:
        return (-1, 1)
    if t[0] is None:      # bwa_gen_cigar2 returned 0
        return (-1, 2)
    lq, rl = int(r["qe"] - r["qb"]), int(r["re"] - r["rb"])
    for w_ in t[1]:
        w = dp_band(opt, lq, rl, w_)
        if w is not None and min(lq, 2 * w + 1) > LONG_COLS:
            return (-1, 2)
    return None


def cover(W, cases, truth, thin):
    """every family on both sides of its boundary, from the reference's side alone (default options)"""
    opt = default_opt()
    fam = lambda k: [(c, t) for c, t in zip(cases, truth) if c.fam == k]
    rev = lambda c: int(c.reg["rb"][0]) >= W.l_pac
    dims = lambda c: (int(c.reg["qe"][0] - c.reg["qb"][0]), int(c.reg["re"][0] - c.reg["rb"][0]))
    band = lambda c, t: dp_band(opt, *dims(c), t[1][-1])
    # 1
    for L in (1, 2, 63, 64, 65, 128, MAX_LEN, MAX_LEN + 1, 1000):
        here = [(c, t) for c, t in fam(1) if dims(c) == (L, L)]
        assert any(band(c, t) is None and t[0][3] > 2 for c, t in here) or L < 3, f"1: no run without DP and with many mismatches at {L}"
        assert any(band(c, t) is None and t[0][3] == 0 for c, t in here) and {rev(c) for c, t in here} == {False, True}, L
        assert all(t[0][1] == 1 for c, t in here if band(c, t) is None)
    assert any(band(c, t) is not None for c, t in fam(1)) and any(4 in c.read[int(c.reg["qb"][0]):int(c.reg["qe"][0])] for c, t in fam(1))
    # 2
    for how in ("dl", "truesc", "clamp"):
        got = {band(c, t) for c, t in fam(2) if c.tag.startswith(how)}
        assert got == {30, 31, 32, 33}, (how, got)
    assert {t[0][1] > 1 for c, t in fam(2)} == {True}
    # 3
    z = lambda c, t: (lambda lq, rl, w: ("diag", ((rl + 7) & ~7) * (2 * w + 1)) if 2 * w + 1 <= 64 else ("lds", min(lq, 2 * w + 1) * ((rl + 1) & ~1), min(lq, 2 * w + 1)))(*dims(c), band(c, t))
    zz = [z(c, t) for c, t in fam(3)]
    assert any(x[0] == "diag" and x[1] <= Z_SMALL for x in zz) and any(x[0] == "diag" and x[1] > Z_SMALL for x in zz)
    assert any(x[0] == "lds" and x[1] <= Z_BIG and x[2] <= MAX_COLS for x in zz) and any(x[0] == "lds" and x[1] > Z_BIG and x[2] <= MAX_COLS for x in zz)
    assert any(x[0] == "lds" and x[2] == MAX_COLS - 1 for x in zz) and any(x[0] == "lds" and x[2] == MAX_COLS + 1 and x[1] <= Z_BIG for x in zz)
    assert max(x[1] for x in zz if x[0] == "diag" and x[1] <= Z_SMALL) + 2 * 152 > Z_SMALL      # (the nearest pair the shape allows)
    # 4
    assert {dims(c) for c, t in fam(4)} == {(a, b) for a in (319, 320, 321) for b in (319, 320, 321)}
    assert all(t[0][1] >= 5 for c, t in fam(4) if c.tag.endswith("pair"))
    # 5
    n_ops = {t[0][1] for c, t in fam(5)}
    assert {5, 6, 7, 8, 63, 64, 65, 66} <= n_ops, sorted(n_ops)
    forms = {(len(t[0][4]), t[0][1] > MAX_OPS) for c, t in fam(5)}
    assert {(m, a) for m in (7, 8, 9, 10) for a in (False, True)} <= forms, sorted(forms)
    # 6
    tries = {(len(t[1]), t[2]) for c, t in fam(6)}
    assert {1, 2, 3} == {a for a, _ in tries} and {"same", "wmax", "cond"} == {w for _, w in tries}, tries
    assert (2, "same") in tries and (3, "same") in tries and (thin or (2, "wmax") in tries) and (1, "wmax") in tries and (1, "cond") in tries, tries
    assert any(c.tag.endswith("+0") and len(t[1]) == 1 for c, t in fam(6)) and any(c.tag.endswith("+2") and len(t[1]) == 2 for c, t in fam(6))
    # 7: a gap in every case, on both strands, and the two strands of a case agree in the reference
    f7 = fam(7)
    assert all(t[0][1] == 3 for c, t in f7) and {t[0][2][1] & 0xf for c, t in f7} == {1, 2}
    for k in range(0, len(f7), 2):
        assert f7[k][0].tag == f7[k + 1][0].tag and not rev(f7[k][0]) and rev(f7[k + 1][0]) and f7[k][1][0] == f7[k + 1][1][0]
    # 8
    ends = {(t[0][2][0] & 0xf == 2, t[0][2][-1] & 0xf == 2, rev(c)) for c, t in fam(8)}
    assert {(True, False, False), (True, False, True), (False, True, False), (False, True, True)} <= ends, ends
    assert any(t[0][3] == 0 and t[0][1] == 2 and t[0][4] == str(dims(c)[0]).encode() for c, t in fam(8))
    # 9
    rules = [predicted_rule(opt, c, t) for c, t in fam(9)]
    assert rules.count((-1, 1)) >= 4 and rules.count((-1, 2)) >= 10 and rules.count(None) >= 6
    assert [r for (c, t), r in zip(fam(9), rules) if c.tag.startswith("band")] == ([None, (-1, 2)] if not thin else [(-1, 2)])
    assert all((r is not None) == (c.rule is not None) and (r is None or r == c.rule) for (c, t), r in zip(fam(9), rules) if not c.tag.startswith("band"))
    assert all(predicted_rule(opt, c, t) is None for c, t in zip(cases, truth) if c.fam != 9)
    # 10
    f10 = fam(10)
    assert any(t[0][1] > TMP_OPS and dims(c)[0] <= MAX_LEN for c, t in f10) and any(MAX_OPS < t[0][1] <= TMP_OPS and dims(c)[0] <= MAX_LEN for c, t in f10)
    assert any((op & 0xf) == 1 and (op >> 4) > 16 for c, t in f10 for op in t[0][2])
    assert thin or any(dims(c)[0] > LONG_QCAP for c, t in f10)
    assert {min(dims(c)) > MAX_LEN for c, t in f10} == {False, True}


# ---- the device side ----------------------------------------------------------------------------------------------------------------------------------------
def run_list(dev, opt, cases, **options):
    """bwagpu_cigars_flat on one read per case, under the handle options given (restored afterwards)"""
    seqs, off = testdata.ragged([c.read for c in cases])
    regs = np.concatenate([c.reg for c in cases]) if cases else np.zeros(0, dtype=ALNREG_DTYPE)
    old = {k: dev.get_option(k) for k in options}
    try:
        for k, v in options.items():
            dev.set_option(k, v)
        return dev.cigars_flat(opt, seqs, off, np.ones(len(cases), dtype=np.int32), regs)
    finally:
        for k, v in old.items():
            dev.set_option(k, v)


def array_spans(cigs):
    """[(first entry, entries)] of every record's claims on the operation array"""
    out = []
    for c in cigs:
        n, ml = int(c["n_cigar"]), int(c["md_len"])
        if n > MAX_OPS:
            out.append((int(c["cigar"][1]) << 32 | int(c["cigar"][0]), n))
        if n >= 0 and ml > 8:
            out.append((int(c["md"]), (ml + 3) // 4))
    return out


def check_records(what, opt, cases, truth, cigs, ops, rules=None):
    """served records equal the truth, the others are the predicted ones with their reason and nothing else; the operation array is claimed once"""
    assert cigs.shape[0] == len(cases)
    dec = hostapi.decode_cigars(cigs, ops)
    for k, (c, t) in enumerate(zip(cases, truth)):
        rule = predicted_rule(opt, c, t) if rules is None else rules[k]
        g = cigs[k]
        if rule is not None:
            assert (int(g["n_cigar"]), int(g["score"])) == rule, f"{what}: {c.fam} {c.tag}: ({int(g['n_cigar'])}, {int(g['score'])}), predicted {rule}"
            assert not g["cigar"].any() and int(g["nm"]) == -1 and int(g["md_len"]) == 0 and int(g["md"]) == 0, f"{what}: {c.fam} {c.tag}: the rest of an unserved record"
        else:
            assert int(g["n_cigar"]) >= 0, f"{what}: {c.fam} {c.tag}: not served: ({int(g['n_cigar'])}, {int(g['score'])}); the reference has {t[0][:2]}"
            assert dec[k] == t[0] and int(g["md_len"]) == len(t[0][4]), f"{what}: {c.fam} {c.tag}:\n device    {dec[k]}\n reference {t[0]}"
            if int(g["n_cigar"]) <= MAX_OPS:
                assert not g["cigar"][max(int(g["n_cigar"]), 0):].any()
    spans = sorted(array_spans(cigs))
    assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:])), f"{what}: two records share entries of the operation array"
    need = sum(n for _, n in spans)
    assert (not spans or spans[0][0] >= 0) and ops.shape[0] == need and (not spans or spans[-1][0] + spans[-1][1] <= need), f"{what}: {ops.shape[0]} entries, the records claim {need}"
    return dec, need


def need_of(truths):
    """entries of the operation array the records of these truths claim: the operations of more than CIG_MAX_OPS, the MD strings of more than 8 characters"""
    return sum((t[0][1] if t[0][1] > MAX_OPS else 0) + ((len(t[0][4]) + 3) // 4 if len(t[0][4]) > 8 else 0) for t in truths)


def run_families(W, seed, thin):
    dev = W.dev
    check_limits(dev)
    cases = cases_of(W, seed, thin)
    for oname, opt in opt_sets():
        truth = truth_of(W, seed, thin, oname, opt)
        if oname == "default":
            cover(W, cases, truth, thin)
        what = f"seed {seed}, {oname}"
        if thin and oname != "default":      # (the mock runtime's budget: the other option sets with all tiers only)
            check_records(what, opt, cases, truth, *run_list(dev, opt, cases))
            continue
        # the tiers, observed: the first alone, the first two, all three
        a = run_list(dev, opt, cases, cig_tiers=1, cig_long=0)
        b = run_list(dev, opt, cases, cig_tiers=2, cig_long=0)
        d = run_list(dev, opt, cases)
        dec_d, need = check_records(what, opt, cases, truth, *d)
        rules = [predicted_rule(opt, c, t) for c, t in zip(cases, truth)]
        s_a, s_b, s_d = (x[0]["n_cigar"] >= 0 for x in (a, b, d))
        assert not (s_a & ~s_b).any() and not (s_b & ~s_d).any(), f"{what}: the served sets do not nest"
        assert set(a[0]["n_cigar"][~s_a].tolist()) <= {-1, -2} and (a[0]["n_cigar"][s_b & ~s_a] == -2).all() and (b[0]["n_cigar"][~s_b] == -1).all(), what
        for got, served, name in ((a, s_a, "first tier alone"), (b, s_b, "two tiers")):
            dec = hostapi.decode_cigars(got[0], got[1])
            for k in np.nonzero(served)[0]:
                assert dec[k] == dec_d[k], f"{what}: {cases[k].fam} {cases[k].tag}: {name} and the defaults differ"
                if not array_spans(got[0][k:k + 1]):
                    assert got[0][k].tobytes() == d[0][k].tobytes()
            for k in np.nonzero(~served)[0]:      # what no tier of this configuration took: -2 / -1 with reason 2, or the rule's record
                g = got[0][k]
                assert (int(g["n_cigar"]), int(g["score"])) == rules[k] if rules[k] is not None else int(g["score"]) == 2, (what, name, cases[k].tag)
                assert not g["cigar"].any() and int(g["nm"]) == -1 and int(g["md_len"]) == 0 and int(g["md"]) == 0
            sp = sorted(array_spans(got[0]))
            assert all(x + n <= y for (x, n), (y, _) in zip(sp, sp[1:])) and sum(n for _, n in sp) == got[1].shape[0]
        if oname == "default":
            tier = np.where(s_a, 0, np.where(s_b, 1, np.where(s_d, 2, -1)))
            for f in (3, 4, 5, 10):
                seen = {int(tier[k]) for k, c in enumerate(cases) if c.fam == f} - {-1}
                assert seen == {0, 1, 2}, f"{what}: family {f} has members first served at tiers {sorted(seen)} only"
            # the second attempt of the operation array, and the long tier with one workgroup
            assert need == need_of([t for t, r in zip(truth, rules) if r is None])
            sub = list(range(0, len(cases), 3 if thin else 1))      # (the mock runtime's budget: a third of the list for the passes below)
            need = need_of([truth[k] for k in sub if rules[k] is None])
            assert need > 40
            for cap in (10, need - 1):
                e = run_list(dev, opt, [cases[k] for k in sub], cig_ops_cap=cap)
                assert hostapi.decode_cigars(*e) == [dec_d[k] for k in sub] and e[1].shape[0] == need, f"{what}: cig_ops_cap {cap}"
            sel = [k for k, c in enumerate(cases) if c.fam == 10]
            e = run_list(dev, opt, [cases[k] for k in sel], cigl_mib=0)
            assert hostapi.decode_cigars(*e) == [dec_d[k] for k in sel], f"{what}: cigl_mib 0"
            # a region's record depends neither on its place nor on its neighbours
            perm = np.random.default_rng(seed).permutation(sub)
            e = run_list(dev, opt, [cases[k] for k in perm])
            assert hostapi.decode_cigars(*e) == [dec_d[k] for k in perm], f"{what}: a permuted list"


def run_filter(W, seed):
    """bwagpu_set_cigar_filter(1): reads of three regions -- the best, and two that score below / not below XA_drop_ratio times its score while they overlap it /
    do not (by mask_level)"""
    rng = np.random.default_rng([seed, 99])
    opt = default_opt()
    reads, regs, want = [], [], []
    for rev in (False, True):
        for s2, overlap in ((79, True), (80, True), (30, True), (79, False), (40, False)):      # against a best score of 100: 100 * 0.8f is 80 in float
            tb = place(W, rng, 100)
            best = craft(W, rng, 9, "best", tb, 100, subst(rng, W.g[tb:tb + 100], 1), rev, score=100, flanks=(5, 100))
            t2 = place(W, rng, 60)
            qb = 5 + 20 if overlap else 5 + 100 + 10
            other = craft(W, rng, 9, "other", t2, 60, subst(rng, W.g[t2:t2 + 60], 1), not rev, score=s2, flanks=(0, 0))
            read = best.read.copy()
            read[qb:qb + 60] = other.read
            other.reg["qb"], other.reg["qe"] = qb, qb + 60
            reads.append(read); regs += [best.reg, other.reg]
            skipped = overlap and np.float32(s2) < np.float32(100) * np.float32(opt.XA_drop_ratio)
            want += [False, bool(skipped)]
    seqs, off = testdata.ragged(reads)
    regs = np.concatenate(regs)
    counts = np.full(len(reads), 2, dtype=np.int32)
    plain = W.dev.cigars_flat(opt, seqs, off, counts, regs)
    assert (plain[0]["n_cigar"] > 0).all()
    assert W.dev.L.bwagpu_set_cigar_filter(W.dev.h, 1) == 0
    try:
        cigs, ops = W.dev.cigars_flat(opt, seqs, off, counts, regs)
    finally:
        assert W.dev.L.bwagpu_set_cigar_filter(W.dev.h, 0) == 0
    want = np.array(want)
    assert want.sum() >= 4 and (~want).sum() >= 12
    assert np.array_equal(cigs["n_cigar"] < 0, want), (cigs["n_cigar"].tolist(), want.tolist())
    f = cigs[want]
    assert (f["n_cigar"] == -1).all() and (f["score"] == 1).all() and (f["nm"] == -1).all() and not f["cigar"].any() and not f["md_len"].any() and not f["md"].any()
    dp, df = hostapi.decode_cigars(*plain), hostapi.decode_cigars(cigs, ops)
    assert all(df[k] == dp[k] for k in np.nonzero(~want)[0])
    for k in np.nonzero(~want)[0]:      # ... and what is served is the reference's
        c = Case(); c.read = reads[k // 2]; c.reg = regs[k:k + 1]
        assert df[k] == ref_region(W.R, opt, c.read, c.reg[0])[0]


def run_concurrent(W, seed, n_regions):
    """thousands of records that all reserve from the operation array: distinct array-form regions of the LDS tiers, repeated in a shuffled list"""
    opt = default_opt()
    cases = cases_of(W, seed, False)
    truth = truth_of(W, seed, False, "default", opt)
    pool = [k for k, (c, t) in enumerate(zip(cases, truth)) if t[0] is not None and predicted_rule(opt, c, t) is None and int(c.reg["qe"][0] - c.reg["qb"][0]) <= MAX_LEN
            and int(c.reg["re"][0] - c.reg["rb"][0]) <= MAX_LEN and (t[0][1] > MAX_OPS or len(t[0][4]) > 8)]
    assert len(pool) >= 60, len(pool)
    order = np.random.default_rng([seed, 7]).choice(pool, n_regions)
    lst, tr = [cases[k] for k in order], [truth[k] for k in order]
    for cap in (0, 10):      # the array as the stage sizes it (4 entries per region: too few here, a second attempt on its own), and the test hook
        cigs, ops = run_list(W.dev, opt, lst, cig_ops_cap=cap)
        dec, need = check_records(f"concurrent, seed {seed}, cap {cap}", opt, lst, tr, cigs, ops)
        assert need == need_of(tr)


def run_non_interference(W, n_reads, seed):
    """a batch's records and operation array survive a bwagpu_cigars_flat call on the same handle, and the other way round"""
    dev, opt = W.dev, default_opt()
    reads = simdata.make_reads_se(W.g, n_reads, seed=seed, sub=0.02, dele=0.02, ins=0.02)
    seqs, off = testdata.flat(reads)
    dev.upload(seqs, off); dev.run(opt)
    counts, regs = dev.download()
    c1, o1 = dev.cigars(opt), dev.cigar_ops()
    assert (c1["n_cigar"] > MAX_OPS).any()
    cases = [c for c in cases_of(W, SIM_SEED, True) if c.fam in (5, 8)]
    f1 = run_list(dev, opt, cases)
    assert f1[1].shape[0] > 0
    o1b = dev.cigar_ops()
    assert o1b.tobytes() == o1.tobytes(), "the batch's operation array changed under bwagpu_cigars_flat"
    c2, o2 = dev.cigars(opt), dev.cigar_ops()
    assert hostapi.decode_cigars(c2, o2) == hostapi.decode_cigars(c1, o1) and o2.shape[0] == o1.shape[0]
    f2 = run_list(dev, opt, cases)
    assert hostapi.decode_cigars(*f2) == hostapi.decode_cigars(*f1) and f2[1].shape[0] == f1[1].shape[0]
    # the batch's lists through the flat entry: the same records
    f3 = dev.cigars_flat(opt, seqs, off, counts, regs)
    assert hostapi.decode_cigars(*f3) == hostapi.decode_cigars(c1, o1)


def run_error_paths(W):
    dev, opt = W.dev, default_opt()
    L, h = dev.L, dev.h
    cases = [c for c in cases_of(W, SIM_SEED, True) if c.fam == 8][:4]
    seqs, off = testdata.ragged([c.read for c in cases])
    regs = np.concatenate([c.reg for c in cases])
    counts = np.ones(4, dtype=np.int32)
    want = hostapi.decode_cigars(*dev.cigars_flat(opt, seqs, off, counts, regs))
    p, n, po, no = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_int64()

    def call(seqs=seqs, off=off, counts=counts, regs=regs, hh=h, oo=opt, n_reads=4, outs=(p, n, po, no)):
        ptr = lambda x: None if x is None else x.ctypes.data
        return L.bwagpu_cigars_flat(hh, None if oo is None else C.byref(oo), n_reads, ptr(seqs), ptr(off), ptr(counts), ptr(regs), *[None if x is None else C.byref(x) for x in outs])

    def rejected(text, **kw):
        assert call(**kw) == -2, kw.keys()
        assert text in L.bwagpu_last_error(h).decode(), (text, L.bwagpu_last_error(h))
        assert call() == 0      # a valid call still works
        got = hostapi.decode_cigars(dev._take(p, n.value, CIGAR_DTYPE), dev._take(po, no.value, np.dtype("<u4")))
        assert got == want

    for kw in (dict(hh=None), dict(oo=None), dict(n_reads=-1), dict(counts=None), dict(off=None), dict(regs=None), dict(seqs=None), dict(outs=(None, n, po, no)), dict(outs=(p, n, None, no))):
        assert call(**kw) == -2, kw.keys()
    bad = counts.copy(); bad[2] = -1
    rejected("negative count", counts=bad)
    lens = np.diff(off)
    for k, f, v, text in ((0, "qb", -1, "qb < 0"), (1, "qe", int(lens[1]) + 1, "qe beyond"), (2, "rb", -1, "rb < 0"), (3, "re", 2 * W.l_pac + 1, "beyond 2 l_pac")):
        bad = regs.copy(); bad[f][k] = v
        rejected(text, regs=bad)
    for f in ("e_del", "e_ins"):
        for v in (0, -1):
            o = default_opt(); setattr(o, f, v)
            rejected("must be positive", oo=o)
    bad = seqs.copy(); bad[7] = 5
    rejected("base code", seqs=bad)
    bad = off.copy(); bad[2] = bad[1] - 1
    rejected("ascend", off=bad)
    # the limits themselves are accepted
    ok = regs.copy(); ok["qb"][0] = 0; ok["qe"][0] = int(lens[0]); ok["rb"][0] = 0; ok["re"][0] = int(lens[0])
    assert call(regs=ok) == 0
    L.bwagpu_free(p); L.bwagpu_free(po)
    # no reads; reads without regions
    assert L.bwagpu_cigars_flat(h, C.byref(opt), 0, None, None, None, None, C.byref(p), C.byref(n), C.byref(po), C.byref(no)) == 0 and n.value == 0 and no.value == 0
    L.bwagpu_free(p); L.bwagpu_free(po)
    cigs, ops = dev.cigars_flat(opt, seqs, off, np.zeros(4, dtype=np.int32), np.zeros(0, dtype=ALNREG_DTYPE))
    assert cigs.shape[0] == 0 and ops.shape[0] == 0


# ---- fixtures and tests -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim():
    import hostsim_build
    w = World(lib_path=hostsim_build.build(), options={"ptab_m": 6})
    yield w
    w.close()


@pytest.fixture(scope="module")
def gpu():
    w = World()
    yield w
    w.close()


def test_limits_and_reference_entry(sim):
    """the limits are the literals the cases are aimed at; bwa_gen_cigar2 is exported and its MD string sits behind the operations"""
    check_limits(sim.dev)
    q = sim.g[1000:1100].copy()
    q[50] = (q[50] + 1) & 3
    t = sim.R.gen(default_opt(), 0, q, 1000, 1100)
    assert t == (95, 1, (100 << 4,), 1, b"50" + b"ACGT"[int(sim.g[1050]):int(sim.g[1050]) + 1] + b"49"), t
    assert sim.R.gen(default_opt(), 10, q, sim.l_pac - 50, sim.l_pac + 50) is None and sim.R.gen(default_opt(), 10, q[:0], 1000, 1100) is None


@pytest.mark.parametrize("seed", GPU_SEEDS)
def test_families_cover_their_boundaries(sim, seed):
    """the full lists of the GPU tests, on the reference's side alone"""
    cover(sim, cases_of(sim, seed, False), truth_of(sim, seed, False, "default", default_opt()), False)


def test_sim_families(sim):
    run_families(sim, SIM_SEED, thin=True)


def test_sim_filter(sim):
    run_filter(sim, SIM_SEED)


def test_sim_non_interference(sim):
    run_non_interference(sim, 6, 96)


def test_sim_error_paths(sim):
    run_error_paths(sim)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", GPU_SEEDS)
def test_gpu_families(gpu, seed):
    run_families(gpu, seed, thin=False)


@pytest.mark.gpu
def test_gpu_operation_array_under_concurrency(gpu):
    run_concurrent(gpu, GPU_SEEDS[0], 4000)


@pytest.mark.gpu
def test_gpu_filter(gpu):
    run_filter(gpu, GPU_SEEDS[1])


@pytest.mark.gpu
def test_gpu_non_interference(gpu):
    run_non_interference(gpu, 400, 96)


@pytest.mark.gpu
def test_gpu_error_paths(gpu):
    run_error_paths(gpu)
