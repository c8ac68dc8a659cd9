"""A crafted genome and read families for the extension stage (mem_chain2aln, bwamem.c:658-812), shared by the CPU and GPU tests of
tests/test_extend_stage.py, and a replay of mem_chain2aln's skip decisions over the reference's own chains and raw regions.

genome(): four contigs, 15.8 kb: 9.3 kb of random bases (the island reads' source; an 8.4 kb read fits), a contig of 400 bases, an 80-copy array of a
37-base unit (each copy 4 % diverged) between random flanks, 2.5 kb of random bases.
batches(): name -> Batch: an option set, its reads and the kernel forms that can take them.  Six families (fam_* below); what each is aimed at is
asserted from the reference's output alone by test_extend_stage.cover().
replay(): the classifier (never a checker): which seeds of a chain the reference skipped, extended although covered, or extended.

Everything is generated from seeds (one stream per name); the expected regions come from the compiled reference at test time."""
import zlib

import numpy as np

from bwa_amd.structs import default_opt, fill_scmat

SEED = 31415
CONTIGS = (9300, 400, 3560, 2500)
UNIT, COPIES, FLANK = 37, 80, 300
LONG_LEN = 1200          # the read that turns a batch of short reads into a long-read batch


def _rng(name):
    return np.random.default_rng([SEED, zlib.crc32(name.encode())])


def rc(x):
    x = np.asarray(x, dtype=np.uint8)
    return np.ascontiguousarray(np.where(x < 4, 3 - x, 4)[::-1]).astype(np.uint8)


def substitute(rng, x, mask):
    """x with every base under the mask replaced by a different one"""
    x = x.copy()
    n = int(mask.sum())
    x[mask] = (x[mask] + rng.integers(1, 4, n).astype(np.uint8)) & 3
    return x


def genome():
    """-> (codes, contig lengths)"""
    rng = _rng("genome")
    unit = rng.integers(0, 4, UNIT).astype(np.uint8)
    arr = np.tile(unit, COPIES)
    arr = substitute(rng, arr, rng.random(arr.shape[0]) < 0.04)
    parts = [rng.integers(0, 4, CONTIGS[0]), rng.integers(0, 4, CONTIGS[1]),
             np.concatenate([rng.integers(0, 4, FLANK), arr, rng.integers(0, 4, FLANK)]), rng.integers(0, 4, CONTIGS[3])]
    g = np.concatenate(parts).astype(np.uint8)
    assert [len(p) for p in parts] == list(CONTIGS) and g.shape[0] < 20000
    return g, list(CONTIGS)


def ctg_off(k):
    return sum(CONTIGS[:k])


class Batch:
    __slots__ = ("name", "fam", "opt", "reads", "tags", "forms", "sim")      # forms: of "short", "ring", "lane"; sim: the reads the mock runtime takes (indices)


def island_opt(k, mcw):
    o = default_opt()
    o.min_seed_len, o.b, o.o_del, o.o_ins, o.min_chain_weight = k, 9, 40, 40, mcw
    o.max_chain_gap = 16      # the islands are 3 .. 6 bases apart: they still chain, and the stage after this one tries to join neighbours only, not every pair of a read's regions
    fill_scmat(o)
    return o


def islands(rng, x, match, sub):
    """x with `sub` substituted bases after every `match`"""
    return substitute(rng, x, (np.arange(x.shape[0]) % (match + sub)) >= match)


def fam_islands_short(g):
    """1: copies of the genome of up to 1100 bases in which every 12 (11) bases are followed by 3 (4) substituted ones: one chain whose seeds -- one per island --
    are nearly all extended (a mismatch costs 9, a gap 40: no extension crosses to the next island); lengths at which the chain has about 31 .. 33, 63 .. 65 seeds"""
    out = []
    for name, match, sub, k, full in (("12+3", 12, 3, 11, 1100), ("12+4", 12, 4, 10, 1100), ("11+3", 11, 3, 10, 1090)):
        rng = _rng("islands " + name)
        b = Batch()
        b.name, b.fam, b.opt, b.reads, b.tags, b.forms = "islands " + name, 1, island_opt(k, 60), [], [], ("short", "ring", "lane")
        per = match + sub
        lens = [full, full] + [n * per - sub for n in ((31, 32, 33, 34, 63, 64, 65, 66, 67) if name == "12+3" else (32, 33, 65))]
        for i, n in enumerate(lens):
            s = 1500 + 97 * i
            r = islands(rng, g[s:s + n], match, sub)
            b.reads.append(rc(r) if i % 2 else r)
            b.tags.append(f"{name} {n} bases{' rev' if i % 2 else ''}")
        b.sim = list(range(len(b.reads)))
        out.append(b)
    return out


def fam_islands_ring(g):
    """2: an 8400-base read, 53 matching bases followed by 6 substituted ones: one chain with more than 128 extended seeds (the ring form's list)"""
    rng = _rng("islands ring")
    b = Batch()
    b.name, b.fam, b.opt, b.forms = "islands 53+6", 2, island_opt(19, 0), ("ring", "lane")
    r = islands(rng, g[600:9000], 53, 6)
    b.reads, b.tags, b.sim = [r, rc(islands(rng, g[450:8850], 53, 6))], ["53+6 8400 bases", "53+6 8400 bases rev"], [0]
    return [b]


def tandem_opt():
    o = default_opt()
    o.min_seed_len, o.max_occ, o.mask_level, o.drop_ratio, o.max_chain_gap = 10, 2000, 0.5, 0.1, 10000
    return o


def fam_tandem(g):
    """3: reads of 100 .. 250 bases from the tandem array at 0 .. 5 % substitutions, both strands: dozens of raw regions per read, most seeds covered by an earlier
    region, many of them with an overlapping seed on another diagonal"""
    out = []
    a0 = ctg_off(2) + FLANK
    for name, opt in (("tandem -k 10", tandem_opt()), ("tandem default", default_opt())):
        rng = _rng("tandem")
        b = Batch()
        b.name, b.fam, b.opt, b.reads, b.tags, b.forms = name, 3, opt, [], [], ("short", "ring", "lane")
        for i in range(60):
            n = int(rng.integers(100, 251))
            s = int(rng.integers(a0 - 40, a0 + UNIT * COPIES + 40 - n))
            r = substitute(rng, g[s:s + n], rng.random(n) < (i % 6) * 0.01)
            b.reads.append(rc(r) if i % 2 else r)
            b.tags.append(f"tandem {n} bases at {s}, {i % 6} %{' rev' if i % 2 else ''}")
        b.sim = list(range(0, 60, 6)) + [1, 3] if name == "tandem -k 10" else [0, 7, 14]
        out.append(b)
    return out


def fam_band(g):
    """4: 150-base reads with one deletion or insertion of 0.6 w .. 1.5 w bases 30 .. 50 bases from an end, for w = 10, 20, 50: max_off on both sides of
    3/4 w, so that the second try with the doubled band runs for some and not for others"""
    out = []
    for w in (10, 20, 50):
        rng = _rng(f"band {w}")
        o = default_opt()
        o.w = w
        b = Batch()
        b.name, b.fam, b.opt, b.reads, b.tags, b.forms = f"band w {w}", 4, o, [], [], ("short", "ring", "lane")
        for i in range(60):
            d = int(rng.integers(round(0.6 * w), round(1.5 * w) + 1))
            near = int(rng.integers(30, 51))
            kind = "DI"[i % 2]
            left = (i >> 1) % 2 == 0
            nq = 150 - (d if kind == "I" else 0)          # bases of the read that come from the genome
            a = near if left else nq - near
            s = int(rng.integers(ctg_off(3) + 100, ctg_off(3) + CONTIGS[3] - 400))
            if kind == "D":
                r = np.concatenate([g[s:s + a], g[s + a + d:s + d + nq]])
            else:
                r = np.concatenate([g[s:s + a], rng.integers(0, 4, d).astype(np.uint8), g[s + a:s + nq]])
            assert r.shape[0] == 150
            rev = (i >> 2) % 2 == 1
            b.reads.append(rc(r) if rev else r)
            b.tags.append(f"w {w}: {kind}{d} {near} bases from the {'left' if left else 'right'} end{' rev' if rev else ''}")
        b.sim = list(range(60))
        out.append(b)
    # the second try for an extension k_ext_pack could have answered (a query of at most w + 1 bases): with gaps at 1 + 1 per base a deletion of 7 .. 9 bases 10 or
    # 11 bases from an end pays, and max_off is then beyond 3/4 w
    rng = _rng("band pack")
    o = default_opt()
    o.w, o.o_del, o.o_ins = 10, 1, 1
    b = Batch()
    b.name, b.fam, b.opt, b.reads, b.tags, b.forms = "band pack", 4, o, [], [], ("short", "ring", "lane")
    for i in range(32):
        d, t = (7, 8, 9, 7)[i % 4], (10, 11, 11, 11)[i % 4]
        s = int(rng.integers(ctg_off(3) + 100, ctg_off(3) + CONTIGS[3] - 400))
        left = (i >> 2) % 2 == 0
        r = np.concatenate([g[s:s + t], g[s + t + d:s + d + 150]]) if left else np.concatenate([g[s:s + 150 - t], g[s + 150 - t + d:s + 150 + d]])
        assert r.shape[0] == 150
        rev = (i >> 3) % 2 == 1
        b.reads.append(rc(r) if rev else r)
        b.tags.append(f"pack: D{d} {t} bases from the {'left' if left else 'right'} end{' rev' if rev else ''}")
    b.sim = list(range(32))
    out.append(b)
    return out


def clip_opts():
    a, b = default_opt(), default_opt()
    a.pen_clip5, a.pen_clip3 = 0, 9
    b.pen_clip5, b.pen_clip3 = 9, 0
    return (("edges default", default_opt()), ("edges clip 0/9", a), ("edges clip 9/0", b))


def edge_reads(g):
    """-> (reads, tags)"""
    rng = _rng("edges")
    L = g.shape[0]
    reads, tags = [], []

    def add(r, tag, both=True):
        r = np.ascontiguousarray(r, dtype=np.uint8)
        reads.append(r); tags.append(tag)
        if both:
            reads.append(rc(r)); tags.append(tag + " rev")

    rnd = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    for k, n in enumerate(CONTIGS):      # hanging over either end of every contig, with random bases and with the neighbour's
        o = ctg_off(k)
        for h in (5, 40, 120):
            add(np.concatenate([rnd(h), g[o:o + 150 - h]]), f"contig {k}: {h} random bases over its start")
            add(np.concatenate([g[o + n - (150 - h):o + n], rnd(h)]), f"contig {k}: {h} random bases over its end")
        if k:
            for h in (50, 75, 100):
                add(g[o - h:o - h + 150], f"across the boundary {k - 1} | {k}, {h} bases before it")
    for m in (0, 1, 3):                  # position 0 and the last base of the last contig (the 0, l_pac and 2 l_pac clamps)
        a, z = g[:150].copy(), g[L - 150:].copy()
        for j in range(m):
            a[20 + 45 * j] ^= 1; z[129 - 45 * j] ^= 1
        add(a, f"position 0, {m} mismatches"); add(z, f"the last base, {m} mismatches")
    c1 = g[ctg_off(1):ctg_off(2)]
    add(c1, "the contig of 400 bases"); add(np.concatenate([rnd(20), c1, rnd(20)]), "the contig of 400 bases and 20 random bases on either side")
    add(substitute(rng, c1, np.arange(400) % 50 == 25), "the contig of 400 bases, a substitution every 50")
    for j in range(4):                   # the best seed starts at base 0 / ends at the last base: no left / no right extension
        s = int(rng.integers(200, 9000))
        x = g[s:s + 150]
        noisy = substitute(rng, x, np.arange(150) % 12 == 5)
        add(np.concatenate([x[:80], noisy[80:]]), f"exact to base 80 ({j})"); add(np.concatenate([noisy[:70], x[70:]]), f"exact from base 70 ({j})")
        add(x, f"exact ({j})")
    for j in range(24):                  # one to three mismatches within 12 bases of either end: to the end or clipped, as pen_clip decides
        s = int(rng.integers(200, 9000))
        x = g[s:s + 150].copy()
        for end in (0, 1):
            m = int(rng.integers(1, 4))
            pos = rng.choice(12, m, replace=False) + 1
            for p in pos:
                q = int(p) if end == 0 else 149 - int(p)
                x[q] = (x[q] + 1 + (j % 3)) & 3
        add(x, f"mismatches near both ends ({j})", both=(j % 2 == 0))
    for j in range(6):                   # N inside an extension
        s = int(rng.integers(ctg_off(3) + 10, ctg_off(3) + 2000))
        x = g[s:s + 150].copy()
        x[[15 + j, 16 + j, 120 + 3 * j]] = 4
        x[60] ^= 2
        add(x, f"N in both extensions ({j})")
    return reads, tags


def bonus_reads(g):
    """150-base reads with a deletion of d = t + 1 bases t = 6 .. 9 bases from an end: with gaps at 1 + 1 per base, w = 10 and pen_clip = 9 at that end the alignment to
    the read's end wins (its score is within 9 of the clipped one), and its path lies outside the band unless pen_clip, as ksw_extend2's end bonus, has widened the
    band's limit from the query's length to nine more"""
    rng = _rng("bonus")
    reads, tags = [], []
    for i in range(24):
        t = 6 + (i // 4 + 2 * (i % 4)) % 4      # the deletion is one base longer than the query left of it: outside a band of t, and at -2 the best way to the end
        d = t + 1
        s = int(rng.integers(ctg_off(3) + 100, ctg_off(3) + CONTIGS[3] - 400))
        left = (i >> 1) % 2 == 0
        r = np.concatenate([g[s:s + t], g[s + t + d:s + d + 150]]) if left else np.concatenate([g[s:s + 150 - t], g[s + 150 - t + d:s + 150 + d]])
        r = r.copy()
        r[100 if left else 49] ^= 1      # a second seed in the chain: the window then reaches 2 w beyond the read's end on the diagonal, not only cal_max_gap of the t bases
        rev = i % 2 == 1
        reads.append(rc(r) if rev else r)
        tags.append(f"bonus: D{d} {t} bases from the {'left' if left != rev else 'right'} end{' rev' if rev else ''}")
    return reads, tags


def fam_edges(g):
    """5: reads at and over the ends of every contig, across contig boundaries, at position 0 and at the last base, on a contig of 400 bases, reads whose
    best seed touches an end of the read, mismatches near the ends (under pen_clip5 != pen_clip3 in both orders), N bases"""
    reads, tags = edge_reads(g)
    out = []
    for name, opt in clip_opts():
        b = Batch()
        b.name, b.fam, b.opt, b.reads, b.tags, b.forms = name, 5, opt, reads, tags, ("short", "ring", "lane")
        b.sim = list(range(len(reads)))
        out.append(b)
    reads, tags = bonus_reads(g)
    for name, (c5, c3) in (("bonus clip 0/9", (0, 9)), ("bonus clip 9/0", (9, 0))):
        b = Batch()
        o = default_opt()
        o.w, o.o_del, o.o_ins, o.pen_clip5, o.pen_clip3 = 10, 1, 1, c5, c3
        b.name, b.fam, b.opt, b.reads, b.tags, b.forms = name, 5, o, reads, tags, ("short", "ring", "lane")
        b.sim = list(range(len(reads)))
        out.append(b)
    return out


def _islands_13_2(rng, R, n):
    """n islands of 13 matching bases, each followed by 2 substituted ones, over R[:15 n]"""
    return islands(rng, R[:15 * n], 13, 2)


def witness_late(g, rng, n):
    """n islands of 13 bases, then A (12 bases), a substituted base, B (11 bases), C (10 bases), where C continues B's last two bases d bases further on in the
    reference: the seed t = B[9:] + C (12 bases) lies on another diagonal.  With scores equal to lengths the order is the islands, t, A, B; A's region
    crosses the substituted base and covers B, and t -- extended after the islands -- is B's only witness under the "other diagonal" rule"""
    for s0 in range(300, 3000):
        Q0 = 15 * n
        r = s0 + Q0
        for d in range(1, 15):
            if (np.array_equal(g[r + 22 + d:r + 24 + d], g[r + 22:r + 24]) and g[r + 24 + d] != g[r + 24] and g[r + 21 + d] != g[r + 21]):
                q = _islands_13_2(rng, g[s0:], n)
                sec = g[r:r + 24].copy()
                sec[12] = (sec[12] + 1) & 3
                end = np.array([next(b for b in range(4) if b != g[r + 34] and b != g[r + 34 + d])] * 3, dtype=np.uint8)
                return np.concatenate([q, sec, g[r + 24 + d:r + 34 + d], end]), f"late witness: {n} islands, d {d}, at {s0}"
    raise AssertionError("no place for the section")


def witness_factor(g, rng, n):
    """n islands of 13 bases, 35 more substituted bases, then C (8 bases), B (11 bases), a substituted base, A (10 bases) and three substituted bases at the
    read's end, where C precedes B's first two bases d bases back in the reference: the seed t = C + B[:2] (10 bases) lies on another diagonal.  With
    mem_seed_sw's scores (min_chain_weight = 1) t's window holds the whole last island (13) and B's and A's only the joint A + B (12), so the order is
    the islands and t, A, B; A's region covers B, and t is B's only candidate witness: 10 bases against .95 * 11 = 10.45 and .9 * 11 = 9.9"""
    for s0 in range(300, 3000):
        T = 15 * (n - 1) + 50
        r = s0 + T
        for d in range(-14, 0):
            if (np.array_equal(g[r + d + 8:r + d + 10], g[r + 8:r + 10]) and g[r + d + 10] != g[r + 10] and g[r + d + 7] != g[r + 7]):
                q = _islands_13_2(rng, g[s0:], n)
                spacer = substitute(rng, g[s0 + 15 * n:r], np.ones(r - s0 - 15 * n, dtype=bool))
                spacer[-1] = next(b for b in range(4) if b != g[r - 1] and b != g[r + d - 1])
                sec = g[r + 8:r + 33].copy()      # B, x, A, three more
                sec[11] = (sec[11] + 1) & 3
                sec[22:25] = (sec[22:25] + 2) & 3
                return np.concatenate([q, spacer, g[r + d:r + d + 8], sec]), f"factor witness: {n} islands, d {d}, at {s0}"
    raise AssertionError("no place for the section")


def fam_witness(g):
    """6: reads on which the "other diagonal" rule hangs on one seed: the 67th extended seed of its chain (beyond the short-read form's 64 registers), and a
    seed of 10 bases against a covered one of 11 -- between .9 and .95 of it -- decided with some 20 and with some 70 seeds extended (registers / the walk)"""
    a, b = Batch(), Batch()
    a.name, a.fam, a.opt, a.forms = "witness late", 6, island_opt(10, 60), ("short", "ring", "lane")
    a.reads, a.tags = map(list, zip(*[witness_late(g, _rng("witness"), n) for n in (65, 68)]))
    b.name, b.fam, b.opt, b.forms = "witness factor", 6, island_opt(10, 1), ("short", "ring", "lane")
    b.opt.max_chain_gap = 64      # (the 37 substituted bases in front of the section stay inside the chain)
    b.reads, b.tags = map(list, zip(*[witness_factor(g, _rng("witness"), n) for n in (19, 24, 66, 68)]))
    for x in (a, b):
        x.sim = list(range(len(x.reads)))
    return [a, b]


def long_read(g):
    """1200 bases of the first contig with a few substitutions and one deletion"""
    rng = _rng("long read")
    x = g[4000:4000 + LONG_LEN + 7]
    x = substitute(rng, x, rng.random(x.shape[0]) < 0.01)
    return np.ascontiguousarray(np.concatenate([x[:500], x[507:]]))


_batches = None


def batches():
    global _batches
    if _batches is None:
        g, _ = genome()
        _batches = {b.name: b for f in (fam_islands_short, fam_islands_ring, fam_tandem, fam_band, fam_edges, fam_witness) for b in f(g)}
    return _batches


# ---- the replay -----------------------------------------------------------------------------------------------------------------------------------------------
def cal_max_gap(opt, qlen):
    """bwamem.c:647-654"""
    l_del = int((qlen * opt.a - opt.o_del) / opt.e_del + 1.)
    l_ins = int((qlen * opt.a - opt.o_ins) / opt.e_ins + 1.)
    l = max(l_del, l_ins, 1)
    return min(l, opt.w << 1)


def window(opt, l_query, seeds, l_pac):
    """bwamem.c:669-683 over a chain's seeds -> (rmax0, rmax1) before any clamp, and after the clamps at 0, 2 l_pac and l_pac"""
    b = min(int(t["rbeg"]) - (int(t["qbeg"]) + cal_max_gap(opt, int(t["qbeg"]))) for t in seeds)
    e = max(int(t["rbeg"]) + int(t["len"]) + (l_query - int(t["qbeg"]) - int(t["len"])) + cal_max_gap(opt, l_query - int(t["qbeg"]) - int(t["len"])) for t in seeds)
    r0, r1 = max(b, 0), min(e, l_pac << 1)
    if r0 < l_pac < r1:
        if int(seeds[0]["rbeg"]) < l_pac:
            r1 = l_pac
        else:
            r0 = l_pac
    return (b, e), (r0, r1)


def replay(opt, l_query, hdr, seeds, regs, info=None):
    """bwamem.c:684-732 over the reference's chains (after mem_flt_chained_seeds) and its raw regions: for every chain, in the order the seeds are processed,
    (index into the chain's seeds, decision, position in the read's region list or -1) with decision 0 skipped, 1 extended although covered, 2 extended.
    Consumes the regions exactly: an extended seed's region has its length as seedlen0, and none is left over (asserted).
    info (a list): for every covered seed, (seeds of its chain extended before it, would .9 in place of .95 decide otherwise, would the chain's first 64 / first
    128 extended seeds alone decide otherwise) is appended."""
    out = []
    n_av = 0
    ks = 0
    P = {f: regs[f].astype(np.int64) for f in ("rb", "re", "qb", "qe", "w", "seedlen0")}
    for c in hdr:
        n = int(c["n"])
        sd = seeds[ks:ks + n]
        ks += n
        qb, ln, rb, sc = (sd[f].astype(np.int64) for f in ("qbeg", "len", "rbeg", "score"))
        order = np.argsort((sc << 32) | np.arange(n), kind="stable")      # the keys are distinct
        oq, ol, orb = qb[order], ln[order], rb[order]
        alive = np.ones(n, dtype=bool)      # srt[] != 0, by position in the sorted order
        rank = np.full(n, 1 << 30)          # the how-manieth extended seed of the chain, by position in the sorted order
        n_ext = 0
        dec = []
        for k in range(n - 1, -1, -1):
            i = int(order[k])
            s_q, s_l, s_r = int(qb[i]), int(ln[i]), int(rb[i])
            covered = False
            inside = ~((s_r < P["rb"][:n_av]) | (s_r + s_l > P["re"][:n_av]) | (s_q < P["qb"][:n_av]) | (s_q + s_l > P["qe"][:n_av])) & ~(s_l - P["seedlen0"][:n_av] > .1 * l_query)
            for j in np.nonzero(inside)[0]:      # (an existence query: the order of the scan does not matter)
                p_rb, p_re, p_qb, p_qe, p_w = (int(P[f][j]) for f in ("rb", "re", "qb", "qe", "w"))
                qd, rd = s_q - p_qb, s_r - p_rb
                w = min(cal_max_gap(opt, min(qd, rd)), p_w)
                if qd - rd < w and rd - qd < w:
                    covered = True
                    break
                qd, rd = p_qe - (s_q + s_l), p_re - (s_r + s_l)
                w = min(cal_max_gap(opt, min(qd, rd)), p_w)
                if qd - rd < w and rd - qd < w:
                    covered = True
                    break
            if covered:
                t_q, t_l, t_r = oq[k + 1:], ol[k + 1:], orb[k + 1:]
                long_enough = alive[k + 1:] & ~(t_l < s_l * .95)
                hit = ((s_q <= t_q) & (s_q + s_l - t_q >= s_l >> 2) & (t_q - s_q != t_r - s_r)) | ((t_q <= s_q) & (t_q + t_l - s_q >= s_l >> 2) & (s_q - t_q != s_r - t_r))
                other = bool((long_enough & hit).any())
                if info is not None:
                    info.append((n_ext, bool((alive[k + 1:] & ~(t_l < s_l * .9) & hit).any()) != other) + tuple(bool((long_enough & hit & (rank[k + 1:] < m)).any()) != other for m in (64, 128)))
                if not other:
                    alive[k] = False
                    dec.append((i, 0, -1))
                    continue
            assert n_av < regs.shape[0] and int(regs["seedlen0"][n_av]) == s_l, "the replay lost step with the reference's regions"
            dec.append((i, 1 if covered else 2, n_av))
            rank[k] = n_ext
            n_ext += 1
            n_av += 1
        out.append(dec)
    assert n_av == regs.shape[0], "regions left over after the replay"
    return out
