"""A crafted genome and read families for the seeding stage (mem_collect_intv, bwamem.c:140-188), shared by the CPU and GPU tests of
tests/test_seed_stage.py, and a replay of mem_collect_intv that knows nothing of an FM-index.

genome(): three contigs, 18.9 kb.  Contig 1: 2.6 kb of random bases, then the graded family (a 200-base unit and 41 copies of its first 9 .. 156
bases, each between random flanks: a forward sweep from the unit's first base changes its interval size at every one of those lengths).  Contig 2:
the copy-count segments (13 random 60-mers, present 3 .. 21 times each, every copy between 6-base random flanks, the first copy followed by 40
private bases; bases 20 .. 38 of six of them twice more on their own).  Contig 3: tandem arrays of period 1 .. 7 (210 bases each), a 60-base palindrome, and 100 random bases that end the genome (reads
across the junction of the two strands).
batches(): name -> Batch: an option set and its reads.  Eight families (fam_* below); the kernel forms each runs under are test_seed_stage.FORMS,
and what each is aimed at is asserted from the replay alone by test_seed_stage.cover().
replay(): mem_collect_intv with bwt_smem1a and bwt_seed_strategy1 (bwt.c:289-379) over `occ`, the number of occurrences of a string in the genome
followed by its reverse complement (Text: a suffix array by prefix doubling and bisection).  It must reproduce the reference's (info, x2) list of
every read (asserted by the caller), and records where the searches went.

Everything is generated from seeds (one stream per name); the expected intervals come from the compiled reference at test time."""
import bisect
import zlib

import numpy as np

from bwa_amd.structs import default_opt

SEED = 27182
BG = 2600
UNIT = 200
GRADED = (9, 10, 11, 12, 13) + tuple(16 + 4 * j for j in range(36))
FLANK = 6
SEG, EXT = 60, 40
COPY_COUNTS = (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 19, 20, 21)
INNER_IN, INNER = (3, 4, 5, 9, 10, 11), (20, 39)      # the segments of family 4 hold 19 bases that occur twice more on their own
PERIODS, ARRAY, SPACER = (1, 2, 3, 4, 5, 6, 7), 210, 30
LONG_LEN = 1300          # the read that turns a batch of short reads into a long-read batch
IDLE = 1 << 20           # min_chain_weight of the batches that leave the stages after seeding without work


def _rng(name):
    return np.random.default_rng([SEED, zlib.crc32(name.encode())])


def rc(x):
    x = np.asarray(x, dtype=np.uint8)
    return np.ascontiguousarray(np.where(x < 4, 3 - x, 4)[::-1]).astype(np.uint8)


def rnd(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def other(*bases):
    """a base that differs from all the given ones"""
    return np.array([next(b for b in range(4) if b not in [int(x) for x in bases])], dtype=np.uint8)


def substitute(rng, x, mask):
    x = x.copy()
    n = int(mask.sum())
    x[mask] = (x[mask] + rng.integers(1, 4, n).astype(np.uint8)) & 3
    return x


class Layout:
    """where the genome's parts lie (offsets into the concatenated contigs)"""


_genome = None


def genome():
    """-> (codes, contig lengths, Layout)"""
    global _genome
    if _genome is not None:
        return _genome
    rng = _rng("genome")
    lay = Layout()
    # contig 1
    parts = [rnd(rng, BG)]
    pos = BG
    unit = rnd(rng, UNIT)
    lay.unit = pos + FLANK
    parts += [rnd(rng, FLANK), unit, rnd(rng, FLANK)]
    pos += UNIT + 2 * FLANK
    lay.graded = []
    for n in GRADED:          # the unit's first n bases, then a base that is not the unit's next
        lay.graded.append(pos + FLANK)
        parts += [rnd(rng, FLANK), unit[:n], other(unit[n]), rnd(rng, FLANK - 1)]
        pos += n + 2 * FLANK
    c1 = pos
    # contig 2
    lay.seg = {}
    for c in COPY_COUNTS:
        seg = rnd(rng, SEG)
        lay.seg[c] = []
        for k in range(c):
            lay.seg[c].append(pos + FLANK)
            tail = FLANK + (EXT if k == 0 else 0)
            parts += [rnd(rng, FLANK), seg, rnd(rng, tail)]
            pos += SEG + FLANK + tail
        if c in INNER_IN:          # its bases 20 .. 38 twice more: what pass 2 finds when it re-seeds a match around them with min_intv = c + 1
            for k in range(2):
                parts += [rnd(rng, FLANK - 1), other(seg[INNER[0] - 1]), seg[INNER[0]:INNER[1]], other(seg[INNER[1]]), rnd(rng, FLANK - 1)]
                pos += INNER[1] - INNER[0] + 2 * FLANK
    c2 = pos - c1
    # contig 3
    lay.array = {}
    for p in PERIODS:
        while True:
            u = rnd(rng, p)
            if all(not np.array_equal(u, np.roll(u, s)) for s in range(1, p)):      # no shorter period
                break
        parts.append(rnd(rng, SPACER))
        lay.array[p] = pos + SPACER
        parts.append(np.tile(u, ARRAY // p + 1)[:ARRAY])
        pos += SPACER + ARRAY
    x = rnd(rng, 30)
    parts += [rnd(rng, SPACER), x, rc(x), rnd(rng, 100)]
    lay.pal = pos + SPACER
    pos += SPACER + 60 + 100
    g = np.concatenate(parts).astype(np.uint8)
    lens = [c1, c2, pos - c1 - c2]
    assert g.shape[0] == pos == sum(lens) < 20000
    _genome = (g, lens, lay)
    return _genome


# ---- occurrences of a string, without an FM-index -----------------------------------------------------------------------------------------------------------------
class Text:
    """the genome followed by its reverse complement (the text the reference's index is built over: matches across the strands' junction and across contig
    borders count), its suffix array, and the narrowing of a suffix-array range by one more base"""
    def __init__(self, g):
        t = np.concatenate([g, rc(g)]).astype(np.int64)
        n = t.shape[0]
        rank, k = t.copy(), 1
        while True:          # prefix doubling: rank by the first k bases -> by the first 2 k (a suffix that ends sorts first)
            r2 = np.full(n, -1, dtype=np.int64)
            r2[:n - k] = rank[k:]
            order = np.lexsort((r2, rank))
            a, b = rank[order], r2[order]
            new = np.empty(n, dtype=np.int64)
            new[order] = np.cumsum(np.concatenate([[0], (a[1:] != a[:-1]) | (b[1:] != b[:-1])]))
            rank = new
            if int(rank.max()) == n - 1:
                break
            k <<= 1
        self.n = n
        self.sa = np.argsort(rank).tolist()
        self.pad = bytes((t + 1).astype(np.uint8)) + bytes(1 << 12)      # bases as 1 .. 4; 0 past the end (it sorts first)

    def narrow(self, lo, hi, depth, c):
        """the suffixes of [lo, hi) -- which share their first `depth` bases, and are sorted by the next -- whose next base is c"""
        pad, sa, c = self.pad, self.sa, c + 1
        if hi - lo == 1:
            return (lo, hi) if pad[sa[lo] + depth] == c else (lo, lo)
        first, last = pad[sa[lo] + depth], pad[sa[hi - 1] + depth]
        if first == c == last:
            return lo, hi
        if first > c or last < c:
            return lo, lo
        key = lambda p: pad[p + depth]
        lo = bisect.bisect_left(sa, c, lo, hi, key=key)
        return lo, bisect.bisect_right(sa, c, lo, hi, key=key)


_text = None


def text():
    global _text
    if _text is None:
        _text = Text(genome()[0])
    return _text


class Occ:
    """occ(i, e): occurrences of q[i:e) in the text, for one read (a row of sizes per start position, grown on demand)"""
    def __init__(self, T, q):
        self.T, self.q, self.rows = T, q, {}
        self.sweeps = {}      # (x, min_intv) -> (ret, matches, Sweep): a search depends on nothing else, so a read's option sets share them

    def __call__(self, i, e):
        row = self.rows.get(i)
        if row is None:
            row = self.rows[i] = [0, self.T.n, [self.T.n]]      # lo, hi, sizes by length
        sizes = row[2]
        while len(sizes) <= e - i:
            if sizes[-1] == 0:
                return 0
            d = len(sizes) - 1
            c = int(self.q[i + d])
            row[0], row[1] = self.T.narrow(row[0], row[1], d, c) if c < 4 else (0, 0)
            sizes.append(row[1] - row[0])
        return sizes[e - i]


# ---- the replay -----------------------------------------------------------------------------------------------------------------------------------------------
class Sweep:
    __slots__ = ("x", "pass_", "min_intv", "lens", "rows", "grown", "n_ext")      # lens: match lengths at the change points (ascending); rows: backward rows run;
    # grown: lengths that entries surviving a backward row reached; n_ext: extensions (forward steps + backward entries visited)


class Trace:
    __slots__ = ("intv", "sweeps", "p1", "p3", "n_ext", "n_p2")      # intv: sorted (info, x2); n_p2: entries pass 2 added; p1: pass 1's entries in emission order (start, end, x2, qualifies for pass 2);
    # p3: (x2, emitted) at every step at which bwt_seed_strategy1 could decide, up to its decision


def smem1(q, x, min_intv, occ, sw):
    """bwt_smem1a (bwt.c:289-351) with max_intv = 0 -> (ret, [(start, end, x2)] by start)"""
    n = q.shape[0]
    sw.x, sw.min_intv, sw.lens, sw.rows, sw.grown, sw.n_ext = x, min_intv, [], 0, set(), 0
    if q[x] > 3:
        return x + 1, []
    min_intv = max(min_intv, 1)
    curr = []
    ik, end = occ(x, x + 1), x + 1
    i = x + 1
    while i < n:
        if q[i] < 4:
            sw.n_ext += 1
            ok = occ(x, i + 1)
            if ok != ik:
                curr.append((end, ik))
                if ok < min_intv:
                    break
            ik, end = ok, i + 1
        else:
            curr.append((end, ik))
            break
        i += 1
    if i == n:
        curr.append((end, ik))
    sw.lens = [e - x for e, _ in curr]
    curr.reverse()
    ret = curr[0][0]
    prev, mem = curr, []
    for i in range(x - 1, -2, -1):
        c = int(q[i]) if i >= 0 and q[i] < 4 else -1
        curr = []
        for e, s in prev:
            ok = 0
            if c >= 0:
                sw.n_ext += 1
                ok = occ(i, e)
            if c < 0 or ok < min_intv:
                if not curr and (not mem or i + 1 < mem[-1][0]):
                    mem.append((i + 1, e, s))
            elif not curr or ok != curr[-1][1]:
                curr.append((e, ok))
                sw.grown.add(e - i)
        if not curr:
            break
        sw.rows += 1
        prev = curr
    mem.reverse()
    return ret, mem


def replay(opt, read, occ=None):
    """mem_collect_intv (bwamem.c:140-188) -> Trace"""
    q = np.asarray(read, dtype=np.uint8)
    n = q.shape[0]
    occ = occ or Occ(text(), q)
    k = opt.min_seed_len
    split_len = int(k * opt.split_factor + .499)
    t = Trace()
    t.sweeps, t.p1, t.p3 = [], [], []
    out = []

    def search(x, min_intv):
        hit = occ.sweeps.get((x, min_intv))
        if hit is None:
            sw = Sweep(); sw.pass_ = 1 if min_intv == 1 else 2
            hit = occ.sweeps[(x, min_intv)] = smem1(q, x, min_intv, occ, sw) + (sw,)
        t.sweeps.append(hit[2])
        return hit[0], hit[1]

    x = 0
    while x < n:          # pass 1
        if q[x] < 4:
            x, mem = search(x, 1)
            out += [m for m in mem if m[1] - m[0] >= k]
        else:
            x += 1
    old = list(out)
    for s, e, x2 in old:          # pass 2
        qual = not (e - s < split_len or x2 > opt.split_width)
        t.p1.append((s, e, x2, qual))
        if qual:
            _, mem = search((s + e) >> 1, x2 + 1)
            out += [m for m in mem if m[1] - m[0] >= k]
    t.n_p2 = len(out) - len(old)
    n3 = 0
    if opt.max_mem_intv > 0:          # pass 3 (bwt_seed_strategy1, bwt.c:358-379)
        x = 0
        while x < n:
            if q[x] > 3:
                x += 1
                continue
            i, nxt = x + 1, n
            while i < n:
                if q[i] > 3:
                    nxt = i + 1
                    break
                n3 += 1
                ok = occ(x, i + 1)
                if i - x >= k:
                    t.p3.append((ok, ok < opt.max_mem_intv))
                if ok < opt.max_mem_intv and i - x >= k:
                    if ok > 0:
                        out.append((x, i + 1, ok))
                    nxt = i + 1
                    break
                i += 1
            x = nxt
    t.intv = sorted(((s << 32) | e, x2) for s, e, x2 in out)
    t.n_ext = sum(s.n_ext for s in t.sweeps) + n3
    return t


# ---- the families ---------------------------------------------------------------------------------------------------------------------------------------------
class Batch:
    __slots__ = ("name", "fam", "opt", "reads", "tags", "chains", "sim")      # chains: the batch lets chains through (the second check); sim: the reads the mock runtime takes


def seed_opt(k=19, split_factor=1.5, split_width=10, max_mem_intv=20, max_occ=500, idle=True):
    o = default_opt()
    o.min_seed_len, o.split_factor, o.split_width, o.max_mem_intv, o.max_occ = k, split_factor, split_width, max_mem_intv, max_occ
    if idle:
        o.min_chain_weight = IDLE
    return o


def _batch(name, fam, opt, reads, tags, chains=False, sim=None):
    b = Batch()
    b.name, b.fam, b.opt, b.reads, b.tags, b.chains = name, fam, opt, [np.ascontiguousarray(r, dtype=np.uint8) for r in reads], tags, chains
    b.sim = list(range(len(reads))) if sim is None else sim
    assert len(reads) == len(tags)
    return b


class Reads:
    def __init__(self):
        self.reads, self.tags = [], []

    def add(self, r, tag, both=False):
        r = np.ascontiguousarray(r, dtype=np.uint8)
        self.reads.append(r); self.tags.append(tag)
        if both:
            self.reads.append(rc(r)); self.tags.append(tag + " rev")


F1_LENGTHS = (0, 1, 9, 10, 11, 12, 15, 16, 17, 18, 19, 20, 31, 32, 33, 255, 256)      # 0, 1, k - 1 .. k + 1 for k = 10, 11, 19, the 16-base windows, the LDS copy's bound
F1_N_AT = (0, 99, 15, 16, 17)


def lengths_reads(g, lay):
    """family 1's reads (all of at most 256 bases)"""
    rng = _rng("lengths")
    R = Reads()
    L = g.shape[0]
    for j, n in enumerate(F1_LENGTHS):
        s = 40 + 131 * j
        R.add(g[s:s + n], f"{n} bases", both=n in (16, 19, 256))
    for n in (40, 256):
        R.add(np.full(n, 4), f"{n} N")
    for p in F1_N_AT:
        for v in (0, 1):
            x = g[300 + 7 * p + 500 * v:400 + 7 * p + 500 * v]
            x = rc(x) if v else x.copy()
            x[p] = 4
            R.add(x, f"100 bases{' rev' if v else ''}, N at {p}")
    x = g[900:1000].copy(); x[[15, 17]] = 4
    R.add(x, "100 bases, N at 15 and 17")
    x = g[1000:1256].copy(); x[[15, 16, 17, 31, 32, 255]] = 4
    R.add(x, "256 bases, N at 15, 16, 17, 31, 32 and 255")
    for k in (10, 11, 19):          # N runs that leave clean pieces of exactly k - 1 and k bases (and one of k + 1)
        x = g[1300 + k:1300 + k + 5 * k + 40].copy()
        at, cut = 0, []
        for piece, run in ((k - 1, 1), (k, 2), (k - 1, 3), (k + 1, 1), (k, 1)):
            at += piece
            cut += list(range(at, at + run)); at += run
        x[cut] = 4
        R.add(x, f"pieces of {k - 1}, {k}, {k - 1}, {k + 1}, {k} bases between N runs", both=True)
    pal = g[lay.pal:lay.pal + 60]
    assert np.array_equal(pal, rc(pal))
    R.add(pal, "the palindrome")
    R.add(g[lay.pal - 20:lay.pal + 80], "the palindrome and its flanks")
    x = pal.copy(); x[30] = 4
    R.add(x, "the palindrome, N in the middle")
    R.add(np.concatenate([g[L - 40:], rc(g[L - 40:])]), "across the strands' junction (40 + 40 bases)")
    R.add(np.concatenate([g[L - 25:], rc(g[L - 60:])]), "across the strands' junction (25 + 60 bases)")
    c1 = genome()[1][0]
    R.add(g[c1 - 50:c1 + 50], "across the border of contigs 1 and 2", both=True)
    for j in range(24):          # clean reads for the rest of the wavefront
        n = int(rng.integers(60, 251))
        s = int(rng.integers(0, BG - n))
        x = substitute(rng, g[s:s + n], rng.random(n) < 0.02)
        R.add(rc(x) if j % 2 else x, f"{n} bases at {s}, 2 %")
    order = rng.permutation(len(R.reads))          # reads with N and clean reads side by side
    return [R.reads[i] for i in order], [R.tags[i] for i in order]


def long_read(g, n=LONG_LEN, name="long read"):
    """n bases of the first contig's random part with a few substitutions"""
    rng = _rng(name)
    s = int(rng.integers(0, BG - n))
    return substitute(rng, g[s:s + n], rng.random(n) < 0.02)


def fam_lengths(g, lay):
    """1: every read length at which a window, a prefix-table look-up or the length filter changes; N at the windows' borders and at the reads' ends;
    batches of at most 256 bases (the 2-bit LDS copy; its reads with N byte by byte), of 257 and of 1100 (the 4-bit array)"""
    reads, tags = lengths_reads(g, lay)
    assert max(r.shape[0] for r in reads) == 256
    out = []
    for k in (10, 11, 19):
        o = seed_opt(k)
        out.append(_batch(f"lengths -k {k}", 1, o, reads, tags))
        out.append(_batch(f"lengths -k {k}, longest 257", 1, o, reads + [long_read(g, 257, "257")], tags + ["257 bases"], sim=list(range(0, len(reads), 4)) + [len(reads)]))
        out.append(_batch(f"lengths -k {k}, longest 1100", 1, o, reads + [long_read(g, 1100, "1100")], tags + ["1100 bases"], sim=list(range(1, len(reads), 6)) + [len(reads)]))
    return out


def unit_reads(g, lay, R, lengths, tag):
    """the graded unit's first T bases behind an N (a sweep that starts at the unit's first base: change points at 9, 10, 11, ...) and behind 15 bases
    that lead into its first base only (the next sweep starts at its second base, and its first backward row prepends the first: entries of
    8, 9, 10, ... bases grow by one)"""
    u = lay.unit
    z = next(z for z in range(20, BG - 2) if g[z] == g[u] and g[z + 1] != g[u + 1] and g[z - 1] != g[u - 1])
    for T in lengths:
        R.add(np.concatenate([g[500:520], [4], g[u:u + T]]), f"{tag}: N, then the unit's first {T} bases")
        R.add(np.concatenate([g[z - 15:z], g[u:u + T]]), f"{tag}: 15 bases that lead into the unit's first base, then its first {T}")


def fam_depth(g, lay):
    """2: matches around the prefix tables' depth d (10 by default, 7 under option ptab_m = 7): change points at d - 1, d and d + 1 bases, entries that a
    backward row grows to d, reads whose every match is shorter than d; min_seed_len = d (no bit mask) and d + 1 (bit mask)"""
    rng = _rng("depth")
    R = Reads()
    unit_reads(g, lay, R, (12, 20, 30, 60, 100), "depth")
    for j in range(12):          # random reads: matches of up to 8 or 9 bases
        R.add(rnd(rng, 24 + j), f"{24 + j} random bases")
    T, found = text(), 0
    while found < 3:          # reads of 8 .. 10 bases none of whose 7-mers occurs (one 7-mer in ten does not, in 37.8 kb): no match of the shallower tables' depth
        x = rnd(rng, 8 + found)
        occ = Occ(T, x)
        if all(occ(i, i + 7) == 0 for i in range(x.shape[0] - 6)):
            R.add(x, f"{x.shape[0]} bases without a 7-mer of the genome")
            found += 1
    for j in range(20):
        n = 120
        s = int(rng.integers(0, g.shape[0] - n))
        x = substitute(rng, g[s:s + n], rng.random(n) < 0.04)
        R.add(rc(x) if j % 2 else x, f"{n} bases at {s}, 4 %")
    out = []
    for k in (7, 8, 10, 11):
        out.append(_batch(f"depth -k {k}", 2, seed_opt(k, split_factor=1.0), R.reads, R.tags, sim=list(range(0, len(R.reads), 3))))
    return out


def deep_reads(g, lay):
    """family 3's reads: sweeps with as many change points as the LDS ring holds, one more, and three times as many"""
    rng = _rng("deep")
    R = Reads()
    unit_reads(g, lay, R, (18, 22) + tuple(range(30, 46, 2)) + (80, 150, 200), "graded")
    u = lay.unit
    R.add(rc(g[u - FLANK:u + UNIT]), "the graded unit and its left flank, rev")
    for p in PERIODS:
        a = lay.array[p]
        for j, (lo, n) in enumerate(((-20, 150), (30, 170), (ARRAY - 120, 140), (5, 200))):
            x = g[a + lo:a + lo + n]
            if j == 3:
                x = substitute(rng, x, np.arange(n) % 67 == 40)
            R.add(rc(x) if j == 1 else x, f"period {p}: {n} bases from {lo}{', a substitution every 67' if j == 3 else ''}")
    for p in (3, 7):          # pieces of one and two bases between N: sweeps with one and two change points beside the deep ones
        a = lay.array[p]
        x = g[a - 10:a + 190].copy(); x[[50, 52, 120, 123]] = 4
        R.add(x, f"period {p}: 200 bases from -10, N at 50, 52, 120 and 123")
    return R.reads, R.tags


def fam_deep(g, lay):
    """3: the interval stack beyond its LDS ring: the graded unit and the tandem arrays"""
    reads, tags = deep_reads(g, lay)
    assert max(r.shape[0] for r in reads) <= 256
    return [_batch("deep", 3, seed_opt(19), reads, tags, sim=list(range(0, 22, 3)) + list(range(23, len(reads), 5)))]


F4_SPLIT = ((4, 1.5), (10, 1.5), (4, 1.0), (10, 1.0))


def split_reads(g, lay):
    """family 4's reads: for c = 3, 4, 5, 9, 10, 11 copies, a stretch of 18 .. 20 and 27 .. 29 bases of the c-copy segment between bases that no copy has there
    (one pass-1 SMEM of exactly that length with x2 = c), and the first copy with its private extension (a long unique SMEM: pass 2 finds the segment)"""
    rng = _rng("split")
    R = Reads()
    for c in (3, 4, 5, 9, 10, 11):
        s0 = lay.seg[c][0]
        for n in (18, 19, 20, 27, 28, 29):
            for j, a in enumerate((19, 20) if n < 27 else (12, 16)):          # (the longer ones, and 20 bases from 19, hold the 19 bases that occur c + 2 times)
                x = np.concatenate([rnd(rng, 15), other(g[s0 + a - 1]), g[s0 + a:s0 + a + n], other(g[s0 + a + n]), rnd(rng, 15)])
                R.add(rc(x) if j else x, f"{n} bases of the {c}-copy segment from {a}{' rev' if j else ''}")
    for c in COPY_COUNTS:
        s0 = lay.seg[c][0]
        R.add(g[s0:s0 + SEG + EXT - 5], f"the {c}-copy segment with its private extension", both=c in (4, 10))
    return R.reads, R.tags


def many_reads(g, lay):
    """250 random bases: under -k 7 / 8 nearly every position starts a match of that length somewhere in a genome of 37 kb (both strands), so pass 1 leaves
    more than 64 entries, most of them rare enough for pass 2"""
    rng = _rng("many")
    return [rnd(rng, 250) for _ in range(8)], [f"250 random bases ({j})" for j in range(8)]


def fam_split(g, lay):
    """4: pass 2's thresholds (length against split_len, x2 against split_width), and its memory of which of pass 1's entries qualify beyond the 64th"""
    reads, tags = split_reads(g, lay)
    out = [_batch(f"split -y {w} -r {f}", 4, seed_opt(19, f, w), reads, tags, sim=list(range(0, len(reads), 3))) for w, f in F4_SPLIT]
    reads, tags = many_reads(g, lay)
    out += [_batch(f"many -k {k}", 4, seed_opt(k, 1.0, 10), reads, tags, sim=[0, 1] if k == 7 else [2]) for k in (7, 8, 9)]
    return out


def fam_pass3(g, lay):
    """5: bwt_seed_strategy1's threshold: stretches of the 4-, 5-, 6-, 19-, 20- and 21-copy segments under max_mem_intv = 0, 5 and 20"""
    rng = _rng("pass3")
    R = Reads()
    for c in (4, 5, 6, 19, 20, 21):
        for j, (a, n) in enumerate(((0, 45), (8, 50), (3, 57))):
            s0 = lay.seg[c][j % c]
            x = np.concatenate([rnd(rng, 12 + j), other(g[s0 + a - 1]), g[s0 + a:s0 + a + n], rnd(rng, 20)])
            R.add(rc(x) if j == 1 else x, f"{n} bases of the {c}-copy segment from {a}")
        s0 = lay.seg[c][0]
        R.add(g[s0 - FLANK:s0 + SEG + EXT], f"the {c}-copy segment with its flank and private extension")
    for j in range(10):
        s = int(rng.integers(0, BG - 150))
        R.add(substitute(rng, g[s:s + 150], rng.random(150) < 0.03), f"150 bases at {s}, 3 %")
    return [_batch(f"pass 3 -y {m}", 5, seed_opt(19, max_mem_intv=m), R.reads, R.tags, sim=list(range(0, len(R.reads), 2))) for m in (0, 5, 20)]


def task_reads(g, lay, k=19):
    """reads aimed at the pass-1 tasks' positions g = j k: N on and next to them, and matches that start exactly at g - k + 1 and at g"""
    rng = _rng("tasks")
    R = Reads()
    for j, at in enumerate((k - 1, k, k + 1, 3 * k - 1, 3 * k, 3 * k + 1)):
        s = 200 + 160 * j
        x = g[s:s + 150].copy(); x[at] = 4
        R.add(x, f"150 bases, N at {at}")
    x = g[1200:1350].copy(); x[[2 * k, 4 * k, 4 * k + 1, 6 * k - 1]] = 4
    R.add(x, f"150 bases, N at {2 * k}, {4 * k}, {4 * k + 1} and {6 * k - 1}")
    for j, p in enumerate((2 * k - k + 1, 2 * k, 3 * k - k + 1, 3 * k, 2 * k - k, 2 * k + 1)):
        s = 1400 + 150 * j
        x = np.concatenate([rnd(rng, p - 1), other(g[s + p - 1]), g[s + p:s + 120]])
        R.add(rc(x) if j % 2 else x, f"120 bases, exact from {p}" if j % 2 == 0 else f"120 bases, exact to {120 - p}, rev")
    return R.reads, R.tags


def fam_heavy(g, lay):
    """6: reads given up by the lane-per-read kernel and seeded by tasks: families 3 and 4 again, and reads aimed at the tasks' positions"""
    r3, t3 = deep_reads(g, lay)
    r4, t4 = split_reads(g, lay)
    rm, tm = many_reads(g, lay)
    rt, tt = task_reads(g, lay)
    reads, tags = r3 + r4 + rm + rt, t3 + t4 + tm + tt
    n3 = len(r3)
    sim = list(range(0, n3, 7)) + list(range(n3, len(reads) - len(rt), 9)) + list(range(len(reads) - len(rt), len(reads), 2))
    sim = sorted(set(sim) | {i for i, t in enumerate(tags) if "of the 10-copy segment" in t})      # (x2 = split_width: k_seed_p2_tasks' threshold)
    return [_batch("heavy", 6, seed_opt(19, 1.5, 10), reads, tags, sim=sim), _batch("heavy -k 8 -r 1", 6, seed_opt(8, 1.0, 10), reads, tags, sim=sim[1::3])]


def fam_long(g, lay):
    """7: long-read batches: families 1 and 3 with a read of 1300 bases appended, and one of 1700 random bases (some 300 intervals under -k 8)"""
    r1, t1 = lengths_reads(g, lay)
    r3, t3 = deep_reads(g, lay)
    extra, etags = [long_read(g), rnd(_rng("long random"), 1700)], ["1300 bases", "1700 random bases"]
    out = []
    deep = [i for i, t in enumerate(t3) if t.startswith("graded: N, then the unit's first 150")]      # (a sweep that fills a task's stack of two entries in this batch too)
    out.append(_batch("long, lengths -k 19", 7, seed_opt(19), r1 + [r3[i] for i in deep] + extra, t1 + [t3[i] for i in deep] + etags, sim=list(range(0, len(r1), 8)) + [len(r1), len(r1) + 1]))
    for k in (19, 8):
        out.append(_batch(f"long, deep -k {k}", 7, seed_opt(k), r3 + extra, t3 + etags, sim=deep + [40, len(r3)] + ([len(r3) + 1] if k == 8 else [])))
    return out


F8_COPIES = (3, 4, 5, 7, 8, 9, 11, 12)


def fam_publish(g, lay):
    """8: the SA rows mem_chain takes from an interval (step = x2 / max_occ, at most max_occ rows): x2 = 3 .. 12 under max_occ = 4 and the default;
    these batches let chains through"""
    rng = _rng("publish")
    R = Reads()
    for c in F8_COPIES:
        for j, (a, n) in enumerate(((2, 50), (6, 40))):
            s0 = lay.seg[c][(j + 1) % c]
            x = np.concatenate([rnd(rng, 20), other(g[s0 + a - 1]), g[s0 + a:s0 + a + n], other(g[s0 + a + n]), rnd(rng, 20)])
            R.add(rc(x) if j else x, f"{n} bases of the {c}-copy segment from {a}{' rev' if j else ''}")
        s0 = lay.seg[c][0]
        R.add(g[s0 - FLANK:s0 + SEG + EXT], f"the {c}-copy segment with its flank and private extension")
    for p in (3, 5):
        a = lay.array[p]
        R.add(g[a + 10:a + 110], f"period {p}: 100 bases")
    for j in range(6):
        s = int(rng.integers(0, BG - 150))
        R.add(substitute(rng, g[s:s + 150], rng.random(150) < 0.02), f"150 bases at {s}, 2 %")
    return [_batch(f"publish -c {m}", 8, seed_opt(19, max_occ=m, idle=False), R.reads, R.tags, chains=True, sim=list(range(0, len(R.reads), 3))) for m in (4, 500)]


_batches = None


def batches():
    global _batches
    if _batches is None:
        g, _, lay = genome()
        _batches = {b.name: b for f in (fam_lengths, fam_depth, fam_deep, fam_split, fam_pass3, fam_heavy, fam_long, fam_publish) for b in f(g, lay)}
    return _batches
