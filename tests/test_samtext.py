"""Single-end SAM text written on the device (bwagpu_batch_sam, bwagpu_sam_flat; bwa_amd/csrc/dev_samtext.h) against the compiled reference's text
(refapi.RefIndex.regs2sam: mem_reg2sam of arbitrary lists), byte for byte.

1. a fuzz of bwagpu_sam_flat over test_alns' crafted lists (0 .. 2500 regions, all families and ALT modes) under every option set, with qualities and without;
   the set of declined reads must EQUAL the one computed here from the rule (a printed region, or one listed in a printed XA, without a CIGAR record);
2. the writer's boundaries: read and name lengths around the wavefront width and the staging area, a 10 kb read, lines longer than the staging area;
3. pa:f: -- exact ties of the third decimal in both directions, quotients no double holds;
4. real batches: upload -> run -> download -> cigars -> sam(opt, id0), and that the call leaves bwagpu_batch_alns / bwagpu_batch_cigars alone;
5. error paths.
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
from bwa_amd.api import CIGAR_DTYPE, BwaGpu, BwaGpuError
from bwa_amd.structs import ALN_NOCIGAR, ALNREG_DTYPE, SamIn, SamOut
from test_alns import F_ALL, F_NO_MULTI, F_PRIMARY5, F_SOFTCLIP, LANE_MAX, SIZES, World, fuzz_cells, make_read, opt_variants
from test_primary import batch_reads, ref_opt

pytestmark = pytest.mark.skipif(not refapi.have_ref(), reason="oracle/_ref not built")

F_XB = 0x2000
STAGING, STEP = 512, 64      # bytes of a wavefront's staging area, places of a list per step (dev_samtext.h); checked against the library under test


def check_limits(dev):
    assert dev.sam_limits() == dict(staging=STAGING, step=STEP), "a switch point of the library moved: aim the cases at it"


def sam_variants():
    out = opt_variants()
    for name, kw in (("XB", dict(flag=F_XB)), ("xa1/3", dict(max_XA_hits=1, max_XA_hits_alt=3))):
        o = ref_opt()
        for k, v in kw.items():
            setattr(o, k, v)
        out.append((name, o))
    return out


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------------------
def ref_marked(opt, counts, regs, ids):
    """the lists as mem_mark_primary_se leaves them, with every region's index in its list as given in seedlen0"""
    L = refapi.lib()
    L.mem_mark_primary_se.restype = C.c_int
    L.mem_mark_primary_se.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    a = np.ascontiguousarray(regs, dtype=ALNREG_DTYPE).copy()
    lo = 0
    for i, c in enumerate(counts):
        c = int(c)
        a["seedlen0"][lo:lo + c] = np.arange(c)
        L.mem_mark_primary_se(C.byref(opt), c, a.ctypes.data + lo * ALNREG_DTYPE.itemsize, int(ids[i]))
        lo += c
    return a


def xa_of(opt, a, k):
    """(places listed in the XA of place k of the marked list a, shown: the hit limits let the string through) -- mem_gen_alt's rule"""
    ratio = float(opt.XA_drop_ratio)      # (the float's value as a double: an int against an int * double product)
    listed = np.nonzero((a["secondary_all"] == k) & (a["score"] >= int(a["score"][k]) * ratio))[0]
    cnt = listed.shape[0]
    has_alt = bool(((a["ncomp_isalt"][listed] >> 30) & 1).any())
    return listed, cnt > 0 and not (cnt > opt.max_XA_hits_alt or (not has_alt and cnt > opt.max_XA_hits))


def expect_declined(opt, counts, marked, sel, cigs):
    """the rule of the header: read i is declined iff a printed region (sel >= 0) or a region listed in the shown XA of a printed region has n_cigar == -1;
    -> (declined bool[n], suppressed: reads with an XA the hit limits held back, far: reads with a shown XA entry past place 64)"""
    n = counts.shape[0]
    dec = np.zeros(n, dtype=bool); suppressed = np.zeros(n, dtype=bool); far = np.zeros(n, dtype=bool)
    lo = 0
    for i in range(n):
        c = int(counts[i])
        a, s = marked[lo:lo + c], sel[lo:lo + c]
        nocig = cigs["n_cigar"][lo + a["seedlen0"]] == -1
        printed = np.nonzero(s >= 0)[0]
        dec[i] = bool(nocig[printed].any())
        if not opt.flag & F_ALL:
            for k in printed:
                listed, shown = xa_of(opt, a, int(k))
                if shown:
                    dec[i] |= bool(nocig[listed].any())
                    far[i] |= bool((listed >= 64).any())
                elif listed.shape[0]:
                    suppressed[i] = True
        lo += c
    return dec, suppressed, far


def ref_lines(idx, opt, names, seqs, quals, off, counts, regs, id0):
    """the reference's text, cut per read (the reads' names are distinct and contain no tab)"""
    sam = idx.regs2sam(opt, names, np.ascontiguousarray(seqs).tobytes(), quals, off, counts, regs, n_processed=int(id0))
    out = {nm: b"" for nm in names}
    for ln in sam.split(b"\n"):
        if ln and not ln.startswith(b"@"):
            out[ln.split(b"\t", 1)[0].decode()] += ln + b"\n"
    return [out[nm] for nm in names]


COUNTERS = ("sa", "xa", "xb", "pa", "hard", "rev", "unmapped", "sec_star", "long_cigar", "long_md", "xa_suppressed", "xa_far")


def check_text(out, want, declined, what, cover, xb=False):
    """every read's slice against the reference's lines; the declined set; coverage over the reads that were written"""
    n = len(want)
    off, flags = out["off"], out["flags"]
    assert off.shape[0] == n + 1 and int(off[0]) == 0 and int(off[n]) == len(out["text"]) and np.all(np.diff(off) >= 0), what
    got_dec = (flags & 1) != 0
    assert np.array_equal(got_dec, declined), f"{what}: declined {np.nonzero(got_dec)[0].tolist()[:20]}, the rule says {np.nonzero(declined)[0].tolist()[:20]}"
    assert out["n_declined"] == int(declined.sum()) and not (flags & ~1).any()
    for i in range(n):
        mine = out["text"][int(off[i]):int(off[i + 1])]
        if declined[i]:
            assert mine == b"" and int(out["n_lines"][i]) == 0, f"{what}: read {i} is declined and has bytes"
            continue
        if mine != want[i]:
            at = next((k for k in range(min(len(mine), len(want[i]))) if mine[k] != want[i][k]), min(len(mine), len(want[i])))
            raise AssertionError(f"{what}: read {i} differs at byte {at} of {len(want[i])} (device {len(mine)}):\n device    {mine[max(0, at - 60):at + 60]!r}\n reference {want[i][max(0, at - 60):at + 60]!r}")
        assert int(out["n_lines"][i]) == mine.count(b"\n")
        for ln in mine.split(b"\n")[:-1]:
            f = ln.split(b"\t")
            fl = int(f[1])
            cover["sa"] += any(t.startswith(b"SA:Z:") for t in f[11:]); cover["xa"] += any(t.startswith(b"XA:Z:") for t in f[11:]); cover["xb"] += any(t.startswith(b"XB:Z:") for t in f[11:])
            cover["pa"] += any(t.startswith(b"pa:f:") for t in f[11:]); cover["hard"] += b"H" in f[5]; cover["rev"] += bool(fl & 0x10); cover["unmapped"] += bool(fl & 0x4)
            cover["sec_star"] += bool(fl & 0x100) and f[9] == b"*" and f[10] == b"*"
            cover["long_cigar"] += sum(ch in b"MIDSH" for ch in f[5]) > 6
            cover["long_md"] += any(t.startswith(b"MD:Z:") and len(t) > 13 for t in f[11:])


def quals_of(rng, n):
    return bytes(rng.integers(33, 74, n).astype(np.uint8))


# ---- 1. the fuzz --------------------------------------------------------------------------------------------------------------------------------------------
def xa_cells(rng, W, T):
    """crafted reads for the XA counters: a non-ALT hit with `n_sec` hits of nearly its score on the same interval -- 3: shown; 8: held back by max_XA_hits;
    100 with ALT hits among them: shown, entries past place 64"""
    made = []
    for n_sec, alt_mode in ((3, "none"), (8, "none"), (100, "mixed"), (70, "all")):
        read, a = make_read(rng, W.g, W.ctg, n_sec + 1, "same", alt_mode, T)
        a["score"] = rng.integers(int(0.9 * 90), 90, n_sec + 1)
        a["score"][0] = 95
        a["ncomp_isalt"][0] = 1      # (the best hit is not ALT)
        a["truesc"] = a["score"]
        made.append((read, a))
    return made


def run_fuzz(W, seed, thin):
    dev = W.dev
    check_limits(dev)
    rng = np.random.default_rng(seed)
    base = ref_opt()
    cells = fuzz_cells(thin, seed)
    made = [make_read(rng, W.g, W.ctg, n, f, m, base.T) for n, f, m in cells] + xa_cells(rng, W, base.T)
    counts = np.array([m[1].shape[0] for m in made], dtype=np.int32)
    assert set(SIZES) <= set(counts.tolist())
    regs = np.concatenate([m[1] for m in made])
    seqs, off = testdata.ragged([m[0] for m in made])
    read_len = np.diff(off).astype(np.int32)
    n = counts.shape[0]
    ids = (1 << 33) + 7 * seed + np.arange(n, dtype=np.int64)
    names = [f"r{i}" for i in range(n)]
    quals = quals_of(rng, int(off[-1]))
    cigs, ops = W.host.region_cigars(base, seqs, off, counts, regs, with_ops=True)
    cover = dict.fromkeys(COUNTERS, 0)
    n_declined = 0
    for name, opt in sam_variants():
        marked = ref_marked(opt, counts, regs, ids)
        sel = dev.alns_flat(opt, counts, regs, ids, read_len, cigs, ops)[0]["sel"]
        declined, suppressed, far = expect_declined(opt, counts, marked, sel, cigs)
        n_declined += int(declined.sum())
        cover["xa_suppressed"] += int((suppressed & ~declined).sum()); cover["xa_far"] += int((far & ~declined).sum())
        for q in ((quals, None) if not thin or name in ("default", "XB") else (quals,)):
            want = ref_lines(W.idx, opt, names, seqs, q, off, counts, regs, ids[0])
            out = dev.sam_flat(opt, seqs, off, counts, regs, ids, cigs, ops, names, quals=q)
            check_text(out, want, declined, f"fuzz seed {seed}, options {name}, {'with' if q else 'without'} qualities", cover)
            assert min(out["kernel_ms"]) >= 0
    zero = [k for k in COUNTERS if cover[k] == 0]
    assert not zero, f"nothing covered {zero}: {cover}"
    # a printed region whose CIGAR record is withheld: exactly that read is declined
    got, _, pri, _, _ = dev.alns_flat(base, counts, regs, ids, read_len, cigs, ops)
    marked = ref_marked(base, counts, regs, ids)
    declined = expect_declined(base, counts, marked, got["sel"], cigs)[0]
    per_read = np.repeat(np.arange(n), counts)
    k = int(np.nonzero((got["sel"] == 0) & (np.repeat(counts, counts) > LANE_MAX) & ~declined[per_read])[0][0])
    lo = np.repeat(np.cumsum(counts) - counts, counts)
    cigs2 = cigs.copy()
    cigs2["n_cigar"][lo[k] + pri["src"][k]] = -1
    want_dec = declined.copy(); want_dec[per_read[k]] = True
    assert np.array_equal(expect_declined(base, counts, marked, got["sel"], cigs2)[0], want_dec)
    out = dev.sam_flat(base, seqs, off, counts, regs, ids, cigs2, ops, names, quals=quals)
    check_text(out, ref_lines(W.idx, base, names, seqs, quals, off, counts, regs, ids[0]), want_dec, f"fuzz seed {seed}, a withheld CIGAR record", dict.fromkeys(COUNTERS, 0))
    return cover, n_declined


# ---- 2. the writer's boundaries ---------------------------------------------------------------------------------------------------------------------------
def exact_region(W, c, tb, ql, rev, qb=0, lq=None, score=None):
    """one region: ql reference bases from tb of contig c on read interval [qb, qb + ql) of a read of lq bases"""
    l_pac = int(W.ctg[-1][0] + W.ctg[-1][1])
    lq = ql if lq is None else lq
    fb = W.ctg[c][0] + tb
    a = np.zeros(1, dtype=ALNREG_DTYPE)
    r = a[0]
    r["rb"], r["re"] = (2 * l_pac - (fb + ql), 2 * l_pac - fb) if rev else (fb, fb + ql)
    r["qb"], r["qe"], r["rid"] = qb, qb + ql, c
    r["score"] = ql if score is None else score
    r["truesc"] = r["score"]
    r["w"], r["seedcov"], r["secondary"], r["secondary_all"] = 100, ql // 2 + 1, -1, -1
    r["ncomp_isalt"] = (np.uint32(c == 2) << np.uint32(30)) | np.uint32(1)
    return a


def piece(W, c, tb, ql, rev):
    seg = W.g[W.ctg[c][0] + tb:W.ctg[c][0] + tb + ql]
    return ((3 - seg)[::-1] if rev else seg).astype(np.uint8)


def run_boundaries(W):
    from test_alns import mutate
    dev = W.dev
    check_limits(dev)
    rng = np.random.default_rng(5)
    opt = ref_opt()
    opt.T = 1      # (reads of one and two bases still print an alignment)
    reads, lists, names = [], [], []
    lens = [1, 2, 63, 64, 65, 127, 128, 129, STAGING - 1, STAGING, STAGING + 1]
    name_lens = [1, 63, 64, 65, 255]
    for j, ql in enumerate(lens):      # exact matches, forward and reverse: the line of a read of STAGING bases is longer than the staging area
        rev = bool(j & 1)
        reads.append(piece(W, 0, 1000 + 700 * j, ql, rev)); lists.append(exact_region(W, 0, 1000 + 700 * j, ql, rev))
        names.append(("n%d_" % j).ljust(name_lens[j % len(name_lens)], "x")[:name_lens[j % len(name_lens)]] if j < 2 * len(name_lens) else f"n{j}")
    names = [nm if nm not in names[:i] else nm[:-1] + "y" for i, nm in enumerate(names)]
    # 10 kb with some hundreds of operations: the operations and the MD string live in the operation array
    long_read = mutate(rng, W.g[20000:30000], 10000, 150)
    reads.append(long_read); lists.append(exact_region(W, 0, 20000, 10000, False, score=6000)); names.append("long10k")
    # two lines that are longer than the staging area only together (a chimera: 150 + 150 bases of a 300-base read), and an unmapped read
    chim = np.concatenate([piece(W, 0, 40000, 150, False), piece(W, 1, 9000, 150, True)])
    reads.append(chim); lists.append(np.concatenate([exact_region(W, 0, 40000, 150, False, 0, 300), exact_region(W, 1, 9000, 150, True, 150, 300, score=140)])); names.append("chimera")
    reads.append(rng.integers(0, 4, 97).astype(np.uint8)); lists.append(np.zeros(0, dtype=ALNREG_DTYPE)); names.append("nohit")
    assert len(set(names)) == len(names) and {len(x) for x in names} >= set(name_lens)
    counts = np.array([a.shape[0] for a in lists], dtype=np.int32)
    regs = np.concatenate(lists)
    seqs, off = testdata.ragged(reads)
    ids = 11 + np.arange(counts.shape[0], dtype=np.int64)
    cigs, ops = W.host.region_cigars(opt, seqs, off, counts, regs, with_ops=True)
    k_long = int(np.cumsum(counts)[names.index("long10k")] - 1)
    assert int(cigs["n_cigar"][k_long]) > 200 and int(cigs["md_len"][k_long]) > 8, "the long read has no long CIGAR"
    assert (cigs["n_cigar"] > 0).all()
    quals = quals_of(rng, int(off[-1]))
    for q in (quals, None):
        want = ref_lines(W.idx, opt, names, seqs, q, off, counts, regs, ids[0])
        out = dev.sam_flat(opt, seqs, off, counts, regs, ids, cigs, ops, names, quals=q)
        check_text(out, want, np.zeros(counts.shape[0], dtype=bool), f"boundaries, {'with' if q else 'without'} qualities", dict.fromkeys(COUNTERS, 0))
    i = names.index("chimera")
    sizes = [len(x) for x in want[i].split(b"\n")[:-1]]
    assert len(sizes) == 2 and max(sizes) + 1 < STAGING < sum(sizes) + 2, sizes
    assert max(len(x) for x in want[lens.index(STAGING)].split(b"\n")) > STAGING


# ---- 3. pa:f: -----------------------------------------------------------------------------------------------------------------------------------------------
# (score, alt_sc).  mem_mark_primary_se sets alt_sc of a non-ALT hit from the ALT hit that shadows it in the first round, and the sort puts the higher score
# first: alt_sc > score in every line that carries the tag.  So the ties are sixteenths -- score / alt_sc = j / 16 for an odd j has 1000 j / 16 = m + 1/2 --:
# 1/16 -> 62.5 -> 0.062 (down to the even digit), 3/16 -> 187.5 -> 0.188 (up), 5/16, 13/16, 15/16 likewise; then quotients no double holds on either
# side of a half in the fourth decimal (0.0125-like values), and the pairs the issue names with the scores swapped into that order.
PA_PAIRS = [(35, 560), (33, 176), (35, 112), (39, 48), (45, 48), (32, 33), (64, 100), (64, 67), (80, 81), (128, 129), (81, 6480), (63, 80), (40, 3200), (73, 80), (99, 160), (31, 32), (30, 31)]


def run_pa(W):
    dev = W.dev
    opt = ref_opt()
    reads, lists = [], []
    for j, (score, alt_sc) in enumerate(PA_PAIRS):      # a hit on chr1 and, over the same bases of the read, a better one on the ALT contig
        assert alt_sc > score >= opt.T
        reads.append(piece(W, 0, 3000 + 200 * j, 150, False))
        lists.append(np.concatenate([exact_region(W, 0, 3000 + 200 * j, 150, False, score=score), exact_region(W, 2, 500 + 200 * j, 150, bool(j & 1), score=alt_sc)]))
    # the pairs as the issue writes them (the hit on chr1 has the higher score: it is not shadowed, no tag): the text is the reference's all the same
    for j, (score, alt_sc) in enumerate([(33, 32), (100, 64), (67, 64), (81, 80), (129, 128)]):
        reads.append(piece(W, 0, 9000 + 200 * j, 150, False))
        lists.append(np.concatenate([exact_region(W, 0, 9000 + 200 * j, 150, False, score=score), exact_region(W, 2, 7000 + 200 * j, 150, False, score=alt_sc)]))
    counts = np.array([a.shape[0] for a in lists], dtype=np.int32)
    regs = np.concatenate(lists)
    seqs, off = testdata.ragged(reads)
    n = counts.shape[0]
    ids = 5 + np.arange(n, dtype=np.int64)
    names = [f"p{i}" for i in range(n)]
    cigs, ops = W.host.region_cigars(opt, seqs, off, counts, regs, with_ops=True)
    want = ref_lines(W.idx, opt, names, seqs, None, off, counts, regs, ids[0])
    out = dev.sam_flat(opt, seqs, off, counts, regs, ids, cigs, ops, names)
    check_text(out, want, np.zeros(n, dtype=bool), "pa:f:", dict.fromkeys(COUNTERS, 0))
    tags = [[t for ln in w.split(b"\n") for t in ln.split(b"\t") if t.startswith(b"pa:f:")] for w in want]
    assert all(len(t) == 1 for t in tags[:len(PA_PAIRS)]), "a crafted pair prints no pa:f: tag"
    assert tags[0] == [b"pa:f:0.062"] and tags[1] == [b"pa:f:0.188"], tags[:2]      # (the reference rounds the ties to even)


# ---- 4. real batches ----------------------------------------------------------------------------------------------------------------------------------------
def run_batches(W, reads, id0s):
    opt = ref_opt()
    dev = W.dev
    rng = np.random.default_rng(9)
    seqs, off = testdata.flat(reads)
    dev.upload(seqs, off); dev.run(opt)
    counts, regs = dev.download()
    cigs = dev.cigars(opt); ops = dev.cigar_ops()
    n = counts.shape[0]
    assert int(counts.max()) > LANE_MAX
    names = [f"read{i}/x" for i in range(n)]
    quals = quals_of(rng, int(off[-1]))
    cover = dict.fromkeys(COUNTERS, 0)
    decoded = hostapi.decode_cigars(cigs, ops)
    for id0 in id0s:
        ids = id0 + np.arange(n, dtype=np.int64)
        before = dev.alns(opt, id0)
        marked = ref_marked(opt, counts, regs, ids)
        declined = expect_declined(opt, counts, marked, before[0]["sel"], cigs)[0]
        out = dev.sam(opt, id0, names, quals=quals)
        check_text(out, ref_lines(W.idx, opt, names, seqs, quals, off, counts, regs, id0), declined, f"batch of {n} reads, id0 {id0}", cover)
        after = dev.alns(opt, id0)
        for x, y in zip(before[:4], after[:4]):
            assert np.array_equal(x, y), "bwagpu_batch_alns returns something else after bwagpu_batch_sam"
        again = dev.cigars(opt)      # (the operation array's order differs from call to call on the device: the decoded records are compared)
        assert hostapi.decode_cigars(again, dev.cigar_ops()) == decoded, "bwagpu_batch_cigars returns something else after bwagpu_batch_sam"
    assert cover["sa"] > 0 and cover["rev"] > 0 and cover["hard"] > 0, cover
    # a table of logarithms too small for any read: the marking records travel to the host for their mapQ and back -- the same text
    dev.set_option("pri_log_cap", 2)
    try:
        again = dev.sam(opt, id0s[-1], names, quals=quals)
    finally:
        dev.set_option("pri_log_cap", 0)
    assert again["text"] == out["text"] and np.array_equal(again["off"], out["off"]) and np.array_equal(again["flags"], out["flags"])


# ---- 6. the command line ------------------------------------------------------------------------------------------------------------------------------------
TRACE = "reads written from device SAM text"


CLI_FLAGS = {"-a": F_ALL, "-M": F_NO_MULTI, "-Y": F_SOFTCLIP, "-u": F_XB, "-V": 0x100}


def expect_written(W, reads, per_batch, extra):
    """the reads of the command line's batches that the rule does not decline, computed with the library's other calls: the batches as the command line cuts
    them, its CIGAR filter on (a region the filter leaves without a CIGAR record and that is printed after all makes its read the host's)"""
    opt = ref_opt()
    for x in extra:
        opt.flag |= CLI_FLAGS.get(x, 0)
    dev = W.dev
    dev.L.bwagpu_set_cigar_filter(dev.h, 1)
    total = 0
    try:
        for lo in range(0, reads.shape[0], per_batch):
            seqs, off = testdata.flat(reads[lo:lo + per_batch])
            dev.upload(seqs, off); dev.run(opt)
            counts, regs = dev.download()
            if int(counts.sum()) == 0:
                continue      # (no CIGAR call: the host prints the batch)
            cigs = dev.cigars(opt)
            sel = dev.alns(opt, lo)[0]["sel"]
            ids = lo + np.arange(counts.shape[0], dtype=np.int64)
            total += int((~expect_declined(opt, counts, ref_marked(opt, counts, regs, ids), sel, cigs)[0]).sum())
    finally:
        dev.L.bwagpu_set_cigar_filter(dev.h, 0)
    return total


def run_cli(W, cli, reads, per_batch, fq, fq_comments, K, env):
    """single-end SAM of `cli` with BWAGPU_CLI_SAMTEXT=1 against `bwa mem`, byte for byte apart from @PG; the trace line counts the reads written from the
    device's text: every read the rule does not decline, or (-5: the host path) none"""
    prefix = W.prefix
    body = lambda t: b"\n".join(l for l in t.split(b"\n") if not l.startswith(b"@PG"))
    n_reads = sum(1 for _ in open(fq)) // 4
    seen = b""
    for extra in ([], ["-a"], ["-M", "-Y"], ["-u"], ["-C"], ["-R", "@RG\\tID:x"], ["-V"], ["-5"]):
        args = ["mem", "-K", str(K), "-t", "2"] + extra + [prefix, fq_comments if extra == ["-C"] else fq]
        p = subprocess.run([refapi.REF_BWA] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()[-1000:]
        want = body(p.stdout)
        p = subprocess.run([cli] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(env, BWAGPU_CLI_TRACE="1", BWAGPU_CLI_SAMTEXT="1"))
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert body(p.stdout) == want, f"BWAGPU_CLI_SAMTEXT=1 {extra}: SAM differs from bwa mem"
        line = [l for l in p.stderr.decode().split("\n") if TRACE in l]
        n_want = 0 if extra == ["-5"] else expect_written(W, reads, per_batch, extra)
        assert extra == ["-5"] or n_reads >= n_want > n_reads // 2
        assert len(line) == 1 and int(line[0].split("]")[1].split()[0]) == n_want, (extra, n_want, p.stderr.decode()[-1500:])
        seen += want
    assert b"SA:Z:" in seen and b"\tBC:Z:ACGT" in seen and b"\tRG:Z:x" in seen
    p = subprocess.run([cli, "mem", "-K", str(K), "-t", "2", prefix, fq], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(env, BWAGPU_CLI_TRACE="1"))
    assert p.returncode == 0 and TRACE not in p.stderr.decode(), "the switch is off by default"
    return seen


def cli_inputs(W, tmp_path, n, seed):
    lens = testdata.small_genome()[1]
    reads = batch_reads(W.g, lens, n, seed)
    fq, fqc = str(tmp_path / "se.fq"), str(tmp_path / "se_comments.fq")
    simdata.write_fastq(fq, reads); simdata.write_fastq(fqc, reads, suffix=" BC:Z:ACGT")
    return reads, fq, fqc


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    import hostsim_build
    w = World(tmp_path_factory.mktemp("sam_sim"), lib_path=hostsim_build.build(), options={"ptab_m": 6})
    yield w
    w.close()


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    w = World(tmp_path_factory.mktemp("sam_gpu"))
    yield w
    w.close()


def test_structs_and_limits(sim):
    check_limits(sim.dev)
    assert C.sizeof(SamIn) == 56 and C.sizeof(SamOut) == 64


def test_sim_sam_flat_fuzz(sim):
    run_fuzz(sim, 31, thin=True)


def test_sim_boundaries(sim):
    run_boundaries(sim)


def test_sim_pa_ties(sim):
    run_pa(sim)


def test_sim_sam_on_batches(sim):
    lens = testdata.small_genome()[1]
    run_batches(sim, batch_reads(sim.g, lens, 60, 521), (7, (1 << 33) + 12345))


def test_sim_cli_samtext(sim, tmp_path):
    import test_cli
    reads, fq, fqc = cli_inputs(sim, tmp_path, 10, 531)
    env = dict(os.environ, BWAGPU_CLI_STREAMS="2", BWAGPU_CLI_SERIALIZE="1", BWAGPU_PTAB_M="6")
    run_cli(sim, test_cli._sim_cli(), reads, 10, fq, fqc, 1500, env)      # (20 reads, ten per batch: id0 > 0 from the second batch on)


def test_contig_names(sim, monkeypatch):
    """a handle made by bwagpu_create has no names until bwagpu_set_contig_names gives it some; a clone shares them, a copy on another device has its own"""
    dev = sim.dev
    meta = dev.index_meta()
    other = BwaGpu.empty(meta, lib_path=dev.L._name)
    try:
        opt = ref_opt()
        args = (opt, np.zeros(0, dtype=np.uint8), np.zeros(2, dtype=np.int64), np.zeros(1, dtype=np.int32), np.zeros(0, dtype=ALNREG_DTYPE), np.arange(1), np.zeros(0, dtype=CIGAR_DTYPE),
                np.zeros(0, dtype=np.uint32), ["q"])
        with pytest.raises(BwaGpuError, match="contig names"):
            other.sam_flat(*args)
        other.set_contig_names(["a", "bb", "ccc"], ["", "x\ty", ""])
        twin = other.clone()
        try:
            for d in (other, twin):
                assert d.sam_flat(*args)["text"] == b"q\t4\t*\t0\t0\t*\t*\t0\t0\t\t*\tAS:i:0\tXS:i:0\n"
        finally:
            twin.close()
        monkeypatch.setenv("MOCK_HIP_DEVICES", "2")      # (the mock's devices share the host's memory)
        far = BwaGpu.__new__(BwaGpu); far.L = other.L; far.h = C.c_void_p()
        other.L.bwagpu_clone_to_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        assert other.L.bwagpu_clone_to_device(other.h, 1, C.byref(far.h)) == 0
        try:
            assert far.sam_flat(*args)["text"].startswith(b"q\t4\t*")
        finally:
            far.close()
        off = np.array([0, 2, 1, 3], dtype=np.int64)
        assert other.L.bwagpu_set_contig_names(other.h, b"abc", off.ctypes.data, None, None) == -2
        assert other.L.bwagpu_set_contig_names(other.h, None, off.ctypes.data, None, None) == -2
    finally:
        other.close()


def test_xr_and_comments(sim):
    """MEM_F_REF_HDR prints the contig's annotation with its tabs as spaces; a comment follows the tags, an empty one prints nothing; RG:Z: and extra_flag"""
    W = sim
    meta = W.dev.index_meta()
    opt = ref_opt()
    reads = [piece(W, 1, 100, 80, False), piece(W, 0, 100, 80, True)]
    lists = [exact_region(W, 1, 100, 80, False), exact_region(W, 0, 100, 80, True)]
    counts = np.array([1, 1], dtype=np.int32)
    regs = np.concatenate(lists)
    seqs, off = testdata.ragged(reads)
    cigs, ops = W.host.region_cigars(opt, seqs, off, counts, regs, with_ops=True)
    names = ["a", "b"]
    plain = ref_lines(W.idx, opt, names, seqs, None, off, counts, regs, 0)
    got = W.dev.sam_flat(opt, seqs, off, counts, regs, np.arange(2), cigs, ops, names, comments=["BC:Z:ACGT x", ""], rg_id="grp1", extra_flag=0x200)
    want = []
    for ln, comment in zip(plain, (b"\tBC:Z:ACGT x", b"")):
        f = ln[:-1].split(b"\t")
        f[1] = str(int(f[1]) | 0x200).encode()
        k = next(i for i, t in enumerate(f) if t.startswith(b"XS:i:"))
        want.append(b"\t".join(f[:k + 1] + [b"RG:Z:grp1"] + f[k + 1:]) + comment + b"\n")
    assert got["text"] == b"".join(want), (got["text"], want)
    # annotations: the handle under test has the index files' (none in this index); set some on a handle of its own
    other = BwaGpu(W.prefix, lib_path=W.dev.L._name, options={"ptab_m": 6})
    try:
        other.set_contig_names(["chr1", "chr2", "chr3"], ["first\tcontig", "", "alt one"])
        o2 = ref_opt(); o2.flag |= 0x100
        got = other.sam_flat(o2, seqs, off, counts, regs, np.arange(2), cigs, ops, names)["text"]
        assert got == plain[0] + plain[1][:-1] + b"\tXR:Z:first contig\n", got
    finally:
        other.close()


def test_error_paths(sim):
    opt = ref_opt()
    dev = sim.dev
    L, h = dev.L, dev.h
    reads = simdata.make_reads_se(sim.g, 4, seed=3)
    seqs, off = testdata.flat(reads)
    names = np.frombuffer(b"abcd", dtype=np.uint8).copy()
    name_off = np.arange(5, dtype=np.int64)
    sin = SamIn(names.ctypes.data, name_off.ctypes.data, None, None, None, None, 0)
    out = SamOut()

    def free(o):
        for p in (o.text, o.off, o.flags, o.n_lines):
            L.bwagpu_free(p)
    dev.upload(seqs, off)
    call = lambda hh=h, oo=opt, i=sin, o=out: L.bwagpu_batch_sam(hh, None if oo is None else C.byref(oo), 0, None if i is None else C.byref(i), None if o is None else C.byref(o))
    assert call() == -2, "before a run"
    dev.run(opt)
    assert call() == -2, "before a download"
    counts, regs = dev.download()
    assert call() == -2, "without the CIGAR call"
    cigs = dev.cigars(opt); ops = dev.cigar_ops()
    for kw in (dict(hh=None), dict(oo=None), dict(i=None), dict(o=None)):
        assert call(**kw) == -2, kw
    o5 = ref_opt(); o5.flag |= F_PRIMARY5
    assert call(oo=o5) == -2, "MEM_F_PRIMARY5"
    assert call(i=SamIn(None, name_off.ctypes.data, None, None, None, None, 0)) == -2 and call(i=SamIn(names.ctypes.data, None, None, None, None, None, 0)) == -2
    assert call(i=SamIn(names.ctypes.data, name_off.ctypes.data, None, names.ctypes.data, None, None, 0)) == -2, "comments without offsets"
    bad = np.array([0, 2, 1, 3, 4], dtype=np.int64)
    assert call(i=SamIn(names.ctypes.data, bad.ctypes.data, None, None, None, None, 0)) == -2 and b"ascend" in L.bwagpu_last_error(h)
    assert call(i=SamIn(names.ctypes.data, name_off.ctypes.data, None, names.ctypes.data, bad.ctypes.data, None, 0)) == -2
    assert call() == 0 and out.n_text > 0 and out.n_declined == 0
    free(out)
    dev.download()
    assert call() == -2, "the CIGAR records of an earlier download"
    dev.cigars(opt)
    # bwagpu_sam_flat
    ids = np.arange(4, dtype=np.int64)
    assert int(counts.sum()) > 0

    def flat(seqs=seqs, off=off, counts=counts, regs=regs, ids=ids, cigs=cigs, ops=ops, n_ops=None, hh=h, oo=opt, i=sin, o=out, n_reads=4):
        ptr = lambda x: None if x is None else x.ctypes.data
        return L.bwagpu_sam_flat(hh, None if oo is None else C.byref(oo), n_reads, ptr(seqs), ptr(off), ptr(counts), ptr(regs), ptr(ids), ptr(cigs), ptr(ops) if ops is not None and ops.shape[0] else None,
                                 (ops.shape[0] if ops is not None else 0) if n_ops is None else n_ops, None if i is None else C.byref(i), None if o is None else C.byref(o))
    assert flat() == 0
    free(out)
    for kw in (dict(hh=None), dict(oo=None), dict(i=None), dict(o=None), dict(seqs=None), dict(off=None), dict(counts=None), dict(regs=None), dict(ids=None), dict(cigs=None), dict(n_reads=-1), dict(n_ops=-1),
               dict(oo=o5)):
        assert flat(**kw) == -2, kw
    assert flat(off=np.array([0, 150, 140, 450, 600], dtype=np.int64)) == -2, "read offsets that do not ascend"
    assert flat(i=SamIn(names.ctypes.data, bad.ctypes.data, None, None, None, None, 0)) == -2
    b = regs.copy(); b["rid"][0] = 3
    assert flat(regs=b) == -2, "a rid outside the index"
    for v in (-2, 32769):
        b = cigs.copy(); b["n_cigar"][0] = v
        assert flat(cigs=b) == -2, v
    b = cigs.copy(); b["n_cigar"][0] = 7; b["cigar"][0][0] = max(0, ops.shape[0] - 6); b["cigar"][0][1] = 0
    assert flat(cigs=b) == -2, "operations past the end of the array"
    b = cigs.copy(); b["md_len"][0] = 9; b["md"][0] = max(0, ops.shape[0] - 2)
    assert flat(cigs=b) == -2, "an MD string past the end of the array"
    # no reads; reads without regions
    assert L.bwagpu_sam_flat(h, C.byref(opt), 0, None, None, None, None, None, None, None, 0, C.byref(SamIn()), C.byref(out)) == 0 and out.n_text == 0
    free(out)
    res = dev.sam_flat(opt, seqs[:300], off[:3], np.zeros(2, dtype=np.int32), np.zeros(0, dtype=ALNREG_DTYPE), np.arange(2), np.zeros(0, dtype=CIGAR_DTYPE), np.zeros(0, dtype=np.uint32), ["u0", "u1"])
    assert res["n_lines"].tolist() == [1, 1] and res["n_declined"] == 0 and res["text"].count(b"\t4\t*\t0\t0\t*\t*\t0\t0\t") == 2


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed", [31, 32, 33])
def test_gpu_sam_flat_fuzz(gpu, seed):
    run_fuzz(gpu, seed, thin=False)


@pytest.mark.gpu
def test_gpu_boundaries(gpu):
    run_boundaries(gpu)


@pytest.mark.gpu
def test_gpu_pa_ties(gpu):
    run_pa(gpu)


@pytest.mark.gpu
def test_gpu_sam_on_batches(gpu):
    lens = testdata.small_genome()[1]
    run_batches(gpu, batch_reads(gpu.g, lens, 1500, 621), (7, (1 << 35) + 7771))


@pytest.mark.gpu
def test_gpu_cli_samtext(gpu, tmp_path):
    from bwa_amd import build as b
    _, cli = b.build_host(verbose=False)
    reads, fq, fqc = cli_inputs(gpu, tmp_path, 600, 631)
    seen = run_cli(gpu, cli, reads, 1000, fq, fqc, 150000, dict(os.environ))      # (1200 reads, 1000 per batch)
    assert b"XA:Z:" in seen and b"XB:Z:" in seen and b"\tpa:f:" in seen
