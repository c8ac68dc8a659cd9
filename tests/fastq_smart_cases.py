"""Interleaved FASTQ inputs (`mem -p`) for the tests of bwagpu_fastq_batch_smart (tests/test_fastq_smart.py, tests/test_gpu_fastq_smart.py)
and the reference they are compared with: the compiled reference's own bseq_read followed by bseq_classify (bwa.c:79-130), called through
ctypes on oracle/_ref/libbwaref.so.

A case is fastq_cases' dict with one file: files (one byte string) and ends (the byte offset behind every record)."""
import ctypes as C
import functools
import os
import tempfile

import numpy as np

import fastq_cases
from fastq_cases import _acgt, _case, _rec

CHUNKS = (1, 7, 150, 1 << 20)


def named(rng, names, ls=None, comments=None):
    """one record per name; ls: the read length (default: 4 + i % 5 -- chunks of 7 and 150 cut everywhere)"""
    out = []
    for i, n in enumerate(names):
        head = n if comments is None or comments[i] is None else n + b" " + comments[i]
        out.append(_rec(head, _acgt(rng, ls if ls else 4 + i % 5)))
    return _case(out)


def runs(lengths, tag=b"r"):
    """names in runs of the given lengths: every run its own name"""
    return [tag + b"%d" % k for k, n in enumerate(lengths) for _ in range(n)]


def cases():
    rng = np.random.default_rng(733)
    c = {}
    c["n1"] = named(rng, [b"a"])
    c["n2_pair"] = named(rng, [b"a", b"a"])
    c["n2_single"] = named(rng, [b"a", b"b"])
    c["n3_run"] = named(rng, [b"a", b"a", b"a"])
    c["n3_pair_first"] = named(rng, [b"a", b"a", b"b"])
    c["n3_pair_last"] = named(rng, [b"a", b"b", b"b"])
    c["all_single"] = named(rng, [b"s%d" % i for i in range(11)])
    c["all_pairs"] = named(rng, runs([2] * 10, b"p"))
    c["odd_last"] = named(rng, runs([2, 2, 2, 1], b"p"))
    c["runs_1_to_5"] = named(rng, runs([1, 2, 3, 4, 5, 1, 5, 4, 3, 2, 1]))      # 3: pair + single; 5: pair, pair, single
    c["trim_readno"] = named(rng, [b"x/1", b"x/2", b"y/1", b"y/12", b"/1", b"/1", b"/1", b"/2", b"z/1", b"z", b"w/a", b"w/b", b"v/1/2", b"v/1/1", b"v/1"])
    c["prefixes"] = named(rng, [b"abc", b"abcd", b"abcd", b"ab", b"abc", b"abc", b"a", b"", b""])
    L70, L130 = b"n" * 69, b"m" * 129
    c["long_names"] = named(rng, [L70 + b"a", L70 + b"a", L70 + b"b", L70[:20] + b"X" + L70[21:] + b"b", L70 + b"b", L70[:7] + b"Y" + L70[8:] + b"b",
                                  L130 + b"a", L130 + b"b", L130 + b"b", L130[:17] + b"Z" + L130[18:] + b"b", L130[:64] + b"Z" + L130[65:] + b"b", L130[:64] + b"Z" + L130[65:] + b"b",
                                  L130 + b"c", L130[:-1] + b"c"])
    c["comments"] = named(rng, [b"a", b"a", b"b", b"b", b"c", b"c", b"d"], comments=[b"one", b"two", None, b"x", b"", b"", b"a"])
    # reads of 50 bases: chunk 150 closes after four reads, chunks 1 and 7 after two -- runs of three and four names are cut
    c["cut_runs"] = named(rng, runs([3, 4, 3, 3, 4, 1, 4]), ls=50)
    # a NUL in a name: strcmp stops there (bwagpu.h: names are compared as strcmp compares them)
    c["nul_in_name"] = named(rng, [b"a\0b", b"a\0c", b"ab\0", b"ab", b"ab", b"ab\0x", b"abcdefghij\0X", b"abcdefghij\0YY", b"abcdefghijk", b"abcdefghij\0", b"\0", b"",
                                   b"q\0/1", b"q\0/2", b"q", b"pq\0rstuvwxyz", b"pq"])
    return c


def hardware_cases():
    """run boundaries on wavefront and block boundaries, and scans over several blocks"""
    rng = np.random.default_rng(734)
    c = {}
    for tag, where in ((b"a", ((63, 3), (255, 4), (1023, 3))), (b"b", ((64, 3), (256, 5), (1024, 2)))):      # 1500 short reads, runs that start at these reads
        names = [b"u%d" % i for i in range(1500)]
        for start, n in where:
            for i in range(start, start + n):
                names[i] = b"run%d" % start
        c["runs_at_boundaries_" + tag.decode()] = named(rng, names)
    c["run_of_700"] = named(rng, [b"h%d" % i for i in range(301)] + [b"same"] * 700 + [b"t%d" % i for i in range(200)])
    c["all_pairs_1024"] = named(rng, runs([2] * 512, b"p"))
    c["all_single_1025"] = named(rng, [b"s%d" % i for i in range(1025)])
    return c


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def classify_py(names):
    """the recurrence itself (names as C strings): paired[i] = eq[i] and not paired[i - 1]"""
    paired = [False] * (len(names) + 1)
    for i in range(1, len(names)):
        paired[i] = names[i] == names[i - 1] and not paired[i - 1]
    return [2 if paired[i] else 1 if paired[i + 1] else 0 for i in range(len(names))]


def _ref_smart(data, chunk):
    L, libc, nt4 = fastq_cases._reflib()
    B = fastq_cases._BSeq1
    L.bseq_classify.restype = None
    L.bseq_classify.argtypes = [C.c_int, C.POINTER(B), C.POINTER(C.c_int), C.POINTER(C.POINTER(B))]
    out = []
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "r.fq")
        with open(p, "wb") as f:
            f.write(data)
        fp = L.gzopen(p.encode(), b"r")
        assert fp
        ks = L.kseq_init(fp)
        try:
            while True:
                n = C.c_int(0)
                seqs = L.bseq_read(chunk, C.byref(n), ks, None)
                if n.value == 0:
                    break
                m = (C.c_int * 2)()
                sep = (C.POINTER(B) * 2)()
                L.bseq_classify(n.value, seqs, m, sep)
                recs = []
                for i in range(n.value):
                    s = seqs[i]
                    seq = C.string_at(s.seq)
                    assert len(seq) == s.l_seq and s.id == i
                    recs.append((C.string_at(s.name), C.string_at(s.comment) if s.comment else None, bytes(nt4[b] for b in seq), C.string_at(s.qual) if s.qual else None))
                idx = [[int(sep[k][j].id) for j in range(m[k])] for k in range(2)]
                for k in range(2):      # (the copies in sep share the reads' strings)
                    assert all(sep[k][j].name == seqs[idx[k][j]].name for j in range(m[k]))
                    libc.free(C.cast(sep[k], C.c_void_p))
                for i in range(n.value):
                    for q in (seqs[i].name, seqs[i].comment, seqs[i].seq, seqs[i].qual):
                        libc.free(q)
                libc.free(C.cast(seqs, C.c_void_p))
                cls = [0] * len(recs)
                for j, i in enumerate(idx[1]):
                    cls[i] = 1 + (j & 1)
                assert cls == classify_py([r[0] for r in recs]) and sorted(idx[0] + idx[1]) == list(range(len(recs)))
                out.append({"recs": recs, "idx": idx, "cls": cls})
        finally:
            L.kseq_destroy(ks)
            L.gzclose(fp)
    return out


@functools.lru_cache(maxsize=None)
def _ref_cached(data, chunk):
    return _ref_smart(data, chunk)


def ref_smart(case, chunk):
    """bseq_read(chunk) + bseq_classify until no read is left: [{recs: [(name as a C string, comment or None, nt4 codes, qualities)], idx: [singles,
    pairs], cls}] -- computed once per (case, chunk)"""
    return _ref_cached(case["files"][0], int(chunk))


# ---- the device's batch against it ---------------------------------------------------------------------------------------------------
def check_batch(r, want, window=None):
    """a batch_smart() result against one reference batch, field by field.  Names: the reference hands out C strings, so a name with a NUL
    is compared up to it -- and the device's name must be the window's whole name (check_recs)"""
    n = len(want["recs"])
    assert r["n_reads"] == n and r["cls"].tolist() == want["cls"]
    assert r["n_sub"] == (len(want["idx"][0]), len(want["idx"][1])) and r["n_sub"][1] % 2 == 0
    for k in range(2):
        sub = r["sub"][k]
        assert r["idx"][k].tolist() == want["idx"][k], k
        assert sub["n_reads"] == r["n_sub"][k] and len(sub["off"]) == sub["n_reads"] + 1
        assert sub["off"][0] == 0 and sub["name_off"][0] == 0 and sub["comment_off"][0] == 0
        got = [(a.split(b"\0", 1)[0], b, c, d) for a, b, c, d in fastq_cases.device_records(sub)]
        assert got == [want["recs"][i] for i in want["idx"][k]], k
        if window is not None:
            fastq_cases.check_recs(sub, [window])


def run_smart(parser, case, chunk, call=None):
    """the device's batches over a case, the whole rest of the file as the window: each equal to bseq_read + bseq_classify's, consumed at the
    generator's record ends, END last.  call(window, chunk): another way to make the call (default: parser.batch_smart)"""
    from bwa_amd import api
    want = ref_smart(case, chunk)
    data = case["files"][0]
    pos, taken = 0, 0
    for bi in range(len(want) + 1):
        win = data[pos:]
        r = call(win, chunk) if call else parser.batch_smart(win, chunk_size=chunk)
        assert r["status"] in (api.FQ_CUT, api.FQ_END), (bi, r["status"], r["declined_at"])
        if bi == len(want):
            assert r["status"] == api.FQ_END and r["n_reads"] == 0 and r["n_sub"] == (0, 0)
            assert all(len(s["off"]) == 1 and s["off"][0] == 0 and s["name_off"][0] == 0 and s["comment_off"][0] == 0 for s in r["sub"])
            break
        check_batch(r, want[bi], win)
        taken += r["n_reads"]
        assert pos + r["consumed"] == int(case["ends"][0][taken - 1]), f"consumed, batch {bi}"
        pos += r["consumed"]
        if r["status"] == api.FQ_END:
            assert bi == len(want) - 1
            break
    assert pos == len(data)
    return len(want)


def run_smart_bgzf(parser, case, comp, chunk):
    """the same through batch_smart_bgzf, each window starting at the virtual offset the call before left"""
    from bwa_amd import api
    want = ref_smart(case, chunk)
    coff, uoff, tpos = 0, 0, 0
    for bi in range(len(want) + 1):
        r = parser.batch_smart_bgzf(comp[coff:], skip=uoff, chunk_size=chunk)
        assert r["status"] in (api.FQ_CUT, api.FQ_END) and r["bgzf"]["damaged_at"] == -1, (bi, r["status"], r["bgzf"])
        if bi == len(want):
            assert r["status"] == api.FQ_END and r["n_reads"] == 0
            break
        check_batch(r, want[bi])
        tpos += r["consumed"]
        coff += r["bgzf"]["next_coff"]
        uoff = r["bgzf"]["next_uoff"]
        if r["status"] == api.FQ_END:
            assert bi == len(want) - 1
            break
    assert tpos == len(case["files"][0])


def run_irregular(parser, case, chunk):
    """fastq_cases.run_irregular for batch_smart: the batches bseq_read closes by its own rule before record k equal the device's, the batch
    that holds k is declined at k"""
    from bwa_amd import api
    want = ref_smart(case, chunk)
    data = case["files"][0]
    pos, taken, n_cut = 0, 0, 0
    for bi in range(len(want) + 1):
        r = parser.batch_smart(data[pos:], chunk_size=chunk)
        b = want[bi] if bi < len(want) else None
        whole = b is not None and taken + len(b["recs"]) <= case["k"] and len(b["recs"]) % 2 == 0 and sum(len(x[2]) for x in b["recs"]) >= chunk
        if not whole:
            assert r["status"] == api.FQ_DECLINED and r["n_reads"] == 0 and "cls" not in r and "sub" not in r, (bi, r["status"])
            assert pos + r["declined_at"] == case["at"], (r["declined_at"], pos, case["at"])
            return n_cut
        assert r["status"] == api.FQ_CUT
        check_batch(r, b, data[pos:])
        n_cut += 1
        taken += r["n_reads"]
        pos += r["consumed"]
    raise AssertionError("the device never declined")


def same_result(r, q):
    assert r["status"] == q["status"] and r["n_reads"] == q["n_reads"] and r["consumed"] == q["consumed"] and r["n_sub"] == q["n_sub"]
    assert np.array_equal(r["cls"], q["cls"])
    for k in range(2):
        assert np.array_equal(r["idx"][k], q["idx"][k])
        for f in ("seqs", "off", "name_off", "comment_off", "has_comment", "recs"):
            assert np.array_equal(r["sub"][k][f], q["sub"][k][f]), (k, f)
        assert all(r["sub"][k][f] == q["sub"][k][f] for f in ("names", "comments", "quals"))


def run_windows(parser, case, chunk):
    """the result does not depend on the window length once the window reaches the cut; a shorter window gives MORE, then the same result"""
    from bwa_amd import api
    data = case["files"][0]
    whole = parser.batch_smart(data, chunk_size=chunk)
    assert whole["status"] == api.FQ_CUT and 0 < whole["consumed"] < len(data)
    rng = np.random.default_rng(6)
    for n in [whole["consumed"], len(data)] + [int(x) for x in rng.integers(whole["consumed"], len(data) + 1, 8)]:
        same_result(parser.batch_smart(data[:n], chunk_size=chunk, eof=n == len(data)), whole)
    for short in (whole["consumed"] - 3, whole["consumed"] // 2 + 1, 1):
        short += short in case["ends"][0]      # (not a record boundary)
        r = parser.batch_smart(data[:short], chunk_size=chunk, eof=False)
        assert r["status"] == api.FQ_MORE and r["n_reads"] == 0 and "cls" not in r and "sub" not in r, short
        same_result(parser.batch_smart(data[:whole["consumed"] + 5], chunk_size=chunk, eof=False), whole)


# ---- the command line with BWAGPU_CLI_FASTQ=1 BWAGPU_CLI_SMARTPE_DEV=1 -----------------------------------------------------------------
def write_interleaved(path, g, n_pairs, orphans, seed):
    """one file: the mates of n_pairs pairs interleaved, with comments and /1 /2 suffixes, and after pair i for every i in orphans a read without a
    mate.  Returns the number of reads"""
    from bwa_amd import simdata
    r1, r2 = simdata.make_reads_pe(g, n_pairs + len(orphans), seed=seed)
    a = simdata._ASCII
    n = 0

    def rec(name, r, i, k):
        q = bytes(33 + (j * 5 + i + k) % 41 for j in range(r.shape[1]))
        return name + f" BC:Z:ACGT{i}\tx\n".encode() + a[r[i]].tobytes() + b"\n+\n" + q + b"\n"

    with open(path, "wb") as f:
        for i in range(n_pairs):
            f.write(rec(b"@p%d/1" % i, r1, i, 1) + rec(b"@p%d/2" % i, r2, i, 2))
            n += 2
            if i in orphans:
                j = n_pairs + sorted(orphans).index(i)
                f.write(rec(b"@orphan%d" % i, r1 if i % 2 else r2, j, 1))
                n += 1
    return n
