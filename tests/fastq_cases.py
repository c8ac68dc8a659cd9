"""FASTQ inputs for the device FASTQ reader's tests (tests/test_fastq.py, tests/test_gpu_fastq.py) and the reference they are compared
with: the compiled reference's own kseq_read / bseq_read (kseq.h:175-215, bwa.c:79-112) and nst_nt4_table, called through ctypes on
oracle/_ref/libbwaref.so.

A case is a dict: files (one or two byte strings), ends (per file: the byte offset behind every record, as the generator wrote them)
and, for an irregular case, k / file / at: the record that is not plain, the file it is in and its byte offset there."""
import ctypes as C
import functools
import os
import re
import subprocess
import tempfile

import numpy as np

import refapi

CHUNKS = (1, 7, 150, 1000)


def _rec(name: bytes, seq: bytes, qual: bytes = None, plus: bytes = b"", eol: bytes = b"\n") -> bytes:
    if qual is None:
        qual = bytes(33 + (7 * j + len(seq)) % 60 for j in range(len(seq)))
    return b"@" + name + eol + seq + eol + b"+" + plus + eol + qual + eol


def _case(*files):
    """files: lists of record byte strings"""
    return {"files": [b"".join(f) for f in files], "ends": [list(np.cumsum([len(r) for r in f])) for f in files]}


def _acgt(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def _cycle(rng, n, tag=b"", len0=0, name0=0):
    """n records, read lengths cycling 1..70 and name lengths 1..40: newlines at every position mod 16 and across the tile edges"""
    out = []
    for i in range(n):
        ls, ln = 1 + (i + len0) % 70, 1 + (i + name0) % 40
        name = (tag + b"%d" % i + b"n" * 40)[:ln]
        out.append(_rec(name + (b" c%d" % i if i % 3 == 0 else b""), _acgt(rng, ls), plus=name if i % 5 == 0 else b""))
    return out


def plain_cases():
    rng = np.random.default_rng(611)
    c = {}
    c["cycle"] = _case(_cycle(rng, 420))                                   # ~50 KB: a few tiles
    c["one_record"] = _case([_rec(b"only", b"ACGTACGTAC")])
    c["one_base"] = _case([_rec(b"b", b"A", b"I")])
    c["empty"] = _case([])
    c["names"] = _case([_rec(n, _acgt(rng, 9)) for n in (b"a/1", b"/1", b"ab/x", b"r/12", b"r/1/2", b"r/1 /2", b"xy/9", b"//7", b"")])
    c["headers"] = _case([_rec(b"nodelim", b"ACGT"), _rec(b"empty_comment ", b"ACGT"), _rec(b"tab\tcomment here", b"ACGT"), _rec(b"blanks   three  blanks ", b"ACGT"),
                          _rec(b"vt\x0bv\x0cw", b"ACGT"), _rec(b"cr\rmid", b"ACGT"), _rec(b" noname", b"ACGT"), _rec(b"s/1 c/2", b"ACGT"), _rec(b"last", b"ACGT")])
    c["plus_name"] = _case([_rec(b"p%d" % i, _acgt(rng, 5 + i), plus=b"p%d anything @ + \r" % i) for i in range(12)])
    c["qual_at"] = _case([_rec(b"q%d" % i, _acgt(rng, 6), q) for i, q in enumerate((b"@@@@@@", b"+IIIII", b"@+@+@+", b">>>>>>", b"I+I@I>", b"!!!!!~"))])
    c["bases"] = _case([_rec(b"lower", b"acgtacgtnn"), _rec(b"iupac", b"RYKMSWBDHVNrykmswbdhvn"), _rec(b"dash", b"AC-GT--a-"), _rec(b"mixed", b"AcGtNn-.*xX"), _rec(b"d1", b"-"), _rec(b"d2", b"--")])
    allb = bytes(range(0x21, 0x80))
    c["all_bytes"] = _case([_rec(b"fwd", b"A" + allb, b"I" + allb), _rec(b"rev", b"C" + allb[::-1], allb[::-1] + b"!"), _rec(b"x", b"N" + allb + allb, allb + allb + b"~")])
    # reads 3 + 4 + 5 + ...: sums that reach the chunk at an odd read count (7 after 2 reads, 12 after 3, ...)
    c["odd_sums"] = _case([_rec(b"o%d" % i, _acgt(rng, 3 + i)) for i in range(9)])
    c["pairs_cycle"] = _case(_cycle(rng, 150, b"p"), _cycle(rng, 150, b"p", len0=17, name0=5))
    c["pairs_diff"] = _case([_rec(b"m%d/1" % i, _acgt(rng, 30 + i % 7), plus=b"x" * (i % 3)) for i in range(40)],
                            [_rec(b"m%d/2 second" % i, _acgt(rng, 3 + (5 * i) % 50)) for i in range(40)])
    c["pairs_one"] = _case([_rec(b"a/1", b"ACG")], [_rec(b"a/2", b"TTTTT")])
    c["pairs_empty"] = _case([], [])
    return c


def irregular_cases():
    """exactly one irregularity each, at record k of file `file`"""
    rng = np.random.default_rng(612)

    def base(n=30, tag=b"r"):
        return [_rec(tag + b"%d c" % i, _acgt(rng, 20 + i % 11)) for i in range(n)]

    def planted(k, rec, files=None, file=0, drop_after=False):
        f = files if files is not None else [base()]
        f[file][k] = rec
        if drop_after:
            del f[file][k + 1:]
        c = _case(*f)
        c.update(k=k, file=file, at=int(c["ends"][file][k - 1]) if k else 0)
        return c

    c = {}
    s = _acgt(rng, 24)
    q = b"I" * 24
    c["crlf"] = planted(11, _rec(b"crlf c", s, q, eol=b"\r\n"))
    c["crlf_header_only"] = planted(4, b"@h c\r\n" + s + b"\n+\n" + q + b"\n")
    c["crlf_qual_only"] = planted(5, b"@h\n" + s + b"\n+\n" + q + b"\r\n")
    c["two_line_seq"] = planted(13, b"@two\n" + s[:10] + b"\n" + s[10:] + b"\n+\n" + q + b"\n")
    c["blank_line"] = planted(9, b"\n" + _rec(b"after_blank", s, q))
    c["fasta_record"] = planted(17, b">fa c\n" + s + b"\n")
    c["seq_starts_gt"] = planted(3, _rec(b"gt", b">" + s[1:], q))
    c["short_qual"] = planted(12, _rec(b"sq", s, q[:20]))
    c["empty_seq"] = planted(6, b"@e\n\n+\n\n")
    c["blank_in_bases"] = planted(14, _rec(b"bl", s[:7] + b" " + s[8:], q))
    c["tab_in_bases"] = planted(0, _rec(b"tb", s[:7] + b"\t" + s[8:], q))
    c["high_byte"] = planted(21, _rec(b"hb", s[:5] + b"\xc3" + s[6:], q))
    c["no_plus"] = planted(8, b"@np\n" + s + b"\n-\n" + q + b"\n")
    c["no_final_newline"] = planted(29, _rec(b"nf", s, q)[:-1])
    c["cut_mid_record"] = planted(22, _rec(b"cut", s, q)[:-9], drop_after=True)
    c["cut_in_header"] = planted(10, b"@cu", drop_after=True)
    c["pair_bad_in_2"] = planted(7, _rec(b"p7 c", s, q, eol=b"\r\n"), files=[base(20, b"p"), base(20, b"p")], file=1)
    c["pair_bad_in_1"] = planted(15, b"@two\n" + s[:10] + b"\n" + s[10:] + b"\n+\n" + q + b"\n", files=[base(20, b"p"), base(20, b"p")], file=0)
    # the second file one record short: the first file's last record is the first one not taken
    f1, f2 = base(20, b"p"), base(19, b"p")
    c["pair_2_short"] = _case(f1, f2)
    c["pair_2_short"].update(k=19, file=0, at=int(c["pair_2_short"]["ends"][0][18]))
    f1, f2 = base(18, b"p"), base(20, b"p")
    c["pair_1_short"] = _case(f1, f2)
    c["pair_1_short"].update(k=18, file=1, at=int(c["pair_1_short"]["ends"][1][17]))
    return c


# ---- the reference ---------------------------------------------------------------------------------------------------------------
class _BSeq1(C.Structure):      # bseq1_t (bwa.h:26-30)
    _fields_ = [("l_seq", C.c_int), ("id", C.c_int), ("name", C.c_void_p), ("comment", C.c_void_p), ("seq", C.c_void_p), ("qual", C.c_void_p), ("sam", C.c_void_p)]


_ref = None


def _reflib():
    global _ref
    if _ref is None:
        L = C.CDLL(refapi.REF_SO)
        L.gzopen.restype = C.c_void_p
        L.gzopen.argtypes = [C.c_char_p, C.c_char_p]
        L.gzclose.argtypes = [C.c_void_p]
        L.kseq_init.restype = C.c_void_p
        L.kseq_init.argtypes = [C.c_void_p]
        L.kseq_destroy.argtypes = [C.c_void_p]
        L.bseq_read.restype = C.POINTER(_BSeq1)
        L.bseq_read.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]
        libc = C.CDLL(None)
        libc.free.argtypes = [C.c_void_p]
        _ref = (L, libc, bytes((C.c_ubyte * 256).in_dll(L, "nst_nt4_table")))
    return _ref


def _ref_batches(files, chunk):
    L, libc, nt4 = _reflib()
    with tempfile.TemporaryDirectory() as d:
        ks = []
        fps = []
        for i, data in enumerate(files):
            p = os.path.join(d, f"r{i}.fq")
            with open(p, "wb") as f:
                f.write(data)
            fp = L.gzopen(p.encode(), b"r")
            assert fp
            fps.append(fp)
            ks.append(L.kseq_init(fp))
        out = []
        try:
            while True:
                n = C.c_int(0)
                seqs = L.bseq_read(chunk, C.byref(n), ks[0], ks[1] if len(ks) > 1 else None)
                if n.value == 0:
                    break
                batch = []
                for i in range(n.value):
                    s = seqs[i]
                    seq = C.string_at(s.seq)
                    assert len(seq) == s.l_seq
                    batch.append((C.string_at(s.name), C.string_at(s.comment) if s.comment else None, bytes(nt4[b] for b in seq), C.string_at(s.qual) if s.qual else None))
                    for p in (s.name, s.comment, s.seq, s.qual):
                        libc.free(p)
                libc.free(C.cast(seqs, C.c_void_p))
                out.append(batch)
        finally:
            for k in ks:
                L.kseq_destroy(k)
            for fp in fps:
                L.gzclose(fp)
        return out


@functools.lru_cache(maxsize=None)
def _ref_cached(files, chunk):
    return _ref_batches(files, chunk)


def ref_batches(case, chunk):
    """bseq_read(chunk) until it returns no read: [[(name, comment or None, nt4 codes, qualities)]] -- computed once per (case, chunk)"""
    return _ref_cached(tuple(case["files"]), int(chunk))


def total_bases(case):
    return sum(len(r[2]) for b in ref_batches(case, 1 << 30) for r in b)


def chunks_for(case):
    t = total_bases(case)
    return list(CHUNKS) + ([t, t + 1] if t else [])


# ---- the device's batch, in the reference's terms ----------------------------------------------------------------------------------
def device_records(r):
    """a FastqParser.batch() result as [(name, comment or None, nt4 codes, qualities)]; a present but empty comment is None, as bseq_read leaves it"""
    out = []
    off, no, co = r["off"], r["name_off"], r["comment_off"]
    for i in range(r["n_reads"]):
        com = r["comments"][co[i]:co[i + 1]]
        assert r["has_comment"][i] or not com
        out.append((r["names"][no[i]:no[i + 1]], com if com else None, r["seqs"][off[i]:off[i + 1]].tobytes(), r["quals"][off[i]:off[i + 1]]))
    return out


def check_recs(r, windows):
    """the record table against the arrays: every field is the window's bytes at the recorded place"""
    for i in range(r["n_reads"]):
        e = r["recs"][i]
        w = windows[int(e["file"])]
        assert int(e["file"]) == (i % len(windows) if len(windows) > 1 else 0)
        assert w[e["name"]:e["name"] + e["l_name"]] == r["names"][r["name_off"][i]:r["name_off"][i + 1]]
        assert w[e["comment"]:e["comment"] + e["l_comment"]] == r["comments"][r["comment_off"][i]:r["comment_off"][i + 1]]
        assert w[e["qual"]:e["qual"] + e["l_qual"]] == r["quals"][r["off"][i]:r["off"][i + 1]]
        assert e["l_seq"] == e["l_qual"] == r["off"][i + 1] - r["off"][i] and int(e["has_comment"]) == int(r["has_comment"][i])


def run_plain(parser, case, chunk):
    """the device's batches over a plain case, whole rest of each file as the window: equal to bseq_read's, consumed at the generator's record ends, END last"""
    from bwa_amd import api
    want = ref_batches(case, chunk)
    files, nf = case["files"], len(case["files"])
    pos, taken = [0] * nf, 0
    for bi in range(len(want) + 1):
        win = [f[p:] for f, p in zip(files, pos)]
        r = parser.batch(win[0], win[1] if nf > 1 else None, chunk_size=chunk)
        assert r["status"] in (api.FQ_CUT, api.FQ_END), (bi, r["status"], r["declined_file"], r["declined_at"])      # no plain case declines a batch
        if bi == len(want):
            assert r["status"] == api.FQ_END and r["n_reads"] == 0
            break
        assert device_records(r) == want[bi], f"batch {bi}"
        check_recs(r, win)
        taken += r["n_reads"]
        for k in range(nf):
            n_k = taken // nf
            assert pos[k] + r["consumed"][k] == (int(case["ends"][k][n_k - 1]) if n_k else 0), f"consumed, batch {bi}, file {k}"
            pos[k] += r["consumed"][k]
        if r["status"] == api.FQ_END:      # (a last batch that reaches the cut at the file's last byte is CUT; the call after it is END with no read)
            assert bi == len(want) - 1
            break
    assert all(p == len(f) for p, f in zip(pos, files))


def run_irregular(parser, case, chunk):
    """every batch bseq_read closes by its own rule before record k equals the device's; the batch that holds k is declined at k"""
    from bwa_amd import api
    want = ref_batches(case, chunk)
    files, nf = case["files"], len(case["files"])
    pos, taken = [0] * nf, 0
    n_cut = 0
    for bi in range(len(want) + 1):
        win = [f[p:] for f, p in zip(files, pos)]
        r = parser.batch(win[0], win[1] if nf > 1 else None, chunk_size=chunk)
        b = want[bi] if bi < len(want) else None
        whole = b is not None and (taken + len(b)) // nf <= case["k"] and len(b) % 2 == 0 and sum(len(x[2]) for x in b) >= chunk
        if not whole:
            assert r["status"] == api.FQ_DECLINED and r["n_reads"] == 0 and "seqs" not in r, (bi, r["status"])
            assert r["declined_file"] == case["file"] and pos[case["file"]] + r["declined_at"] == case["at"], (r["declined_file"], r["declined_at"], pos, case["at"])
            return n_cut
        assert r["status"] == api.FQ_CUT and device_records(r) == b, f"batch {bi}"
        n_cut += 1
        taken += r["n_reads"]
        for k in range(nf):
            pos[k] += r["consumed"][k]
    raise AssertionError("the device never declined")


def run_windows(parser, PLAIN):
    """the result does not depend on the window length once the window reaches the cut; a window that stops short gives MORE, or DECLINED with eof"""
    from bwa_amd import api
    rng = np.random.default_rng(5)
    for name, chunk in (("cycle", 1000), ("pairs_cycle", 700)):
        files = PLAIN[name]["files"]
        nf = len(files)
        whole = parser.batch(files[0], files[1] if nf > 1 else None, chunk_size=chunk)
        assert whole["status"] == api.FQ_CUT
        for _ in range(12):
            lens = [int(rng.integers(whole["consumed"][k], len(files[k]) + 1)) for k in range(nf)]
            win = [f[:n] for f, n in zip(files, lens)]
            r = parser.batch(win[0], win[1] if nf > 1 else None, chunk_size=chunk, eof=tuple(n == len(f) for n, f in zip(lens, files)) + (True,) * (2 - nf))
            assert r["status"] == api.FQ_CUT and r["consumed"] == whole["consumed"], lens
            for k in ("seqs", "off", "name_off", "comment_off", "has_comment", "recs"):
                assert np.array_equal(r[k], whole[k]), (k, lens)
            assert (r["names"], r["comments"], r["quals"]) == (whole["names"], whole["comments"], whole["quals"])
        # a window that stops short of the cut, in the middle of a record
        for short in (whole["consumed"][0] - 3, whole["consumed"][0] // 2 + 1, 1):
            short += short in PLAIN[name]["ends"][0]      # (not a record boundary)
            win = [files[0][:short]] + [f for f in files[1:]]
            r = parser.batch(win[0], win[1] if nf > 1 else None, chunk_size=chunk, eof=(False, True))
            assert r["status"] == api.FQ_MORE and r["n_reads"] == 0 and "seqs" not in r, short
            r = parser.batch(win[0], win[1] if nf > 1 else None, chunk_size=chunk, eof=(True, True))
            assert r["status"] == api.FQ_DECLINED and r["declined_file"] == 0, short
            ends = [0] + [int(e) for e in PLAIN[name]["ends"][0]]
            assert r["declined_at"] == max(e for e in ends if e <= short), short
    # a window that ends on a record boundary before the cut: MORE without eof, the rest of the input with it
    one = PLAIN["cycle"]
    r = parser.batch(one["files"][0][:one["ends"][0][4]], chunk_size=1 << 20, eof=(False, True))
    assert r["status"] == api.FQ_MORE
    r = parser.batch(one["files"][0][:one["ends"][0][4]], chunk_size=1 << 20, eof=(True, True))
    assert r["status"] == api.FQ_END and r["n_reads"] == 5


# ---- the command line with BWAGPU_CLI_FASTQ=1 ---------------------------------------------------------------------------------------
TRACE = re.compile(rb"\[D::input\] (\d+) batches \((\d+) reads\) parsed on the device, (\d+) by the host reader")


def write_cli_inputs(tmp_path, g, n_pairs, seed):
    """two files of mates with comments and /1 /2 suffixes, and a copy of the first with one CRLF record in its second half"""
    from bwa_amd import simdata
    r1, r2 = simdata.make_reads_pe(g, n_pairs, seed=seed)
    a = simdata._ASCII
    paths = []
    for k, r in ((1, r1), (2, r2)):
        p = str(tmp_path / f"c{k}.fq")
        with open(p, "wb") as f:
            for i in range(n_pairs):
                q = bytes(33 + (j * 5 + i + k) % 41 for j in range(r.shape[1]))
                f.write(f"@p{i}/{k} BC:Z:ACGT{i}\tx\n".encode() + a[r[i]].tobytes() + b"\n+\n" + q + b"\n")
        paths.append(p)
    recs = open(paths[0], "rb").read().split(b"\n@")
    k = (2 * n_pairs) // 3
    recs[k] = recs[k].replace(b"\n", b"\r\n")
    irr = str(tmp_path / "irregular.fq")
    with open(irr, "wb") as f:
        f.write(b"\n@".join(recs))
    return paths[0], paths[1], irr


def run_cli(binary, args, env):
    """(SAM without @PG, (device batches, device reads, host batches) of the trace line or None)"""
    p = subprocess.run([binary, "mem"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    m = TRACE.search(p.stderr)
    return b"\n".join(l for l in p.stdout.split(b"\n") if not l.startswith(b"@PG")), tuple(int(x) for x in m.groups()) if m else None


def check_cli(cli, ref_bwa, args, env, irregular=False, n_reads=None):
    want, _ = run_cli(ref_bwa, args, None)
    got, tr = run_cli(cli, args, env)
    assert got == want, args
    assert tr is not None, "no [D::input] line"
    assert tr[0] > 0 and (tr[2] > 0) == irregular, tr
    if not irregular and n_reads is not None:
        assert tr[1] == n_reads, tr
    return tr
