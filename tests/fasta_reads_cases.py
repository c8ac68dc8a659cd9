"""FASTA read files for the device FASTA reader's tests (tests/test_fasta_reads.py, tests/test_gpu_fasta_reads.py).  The expected batches
are the compiled reference's own kseq_read / bseq_read through fastq_cases.ref_batches, never the code under test.

A case is fastq_cases' dict: files (one or two byte strings), ends (per file: the byte offset behind every record as the generator wrote
it -- empty lines behind a record's bases belong to it) and, for an irregular case, k / file / at: the record the device declines, the
file it is in and its byte offset there."""
import numpy as np

import fastq_cases
from fastq_cases import ref_batches, chunks_for      # noqa: F401  (the tests take them from here)

# the edges of the kernels' steps (bwagpu_fasta_reads_limits: 8192-byte tiles, 32 bytes per lane, 64 body bytes per emit step)
WIDTHS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128)


def _acgt(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def _wrap(seq: bytes, widths, eol=b"\n", last_eol=None) -> bytes:
    """seq cut into lines of widths[0], widths[1], ... (cycling), each ended by eol (the last one by last_eol if given)"""
    out, o, i = [], 0, 0
    widths = (widths,) if isinstance(widths, int) else tuple(widths)
    while o < len(seq):
        w = widths[i % len(widths)]
        out.append(seq[o:o + w])
        o += w
        i += 1
    body = eol.join(out)
    return body + (eol if last_eol is None else last_eol)


def _fa(name: bytes, seq: bytes, widths=60, eol=b"\n", hdr_eol=None, last_eol=None) -> bytes:
    return b">" + name + (eol if hdr_eol is None else hdr_eol) + _wrap(seq, widths, eol, last_eol)


def _case(*files):
    """files: lists of record byte strings"""
    return {"files": [b"".join(f) for f in files], "ends": [[int(x) for x in np.cumsum([len(r) for r in f])] for f in files]}


def _cycle(rng, n, tag=b"", eol=b"\n", w0=0, name0=0):
    """n records of 1 .. 4 lines, line widths cycling 1 .. 70, names of 1 .. 40 bytes: line starts at every offset mod 16 and across the tile edges"""
    out, w = [], w0
    for i in range(n):
        n_lines = 1 + i % 4
        widths = [1 + (w + j) % 70 for j in range(n_lines)]
        w += n_lines
        last = 1 + (i * 7) % widths[-1]                      # the last line is not always full
        name = (tag + b"%d" % i + b"n" * 40)[:1 + (i + name0) % 40]
        out.append(_fa(name + (b" c%d" % i if i % 3 == 0 else b""), _acgt(rng, sum(widths[:-1]) + last), widths, eol))
    return out


NAMES = (b"a/1", b"/1", b"ab/x", b"r/12", b"r/1/2", b"r/1 /2", b"xy/9", b"//7", b"")                       # fastq_cases.plain_cases' lists
HEADERS = (b"nodelim", b"empty_comment ", b"tab\tcomment here", b"blanks   three  blanks ", b"vt\x0bv\x0cw", b"cr\rmid", b" noname", b"s/1 c/2", b"last")


def regular_cases():
    """cases the device never declines"""
    rng = np.random.default_rng(811)
    c = {}
    c["cycle"] = _case(_cycle(rng, 400))
    c["widths"] = _case([_fa(b"w%d" % w, _acgt(rng, 200), w) for w in WIDTHS])
    c["long"] = _case([_fa(b"wrapped 20000/60", _acgt(rng, 20000), 60), _fa(b"unwrapped", _acgt(rng, 20000), 20000), _fa(b"tail", _acgt(rng, 70), 60)])
    c["crlf"] = _case(_cycle(rng, 120, eol=b"\r\n") + [_fa(b"blank_then_cr ", b"ACGTAC", 4, b"\r\n"), _fa(b"nocomment", b"A", 1, b"\r\n")])
    c["crlf_mixed"] = _case([_fa(b"h%d c" % i, _acgt(rng, 50 + i), 17, b"\n", hdr_eol=b"\r\n") for i in range(6)] +
                            [_fa(b"s%d" % i, _acgt(rng, 50 + i), (16, 1, 31), b"\r\n", hdr_eol=b"\n") for i in range(6)])
    s = _acgt(rng, 40)
    c["blank_lines"] = _case([_fa(b"b0", s, 10) + b"\n", _fa(b"b1 c", s, 10) + b"\n\n\n", b">b2\n\n" + _wrap(s, 10), b">b3\n" + s[:10] + b"\n\n\n" + s[10:] + b"\n",
                              _fa(b"b4", s, 7, b"\r\n") + b"\r\n", b">b5\r\n" + s[:9] + b"\r\n\r\n" + s[9:] + b"\r\n\r\n\r\n",      # a "\r"-only line behind a base adds nothing
                              _fa(b"b6", s, 40) + b"\n\n\n\n"])
    for tag, tail in (("lf_one", b"AC\nG"), ("lf_several", b"AC\nGTTCA"), ("crlf_one", b"AC\r\nG"), ("crlf_several", b"AC\r\nGTTCA"), ("cr_without_lf", b"AC\r\nGTT\r")):
        eol = b"\n" if tag.startswith("lf") else b"\r\n"
        c["no_final_newline_" + tag] = _case([_fa(b"n%d c" % i, _acgt(rng, 30 + i), 11, eol) for i in range(5)] + [b">last x" + eol + tail])
    c["names"] = _case([_fa(n, _acgt(rng, 9), 4) for n in NAMES])
    c["headers"] = _case([_fa(h, b"ACGT") for h in HEADERS])
    c["headers_crlf"] = _case([_fa(h, b"ACGT", eol=b"\r\n") for h in HEADERS])
    c["bases"] = _case([_fa(b"lower", b"acgtacgtnn", 3), _fa(b"iupac", b"RYKMSWBDHVNrykmswbdhvn", 5), _fa(b"dash", b"AC-GT--a-", 2), _fa(b"mixed", b"AcGtNn-.*xX", 4),
                        _fa(b"d1", b"-"), _fa(b"allbytes", bytes(range(0x21, 0x80)).replace(b">", b"").replace(b"@", b"").replace(b"+", b""), 13)])
    c["one_record"] = _case([_fa(b"only", b"ACGTACGTAC", 4)])
    c["one_base"] = _case([_fa(b"b", b"A")])
    c["empty"] = _case([])
    c["odd_sums"] = _case([_fa(b"o%d" % i, _acgt(rng, 3 + i), 2) for i in range(9)])
    c["pairs_cycle"] = _case(_cycle(rng, 150, b"p"), _cycle(rng, 150, b"p", w0=23, name0=5))
    c["pairs_diff"] = _case([_fa(b"m%d/1" % i, _acgt(rng, 30 + i % 7), 60) for i in range(40)],
                            [_fa(b"m%d/2 second" % i, _acgt(rng, 3 + (5 * i) % 50), (7, 3), b"\r\n") for i in range(40)])
    c["pairs_one"] = _case([_fa(b"a/1", b"ACG")], [_fa(b"a/2", b"TTTTT", 2)])
    return c


def irregular_cases():
    """exactly one irregularity each, at record k of file `file`"""
    rng = np.random.default_rng(812)

    def base(n=30, tag=b"r"):
        return [_fa(tag + b"%d c" % i, _acgt(rng, 20 + i % 11), 9) for i in range(n)]

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
    c["fastq_record"] = planted(17, b"@fq c\n" + s + b"\n+\n" + b"I" * 24 + b"\n")
    c["plus_line"] = planted(11, b">pl\n" + s[:10] + b"\n+\n" + s[10:] + b"\n")
    c["header_header"] = planted(13, b">nobases c\n")
    c["header_blank_header"] = planted(6, b">nobases\n\n\n")
    c["blank_in_bases"] = planted(14, _fa(b"bl", s[:7] + b" " + s[8:], 10))
    c["tab_in_bases"] = planted(0, _fa(b"tb", s[:17] + b"\t" + s[18:], 10))
    c["high_byte"] = planted(21, _fa(b"hb", s[:5] + b"\xc3" + s[6:], 10))
    c["nul_byte"] = planted(9, _fa(b"nu", s[:15] + b"\x00" + s[16:], 10))
    c["nul_line_start"] = planted(4, b">n0\n" + s[:10] + b"\n\x00" + s[11:] + b"\n")
    for name in ("nul_byte", "nul_line_start"):
        c[name]["ref_files"] = [c[name]["files"][0][:c[name]["at"]]]
    c["cr_mid_line"] = planted(8, b">cm\n" + s[:5] + b"\r" + s[6:] + b"\n")
    c["gt_last_byte"] = planted(29, b">", drop_after=True)
    c["starts_with_at"] = planted(0, b"@fq0\n" + s + b"\n+\n" + b"I" * 24 + b"\n")
    # the corner shapes the rule declines (dev_fasta_reads.h): a line that is only "\r" as its record's first sequence line, and as the stream's last line
    c["cr_line_first"] = planted(12, b">cf\n\r\n" + s + b"\n")
    c["cr_line_first_behind_blank"] = planted(5, b">cf\r\n\n\r\n" + s + b"\r\n")
    c["cr_line_last"] = planted(20, b">cl\n" + s + b"\n\r", drop_after=True)
    c["pair_bad_in_2"] = planted(7, b">p7 c\n" + s[:9] + b"\n+\n", files=[base(20, b"p"), base(20, b"p")], file=1)
    c["pair_bad_in_1"] = planted(15, _fa(b"sp", s[:3] + b" " + s[4:]), files=[base(20, b"p"), base(20, b"p")], file=0)
    c["pair_second_is_fastq"] = planted(0, b"@fq0\n" + s + b"\n+\n" + b"I" * 24 + b"\n", files=[base(10, b"p"), base(10, b"p")], file=1)
    f1, f2 = base(20, b"p"), base(19, b"p")
    c["pair_2_short"] = _case(f1, f2)
    c["pair_2_short"].update(k=19, file=0, at=int(c["pair_2_short"]["ends"][0][18]))
    f1, f2 = base(18, b"p"), base(20, b"p")
    c["pair_1_short"] = _case(f1, f2)
    c["pair_1_short"].update(k=18, file=1, at=int(c["pair_1_short"]["ends"][1][17]))
    return c


# ---- the device's batch, in the reference's terms ----------------------------------------------------------------------------------
class _NoQuals:
    """quals of a FASTA batch for fastq_cases.device_records: every read's slice is None, as bseq_read leaves qual"""
    def __getitem__(self, _):
        return None


def device_records(r):
    assert r["quals"] is None
    return fastq_cases.device_records(dict(r, quals=_NoQuals()))


class AsFastq:
    """a FastqParser whose batch / batch_bgzf are the FASTA calls, for the runners of fastq_cases and bgzf_cases that compare through device_records"""
    def __init__(self, parser):
        self.p = parser

    def batch(self, *a, **kw):
        r = self.p.batch_fasta(*a, **kw)
        if "seqs" in r:
            assert r["quals"] is None
            r["quals"] = _NoQuals()
        return r

    def batch_bgzf(self, *a, **kw):
        r = self.p.batch_fasta_bgzf(*a, **kw)
        if "seqs" in r:
            assert r["quals"] is None
            r["quals"] = _NoQuals()
        return r


_NT4 = None


def check_recs(r, windows):
    """the record table against the arrays: every field is the window's bytes at the recorded place; the bases are the window's bytes from
    seq on with '\\n' and '\\r' removed, recoded"""
    global _NT4
    if _NT4 is None:
        _NT4 = np.frombuffer(fastq_cases._reflib()[2], dtype=np.uint8)
    for i in range(r["n_reads"]):
        e = r["recs"][i]
        w = windows[int(e["file"])]
        assert int(e["file"]) == (i % len(windows) if len(windows) > 1 else 0)
        assert w[e["name"]:e["name"] + e["l_name"]] == r["names"][r["name_off"][i]:r["name_off"][i + 1]]
        assert w[e["comment"]:e["comment"] + e["l_comment"]] == r["comments"][r["comment_off"][i]:r["comment_off"][i + 1]]
        assert e["qual"] == -1 and e["l_qual"] == 0 and int(e["has_comment"]) == int(r["has_comment"][i])
        ls = int(e["l_seq"])
        assert ls == r["off"][i + 1] - r["off"][i] and ls > 0
        assert w[e["seq"]] not in b"\r\n" and w[e["seq"] - 1] in b"\n"
        body = w[e["seq"]:e["seq"] + 4 * ls + 64].replace(b"\n", b"").replace(b"\r", b"")[:ls]      # (the corpus has no read with more line ends than that)
        assert len(body) == ls and np.array_equal(_NT4[np.frombuffer(body, dtype=np.uint8)], r["seqs"][r["off"][i]:r["off"][i + 1]])


def run_regular(parser, case, chunk):
    """the device's batches over a regular case, the whole rest of each file as the window: bseq_read's, consumed at the generator's record
    ends, END last"""
    from bwa_amd import api
    want = ref_batches(case, chunk)
    files, nf = case["files"], len(case["files"])
    pos, taken = [0] * nf, 0
    for bi in range(len(want) + 1):
        win = [f[p:] for f, p in zip(files, pos)]
        r = parser.batch_fasta(win[0], win[1] if nf > 1 else None, chunk_size=chunk)
        assert r["status"] in (api.FQ_CUT, api.FQ_END), (bi, r["status"], r["declined_file"], r["declined_at"])
        if bi == len(want):
            assert r["status"] == api.FQ_END and r["n_reads"] == 0
            break
        assert device_records(r) == want[bi], f"batch {bi}"
        check_recs(r, win)
        taken += r["n_reads"]
        for k in range(nf):
            n_k = taken // nf
            assert pos[k] + r["consumed"][k] == (case["ends"][k][n_k - 1] if n_k else 0), f"consumed, batch {bi}, file {k}"
            pos[k] += r["consumed"][k]
        if r["status"] == api.FQ_END:
            assert bi == len(want) - 1
            break
    assert all(p == len(f) for p, f in zip(pos, files))


def run_irregular(parser, case, chunk):
    """every batch bseq_read closes by its own rule before record k equals the device's; the batch that holds k is declined at k.  Returns
    the number of batches before it.  (ref_files: what the reference reads where record k holds a NUL, which fastq_cases' reader of the
    reference's C strings cannot take: the file up to record k -- the batches closed before k are the same)"""
    from bwa_amd import api
    want = ref_batches({"files": case.get("ref_files", case["files"])}, chunk)
    files, nf = case["files"], len(case["files"])
    pos, taken = [0] * nf, 0
    n_cut = 0
    for bi in range(len(want) + 1):
        win = [f[p:] for f, p in zip(files, pos)]
        r = parser.batch_fasta(win[0], win[1] if nf > 1 else None, chunk_size=chunk)
        b = want[bi] if bi < len(want) else None
        whole = b is not None and (taken + len(b)) // nf <= case["k"] and len(b) % 2 == 0 and sum(len(x[2]) for x in b) >= chunk
        if not whole:
            assert r["status"] == api.FQ_DECLINED and r["n_reads"] == 0 and "seqs" not in r, (bi, r["status"])
            assert r["declined_file"] == case["file"] and pos[case["file"]] + r["declined_at"] == case["at"], (r["declined_file"], r["declined_at"], pos, case["at"])
            return n_cut
        assert r["status"] == api.FQ_CUT and device_records(r) == b, f"batch {bi}"
        check_recs(r, win)
        n_cut += 1
        taken += r["n_reads"]
        for k in range(nf):
            pos[k] += r["consumed"][k]
    raise AssertionError("the device never declined")


def run_windows(parser, REGULAR):
    """the result does not depend on the window length once the window shows the end of the batch's last record -- the first byte of the
    next header; a window without eof that stops short of it gives MORE"""
    from bwa_amd import api
    rng = np.random.default_rng(5)
    for name, chunk in (("cycle", 1000), ("pairs_cycle", 700), ("long", 20001), ("crlf", 500)):
        files = REGULAR[name]["files"]
        nf = len(files)
        whole = parser.batch_fasta(files[0], files[1] if nf > 1 else None, chunk_size=chunk)
        assert whole["status"] == api.FQ_CUT
        for it in range(12):
            lens = [whole["consumed"][k] + 1 if it == 0 else int(rng.integers(whole["consumed"][k] + 1, len(files[k]) + 1)) for k in range(nf)]
            win = [f[:n] for f, n in zip(files, lens)]
            r = parser.batch_fasta(win[0], win[1] if nf > 1 else None, chunk_size=chunk, eof=tuple(n == len(f) for n, f in zip(lens, files)) + (True,) * (2 - nf))
            assert r["status"] == api.FQ_CUT and r["consumed"] == whole["consumed"], lens
            for k in ("seqs", "off", "name_off", "comment_off", "has_comment", "recs"):
                assert np.array_equal(r[k], whole[k]), (k, lens)
            assert (r["names"], r["comments"], r["quals"]) == (whole["names"], whole["comments"], None)
        # windows that stop short: at the end of the last record's text (its end is not in view), in the middle of a line, in its header
        ends = [0] + REGULAR[name]["ends"][0]
        for short in (whole["consumed"][0], whole["consumed"][0] - 3, whole["consumed"][0] // 2 + 1, 1):
            win = [files[0][:short]] + [f for f in files[1:]]
            r = parser.batch_fasta(win[0], win[1] if nf > 1 else None, chunk_size=chunk, eof=(False, True))
            assert r["status"] == api.FQ_MORE and r["n_reads"] == 0 and "seqs" not in r, short
    # a window that ends on a record boundary before the cut: MORE without eof, the rest of the input with it
    one = REGULAR["cycle"]
    r = parser.batch_fasta(one["files"][0][:one["ends"][0][4]], chunk_size=1 << 20, eof=(False, True))
    assert r["status"] == api.FQ_MORE
    r = parser.batch_fasta(one["files"][0][:one["ends"][0][4]], chunk_size=1 << 20, eof=(True, True))
    assert r["status"] == api.FQ_END and r["n_reads"] == 5 and r["consumed"][0] == one["ends"][0][4]
    # a header cut off at eof has no bases: declined at its offset
    r = parser.batch_fasta(one["files"][0][:one["ends"][0][4] + 3], chunk_size=1 << 20, eof=(True, True))
    assert r["status"] == api.FQ_DECLINED and r["declined_file"] == 0 and r["declined_at"] == one["ends"][0][4]


# ---- the command line with BWAGPU_CLI_FASTQ=1 BWAGPU_CLI_FASTA_DEV=1 ------------------------------------------------------------------
def write_fasta_reads(path, reads, names, widths=60, eol=b"\n"):
    """reads: rows of nt4 codes (or a list of rows of different lengths), written as wrapped FASTA"""
    from bwa_amd import simdata
    with open(path, "wb") as f:
        for r, name in zip(reads, names):
            f.write(_fa(name, simdata._ASCII[np.asarray(r)].tobytes(), widths, eol))
    return path


def write_cli_inputs(tmp_path, g, n_pairs, seed):
    """two FASTA files of mates with comments and /1 /2 suffixes, wrapped differently, and a copy of the first with a FASTQ record in its second half"""
    from bwa_amd import simdata
    r1, r2 = simdata.make_reads_pe(g, n_pairs, seed=seed)
    f1 = write_fasta_reads(str(tmp_path / "c1.fa"), r1, [f"p{i}/1 BC:Z:ACGT{i}\tx".encode() for i in range(n_pairs)], 60)
    f2 = write_fasta_reads(str(tmp_path / "c2.fa"), r2, [f"p{i}/2 BC:Z:ACGT{i}\tx".encode() for i in range(n_pairs)], (70, 33, 1), b"\r\n")
    recs = open(f1, "rb").read().split(b"\n>")
    k = (2 * n_pairs) // 3
    name, body = recs[k].split(b"\n", 1)
    seq = body.replace(b"\n", b"")
    irr = str(tmp_path / "irregular.fa")
    with open(irr, "wb") as f:
        f.write(b"\n>".join(recs[:k]) + b"\n@" + name + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n>" + b"\n>".join(recs[k + 1:]))
    return f1, f2, irr
