"""CPU: `mem -p` on the device FASTQ reader (bwagpu_fastq_batch_smart*, bwa_amd/csrc/dev_fastq_smart.h) under the mock HIP runtime against the
compiled reference's own bseq_read + bseq_classify (tests/fastq_smart_cases.py), and `bwa-amd mem -p` with BWAGPU_CLI_FASTQ=1
BWAGPU_CLI_SMARTPE_DEV=1 against the reference `bwa mem -p`."""
import ctypes as C
import os
import re
import subprocess

import pytest

import bgzf_cases
import fastq_cases
import fastq_smart_cases as sc
import refapi
from bwa_amd import api

pytestmark = pytest.mark.skipif(not refapi.have_ref(), reason="oracle/_ref not built")

CASES = sc.cases()
IRREGULAR = {k: v for k, v in fastq_cases.irregular_cases().items() if k in ("crlf", "two_line_seq", "no_final_newline", "tab_in_bases")}


@pytest.fixture(scope="module")
def parser():
    import hostsim_build
    p = api.FastqParser(lib_path=hostsim_build.build())
    yield p
    p.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_batches_equal_bseq_read_and_bseq_classify(parser, name):
    for chunk in sc.CHUNKS:
        sc.run_smart(parser, CASES[name], chunk)


def test_the_corpus_holds_what_it_is_meant_to_hold():
    """the reference's own answers on the shapes the corpus is built around"""
    one = lambda name, chunk=1 << 20: sc.ref_smart(CASES[name], chunk)
    assert [b["cls"] for b in one("n1")] == [[0]] and [b["cls"] for b in one("n3_run")] == [[1, 2, 0]]
    assert one("runs_1_to_5")[0]["cls"][:15] == [0, 1, 2, 1, 2, 0, 1, 2, 1, 2, 1, 2, 1, 2, 0]
    assert one("trim_readno")[0]["cls"] == [1, 2, 0, 0, 1, 2, 0, 0, 1, 2, 0, 0, 1, 2, 0]            # x/1 x/2 pair; y/1 y/12 not; /1 /1 pair, /1 /2 not; v/1/2 v/1/1 lose one suffix only
    assert one("prefixes")[0]["cls"] == [0, 1, 2, 0, 1, 2, 0, 1, 2]
    assert one("long_names")[0]["cls"] == [1, 2, 0, 0, 0, 0, 0, 1, 2, 0, 1, 2, 0, 0]
    assert one("comments")[0]["cls"] == [1, 2, 1, 2, 1, 2, 0]
    assert one("nul_in_name")[0]["cls"] == [1, 2, 1, 2, 1, 2, 1, 2, 0, 0, 1, 2, 1, 2, 0, 1, 2]
    assert one("odd_last")[-1]["cls"][-1] == 0 and len(one("odd_last")[0]["recs"]) == 7
    # a cut inside a run: the three equal names r0 r0 r0 are pair + single in one batch, pair | single in batches of two
    assert one("cut_runs")[0]["cls"][:7] == [1, 2, 0, 1, 2, 1, 2]
    assert [b["cls"] for b in one("cut_runs", 7)][:4] == [[1, 2], [0, 0], [1, 2], [0, 0]]
    assert [b["cls"] for b in one("cut_runs", 150)][:2] == [[1, 2, 0, 0], [1, 2, 0, 0]]


def test_nul_in_a_name_compares_as_strcmp_and_the_name_is_kept_whole(parser):
    case = CASES["nul_in_name"]
    r = parser.batch_smart(case["files"][0], chunk_size=1 << 20)
    assert r["status"] == api.FQ_END and r["n_sub"] == (3, 14)
    names = [r["sub"][1]["names"][a:b] for a, b in zip(r["sub"][1]["name_off"][:-1], r["sub"][1]["name_off"][1:])]
    assert names[:6] == [b"a\0b", b"a\0c", b"ab\0", b"ab", b"ab", b"ab\0x"]


@pytest.mark.parametrize("name", sorted(IRREGULAR))
def test_irregular_record_declines_its_batch_and_no_other(parser, name):
    case = IRREGULAR[name]
    n_cut = {chunk: sc.run_irregular(parser, case, chunk) for chunk in (1, 150, 1 << 20)}
    assert n_cut[1 << 20] == 0
    if case["k"] >= 2:
        assert n_cut[1] > 0


def test_result_does_not_depend_on_the_window_length(parser):
    sc.run_windows(parser, CASES["runs_1_to_5"], 40)
    sc.run_windows(parser, CASES["cut_runs"], 150)
    # a window that ends on a record boundary before the cut: MORE without eof, the rest of the input with it
    case = CASES["all_pairs"]
    part = case["files"][0][:case["ends"][0][4]]
    assert parser.batch_smart(part, chunk_size=1 << 20, eof=False)["status"] == api.FQ_MORE
    r = parser.batch_smart(part, chunk_size=1 << 20, eof=True)
    assert r["status"] == api.FQ_END and r["n_reads"] == 5 and r["cls"].tolist() == [1, 2, 1, 2, 0]


def test_bgzf_windows(parser):
    for name in ("runs_1_to_5", "cut_runs", "comments", "all_single"):
        case = CASES[name]
        comp = bgzf_cases.bgzf_file(case["files"][0], 97, seed=3)      # blocks of 97 text bytes: batches start inside blocks
        for chunk in sc.CHUNKS:
            sc.run_smart_bgzf(parser, case, comp, chunk)
    case = CASES["cut_runs"]
    comp = bgzf_cases.bgzf_file(case["files"][0], 97, seed=3)
    r = parser.batch_smart_bgzf(comp[:40], chunk_size=150, eof=False)
    assert r["status"] == api.FQ_MORE and "cls" not in r
    damaged = bytearray(comp)
    damaged[bgzf_cases.block_len(comp) + 30] ^= 0x55      # in the second block's payload
    r = parser.batch_smart_bgzf(bytes(damaged), chunk_size=150)
    assert r["status"] == api.FQ_DAMAGED and r["bgzf"]["damaged_at"] == bgzf_cases.block_len(comp) and "cls" not in r


def test_invalid_arguments(parser):
    EINVAL = -2
    o = api.FastqSmart()
    buf = C.create_string_buffer(b"@a\nA\n+\nI\n@a\nC\n+\nI\n")
    ok = (buf, 18, 1, 100, C.byref(o))

    def with_(i, v):
        a = list(ok)
        a[i] = v
        return a

    assert parser.batch_smart_rc(*ok) == 0 and o.status == api.FQ_END and o.n_reads == 2 and tuple(o.n_sub) == (0, 2)
    parser.L.bwagpu_fastq_smart_free(C.byref(o))
    assert parser.batch_smart_rc(*with_(0, None)) == EINVAL                       # NULL window
    assert parser.batch_smart_rc(*with_(4, None)) == EINVAL                       # NULL out
    assert parser.batch_smart_rc(*with_(1, -1)) == EINVAL                         # negative length
    assert parser.batch_smart_rc(*with_(1, 1 << 31)) == EINVAL                    # a window of 2^31 bytes
    assert parser.batch_smart_rc(*with_(3, 0)) == EINVAL and parser.batch_smart_rc(*with_(3, -5)) == EINVAL   # chunk_size <= 0
    assert b"bwagpu_fastq_batch_smart" in parser.L.bwagpu_fastq_last_error(parser.h)
    assert parser.L.bwagpu_fastq_batch_smart(None, buf, 18, 1, 100, C.byref(o)) == EINVAL      # NULL parser
    # BGZF
    blk = bgzf_cases.block_of(b"@a\nA\n+\nI\n") + bgzf_cases.EOF_MARKER
    cb = C.create_string_buffer(blk, len(blk))
    info = api.BgzfInfo()
    w = api.BgzfWin(C.cast(cb, C.c_void_p).value, len(blk), 0, 1)
    assert parser.batch_smart_bgzf_rc(C.byref(w), 100, C.byref(o), C.byref(info)) == 0 and o.status == api.FQ_END and o.n_reads == 1 and tuple(o.n_sub) == (1, 0)
    parser.L.bwagpu_fastq_smart_free(C.byref(o))
    assert parser.batch_smart_bgzf_rc(None, 100, C.byref(o), C.byref(info)) == EINVAL
    assert parser.batch_smart_bgzf_rc(C.byref(w), 100, None, C.byref(info)) == EINVAL
    assert parser.batch_smart_bgzf_rc(C.byref(w), 100, C.byref(o), None) == EINVAL
    assert parser.batch_smart_bgzf_rc(C.byref(w), 0, C.byref(o), C.byref(info)) == EINVAL
    for bad in (api.BgzfWin(None, len(blk), 0, 1), api.BgzfWin(w.comp, -1, 0, 1), api.BgzfWin(w.comp, len(blk), -1, 1), api.BgzfWin(w.comp, len(blk), 10, 1)):
        assert parser.batch_smart_bgzf_rc(C.byref(bad), 100, C.byref(o), C.byref(info)) == EINVAL      # NULL comp, negative length / skip, skip beyond the first block's text
    assert parser.L.bwagpu_fastq_batch_smart_bgzf(None, C.byref(w), 100, C.byref(o), C.byref(info)) == EINVAL
    assert parser.batch_smart_rc(*ok) == 0 and o.n_reads == 2                     # the parser still works
    parser.L.bwagpu_fastq_smart_free(C.byref(o))
    parser.L.bwagpu_fastq_smart_free(C.byref(o))                                  # (idempotent)
    parser.L.bwagpu_fastq_smart_free(None)
    # the other calls still pass on the same parser
    fastq_cases.run_plain(parser, fastq_cases.plain_cases()["names"], 7)


# ---- the command line: BWAGPU_CLI_FASTQ=1 BWAGPU_CLI_SMARTPE_DEV=1 ---------------------------------------------------------------------
def test_cli_smartpe_switch_on_the_mock_runtime(tmp_path):
    import test_cli
    import testdata
    prefix, g = testdata.small_index()
    f = str(tmp_path / "inter.fq")
    n_reads = sc.write_interleaved(f, g, 14, {0, 5, 6, 13}, seed=433)
    assert n_reads == 32
    cli = test_cli._sim_cli()
    env = dict(os.environ, BWAGPU_CLI_STREAMS="2", BWAGPU_CLI_SERIALIZE="1", BWAGPU_PTAB_M="6", BWAGPU_CLI_FASTQ="1", BWAGPU_CLI_SMARTPE_DEV="1", BWAGPU_CLI_TRACE="1")
    big, small = ["-K", "100000000", "-t", "2"], ["-K", "1000", "-t", "2"]
    for args in (big + ["-p", prefix, f], big + ["-p", "-C", prefix, f], small + ["-p", prefix, f], small + ["-p", "-C", prefix, f]):
        tr = fastq_cases.check_cli(cli, refapi.REF_BWA, args, env, n_reads=n_reads)
        assert (tr[0] > 1) == (args[1] == "1000")
    # the second query file is ignored, with the reference's warning
    p = subprocess.run([cli, "mem"] + big + ["-p", prefix, f, f], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    want, _ = fastq_cases.run_cli(refapi.REF_BWA, big + ["-p", prefix, f, f], None)
    assert p.returncode == 0 and b"the second query file is ignored" in p.stderr and fastq_cases.TRACE.search(p.stderr)
    assert b"\n".join(l for l in p.stdout.split(b"\n") if not l.startswith(b"@PG")) == want
    # the text from the device as well: the sub-batches' blobs go to bwagpu_batch_sam / bwagpu_batch_sam_pe as they are
    env_t = dict(env, BWAGPU_CLI_SAMTEXT="1")
    args = small + ["-p", "-C", prefix, f]
    want, _ = fastq_cases.run_cli(refapi.REF_BWA, args, None)
    p = subprocess.run([cli, "mem"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env_t)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert b"\n".join(l for l in p.stdout.split(b"\n") if not l.startswith(b"@PG")) == want
    n_text = {kind: int(x) for x, kind in re.findall(rb"(\d+) (reads|pairs) written from device SAM text", p.stderr)}
    assert fastq_cases.TRACE.search(p.stderr) and n_text[b"reads"] > 0 and n_text[b"pairs"] > 0, p.stderr.decode()[-1500:]
    # a BGZF copy, inflated on the device: blocks of 700 text bytes, every batch of -K 1000 starts inside one
    z = bgzf_cases.write_bgzf(f + ".gz", open(f, "rb").read(), 700)
    fastq_cases.check_cli(cli, refapi.REF_BWA, small + ["-p", "-C", prefix, z], dict(env, BWAGPU_CLI_BGZF_DEV="1"), n_reads=n_reads)
    _, tr = fastq_cases.run_cli(cli, small + ["-p", prefix, z], env)      # (without BWAGPU_CLI_BGZF_DEV the BGZF file stays with the host reader)
    assert tr is None
    # an irregular record in the middle: the streaming reader takes over from that batch's start
    recs = open(f, "rb").read().split(b"\n@")
    recs[20] = recs[20].replace(b"\n", b"\r\n")
    irr = str(tmp_path / "irregular.fq")
    open(irr, "wb").write(b"\n@".join(recs))
    fastq_cases.check_cli(cli, refapi.REF_BWA, small + ["-p", "-C", prefix, irr], env, irregular=True)
    # the new switch alone changes nothing, and BWAGPU_CLI_FASTQ=1 alone still leaves -p to the host reader
    _, tr = fastq_cases.run_cli(cli, big + ["-p", prefix, f], dict(env, BWAGPU_CLI_FASTQ="0"))
    assert tr is None
    _, tr = fastq_cases.run_cli(cli, big + ["-p", prefix, f], dict(env, BWAGPU_CLI_SMARTPE_DEV="0"))
    assert tr is None
