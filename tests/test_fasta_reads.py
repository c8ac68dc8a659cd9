"""CPU: the device reader for FASTA read files (bwagpu_fastq_batch_fasta*, bwa_amd/csrc/dev_fasta_reads.h) under the mock HIP runtime
against the compiled reference's own bseq_read / kseq_read (tests/fasta_reads_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import bgzf_cases
import fasta_reads_cases as cases
import refapi
from bwa_amd import api

pytestmark = pytest.mark.skipif(not refapi.have_ref(), reason="oracle/_ref not built")

REGULAR = cases.regular_cases()
IRREGULAR = cases.irregular_cases()


@pytest.fixture(scope="module")
def parser():
    import hostsim_build
    p = api.FastqParser(lib_path=hostsim_build.build())
    yield p
    p.close()


def test_the_corpus_sits_on_the_kernels_edges(parser):
    lim = parser.fasta_reads_limits()
    assert lim == {"tile_bytes": 8192, "lane_bytes": 32, "emit_step_bytes": 64}
    for edge in (lim["lane_bytes"] // 2, lim["lane_bytes"], lim["emit_step_bytes"]):
        assert {edge - 1, edge, edge + 1} <= set(cases.WIDTHS)
    assert len(REGULAR["cycle"]["files"][0]) > 4 * lim["tile_bytes"] and len(REGULAR["long"]["files"][0]) > 4 * lim["tile_bytes"]


@pytest.mark.parametrize("name", sorted(REGULAR))
def test_regular_batches_equal_bseq_read(parser, name):
    case = REGULAR[name]
    for chunk in cases.chunks_for(case):
        cases.run_regular(parser, case, chunk)


def test_an_empty_file_ends_with_no_read(parser):
    r = parser.batch_fasta(b"")
    assert r["status"] == api.FQ_END and r["n_reads"] == 0 and r["quals"] is None and list(r["off"]) == [0]


def test_sums_that_reach_the_chunk_at_an_odd_read_count(parser):
    case = REGULAR["odd_sums"]
    assert [len(b) for b in cases.ref_batches(case, 12)][:2] == [4, 2]
    r = parser.batch_fasta(case["files"][0], chunk_size=12)
    assert r["status"] == api.FQ_CUT and r["n_reads"] == 4 and r["consumed"][0] == case["ends"][0][3]


@pytest.mark.parametrize("name", sorted(IRREGULAR))
def test_irregular_record_declines_its_batch_and_no_other(parser, name):
    case = IRREGULAR[name]
    n_cut = {chunk: cases.run_irregular(parser, case, chunk) for chunk in (1, 150, 1 << 20)}
    assert n_cut[1 << 20] == 0
    if case["k"] >= 2:
        assert n_cut[1] > 0


def test_the_fastq_entry_point_still_declines_fasta(parser):
    r = parser.batch(REGULAR["cycle"]["files"][0], chunk_size=100)
    assert r["status"] == api.FQ_DECLINED and r["declined_at"] == 0
    r = parser.batch_fasta(b"@a\nACGT\n+\nIIII\n", chunk_size=100)
    assert r["status"] == api.FQ_DECLINED and r["declined_file"] == 0 and r["declined_at"] == 0
    r = parser.batch_fasta(b"\n>a\nACGT\n", chunk_size=100)      # a window starts at a '>'
    assert r["status"] == api.FQ_DECLINED and r["declined_at"] == 0


def test_result_does_not_depend_on_the_window_length(parser):
    cases.run_windows(parser, REGULAR)


def test_invalid_arguments(parser):
    EINVAL = -2
    o = api.FastqOut()
    buf = C.create_string_buffer(b">a\nAC\nG\n")
    ok = (buf, 8, 1, None, 0, 1, 100, C.byref(o))

    def with_(i, v):
        a = list(ok)
        a[i] = v
        return a

    assert parser.batch_fasta_rc(*ok) == 0 and o.status == api.FQ_END and o.n_reads == 1 and not o.quals
    parser.L.bwagpu_fastq_out_free(C.byref(o))
    assert parser.batch_fasta_rc(*with_(0, None)) == EINVAL                       # NULL window
    assert parser.batch_fasta_rc(*with_(7, None)) == EINVAL                       # NULL out
    assert parser.batch_fasta_rc(*with_(1, -1)) == EINVAL                         # negative length
    assert parser.batch_fasta_rc(*with_(4, -1)) == EINVAL
    assert parser.batch_fasta_rc(*with_(1, 1 << 31)) == EINVAL                    # a window of 2^31 bytes
    assert parser.batch_fasta_rc(*with_(6, 0)) == EINVAL and parser.batch_fasta_rc(*with_(6, -5)) == EINVAL   # chunk_size <= 0
    assert parser.batch_fasta_rc(*with_(4, 9)) == EINVAL                          # a length without a second window
    assert b"bwagpu_fastq_batch_fasta" in parser.L.bwagpu_fastq_last_error(parser.h)
    assert parser.L.bwagpu_fastq_batch_fasta(None, buf, 8, 1, None, 0, 1, 100, C.byref(o)) == EINVAL   # NULL parser
    comp = bgzf_cases.bgzf_file(b">a\nAC\nG\n", sizes=5)
    cb = np.frombuffer(comp, dtype=np.uint8)
    w = api.BgzfWin(cb.ctypes.data, len(comp), 0, 1)
    info = (api.BgzfInfo * 2)()
    assert parser.batch_fasta_bgzf_rc(C.byref(w), None, 100, C.byref(o), info) == 0 and o.status == api.FQ_END and o.n_reads == 1
    parser.L.bwagpu_fastq_out_free(C.byref(o))
    assert parser.batch_fasta_bgzf_rc(None, None, 100, C.byref(o), info) == EINVAL
    assert parser.batch_fasta_bgzf_rc(C.byref(w), None, 0, C.byref(o), info) == EINVAL
    assert parser.batch_fasta_bgzf_rc(C.byref(w), None, 100, None, info) == EINVAL
    assert parser.batch_fasta_bgzf_rc(C.byref(w), None, 100, C.byref(o), None) == EINVAL
    assert parser.batch_fasta_bgzf_rc(C.byref(api.BgzfWin(cb.ctypes.data, -1, 0, 1)), None, 100, C.byref(o), info) == EINVAL
    assert parser.batch_fasta_bgzf_rc(C.byref(api.BgzfWin(cb.ctypes.data, len(comp), -1, 1)), None, 100, C.byref(o), info) == EINVAL
    assert b"bwagpu_fastq_batch_fasta_bgzf" in parser.L.bwagpu_fastq_last_error(parser.h)
    assert parser.L.bwagpu_fastq_batch_fasta_bgzf(None, C.byref(w), None, 100, C.byref(o), info) == EINVAL
    assert parser.batch_fasta_rc(*ok) == 0 and o.n_reads == 1                     # the parser still works
    parser.L.bwagpu_fastq_out_free(C.byref(o))
    parser.L.bwagpu_fastq_out_free(C.byref(o))                                    # (idempotent)


# ---- BGZF ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sizes,chunk", [("cycle", 700, 1000), ("cycle", 0xff00, 150), ("long", 700, 20001), ("long", 0xff00, 7), ("pairs_cycle", 700, 700),
                                              ("pairs_cycle", 0xff00, 1 << 20)])
def test_bgzf_chain_equals_bseq_read(parser, name, sizes, chunk):
    case = REGULAR[name]
    comp = bgzf_cases.bgzf_case(case, sizes=sizes)
    bgzf_cases.run_chain(cases.AsFastq(parser), case, comp, chunk)
    n_more = bgzf_cases.run_chain(cases.AsFastq(parser), case, comp, chunk, window=200)      # windows that grow on MORE
    assert n_more > 0


def test_bgzf_damaged_block(parser):
    case = REGULAR["cycle"]
    comp = bytearray(bgzf_cases.bgzf_case(case, sizes=700)[0])
    first = bgzf_cases.block_len(bytes(comp))
    second = bgzf_cases.block_len(bytes(comp[first:]))
    comp[first + second - 6] ^= 0x10                                              # the second block's CRC-32
    r = parser.batch_fasta_bgzf(bytes(comp), chunk_size=1000)
    assert r["status"] == api.FQ_DAMAGED and r["n_reads"] == 0 and "seqs" not in r and r["bgzf"][0]["damaged_at"] == first


# ---- the command line: BWAGPU_CLI_FASTQ=1 BWAGPU_CLI_FASTA_DEV=1 ------------------------------------------------------------------------
def test_cli_fasta_switch_on_the_mock_runtime(tmp_path):
    import os
    import re
    import subprocess
    import fastq_cases
    import test_cli
    import testdata
    prefix, g = testdata.small_index()
    n_pairs = 14
    f1, f2, irr = cases.write_cli_inputs(tmp_path, g, n_pairs, seed=431)
    assert open(irr, "rb").read().count(b"\n@") == 1 and open(irr, "rb").read().count(b">") == n_pairs - 1
    cli = test_cli._sim_cli()
    env0 = dict(os.environ, BWAGPU_CLI_STREAMS="2", BWAGPU_CLI_SERIALIZE="1", BWAGPU_PTAB_M="6", BWAGPU_CLI_FASTQ="1", BWAGPU_CLI_TRACE="1")
    env = dict(env0, BWAGPU_CLI_FASTA_DEV="1")
    K = ["-K", "100000000", "-t", "2"]
    fastq_cases.check_cli(cli, refapi.REF_BWA, K + [prefix, f1], env, n_reads=n_pairs)                                     # single-end
    fastq_cases.check_cli(cli, refapi.REF_BWA, K + [prefix, f1, f2], env, n_reads=2 * n_pairs)                             # paired-end, two files
    fastq_cases.check_cli(cli, refapi.REF_BWA, K + ["-C", prefix, f1, f2], env, n_reads=2 * n_pairs)                       # comments
    tr = fastq_cases.check_cli(cli, refapi.REF_BWA, ["-K", "3000", "-t", "2", prefix, f1, f2], env, n_reads=2 * n_pairs)   # many batches
    assert tr[0] > 1
    fastq_cases.check_cli(cli, refapi.REF_BWA, ["-K", "1000", "-t", "2", "-C", prefix, irr], env, irregular=True)          # a FASTQ record in the middle: fallback
    # the text from the device as well: quals == NULL in bwagpu_sam_in_t
    env_t = dict(env, BWAGPU_CLI_SAMTEXT="1")
    for args in (["-K", "1000", "-t", "2", "-C", prefix, f1], ["-K", "3000", "-t", "2", "-C", prefix, f1, f2]):
        want, _ = fastq_cases.run_cli(refapi.REF_BWA, args, None)
        p = subprocess.run([cli, "mem"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env_t)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert b"\n".join(l for l in p.stdout.split(b"\n") if not l.startswith(b"@PG")) == want, args
        n_text = sum(int(x) for x, _ in re.findall(rb"(\d+) (reads|pairs) written from device SAM text", p.stderr))
        m = fastq_cases.TRACE.search(p.stderr)
        assert m and int(m.group(1)) > 0 and n_text > 0, p.stderr.decode()[-1500:]
    # without the new switch the same input never reaches the device reader's batches, and the output is the same
    for args in (K + [prefix, f1], K + ["-C", prefix, f1, f2]):
        want, _ = fastq_cases.run_cli(refapi.REF_BWA, args, None)
        got, tr = fastq_cases.run_cli(cli, args, env0)
        assert got == want and tr is not None and tr[0] == 0 and tr[2] > 0, tr
    # a FASTA file and a FASTQ file: the switch does not apply; -p stays with the host reader
    fq = str(tmp_path / "mate.fq")
    with open(fq, "wb") as f:
        for rec in open(f2, "rb").read().split(b">")[1:]:
            name, body = rec.split(b"\r\n", 1)
            seq = body.replace(b"\r\n", b"")
            f.write(b"@" + name + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n")
    want, _ = fastq_cases.run_cli(refapi.REF_BWA, K + [prefix, f1, fq], None)
    got, tr = fastq_cases.run_cli(cli, K + [prefix, f1, fq], env)
    assert got == want and tr is None
    _, tr = fastq_cases.run_cli(cli, K + ["-p", prefix, f1], env)
    assert tr is None
