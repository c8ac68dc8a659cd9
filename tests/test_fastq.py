"""CPU: the device FASTQ reader (bwagpu_fastq_*, bwa_amd/csrc/dev_fastq.h) under the mock HIP runtime against the compiled reference's own
bseq_read / kseq_read (tests/fastq_cases.py), and `bwa-amd mem` with BWAGPU_CLI_FASTQ=1 against the reference `bwa mem`."""
import ctypes as C
import os
import re
import subprocess

import pytest

import fastq_cases
import refapi
from bwa_amd import api

pytestmark = pytest.mark.skipif(not refapi.have_ref(), reason="oracle/_ref not built")

PLAIN = fastq_cases.plain_cases()
IRREGULAR = fastq_cases.irregular_cases()


@pytest.fixture(scope="module")
def parser():
    import hostsim_build
    p = api.FastqParser(lib_path=hostsim_build.build())
    yield p
    p.close()


@pytest.mark.parametrize("name", sorted(PLAIN))
def test_plain_batches_equal_bseq_read(parser, name):
    case = PLAIN[name]
    for chunk in fastq_cases.chunks_for(case):
        fastq_cases.run_plain(parser, case, chunk)


def test_sums_that_reach_the_chunk_at_an_odd_read_count(parser):
    """reads of 3, 4, 5, ... bases and a chunk of 12: the sum is 12 after three reads, the batch closes after four (bwa.c:104)"""
    case = PLAIN["odd_sums"]
    assert [len(b) for b in fastq_cases.ref_batches(case, 12)][:2] == [4, 2]
    r = parser.batch(case["files"][0], chunk_size=12)
    assert r["status"] == api.FQ_CUT and r["n_reads"] == 4 and r["consumed"][0] == case["ends"][0][3]
    fastq_cases.run_plain(parser, case, 12)


@pytest.mark.parametrize("name", sorted(IRREGULAR))
def test_irregular_record_declines_its_batch_and_no_other(parser, name):
    case = IRREGULAR[name]
    n_cut = {chunk: fastq_cases.run_irregular(parser, case, chunk) for chunk in (1, 150, 1 << 20)}
    assert n_cut[1 << 20] == 0
    if case["k"] >= 2:
        assert n_cut[1] > 0      # the whole rest of the file was the window: the non-plain record lay behind those cuts


def test_result_does_not_depend_on_the_window_length(parser):
    fastq_cases.run_windows(parser, PLAIN)


def test_reserve_and_reuse(parser):
    parser.reserve(1 << 16)
    fastq_cases.run_plain(parser, PLAIN["cycle"], 150)
    fastq_cases.run_plain(parser, PLAIN["pairs_one"], 150)


def test_invalid_arguments(parser):
    EINVAL = -2
    assert parser.L.bwagpu_strerror(EINVAL) and b"argument" in parser.L.bwagpu_strerror(EINVAL).lower()
    o = api.FastqOut()
    buf = C.create_string_buffer(b"@a\nA\n+\nI\n")
    ok = (buf, 9, 1, None, 0, 1, 100, C.byref(o))

    def with_(i, v):
        a = list(ok)
        a[i] = v
        return a

    assert parser.batch_rc(*ok) == 0 and o.status == api.FQ_END and o.n_reads == 1
    parser.L.bwagpu_fastq_out_free(C.byref(o))
    assert parser.batch_rc(*with_(0, None)) == EINVAL                       # NULL window
    assert parser.batch_rc(*with_(7, None)) == EINVAL                       # NULL out
    assert parser.batch_rc(*with_(1, -1)) == EINVAL                         # negative length
    assert parser.batch_rc(*with_(4, -1)) == EINVAL
    assert parser.batch_rc(*with_(1, 1 << 31)) == EINVAL                    # a window of 2^31 bytes
    assert parser.batch_rc(*with_(6, 0)) == EINVAL and parser.batch_rc(*with_(6, -5)) == EINVAL   # chunk_size <= 0
    assert parser.batch_rc(*with_(4, 9)) == EINVAL                          # a length without a second window
    assert b"bwagpu_fastq_batch" in parser.L.bwagpu_fastq_last_error(parser.h)
    assert parser.L.bwagpu_fastq_batch(None, buf, 9, 1, None, 0, 1, 100, C.byref(o)) == EINVAL   # NULL parser
    assert parser.L.bwagpu_fastq_reserve(parser.h, -1) == EINVAL and parser.L.bwagpu_fastq_reserve(None, 10) == EINVAL
    assert parser.L.bwagpu_fastq_begin(None, 0, None, 0) == EINVAL
    assert parser.batch_rc(*ok) == 0 and o.n_reads == 1                     # the parser still works
    parser.L.bwagpu_fastq_out_free(C.byref(o))
    parser.L.bwagpu_fastq_out_free(C.byref(o))                              # (idempotent)
    parser.L.bwagpu_fastq_out_free(None)


# ---- the command line: BWAGPU_CLI_FASTQ=1 --------------------------------------------------------------------------------------------
def test_cli_fastq_switch_on_the_mock_runtime(tmp_path):
    import test_cli
    import testdata
    prefix, g = testdata.small_index()
    n_pairs = 14
    f1, f2, irr = fastq_cases.write_cli_inputs(tmp_path, g, n_pairs, seed=431)
    cli = test_cli._sim_cli()
    env = dict(os.environ, BWAGPU_CLI_STREAMS="2", BWAGPU_CLI_SERIALIZE="1", BWAGPU_PTAB_M="6", BWAGPU_CLI_FASTQ="1", BWAGPU_CLI_TRACE="1")
    K = ["-K", "100000000", "-t", "2"]
    fastq_cases.check_cli(cli, refapi.REF_BWA, K + [prefix, f1], env, n_reads=n_pairs)                                     # single-end
    fastq_cases.check_cli(cli, refapi.REF_BWA, K + [prefix, f1, f2], env, n_reads=2 * n_pairs)                             # paired-end, two files
    fastq_cases.check_cli(cli, refapi.REF_BWA, K + ["-C", prefix, f1, f2], env, n_reads=2 * n_pairs)                       # comments
    tr = fastq_cases.check_cli(cli, refapi.REF_BWA, ["-K", "3000", "-t", "2", prefix, f1, f2], env, n_reads=2 * n_pairs)   # many batches
    assert tr[0] > 1
    fastq_cases.check_cli(cli, refapi.REF_BWA, ["-K", "1000", "-t", "2", "-C", prefix, irr], env, irregular=True)          # fallback in the middle of the run
    # the text from the device as well: the parse's blobs go to bwagpu_batch_sam / bwagpu_batch_sam_pe as they are
    env_t = dict(env, BWAGPU_CLI_SAMTEXT="1")
    for args in (["-K", "1000", "-t", "2", "-C", prefix, f1], ["-K", "3000", "-t", "2", "-C", prefix, f1, f2]):
        want, _ = fastq_cases.run_cli(refapi.REF_BWA, args, None)
        p = subprocess.run([cli, "mem"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env_t)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert b"\n".join(l for l in p.stdout.split(b"\n") if not l.startswith(b"@PG")) == want, args
        n_text = sum(int(x) for x, _ in re.findall(rb"(\d+) (reads|pairs) written from device SAM text", p.stderr))
        assert fastq_cases.TRACE.search(p.stderr) and n_text > 0, p.stderr.decode()[-1500:]
    # the switch does not apply: -p, and gzip input
    _, tr = fastq_cases.run_cli(cli, K + ["-p", prefix, f1], env)
    assert tr is None
