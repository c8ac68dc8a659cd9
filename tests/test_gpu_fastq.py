"""GPU: the device FASTQ reader's kernels (bwa_amd/csrc/dev_fastq.h) on hardware -- the whole corpus of tests/fastq_cases.py against the
compiled reference's bseq_read (the mock runtime of the CPU tests runs lanes one at a time and cannot see wave-level errors), the window
property, and `bwa-amd mem` with BWAGPU_CLI_FASTQ=1 against the reference `bwa mem`."""
import os

import pytest

import fastq_cases
import refapi
import testdata
from bwa_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parser():
    assert refapi.have_ref(), "oracle/_ref (the compiled reference) is missing on the GPU box"
    p = api.FastqParser()
    yield p
    p.close()


def test_gpu_plain_corpus_equals_bseq_read(parser):
    for name, case in sorted(fastq_cases.plain_cases().items()):
        for chunk in fastq_cases.chunks_for(case):
            fastq_cases.run_plain(parser, case, chunk)


def test_gpu_irregular_corpus_declines_at_the_planted_record(parser):
    for name, case in sorted(fastq_cases.irregular_cases().items()):
        n_cut = {chunk: fastq_cases.run_irregular(parser, case, chunk) for chunk in (1, 150, 1 << 20)}
        assert n_cut[1 << 20] == 0 and (case["k"] < 2 or n_cut[1] > 0), name


def test_gpu_result_does_not_depend_on_the_window_length(parser):
    fastq_cases.run_windows(parser, fastq_cases.plain_cases())


@pytest.fixture(scope="module")
def cli_inputs(tmp_path_factory):
    assert refapi.have_ref(), "oracle/_ref (the compiled reference) is missing on the GPU box"
    from bwa_amd import build as b
    _, cli = b.build_host(verbose=False)
    prefix, g = testdata.small_index()
    n_pairs = 300
    f1, f2, irr = fastq_cases.write_cli_inputs(tmp_path_factory.mktemp("fastq_cli"), g, n_pairs, seed=831)
    return cli, prefix, f1, f2, n_pairs


def test_gpu_cli_fastq(cli_inputs):
    cli, prefix, f1, f2, n_pairs = cli_inputs
    env = dict(os.environ, BWAGPU_CLI_FASTQ="1", BWAGPU_CLI_TRACE="1")
    fastq_cases.check_cli(cli, refapi.REF_BWA, ["-K", "100000000", "-t", "4", "-C", prefix, f1, f2], env, n_reads=2 * n_pairs)


def test_gpu_cli_fastq_and_samtext(cli_inputs):
    cli, prefix, f1, f2, n_pairs = cli_inputs
    env = dict(os.environ, BWAGPU_CLI_FASTQ="1", BWAGPU_CLI_SAMTEXT="1", BWAGPU_CLI_TRACE="1")
    fastq_cases.check_cli(cli, refapi.REF_BWA, ["-K", "100000000", "-t", "4", "-C", prefix, f1, f2], env, n_reads=2 * n_pairs)


def test_gpu_cli_fastq_many_batches(cli_inputs):
    cli, prefix, f1, f2, n_pairs = cli_inputs
    env = dict(os.environ, BWAGPU_CLI_FASTQ="1", BWAGPU_CLI_TRACE="1")
    tr = fastq_cases.check_cli(cli, refapi.REF_BWA, ["-K", "3000", "-t", "4", prefix, f1, f2], env, n_reads=2 * n_pairs)
    assert tr[0] >= 20
