"""GPU: the device reader for FASTA read files (bwa_amd/csrc/dev_fasta_reads.h) on hardware -- the whole corpus of
tests/fasta_reads_cases.py against the compiled reference's bseq_read (the mock runtime of the CPU tests runs lanes one at a time and cannot
see a wrong ballot or scan), the window property, the BGZF chain, and `bwa-amd mem` with BWAGPU_CLI_FASTQ=1 BWAGPU_CLI_FASTA_DEV=1 against
the reference `bwa mem`."""
import os

import numpy as np
import pytest

import bgzf_cases
import fasta_reads_cases as cases
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


def test_gpu_regular_corpus_equals_bseq_read(parser):
    for name, case in sorted(cases.regular_cases().items()):
        for chunk in cases.chunks_for(case):
            cases.run_regular(parser, case, chunk)


def test_gpu_irregular_corpus_declines_at_the_planted_record(parser):
    for name, case in sorted(cases.irregular_cases().items()):
        n_cut = {chunk: cases.run_irregular(parser, case, chunk) for chunk in (1, 150, 1 << 20)}
        assert n_cut[1 << 20] == 0 and (case["k"] < 2 or n_cut[1] > 0), name


def test_gpu_result_does_not_depend_on_the_window_length(parser):
    cases.run_windows(parser, cases.regular_cases())


@pytest.mark.parametrize("name,sizes,chunk", [("cycle", 700, 1000), ("cycle", 0xff00, 150), ("long", 700, 20001), ("long", 0xff00, 7)])
def test_gpu_bgzf_chain_equals_bseq_read(parser, name, sizes, chunk):
    case = cases.regular_cases()[name]
    comp = bgzf_cases.bgzf_case(case, sizes=sizes)
    bgzf_cases.run_chain(cases.AsFastq(parser), case, comp, chunk)
    assert bgzf_cases.run_chain(cases.AsFastq(parser), case, comp, chunk, window=200) > 0      # windows that grow on MORE


@pytest.fixture(scope="module")
def cli_inputs(tmp_path_factory):
    assert refapi.have_ref(), "oracle/_ref (the compiled reference) is missing on the GPU box"
    from bwa_amd import build as b
    _, cli = b.build_host(verbose=False)
    prefix, g = testdata.small_index()
    n_pairs = 300
    f1, f2, _ = cases.write_cli_inputs(tmp_path_factory.mktemp("fasta_cli"), g, n_pairs, seed=832)
    return cli, prefix, f1, f2, n_pairs


ENV = dict(BWAGPU_CLI_FASTQ="1", BWAGPU_CLI_FASTA_DEV="1", BWAGPU_CLI_TRACE="1")


@pytest.mark.parametrize("samtext", [False, True])
def test_gpu_cli_fasta_one_batch(cli_inputs, samtext):
    cli, prefix, f1, f2, n_pairs = cli_inputs
    env = dict(os.environ, **ENV, **({"BWAGPU_CLI_SAMTEXT": "1"} if samtext else {}))
    tr = fastq_cases.check_cli(cli, refapi.REF_BWA, ["-K", "100000000", "-t", "4", "-C", prefix, f1, f2], env, n_reads=2 * n_pairs)
    assert tr[0] == 1


@pytest.mark.parametrize("samtext", [False, True])
def test_gpu_cli_fasta_many_batches(cli_inputs, samtext):
    cli, prefix, f1, f2, n_pairs = cli_inputs
    env = dict(os.environ, **ENV, **({"BWAGPU_CLI_SAMTEXT": "1"} if samtext else {}))
    tr = fastq_cases.check_cli(cli, refapi.REF_BWA, ["-K", "3000", "-t", "4", prefix, f1, f2], env, n_reads=2 * n_pairs)
    assert tr[0] >= 20


def test_gpu_cli_fasta_long_reads(cli_inputs, tmp_path):
    """-x pacbio on 40 reads of 4 to 10 kb wrapped at 60"""
    cli, prefix = cli_inputs[:2]
    from bwa_amd import simdata
    _, g = testdata.small_index()
    rng = np.random.default_rng(833)
    reads = [simdata.make_reads_long(g, 1, length=int(rng.integers(4000, 10001)), seed=900 + i)[0] for i in range(40)]
    fa = cases.write_fasta_reads(str(tmp_path / "long.fa"), reads, [b"lr%d len=%d" % (i, len(r)) for i, r in enumerate(reads)], 60)
    fastq_cases.check_cli(cli, refapi.REF_BWA, ["-x", "pacbio", "-t", "4", prefix, fa], dict(os.environ, **ENV), n_reads=40)
