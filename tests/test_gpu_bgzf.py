"""GPU: the BGZF inflate kernel (bwa_amd/csrc/dev_bgzf.h) on hardware -- the corpus of tests/bgzf_cases.py against zlib, and the chained
batches, window and block-size properties of tests/test_bgzf.py against the compiled reference's bseq_read (the mock runtime of the CPU
tests runs lanes as fibers and cannot see wave-level errors).  The damaged blocks are the deterministic corpus, run once: they test the
error path of bounded code."""
import pytest

import bgzf_cases
import fastq_cases
import refapi
from bwa_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parser():
    assert refapi.have_ref(), "oracle/_ref (the compiled reference) is missing on the GPU box"
    p = api.FastqParser()
    yield p
    p.close()


def test_gpu_valid_corpus_inflates_as_zlib_inflates_it(parser):
    for name, (text, blk) in bgzf_cases.VALID.items():
        info = bgzf_cases.check_inflate(parser, blk)
        assert info["n_blocks"] == 1 and info["inflated"] == len(text) and info["used_comp"] == len(blk), name
    blocks = [b for _, b in bgzf_cases.VALID.values()]
    info = bgzf_cases.check_inflate(parser, b"".join(blocks) * 3)      # more blocks than one CU holds at a time
    assert info["n_blocks"] == 3 * len(blocks)


def test_gpu_damaged_corpus_is_damaged_where_it_was_planted(parser):
    for i, name in enumerate(bgzf_cases.DAMAGED):
        for where in (("first", "middle", "last") if not name.startswith("mutation") else (("first", "middle", "last")[i % 3],)):
            win, at = bgzf_cases.planted(name, where)
            assert bgzf_cases.check_inflate(parser, win)["damaged_at"] == at, (name, where)
    win, at = bgzf_cases.planted("crc_off_by_one_bit", "middle")
    r = parser.batch_bgzf(bgzf_cases.VALID["fixed"][1], win, chunk_size=100)
    assert r["status"] == api.FQ_DAMAGED and r["n_reads"] == 0 and "seqs" not in r and [i["damaged_at"] for i in r["bgzf"]] == [-1, at]
    bgzf_cases.check_inflate(parser, bgzf_cases.VALID["dynamic_level6"][1])      # the parser works afterwards


def test_gpu_chained_batches_equal_bseq_read(parser):
    for name, case in sorted(fastq_cases.plain_cases().items()):
        comp = bgzf_cases.bgzf_case(case)
        for chunk in fastq_cases.chunks_for(case):
            bgzf_cases.run_chain(parser, case, comp, chunk, window=None if chunk >= 150 else 600 + 2 * chunk, compare_plain=chunk in (150, 1000))


def test_gpu_result_does_not_depend_on_blocks_or_windows(parser):
    plain = fastq_cases.plain_cases()
    for name in ("cycle", "names", "pairs_cycle", "pairs_diff", "empty"):
        for comp in (bgzf_cases.bgzf_case(plain[name], 0xff00), bgzf_cases.bgzf_case(plain[name], 333, eof_marker=False)):
            bgzf_cases.run_chain(parser, plain[name], comp, 1000)
    bgzf_cases.run_windows(parser, plain)


def test_gpu_irregular_corpus_declines_at_the_planted_record(parser):
    for name, case in sorted(fastq_cases.irregular_cases().items()):
        comp = bgzf_cases.bgzf_case(case)
        for chunk in (150, 1 << 20):
            assert bgzf_cases.run_irregular(parser, case, comp, chunk) == fastq_cases.run_irregular(parser, case, chunk), (name, chunk)


# ---- the command line ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_inputs(tmp_path_factory):
    import testdata
    assert refapi.have_ref(), "oracle/_ref (the compiled reference) is missing on the GPU box"
    from bwa_amd import build as b
    _, cli = b.build_host(verbose=False)
    prefix, g = testdata.small_index()
    n_pairs = 300
    d = tmp_path_factory.mktemp("bgzf_cli")
    f1, f2, _ = fastq_cases.write_cli_inputs(d, g, n_pairs, seed=831)
    z1, z2 = (bgzf_cases.write_bgzf(f + ".gz", open(f, "rb").read(), 0xff00 if k else 5000) for k, f in enumerate((f1, f2)))
    return cli, prefix, z1, z2, n_pairs


def _cli(cli_inputs, args, **env):
    import os
    cli, prefix, z1, z2, n_pairs = cli_inputs
    e = dict(os.environ, BWAGPU_CLI_FASTQ="1", BWAGPU_CLI_BGZF_DEV="1", BWAGPU_CLI_TRACE="1", **env)
    return fastq_cases.check_cli(cli, refapi.REF_BWA, args + [prefix, z1, z2], e, n_reads=2 * n_pairs)


def test_gpu_cli_bgzf(cli_inputs):
    _cli(cli_inputs, ["-K", "100000000", "-t", "4", "-C"])


def test_gpu_cli_bgzf_and_samtext(cli_inputs):
    _cli(cli_inputs, ["-K", "100000000", "-t", "4", "-C"], BWAGPU_CLI_SAMTEXT="1")


def test_gpu_cli_bgzf_many_batches(cli_inputs):
    assert _cli(cli_inputs, ["-K", "3000", "-t", "4"])[0] >= 20
