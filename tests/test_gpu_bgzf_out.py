"""GPU: the BGZF writer's kernel (bwa_amd/csrc/dev_bgzf_out.h) on hardware -- the corpus and checks of tests/bgzf_out_cases.py against zlib
and against this library's own inflate, the digests of the mock runtime's output (tests/golden/bgzf_out_digests.json: the bytes are a
function of the text and the block size alone, so the hardware must write the same), and the command line with BWAGPU_CLI_BGZF_OUT=1
against the compiled reference's SAM."""
import os
import zlib

import pytest

import bgzf_cases
import bgzf_out_cases as oc
import fastq_cases
import refapi
from bwa_amd import api
from test_bgzf_out import run_cli_bgzf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parser():
    p = api.FastqParser()
    yield p
    p.close()


def test_gpu_corpus(parser):
    gold = oc.golden()
    for name, bs in oc.RUNS:
        comp, _ = oc.check_case(parser, oc.CASES[name][0], bs)
        assert oc.digest(comp) == gold[f"{name}@{bs}"], (name, bs, "not the bytes the mock runtime writes")
    assert parser.deflate_bgzf(b"", 0, True)[0] == bgzf_cases.EOF_MARKER and parser.deflate_bgzf(b"", 0, False)[0] == b""
    oc.check_case(parser, b"GATTACA!", 1)
    oc.check_far_copies([len(parser.deflate_bgzf(oc.CASES[f"distance_{d}"][0], 0, False)[0]) for d in (32767, 32768, 32769)])
    oc.check_case(parser, oc.CASES["tandem3"][0], 0, eof_marker=False)


def test_gpu_window_of_three_times_the_corpus(parser):
    w = oc.window()
    comp, info = parser.deflate_bgzf(w, 0)
    oc.check_stream(comp, w, 0)
    assert parser.inflate_bgzf(comp)[0] == w
    assert oc.digest(comp) == oc.golden()["window@%d" % oc.FULL]


def test_gpu_sizes(parser, tmp_path):
    assert refapi.have_ref(), "oracle/_ref (the compiled reference) is missing on the GPU box"
    text = oc.CASES["acgt"][0]
    comp, _ = parser.deflate_bgzf(text, 0, False)
    print("acgt:", len(comp) / len(text))
    assert len(comp) <= 0.38 * len(text)
    assert len(parser.deflate_bgzf(oc.CASES["equal_bytes"][0], 0, False)[0]) <= oc.FULL // 50
    sam = oc.sam_text(tmp_path)
    comp, info = oc.check_case(parser, sam, 0, eof_marker=False)
    z = {k: oc.zlib_total(sam, **kw) for k, kw in (("huffman_only", dict(strategy=zlib.Z_HUFFMAN_ONLY)), ("level1", dict(level=1)), ("level6", dict(level=6)))}
    print(f"SAM text {len(sam)} bytes: device {len(comp)} ({len(comp) / len(sam):.3f}), zlib {z}; {info['deflate_ms']:.3f} ms")
    assert len(comp) < z["huffman_only"]
    assert oc.digest(comp + bgzf_cases.EOF_MARKER) == oc.golden()["sam@%d" % oc.FULL]


# ---- the command line ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_inputs(tmp_path_factory):
    import testdata
    assert refapi.have_ref(), "oracle/_ref (the compiled reference) is missing on the GPU box"
    from bwa_amd import build as b
    _, cli = b.build_host(verbose=False)
    prefix, g = testdata.small_index()
    d = tmp_path_factory.mktemp("bgzf_out_cli")
    f1, f2, _ = fastq_cases.write_cli_inputs(d, g, 300, seed=835)
    return cli, prefix, f1, f2, str(d / "out.sam.gz")


@pytest.mark.parametrize("samtext", ["0", "1"])
@pytest.mark.parametrize("K", ["3000", "100000000"])
def test_gpu_cli_bgzf_out(cli_inputs, K, samtext):
    cli, prefix, f1, f2, out = cli_inputs
    env = dict(os.environ, BWAGPU_CLI_BGZF_OUT="1", BWAGPU_CLI_TRACE="1", BWAGPU_CLI_SAMTEXT=samtext)
    for args in (["-K", K, "-t", "4", prefix, f1, f2], ["-K", K, "-t", "4", "-C", prefix, f1]):
        want, _ = fastq_cases.run_cli(refapi.REF_BWA, args, None)
        assert run_cli_bgzf(cli, args, env)[0] == want, args
    if K == "3000":
        assert run_cli_bgzf(cli, args, env, out_file=out)[0] == want
