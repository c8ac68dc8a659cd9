"""CPU: the device BGZF writer (bwagpu_bgzf_deflate; bwa_amd/csrc/dev_bgzf_out.h) under the mock HIP runtime.  tests/bgzf_out_cases.py has the
corpus and the checks: every block against zlib (decompressobj(-15), crc32), the stream against gzip.decompress and against this library's
own bwagpu_bgzf_inflate, two calls against each other and against the digests of tests/golden/bgzf_out_digests.json (which the GPU test
holds the hardware's output against).  The size conditions keep a coder that finds no matches, or sends no dynamic codes, from passing; their
numbers are zlib's, measured by the test itself on the same slices."""
import ctypes as C
import gzip
import os
import re
import subprocess
import zlib

import pytest

import bgzf_cases
import bgzf_out_cases as oc
import fastq_cases
import refapi
from bwa_amd import api

needs_ref = pytest.mark.skipif(not refapi.have_ref(), reason="oracle/_ref not built")
EINVAL = -2
OUT_LINE = re.compile(rb"\[D::output\] (\d+) blocks, (\d+) text bytes, (\d+) compressed bytes, ([0-9.]+) ms on the device")


@pytest.fixture(scope="module")
def parser():
    import hostsim_build
    p = api.FastqParser(lib_path=hostsim_build.build())
    yield p
    p.close()


@pytest.fixture(scope="module")
def sam(tmp_path_factory):
    return oc.sam_text(tmp_path_factory.mktemp("bgzf_out_sam"))


def test_limits(parser):
    assert parser.bgzf_out_limits() == {"max_block_text": 0xff00, "min_match": 4, "max_match": 258, "max_dist": 32768}


@pytest.mark.parametrize("name,bs", oc.RUNS)
def test_case_is_bgzf_that_zlib_and_the_own_reader_inflate_to_the_text(parser, name, bs):
    comp, _ = oc.check_case(parser, oc.CASES[name][0], bs)
    assert oc.digest(comp) == oc.golden()[f"{name}@{bs}"], "the bytes changed: python tests/bgzf_out_cases.py --write-golden, and run the GPU test"


def test_empty_text(parser):
    assert parser.deflate_bgzf(b"", 0, True)[0] == bgzf_cases.EOF_MARKER and parser.deflate_bgzf(b"", 0, False)[0] == b""
    assert parser.deflate_bgzf(b"", 333, True)[1] == {"n_blocks": 0, "text_len": 0, "comp_len": 28, "deflate_ms": 0.0}


def test_without_the_end_of_file_block(parser):
    for name in ("len4", "full_plus_1", "tandem3"):
        text = oc.CASES[name][0]
        with_eof, _ = parser.deflate_bgzf(text, 0, True)
        without, _ = oc.check_case(parser, text, 0, eof_marker=False)
        assert with_eof == without + bgzf_cases.EOF_MARKER


def test_block_size_zero_is_bgzips(parser):
    text = oc.CASES["full_plus_1"][0]
    assert parser.deflate_bgzf(text, 0)[0] == parser.deflate_bgzf(text, 0xff00)[0]
    assert [len(b) for b in oc.blocks_of(parser.deflate_bgzf(text, 0)[0])][1] <= 1 + 31      # the second block: one byte


def test_block_size_one(parser):
    text = b"GATTACA!"
    comp, info = oc.check_case(parser, text, 1)
    assert info["n_blocks"] == len(text)


def test_a_block_does_not_depend_on_its_neighbours(parser):
    """a block's bytes are a function of its own text: the straddling repeat's second block equals the block of that text alone"""
    text = oc.CASES["straddle"][0]
    both = oc.blocks_of(parser.deflate_bgzf(text, 0)[0])
    alone = oc.blocks_of(parser.deflate_bgzf(text[oc.FULL:], 0)[0])
    assert both[1:] == alone


def test_window_of_three_times_the_corpus(parser):
    w = oc.window()
    comp, info = parser.deflate_bgzf(w, 0)
    oc.check_stream(comp, w, 0)
    assert parser.inflate_bgzf(comp)[0] == w
    assert oc.digest(comp) == oc.golden()["window@%d" % oc.FULL]


def test_the_largest_distance_is_taken_and_one_more_is_not(parser):
    sizes = [len(parser.deflate_bgzf(oc.CASES[f"distance_{d}"][0], 0, False)[0]) for d in (32767, 32768, 32769)]
    print("far copies:", sizes)
    oc.check_far_copies(sizes)


def test_long_matches_are_found(parser):
    """65280 equal bytes: chains of 258-byte matches at a short distance -- zlib level 1 takes 0.4 % of the text, 2 % is far from any
    coder that does not find them (Huffman-only: 12.5 %)"""
    comp, _ = parser.deflate_bgzf(oc.CASES["equal_bytes"][0], 0, False)
    print("equal bytes:", len(comp), "zlib level 1:", oc.zlib_total(oc.CASES["equal_bytes"][0], level=1))
    assert len(comp) <= oc.FULL // 50


def test_uniform_acgt_takes_dynamic_codes(parser):
    """at most 0.38 of the text: zlib gives 0.281 Huffman-only, 0.333 at level 1, and 0.41 at best with fixed codes"""
    text = oc.CASES["acgt"][0]
    comp, _ = parser.deflate_bgzf(text, 0, False)
    z = {k: oc.zlib_total(text, **kw) / len(text) for k, kw in (("huffman_only", dict(strategy=zlib.Z_HUFFMAN_ONLY)), ("level1", dict(level=1)), ("fixed", dict(level=9, strategy=zlib.Z_FIXED)))}
    print("acgt:", len(comp) / len(text), "zlib:", z)
    assert len(comp) <= 0.38 * len(text)


@needs_ref
def test_sam_text(parser, sam):
    """matches pay: strictly below zlib's Z_HUFFMAN_ONLY total over the same blocks.  The ratios against level 1 and level 6 are printed,
    not bounded (profiles/dev_bgzf_out.md has them)"""
    comp, _ = oc.check_case(parser, sam, 0, eof_marker=False)
    ours = len(comp)
    z = {k: oc.zlib_total(sam, **kw) for k, kw in (("huffman_only", dict(strategy=zlib.Z_HUFFMAN_ONLY)), ("level1", dict(level=1)), ("level6", dict(level=6)))}
    print(f"SAM text {len(sam)} bytes: device {ours} ({ours / len(sam):.3f}), zlib {z}; device / level 1 = {ours / z['level1']:.3f}, device / level 6 = {ours / z['level6']:.3f}")
    assert ours < z["huffman_only"]
    assert oc.digest(comp + bgzf_cases.EOF_MARKER) == oc.golden()["sam@%d" % oc.FULL]
    oc.check_case(parser, sam[:20000], oc.SMALL)


def test_invalid_arguments(parser):
    text = b"some text, some text"
    buf = C.create_string_buffer(text, len(text))
    comp, info = C.c_void_p(), api.BgzfOutInfo()

    def call(t=buf, n=len(text), bs=0, eof=1, c=C.byref(comp), i=C.byref(info)):
        rc = parser.deflate_bgzf_rc(t, n, bs, eof, c, i)
        if rc == 0:
            parser.L.bwagpu_free(comp)
        return rc

    assert call() == 0 and info.n_blocks == 1 and info.text_len == len(text)
    assert call(t=None) == EINVAL and comp.value is None
    assert b"bwagpu_bgzf_deflate" in parser.L.bwagpu_fastq_last_error(parser.h)
    assert call(n=-1) == EINVAL and call(c=None) == EINVAL and call(i=None) == EINVAL
    assert call(bs=-1) == EINVAL and call(bs=0xff01) == EINVAL and call(bs=1 << 20) == EINVAL
    assert call(bs=0xff00) == 0 and call(bs=1) == 0 and info.n_blocks == len(text)
    assert parser.L.bwagpu_bgzf_deflate(None, buf, len(text), 0, 1, C.byref(comp), C.byref(info)) == EINVAL
    assert parser.deflate_bgzf(text)[0] == parser.deflate_bgzf(bytearray(text))[0]      # the parser works afterwards
    assert parser.batch(b"@a\nA\n+\nI\n", chunk_size=100)["n_reads"] == 1                 # and its other entry points


# ---- the command line: BWAGPU_CLI_BGZF_OUT=1 --------------------------------------------------------------------------------------------
def run_cli_bgzf(cli, args, env, out_file=None):
    """(SAM without @PG from the BGZF stream on stdout or in out_file, the [D::output] line's numbers)"""
    p = subprocess.run([cli, "mem"] + (["-o", out_file] if out_file else []) + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    raw = open(out_file, "rb").read() if out_file else p.stdout
    assert not out_file or p.stdout == b""
    assert raw.endswith(bgzf_cases.EOF_MARKER)
    text = gzip.decompress(raw)
    oc.blocks_of(raw)
    m = OUT_LINE.search(p.stderr)
    assert m, p.stderr.decode()[-1500:]
    n_blocks, n_text, n_comp = (int(m.group(k)) for k in (1, 2, 3))
    assert n_text == len(text) and n_comp == len(raw) and n_blocks == len(oc.blocks_of(raw)), (m.groups(), len(text), len(raw))
    return b"\n".join(l for l in text.split(b"\n") if not l.startswith(b"@PG")), raw


@needs_ref
def test_cli_switch_on_the_mock_runtime(tmp_path):
    import test_cli
    import testdata
    prefix, g = testdata.small_index()
    f1, f2, _ = fastq_cases.write_cli_inputs(tmp_path, g, 14, seed=437)
    cli = test_cli._sim_cli()
    env = dict(os.environ, BWAGPU_CLI_STREAMS="2", BWAGPU_CLI_SERIALIZE="1", BWAGPU_PTAB_M="6", BWAGPU_CLI_BGZF_OUT="1", BWAGPU_CLI_TRACE="1")
    for args in (["-K", "100000000", "-t", "2", prefix, f1, f2], ["-K", "3000", "-t", "2", "-C", prefix, f1, f2], ["-K", "3000", "-t", "2", prefix, f1]):
        want, _ = fastq_cases.run_cli(refapi.REF_BWA, args, None)
        assert run_cli_bgzf(cli, args, env)[0] == want, args
        assert run_cli_bgzf(cli, args, dict(env, BWAGPU_CLI_SAMTEXT="1"))[0] == want, args
    args = ["-K", "3000", "-t", "2", prefix, f1, f2]
    want, _ = fastq_cases.run_cli(refapi.REF_BWA, args, None)
    got, raw = run_cli_bgzf(cli, args, env, out_file=str(tmp_path / "out.sam.gz"))
    assert got == want
    # the switch is off by default: plain text
    plain, _ = fastq_cases.run_cli(cli, args, dict(env, BWAGPU_CLI_BGZF_OUT="0"))
    assert plain == want
