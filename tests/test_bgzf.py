"""CPU: BGZF input inflated by the device library (bwagpu_bgzf_inflate, bwagpu_fastq_batch_bgzf; bwa_amd/csrc/dev_bgzf.h) under the mock HIP
runtime.  The inflate is held against zlib block by block (tests/bgzf_cases.py: the corpus and its oracle), the batches against the compiled
reference's bseq_read on the plain text (tests/fastq_cases.py)."""
import ctypes as C
import gzip
import os
import re
import subprocess

import pytest

import bgzf_cases
import fastq_cases
import refapi
from bwa_amd import api

PLAIN = fastq_cases.plain_cases()
IRREGULAR = fastq_cases.irregular_cases()
needs_ref = pytest.mark.skipif(not refapi.have_ref(), reason="oracle/_ref not built")
EINVAL = -2


@pytest.fixture(scope="module")
def parser():
    import hostsim_build
    p = api.FastqParser(lib_path=hostsim_build.build())
    yield p
    p.close()


# ---- the decoder against zlib ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k in bgzf_cases.VALID if not k.startswith("mutation")])
def test_valid_block_inflates_as_zlib_inflates_it(parser, name):
    text, blk = bgzf_cases.VALID[name]
    info = bgzf_cases.check_inflate(parser, blk)
    assert info["n_blocks"] == 1 and info["inflated"] == len(text) and info["used_comp"] == len(blk)


def test_mutations_zlib_still_accepts_inflate_to_zlibs_text(parser):
    for name, (text, blk) in bgzf_cases.VALID.items():
        if name.startswith("mutation"):
            assert parser.inflate_bgzf(blk)[0] == text, name


def test_all_valid_blocks_in_one_window(parser):
    blocks = [b for _, b in bgzf_cases.VALID.values()]
    info = bgzf_cases.check_inflate(parser, b"".join(blocks))
    assert info["n_blocks"] == len(blocks) and info["used_comp"] == sum(len(b) for b in blocks)
    assert info["inflated"] == sum(len(t) for t, _ in bgzf_cases.VALID.values())


NAMED_DAMAGE = [k for k in bgzf_cases.DAMAGED if not k.startswith("mutation")]


@pytest.mark.parametrize("name", NAMED_DAMAGE)
def test_damaged_block_is_damaged_where_it_was_planted(parser, name):
    for where in ("first", "middle", "last"):
        win, at = bgzf_cases.planted(name, where)
        info = bgzf_cases.check_inflate(parser, win)
        assert info["damaged_at"] == at, (where, info)
        r = parser.batch_bgzf(win, chunk_size=100)
        assert r["status"] == api.FQ_DAMAGED and r["n_reads"] == 0 and "seqs" not in r and r["bgzf"][0]["damaged_at"] == at, (where, r)
    bgzf_cases.check_inflate(parser, bgzf_cases.VALID["fixed"][1])      # the parser works afterwards


def test_mutated_blocks_are_damaged_where_they_were_planted(parser):
    names = [k for k in bgzf_cases.DAMAGED if k.startswith("mutation")]
    assert len(names) >= bgzf_cases.N_MUTATIONS * 19 // 20
    for i, name in enumerate(names):
        win, at = bgzf_cases.planted(name, ("first", "middle", "last")[i % 3])
        info = bgzf_cases.check_inflate(parser, win)
        assert info["damaged_at"] == at, (name, info)
    bgzf_cases.check_inflate(parser, bgzf_cases.VALID["fixed"][1])


def test_damage_in_the_second_window_only(parser):
    good = bgzf_cases.bgzf_file(PLAIN["pairs_diff"]["files"][0])
    bad, at = bgzf_cases.planted("crc_off_by_one_bit", "middle")
    r = parser.batch_bgzf(good, bad, chunk_size=100)
    assert r["status"] == api.FQ_DAMAGED and [i["damaged_at"] for i in r["bgzf"]] == [-1, at]
    r = parser.batch_bgzf(bad, bad, chunk_size=100)
    assert r["status"] == api.FQ_DAMAGED and [i["damaged_at"] for i in r["bgzf"]] == [at, at]


def test_damaged_wins_over_declined(parser):
    case = IRREGULAR["crlf"]
    comp = bgzf_cases.bgzf_file(case["files"][0], 700, eof_marker=False)
    assert parser.batch_bgzf(comp, chunk_size=1 << 20)["status"] == api.FQ_DECLINED
    r = parser.batch_bgzf(comp + bgzf_cases.DAMAGED["crc_off_by_one_bit"], chunk_size=1 << 20)
    assert r["status"] == api.FQ_DAMAGED and r["bgzf"][0]["damaged_at"] == len(comp) and r["declined_at"] == -1


def test_trailing_partial_block(parser):
    blocks = [bgzf_cases.VALID[k][1] for k in ("fixed", "stored", "rle")]
    whole = b"".join(blocks)
    two = len(blocks[0]) + len(blocks[1])
    for cut in (two + 1, two + 17, two + 18, len(whole) - 1):
        text, info = parser.inflate_bgzf(whole[:cut], eof=False)
        assert info["damaged_at"] == -1 and info["n_blocks"] == 2 and info["used_comp"] == two and text == bgzf_cases.VALID["fixed"][0] + bgzf_cases.VALID["stored"][0]
        text, info = parser.inflate_bgzf(whole[:cut], eof=True)
        assert text is None and info["damaged_at"] == two
    text, info = parser.inflate_bgzf(whole[:5], eof=False)
    assert text == b"" and info["n_blocks"] == 0 and info["used_comp"] == 0 and info["damaged_at"] == -1
    text, info = parser.inflate_bgzf(b"", eof=True)
    assert text == b"" and info["n_blocks"] == 0 and info["damaged_at"] == -1
    assert parser.inflate_bgzf(whole + b"not a block, and long enough to be one", eof=True)[1]["damaged_at"] == len(whole)
    assert parser.inflate_bgzf(bgzf_cases.EOF_MARKER * 3 + whole + bgzf_cases.EOF_MARKER)[0] == bgzf_cases.oracle_window(whole)[0]


# ---- batches from BGZF windows -----------------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("name", sorted(PLAIN))
def test_chained_batches_equal_bseq_read(parser, name):
    """from the start of the file(s) to END by next_coff / next_uoff, blocks of 1 .. 4000 text bytes: records straddle blocks everywhere"""
    case = PLAIN[name]
    comp = bgzf_cases.bgzf_case(case)
    for chunk in fastq_cases.chunks_for(case):
        # (small chunks: short compressed windows, so that a call does not inflate the rest of the file for one record)
        bgzf_cases.run_chain(parser, case, comp, chunk, window=None if chunk >= 1000 else 600 + 2 * chunk, compare_plain=chunk in (150, 1000))


@needs_ref
@pytest.mark.parametrize("name", ["cycle", "names", "pairs_cycle", "pairs_diff", "empty"])
def test_result_does_not_depend_on_the_block_sizes(parser, name):
    case = PLAIN[name]
    for comp in (bgzf_cases.bgzf_case(case, 0xff00), bgzf_cases.bgzf_case(case, 0xff00, eof_marker=False), bgzf_cases.bgzf_case(case, 333, eof_marker=False)):
        bgzf_cases.run_chain(parser, case, comp, 1000)


@needs_ref
def test_result_does_not_depend_on_the_compressed_windows_length(parser):
    bgzf_cases.run_windows(parser, PLAIN)


@needs_ref
@pytest.mark.parametrize("name", sorted(IRREGULAR))
def test_irregular_record_declines_its_batch_at_its_offset_in_the_text_window(parser, name):
    case = IRREGULAR[name]
    comp = bgzf_cases.bgzf_case(case)
    n_cut = {chunk: bgzf_cases.run_irregular(parser, case, comp, chunk) for chunk in (150, 1 << 20)}
    plain = {chunk: fastq_cases.run_irregular(parser, case, chunk) for chunk in (150, 1 << 20)}
    assert n_cut == plain and n_cut[1 << 20] == 0


def test_invalid_arguments(parser):
    blk = bgzf_cases.block_of(b"@a\nA\n+\nI\n")
    buf = C.create_string_buffer(blk, len(blk))
    o, info = api.FastqOut(), (api.BgzfInfo * 2)()

    def call(w1, w2=None, chunk=100, out=o, inf=info):
        return parser.batch_bgzf_rc(None if w1 is None else C.byref(w1), None if w2 is None else C.byref(w2), chunk, None if out is None else C.byref(out), inf)

    def win(comp=C.addressof(buf), n=len(blk), skip=0, eof=1):
        return api.BgzfWin(comp, n, skip, eof)

    assert call(win()) == 0 and o.status == api.FQ_END and o.n_reads == 1 and info[0].n_blocks == 1 and info[0].next_coff == len(blk)
    parser.L.bwagpu_fastq_out_free(C.byref(o))
    assert call(win(skip=9)) == 0 and o.status == api.FQ_END and o.n_reads == 0      # skip == ISIZE: everything was consumed before
    parser.L.bwagpu_fastq_out_free(C.byref(o))
    assert call(win(skip=10)) == EINVAL and call(win(skip=-1)) == EINVAL              # skip out of range
    assert b"bwagpu_fastq_batch_bgzf" in parser.L.bwagpu_fastq_last_error(parser.h)
    assert call(win(n=0, skip=1)) == EINVAL                                           # (no block taken: no text to skip)
    assert call(None) == EINVAL and call(win(comp=None)) == EINVAL and call(win(), win(comp=None)) == EINVAL
    assert call(win(n=-1)) == EINVAL and call(win(), win(n=-1)) == EINVAL
    assert call(win(), out=None) == EINVAL and call(win(), inf=None) == EINVAL
    assert call(win(), chunk=0) == EINVAL and call(win(), chunk=-3) == EINVAL
    assert parser.L.bwagpu_fastq_batch_bgzf(None, C.byref(win()), None, 100, C.byref(o), info) == EINVAL
    dst = C.create_string_buffer(16)
    one = api.BgzfInfo()
    inflate = parser.L.bwagpu_bgzf_inflate
    assert inflate(parser.h, buf, len(blk), 1, dst, 16, C.byref(one)) == 0 and dst.raw[:9] == b"@a\nA\n+\nI\n" and one.inflated == 9
    assert inflate(parser.h, buf, len(blk), 1, dst, 8, C.byref(one)) == EINVAL and one.inflated == 9      # dst_cap too small: the size is reported
    assert inflate(parser.h, None, len(blk), 1, dst, 16, C.byref(one)) == EINVAL and inflate(parser.h, buf, -1, 1, dst, 16, C.byref(one)) == EINVAL
    assert inflate(parser.h, buf, len(blk), 1, None, 16, C.byref(one)) == EINVAL and inflate(parser.h, buf, len(blk), 1, dst, 16, None) == EINVAL
    assert inflate(None, buf, len(blk), 1, dst, 16, C.byref(one)) == EINVAL
    # bwagpu_fastq_batch on plain text still passes on the same parser
    r = parser.batch(b"@a\nA\n+\nI\n", chunk_size=100)
    assert r["status"] == api.FQ_END and r["n_reads"] == 1
    if refapi.have_ref():
        fastq_cases.run_plain(parser, PLAIN["names"], 7)


# ---- the command line: BWAGPU_CLI_FASTQ=1 BWAGPU_CLI_BGZF_DEV=1 ------------------------------------------------------------------------
BLOCKS_LINE = re.compile(rb"\[D::input\] (\d+) BGZF blocks inflated on the device")


@needs_ref
def test_cli_bgzf_switch_on_the_mock_runtime(tmp_path):
    import test_cli
    import testdata
    prefix, g = testdata.small_index()
    n_pairs = 14
    p1, p2, pirr = fastq_cases.write_cli_inputs(tmp_path, g, n_pairs, seed=431)
    # blocks of 700 text bytes: every batch of -K 3000 starts inside a block
    f1, f2, irr = (bgzf_cases.write_bgzf(p + ".gz", open(p, "rb").read(), 700) for p in (p1, p2, pirr))
    cli = test_cli._sim_cli()
    env = dict(os.environ, BWAGPU_CLI_STREAMS="2", BWAGPU_CLI_SERIALIZE="1", BWAGPU_PTAB_M="6", BWAGPU_CLI_FASTQ="1", BWAGPU_CLI_BGZF_DEV="1", BWAGPU_CLI_TRACE="1")
    K = ["-K", "100000000", "-t", "2"]
    fastq_cases.check_cli(cli, refapi.REF_BWA, K + [prefix, f1], env, n_reads=n_pairs)                                     # single-end
    fastq_cases.check_cli(cli, refapi.REF_BWA, K + [prefix, f1, f2], env, n_reads=2 * n_pairs)                             # paired-end, two files
    fastq_cases.check_cli(cli, refapi.REF_BWA, K + ["-C", prefix, f1, f2], env, n_reads=2 * n_pairs)                       # comments
    tr = fastq_cases.check_cli(cli, refapi.REF_BWA, ["-K", "3000", "-t", "2", prefix, f1, f2], env, n_reads=2 * n_pairs)   # many batches, positions inside blocks
    assert tr[0] > 1
    fastq_cases.check_cli(cli, refapi.REF_BWA, ["-K", "1000", "-t", "2", "-C", prefix, irr], env, irregular=True)          # fallback in the middle of the run
    p = subprocess.run([cli, "mem"] + K + [prefix, f1, f2], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    n_blocks = sum(len(open(f, "rb").read().split(b"\x1f\x8b\x08\x04")) - 1 for f in (f1, f2))
    assert p.returncode == 0 and int(BLOCKS_LINE.search(p.stderr).group(1)) == n_blocks, p.stderr.decode()[-1500:]
    env_t = dict(env, BWAGPU_CLI_SAMTEXT="1")
    for args in (["-K", "1000", "-t", "2", "-C", prefix, f1], ["-K", "3000", "-t", "2", "-C", prefix, f1, f2]):
        want, _ = fastq_cases.run_cli(refapi.REF_BWA, args, None)
        p = subprocess.run([cli, "mem"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env_t)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert b"\n".join(l for l in p.stdout.split(b"\n") if not l.startswith(b"@PG")) == want, args
        n_text = sum(int(x) for x, _ in re.findall(rb"(\d+) (reads|pairs) written from device SAM text", p.stderr))
        assert fastq_cases.TRACE.search(p.stderr) and BLOCKS_LINE.search(p.stderr) and n_text > 0, p.stderr.decode()[-1500:]
    # a byte flipped inside a block
    data = bytearray(open(f2, "rb").read())
    data[len(data) // 2] ^= 0x20
    bad = str(tmp_path / "flipped.fq.gz")
    open(bad, "wb").write(bytes(data))
    p = subprocess.run([cli, "mem"] + K + [prefix, f1, bad], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert p.returncode != 0 and b"BGZF" in p.stderr and b"flipped.fq.gz" in p.stderr, p.stderr.decode()[-1500:]
    # the switch does not apply: plain gzip, -p, a mixed pair -- same SAM, no device line
    gz = str(tmp_path / "plain.fq.gz")
    with gzip.open(gz, "wb") as f:
        f.write(open(p1, "rb").read())
    for args in (K + [prefix, gz], K + ["-p", prefix, f1], K + [prefix, f1, p2], K + [prefix, p1, f2]):
        want, _ = fastq_cases.run_cli(refapi.REF_BWA, args, None)
        got, tr = fastq_cases.run_cli(cli, args, env)
        assert got == want and tr is None, args
    # without the new switch BGZF input stays with the host reader
    _, tr = fastq_cases.run_cli(cli, K + [prefix, f1, f2], dict(env, BWAGPU_CLI_BGZF_DEV="0"))
    assert tr is None
