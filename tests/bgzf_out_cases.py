"""Texts for the device BGZF writer's tests (tests/test_bgzf_out.py on the mock runtime, tests/test_gpu_bgzf_out.py on hardware; the kernel is
bwa_amd/csrc/dev_bgzf_out.h, the entry point bwagpu_bgzf_deflate) and the checks both share.  The corpus is generated from seeds.  The
oracle is zlib: decompressobj(-15) and crc32 per block behind the block walk of bgzf_cases.block_len (BgzfPipe::block_len's test),
gzip.decompress for a whole stream -- never the code under test.

    python tests/bgzf_out_cases.py --write-golden     digests of the mock runtime's output -> tests/golden/bgzf_out_digests.json
    python tests/bgzf_out_cases.py --dump DIR         the corpus as files, one per case"""
import gzip
import hashlib
import json
import os
import struct
import sys
import zlib

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bgzf_cases

FULL = 0xff00
SMALL = 333
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bgzf_out_digests.json")


def _rand(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _fib_text(n_symbols, seed):
    """byte value k occurs F(k + 2) times (1, 2, 3, 5, ...): with the end-of-block symbol's one that is F(1), F(2), ... over
    n_symbols + 1 symbols, the counts an unlimited Huffman code is n_symbols bits deep for.  Shuffled, so that literals remain."""
    f = [1, 2]
    while len(f) < n_symbols:
        f.append(f[-1] + f[-2])
    a = np.concatenate([np.full(c, 65 + k, dtype=np.uint8) for k, c in enumerate(f)])
    np.random.default_rng(seed).shuffle(a)
    return a.tobytes()


def _cl_text(seed):
    """byte counts 2^(16 - L) for 21 / 13 / 8 / 5 / 3 / 2 / 1 / 1 values with L = 5 .. 12: the numbers of values per code length rise like
    the Fibonacci numbers below 232 zeros, which is what drives the code-length code towards its 7-bit limit (profiles/dev_bgzf_out.md)"""
    parts, v = [], 0
    for L, k in zip(range(5, 13), (21, 13, 8, 5, 3, 2, 1, 1)):
        for _ in range(k):
            parts.append(np.full(1 << (16 - L), v, dtype=np.uint8))
            v += 1
    a = np.concatenate(parts)
    np.random.default_rng(seed).shuffle(a)
    return a.tobytes()


def _cases():
    c = {}
    c["empty"] = (b"", (FULL, SMALL))
    for n in (1, 2, 3, 4):
        c[f"len{n}"] = (b"GATC"[:n], (FULL, SMALL))
    # one literal value + end-of-block, no distance code.  (Fixed codes are smaller for texts this short, so these come out as fixed blocks; the
    # code builder still runs on their counts.  "one_distance" below is the text whose dynamic block has one used distance symbol.)
    c["one_value_1"] = (b"N", (FULL,))
    c["one_value_2"] = (b"NN", (FULL,))
    for name, n in (("full_minus_1", FULL - 1), ("full", FULL), ("full_plus_1", FULL + 1)):
        t = np.random.default_rng(11).integers(0, 4, n, dtype=np.uint8)
        c[name] = (np.frombuffer(b"ACGT", dtype=np.uint8)[t].tobytes(), (FULL,))
    c["equal_bytes"] = (b"F" * FULL, (FULL, SMALL))       # distance 1, chains of 258, a match that ends on the block's last byte
    for p in range(2, 8):
        c[f"tandem{p}"] = ((b"ACGTNWS"[:p] * (5000 // p + 1))[:5000 + p], (FULL, SMALL))
    unit = _rand(21, 300)
    # zeros between the two copies: they enter one hash head only, so the first copy's heads are still there when the second copy looks them up.
    # 32767 and 32768 are taken, 32769 is not (FAR_COPY_GAP below; zlib's 32 KiB window is the judge of what is sent)
    for d in (32767, 32768, 32769):
        c[f"distance_{d}"] = (unit + b"\0" * (d - 300) + unit + b"tail", (FULL,))
    c["one_distance"] = (unit + unit, (FULL,))            # two matches at distance 300: a distance code with one used symbol, one bit long
    c["straddle"] = (_rand(23, FULL - 150) + unit + unit + _rand(24, 100), (FULL, SMALL))      # the unit's second half and its repeat lie in the second block
    c["random"] = (_rand(25, FULL + 2000), (FULL, SMALL))                                      # the stored fall-back
    c["all_values"] = (bytes(range(256)), (FULL, SMALL))
    c["fibonacci_21"] = (_fib_text(21, 26), (FULL,))      # 46366 bytes, one block: 22 symbols with the end-of-block one, depth 21 unlimited
    c["fibonacci_23"] = (_fib_text(23, 27), (FULL,))      # 121391 bytes, two blocks of the same skew (23 values cannot fit one block: their counts sum to 121391)
    c["code_lengths"] = (_cl_text(28), (FULL,))
    t = np.random.default_rng(29).integers(0, 4, 8 * FULL, dtype=np.uint8)
    c["acgt"] = (np.frombuffer(b"ACGT", dtype=np.uint8)[t].tobytes(), (FULL,))
    return c


CASES = _cases()
RUNS = [(name, bs) for name, (_, sizes) in CASES.items() for bs in sizes]


# The second copy of the 300 random bytes costs two matches (a few bytes) when it is taken and 300 literals of a code in which half the
# text is one value -- nine bits or more each -- when it is not: over 300 bytes apart, 200 asked
FAR_COPY_GAP = 200


def check_far_copies(sizes):
    """sizes: bytes written for distance_32767 / _32768 / _32769 (no end-of-file block)"""
    s67, s68, s69 = sizes
    assert abs(s67 - s68) <= 16 and s69 - max(s67, s68) >= FAR_COPY_GAP, sizes


def sam_text(tmp_dir, n_pairs=300, seed=833):
    """SAM of the compiled reference for fastq_cases.write_cli_inputs' pairs on the small index (without @PG)"""
    import fastq_cases
    import refapi
    import testdata
    prefix, g = testdata.small_index()
    f1, f2, _ = fastq_cases.write_cli_inputs(tmp_dir, g, n_pairs, seed=seed)
    sam, _ = fastq_cases.run_cli(refapi.REF_BWA, ["-K", "100000000", "-t", "2", "-C", prefix, f1, f2], None)
    return sam


def window():
    """one text of 3 x the whole corpus: more blocks than the chip holds at a time per CU"""
    return b"".join(t for t, _ in CASES.values()) * 3


def blocks_of(comp, eof_marker=True):
    """the stream cut into blocks by the reader's own header walk; the end-of-file block is checked and dropped"""
    out, o = [], 0
    while o < len(comp):
        bl = bgzf_cases.block_len(comp[o:])
        assert bl, f"no BGZF block at offset {o}"
        out.append(comp[o:o + bl])
        o += bl
    if eof_marker:
        assert out and out[-1] == bgzf_cases.EOF_MARKER and comp.endswith(bgzf_cases.EOF_MARKER), "the stream does not end with the 28-byte end-of-file block"
        out.pop()
    return out


def check_stream(comp, text, bs, eof_marker=True):
    """every property of the format; returns the blocks' lengths"""
    bs = bs or FULL
    blocks = blocks_of(comp, eof_marker)
    assert len(blocks) == (len(text) + bs - 1) // bs
    for j, b in enumerate(blocks):
        part = text[j * bs:(j + 1) * bs]
        assert b[:16] == bytes.fromhex("1f8b08040000000000ff060042430200") and struct.unpack("<H", b[16:18])[0] == len(b) - 1, j
        crc, isize = struct.unpack("<II", b[-8:])
        assert isize == len(part) and crc == zlib.crc32(part), j
        d = zlib.decompressobj(-15)
        got = d.decompress(b[18:-8])
        assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b"" and got == part, j
        assert len(b) <= 65536 and len(b) <= len(part) + 31, (j, len(b), len(part))      # never larger than the stored form
    assert gzip.decompress(comp) == text if comp else text == b""
    return [len(b) for b in blocks]


def check_case(parser, text, bs, eof_marker=True):
    """format, round trip through the library's own reader, determinism; returns (compressed bytes, info)"""
    comp, info = parser.deflate_bgzf(text, bs, eof_marker)
    sizes = check_stream(comp, text, bs, eof_marker)
    assert info["n_blocks"] == len(sizes) and info["text_len"] == len(text) and info["comp_len"] == len(comp)
    back, inf = parser.inflate_bgzf(comp)
    assert inf["damaged_at"] == -1 and back == text and inf["n_blocks"] == len(sizes) + (1 if eof_marker else 0)
    again, _ = parser.deflate_bgzf(text, bs, eof_marker)
    assert again == comp, "two calls, two results"
    return comp, info


def zlib_total(text, bs=FULL, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    """bytes of the BGZF blocks zlib's compressor makes of the same slices"""
    return sum(len(bgzf_cases.bgzf_block(bgzf_cases.deflate(text[o:o + bs], level, strategy), 0, 0)) for o in range(0, len(text), bs))


def digest(comp):
    return hashlib.sha256(comp).hexdigest()[:32]


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def dump(path):
    os.makedirs(path, exist_ok=True)
    for name, (text, _) in CASES.items():
        with open(os.path.join(path, name + ".txt"), "wb") as f:
            f.write(text)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--dump"]:
        dump(sys.argv[2])
    elif sys.argv[1:2] == ["--write-golden"]:
        import hostsim_build
        from bwa_amd import api
        p = api.FastqParser(lib_path=hostsim_build.build())
        d = {f"{name}@{bs}": digest(p.deflate_bgzf(CASES[name][0], bs)[0]) for name, bs in RUNS}
        d["window@%d" % FULL] = digest(p.deflate_bgzf(window(), FULL)[0])
        import pathlib
        import tempfile
        import refapi
        assert refapi.have_ref(), "oracle/_ref (the compiled reference) makes the SAM text"
        with tempfile.TemporaryDirectory() as t:
            d["sam@%d" % FULL] = digest(p.deflate_bgzf(sam_text(pathlib.Path(t)), FULL)[0])
        with open(GOLDEN, "w") as f:
            json.dump(d, f, indent=1, sort_keys=True)
            f.write("\n")
        print(len(d), "digests ->", GOLDEN)
    else:
        sys.exit(__doc__)
