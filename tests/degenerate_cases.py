"""Tiny and degenerate genomes, shared by the index-builder tests (tests/test_index_build.py on the mock runtime, tests/test_gpu_index.py and
tests/test_gpu_fasta_index.py on the device) and the hot-path tests (tests/test_hostsim.py, tests/test_gpu_parity.py).

index_cases(): texts shorter than the structures built over them (the first-pass key of B + 29 bases, the 10-base prefix tables, Occ blocks of 128
and 64 symbols, 32 bases to a packed word, an SA sample every 32 rows) and texts that are all repeat (prefix doubling runs about log2(n) rounds with
one group peeling off h suffixes a round; the terminator's place is decided on every round).
align_cases(): a subset small enough for the reference's mem_align1_core, with reads whose SA intervals span whole symbol ranges and that have
hundreds to thousands of regions.

Everything is generated from seeds (one stream per name, so a case does not depend on which others exist); the expected outputs come from the compiled
reference at test time."""
import zlib

import numpy as np

SEED = 20240
RAND_LENS = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257)
POLY_LENS = (1, 2, 14, 15, 16, 29, 30, 64, 1000, 20000)
TANDEM_PERIODS = (2, 3, 4, 5, 29, 30, 31, 32, 33, 58, 64)       # (29 bases follow the bucket in the first-pass key: the key width and twice it, +- 1)
ALIGN_RAND_LENS = (1, 5, 9, 10, 11, 20, 63, 64, 65, 200)


def _rng(name):
    return np.random.default_rng([SEED, zlib.crc32(name.encode())])


def _rand(name, n):
    return _rng(name).integers(0, 4, n).astype(np.uint8)


def rc(x):
    return np.ascontiguousarray(3 - x[::-1]).astype(np.uint8)


def _fib(n):
    a, b = np.array([0], np.uint8), np.array([0, 1], np.uint8)
    while len(b) < n:
        a, b = b, np.concatenate([b, a])
    return np.ascontiguousarray(b[:n])


def _multi_contig():
    """name -> (codes, contig lengths)"""
    u = _rand("two_equal_contigs", 500)
    return {"two_equal_contigs": (np.concatenate([u, u]), [500, 500]), "contig_of_one_base": (_rand("contig_of_one_base", 42), [1, 1, 40])}


def index_cases():
    """name -> uint8 codes (0..3); one contig each, except the names contig_lens() knows"""
    c = {}
    for n in RAND_LENS:
        c[f"rand{n}"] = _rand(f"rand{n}", n)
    for n in POLY_LENS:
        for ch, code in (("A", 0), ("C", 1), ("T", 3)):
            c[f"poly{ch}{n}"] = np.full(n, code, np.uint8)
    for p in TANDEM_PERIODS:
        c[f"tandem{p}"] = np.tile(_rand(f"tandem{p}", p), 6000 // p + 1)[:6000]
    c["acgt_pal"] = np.tile(np.array([0, 1, 2, 3], np.uint8), 1500)      # its own reverse complement: T = XX
    c["ac"] = np.tile(np.array([0, 1], np.uint8), 3000)
    c["at"] = np.tile(np.array([0, 3], np.uint8), 3000)
    x = _rand("x3000", 3000)
    c["x_rcx"] = np.concatenate([x, rc(x)])
    c["x_x"] = np.concatenate([x, x])
    c["x_x_x_rc"] = np.concatenate([x, x, rc(x), x])
    c["polyA_then_C"] = np.concatenate([np.zeros(5000, np.uint8), np.ones(1, np.uint8)])
    c["C_then_polyA"] = np.concatenate([np.ones(1, np.uint8), np.zeros(5000, np.uint8)])
    c["fib"] = _fib(8000)
    for name, (g, _) in _multi_contig().items():
        c[name] = g
    return c


def contig_lens(name, codes):
    m = _multi_contig()
    return list(m[name][1]) if name in m else [int(codes.shape[0])]


def contigs(name, codes):
    """[(name, length)] as simdata.write_fasta names them"""
    return [(f"chr{i + 1}", l) for i, l in enumerate(contig_lens(name, codes))]


def _reads(name, g, lens=None):
    rng = _rng("reads " + name)
    n = g.shape[0]
    out = []
    for rl in (25, 60, 100):
        k = min(rl, n)
        s = int(rng.integers(0, n - k + 1))
        r = g[s:s + k].copy()
        if rl > n:
            r = np.concatenate([r, rng.integers(0, 4, rl - k).astype(np.uint8)])      # the genome is shorter than the read: padded with random bases
        out.append(r)
        r2 = rc(r)
        r2[len(r2) // 2] = (r2[len(r2) // 2] + 1) % 4
        out.append(r2)
    out.append(np.zeros(40, np.uint8))
    out.append(np.tile(g, 100 // n + 2)[:100].astype(np.uint8))      # runs off the end of the text and across the forward / reverse boundary
    out.append(np.full(60, 4, np.uint8))
    k = min(17, n)
    s = int(rng.integers(0, n - k + 1))
    out.append(np.concatenate([g[s:s + k], rng.integers(0, 4, 17 - k).astype(np.uint8)]))      # shorter than the minimum seed length
    if lens and len(lens) > 1:
        out.append(g[max(0, lens[0] - 50):lens[0] + 50].copy())      # straddles the first contig boundary
    return out


def align_cases():
    """name -> (codes, contig lengths, [reads as uint8 codes 0..4])"""
    c = {}
    for n in ALIGN_RAND_LENS:
        c[f"rand{n}"] = _rand(f"rand{n}", n)
    c["polyA300"] = np.zeros(300, np.uint8)
    c["polyA2000"] = np.zeros(2000, np.uint8)
    c["tandem2"] = np.tile(np.array([0, 1], np.uint8), 400)
    c["tandem3"] = np.tile(np.array([2, 0, 3], np.uint8), 300)
    c["acgt_pal"] = np.tile(np.array([0, 1, 2, 3], np.uint8), 150)
    x = _rand("x400", 400)
    c["x_rcx"] = np.concatenate([x, rc(x)])
    c["x_x"] = np.concatenate([x, x])
    out = {name: (g, [int(g.shape[0])], _reads(name, g)) for name, g in c.items()}
    for name, (g, lens) in _multi_contig().items():
        out[name] = (g, list(lens), _reads(name, g, lens))
    return out


ALIGN_NAMES = tuple(f"rand{n}" for n in ALIGN_RAND_LENS) + ("polyA300", "polyA2000", "tandem2", "tandem3", "acgt_pal", "x_rcx", "x_x", "two_equal_contigs", "contig_of_one_base")
MANY_REGIONS = ("polyA2000", "tandem2", "tandem3", "acgt_pal")      # genomes on which some read has more regions than the marking / dedup kernels' first LDS forms hold


def write_fastq(path, reads):
    """ragged reads (codes 0..4) as FASTQ, names r0, r1, ..."""
    asc = np.frombuffer(b"ACGTN", dtype=np.uint8)
    with open(path, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@r%d\n" % i + asc[r].tobytes() + b"\n+\n" + b"I" * len(r) + b"\n")
