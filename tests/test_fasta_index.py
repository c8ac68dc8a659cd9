"""`bwa-amd index` (bwagpu_fasta_* + bwagpu_index_build) against the reference's `bwa index`: the five files must be byte-identical
for FASTA inputs with every structure kseq_read + add1 (kseq.h:175-215, bntseq.c:232-278) gives a meaning to -- ambiguity codes,
CRLF, odd headers, blank lines, records without bases.  CPU: the unmodified HIP source under the mock runtime of tests/hostsim;
the same cases on the GPU in tests/test_gpu_fasta_index.py."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import fasta_cases
import hostsim_build
import refapi
from bwa_amd.api import BwaGpuError
from bwa_amd.index import build_index_from_fasta, parse_fasta

EXTS = ("pac", "ann", "amb", "bwt", "sa")
need_ref = pytest.mark.skipif(not refapi.have_ref(), reason="oracle/_ref not built")


def _sim_cli():
    import test_cli
    return test_cli._sim_cli()


def _same_files(a, b):
    return [e for e in EXTS if not filecmp.cmp(a + "." + e, b + "." + e, shallow=False)]


def _ref_index(path, d):
    """`bwa index` of a copy of path in d (the reference names its files after the input)"""
    ref = os.path.join(d, "ref_" + os.path.basename(path))
    with open(path, "rb") as s, open(ref, "wb") as t:
        t.write(s.read())
    subprocess.run([refapi.REF_BWA, "index", ref], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return ref


@need_ref
@pytest.mark.parametrize("which", ["small", "big"])
def test_fasta_index_equals_bwa_index(tmp_path, which):
    cases = fasta_cases.small_cases() if which == "small" else fasta_cases.big_cases()
    lib = hostsim_build.build()
    for p in fasta_cases.write_all(str(tmp_path), cases):
        ref = _ref_index(p, str(tmp_path))
        mine = str(tmp_path / ("mine_" + os.path.basename(p)))
        info = build_index_from_fasta(p, mine, lib_path=lib)
        assert not _same_files(mine, ref), (p, _same_files(mine, ref))
        with open(ref + ".amb") as f:
            l_pac, n_seqs, n_holes = map(int, f.readline().split())
        assert (info["l_pac"], info["n_seqs"], info["n_holes"]) == (l_pac, n_seqs, n_holes)


@need_ref
def test_fasta_index_cli_equals_bwa_index(tmp_path):
    cli = _sim_cli()
    env = dict(os.environ, BWAGPU_FASTA_CHUNK="4096")
    for p in fasta_cases.write_all(str(tmp_path), fasta_cases.small_cases()):
        ref = _ref_index(p, str(tmp_path))
        mine = str(tmp_path / ("cli_" + os.path.basename(p)))
        r = subprocess.run([cli, "index", "-p", mine, p], env=env, capture_output=True)
        assert r.returncode == 0, r.stderr.decode()
        assert not _same_files(mine, ref), (p, _same_files(mine, ref))
    # -6 and the default prefix, -a / -b accepted
    p = str(tmp_path / "multi_contig.fa")
    r = subprocess.run([cli, "index", "-6", "-a", "bwtsw", "-b", "10000000", p], env=env, capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert not _same_files(p + ".64", str(tmp_path / "ref_multi_contig.fa"))


@pytest.mark.parametrize("chunk", [1, 2, 3, 7, 4096])
def test_fasta_parse_is_independent_of_chunks_and_pieces(tmp_path, chunk):
    """Random feed pieces and tiny device chunks cut headers, CRLF pairs, holes and .pac bytes everywhere: same result."""
    lib = hostsim_build.build()
    rng = np.random.default_rng(chunk)
    for name, data in fasta_cases.small_cases().items():
        if chunk < 7 and len(data) > 3000:
            data = data[:2000] + data[-1000:]                 # (one-byte chunks are slow under the lane-serial mock)
        want = parse_fasta(_BytesPieces(data, rng, 1 << 20), lib_path=lib)
        got = parse_fasta(_BytesPieces(data, rng, 11), lib_path=lib, chunk_bytes=chunk)
        assert np.array_equal(want[0], got[0]) and want[1:5] == got[1:5], (name, chunk)


class _BytesPieces:
    """a file object whose read() returns pieces of random length (1 .. max_piece)"""
    def __init__(self, data, rng, max_piece):
        self.data, self.pos, self.rng, self.max_piece = data, 0, rng, max_piece

    def read(self, n):
        k = min(n, int(self.rng.integers(1, self.max_piece + 1)))
        out = self.data[self.pos:self.pos + k]
        self.pos += len(out)
        return out


@pytest.mark.parametrize("name", sorted(fasta_cases.REJECTED))
def test_rejected_input_leaves_no_files(tmp_path, name):
    lib = hostsim_build.build()
    p = str(tmp_path / "bad.fa")
    with open(p, "wb") as f:
        f.write(fasta_cases.REJECTED[name])
    prefix = str(tmp_path / "idx")
    with pytest.raises(BwaGpuError) as e:
        build_index_from_fasta(p, prefix, lib_path=lib, chunk_bytes=5)
    assert "invalid argument" in str(e.value)
    if name in ("nul_byte", "high_byte", "plus_line", "at_line", "at_before_gt"):
        assert "byte offset" in str(e.value)
    if refapi.have_ref():
        r = subprocess.run([_sim_cli(), "index", "-p", prefix, p], capture_output=True)
        assert r.returncode != 0
    assert not [f for f in os.listdir(tmp_path) if f.startswith("idx")]


def test_error_offset_is_the_first_bad_byte(tmp_path):
    lib = hostsim_build.build()
    data = b"xx\n>a\nACGT\nAC\x00G\x80T\n"
    with pytest.raises(BwaGpuError, match="byte offset 13"):
        parse_fasta(_BytesPieces(data, np.random.default_rng(1), 3), lib_path=lib, chunk_bytes=4)
