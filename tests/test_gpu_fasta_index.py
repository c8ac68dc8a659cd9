"""GPU: `bwa-amd index` (the bwagpu_fasta_* parse kernels + bwagpu_index_build) on the MI355X against the reference's `bwa index` --
the corpus of tests/test_fasta_index.py through the real kernels (the mock runs lanes one at a time and cannot catch wave-level
bugs), a 64 Mbp FASTA with GRCh38-like ambiguity structure through the command line at two chunk sizes, and `bwa-amd mem` on the
result against `bwa mem` on the reference's index."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import degenerate_cases
import fasta_cases
import refapi
from bwa_amd import simdata
from bwa_amd.index import build_index_from_fasta, parse_fasta

pytestmark = pytest.mark.gpu

EXTS = ("pac", "ann", "amb", "bwt", "sa")


def need_ref():
    assert refapi.have_ref(), "oracle/_ref (the compiled reference) did not travel with the snapshot"


def _diff(a, b):
    return [e for e in EXTS if not filecmp.cmp(a + "." + e, b + "." + e, shallow=False)]


def _ref_index(path, d):
    ref = os.path.join(d, "ref_" + os.path.basename(path))
    with open(path, "rb") as s, open(ref, "wb") as t:
        t.write(s.read())
    subprocess.run([refapi.REF_BWA, "index", ref], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return ref


def test_gpu_fasta_corpus_equals_bwa_index(tmp_path):
    need_ref()
    cases = dict(fasta_cases.small_cases(), **fasta_cases.big_cases())
    for p in fasta_cases.write_all(str(tmp_path), cases):
        ref = _ref_index(p, str(tmp_path))
        for chunk in (None, 4096, 7):
            if chunk == 7 and os.path.getsize(p) > 100_000:
                continue
            mine = str(tmp_path / (f"mine{chunk}_" + os.path.basename(p)))
            build_index_from_fasta(p, mine, chunk_bytes=chunk)
            assert not _diff(mine, ref), (p, chunk, _diff(mine, ref))


def test_gpu_fasta_degenerate_texts_equal_bwa_index(tmp_path):
    """The FASTA route on texts of tests/degenerate_cases.py: a genome of one base, a 20 kb poly-A, contigs of one base, two equal contigs."""
    need_ref()
    cases = degenerate_cases.index_cases()
    for name in ("rand1", "polyA20000", "contig_of_one_base", "two_equal_contigs"):
        g = cases[name]
        fa = str(tmp_path / (name + ".fa"))
        simdata.write_fasta(fa, g, degenerate_cases.contig_lens(name, g))
        refapi.build_index(fa)
        mine = str(tmp_path / ("mine_" + name))
        info = build_index_from_fasta(fa, mine)
        assert info["l_pac"] == g.shape[0] and info["n_seqs"] == len(degenerate_cases.contig_lens(name, g)), name
        assert not _diff(mine, fa), (name, _diff(mine, fa))


def test_gpu_fasta_parse_one_byte_chunks():
    for name, data in fasta_cases.small_cases().items():
        want = parse_fasta(_Bytes(data))
        got = parse_fasta(_Bytes(data), chunk_bytes=1, piece_bytes=5)
        assert np.array_equal(want[0], got[0]) and want[1:5] == got[1:5], name


class _Bytes:
    def __init__(self, data):
        self.data, self.pos = data, 0

    def read(self, n):
        out = self.data[self.pos:self.pos + n]
        self.pos += len(out)
        return out


def mem_sam_pair(cli, runs, args):
    """SAM text (without @PG) of `bwa mem` and of `cli mem`, each on its own (index prefix, input files) of `runs`; both must exit 0."""
    outs = []
    for binary, (idx, files) in zip((refapi.REF_BWA, cli), runs):
        p = subprocess.run([binary, "mem"] + list(args) + [idx] + list(files), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, (binary, p.stderr.decode()[-1000:])
        outs.append(b"\n".join(l for l in p.stdout.split(b"\n") if not l.startswith(b"@PG")))
    return outs


def test_gpu_cli_index_64mbp_and_mem(tmp_path):
    need_ref()
    from bwa_amd import build as b
    _, cli = b.build_host(verbose=False)
    g, lens = simdata.make_genome_large(64_000_000, n_contigs=5, seed=65)
    fa = str(tmp_path / "g64a.fa")
    n_amb = simdata.write_fasta_ambiguous(fa, g, lens, seed=65)
    assert n_amb > 3_000_000
    subprocess.run([refapi.REF_BWA, "index", fa], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    for chunk in ("0", str((1 << 20) + 3)):
        prefix = str(tmp_path / f"gpu{chunk}")
        r = subprocess.run([cli, "index", "-p", prefix, fa], env=dict(os.environ, BWAGPU_FASTA_CHUNK=chunk), capture_output=True)
        assert r.returncode == 0, r.stderr.decode()[-1000:]
        print(r.stderr.decode())
        assert not _diff(prefix, fa), (chunk, _diff(prefix, fa))
    # reads from the original genome: those that overlap N runs and their edges align against random replacement bases
    r1, r2 = simdata.make_reads_pe(g, 20000, seed=66)
    f1, f2 = str(tmp_path / "h1.fq"), str(tmp_path / "h2.fq")
    simdata.write_fastq(f1, r1, suffix="/1"); simdata.write_fastq(f2, r2, suffix="/2")
    outs = mem_sam_pair(cli, ((fa, [f1, f2]), (str(tmp_path / "gpu0"), [f1, f2])), ["-K", "10000000", "-t", "16"])
    assert outs[0] == outs[1], "SAM on the bwa-amd index"
    assert outs[0].count(b"\n") >= 40000
