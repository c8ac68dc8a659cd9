"""The device-side index builder (bwagpu_index_build in bwa_amd/csrc/bwagpu_index.hip, bound by bwa_amd/index.py) must write
the same five files as the reference's `bwa index`.  CPU here: the unmodified HIP source under the mock runtime of
tests/hostsim (rocPRIM's sort/scan replaced by std:: stand-ins); the same code on the GPU in tests/test_gpu_index.py.
The tiny and all-repeat texts of tests/degenerate_cases.py (index_cases) go through every form of the builder here and, unchanged, on the device."""
import filecmp
import os
import numpy as np
import pytest

import degenerate_cases
import hostsim_build
import refapi
import testdata
from bwa_amd import simdata
from bwa_amd.index import build_index


def test_small_index_equals_committed_reference_index(tmp_path):
    g, lens = testdata.small_genome()
    prefix = str(tmp_path / "mine")
    build_index(prefix, g, [(f"chr{i + 1}", l) for i, l in enumerate(lens)], lib_path=hostsim_build.build())
    for ext in ("bwt", "sa", "pac", "ann", "amb"):
        assert filecmp.cmp(prefix + "." + ext, os.path.join(testdata.GOLDEN, "g200k." + ext), shallow=False), ext


@pytest.mark.skipif(not refapi.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("total,seed", [(1003, 5), (65536, 6), (300001, 7)])
def test_index_equals_bwa_index(tmp_path, total, seed):
    g, lens = simdata.make_genome(total, n_contigs=2 if total > 5000 else 1, seed=seed, repeats=total > 5000)
    if total < 5000:
        lens = [total]
        g[100:400] = np.tile(g[100:130], 10)       # an exact tandem repeat: deep prefix doubling
    fa = str(tmp_path / "ref.fa")
    simdata.write_fasta(fa, g, lens)
    refapi.build_index(fa)
    prefix = str(tmp_path / "mine")
    build_index(prefix, g, [(f"chr{i + 1}", l) for i, l in enumerate(lens)], lib_path=hostsim_build.build())
    for ext in ("bwt", "sa", "pac", "ann", "amb"):
        assert filecmp.cmp(prefix + "." + ext, fa + "." + ext, shallow=False), ext


@pytest.mark.skipif(not refapi.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("env", [{"BWAGPU_INDEX_BUCKET_BASES": "2"}, {"BWAGPU_INDEX_BUCKET_BASES": "3", "BWAGPU_INDEX_SPLIT_SORT": "1"}])
def test_index_bucketed_and_split_sort_paths(tmp_path, monkeypatch, env):
    """Large-genome code paths forced on a small genome: several first-pass buckets, and the two-sort form of a doubling
    round (used when group number + rank exceed 64 bits)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g, lens = simdata.make_genome(50_000, n_contigs=2, seed=11)
    g[7000:9000] = np.tile(g[7000:7050], 40)          # long exact tandem repeat
    g[-300:] = 0                                       # poly-A up to the end of the text: exercises the terminator ordering
    fa = str(tmp_path / "ref.fa")
    simdata.write_fasta(fa, g, lens)
    refapi.build_index(fa)
    prefix = str(tmp_path / "mine")
    build_index(prefix, g, [(f"chr{i + 1}", l) for i, l in enumerate(lens)], lib_path=hostsim_build.build())
    for ext in ("bwt", "sa", "pac", "ann", "amb"):
        assert filecmp.cmp(prefix + "." + ext, fa + "." + ext, shallow=False), ext


# the builder's forms: one bucket and one sort per doubling round; 16 and 4096 first-pass buckets; 64 buckets with the two-sort form of a round
BUILDER_ENVS = [{}, {"BWAGPU_INDEX_BUCKET_BASES": "2"}, {"BWAGPU_INDEX_BUCKET_BASES": "3", "BWAGPU_INDEX_SPLIT_SORT": "1"}, {"BWAGPU_INDEX_BUCKET_BASES": "6"}]
EXTS = ("bwt", "sa", "pac", "ann", "amb")


@pytest.fixture(scope="module")
def degenerate_ref(tmp_path_factory):
    """`bwa index` of every text of the corpus, once for the module: name -> (codes, contigs, FASTA path = prefix of the reference's files)"""
    d = tmp_path_factory.mktemp("degenerate_ref")
    out = {}
    for name, g in degenerate_cases.index_cases().items():
        fa = str(d / (name + ".fa"))
        simdata.write_fasta(fa, g, degenerate_cases.contig_lens(name, g))
        refapi.build_index(fa)
        out[name] = (g, degenerate_cases.contigs(name, g), fa)
    return out


def degenerate_mismatches(ref, d, lib_path=None, sa_intv=None):
    """Builds every text of `ref` under the environment as it stands; returns one message per text whose files differ from the reference's (or whose
    build raised).  sa_intv: compare .sa only, against ref[name][2] + f".sa{sa_intv}"."""
    bad = []
    for name, (g, contigs, fa) in ref.items():
        prefix = os.path.join(str(d), "mine_" + name)
        try:
            if sa_intv is None:
                build_index(prefix, g, contigs, lib_path=lib_path)
                diff = [e for e in EXTS if not filecmp.cmp(prefix + "." + e, fa + "." + e, shallow=False)]
            else:
                build_index(prefix, g, contigs, lib_path=lib_path, sa_intv=sa_intv)
                diff = [] if filecmp.cmp(prefix + ".sa", fa + f".sa{sa_intv}", shallow=False) else ["sa"]
        except Exception as e:      # (a text the builder rejects is a mismatch like any other: the reference built it)
            diff = [repr(e)[:200]]
        if diff:
            bad.append(f"{name} (l_pac {g.shape[0]}): differs from bwa index in {diff}")
        for e in EXTS:
            if os.path.exists(prefix + "." + e):
                os.remove(prefix + "." + e)
    return bad


@pytest.mark.skipif(not refapi.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("env", BUILDER_ENVS, ids=["default", "buckets2", "buckets3_split_sort", "buckets6"])
def test_index_degenerate_texts_equal_bwa_index(tmp_path, monkeypatch, degenerate_ref, env):
    """Every text of tests/degenerate_cases.py: all five files equal `bwa index`'s, under each form of the builder."""
    for k in ("BWAGPU_INDEX_BUCKET_BASES", "BWAGPU_INDEX_SPLIT_SORT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert len(degenerate_ref) == 75
    bad = degenerate_mismatches(degenerate_ref, tmp_path, lib_path=hostsim_build.build())
    assert not bad, f"{len(bad)} of {len(degenerate_ref)} texts under {env}:\n" + "\n".join(bad)
