"""GPU: `mem -p` on the device FASTQ reader (bwa_amd/csrc/dev_fastq_smart.h) on hardware -- the corpus of tests/fastq_smart_cases.py against the
compiled reference's bseq_read + bseq_classify (the mock runtime of the CPU tests runs lanes one at a time and cannot see scan errors across
wavefronts and blocks), batches whose runs of equal names lie on wavefront and block boundaries, and `bwa-amd mem -p` with BWAGPU_CLI_FASTQ=1
BWAGPU_CLI_SMARTPE_DEV=1 against the reference `bwa mem -p`."""
import os
import subprocess

import pytest

import bgzf_cases
import fastq_cases
import fastq_smart_cases as sc
import refapi
import testdata
from bwa_amd import api

pytestmark = pytest.mark.gpu

HARD = sc.hardware_cases()


@pytest.fixture(scope="module")
def parser():
    assert refapi.have_ref(), "oracle/_ref (the compiled reference) is missing on the GPU box"
    p = api.FastqParser()
    yield p
    p.close()


def test_gpu_corpus_equals_bseq_read_and_bseq_classify(parser):
    for name, case in sorted(sc.cases().items()):
        for chunk in sc.CHUNKS:
            sc.run_smart(parser, case, chunk)


@pytest.mark.parametrize("name", sorted(HARD))
def test_gpu_runs_on_hardware_boundaries(parser, name):
    case = HARD[name]
    want = sc.ref_smart(case, 1 << 20)
    assert len(want) == 1
    cls = want[0]["cls"]
    if name == "runs_at_boundaries_a":      # the reference's answer is what the case was built for
        assert len(cls) == 1500 and cls[62:67] == [0, 1, 2, 0, 0] and cls[255:260] == [1, 2, 1, 2, 0] and cls[1023:1027] == [1, 2, 0, 0] and sum(cls) == 12
    if name == "runs_at_boundaries_b":
        assert len(cls) == 1500 and cls[63:68] == [0, 1, 2, 0, 0] and cls[256:262] == [1, 2, 1, 2, 0, 0] and cls[1024:1027] == [1, 2, 0] and sum(cls) == 12
    if name == "run_of_700":
        assert cls[300:303] == [0, 1, 2] and cls[301:1001] == [1, 2] * 350 and cls[1001] == 0
    if name == "all_pairs_1024":
        assert cls == [1, 2] * 512
    if name == "all_single_1025":
        assert cls == [0] * 1025
    for chunk in (1 << 20, 1000, 150):      # one batch; batches of a few hundred reads; of about thirty
        sc.run_smart(parser, case, chunk)


def test_gpu_run_of_700_at_every_parity(parser):
    """the same long run one read further on: its parity against the blocks of the scan changes, the classes relative to its start do not"""
    rng = __import__("numpy").random.default_rng(735)
    for lead in (255, 256):
        case = sc.named(rng, [b"h%d" % i for i in range(lead)] + [b"same"] * 701 + [b"tail"])
        assert sc.ref_smart(case, 1 << 20)[0]["cls"] == [0] * lead + [1, 2] * 350 + [0, 0]
        sc.run_smart(parser, case, 1 << 20)


def test_gpu_irregular_and_windows(parser):
    irregular = fastq_cases.irregular_cases()
    for name in ("crlf", "two_line_seq", "no_final_newline"):
        n_cut = {chunk: sc.run_irregular(parser, irregular[name], chunk) for chunk in (1, 150, 1 << 20)}
        assert n_cut[1 << 20] == 0 and n_cut[1] > 0, name
    sc.run_windows(parser, HARD["runs_at_boundaries_a"], 3000)
    sc.run_windows(parser, sc.cases()["cut_runs"], 150)


def test_gpu_bgzf_windows(parser):
    for case, chunk in ((HARD["runs_at_boundaries_b"], 2000), (HARD["run_of_700"], 1 << 20), (sc.cases()["cut_runs"], 150)):
        sc.run_smart_bgzf(parser, case, bgzf_cases.bgzf_file(case["files"][0], 1900, seed=4), chunk)


def test_gpu_cli_smartpe(tmp_path):
    assert refapi.have_ref(), "oracle/_ref (the compiled reference) is missing on the GPU box"
    from bwa_amd import build as b
    _, cli = b.build_host(verbose=False)
    prefix, g = testdata.small_index()
    f = str(tmp_path / "inter.fq")
    n_reads = sc.write_interleaved(f, g, 300, set(range(0, 300, 23)) | {150, 151, 299}, seed=833)
    env = dict(os.environ, BWAGPU_CLI_FASTQ="1", BWAGPU_CLI_SMARTPE_DEV="1", BWAGPU_CLI_TRACE="1")
    args = ["-K", "3000", "-t", "4", "-p", "-C", prefix, f]
    want, _ = fastq_cases.run_cli(refapi.REF_BWA, args, None)
    p = subprocess.run([cli, "mem"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert b"\n".join(l for l in p.stdout.split(b"\n") if not l.startswith(b"@PG")) == want
    tr = tuple(int(x) for x in fastq_cases.TRACE.search(p.stderr).groups())
    assert tr[0] >= 20 and tr[1] == n_reads and tr[2] == 0, tr
