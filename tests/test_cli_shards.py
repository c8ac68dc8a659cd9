"""`bwa-amd mem` with every batch split over several devices (BWAGPU_CLI_MULTI=split), under every switch that moves a stage onto the device: device_sub
(bwa_amd/csrc/host/main_mem.cpp) joins the shards' results in read order, and the SAM must stay `bwa mem`'s byte for byte except for @PG.  The inputs are the
smallest that reach every arm of that gathering: gap-rich reads (CIGARs of 7 or more operations point into a shard's operation array, and the reference moves
when the arrays are joined), a second shard without a single region (its per-pair records are filled in on the host), and one pair over three devices (more
devices than pairs).  Each run also has to show its switch's own trace line: a run that fell back to the host path does not pass.
CPU variant: the command line on 2 and 3 devices of the mock runtime.  GPU variant (-m gpu): the real binary on devices 0 and 1 where the box has two, else on the
one device (a single shard's blocks are handed over as they are)."""
import os
import re
import subprocess

import numpy as np
import pytest

import refapi
import testdata
from bwa_amd import simdata
from test_cli import _body, _run, _sim_cli

OPTS = ["-K", "100000000", "-t", "2"]
ENV = dict(BWAGPU_CLI_STREAMS="2", BWAGPU_CLI_SERIALIZE="1", BWAGPU_PTAB_M="6", BWAGPU_CLI_TRACE="1", BWAGPU_CLI_MULTI="split")
RG = ["-C", "-R", "@RG\\tID:x\\tSM:y"]
N = 24      # pairs, or single-end reads, per input: twelve per shard on two devices, eight on three

# the trace line of a switch: the count it must show above zero
T_PAIR = rb"(\d+) pairs paired from device records \(BWAGPU_CLI_PAIR\)"
T_RESCUE = rb"(\d+) pairs merged on the device \(BWAGPU_CLI_RESCUE\)"
T_SAMPE = rb"(\d+) pairs finished from the device's pair records \(BWAGPU_CLI_SAMPE\)"
T_TEXT_PE = rb"(\d+) pairs written from device SAM text \(BWAGPU_CLI_SAMTEXT\)"
T_TEXT_SE = rb"(\d+) reads written from device SAM text \(BWAGPU_CLI_SAMTEXT\)"
T_PESTAT = rb"insert-size windows from (\d+) device\(s\) \(BWAGPU_CLI_PESTAT\)"
T_PRIMARY = rb"(\d+) reads finalized from device primary/mapQ records \(BWAGPU_CLI_PRIMARY\)"
T_ALNS = rb"(\d+) reads finalized from device alignment records \(BWAGPU_CLI_ALNS\)"
T_FASTQ = rb"\((\d+) reads\) parsed on the device"

# (name, switches, command-line options, trace lines)
PE_SETS = [
    ("default", {}, [], []),
    ("pair", {"PAIR": "1"}, [], [T_PAIR]),
    ("rescue", {"RESCUE": "1"}, [], [T_RESCUE]),
    ("sampe", {"SAMPE": "1"}, [], [T_SAMPE]),
    ("samtext", {"SAMTEXT": "1"}, [], [T_TEXT_PE]),
    ("pestat_samtext", {"PESTAT": "1", "SAMTEXT": "1"}, [], [T_PESTAT, T_TEXT_PE]),
    ("host_matesw", {"MATESW": "0"}, [], []),
    ("host_cigars", {"CIGARS": "0"}, [], []),
    ("samtext_fastq", {"SAMTEXT": "1", "FASTQ": "1"}, [], [T_TEXT_PE, T_FASTQ]),
    ("sampe_fastq", {"SAMPE": "1", "FASTQ": "1"}, [], [T_SAMPE, T_FASTQ]),
    ("samtext_fastq_rg", {"SAMTEXT": "1", "FASTQ": "1"}, RG, [T_TEXT_PE, T_FASTQ]),
    ("sampe_fastq_rg", {"SAMPE": "1", "FASTQ": "1"}, RG, [T_SAMPE, T_FASTQ]),
]
SE_SETS = [
    ("default", {}, [], []),
    ("primary", {"PRIMARY": "1"}, [], [T_PRIMARY]),
    ("alns", {"ALNS": "1"}, [], [T_ALNS]),
    ("samtext", {"SAMTEXT": "1"}, [], [T_TEXT_SE]),
    ("samtext_fastq", {"SAMTEXT": "1", "FASTQ": "1"}, [], [T_TEXT_SE, T_FASTQ]),
]
PE_INPUTS, SE_INPUTS = ("gaps_pe", "empty_pe"), ("gaps_se", "empty_se")
CASES = [(i, s) for i in PE_INPUTS for s in PE_SETS] + [(i, s) for i in SE_INPUTS for s in SE_SETS]
IDS = [f"{i}-{s[0]}" for i, s in CASES]


def _records(sam: bytes):
    return [l.split(b"\t") for l in sam.split(b"\n") if l and not l.startswith(b"@")]


class Inputs:
    """The files of every input, written once, and the reference's SAM of each (input, options), computed once."""

    def __init__(self, d, prefix, g):
        self.prefix, self.files, self.want = prefix, {}, {}

        def fq(name, reads):
            simdata.write_fastq(str(d / name), reads)
            return str(d / name)

        rng = np.random.default_rng(915)
        r1, r2 = simdata.make_reads_pe(g, N, seed=911, sub=0.02, dele=0.03, ins=0.03)
        self.files["gaps_pe"] = [fq("gaps_1.fq", r1), fq("gaps_2.fq", r2)]
        self.files["gaps_se"] = [fq("gaps_se.fq", simdata.make_reads_se(g, N, seed=912, sub=0.02, dele=0.03, ins=0.03))]
        r1, r2 = simdata.make_reads_pe(g, N // 2, seed=913)
        noise = lambda: rng.integers(0, 4, size=(N // 2, r1.shape[1]), dtype=np.uint8)
        self.files["empty_pe"] = [fq("empty_1.fq", np.concatenate([r1, noise()])), fq("empty_2.fq", np.concatenate([r2, noise()]))]
        self.files["empty_se"] = [fq("empty_se.fq", np.concatenate([simdata.make_reads_se(g, N // 2, seed=914), noise()]))]
        r1, r2 = simdata.make_reads_pe(g, 1, seed=916)
        self.files["one_pair"] = [fq("one_1.fq", r1), fq("one_2.fq", r2)]

    def reference(self, name, extra):
        key = (name, tuple(extra))
        if key not in self.want:
            self.want[key] = _run(refapi.REF_BWA, OPTS + extra + [self.prefix] + self.files[name])
            self.check_reaches(name, _records(self.want[key]))
        return self.want[key]

    @staticmethod
    def check_reaches(name, rec):
        """what makes the input reach its arm, on the reference's own SAM (records are in read order; the first N, or 2 N, names are r0.. in order)"""
        second = [r for r in rec if int(r[0][1:]) >= N // 2]
        if name.startswith("gaps"):       # a CIGAR of 7 or more operations lives in the operation array: behind another shard's, its reference is rebased
            assert any(len(re.findall(rb"\d+[MIDSH]", r[5])) >= 7 for r in second), "no read of the second half has a CIGAR of 7 or more operations"
        if name.startswith("empty"):      # random bases: no region in the second half, hence none in the last shard of 2 and of 3 devices
            assert second and all(int(r[1]) & 4 and r[5] == b"*" for r in second), "a read of the second half is mapped"
            assert any(not int(r[1]) & 4 for r in rec), "nothing is mapped at all"


def _check(inp, cli, name, sets, env, one_pair=False):
    _, switches, extra, traces = sets
    e = dict(os.environ, **env)
    e.update({"BWAGPU_CLI_" + k: v for k, v in switches.items()})
    p = subprocess.run([cli, "mem"] + OPTS + extra + [inp.prefix] + inp.files[name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert _body(p.stdout) == inp.reference(name, extra), f"{name} {switches} {extra}: SAM differs from bwa mem"
    for t in traces:
        m = re.search(t, p.stderr)
        print(f"{name} {switches}: {m.group(0).decode() if m else None}")
        assert m and int(m.group(1)) > 0, f"{name} {switches}: no trace line {t!r} with a count above zero\n" + p.stderr.decode()[-1500:]
    return p.stderr


@pytest.fixture(scope="module")
def sim_inputs(tmp_path_factory):
    prefix, g = testdata.small_index()
    return Inputs(tmp_path_factory.mktemp("shards_sim"), prefix, g)


def _mock_env(n_dev):
    return dict(ENV, MOCK_HIP_DEVICES=str(n_dev), BWAGPU_DEVICES=",".join(str(d) for d in range(n_dev)))


@pytest.mark.skipif(not refapi.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("n_dev", (2, 3))
@pytest.mark.parametrize("name,sets", CASES, ids=IDS)
def test_sim_cli_shards(sim_inputs, name, sets, n_dev):
    err = _check(sim_inputs, _sim_cli(), name, sets, _mock_env(n_dev))
    assert re.search(rb"\d+ reads on %d device\(s\)" % n_dev, err), "the batch was not split over the devices"


# One pair cannot be split: device_sub uses as many devices as there are pairs.  With a single pair mem_pestat has no orientation with enough pairs, so nothing
# is paired or rescued and those switches' counts may be zero: the switches whose count is the number of pairs they finished or wrote keep the check
@pytest.mark.skipif(not refapi.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("sets", [s for s in PE_SETS if s[0] in ("default", "sampe", "samtext", "pestat_samtext", "host_cigars", "samtext_fastq_rg")], ids=lambda s: s[0])
def test_sim_cli_one_pair_on_three_devices(sim_inputs, sets):
    err = _check(sim_inputs, _sim_cli(), "one_pair", sets, _mock_env(3))
    assert b"2 reads on 1 device(s)" in err, "more devices than pairs: the pair goes to one"


# ---- on hardware ---------------------------------------------------------------------------------------------------------------------------------------
def _n_gpus():
    import torch
    return torch.cuda.device_count()


@pytest.fixture(scope="module")
def gpu_inputs(tmp_path_factory):
    assert refapi.have_ref(), "oracle/_ref (the compiled reference) is missing on the GPU box"
    from bwa_amd import build as b
    _, cli = b.build_host(verbose=False)
    fa, g = testdata.medium_index()
    inp = Inputs(tmp_path_factory.mktemp("shards_gpu"), fa, g)
    inp.cli = cli
    inp.env = dict(BWAGPU_CLI_TRACE="1", BWAGPU_CLI_MULTI="split", **({"BWAGPU_DEVICES": "0,1"} if _n_gpus() >= 2 else {}))
    return inp


@pytest.mark.gpu
@pytest.mark.parametrize("name,sets", CASES, ids=IDS)
def test_gpu_cli_shards(gpu_inputs, name, sets):
    """one process per run, on devices 0 and 1 where there are two; on one device the same runs pin the single shard's hand-over"""
    err = _check(gpu_inputs, gpu_inputs.cli, name, sets, gpu_inputs.env)
    n_dev = 2 if "BWAGPU_DEVICES" in gpu_inputs.env else 1
    assert re.search(rb"\d+ reads on %d device\(s\)" % n_dev, err), err.decode()[-800:]


@pytest.mark.gpu
def test_gpu_cli_shards_on_two_devices(gpu_inputs):
    """whether the runs above split their batches at all: with one GPU they did not, and the report says so"""
    n = _n_gpus()
    if n < 2:
        pytest.skip(f"this box has {n} GPU(s): the multi-device path of bwa-amd mem (BWAGPU_DEVICES, hipMemcpyPeer) needs two and was NOT exercised on hardware by this run")
    p = subprocess.run([gpu_inputs.cli, "mem"] + OPTS + ["-v", "3", gpu_inputs.prefix] + gpu_inputs.files["gaps_pe"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **gpu_inputs.env))
    assert p.returncode == 0 and b"index copied to 2 devices; every batch is split over them" in p.stderr, p.stderr.decode()[-800:]
