#!/usr/bin/env python3
"""`mem -p` on the device FASTQ reader (bwa_amd/csrc/dev_fastq_smart.h), measured: profiles/dev_fastq_smart.md has the results.
  python tools/smartpe_probe.py --resources        registers, LDS and instruction count of the kernels (CPU only)
  python tools/smartpe_probe.py [--pairs N]        one interleaved file of N pairs of 2 x 150 bp (make_reads_pe seed 77 on the bench's 32 Mbp genome) with a
                                                   read without a mate behind every 50th pair: bwagpu_fastq_batch_smart and, beside it, the one-window
                                                   bwagpu_fastq_batch on the same bytes in one process, median of calls 2-6, one JSON line
  python tools/smartpe_probe.py --cli [--pairs N]  bwa-amd mem -p -t 16 -K 100000000 -v 3 on such a file, three rounds each without the switches (the host's
                                                   bseq_classify and two encodes), with BWAGPU_CLI_FASTQ=1 BWAGPU_CLI_SMARTPE_DEV=1, and both with BWAGPU_CLI_SAMTEXT=1"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def resources():
    import isa_resources
    from bwa_amd import build
    for r in isa_resources.kernels(os.path.join(build.CSRC, "bwagpu_index.hip")):
        if "k_fq" in r[0]:
            print(dict(zip(("kernel", "vgpr", "agpr", "sgpr", "scratch", "lds", "spill", "wg", "instrs"), r)))


def interleaved(cache, n_pairs):
    """(path, reads): mates as <name>/1, <name>/2, and a read without a mate behind every 50th pair"""
    import numpy as np
    from bwa_amd import simdata
    os.makedirs(cache, exist_ok=True)
    path = os.path.join(cache, f"smartpe_probe_{n_pairs}.fq")
    n_orphans = (n_pairs + 49) // 50
    if not os.path.exists(path):
        g, _ = simdata.make_genome_large(32_000_000, n_contigs=24, seed=42, threads=4)
        r1, r2 = simdata.make_reads_pe(g, n_pairs + n_orphans, seed=77)
        a = simdata._ASCII
        q = b"I" * r1.shape[1]
        with open(path + ".tmp", "wb") as f:
            for lo in range(0, n_pairs, 50):
                out = []
                for i in range(lo, min(lo + 50, n_pairs)):
                    out.append(b"@frag%d/1\n%b\n+\n%b\n@frag%d/2\n%b\n+\n%b\n" % (i, a[r1[i]].tobytes(), q, i, a[r2[i]].tobytes(), q))
                out.append(b"@lone%d\n%b\n+\n%b\n" % (lo, a[r1[n_pairs + lo // 50]].tobytes(), q))
                f.write(b"".join(out))
        os.replace(path + ".tmp", path)
    return path, 2 * n_pairs + n_orphans


def cli_runs(a):
    import hashlib
    import re
    import subprocess
    import torch
    import bench
    fa, g, _ = bench.build_or_load_index(32.0, a.cache, 0, lambda: torch.cuda.synchronize())
    path, n_reads = interleaved(a.cache, a.pairs)
    cli = os.path.join(ROOT, "bwa_amd", "bwa-amd")
    base = ["mem", "-p", "-t", "16", "-K", "100000000", "-v", "3", fa, path]

    def run(env):
        t = time.perf_counter()
        p = subprocess.run([cli] + base, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, BWAGPU_CLI_TRACE="1", **env), timeout=600)
        wall = time.perf_counter() - t
        err = p.stderr.decode()
        sha = hashlib.sha256(b"\n".join(l for l in p.stdout.split(b"\n") if not l.startswith(b"@PG"))).hexdigest()[:16]
        m = re.search(r"(\d+) reads/s", err)
        busy = re.search(r"stage busy time: .*", err)
        dev = re.search(r"\[D::input\] \d+ batches.*", err)
        n_batches = len(re.findall(r"\[D::timeline\] batch \d+ read ", err))
        return {"rc": p.returncode, "reads_per_s": int(m.group(1)) if m else None, "wall_s": round(wall, 2), "sam_sha": sha, "batches": n_batches,
                "busy": busy.group(0) if busy else "", "input": dev.group(0) if dev else ""}

    dev = {"BWAGPU_CLI_FASTQ": "1", "BWAGPU_CLI_SMARTPE_DEV": "1"}
    sets = [("defaults", {}), ("FASTQ=1 SMARTPE_DEV=1", dev), ("SAMTEXT=1", {"BWAGPU_CLI_SAMTEXT": "1"}), ("SAMTEXT=1 FASTQ=1 SMARTPE_DEV=1", dict(dev, BWAGPU_CLI_SAMTEXT="1"))]
    print(f"[probe] {n_reads} reads in {path}", flush=True)
    for rnd in range(3):
        for name, env in sets:
            r = run(env)
            print(f"[probe] round {rnd + 1} [{name}]: {json.dumps(r)}", flush=True)
            if r["rc"] != 0:
                return 1
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--cli", action="store_true", help="the command-line runs instead of the library calls")
    ap.add_argument("--pairs", type=int, default=327_000, help="327000 pairs and 6540 single reads: 660540 reads, 99 Mbp -- one batch of -K 100000000")
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--cache", default=os.environ.get("BWA_AMD_CACHE", "/tmp/bwa_amd_bench"))
    a = ap.parse_args()
    if a.resources:
        return resources()
    if a.cli:
        return cli_runs(a)
    import numpy as np
    from bwa_amd import api
    path, n_reads = interleaved(a.cache, a.pairs)
    raw = np.fromfile(path, dtype=np.uint8)
    P = api.FastqParser()
    P.reserve(len(raw))
    med = lambda xs: statistics.median(xs[1:]) if len(xs) > 1 else xs[0]
    out = {"pairs": a.pairs, "reads": n_reads, "bytes": len(raw)}
    o = api.FastqSmart()
    wall, k = [], [[], [], [], []]
    for _ in range(a.calls):
        t = time.perf_counter()
        rc = P.L.bwagpu_fastq_batch_smart(P.h, raw.ctypes.data, len(raw), 1, 1 << 30, C.byref(o))
        wall.append((time.perf_counter() - t) * 1e3)
        assert rc == 0 and o.status == api.FQ_END and o.n_reads == n_reads and tuple(o.n_sub) == (n_reads - 2 * a.pairs, 2 * a.pairs), (rc, o.status, o.n_reads, tuple(o.n_sub))
        for j in range(4):
            k[j].append(o.kernel_ms[j])
        P.L.bwagpu_fastq_smart_free(C.byref(o))
    out["batch_smart"] = {"wall_ms": med(wall), "kernel_ms": {"newlines_checks": med(k[0]), "cut": med(k[1]), "classify": med(k[2]), "emit": med(k[3])}}
    q = api.FastqOut()
    wall, k = [], [[], [], []]
    for _ in range(a.calls):
        t = time.perf_counter()
        rc = P.L.bwagpu_fastq_batch(P.h, raw.ctypes.data, len(raw), 1, None, 0, 1, 1 << 30, C.byref(q))
        wall.append((time.perf_counter() - t) * 1e3)
        assert rc == 0 and q.status == api.FQ_END and q.n_reads == n_reads
        for j in range(3):
            k[j].append(q.kernel_ms[j])
        P.L.bwagpu_fastq_out_free(C.byref(q))
    out["batch_one_window"] = {"wall_ms": med(wall), "kernel_ms": {"newlines_checks": med(k[0]), "cut": med(k[1]), "emit": med(k[2])}}
    P.close()
    print(json.dumps(out))


if __name__ == "__main__":
    sys.exit(main())
