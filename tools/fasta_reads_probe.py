#!/usr/bin/env python3
"""The device reader for FASTA read files (bwa_amd/csrc/dev_fasta_reads.h), measured: profiles/dev_fasta_reads.md has the results.
  python tools/fasta_reads_probe.py --resources          registers, LDS and instruction count of the kernels (CPU only)
  python tools/fasta_reads_probe.py [--pairs N --long M] the input stage alone, one JSON line per file set: N pairs of 2 x 150 bp unwrapped (one
                                                         file, and both files of mates) and M reads of 10 kb wrapped at 60, through
                                                         bwagpu_fastq_batch_fasta and -- the same reads as four-line FASTQ -- bwagpu_fastq_batch, in
                                                         one process: wall time per call and HIP-event kernel times per pass (kernel_ms), median,
                                                         minimum and maximum of calls 2 .. --calls
  python tools/fasta_reads_probe.py --host [...]         the same FASTA files through the streaming host reader and encoder (bwa-amd mem with
                                                         BWAGPU_CLI_PARSE_ONLY=3 on the test suite's small index), three runs each"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def resources():
    import isa_resources
    from bwa_amd import build
    for r in isa_resources.kernels(os.path.join(build.CSRC, "bwagpu_index.hip")):
        if "k_fr_" in r[0] or r[0] in ("k_fq_count", "k_fq_index", "k_fq_emit"):
            print(dict(zip(("kernel", "vgpr", "agpr", "sgpr", "scratch", "lds", "spill", "wg", "instrs"), r)))


def texts(n_pairs, n_long):
    """{set: (FASTA files, FASTQ files of the same reads, reads)} -- uniform random bases: the reader does not look at what they spell"""
    import numpy as np
    rng = np.random.default_rng(77)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)

    def short(mate):
        b = acgt[rng.integers(0, 4, (n_pairs, 150))]
        fa = b"".join(b">frag%d/%d\n%b\n" % (i, mate, b[i].tobytes()) for i in range(n_pairs))
        fq = b"".join(b"@frag%d/%d\n%b\n+\n%b\n" % (i, mate, b[i].tobytes(), b"I" * 150) for i in range(n_pairs))
        return fa, fq

    def long_():
        fa, fq = [], []
        for i in range(n_long):
            s = acgt[rng.integers(0, 4, 10000)].tobytes()
            fa.append(b">long%d\n" % i + b"\n".join(s[o:o + 60] for o in range(0, len(s), 60)) + b"\n")
            fq.append(b"@long%d\n%b\n+\n%b\n" % (i, s, b"I" * len(s)))
        return b"".join(fa), b"".join(fq)

    a1, q1 = short(1)
    a2, q2 = short(2)
    al, ql = long_()
    return {"short_one_file": ([a1], [q1], n_pairs), "short_pair": ([a1, a2], [q1, q2], 2 * n_pairs), "long_wrapped_60": ([al], [ql], n_long)}


def stats(xs):
    xs = xs[1:] if len(xs) > 1 else xs
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def measure(P, call, files, n_reads, calls):
    import numpy as np
    from bwa_amd import api
    bufs = [np.frombuffer(f, dtype=np.uint8) for f in files]
    o = api.FastqOut()
    wall, k = [], [[], [], []]
    for _ in range(calls):
        t = time.perf_counter()
        rc = call(P.h, bufs[0].ctypes.data, len(files[0]), 1, bufs[1].ctypes.data if len(bufs) > 1 else None, len(files[1]) if len(bufs) > 1 else 0, 1, 1 << 30, C.byref(o))
        wall.append((time.perf_counter() - t) * 1e3)
        assert rc == 0 and o.status == api.FQ_END and o.n_reads == n_reads, (rc, o.status, o.n_reads)
        for j in range(3):
            k[j].append(o.kernel_ms[j])
        P.L.bwagpu_fastq_out_free(C.byref(o))
    nbytes = sum(len(f) for f in files)
    w = stats(wall)
    return {"text_bytes": nbytes, "wall_ms": w, "kernel_ms": {"line_passes": stats(k[0]), "cut": stats(k[1]), "emit": stats(k[2])},
            "mreads_per_s": round(n_reads / w["median"] / 1e3, 3), "gb_per_s": round(nbytes / w["median"] / 1e6, 3)}


def host_runs(a, sets):
    import testdata
    prefix, _ = testdata.small_index()
    cli = os.path.join(ROOT, "bwa_amd", "bwa-amd")
    os.makedirs(a.cache, exist_ok=True)
    for name, (fa, _, n_reads) in sets.items():
        paths = []
        for k, f in enumerate(fa):
            p = os.path.join(a.cache, f"fasta_reads_probe_{name}_{k}.fa")
            with open(p, "wb") as fh:
                fh.write(f)
            paths.append(p)
        rows = []
        for _ in range(3):
            p = subprocess.run([cli, "mem", "-t", "16", "-K", "1000000000", prefix] + paths, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                               env=dict(os.environ, BWAGPU_CLI_PARSE_ONLY="3"), timeout=600)
            err = p.stderr.decode()
            m, e = re.search(r"parsed (\d+) records \((\d+) bp\) in ([0-9.]+) s", err), re.search(r"encoded in ([0-9.]+) s", err)
            assert p.returncode == 0 and m and int(m.group(1)) == n_reads, err[-1000:]
            rows.append({"parse_and_encode_s": float(m.group(3)), "encode_s": float(e.group(1)) if e else None})
        print(json.dumps({"set": name, "reads": n_reads, "text_bytes": sum(len(f) for f in fa), "host_reader": rows}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--host", action="store_true", help="the streaming host reader's runs instead of the library calls")
    ap.add_argument("--pairs", type=int, default=300_000)
    ap.add_argument("--long", type=int, default=9_000)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--cache", default=os.environ.get("BWA_AMD_CACHE", "/tmp/bwa_amd_bench"))
    a = ap.parse_args()
    if a.resources:
        return resources()
    sets = texts(a.pairs, a.long)
    if a.host:
        return host_runs(a, sets)
    from bwa_amd import api
    P = api.FastqParser()
    for name, (fa, fq, n_reads) in sets.items():
        out = {"set": name, "reads": n_reads, "calls": a.calls,
               "fasta": measure(P, P.L.bwagpu_fastq_batch_fasta, fa, n_reads, a.calls), "fastq": measure(P, P.L.bwagpu_fastq_batch, fq, n_reads, a.calls)}
        bases = n_reads * (10000 if name.startswith("long") else 150)
        out["emit_ns_per_base"] = {k: round(out[k]["kernel_ms"]["emit"]["median"] * 1e6 / bases, 5) for k in ("fasta", "fastq")}
        print(json.dumps(out), flush=True)
    P.close()


if __name__ == "__main__":
    sys.exit(main())
