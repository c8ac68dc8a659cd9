#!/usr/bin/env python3
"""The BGZF inflate on the device (bwa_amd/csrc/dev_bgzf.h), measured: profiles/dev_bgzf.md has the results.
  python tools/bgzf_probe.py --resources         registers, LDS and instruction count of the kernel (CPU only)
  python tools/bgzf_probe.py [--pairs N]         N pairs of 2 x 150 bp (make_reads_pe seed 77 on the bench's 32 Mbp genome) as two FASTQ files, plain and
                                                 bgzip-compressed (level 6, blocks of 0xff00 text bytes): bwagpu_bgzf_inflate, bwagpu_fastq_batch_bgzf and
                                                 bwagpu_fastq_batch on them in one process, median of calls 2-6, one JSON line
The files stay in --cache for the command-line runs (tools/e2e_probe.py style: bwa-amd mem on the .gz files with and without the switches)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def resources():
    import isa_resources
    from bwa_amd import build
    for r in isa_resources.kernels(os.path.join(build.CSRC, "bwagpu_index.hip")):
        if "k_bz" in r[0]:
            print(dict(zip(("kernel", "vgpr", "agpr", "sgpr", "scratch", "lds", "spill", "wg", "instrs"), r)))


def bgzip(text: bytes, threads: int = 16, block: int = 0xff00, level: int = 6) -> bytes:
    import bgzf_cases

    def one(o):
        t = text[o:o + block]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        return bgzf_cases.bgzf_block(co.compress(t) + co.flush(), len(t), zlib.crc32(t))

    with ThreadPoolExecutor(threads) as ex:
        return b"".join(ex.map(one, range(0, len(text), block))) + bgzf_cases.EOF_MARKER


def inputs(cache, n_pairs):
    from bwa_amd import simdata
    os.makedirs(cache, exist_ok=True)
    paths = [os.path.join(cache, f"bgzf_probe_{n_pairs}_{k}.fq") for k in (1, 2)]
    if not all(os.path.exists(p) and os.path.exists(p + ".gz") for p in paths):
        g, _ = simdata.make_genome_large(32_000_000, n_contigs=24, seed=42, threads=4)
        r1, r2 = simdata.make_reads_pe(g, n_pairs, seed=77)
        for p, r in zip(paths, (r1, r2)):
            simdata.write_fastq(p, r)
            with open(p + ".gz", "wb") as f:
                f.write(bgzip(open(p, "rb").read()))
    return paths


def cli_runs(a):
    """bwa-amd mem -t 16 -K 20000000 on the .gz files: the input stage alone (BWAGPU_CLI_PARSE_ONLY=1), then FASTQ -> SAM with and without the switches"""
    import hashlib
    import re
    import subprocess
    import torch
    import bench
    fa, g, _ = bench.build_or_load_index(32.0, a.cache, 0, lambda: torch.cuda.synchronize())
    paths = inputs(a.cache, a.pairs)
    gz = [p + ".gz" for p in paths]
    cli = os.path.join(ROOT, "bwa_amd", "bwa-amd")
    base = ["mem", "-t", "16", "-K", "20000000", "-v", "3", fa]
    for rnd in range(3):
        p = subprocess.run([cli] + base + gz, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, env=dict(os.environ, BWAGPU_CLI_PARSE_ONLY="1"))
        print(f"[probe] input stage alone, host BGZF reader, round {rnd + 1}:", re.findall(r"parsed \d+ records.*", p.stderr), flush=True)

    def run(files, env):
        p = subprocess.run([cli] + base + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, BWAGPU_CLI_TRACE="1", **env))
        err = p.stderr.decode()
        sha = hashlib.sha256(b"\n".join(l for l in p.stdout.split(b"\n") if not l.startswith(b"@PG"))).hexdigest()[:16]
        m = re.search(r"(\d+) reads/s", err)
        busy = re.search(r"stage busy time: .*", err)
        dev = re.search(r"\[D::input\] \d+ batches.*", err)
        blocks = re.search(r"\[D::input\] \d+ BGZF blocks.*", err)
        return p.returncode, int(m.group(1)) if m else None, sha, busy.group(0) if busy else "", (dev.group(0) if dev else "") + " " + (blocks.group(0) if blocks else "")

    sets = [("defaults", {}), ("FASTQ=1 BGZF_DEV=1", {"BWAGPU_CLI_FASTQ": "1", "BWAGPU_CLI_BGZF_DEV": "1"}), ("SAMTEXT=1", {"BWAGPU_CLI_SAMTEXT": "1"}),
            ("SAMTEXT=1 FASTQ=1 BGZF_DEV=1", {"BWAGPU_CLI_SAMTEXT": "1", "BWAGPU_CLI_FASTQ": "1", "BWAGPU_CLI_BGZF_DEV": "1"})]
    print("[probe] plain files, defaults:", run(paths, {}), flush=True)
    for rnd in range(3):
        for name, env in sets:
            print(f"[probe] round {rnd + 1} .gz [{name}]:", run(gz, env), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--cli", action="store_true", help="the command-line runs on the .gz files instead of the library calls")
    ap.add_argument("--pairs", type=int, default=500_000)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--cache", default=os.environ.get("BWA_AMD_CACHE", "/tmp/bwa_amd_bench"))
    a = ap.parse_args()
    if a.resources:
        return resources()
    if a.cli:
        return cli_runs(a)
    import numpy as np
    from bwa_amd import api
    paths = inputs(a.cache, a.pairs)
    plain = [np.fromfile(p, dtype=np.uint8) for p in paths]
    comp = [np.fromfile(p + ".gz", dtype=np.uint8) for p in paths]
    P = api.FastqParser()
    P.reserve(max(len(x) for x in plain))
    med = lambda xs: statistics.median(xs[1:]) if len(xs) > 1 else xs[0]
    out = {"pairs": a.pairs, "plain_bytes": [len(x) for x in plain], "compressed_bytes": [len(x) for x in comp]}
    # the decoder alone (one file; wall includes the text's way down to the host)
    dst = np.zeros(len(plain[0]) + 16, dtype=np.uint8)
    info = api.BgzfInfo()
    wall, ms = [], []
    for _ in range(a.calls):
        t = time.perf_counter()
        rc = P.L.bwagpu_bgzf_inflate(P.h, comp[0].ctypes.data, len(comp[0]), 1, dst.ctypes.data, len(dst), C.byref(info))
        wall.append((time.perf_counter() - t) * 1e3)
        assert rc == 0 and info.damaged_at == -1 and info.inflated == len(plain[0]) and np.array_equal(dst[:len(plain[0])], plain[0])
        ms.append(info.inflate_ms)
    out["inflate_one_file"] = {"blocks": info.n_blocks, "inflate_ms": med(ms), "wall_ms": med(wall), "inflated_GBps": len(plain[0]) / med(ms) / 1e6}
    # the batch entries: everything in one call
    for nw in (2, 1):
        o, infos = api.FastqOut(), (api.BgzfInfo * 2)()
        w = [api.BgzfWin(c.ctypes.data, len(c), 0, 1) for c in comp]
        wall, ms, k0, k1, k2 = [], [], [], [], []
        for _ in range(a.calls):
            t = time.perf_counter()
            rc = P.L.bwagpu_fastq_batch_bgzf(P.h, C.byref(w[0]), C.byref(w[1]) if nw > 1 else None, 1 << 30, C.byref(o), infos)
            wall.append((time.perf_counter() - t) * 1e3)
            assert rc == 0 and o.status == api.FQ_END and o.n_reads == nw * a.pairs, (rc, o.status, o.n_reads)
            ms.append(infos[0].inflate_ms); k0.append(o.kernel_ms[0]); k1.append(o.kernel_ms[1]); k2.append(o.kernel_ms[2])
            P.L.bwagpu_fastq_out_free(C.byref(o))
        n_bytes = sum(len(x) for x in plain[:nw])
        out[f"batch_bgzf_{nw}"] = {"reads": nw * a.pairs, "wall_ms": med(wall), "inflate_ms": med(ms), "inflate_ms_per_Mreads": med(ms) / (nw * a.pairs / 1e6),
                                   "inflated_GBps": n_bytes / med(ms) / 1e6, "kernel_ms": [med(k0), med(k1), med(k2)]}
        wall = []
        for _ in range(a.calls):
            t = time.perf_counter()
            rc = P.L.bwagpu_fastq_batch(P.h, plain[0].ctypes.data, len(plain[0]), 1, plain[1].ctypes.data if nw > 1 else None, len(plain[1]) if nw > 1 else 0, 1, 1 << 30, C.byref(o))
            wall.append((time.perf_counter() - t) * 1e3)
            assert rc == 0 and o.status == api.FQ_END and o.n_reads == nw * a.pairs
            P.L.bwagpu_fastq_out_free(C.byref(o))
        out[f"batch_plain_{nw}"] = {"wall_ms": med(wall)}
    P.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
