#!/usr/bin/env python3
"""The BGZF writer on the device (bwa_amd/csrc/dev_bgzf_out.h), measured: profiles/dev_bgzf_out.md has the results.
  python tools/bgzf_out_probe.py --resources        registers, LDS and instruction count of the kernels (CPU only)
  python tools/bgzf_out_probe.py [--pairs N]        N pairs of 2 x 150 bp on the tests' small index: `bwa-amd mem` makes their SAM text once; then
      kernel:  bwagpu_bgzf_deflate on that text in one process, --calls calls, median of calls 2.. of the kernel's HIP-event time and of the
               call's wall time; zlib level 1 on the same blocks on --threads host threads (what `| bgzip -@16 -l1` would give)
      e2e:     `bwa-amd mem` FASTQ -> SAM with and without BWAGPU_CLI_BGZF_OUT=1, --rounds alternating runs, reads/s of each and the trace line
  One JSON line at the end."""
import argparse
import json
import os
import re
import statistics
import subprocess
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
        if "k_bo" in r[0]:
            print(dict(zip(("kernel", "vgpr", "agpr", "sgpr", "scratch", "lds", "spill", "wg", "instrs"), r)))


def zlib_blocks(text, threads, level=1, block=0xff00):
    def one(o):
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        t = text[o:o + block]
        return len(co.compress(t) + co.flush()) + 26

    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        total = sum(ex.map(one, range(0, len(text), block)))
    return total, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cache", default=os.environ.get("BWA_AMD_CACHE", "/tmp/bwa_amd_bench"))
    a = ap.parse_args()
    if a.resources:
        return resources()
    import testdata
    from bwa_amd import api, simdata
    os.makedirs(a.cache, exist_ok=True)
    prefix, g = testdata.small_index()
    r1, r2 = simdata.make_reads_pe(g, a.pairs, seed=79)
    files = [os.path.join(a.cache, f"bgzf_out_probe_{a.pairs}_{k}.fq") for k in (1, 2)]
    for p, r in zip(files, (r1, r2)):
        simdata.write_fastq(p, r)
    cli = os.path.join(ROOT, "bwa_amd", "bwa-amd")
    base = [cli, "mem", "-t", str(a.threads), "-v", "3", prefix] + files

    def run(env):
        p = subprocess.run(base, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, BWAGPU_CLI_TRACE="1", **env))
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        err = p.stderr.decode()
        m = re.search(r"(\d+) reads/s", err)
        o = re.search(r"\[D::output\] .*", err)
        w = re.search(r"write ([0-9.]+) s\n", err)
        return p.stdout, int(m.group(1)), o.group(0) if o else "", float(w.group(1)) if w else None

    nopg = lambda t: b"\n".join(l for l in t.split(b"\n") if not l.startswith(b"@PG"))
    sam, _, _, _ = run({})
    out = {"pairs": a.pairs, "sam_bytes": len(sam), "bytes_per_read": len(sam) / (2 * a.pairs)}
    # the kernel alone
    P = api.FastqParser()
    ms, wall = [], []
    for _ in range(a.calls):
        t = time.perf_counter()
        comp, info = P.deflate_bgzf(sam, 0, True)
        wall.append((time.perf_counter() - t) * 1e3)
        ms.append(info["deflate_ms"])
    P.close()
    import gzip
    assert gzip.decompress(comp) == sam
    med = lambda xs: statistics.median(xs[1:]) if len(xs) > 1 else xs[0]
    out["kernel"] = {"blocks": info["n_blocks"], "comp_bytes": len(comp), "ratio": len(comp) / len(sam), "deflate_ms": ms, "deflate_ms_median": med(ms), "kernel_GBps": len(sam) / med(ms) / 1e6,
                     "call_wall_ms": wall, "call_wall_ms_median": med(wall), "call_GBps": len(sam) / med(wall) / 1e6}
    z = [zlib_blocks(sam, a.threads) for _ in range(a.calls)]
    out["zlib_level1"] = {"threads": a.threads, "comp_bytes": z[0][0], "ratio": z[0][0] / len(sam), "seconds": [s for _, s in z], "GBps": len(sam) / med([s for _, s in z]) / 1e9}
    # FASTQ -> SAM with and without the switch, alternating
    rates = {"off": [], "on": []}
    for _ in range(a.rounds):
        for name, env in (("off", {}), ("on", {"BWAGPU_CLI_BGZF_OUT": "1"})):
            text, rate, line, w = run(env)
            rates[name].append(rate)
            if name == "on":
                assert nopg(gzip.decompress(text)) == nopg(sam)
                out["trace"] = line
            out.setdefault("write_busy_s", {}).setdefault(name, []).append(w)
    out["e2e_reads_per_s"] = {k: {"runs": v, "median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in rates.items()}
    out["needed_GBps"] = out["e2e_reads_per_s"]["off"]["median"] * out["bytes_per_read"] / 1e9
    print(json.dumps(out))


if __name__ == "__main__":
    main()
