#!/usr/bin/env python3
"""`bwa-amd index` on a GRCh38-sized synthetic FASTA: make_genome_large (3.1 Gbp by default) written by
simdata.write_fasta_ambiguous -- ~5 % N in runs of 10 bp to 100 kbp and at every contig's ends, scattered IUPAC codes,
soft-masked lower-case stretches, 60-column lines -- then indexed from the page cache (the file is read once before the
timed run).  Prints the command line's stage times (-v 3) and one JSON line.

    python tools/fasta_index_bench.py [--mbp 3100] [--dir /tmp/bwa_amd_fasta_bench] [--keep]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbp", type=int, default=3100)
    ap.add_argument("--dir", default="/tmp/bwa_amd_fasta_bench")
    ap.add_argument("--keep", action="store_true", help="keep the FASTA and the index files")
    a = ap.parse_args()
    from bwa_amd import build, simdata
    _, cli = build.build_host(verbose=False)
    os.makedirs(a.dir, exist_ok=True)
    fa = os.path.join(a.dir, f"synth{a.mbp}.fa")
    t = time.time()
    g, lens = simdata.make_genome_large(a.mbp * 1_000_000, seed=31)
    n_amb = simdata.write_fasta_ambiguous(fa, g, lens, seed=31)
    del g
    t_gen = time.time() - t
    with open(fa, "rb") as f:                          # into the page cache
        while f.read(1 << 26):
            pass
    prefix = os.path.join(a.dir, "idx")
    t = time.time()
    p = subprocess.run([cli, "index", "-v", "3", "-p", prefix, fa], capture_output=True, text=True)
    wall = time.time() - t
    sys.stderr.write(p.stderr)
    if p.returncode != 0:
        sys.exit(p.returncode)
    num = lambda pat: float(re.search(pat, p.stderr).group(1))
    out = {"metric": "bwa-amd index wall seconds", "genome_mbp": a.mbp, "fasta_bytes": os.path.getsize(fa), "ambiguous_bases": n_amb,
           "wall_s": round(wall, 2), "read_wait_s": num(r"read \+ inflate \(waits\) ([\d.]+)"), "parse_s": num(r"FASTA parse ([\d.]+) sec"),
           "parse_kernels_ms": num(r"kernels ([\d.]+) ms"), "sort_s": num(r"suffix sort \+ BWT \+ SA ([\d.]+)"),
           "sort_device_ms": num(r"device ([\d.]+) ms"), "write_s": num(r"file writes ([\d.]+)"), "generate_s": round(t_gen, 1),
           "holes": int(re.search(r"(\d+) holes", p.stderr).group(1))}
    print(json.dumps(out))
    if not a.keep:
        for e in ("", ".pac", ".ann", ".amb", ".bwt", ".sa"):
            path = (fa if e == "" else prefix + e)
            if os.path.exists(path):
                os.remove(path)


if __name__ == "__main__":
    main()
