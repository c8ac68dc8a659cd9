"""Pairing of the two ends on the device (bwagpu_batch_pair, bwagpu_pair_flat; bwa_amd/csrc/dev_pair.h) against the compiled reference's own mem_pair
(bwamem_pair.c:208-269), mem_mark_primary_se and mem_pestat, which oracle/_ref/libbwaref.so exports: called through ctypes on arrays of the reference's
mem_alnreg_t, with bns from refshim_idx_bns of the loaded index, pac NULL and s a zeroed buffer (mem_pair reads neither).  score, sub, n_sub and z must
be equal, exactly; where the reference has no candidate it leaves z untouched, and our side has -1.  mem_pair does not return u.n: n_cand is held to a
direct count of the definition (hit pairs of the two ends on one contig whose distance lies in the window of their orientation) on the same lists.

1. a fuzz of bwagpu_pair_flat over numbers of hits around every switch point of the kernels (bwagpu_pair_limits), families of lists, windows and options;
2. real batches: run -> download -> pair(opt, pes, id0) with pes from the reference's mem_pestat;
3. `bwa-amd mem` with BWAGPU_CLI_PAIR=1 against `bwa mem`;
4. error paths.
CPU: on the mock runtime (tests/hostsim), thinned.  -m gpu: everything, three seeds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import refapi
import testdata
import test_primary as tp
from bwa_amd import simdata
from bwa_amd.api import BwaGpu
from bwa_amd.structs import ALNREG_DTYPE, PAIR_DTYPE, PESTAT_DTYPE, MemPestat

pytestmark = pytest.mark.skipif(not refapi.have_ref(), reason="oracle/_ref not built")

# where the kernels change their form (dev_pair.h); the cases are aimed at these, so they are checked against the library under test
LANE_MAX, LDS_SMALL, LDS_BIG = 4, 128, 1024
SIZES = ((0, 3), (3, 0), (0, 0), (1, 1), (1, 2), (2, 2), (1, 3), (2, 3), (4, 1), (63, 64), (1, 127), (64, 64), (100, 29), (500, 523), (1, 1023), (512, 512),
         (1000, 25), (1050, 1050))
FAMILIES = ("proper", "cluster", "none", "edge", "equal", "strands")
PES_VARIANTS = ("one", "four", "failed", "wide")
FIELDS = ("score", "sub", "n_sub", "n_cand")


def form_of(n0, n1):
    s = n0 + n1
    return 0 if s <= LANE_MAX else 1 if s <= LDS_SMALL else 2 if s <= LDS_BIG else 3


def check_limits(dev):
    assert dev.pair_limits() == dict(lane_max=LANE_MAX, lds_small=LDS_SMALL, lds_big=LDS_BIG), "a switch point of the library moved: aim the cases at it"
    sums = {a + b for a, b in SIZES}
    for n in (LANE_MAX, LDS_SMALL, LDS_BIG):
        assert {n - 1, n, n + 1} <= sums, n
    assert max(sums) > 2 * LDS_BIG and (1, 1) in SIZES and any(a == 0 and b > 0 for a, b in SIZES)


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------------------
class AlnV(C.Structure):      # mem_alnreg_v (bwamem.h:106)
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("a", C.c_void_p)]


class Ref:
    """The reference's index (for bns) and its mem_pair / mem_pestat."""
    def __init__(self, prefix):
        self.idx = refapi.RefIndex(prefix)
        L = self.L = refapi.lib()
        sz = (C.c_int32 * 16)()
        L.refshim_sizes(sz)
        assert sz[6] == PESTAT_DTYPE.itemsize == C.sizeof(MemPestat) == 32 and sz[1] == ALNREG_DTYPE.itemsize
        self.bns = L.refshim_idx_bns(self.idx.h)
        L.mem_pair.restype = C.c_int
        L.mem_pair.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mem_pestat.restype = None
        L.mem_pestat.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
        self.s = C.create_string_buffer(512)

    def close(self):
        self.idx.close()

    def pestat(self, opt, counts, regs):
        regs = np.ascontiguousarray(regs, dtype=ALNREG_DTYPE)
        v = (AlnV * max(1, len(counts)))()
        lo = 0
        for i, c in enumerate(counts):
            v[i].n = v[i].m = int(c); v[i].a = regs.ctypes.data + lo * ALNREG_DTYPE.itemsize
            lo += int(c)
        pes = np.zeros(4, dtype=PESTAT_DTYPE)
        self.L.mem_pestat(C.byref(opt), self.idx.l_pac, len(counts), v, pes.ctypes.data)
        return pes

    def pair(self, opt, pes, a0, a1, n_pri, pid):
        """mem_pair of one pair: marked lists a0, a1 (ALNREG_DTYPE), n_pri = (n0, n1), the id as the `int` the reference takes -> (ret, sub, n_sub, z0, z1)"""
        v = (AlnV * 2)()
        keep = [np.ascontiguousarray(a0), np.ascontiguousarray(a1)]
        for r in range(2):
            v[r].n = v[r].m = keep[r].shape[0]; v[r].a = keep[r].ctypes.data
        sub, n_sub = C.c_int(-77), C.c_int(-77)
        z = (C.c_int * 2)(-7, -7)
        np_ = (C.c_int * 2)(int(n_pri[0]), int(n_pri[1]))
        pid = ((int(pid) + (1 << 31)) % (1 << 32)) - (1 << 31)
        ret = self.L.mem_pair(C.byref(opt), self.bns, None, pes.ctypes.data, self.s, v, pid, C.byref(sub), C.byref(n_sub), z, np_)
        return ret, sub.value, n_sub.value, z[0], z[1]


def count_candidates(pes, l_pac, ctg_off, a0, a1, n0, n1):
    """u.n by its definition: pairs (hit of end 0, hit of end 1) with the same rid whose distance lies in [low, high] of the orientation
    (strand of the hit at the lower position) << 1 | (strand of the other), that orientation not failed.  Windows have low >= 1, so equal positions never count."""
    if n0 == 0 or n1 == 0:
        return 0
    def key(a, n):
        rb = a["rb"][:n].astype(np.int64)
        st = (rb >= l_pac).astype(np.int64)
        fwd = np.where(st == 1, 2 * l_pac - 1 - rb, rb) - ctg_off[a["rid"][:n]]
        return a["rid"][:n].astype(np.int64), fwd, st
    r0, x0, s0 = key(a0, n0)
    r1, x1, s1 = key(a1, n1)
    d = x1[None, :] - x0[:, None]
    same = r0[:, None] == r1[None, :]
    dirs = np.where(d > 0, s0[:, None] * 2 + s1[None, :], s1[None, :] * 2 + s0[:, None])
    dist = np.abs(d)
    ok = same & (d != 0) & (pes["failed"][dirs] == 0) & (dist >= pes["low"][dirs]) & (dist <= pes["high"][dirs])
    return int(ok.sum())


def ref_pairs(ref, opt, pes, ctg_off, counts, n_pri, regs, ids):
    """-> PAIR_DTYPE records of the pairs (reads 2p, 2p + 1 of counts / regs, already in marked order)"""
    assert (pes["low"][pes["failed"] == 0] >= 1).all()
    out = np.zeros(len(ids), dtype=PAIR_DTYPE)
    ends = np.concatenate([[0], np.cumsum(counts)])
    for p in range(len(ids)):
        a0, a1 = regs[ends[2 * p]:ends[2 * p + 1]], regs[ends[2 * p + 1]:ends[2 * p + 2]]
        n0, n1 = int(n_pri[2 * p]), int(n_pri[2 * p + 1])
        nc = count_candidates(pes, ref.idx.l_pac, ctg_off, a0, a1, n0, n1)
        ret, sub, n_sub, z0, z1 = ref.pair(opt, pes, a0, a1, (n0, n1), ids[p]) if n0 and n1 else (0, 0, 0, -7, -7)      # (mem_sam_pe does not call mem_pair otherwise)
        assert (nc == 0) == (z0 == -7) == (z1 == -7), (p, nc, z0, z1)      # the reference leaves z untouched exactly when u is empty
        out[p] = (ret, sub, n_sub, (z0, z1) if nc else (-1, -1), 0, nc)
    return out


def assert_pairs_equal(got, want, what, flags_zero=True):
    assert got.shape == want.shape, what
    bad = np.zeros(got.shape[0], dtype=bool)
    for f in FIELDS:
        bad |= got[f] != want[f]
    bad |= (got["z"] != want["z"]).any(axis=1)
    if bad.any():
        k = int(np.nonzero(bad)[0][0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.shape[0]} records differ; first: pair {k}\n device    {got[k]}\n reference {want[k]}")
    assert not (got["flags"] & ~1).any()
    if flags_zero:
        assert not (got["flags"] & 1).any(), f"{what}: {int((got['flags'] & 1).sum())} pairs were left to the host's erfc / log"


# ---- generated lists --------------------------------------------------------------------------------------------------------------------------------------
def make_pes(variant):
    pes = np.zeros(4, dtype=PESTAT_DTYPE)
    pes["failed"] = 1; pes["low"] = 1; pes["high"] = 1; pes["std"] = 1.0
    live = {"one": {1: (200, 600, 400.0, 50.0)},
            "four": {0: (1, 300, 150.5, 61.0), 1: (200, 600, 403.7, 48.2), 2: (100, 1500, 800.0, 333.3), 3: (50, 250, 149.0, 20.0)},
            "failed": {},
            "wide": {0: (30, 90, 60.0, 10.0), 1: (1, 9001, 4500.0, 1500.0)}}[variant]
    for d, (lo, hi, avg, std) in live.items():
        pes[d] = (lo, hi, 0, avg, std)
    return pes


def make_pair(rng, meta, pes, n0, n1, family, extra):
    """Two marked lists with n0 / n1 primary-assembly hits (+ `extra` records behind them that take no part), every hit inside a contig of the index."""
    l_pac, off, ln = int(meta["l_pac"]), meta["ctg_offset"], meta["ctg_len"]
    nctg = len(ln)
    live = [d for d in range(4) if not pes["failed"][d]]
    d = live[int(rng.integers(len(live)))] if live else 1
    lo, hi = int(pes["low"][d]), int(pes["high"][d])
    n = (n0, n1)
    rid = [np.zeros(k, dtype=np.int64) for k in n]; pos = [np.zeros(k, dtype=np.int64) for k in n]; st = [rng.integers(0, 2, k) for k in n]
    score = [rng.integers(30, 151, k) for k in n]
    c = int(rng.integers(nctg)); L = int(ln[c])
    room = L - hi - 400
    assert room > 100
    base = int(rng.integers(50, room))
    if family in ("proper", "edge"):      # scattered hits, then the first of each end put at a chosen distance and orientation
        for e in range(2):
            rid[e][:] = rng.integers(0, nctg, n[e]); pos[e][:] = (rng.random(n[e]) * (ln[rid[e]] - 1)).astype(np.int64)
        if n0 and n1:
            dist = int(rng.integers(lo, hi + 1)) if family == "proper" else (lo - 1, lo, hi, hi + 1)[int(rng.integers(4))]
            first = int(rng.integers(2))      # which end is at the lower position
            rid[first][0] = rid[1 - first][0] = c; pos[first][0] = base; pos[1 - first][0] = base + dist
            st[first][0] = d >> 1; st[1 - first][0] = d & 1
            if family == "edge":      # ... and the other three edge distances too, while there is room
                for j, dd in enumerate((lo - 1, lo, hi, hi + 1)):
                    if j + 1 < n[1 - first]:
                        rid[1 - first][j + 1] = c; pos[1 - first][j + 1] = base + dd; st[1 - first][j + 1] = d & 1
    elif family == "cluster":      # many hits close together, few distinct scores: equal q, the hash decides
        span = max(8, min(room - base + hi, 6 * hi if n0 + n1 > 300 else hi))
        for e in range(2):
            rid[e][:] = c; pos[e][:] = base + rng.integers(0, span, n[e]); score[e] = rng.choice([50, 50, 60], n[e])
            st[e][:] = (d >> 1, d & 1)[e] if rng.random() < 0.5 else rng.integers(0, 2, n[e])
    elif family == "none":
        if nctg > 1 and rng.random() < 0.5:      # adjacent positions on different contigs
            c = int(rng.integers(nctg - 1))
            rid[0][:] = c; pos[0][:] = int(ln[c]) - 1 - rng.integers(0, 3, n0)
            rid[1][:] = c + 1; pos[1][:] = rng.integers(0, 3, n1)
        else:      # far apart
            rid[0][:] = c; pos[0][:] = rng.integers(0, 40, n0)
            rid[1][:] = c; pos[1][:] = L - 1 - rng.integers(0, 40, n1)
            assert L - 80 > int(pes["high"].max())
    elif family == "equal":
        for e in range(2):
            rid[e][:] = c; pos[e][:] = base
    else:      # strands: both strands for both ends within reach of each other
        for e in range(2):
            rid[e][:] = c; pos[e][:] = base + rng.integers(0, hi + 50, n[e])
    lists = []
    for e in range(2):
        a = np.zeros(n[e] + extra[e], dtype=ALNREG_DTYPE)
        k = n[e]
        f = off[rid[e]] + pos[e]
        assert k == 0 or (pos[e].min() >= 0 and (pos[e] < ln[rid[e]]).all())
        a["rid"][:k] = rid[e]; a["rb"][:k] = np.where(st[e] == 1, 2 * l_pac - 1 - f, f); a["score"][:k] = score[e]
        a["re"][:k] = a["rb"][:k] + 100; a["qe"][:k] = 100
        if extra[e]:      # what lies behind n_pri is ignored: hits that would pair with everything, and a rid no index has
            a["rid"][k:] = 1 << 20; a["rb"][k:] = off[c] + base + 1; a["score"][k:] = 1000
        lists.append(a)
    return lists


def opt_variants():
    out = []
    for name, kw in (("default", {}), ("a2b3", dict(a=2, b=3)), ("gaps", dict(o_del=20, e_del=3, o_ins=2, e_ins=1))):
        o = tp.ref_opt()
        for k, v in kw.items():
            setattr(o, k, v)
        out.append((name, o))
    return out


def fuzz_cells(thin, call):
    """(n0, n1, family, pes variant): the full cross product, or (thin) every family for the sizes one lane does and one per call for the others, dealt so that
    every form sees every family over the three calls."""
    cells, seen = [], {}
    for n0, n1 in SIZES:
        form = form_of(n0, n1)
        if not thin:
            cells += [(n0, n1, f, v) for f in FAMILIES for v in PES_VARIANTS]
            continue
        k = seen.get(form, 0); seen[form] = k + 1
        per = sum(1 for a, b in SIZES if form_of(a, b) == form)
        fams = FAMILIES if form == 0 else (FAMILIES[(call * per + k) % len(FAMILIES)],)
        for j, f in enumerate(fams):
            cells.append((n0, n1, f, PES_VARIANTS[(call + k + j) % len(PES_VARIANTS)]))
    return cells


def build_call(rng, meta, cells):
    by_pes = {}
    for cell in cells:
        by_pes.setdefault(cell[3], []).append(cell)
    for v, group in by_pes.items():
        pes = make_pes(v)
        lists, counts, n_pri = [], [], []
        for j, (n0, n1, f, _) in enumerate(group):
            extra = (int(rng.integers(0, 4)), int(rng.integers(0, 4))) if j % 3 == 1 else (0, 0)
            a0, a1 = make_pair(rng, meta, pes, n0, n1, f, extra)
            lists += [a0, a1]; counts += [a0.shape[0], a1.shape[0]]; n_pri += [n0, n1]
        ids = rng.integers(0, 1 << 20, len(group)).astype(np.int64)
        ids[::3] += 1 << 23      # id << 8 overflows 32 bits
        ids[1::5] = (1 << 31) - 1 - np.arange(len(ids[1::5]))
        ids[2::7] += 1 << 35     # beyond int: truncated as the reference's `int id`
        yield v, pes, group, np.array(counts, dtype=np.int32), np.array(n_pri, dtype=np.int32), np.concatenate(lists), ids


def run_fuzz(dev, ref, seed, thin):
    check_limits(dev)
    rng = np.random.default_rng(seed)
    meta = dev.index_meta()
    seen, ncand = {}, set()
    any_extra = False
    for vi, (name, opt) in enumerate(opt_variants()):
        for v, pes, group, counts, n_pri, regs, ids in build_call(rng, meta, fuzz_cells(thin, vi)):
            want = ref_pairs(ref, opt, pes, meta["ctg_offset"], counts, n_pri, regs, ids)
            got, ms = dev.pair_flat(opt, pes, counts, n_pri, regs, ids)
            assert ms >= 0
            assert_pairs_equal(got, want, f"fuzz seed {seed}, options {name}, windows {v}")
            any_extra |= bool((counts > n_pri).any())
            for (n0, n1, f, _), w in zip(group, want):
                seen.setdefault(form_of(n0, n1), set()).add(f)
                ncand.add("0" if w["n_cand"] == 0 else "1" if w["n_cand"] == 1 else ">64" if w["n_cand"] > 64 else "few")
    for form in range(4):
        assert seen[form] == set(FAMILIES), (form, seen[form])
    assert {"0", "1", ">64"} <= ncand and any_extra
    run_mixed(dev, ref, seed)


def run_mixed(dev, ref, seed):
    """128 consecutive pairs whose sizes run through every form of the kernels (and the pairs with an empty end) within each wavefront, a cycle of seven, so the
    places shift from one wavefront to the next: the lanes' hand-over with all three lists live in one ballot and no list taking a whole wavefront."""
    rng = np.random.default_rng(seed + 1000)
    meta = dev.index_meta()
    opt = tp.ref_opt()
    cyc = ((2, 2), (3, 2), (0, 3), (LDS_SMALL // 2, LDS_SMALL // 2 + 1), (1, 1), (LDS_BIG // 2, LDS_BIG // 2 + 1), (LDS_SMALL // 2, LDS_SMALL // 2))
    assert {form_of(a, b) for a, b in cyc} == {0, 1, 2, 3}
    cells = [cyc[i % len(cyc)] + (FAMILIES[i % len(FAMILIES)], "four") for i in range(128)]
    (v, pes, group, counts, n_pri, regs, ids), = build_call(rng, meta, cells)
    want = ref_pairs(ref, opt, pes, meta["ctg_offset"], counts, n_pri, regs, ids)
    got, _ = dev.pair_flat(opt, pes, counts, n_pri, regs, ids)
    assert_pairs_equal(got, want, f"128 pairs of mixed forms, seed {seed}")


def run_tab_cap(dev, ref, seed):
    """A table of two entries: nearly every pair with a candidate meets a distance outside it, is flagged and comes from the host side of the call -- the same record."""
    rng = np.random.default_rng(seed)
    meta = dev.index_meta()
    opt = tp.ref_opt()
    cells = [(n0, n1, f, "four") for n0, n1 in SIZES if n0 + n1 <= 2 * LDS_SMALL for f in ("proper", "cluster", "edge")]
    (v, pes, group, counts, n_pri, regs, ids), = build_call(rng, meta, cells)
    want = ref_pairs(ref, opt, pes, meta["ctg_offset"], counts, n_pri, regs, ids)
    dev.set_option("pair_tab_cap", 2)
    try:
        got, _ = dev.pair_flat(opt, pes, counts, n_pri, regs, ids)
        assert_pairs_equal(got, want, "table of two entries", flags_zero=False)
        assert int((got["flags"] & 1).sum()) > len(ids) // 4, "too few pairs were flagged"
    finally:
        dev.set_option("pair_tab_cap", 0)
    got, _ = dev.pair_flat(opt, pes, counts, n_pri, regs, ids)
    assert_pairs_equal(got, want, "table grown again")


# ---- real batches -----------------------------------------------------------------------------------------------------------------------------------------
def pe_reads(g, n_pairs, n_foreign, seed):
    """n_pairs ordinary pairs and n_foreign whose second end is drawn from elsewhere, every fifth place while they last; mates interleaved"""
    a, b = simdata.make_reads_pe(g, n_pairs + n_foreign, seed=seed)
    other = simdata.make_reads_se(g, n_foreign, seed=seed + 1)
    order, fo, k = [], 0, 0
    while k < n_pairs or fo < n_foreign:
        if fo < n_foreign and (len(order) % 5 == 4 or k >= n_pairs):
            b[n_pairs + fo] = other[fo]; order.append(n_pairs + fo); fo += 1
        else:
            order.append(k); k += 1
    a, b = a[order], b[order]
    return np.stack([a, b], axis=1).reshape(-1, a.shape[1]), a, b


def run_batches(dev, ref, g, n_pairs, n_foreign, seed, id0s):
    opt = tp.ref_opt()
    reads, _, _ = pe_reads(g, n_pairs, n_foreign, seed)
    dev.upload(*testdata.flat(reads)); dev.run(opt)
    counts, regs = dev.download()
    pes = ref.pestat(opt, counts, regs)
    assert not pes["failed"].all(), "mem_pestat found no orientation: the batch is too small"
    meta = dev.index_meta()
    ends = np.concatenate([[0], np.cumsum(counts)])
    for id0 in id0s:
        ids = id0 + np.arange(counts.shape[0], dtype=np.int64)
        wpri, wnp = tp.ref_primary(opt, counts, regs, ids)      # mem_mark_primary_se(id0 + 2p | r) of each end
        marked = regs.copy()
        for i in range(counts.shape[0]):
            lo, hi = int(ends[i]), int(ends[i + 1])
            marked[lo:hi] = regs[lo:hi][wpri["src"][lo:hi]]
        want = ref_pairs(ref, opt, pes, meta["ctg_offset"], counts, wnp, marked, (id0 >> 1) + np.arange(counts.shape[0] // 2, dtype=np.int64))
        got, pri, n_pri, ms = dev.pair(opt, pes, id0)
        assert ms >= 0
        assert_pairs_equal(got, want, f"batch of {counts.shape[0] // 2} pairs, id0 {id0}")
        tp.assert_records_equal(pri, n_pri, wpri, wnp, counts, f"marking records of the pair call, id0 {id0}")
        pri2, n_pri2, _ = dev.primary(opt, id0)
        assert np.array_equal(pri, pri2) and np.array_equal(n_pri, n_pri2)
    assert (want["n_cand"] > 0).any() and (want["n_cand"] == 0).any() and (want["score"] > 0).any()
    return want


# ---- the command line -------------------------------------------------------------------------------------------------------------------------------------
def run_cli(cli, prefix, f1, f2, K, env, n_pairs):
    """paired-end SAM of `cli` with and without BWAGPU_CLI_PAIR against `bwa mem`; returns the share of pairs taken from the device's records"""
    body = lambda t: b"\n".join(l for l in t.split(b"\n") if not l.startswith(b"@PG"))
    args = ["mem", "-K", str(K), "-t", "2"]
    p = subprocess.run([refapi.REF_BWA] + args + [prefix, f1, f2], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-1000:]
    want = body(p.stdout)
    assert want.count(b"\n") >= 2 * n_pairs
    outs = {}
    for on in (True, False):
        e = dict(env, BWAGPU_CLI_TRACE="1")
        e.pop("BWAGPU_CLI_PAIR", None)
        if on:
            e["BWAGPU_CLI_PAIR"] = "1"
        p = subprocess.run([cli] + args + [prefix, f1, f2], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        outs[on] = (body(p.stdout), p.stderr.decode())
    assert outs[True][0] == want, "BWAGPU_CLI_PAIR=1: SAM differs from bwa mem"
    assert outs[False][0] == want, "switch unset: SAM differs from bwa mem"
    line = [l for l in outs[True][1].split("\n") if "pairs paired from device records (BWAGPU_CLI_PAIR)" in l]
    assert len(line) == 1, outs[True][1][-1500:]
    n = int(line[0].split("]")[1].split()[0])
    assert 0 < n < n_pairs, (n, n_pairs)
    assert "pairs paired from device records" not in outs[False][1]
    print(f"BWAGPU_CLI_PAIR: {n} of {n_pairs} pairs paired from device records ({n / n_pairs:.3f})")
    return n / n_pairs


def cli_inputs(tmp_path, g, n_pairs, n_foreign, seed):
    _, a, b = pe_reads(g, n_pairs, n_foreign, seed)
    f1, f2 = str(tmp_path / "p_1.fq"), str(tmp_path / "p_2.fq")
    simdata.write_fastq(f1, a); simdata.write_fastq(f2, b)
    return f1, f2


# ---- mock runtime -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim():
    import hostsim_build
    prefix, _ = testdata.small_index()
    s = BwaGpu(prefix, lib_path=hostsim_build.build(), options={"ptab_m": 6})
    yield s
    s.close()


@pytest.fixture(scope="module")
def ref_small():
    r = Ref(testdata.small_index()[0])
    yield r
    r.close()


def test_structs_and_limits(sim):
    assert PAIR_DTYPE.itemsize == 32 and PESTAT_DTYPE.itemsize == 32 and PAIR_DTYPE.fields["n_cand"][1] == 24 and PESTAT_DTYPE.fields["avg"][1] == 16
    sz = (C.c_int32 * 16)()
    refapi.lib().refshim_sizes(sz)
    assert sz[6] == PESTAT_DTYPE.itemsize
    check_limits(sim)


def test_sim_pair_flat_fuzz(sim, ref_small):
    run_fuzz(sim, ref_small, 31, thin=True)


def test_sim_pair_tab_cap(sim, ref_small):
    run_tab_cap(sim, ref_small, 32)


def test_sim_pair_on_batches(sim, ref_small):
    run_batches(sim, ref_small, testdata.small_index()[1], 28, 8, 701, (0, (1 << 35) + 7770))


def test_sim_cli_pair(tmp_path):
    import test_cli
    prefix, g = testdata.small_index()
    alt = tp.alt_prefix(tmp_path, prefix, ["chr3"])
    f1, f2 = cli_inputs(tmp_path, g, 32, 8, 711)
    env = dict(os.environ, BWAGPU_CLI_STREAMS="2", BWAGPU_CLI_SERIALIZE="1", BWAGPU_PTAB_M="6")
    run_cli(test_cli._sim_cli(), alt, f1, f2, 6000, env, 40)      # (twenty pairs per batch: id0 > 0 in the second)


def test_error_paths(sim, ref_small):
    opt = tp.ref_opt()
    L, h = sim.L, sim.h
    pes = make_pes("one")
    P = pes.ctypes.data
    pp, n, pr, nr, ms = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_int64(), C.c_float()
    g = testdata.small_genome()[0]
    reads, _, _ = pe_reads(g, 3, 0, 5)
    sim.upload(*testdata.flat(reads))
    call = lambda *a: L.bwagpu_batch_pair(*a)
    ok = lambda: (h, C.byref(opt), P, 0, C.byref(pp), C.byref(n), None, None, None, None)
    assert call(*ok()) == -2, "before a run"
    sim.run(opt)
    assert call(*ok()) == -2, "before a download"
    counts, regs = sim.download()
    for k in (0, 1, 2, 4, 5):      # NULL h, opt, pes, pairs, n_pairs
        a = list(ok()); a[k] = None
        assert call(*a) == -2, k
    a = list(ok()); a[3] = 7
    assert call(*a) == -2, "odd id0"
    o5 = tp.ref_opt(); o5.flag |= 0x800
    a = list(ok()); a[1] = C.byref(o5)
    assert call(*a) == -2, "MEM_F_PRIMARY5"
    assert call(*ok()) == 0 and n.value == 3      # pri, n_pri_recs, n_pri and kernel_ms may be NULL
    L.bwagpu_free(pp)
    assert L.bwagpu_batch_pair(h, C.byref(opt), P, 0, C.byref(pp), C.byref(n), C.byref(pr), C.byref(nr), None, C.byref(ms)) == 0 and nr.value == int(counts.sum())
    L.bwagpu_free(pp); L.bwagpu_free(pr)
    # an odd number of reads
    sim.upload(*testdata.flat(reads[:3])); sim.run(opt); sim.download()
    assert call(*ok()) == -2, "odd number of reads"
    # zero pairs
    sim.upload(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64)); sim.run(opt); sim.download()
    got, pri, n_pri, _ = sim.pair(opt, pes, 0)
    assert got.shape[0] == 0 and pri.shape[0] == 0 and n_pri.shape[0] == 0
    # pairs with no hit on one or both ends: the no-candidate record
    junk = np.tile(np.array([0, 1, 2, 3], dtype=np.uint8), 5)
    mixed = [reads[0], junk, junk, reads[1], junk, junk]
    sim.upload(*testdata.ragged(mixed)); sim.run(opt)
    counts, regs = sim.download()
    got, pri, n_pri, _ = sim.pair(opt, pes, 4)
    assert counts[0] > 0 and n_pri.tolist()[1:3] == [0, 0] and n_pri.tolist()[4:] == [0, 0]
    for r in got:
        assert (r["score"], r["sub"], r["n_sub"], r["n_cand"], r["flags"]) == (0, 0, 0, 0, 0) and r["z"].tolist() == [-1, -1]
    # bwagpu_pair_flat: NULL arguments, counts and n_pri out of range, a rid outside the index, no pairs
    rng = np.random.default_rng(2)
    meta = sim.index_meta()
    a0, a1 = make_pair(rng, meta, pes, 2, 1, "proper", (0, 0))
    regs2 = np.concatenate([a0, a1]); c2 = np.array([2, 1], dtype=np.int32); ids2 = np.array([9], dtype=np.int64)
    flat = lambda *a: L.bwagpu_pair_flat(*a)
    okf = lambda: [h, C.byref(opt), P, 1, c2.ctypes.data, c2.ctypes.data, regs2.ctypes.data, ids2.ctypes.data, C.byref(pp), None]
    for k in (0, 1, 2, 4, 5, 6, 7, 8):
        a = okf(); a[k] = None
        assert flat(*a) == -2, k
    a = okf(); a[3] = -1
    assert flat(*a) == -2
    for bad in ([-1, 1], [3, 1]):      # n_pri outside [0, counts]
        b = np.array(bad, dtype=np.int32)
        a = okf(); a[5] = b.ctypes.data
        assert flat(*a) == -2, bad
    b = np.array([-2, 1], dtype=np.int32)
    a = okf(); a[4] = b.ctypes.data
    assert flat(*a) == -2
    r3 = regs2.copy(); r3["rid"][0] = int(meta["n_seqs"])
    a = okf(); a[6] = r3.ctypes.data
    assert flat(*a) == -2, "rid outside the index"
    assert flat(*okf()) == 0      # kernel_ms may be NULL
    L.bwagpu_free(pp)
    assert flat(h, C.byref(opt), P, 0, None, None, None, None, C.byref(pp), None) == 0
    L.bwagpu_free(pp)
    z = np.zeros(4, dtype=np.int32)
    got, _ = sim.pair_flat(opt, pes, z, z, np.zeros(0, dtype=ALNREG_DTYPE), np.arange(2))
    assert got.shape[0] == 2 and (got["n_cand"] == 0).all() and (got["z"] == -1).all()


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    g = BwaGpu(testdata.small_index()[0])
    yield g
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [41, 42, 43])
def test_gpu_pair_flat_fuzz(gpu, ref_small, seed):
    run_fuzz(gpu, ref_small, seed, thin=False)


@pytest.mark.gpu
def test_gpu_pair_tab_cap(gpu, ref_small):
    run_tab_cap(gpu, ref_small, 44)


@pytest.mark.gpu
def test_gpu_pair_on_batches():
    fa, g = testdata.medium_index()
    dev, ref = BwaGpu(fa), Ref(fa)
    try:
        want = run_batches(dev, ref, g, 6000, 1000, 801, (0, (1 << 35) + 7770))
        assert int((want["n_cand"] > 1).sum()) > 0
    finally:
        dev.close(); ref.close()


@pytest.mark.gpu
def test_gpu_cli_pair(tmp_path):
    from bwa_amd import build as b
    _, cli = b.build_host(verbose=False)
    fa, g = testdata.medium_index()
    alt = tp.alt_prefix(tmp_path, fa, ["chr3"])
    f1, f2 = cli_inputs(tmp_path, g, 3200, 800, 811)
    run_cli(cli, alt, f1, f2, 300000, dict(os.environ), 4000)      # (a thousand pairs per batch)
