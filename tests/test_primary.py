"""Primary/secondary marking and mapQ on the device (bwagpu_batch_primary, bwagpu_primary_flat; bwa_amd/csrc/dev_primary.h) against the compiled
reference's own mem_mark_primary_se (bwamem.c:547-584) and mem_approx_mapq_se (bwamem.c:982-1006), which oracle/_ref/libbwaref.so exports: both are
called through ctypes on arrays of the reference's mem_alnreg_t with a mem_opt_t that starts from mem_opt_init (refshim_opt_init).  Every field of every
record and every return value must be equal, exactly.

1. a fuzz of bwagpu_primary_flat over region counts around every switch point of the kernels (bwagpu_primary_limits) and families of region lists;
2. real batches against an index with an ALT contig: run -> download -> primary(opt, id0);
3. `bwa-amd mem` with BWAGPU_CLI_PRIMARY=1 against `bwa mem`;
4. error paths.
CPU: on the mock runtime (tests/hostsim), thinned -- a wavefront's step is 64 fiber switches there.  -m gpu: everything, several seeds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import refapi
import testdata
from bwa_amd import simdata
from bwa_amd.api import BwaGpu
from bwa_amd.structs import ALNREG_DTYPE, PRIMARY_DTYPE, MemOpt

pytestmark = pytest.mark.skipif(not refapi.have_ref(), reason="oracle/_ref not built")

# where the kernels change their form (dev_primary.h); the cases are aimed at these, so they are checked against the library under test
LANE_MAX, LDS_SMALL, LDS_BIG, SCAN = 4, 128, 1024, 64
SIZES = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2500)
FAMILIES = ("overlap", "disjoint", "equal", "nested", "random")
ALT_MODES = ("none", "all", "mixed")
FIELDS = ("src", "secondary", "secondary_all", "sub", "alt_sc", "sub_n", "mapq")


def check_limits(dev):
    assert dev.primary_limits() == dict(lane_max=LANE_MAX, lds_small=LDS_SMALL, lds_big=LDS_BIG, scan=SCAN), "a switch point of the library moved: aim the cases at it"
    for n in (LANE_MAX, LDS_SMALL, LDS_BIG, SCAN):
        assert {n - 1, n, n + 1} <= set(SIZES), n
    assert max(SIZES) > 2 * LDS_BIG


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------------------
def ref_opt() -> MemOpt:
    """mem_opt_init()'s mem_opt_t, copied into the mirror struct (same layout: refapi.lib() asserts the sizes)."""
    L = refapi.lib()
    L.refshim_opt_init.restype = C.c_void_p
    p = L.refshim_opt_init()
    o = MemOpt()
    C.memmove(C.byref(o), p, C.sizeof(MemOpt))
    L.refshim_free(p)
    return o


def ref_primary(opt, counts, regs, ids):
    """mem_mark_primary_se on every list, then mem_approx_mapq_se on every marked region -> (PRIMARY_DTYPE records, n_pri).  A region's index in its list
    travels in seedlen0, which neither function reads."""
    L = refapi.lib()
    L.mem_mark_primary_se.restype = C.c_int
    L.mem_mark_primary_se.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    L.mem_approx_mapq_se.restype = C.c_int
    L.mem_approx_mapq_se.argtypes = [C.c_void_p, C.c_void_p]
    a = np.ascontiguousarray(regs, dtype=ALNREG_DTYPE).copy()
    n_pri = np.zeros(len(counts), dtype=np.int32)
    lo = 0
    for i, c in enumerate(counts):
        c = int(c)
        a["seedlen0"][lo:lo + c] = np.arange(c)
        n_pri[i] = L.mem_mark_primary_se(C.byref(opt), c, a.ctypes.data + lo * ALNREG_DTYPE.itemsize, int(ids[i]))
        h = a["hash"][lo:lo + c]      # (the hash the records leave to their consumer: hash_64(id + src))
        assert c == 0 or len(set(h.tolist())) == c
        lo += c
    out = np.zeros(a.shape[0], dtype=PRIMARY_DTYPE)
    out["src"] = a["seedlen0"]
    for f in ("secondary", "secondary_all", "sub", "alt_sc", "sub_n"):
        out[f] = a[f]
    base = a.ctypes.data
    for k in range(a.shape[0]):
        out["mapq"][k] = L.mem_approx_mapq_se(C.byref(opt), base + k * ALNREG_DTYPE.itemsize)
    return out, n_pri


def assert_records_equal(got, n_pri, want, want_n_pri, counts, what, flags_zero=True):
    assert got.shape == want.shape, what
    assert np.array_equal(n_pri, want_n_pri), f"{what}: n_pri differs for reads {np.nonzero(n_pri != want_n_pri)[0][:10].tolist()}"
    bad = np.zeros(got.shape[0], dtype=bool)
    for f in FIELDS:
        bad |= got[f] != want[f]
    if bad.any():
        k = int(np.nonzero(bad)[0][0])
        ends = np.cumsum(counts)
        r = int(np.searchsorted(ends, k, side="right"))
        lo = int(ends[r] - counts[r])
        raise AssertionError(f"{what}: {int(bad.sum())} records differ; first: read {r} ({int(counts[r])} regions), record {k - lo}\n device    {got[k]}\n reference {want[k]}")
    if flags_zero:
        assert not (got["flags"] & 1).any(), f"{what}: {int((got['flags'] & 1).sum())} records were left to the host's logarithms"


# ---- generated region lists -----------------------------------------------------------------------------------------------------------------------------
def make_list(rng, n, family, alt_mode, extras):
    """n regions of one read.  Inputs stay where the reference is defined: qe > qb, re > rb, score >= 0, seedcov >= 1."""
    a = np.zeros(n, dtype=ALNREG_DTYPE)
    if n == 0:
        return a
    k = np.arange(n)
    if family == "overlap":
        qb = rng.integers(0, 10, n); qe = rng.integers(90, 101, n)
    elif family == "disjoint":
        qb = k * 10 + rng.integers(0, 2, n); qe = qb + rng.integers(1, 8, n)
    elif family == "nested":
        p = rng.permutation(n); qb = p; qe = 2 * n + 10 - p
    else:
        qb = rng.integers(0, 140, n); qe = qb + rng.integers(1, 151 - qb)
    a["qb"], a["qe"] = qb, qe
    a["score"] = 57 if family == "equal" else rng.integers(0, 151, n)
    if family == "random" and n > 2:
        a["score"][rng.integers(0, n, max(1, n // 8))] = a["score"][0]      # runs of equal scores: the hash decides
    a["rb"] = rng.integers(0, 1 << 40, n)
    a["re"] = a["rb"] + np.maximum(1, (qe - qb) + rng.integers(-3, 12, n))
    a["seedcov"] = rng.integers(1, 201, n)
    a["truesc"] = a["score"]; a["rid"] = rng.integers(0, 3, n); a["w"] = 100
    alt = {"none": np.zeros(n, dtype=np.uint32), "all": np.ones(n, dtype=np.uint32), "mixed": rng.integers(0, 2, n).astype(np.uint32)}[alt_mode]
    a["ncomp_isalt"] = (alt << np.uint32(30)) | rng.integers(1, 4, n).astype(np.uint32)
    a["csub"] = np.where(rng.random(n) < 0.5, 0, rng.integers(0, 160, n))
    if extras:      # values a caller may bring along: they are read as given
        a["sub_n"] = rng.integers(0, 40, n)
        a["frac_rep"] = rng.random(n).astype(np.float32) * np.float32(0.9)
        a["sub"] = rng.integers(0, 99, n); a["secondary"] = rng.integers(-1, 5, n); a["alt_sc"] = 7      # (all reset by the marking)
    a["hash"] = rng.integers(0, 1 << 62, n).astype(np.uint64)
    return a


def opt_variants():
    """(name, opt): mask_level 0 .. 1, gap penalties that change `tmp` (bwamem.c:522-524), both mapQ branches, other scores."""
    out = []
    for name, kw in (("default", {}), ("mask0", dict(mask_level=0.0)), ("mask1", dict(mask_level=1.0)), ("mask0.8", dict(mask_level=0.8)),
                     ("del20", dict(o_del=20, e_del=3)), ("ins15", dict(o_ins=15, e_ins=2, mask_level=0.3)), ("coef0", dict(mapQ_coef_len=0.0)),
                     ("coef0_a2", dict(mapQ_coef_len=0.0, a=2, b=3, min_seed_len=25)), ("coef200_fac5", dict(mapQ_coef_len=200.0, mapQ_coef_fac=5, b=9))):
        o = ref_opt()
        for k, v in kw.items():
            setattr(o, k, v)
        out.append((name, o))
    return out


def fuzz_cells(thin, rot):
    """(size, family, alt mode, extras): the full cross product, or (thin) every cell for the sizes one lane handles and a rotating few for the others
    -- every size in every call, every family and ALT mode at every form of the kernels over the calls."""
    cells = []
    for si, n in enumerate(SIZES):
        combos = [(f, m) for f in FAMILIES for m in ALT_MODES]
        if thin and n > LANE_MAX + 1:
            take = 3 if n <= LDS_SMALL + 1 else 1
            combos = [combos[(rot * 4 + si * 7 + j * 5) % len(combos)] for j in range(take)]
        for j, (f, m) in enumerate(combos):
            cells.append((n, f, m, (si + j + rot) % 3 == 0))
    return cells


def run_fuzz(dev, seed, thin):
    check_limits(dev)
    rng = np.random.default_rng(seed)
    seen_f, seen_m, seen_np = {}, {}, set()
    for vi, (name, opt) in enumerate(opt_variants()):
        cells = fuzz_cells(thin, vi + seed)
        lists = [make_list(rng, n, f, m, x) for n, f, m, x in cells]
        counts = np.array([c[0] for c in cells], dtype=np.int32)
        regs = np.concatenate(lists)
        ids = rng.integers(0, 1 << 20, len(cells)).astype(np.int64)
        ids[::3] += rng.integers(1 << 32, 1 << 50, len(ids[::3]))      # ids above 2^32
        want, want_np = ref_primary(opt, counts, regs, ids)
        got, n_pri, ms = dev.primary_flat(opt, counts, regs, ids)
        assert ms >= 0
        assert_records_equal(got, n_pri, want, want_np, counts, f"fuzz seed {seed}, options {name}")
        assert set(counts.tolist()) == set(SIZES)
        for (n, f, m, x), p in zip(cells, want_np):
            form = 0 if n <= LANE_MAX else 1 if n <= LDS_SMALL else 2 if n <= LDS_BIG else 3
            seen_f.setdefault(form, set()).add(f); seen_m.setdefault(form, set()).add(m)
            if n > 1:
                seen_np.add("zero" if p == 0 else "all" if p == n else "between")
    for form in range(4):
        assert seen_f[form] == set(FAMILIES) and seen_m[form] == set(ALT_MODES), (form, seen_f[form], seen_m[form])
    assert seen_np == {"zero", "all", "between"}      # both rounds of bwamem.c:564-577 ran, and neither
    run_mixed(dev, seed)


def run_mixed(dev, seed):
    """128 consecutive reads whose sizes run through every form of the kernels within each wavefront (a cycle of seven, so the places shift from one wavefront
    to the next): the lanes' hand-over with all three lists live in one ballot and no list taking a whole wavefront."""
    rng = np.random.default_rng(seed + 1000)
    opt = ref_opt()
    cyc = (LANE_MAX, LDS_SMALL + 1, 0, LANE_MAX + 1, LDS_BIG + 1, 1, LDS_SMALL)
    counts = np.array([cyc[i % len(cyc)] for i in range(128)], dtype=np.int32)
    regs = np.concatenate([make_list(rng, int(n), FAMILIES[i % len(FAMILIES)], ALT_MODES[i % len(ALT_MODES)], i % 4 == 0) for i, n in enumerate(counts)])
    ids = rng.integers(0, 1 << 40, counts.shape[0]).astype(np.int64)
    want, want_np = ref_primary(opt, counts, regs, ids)
    got, n_pri, _ = dev.primary_flat(opt, counts, regs, ids)
    assert_records_equal(got, n_pri, want, want_np, counts, f"128 reads of mixed forms, seed {seed}")


# ---- real batches ---------------------------------------------------------------------------------------------------------------------------------------
def alt_prefix(tmp_path, prefix, alt_names):
    new = str(tmp_path / "alt_idx")
    for ext in ("bwt", "sa", "pac", "ann", "amb"):
        os.symlink(os.path.abspath(prefix + "." + ext), new + "." + ext)
    with open(new + ".alt", "w") as f:
        for nme in alt_names:
            f.write(f"{nme}\t0\tchr1\t1\t60\t100M\t*\t0\t0\t*\t*\n")
    return new


def batch_reads(g, lens, n, seed):
    """Reads from the whole genome (its repeat families give several regions per read), from the contig that is flagged ALT, and chimeras of two places
    (two regions that do not overlap on the read)."""
    lo = sum(lens[:2])
    a = simdata.make_reads_se(g, n, seed=seed)
    b = simdata.make_reads_se(g[lo:], n // 2, seed=seed + 1)
    c = simdata.make_reads_se(g, n // 2, seed=seed + 2)
    d = simdata.make_reads_se(g, n // 2, seed=seed + 3)
    chim = np.concatenate([c[:, :75], d[:, 75:]], axis=1)
    return np.concatenate([a, b, chim])


def run_batches(dev, g, lens, n, seed, id0s):
    opt = ref_opt()
    reads = batch_reads(g, lens, n, seed)
    seqs, off = testdata.flat(reads)
    dev.upload(seqs, off); dev.run(opt)
    counts, regs = dev.download()
    assert int((regs["ncomp_isalt"] >> 30).sum()) > 0 and int(counts.max()) >= 3, "the batch has no ALT hit or no read with several regions"
    for id0 in id0s:
        ids = id0 + np.arange(counts.shape[0], dtype=np.int64)
        want, want_np = ref_primary(opt, counts, regs, ids)
        got, n_pri, ms = dev.primary(opt, id0)
        assert_records_equal(got, n_pri, want, want_np, counts, f"batch of {counts.shape[0]} reads, id0 {id0}")
    assert len({int(p == 0) + 2 * int(p == c) for p, c in zip(want_np, counts) if c > 1}) >= 2
    # a table of logarithms too small for any read: every mapQ that needs one is flagged and comes from the host side of the call -- the same value
    dev.set_option("pri_log_cap", 2)
    try:
        got, n_pri, _ = dev.primary(opt, id0s[-1])
        assert_records_equal(got, n_pri, want, want_np, counts, "tiny table of logarithms", flags_zero=False)
        assert int((got["flags"] & 1).sum()) > counts.shape[0] // 4, "no record was flagged"
    finally:
        dev.set_option("pri_log_cap", 0)
    got, n_pri, _ = dev.primary(opt, id0s[-1])
    assert_records_equal(got, n_pri, want, want_np, counts, "table of logarithms grown again")
    return counts, regs


# ---- the command line -----------------------------------------------------------------------------------------------------------------------------------
def run_cli(cli, ref_prefix, prefix, fq, K, env):
    """single-end SAM of `cli` with and without BWAGPU_CLI_PRIMARY against `bwa mem` (ref_prefix: the same index for the reference binary)"""
    body = lambda t: b"\n".join(l for l in t.split(b"\n") if not l.startswith(b"@PG"))
    args = ["mem", "-K", str(K), "-t", "2"]
    p = subprocess.run([refapi.REF_BWA] + args + [ref_prefix, fq], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-1000:]
    want = body(p.stdout)
    assert b"\tpa:f:" in want or b"AH:*" in want or b"XA:Z:" in want
    outs = {}
    for on in (True, False):
        e = dict(env, BWAGPU_CLI_TRACE="1")
        e.pop("BWAGPU_CLI_PRIMARY", None)
        if on:
            e["BWAGPU_CLI_PRIMARY"] = "1"
        p = subprocess.run([cli] + args + [prefix, fq], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        outs[on] = (body(p.stdout), p.stderr.decode())
    assert outs[True][0] == want, "BWAGPU_CLI_PRIMARY=1: SAM differs from bwa mem"
    assert outs[False][0] == want, "switch unset: SAM differs from bwa mem"
    line = [l for l in outs[True][1].split("\n") if "reads finalized from device primary/mapQ records" in l]
    assert len(line) == 1 and int(line[0].split("]")[1].split()[0]) > 0, outs[True][1][-1500:]
    assert "reads finalized from device primary/mapQ records" not in outs[False][1]
    return want


# ---- mock runtime ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim():
    import hostsim_build
    prefix, _ = testdata.small_index()
    s = BwaGpu(prefix, lib_path=hostsim_build.build(), options={"ptab_m": 6})
    yield s
    s.close()


def test_struct_and_limits(sim):
    assert PRIMARY_DTYPE.itemsize == 32
    check_limits(sim)
    o = ref_opt()
    assert (o.a, o.b, o.min_seed_len, o.mapQ_coef_fac) == (1, 4, 19, 3) and abs(o.mask_level - 0.5) < 1e-9 and o.mapQ_coef_len == 50.0


def test_sim_primary_flat_fuzz(sim):
    run_fuzz(sim, 11, thin=True)


def test_sim_primary_on_batches(tmp_path):
    import hostsim_build
    prefix, g = testdata.small_index()
    lens = testdata.small_genome()[1]
    s = BwaGpu(alt_prefix(tmp_path, prefix, ["chr3"]), lib_path=hostsim_build.build(), options={"ptab_m": 6})
    try:
        run_batches(s, g, lens, 60, 501, (0, (1 << 33) + 12345))
    finally:
        s.close()


def test_sim_cli_primary(tmp_path):
    import test_cli
    prefix, g = testdata.small_index()
    lens = testdata.small_genome()[1]
    alt = alt_prefix(tmp_path, prefix, ["chr3"])
    fq = str(tmp_path / "se.fq")
    simdata.write_fastq(fq, batch_reads(g, lens, 20, 511))
    env = dict(os.environ, BWAGPU_CLI_STREAMS="2", BWAGPU_CLI_SERIALIZE="1", BWAGPU_PTAB_M="6")
    want = run_cli(test_cli._sim_cli(), alt, alt, fq, 1500, env)      # (ten reads per batch: id0 > 0 from the second batch on)
    assert want.count(b"\n") >= 40


def test_error_paths(sim):
    opt = ref_opt()
    L, h = sim.L, sim.h
    p, n, ms = C.c_void_p(), C.c_int64(), C.c_float()
    reads = simdata.make_reads_se(testdata.small_genome()[0], 4, seed=3)
    seqs, off = testdata.flat(reads)
    sim.upload(seqs, off)
    assert L.bwagpu_batch_primary(h, C.byref(opt), 0, C.byref(p), C.byref(n), None, None) == -2, "before a run"
    sim.run(opt)
    assert L.bwagpu_batch_primary(h, C.byref(opt), 0, C.byref(p), C.byref(n), None, None) == -2, "before a download"
    counts, regs = sim.download()
    for args in ((None, C.byref(opt), 0, C.byref(p), C.byref(n), None, None), (h, None, 0, C.byref(p), C.byref(n), None, None),
                 (h, C.byref(opt), 0, None, C.byref(n), None, None), (h, C.byref(opt), 0, C.byref(p), None, None, None)):
        assert L.bwagpu_batch_primary(*args) == -2
    assert L.bwagpu_batch_primary(h, C.byref(opt), 0, C.byref(p), C.byref(n), None, None) == 0 and n.value == int(counts.sum())      # n_pri and kernel_ms may be NULL
    L.bwagpu_free(p)
    got, n_pri, _ = sim.primary(opt, 5)
    want, want_np = ref_primary(opt, counts, regs, 5 + np.arange(4))
    assert_records_equal(got, n_pri, want, want_np, counts, "four reads")
    # bwagpu_primary_flat: NULL arguments, a negative count, no reads, reads without regions
    c1, ids1 = np.array([1], dtype=np.int32), np.array([9], dtype=np.int64)
    r1 = make_list(np.random.default_rng(1), 1, "random", "none", False)
    assert L.bwagpu_primary_flat(None, C.byref(opt), 1, c1.ctypes.data, r1.ctypes.data, ids1.ctypes.data, C.byref(p), None, None) == -2
    assert L.bwagpu_primary_flat(h, None, 1, c1.ctypes.data, r1.ctypes.data, ids1.ctypes.data, C.byref(p), None, None) == -2
    assert L.bwagpu_primary_flat(h, C.byref(opt), 1, None, r1.ctypes.data, ids1.ctypes.data, C.byref(p), None, None) == -2
    assert L.bwagpu_primary_flat(h, C.byref(opt), 1, c1.ctypes.data, None, ids1.ctypes.data, C.byref(p), None, None) == -2
    assert L.bwagpu_primary_flat(h, C.byref(opt), 1, c1.ctypes.data, r1.ctypes.data, None, C.byref(p), None, None) == -2
    assert L.bwagpu_primary_flat(h, C.byref(opt), 1, c1.ctypes.data, r1.ctypes.data, ids1.ctypes.data, None, None, None) == -2
    assert L.bwagpu_primary_flat(h, C.byref(opt), -1, c1.ctypes.data, r1.ctypes.data, ids1.ctypes.data, C.byref(p), None, None) == -2
    neg = np.array([-1], dtype=np.int32)
    assert L.bwagpu_primary_flat(h, C.byref(opt), 1, neg.ctypes.data, r1.ctypes.data, ids1.ctypes.data, C.byref(p), None, None) == -2
    assert L.bwagpu_primary_flat(h, C.byref(opt), 1, c1.ctypes.data, r1.ctypes.data, ids1.ctypes.data, C.byref(p), None, None) == 0
    L.bwagpu_free(p)
    assert L.bwagpu_primary_flat(h, C.byref(opt), 0, None, None, None, C.byref(p), None, None) == 0
    L.bwagpu_free(p)
    got, n_pri, _ = sim.primary_flat(opt, np.zeros(3, dtype=np.int32), np.zeros(0, dtype=ALNREG_DTYPE), np.arange(3))
    assert got.shape[0] == 0 and n_pri.tolist() == [0, 0, 0]
    # a batch without reads
    sim.upload(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64)); sim.run(opt)
    assert L.bwagpu_batch_primary(h, C.byref(opt), 0, C.byref(p), C.byref(n), None, None) == -2
    counts, regs = sim.download()
    got, n_pri, ms = sim.primary(opt, 0)
    assert got.shape[0] == 0 and n_pri.shape[0] == 0 and ms == 0.0
    # reads none of which has a region
    junk = np.tile(np.array([0, 1, 2, 3], dtype=np.uint8), 5)[None, :].repeat(2, axis=0)
    sim.upload(*testdata.flat(junk)); sim.run(opt)
    counts, regs = sim.download()
    if int(counts.sum()) == 0:
        got, n_pri, _ = sim.primary(opt, 0)
        assert got.shape[0] == 0 and n_pri.tolist() == [0, 0]


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    prefix, _ = testdata.small_index()
    g = BwaGpu(prefix)
    yield g
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [21, 22, 23])
def test_gpu_primary_flat_fuzz(gpu, seed):
    run_fuzz(gpu, seed, thin=False)


@pytest.mark.gpu
def test_gpu_primary_on_batches(tmp_path):
    fa, g = testdata.medium_index()
    lens = simdata.make_genome(**testdata.MEDIUM)[1]
    dev = BwaGpu(alt_prefix(tmp_path, fa, ["chr3"]))
    try:
        counts, regs = run_batches(dev, g, lens, 6000, 601, (0, (1 << 35) + 7771))
        assert int(counts.max()) > LANE_MAX, "no read for the wavefront form"
    finally:
        dev.close()


@pytest.mark.gpu
def test_gpu_cli_primary(tmp_path):
    from bwa_amd import build as b
    _, cli = b.build_host(verbose=False)
    fa, g = testdata.medium_index()
    lens = simdata.make_genome(**testdata.MEDIUM)[1]
    alt = alt_prefix(tmp_path, fa, ["chr3"])
    fq = str(tmp_path / "se.fq")
    simdata.write_fastq(fq, batch_reads(g, lens, 4000, 611))
    want = run_cli(cli, alt, alt, fq, 300000, dict(os.environ))      # (2000 reads per batch)
    assert want.count(b"\n") >= 8000
