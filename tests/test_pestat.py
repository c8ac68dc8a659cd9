"""Insert-size statistics on the device (bwagpu_batch_pestat, bwagpu_pestat_flat, bwagpu_batch_pestat_hist, bwagpu_pestat_finish; bwa_amd/csrc/dev_pestat.h)
against the compiled reference's own mem_pestat (bwamem_pair.c:72-135), which oracle/_ref/libbwaref.so exports, called as test_pair.Ref.pestat does.  All 128
bytes of pes must be equal.  info.n is held to a direct count of the filter's definition (:78-90) in numpy, info.p25 / p50 / p75 to the order statistics of
that list, and info's remaining fields (the outlier bounds, x, sum) to the same lines restated on the list -- so a mismatch in pes can be pinned to an operation.

1. a crafted fuzz of bwagpu_pestat_flat: lists synthesised region by region and aimed at every decision of the function (SCENARIOS);
2. real batches: run -> download -> pestat(opt) against the reference on the downloaded lists;
3. additivity: the batch cut into two and three shards, pestat_hist per shard, summed, pestat_finish; pestat_hist + pestat_finish on one handle;
4. `bwa-amd mem` with BWAGPU_CLI_PESTAT=1 against `bwa mem`: SAM, two devices (the histogram path), the [M::mem_pestat] lines at -v 3;
5. error paths.
CPU: on the mock runtime (tests/hostsim), thinned.  -m gpu: everything, three seeds."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import refapi
import testdata
import test_pair as tpair
import test_primary as tp
from bwa_amd import simdata
from bwa_amd.api import BwaGpu
from bwa_amd.structs import ALNREG_DTYPE, PESTAT_DTYPE, PESTAT_INFO_DTYPE

pytestmark = pytest.mark.skipif(not refapi.have_ref(), reason="oracle/_ref not built")

MIN_DIR_CNT, MAX_INS_LIMIT = 10, 1 << 22


# ---- the filter and the scalars by their definition -------------------------------------------------------------------------------------------------------
def np_cal_sub(opt, a):
    """cal_sub (:58-70): the overlap test is int >= int * float in single precision"""
    for j in range(1, a.shape[0]):
        b_max = max(int(a["qb"][j]), int(a["qb"][0])); e_min = min(int(a["qe"][j]), int(a["qe"][0]))
        if e_min > b_max:
            min_l = min(int(a["qe"][j]) - int(a["qb"][j]), int(a["qe"][0]) - int(a["qb"][0]))
            if np.float32(e_min - b_max) >= np.float32(min_l) * np.float32(opt.mask_level):
                return int(a["score"][j])
    return opt.min_seed_len * opt.a


def np_isizes(opt, l_pac, counts, regs):
    """-> the four lists isize[d] (:78-90), unsorted"""
    out = [[] for _ in range(4)]
    ends = np.concatenate([[0], np.cumsum(counts)])
    for p in range(len(counts) >> 1):
        a0, a1 = regs[ends[2 * p]:ends[2 * p + 1]], regs[ends[2 * p + 1]:ends[2 * p + 2]]
        if a0.shape[0] == 0 or a1.shape[0] == 0:
            continue
        if np_cal_sub(opt, a0) > 0.8 * int(a0["score"][0]) or np_cal_sub(opt, a1) > 0.8 * int(a1["score"][0]):
            continue
        if a0["rid"][0] != a1["rid"][0]:
            continue
        b1, b2 = int(a0["rb"][0]), int(a1["rb"][0])
        r1, r2 = b1 >= l_pac, b2 >= l_pac
        p2 = b2 if r1 == r2 else 2 * l_pac - 1 - b2
        dist = abs(p2 - b1)
        d = (0 if r1 == r2 else 1) ^ (0 if p2 > b1 else 3)
        if dist and dist <= opt.max_ins:
            out[d].append(dist)
    return out


def check_info(info, isz, what):
    """info against the lists; returns for every live orientation whether the MAX_STDDEV widening moved (low, high)"""
    widened = {}
    for d in range(4):
        q = sorted(isz[d]); n = len(q)
        assert int(info["n"][d]) == n, f"{what}: orientation {d}: n {int(info['n'][d])}, the filter's definition gives {n}"
        if n < MIN_DIR_CNT:
            for f in ("p25", "p50", "p75", "lo_out", "hi_out", "x", "sum", "sumsq"):
                assert info[f][d] == 0, (what, d, f)
            continue
        p25, p50, p75 = q[int(.25 * n + .499)], q[int(.50 * n + .499)], q[int(.75 * n + .499)]
        assert (int(info["p25"][d]), int(info["p50"][d]), int(info["p75"][d])) == (p25, p50, p75), f"{what}: orientation {d}: percentiles {info['p25'][d], info['p50'][d], info['p75'][d]}, the list's are {p25, p50, p75}"
        low = max(1, int(p25 - 2.0 * (p75 - p25) + .499)); high = int(p75 + 2.0 * (p75 - p25) + .499)
        inside = [v for v in q if low <= v <= high]
        assert len(inside) >= 1, "the reference would divide by zero"      # (p25 itself lies inside)
        assert (int(info["lo_out"][d]), int(info["hi_out"][d]), int(info["x"][d])) == (low, high, len(inside)), (what, d)
        assert float(info["sum"][d]) == float(sum(inside)), (what, d)
        widened[d] = (low, high, len(inside), int(p25 - 3.0 * (p75 - p25) + .499), int(p75 + 3.0 * (p75 - p25) + .499))
    return widened


def assert_pes_equal(got, want, info, what):
    assert got.dtype == want.dtype == PESTAT_DTYPE and got.shape == want.shape == (4,)
    if got.tobytes() == want.tobytes():
        return
    lines = [f"{what}: pes differs from mem_pestat"]
    for d in range(4):
        if got[d].tobytes() != want[d].tobytes():
            x = int(info["x"][d])
            avg = float(info["sum"][d]) / x if x else float("nan")
            lines.append(f" orientation {d}: device {got[d]}  reference {want[d]}  info: n {info['n'][d]} x {x} sum {info['sum'][d]!r} sumsq {info['sumsq'][d]!r}; "
                         f"sum / x = {avg!r}, sqrt(sumsq / x) = {math.sqrt(float(info['sumsq'][d]) / x) if x else float('nan')!r}")
    raise AssertionError("\n".join(lines))


# ---- generated lists --------------------------------------------------------------------------------------------------------------------------------------
# An end's list by kind: (kept by the cal_sub test?, builder).  The first region is read positions [0, 100) with score S.
def _regs(rows):
    a = np.zeros(len(rows), dtype=ALNREG_DTYPE)
    for k, (qb, qe, score) in enumerate(rows):
        a["qb"][k] = qb; a["qe"][k] = qe; a["score"][k] = score
    a["re"] = 100
    return a


def end_list(kind):
    if kind == "single":      return _regs([(0, 100, 60)])                                  # falls back to min_seed_len * a = 19 <= 48
    if kind == "single24":    return _regs([(0, 100, 24)])                                  # 19 <= 19.2
    if kind == "single23":    return _regs([(0, 100, 23)])                                  # 19 > 18.4: dropped
    if kind == "no_overlap":  return _regs([(0, 100, 50), (100, 150, 49)])                  # e_min == b_max: no overlap, falls back
    if kind == "one_short":   return _regs([(0, 100, 50), (51, 151, 49)])                   # 49 < 100 * 0.5: one base short of mask_level
    if kind == "at_level41":  return _regs([(0, 100, 50), (50, 150, 41)])                   # 50 >= 50.0: significant; 41 > 40.0: dropped
    if kind == "sub40":       return _regs([(0, 100, 50), (10, 90, 40)])                    # 40 > 40.0 is false: kept
    if kind == "sub41":       return _regs([(0, 100, 50), (10, 90, 41)])                    # dropped
    if kind == "short_first": return _regs([(0, 100, 50), (60, 100, 30)])                   # min_l is the other region's 40; overlap 40 >= 20: sub 30, kept
    if kind == "later":       return _regs([(0, 100, 50), (100, 160, 49), (71, 131, 49), (20, 80, 45)])      # the first significant overlap is the fourth region's: dropped
    if kind in ("long_keep", "long_drop"):      # 300 regions whose only significant overlap is the last
        rows = [(0, 100, 50)] + [(100 + k, 140 + k, 49) for k in range(298)] + [(0, 100, 30 if kind == "long_keep" else 45)]
        return _regs(rows)
    raise KeyError(kind)


KEEP = ("single", "single24", "no_overlap", "one_short", "sub40", "short_first", "long_keep")
DROP = ("single23", "at_level41", "sub41", "later", "long_drop")


def place(a0, a1, l_pac, d, dist, r1, rid=0):
    """put the two ends' first regions on contig rid so that mem_infer_dir gives orientation d and distance dist, the first end on strand r1"""
    big = dist > l_pac // 4
    if big:      # the mate's coordinate on the first end's strand must stay on that side of l_pac: a large distance has one way to go
        r1 = 1 if d in (0, 1) else 0
    b1 = (l_pac + l_pac // 2 + 7 * (dist % 97)) if r1 else (l_pac // 2 + 11 * (dist % 89))
    p2 = b1 + dist if d in (0, 1) else b1 - dist
    assert (p2 >= l_pac) == bool(r1) or dist == 0
    b2 = p2 if d in (0, 3) else 2 * l_pac - 1 - p2
    a0["rb"][0] = b1; a1["rb"][0] = b2; a0["rid"] = rid; a1["rid"] = rid
    a0["re"] = a0["rb"] + 100; a1["re"] = a1["rb"] + 100
    return a0, a1


class Builder:
    def __init__(self, rng, l_pac):
        self.rng, self.l_pac, self.lists, self.k = rng, l_pac, [], 0

    def kept(self, d, dist, long_every=0):
        """a pair that passes the filter (when 1 <= dist <= max_ins) with orientation d and insert size dist; the kinds, strands and contigs rotate"""
        k = self.k; self.k += 1
        kinds = KEEP if long_every and k % long_every == 0 else KEEP[:-1]
        a0, a1 = end_list(kinds[k % len(kinds)]), end_list(kinds[(k // len(kinds) + 3) % len(kinds)])
        self.lists += list(place(a0, a1, self.l_pac, d, int(dist), k & 1, rid=k % 3))

    def noise(self, max_ins, long_lists):
        """pairs the filter must drop: every dropping kind on either end, empty ends, unequal contigs, distances 0 and max_ins + 1"""
        for j, kind in enumerate(DROP if long_lists else DROP[:-1]):
            a0, a1 = end_list(kind), end_list("single")
            if j & 1:
                a0, a1 = a1, a0
            self.lists += list(place(a0, a1, self.l_pac, j % 4, 1 + j, j & 1))
        e = np.zeros(0, dtype=ALNREG_DTYPE)
        for j in range(3):
            a0, a1 = place(end_list("single"), end_list("sub40"), self.l_pac, j, 5 + j, j & 1)
            self.lists += [(e, a1), (a0, e), (e, e)][j]
        a0, a1 = place(end_list("single"), end_list("single"), self.l_pac, 1, 7, 0); a1["rid"] = 1
        self.lists += [a0, a1]
        for d in range(4):
            for dist in (0, max_ins + 1):
                self.lists += list(place(end_list("single"), end_list("single"), self.l_pac, d, dist, d & 1))

    def done(self, odd):
        if odd:      # a trailing unpaired read: n >> 1 ignores it
            self.lists.append(place(end_list("single"), end_list("single"), self.l_pac, 1, 3, 0)[0])
        counts = np.array([a.shape[0] for a in self.lists], dtype=np.int32)
        return counts, np.concatenate(self.lists) if self.lists else np.zeros(0, dtype=ALNREG_DTYPE)


def tails(n, center=400, core=5, far=14):
    """a narrow core with a fifth of the values at either edge of the outlier bounds: 4 std exceeds 3 IQR, the MAX_STDDEV widening applies"""
    k = n // 5
    return [center - far] * k + [center + far] * k + [center - core + (j % (2 * core + 1)) for j in range(n - 2 * k)]


def scenarios(thin):
    """(name, max_ins, {orientation: values})"""
    out = []
    for c in (9, 10, 11):
        out.append((f"four orientations of {c}", 10000, {d: [300 + 10 * d + 3 * j for j in range(c)] for d in range(4)}))
    for c in range(10, 18):      # every rounding of the three percentile indices
        out.append((f"one orientation of {c}", 10000, {c % 4: [200 + (j * j) % 37 for j in range(c)]}))
    for mx in (200, 201):        # MIN_DIR_RATIO on both sides of equality: 10 < 200 * 0.05 is false, 10 < 201 * 0.05 is true
        for c in (9, 10, 11):
            out.append((f"{c} against a maximum of {mx}", 10000, {1: [350 + j % 90 for j in range(mx)], 2: [100 + j for j in range(c)]}))
    out.append(("none", 10000, {}))
    out.append(("all equal", 10000, {1: [417] * 25}))
    out.append(("two clusters with outliers", 10000, {0: [300 + j % 7 for j in range(40)] + [340 + j % 5 for j in range(40)] + [1, 2, 5000, 9999, 10000], 3: [50] * 6 + [60] * 6 + [2000]}))
    out.append(("low below 1", 10000, {2: [1, 1, 2, 3] + [40 + 13 * j for j in range(20)]}))
    out.append(("widened by MAX_STDDEV", 10000, {1: tails(100), 0: tails(55, 900, 3, 9)}))
    out.append(("edges of max_ins 50", 50, {1: [1] * 6 + [50] * 7, 3: [20 + j % 11 for j in range(30)]}))
    out.append(("max_ins 50, one below", 50, {0: [49, 50] * 7 + [48]}))
    big = MAX_INS_LIMIT
    out.append(("max_ins 1 << 22", big, {1: [big - j % 200 for j in range(64)] + [big, big], 2: [big - 100000 + 3 * j for j in range(12)], 0: [1] * 3}))
    if not thin:
        out.append(("max_ins 1 << 22, both ends of the histogram", big, {3: [1] * 8 + [big] * 9}))
    return out


def run_scenario(dev, ref, rng, name, max_ins, values, seen, long_lists, odd):
    opt = tp.ref_opt(); opt.max_ins = max_ins
    l_pac = ref.idx.l_pac
    B = Builder(rng, l_pac)
    items = [(d, v) for d, vs in values.items() for v in vs]
    for i in rng.permutation(len(items)):
        B.kept(items[i][0], items[i][1], long_every=17 if long_lists else 0)
    B.noise(max_ins, long_lists)
    counts, regs = B.done(odd)
    isz = np_isizes(opt, l_pac, counts, regs)
    for d in range(4):      # the case is what it was meant to be
        assert sorted(isz[d]) == sorted(values.get(d, [])), (name, d)
    want = ref.pestat(opt, counts, regs)
    got, info, ms = dev.pestat_flat(opt, counts, regs)
    assert ms >= 0
    aux = check_info(info, isz, name)
    assert_pes_equal(got, want, info, name)
    for d in range(4):
        n = len(isz[d])
        assert bool(want["failed"][d]) == (n < MIN_DIR_CNT or n < max(len(q) for q in isz) * 0.05), (name, d)
        if n < MIN_DIR_CNT:
            seen.add("few")
            continue
        low, high, x, lo3, hi3 = aux[d]
        seen.add("ratio" if want["failed"][d] else "live")
        seen.add("std0" if want["std"][d] == 0 else "std>0")
        seen.add("widened" if (int(want["low"][d]), int(want["high"][d])) != (max(1, lo3), hi3) else "not widened")
        if int(want["low"][d]) == 1 and lo3 < 1:
            seen.add("low clamped")
        if x < n:
            seen.add("outliers")
    seen.add(f"live {int((want['failed'] == 0).sum())}")
    return got


def run_fuzz(dev, ref, seed, thin):
    assert dev.pestat_limits() == dict(min_dir_cnt=MIN_DIR_CNT, max_ins=MAX_INS_LIMIT)
    rng = np.random.default_rng(seed)
    seen = set()
    for k, (name, max_ins, values) in enumerate(scenarios(thin)):
        run_scenario(dev, ref, rng, name, max_ins, values, seen, long_lists=not thin or k % 6 == 0, odd=bool(k & 1))
    # many workgroups on hot bins, and thousands of rounded additions in the sum of squares
    v = np.clip(np.rint(rng.normal(400, 40, 5000)), 1, 10000).astype(np.int64)
    run_scenario(dev, ref, rng, "5000 pairs, normal", 10000, {1: v.tolist()}, seen, long_lists=False, odd=False)
    need = {"few", "ratio", "live", "std0", "std>0", "widened", "not widened", "low clamped", "outliers", "live 0", "live 1", "live 4"}
    assert need <= seen, need - seen
    # beyond the limit: refused with a message, the host function stays for it
    opt = tp.ref_opt(); opt.max_ins = MAX_INS_LIMIT + 1
    a0, a1 = place(end_list("single"), end_list("single"), ref.idx.l_pac, 1, 100, 0)
    c2 = np.array([1, 1], dtype=np.int32); r2 = np.concatenate([a0, a1])
    pes = np.zeros(4, dtype=PESTAT_DTYPE)
    assert dev.L.bwagpu_pestat_flat(dev.h, C.byref(opt), 2, c2.ctypes.data, r2.ctypes.data, pes.ctypes.data, None, None) == -2
    assert b"max_ins" in dev.L.bwagpu_last_error(dev.h)
    for mi in (0, -5):      # no pair can qualify
        opt.max_ins = mi
        got, info, _ = dev.pestat_flat(opt, c2, r2)
        assert got.tobytes() == ref.pestat(opt, c2, r2).tobytes() and (got["failed"] == 1).all() and not info["n"].any()


# ---- real batches -----------------------------------------------------------------------------------------------------------------------------------------
def aligned(dev, opt, reads):
    dev.upload(*testdata.flat(reads)); dev.run(opt)
    return dev.download()


def run_batch(dev, ref, g, n_pairs, n_foreign, seed, shards):
    """n_pairs pairs in all, n_foreign of them with a foreign mate"""
    opt = tp.ref_opt()
    reads, _, _ = tpair.pe_reads(g, n_pairs - n_foreign, n_foreign, seed)
    what = f"batch of {n_pairs} pairs ({n_foreign} foreign mates), seed {seed}"
    parts = {}
    for S in shards:      # first, so that the whole batch is the handle's last download
        total = None
        for s in range(S):
            lo, hi = 2 * (n_pairs * s // S), 2 * (n_pairs * (s + 1) // S)
            aligned(dev, opt, reads[lo:hi])
            h, ms = dev.pestat_hist(opt)
            assert h.shape == (4, opt.max_ins + 1) and h.dtype == np.uint32 and ms >= 0
            total = h.astype(np.uint64) if total is None else total + h
        parts[S] = total
    counts, regs = aligned(dev, opt, reads)
    want = ref.pestat(opt, counts, regs)
    assert not want["failed"].all(), "mem_pestat found no orientation: the batch is too small"
    isz = np_isizes(opt, ref.idx.l_pac, counts, regs)
    got, info, ms = dev.pestat(opt)
    assert ms >= 0
    check_info(info, isz, what)
    assert_pes_equal(got, want, info, what)
    h1, _ = dev.pestat_hist(opt)
    for d in range(4):
        assert np.array_equal(h1[d], np.bincount(np.array(isz[d], dtype=np.int64), minlength=opt.max_ins + 1)), (what, d)
    got1, info1, _ = dev.pestat_finish(opt, h1)
    assert got1.tobytes() == got.tobytes() and info1.tobytes() == info.tobytes(), f"{what}: pestat_hist + pestat_finish is not pestat"
    for S, total in parts.items():
        assert np.array_equal(total, h1), f"{what}: the histograms of {S} shards do not add up to the batch's"
        gs, infos, _ = dev.pestat_finish(opt, total.astype(np.uint32))
        assert_pes_equal(gs, want, infos, f"{what}, {S} shards")
        assert infos.tobytes() == info.tobytes()
    return want


# ---- the command line -------------------------------------------------------------------------------------------------------------------------------------
def _mem(exe, args, env=None):
    p = subprocess.run([exe, "mem"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return b"\n".join(l for l in p.stdout.split(b"\n") if not l.startswith(b"@PG")), p.stderr.decode()


def pestat_lines(err):
    return [l for l in err.split("\n") if l.startswith("[M::mem_pestat]")]


def run_cli(cli, prefix, f1, f2, K, env, n_pairs, env2=None):
    """paired-end SAM of `cli` with BWAGPU_CLI_PESTAT=1 against `bwa mem`: device mate rescue on and off, BWAGPU_CLI_RESCUE on top, the switch unset, -I;
    one batch at -v 3; env2: the same over two devices (the histogram path)"""
    base = ["-K", str(K), "-t", "2"]
    files = [prefix, f1, f2]
    want, _ = _mem(refapi.REF_BWA, base + files)
    assert want.count(b"\n") >= 2 * n_pairs
    e_off = dict(env, BWAGPU_CLI_TRACE="1"); e_off.pop("BWAGPU_CLI_PESTAT", None)
    e_on = dict(e_off, BWAGPU_CLI_PESTAT="1")
    mark = "insert-size windows from 1 device(s) (BWAGPU_CLI_PESTAT)"
    for name, e in (("device mate rescue on", e_on), ("BWAGPU_CLI_MATESW=0", dict(e_on, BWAGPU_CLI_MATESW="0")), ("BWAGPU_CLI_RESCUE=1", dict(e_on, BWAGPU_CLI_RESCUE="1"))):
        sam, err = _mem(cli, base + files, e)
        assert sam == want, f"BWAGPU_CLI_PESTAT=1, {name}: SAM differs from bwa mem"
        assert err.count(mark) == 4, (name, err[-1500:])      # every batch
    sam, err = _mem(cli, base + files, e_off)
    assert sam == want and "BWAGPU_CLI_PESTAT" not in err, "switch unset"
    want_i, _ = _mem(refapi.REF_BWA, base + ["-I", "380,50"] + files)
    sam, err = _mem(cli, base + ["-I", "380,50"] + files, e_on)
    assert sam == want_i and mark not in err, "-I: the switch is ignored"
    if env2 is not None:
        sam, err = _mem(cli, base + files, dict(env2, BWAGPU_CLI_PESTAT="1", BWAGPU_CLI_TRACE="1", BWAGPU_CLI_MULTI="split"))
        assert sam == want, "BWAGPU_CLI_PESTAT=1 over two devices: SAM differs from bwa mem"
        assert err.count("insert-size windows from 2 device(s) (BWAGPU_CLI_PESTAT)") == 4, err[-1500:]
    one = ["-K", "100000000", "-t", "2", "-v", "3"]
    want1, werr = _mem(refapi.REF_BWA, one + files)
    sam, err = _mem(cli, one + files, e_on)
    assert sam == want1 and err.count(mark) == 1
    assert len(pestat_lines(werr)) >= 7 and pestat_lines(err) == pestat_lines(werr), "\n".join(pestat_lines(err) + ["-- reference:"] + pestat_lines(werr))
    _, err = _mem(cli, one + files, e_off)
    assert pestat_lines(err) == pestat_lines(werr)      # (the host path prints the same)


def cli_inputs(tmp_path, g, n_pairs, seed):
    a, b = simdata.make_reads_pe(g, n_pairs, seed=seed)
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
    r = tpair.Ref(testdata.small_index()[0])
    yield r
    r.close()


def test_structs():
    assert PESTAT_INFO_DTYPE.itemsize == 208 and PESTAT_INFO_DTYPE.fields["x"][1] == 112 and PESTAT_INFO_DTYPE.fields["sumsq"][1] == 176
    for kind in KEEP + DROP:
        o = tp.ref_opt()
        a = end_list(kind)
        assert (np_cal_sub(o, a) <= 0.8 * int(a["score"][0])) == (kind in KEEP), kind


def test_sim_pestat_flat_fuzz(sim, ref_small):
    run_fuzz(sim, ref_small, 61, thin=True)


def test_sim_pestat_on_batches(sim, ref_small):
    g = testdata.small_index()[1]
    run_batch(sim, ref_small, g, 36, 0, 721, (2,))
    run_batch(sim, ref_small, g, 36, 7, 722, (3,))


def test_sim_cli_pestat(tmp_path):
    import test_cli
    prefix, g = testdata.small_index()
    f1, f2 = cli_inputs(tmp_path, g, 64, 731)
    env = dict(os.environ, BWAGPU_CLI_STREAMS="2", BWAGPU_CLI_SERIALIZE="1", BWAGPU_PTAB_M="6")
    env2 = dict(env, MOCK_HIP_DEVICES="2", BWAGPU_DEVICES="0,1")
    run_cli(test_cli._sim_cli(), prefix, f1, f2, 4800, env, 64, env2)      # (sixteen pairs per batch)


def test_error_paths(sim, ref_small):
    opt = tp.ref_opt()
    L, h = sim.L, sim.h
    pes, info = np.zeros(4, dtype=PESTAT_DTYPE), np.zeros(1, dtype=PESTAT_INFO_DTYPE)
    P, I = pes.ctypes.data, info.ctypes.data
    ph, nb, ms = C.c_void_p(), C.c_int64(), C.c_float()
    g = testdata.small_genome()[0]
    reads, _, _ = tpair.pe_reads(g, 3, 0, 5)
    sim.upload(*testdata.flat(reads))
    ok = lambda: [h, C.byref(opt), P, I, C.byref(ms)]
    okh = lambda: [h, C.byref(opt), C.byref(ph), C.byref(nb), C.byref(ms)]
    assert L.bwagpu_batch_pestat(*ok()) == -2 and L.bwagpu_batch_pestat_hist(*okh()) == -2, "before a run"
    sim.run(opt)
    assert L.bwagpu_batch_pestat(*ok()) == -2 and L.bwagpu_batch_pestat_hist(*okh()) == -2, "before a download"
    counts, regs = sim.download()
    for k in (0, 1, 2):      # NULL h, opt, pes
        a = ok(); a[k] = None
        assert L.bwagpu_batch_pestat(*a) == -2, k
    for k in (0, 1, 2, 3):   # NULL h, opt, hist, n_bins
        a = okh(); a[k] = None
        assert L.bwagpu_batch_pestat_hist(*a) == -2, k
    assert L.bwagpu_batch_pestat(h, C.byref(opt), P, None, None) == 0      # info and kernel_ms may be NULL
    assert pes.tobytes() == ref_small.pestat(opt, counts, regs).tobytes() and (pes["failed"] == 1).all()      # (three pairs)
    assert L.bwagpu_batch_pestat_hist(h, C.byref(opt), C.byref(ph), C.byref(nb), None) == 0 and nb.value == 4 * (opt.max_ins + 1)
    hist = np.frombuffer(C.string_at(ph, nb.value * 4), dtype=np.uint32).copy()
    L.bwagpu_free(ph)
    # bwagpu_pestat_finish: NULL arguments, a wrong number of bins
    okf = lambda: [h, C.byref(opt), hist.ctypes.data, hist.size, P, I, C.byref(ms)]
    for k in (0, 1, 2, 4):
        a = okf(); a[k] = None
        assert L.bwagpu_pestat_finish(*a) == -2, k
    for bad in (hist.size - 1, hist.size + 4, 0, opt.max_ins + 1):
        a = okf(); a[3] = bad
        assert L.bwagpu_pestat_finish(*a) == -2, bad
    assert L.bwagpu_pestat_finish(h, C.byref(opt), hist.ctypes.data, hist.size, P, None, None) == 0
    big = tp.ref_opt(); big.max_ins = MAX_INS_LIMIT + 1
    for call, a in ((L.bwagpu_batch_pestat, ok()), (L.bwagpu_batch_pestat_hist, okh()), (L.bwagpu_pestat_finish, okf())):
        a[1] = C.byref(big)
        assert call(*a) == -2 and b"max_ins" in L.bwagpu_last_error(h)
    # bwagpu_pestat_flat: NULL arguments, a negative count, no reads, one read
    c2 = np.array([1, 1], dtype=np.int32)
    r2 = np.concatenate(place(end_list("single"), end_list("single"), ref_small.idx.l_pac, 1, 100, 0))
    okp = lambda: [h, C.byref(opt), 2, c2.ctypes.data, r2.ctypes.data, P, I, C.byref(ms)]
    for k in (0, 1, 3, 4, 5):
        a = okp(); a[k] = None
        assert L.bwagpu_pestat_flat(*a) == -2, k
    a = okp(); a[2] = -1
    assert L.bwagpu_pestat_flat(*a) == -2
    b = np.array([-1, 1], dtype=np.int32)
    a = okp(); a[3] = b.ctypes.data
    assert L.bwagpu_pestat_flat(*a) == -2
    assert L.bwagpu_pestat_flat(h, C.byref(opt), 2, c2.ctypes.data, r2.ctypes.data, P, None, None) == 0
    got, inf, _ = sim.pestat_flat(opt, c2, r2)
    assert inf["n"].tolist() == [0, 1, 0, 0] and (got["failed"] == 1).all()
    for n in (0, 1):
        got, inf, _ = sim.pestat_flat(opt, c2[:n], r2[:n])
        assert (got["failed"] == 1).all() and not inf["n"].any()
    # a batch without any region, and one without reads: four failed orientations
    junk = np.tile(np.array([0, 1, 2, 3], dtype=np.uint8), 5)
    sim.upload(*testdata.ragged([junk, junk, junk, junk])); sim.run(opt)
    counts, regs = sim.download()
    assert counts.sum() == 0
    got, inf, ms0 = sim.pestat(opt)
    assert (got["failed"] == 1).all() and got.tobytes() == ref_small.pestat(opt, counts, regs).tobytes() and ms0 == 0
    hz, _ = sim.pestat_hist(opt)
    assert hz.shape == (4, opt.max_ins + 1) and not hz.any()
    sim.upload(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64)); sim.run(opt); sim.download()
    got, inf, _ = sim.pestat(opt)
    assert (got["failed"] == 1).all() and not inf["n"].any()


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    g = BwaGpu(testdata.small_index()[0])
    yield g
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [71, 72, 73])
def test_gpu_pestat_flat_fuzz(gpu, ref_small, seed):
    run_fuzz(gpu, ref_small, seed, thin=False)


@pytest.fixture(scope="module")
def gpu_medium():
    fa, g = testdata.medium_index()
    dev, ref = BwaGpu(fa), tpair.Ref(fa)
    yield dev, ref, g
    dev.close(); ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [821, 822, 823])
def test_gpu_pestat_on_batches(gpu_medium, seed):
    dev, ref, g = gpu_medium
    run_batch(dev, ref, g, 4000, 0, seed, (2, 3))
    want = run_batch(dev, ref, g, 4000, 800, seed + 10, (2, 3))
    assert want["failed"][1] == 0


@pytest.mark.gpu
def test_gpu_cli_pestat(tmp_path):
    from bwa_amd import build as b
    _, cli = b.build_host(verbose=False)
    fa, g = testdata.medium_index()
    f1, f2 = cli_inputs(tmp_path, g, 4000, 831)
    run_cli(cli, fa, f1, f2, 300000, dict(os.environ), 4000)      # (a thousand pairs per batch)
