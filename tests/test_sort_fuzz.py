"""Differential fuzz of every form in which this tree restates klib's unstable ks_introsort (ksort.h:176-226), against the compiled reference's own
instances of it (KSORT_INIT emits non-static functions: ks_introsort_64, _128, _mem_intv, _mem_flt, _mem_ars2, _mem_ars, _mem_ars_hash, _mem_ars_hash2).
BWA-MEM's output depends on the tie behaviour of that sort -- which of two equally heavy chains is kept (bwamem.c:367), which of two regions with the same
end is p and which q (bwamem.c:467), which of two equal hits survives (bwamem.c:504), the order of equal-hash hits in the SAM (bwamem.c:423-426).

Device forms run through bwagpu_debug_sort (dev_debug.h: the product's routine, called where the product calls it, arrays where the product keeps them),
host forms through bwamem_host_debug_sort.  Expected orders: arrays of the reference's own structs, each element's index in a field the comparator
does not read, sorted by the reference.  Exact equality of permutations; for intervals and bare numbers, whose equal elements are identical records,
and for the two networks over distinct keys, equality of the sorted key sequence and that the output is a permutation.  Cases: tests/sortcases.py.

CPU: a thinned cross product of families and sizes on the mock runtime (tests/hostsim).  -m gpu: the full one, several draws."""
import ctypes as C

import numpy as np
import pytest

import refapi
import sortcases as sc
import testdata
from bwa_amd.api import BwaGpu, SORT_KEY_DTYPE
from bwa_amd.structs import ALNREG_DTYPE, INTV_DTYPE

pytestmark = pytest.mark.skipif(not refapi.have_ref(), reason="oracle/_ref not built")

K_U64, K_CHAIN_SEEDS, K_INTV, K_INTV_BLK, K_CHAIN_W, K_REG_END, K_REG_BEST, K_PAR_END, K_PAR_BEST = range(9)
# Where the forms change their method (dev_seed.h, dev_chainw.h, dev_dedup.h, dev_debug.h, dev_extw.h, dev_dedupp.h).  The cases are aimed at these, so they
# are checked against what the library under test was compiled with (bwagpu_debug_sort_limits) and have to be among the sizes the cases take.
PUB_MAX, CW_PW_LDS, CW_FLT_LDS, DEDUP_KEYSORT_MIN, PAR_CAP_MAX, CHAIN_SORT_LANE_MAX, DD_NET_DEFAULT = 4096, 768, 256, 24, 1100, 32, 129


def check_limits(dev):
    assert dev.debug_sort_limits() == dict(pub_max=PUB_MAX, cw_pw_lds=CW_PW_LDS, cw_flt_lds=CW_FLT_LDS, dedup_keysort_min=DEDUP_KEYSORT_MIN, par_cap_max=PAR_CAP_MAX,
                                           chain_sort_lane_max=CHAIN_SORT_LANE_MAX, dd_net_default=DD_NET_DEFAULT), "a switch point of the library moved: aim the cases at it"
    for n in (DEDUP_KEYSORT_MIN, CHAIN_SORT_LANE_MAX, DD_NET_DEFAULT, CW_FLT_LDS):
        assert {n - 1, n, n + 1} <= set(sc.SIZES), n


def test_mirrors_of_the_reference_structs():
    refapi.lib()                                           # (asserts the struct sizes against refshim_sizes)
    c = refapi.RefChain(); c.w = 5; c.kept = 3; c.is_alt = 1; c.rid = 9
    a = np.frombuffer(bytes(c), dtype=refapi.REF_CHAIN_DTYPE)
    assert int(a["wbits"][0]) == 5 | 3 << 29 | 1 << 31 and int(a["rid"][0]) == 9
    assert sc.SORT_KEY_DTYPE == SORT_KEY_DTYPE


# ---- expected orders from the compiled reference ---------------------------------------------------------------------------------------------------------
def ref_order(cls, k):
    """The case's records in the reference's struct for order `cls`, sorted by the reference -> (perm or None, sorted key columns)."""
    L = refapi.lib()
    n = k.shape[0]
    idx = np.arange(n)
    if cls == "u64":
        a = ((k["b"].astype(np.int64) << 32).astype(np.uint64)) | idx.astype(np.uint64)
        a = np.ascontiguousarray(a)
        L.ks_introsort_64(n, a.ctypes.data)
        return (a & np.uint64(0xffffffff)).astype(np.int64), None
    if cls == "u64raw":
        a = np.ascontiguousarray(k["a"].astype(np.uint64))
        L.ks_introsort_64(n, a.ctypes.data)
        return None, a
    if cls == "pair":
        a = np.zeros(n, dtype=refapi.REF_PAIR64_DTYPE)
        a["x"] = k["a"].astype(np.uint64)
        a["y"] = (k["b"].astype(np.uint32).astype(np.uint64) << np.uint64(32)) | k["c"].astype(np.uint32).astype(np.uint64)
        L.ks_introsort_128(n, a.ctypes.data)
        return None, a
    if cls == "intv":
        a = np.zeros(n, dtype=INTV_DTYPE)
        a["info"] = k["a"].astype(np.uint64); a["x0"] = idx
        L.ks_introsort_mem_intv(n, a.ctypes.data)
        return a["x0"].astype(np.int64), a["info"].copy()
    if cls == "chainw":
        assert n == 0 or (0 <= int(k["b"].min()) and int(k["b"].max()) < 1 << 29)
        a = np.zeros(n, dtype=refapi.REF_CHAIN_DTYPE)
        a["wbits"] = k["b"].astype(np.uint32); a["rid"] = idx
        L.ks_introsort_mem_flt(n, a.ctypes.data)
        return a["rid"].astype(np.int64), None
    a = np.zeros(n, dtype=ALNREG_DTYPE)
    a["seedlen0"] = idx; a["score"] = k["b"]
    if cls in ("hash", "hash2"):
        a["ncomp_isalt"] = (k["c"].astype(np.uint32) & np.uint32(1)) << np.uint32(30); a["hash"] = k["a"].astype(np.uint64)
    else:
        a["rb"] = k["a"]; a["re"] = k["a"]; a["qb"] = k["c"]
    {"end": L.ks_introsort_mem_ars2, "best": L.ks_introsort_mem_ars, "hash": L.ks_introsort_mem_ars_hash, "hash2": L.ks_introsort_mem_ars_hash2}[cls](n, a.ctypes.data)
    return a["seedlen0"].astype(np.int64), None


class Tally:
    """compared + expected declines == generated, every family took part and every mode of key_records was used"""

    def __init__(self):
        self.generated = self.compared = self.declined = 0
        self.fams = {}
        self.modes = {}
        self.comb = self.rule11 = self.ties_in_comb = 0

    def add(self, recs):
        self.generated += len(recs)

    def done(self, case):
        self.fams[case.family] = self.fams.get(case.family, 0) + 1
        if case.stat:
            assert case.stat["comb"] > 0
            self.comb += 1; self.rule11 += case.stat["rule11"] > 0; self.ties_in_comb += case.stat["ties_in_comb"] > 0

    def check(self, families, depth=True):
        assert self.compared + self.declined == self.generated, (self.compared, self.declined, self.generated)
        for cls, used in self.modes.items():
            assert used == set(range(sc.N_MODES[cls])), f"key_records modes used for {cls}: {sorted(used)}"
        missing = [f for f in families if not self.fams.get(f)]
        assert not missing, f"families without a case: {missing}"
        if depth:
            assert self.comb > 0 and self.comb == self.fams["depth"] + self.fams["depth_tied"], "a depth-limit case did not enter the comb sort in the model"
            assert self.rule11 > 0 and self.ties_in_comb > 0, (self.rule11, self.ties_in_comb)


def check_cases(name, cls, recs, perm, status, off, tally, exact=lambda n: True, declines=False, sizes=()):
    """perm / status of one bwagpu_debug_sort (or host) call -- one setting of a kind's switches -- against the reference, case by case; every size in
    `sizes` has to be among the cases compared."""
    tally.add(recs)
    seen = set()
    for i, (case, k) in enumerate(recs):
        n = k.shape[0]
        if case.special is None and n > 1:
            tally.modes.setdefault(cls, set()).add(case.mode % sc.N_MODES[cls])
        got = perm[off[i]:off[i + 1]].astype(np.int64)
        what = f"{name}: case {i} ({case.family}, n = {n})"
        if declines and case.decline:
            assert status[i] == 1, f"{what}: status {status[i]}, expected the routine to decline"
            assert (got == -1).all(), f"{what}: declined, but wrote {got.tolist()}"
            tally.declined += 1; tally.done(case); seen.add(n)
            continue
        assert status is None or status[i] == 0, f"{what}: status {status[i]}"
        exp, exp_keys = ref_order(cls, k)
        assert np.array_equal(np.sort(got), np.arange(n)), f"{what}: not a permutation: {got.tolist()}"
        if exact(n):
            assert np.array_equal(got, exp), f"{what}: order differs from the reference's ks_introsort\n device {got.tolist()}\n reference {exp.tolist()}\n keys {k.tolist()}"
        else:
            col = "a" if cls == "intv" else "b"
            assert np.array_equal(k[col][got], k[col][exp]), f"{what}: key sequence differs from the reference's\n device {k[col][got].tolist()}\n reference {k[col][exp].tolist()}"
        tally.compared += 1; tally.done(case); seen.add(n)
    missing = sorted(set(sizes) - seen)
    assert not missing, f"{name}: no case of size {missing}"


GENERIC = sc.FAMILIES


def run_device(dev, kind, thin, reps, seed):
    """thin > 1 (the mock runtime, where a wave's step is 64 fiber switches): every thin-th cell of families x sizes, one tied variant per depth-limit size,
    and the secondary settings of a kind's switches thinner again (one family per size) -- every size runs in every setting, which check_cases asserts, and
    every family for every kind."""
    check_limits(dev)
    t = Tally()
    lite = thin > 1
    mt = 1 if lite else 3
    if kind in (K_U64, K_CHAIN_SEEDS):
        # (the keys score << 32 | index are distinct, so whatever sorts them must give the reference's permutation -- wave_sort_u64 above 32 seeds included)
        recs = sc.build("u64", seed, thin, reps, max_tied=mt)
        keys, off = sc.flatten(recs)
        perm, st = dev.debug_sort(kind, keys, off)
        check_cases(f"kind {kind}", "u64", recs, perm, st, off, t, sizes=sc.requested_sizes())
        t.check(GENERIC)
    elif kind in (K_INTV, K_INTV_BLK):
        # one lane's introsort: the reference's permutation; the workgroup's network (2 .. PUB_MAX intervals): the reference's key sequence
        recs = sc.build("intv", seed, thin, reps, extra_sizes=(PUB_MAX - 1, PUB_MAX, PUB_MAX + 1), extra_depth=(PUB_MAX, PUB_MAX + 1), max_tied=mt)
        keys, off = sc.flatten(recs)
        perm, st = dev.debug_sort(kind, keys, off)
        check_cases(f"kind {kind}", "intv", recs, perm, st, off, t, exact=(lambda n: True) if kind == K_INTV else (lambda n: n > PUB_MAX),
                    sizes=sc.requested_sizes(sc.SIZES + (PUB_MAX - 1, PUB_MAX, PUB_MAX + 1), sc.DEPTH_SIZES + (PUB_MAX, PUB_MAX + 1)))
        t.check(GENERIC)
    elif kind == K_CHAIN_W:
        for flt in (CW_FLT_LDS, 16, 0):                     # the pairs and the sorted order in LDS; the order in HBM from 17 chains on; everything in HBM
            main = flt == CW_FLT_LDS
            recs = sc.build("chainw", seed + flt, thin if main else 3 * thin, reps, extra_sizes=(CW_PW_LDS - 1, CW_PW_LDS, CW_PW_LDS + 1),
                            extra_depth=(CW_PW_LDS, CW_PW_LDS + 1) if main or not lite else (), max_tied=mt)
            keys, off = sc.flatten(recs)
            perm, st = dev.debug_sort(kind, keys, off, chain_flt_lds=flt)
            check_cases(f"kind {kind} chain_flt_lds {flt}", "chainw", recs, perm, st, off, t, sizes=sc.requested_sizes(sc.SIZES + (CW_PW_LDS - 1, CW_PW_LDS, CW_PW_LDS + 1)))
        t.check(GENERIC)
    elif kind in (K_REG_END, K_REG_BEST):
        cls = "end" if kind == K_REG_END else "best"
        recs = sc.build(cls, seed, thin, reps, boundary=120, max_tied=mt)
        keys, off = sc.flatten(recs)
        perm, st = dev.debug_sort(kind, keys, off)
        check_cases(f"kind {kind}", cls, recs, perm, st, off, t, sizes=sc.requested_sizes())          # (full-width keys: nothing is declined here)
        t.check(GENERIC + (("end_edges",) if cls == "end" else ("best_boundary", "best_decline")))
    else:
        cls = "end" if kind == K_PAR_END else "best"
        # (dd_net, par_cap): counting only; the network from 16 and from the default 129 elements on; LDS arrays that hold N = 1024 but not 2048 (1025 elements
        # finish by counting), and arrays of 600 that do not hold 1024 (513 .. 600 finish by counting)
        for dd_net, par_cap in ((0, PAR_CAP_MAX), (16, PAR_CAP_MAX), (DD_NET_DEFAULT, PAR_CAP_MAX), (DD_NET_DEFAULT, 600), (DD_NET_DEFAULT, 128)):
            full = par_cap == PAR_CAP_MAX
            sizes = tuple(n for n in sc.SIZES if n <= par_cap) + (par_cap - 1, par_cap)
            depth = tuple(n for n in sc.DEPTH_SIZES if n <= par_cap) + ((par_cap,) if par_cap > 100 else ())
            main = full and dd_net == 0
            rc = sc.rank_cases(seed + dd_net + par_cap, sizes, depth, thin if main else 3 * thin, reps, mt)
            recs = [(c, sc.key_records(cls, c.ranks, mode=c.mode)) for c in rc]
            if cls == "best":
                recs += [(c, c.special) for c in sc.best_boundary_cases(seed + dd_net, 120 if full else 30)]
            else:
                recs += sc.end_edge_cases(seed)
            recs = [r for r in recs if r[1].shape[0] <= par_cap]
            keys, off = sc.flatten(recs)
            perm, st = dev.debug_sort(kind, keys, off, dd_net=dd_net, par_cap=par_cap)
            check_cases(f"kind {kind} dd_net {dd_net} par_cap {par_cap}", cls, recs, perm, st, off, t, declines=True, sizes=sc.requested_sizes(sizes, depth))
        # beyond the LDS arrays the entry says so (k_dedup_wave sorts such a read in place)
        k = sc.key_records(cls, list(range(130)))
        perm, st = dev.debug_sort(kind, k, np.array([0, 130]), dd_net=129, par_cap=128)
        assert st[0] == -2 and (perm == -1).all()
        t.check(GENERIC + (("end_edges",) if cls == "end" else ("best_boundary", "best_decline")))
        if cls == "best":
            assert t.declined > 0
    return t


# ---- mock runtime ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim():
    import hostsim_build
    prefix, _ = testdata.small_index()
    s = BwaGpu(prefix, lib_path=hostsim_build.build())
    yield s
    s.close()


SIM_THIN = 7


def test_sim_sort_u64(sim):
    run_device(sim, K_U64, SIM_THIN, 1, 101)


def test_sim_sort_chain_seeds(sim):
    run_device(sim, K_CHAIN_SEEDS, SIM_THIN, 1, 102)


def test_sim_sort_intervals(sim):
    run_device(sim, K_INTV, SIM_THIN, 1, 103)


def test_sim_sort_intervals_blk(sim):
    run_device(sim, K_INTV_BLK, SIM_THIN, 1, 104)


def test_sim_sort_chain_weights(sim):
    run_device(sim, K_CHAIN_W, SIM_THIN, 1, 105)


def test_sim_sort_regs_end(sim):
    run_device(sim, K_REG_END, SIM_THIN, 1, 106)


def test_sim_sort_regs_best(sim):
    run_device(sim, K_REG_BEST, SIM_THIN, 1, 107)


def test_sim_sort_par_end(sim):
    run_device(sim, K_PAR_END, SIM_THIN, 1, 108)


def test_sim_sort_par_best(sim):
    run_device(sim, K_PAR_BEST, SIM_THIN, 1, 109)


def test_debug_sort_rejects_bad_arguments(sim):
    k = sc.key_records("end", [1, 0])
    with pytest.raises(Exception):
        sim.debug_sort(99, k, np.array([0, 2]))
    with pytest.raises(Exception):
        sim.debug_sort(K_PAR_END, k, np.array([0, 2]), par_cap=PAR_CAP_MAX + 1)
    perm, st = sim.debug_sort(K_PAR_END, k, np.array([0, 2]))
    assert perm.tolist() == [1, 0] and st.tolist() == [0]


# ---- host ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_host_sort_fuzz():
    """hostmem::introsort (host_sort.h) with HashLess, HashLess2, U64Less, Pair64Less, RegEndLess, RegBestLess."""
    import hostapi
    for kind, cls in enumerate(("hash", "hash2", "u64raw", "pair", "end", "best")):
        t = Tally()
        recs = sc.build(cls, 200 + kind, 1, 1, extra_sizes=(4097,), extra_depth=(4096,), boundary=120)
        keys, off = sc.flatten(recs)
        out, perm = hostapi.debug_sort(kind, keys, off)
        if cls in ("u64raw", "pair"):                      # bare numbers: the sorted sequence
            t.add(recs)
            for i, (case, k) in enumerate(recs):
                _, exp = ref_order(cls, k)
                got = out[off[i]:off[i + 1]]
                if cls == "u64raw":
                    assert np.array_equal(got["a"].astype(np.uint64), exp), f"host kind {kind} case {i} ({case.family}, n = {k.shape[0]})"
                else:
                    assert np.array_equal(got["a"].astype(np.uint64), exp["x"]) and np.array_equal(got["b"].astype(np.uint32), (exp["y"] >> np.uint64(32)).astype(np.uint32)) \
                        and np.array_equal(got["c"].astype(np.uint32), exp["y"].astype(np.uint32)), f"host kind {kind} case {i} ({case.family}, n = {k.shape[0]})"
                t.compared += 1; t.done(case)
        else:
            check_cases(f"host kind {kind}", cls, recs, perm, None, off, t, sizes=sc.requested_sizes(sc.SIZES + (4097,), sc.DEPTH_SIZES + (4096,)))
        t.check(GENERIC + {"end": ("end_edges",), "best": ("best_boundary", "best_decline")}.get(cls, ()))


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    prefix, _ = testdata.small_index()
    g = BwaGpu(prefix)
    yield g
    g.close()


@pytest.mark.gpu
def test_gpu_sort_u64(gpu):
    run_device(gpu, K_U64, 1, 4, 301)


@pytest.mark.gpu
def test_gpu_sort_chain_seeds(gpu):
    run_device(gpu, K_CHAIN_SEEDS, 1, 4, 302)


@pytest.mark.gpu
def test_gpu_sort_intervals(gpu):
    run_device(gpu, K_INTV, 1, 4, 303)


@pytest.mark.gpu
def test_gpu_sort_intervals_blk(gpu):
    run_device(gpu, K_INTV_BLK, 1, 4, 304)


@pytest.mark.gpu
def test_gpu_sort_chain_weights(gpu):
    run_device(gpu, K_CHAIN_W, 1, 2, 305)


@pytest.mark.gpu
def test_gpu_sort_regs_end(gpu):
    run_device(gpu, K_REG_END, 1, 4, 306)


@pytest.mark.gpu
def test_gpu_sort_regs_best(gpu):
    run_device(gpu, K_REG_BEST, 1, 4, 307)


@pytest.mark.gpu
def test_gpu_sort_par_end(gpu):
    run_device(gpu, K_PAR_END, 1, 1, 308)


@pytest.mark.gpu
def test_gpu_sort_par_best(gpu):
    run_device(gpu, K_PAR_BEST, 1, 1, 309)
