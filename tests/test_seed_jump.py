"""Option seed_jump of the seeding stage (bwa_amd/csrc/dev_seed.h): a sweep's steps below the prefix tables' depth m answered from ONE table entry -- its
interval and its change bits (k_ptab_records: bit k-1 of the j-base prefix's entry = the (k+1)-base prefix has another interval size than the k-base one).
Bit 1: forward sweeps of k_seed and the walks of k_seed3 enter at depth m; bit 2: a backward row's short entries are decided from the look-up of the
longest of them.  Every case runs under seed_jump = 0, 1, 2 and 3 and must give mem_collect_intv's list: truth is refapi.RefIndex.intervals(opt, read),
compared in x0, x2, info and order (the World, the genome and the replay are those of tests/test_seed_stage.py and tests/seed_cases.py).

 * families 1, 2, 3, 4, 5 and 7 of seed_cases under tables of depth 10 and 7, both index layouts, seed_mrg 2 and 0;
 * crafted reads (crafted(m), a few dozen per depth m = 10 and 7) under -k m - 1, m, m + 1 and 19 (k_seed3 enters at depth m up to -k m; the bit mask of short
   matches, and with it k_seed's fast paths, is on from -k m + 1): a search that starts at len - m - 1, len - m and len - m + 1 (behind an N); an N at window
   bases 0, m - 1 and m; random bases (windows absent from the genome; rows whose longest short entry dies);
 * pass 2 on tables of depth 4 (pass2_reads: -k 5 -r 1 -y 1000): re-seeding searches whose min_intv lies below and above the count of the 4-mer they start on;
 * cover(): counted from the replay (events(): the device's short-entry bookkeeping restated over seed_cases.Occ), before any device run: forward jumps taken and
   fallen back from, backward rows decided at once and rows whose longest short entry dies, for every depth; a condition on the inputs, not a measurement;
 * counters: the same batch counts strictly fewer table look-ups (stats()["n_tab_lookups"]) under seed_jump = 3 than under 0 and as many index blocks;
 * the tables: every entry's change bits recomputed in numpy from the sizes of the record's own prefixes (bwagpu_debug_ptab), for depth 4 and 7.

The 4-mers of this genome occur 150 times and more while a pass-1 match of five or more bases that is frequent enough to put min_intv above that exists only
inside the tandem arrays, so at depth 4 "just above / just below" is as close as those arrays allow: pass2_reads() searches them for the nearest cases (a
jump with 29 occurrences to spare, a fall-back 14 short), and cover() asserts both signs (and those distances, with some room).  The comparison itself is met
at equality and one below on the deeper tables: crafted(m) picks stretches of the n-copy segments whose middle window occurs n times (pass 2 asks for n + 1: it
falls back) or n + 1 times (it jumps; depth 7 only -- a chance tenth base elsewhere is too rare), and pass 1's windows occur once and not at all.

Measured, seconds on the mock runtime / on an MI355X: coverage 0.3 / 0.1, a family under one value of seed_jump 0.1 - 2.0 / 0.02 - 0.37, crafted 0.2 - 3.3 / < 0.1,
pass 2 1.1 - 2.1 / < 0.1, counters 5.9 / 0.12, a table 0.01 - 0.24.

CPU: the mock runtime takes each batch's `sim` reads under one form per value of seed_jump (rotating over the forms); -m gpu: every read under every form."""
import ctypes as C
import functools

import numpy as np
import pytest

import refapi
import seed_cases as X
import testdata
import test_seed_stage as S

JUMPS = (0, 1, 2, 3)
FAMILIES = (1, 2, 3, 4, 5, 7)
FORMS = [(dict(ptab_m=m, occ32=o), dict(seed_mrg=g)) for m in (10, 7) for o in (1, 0) for g in (2, 0)]


# ---- what the fast paths will meet, from the replay's occurrence counts ------------------------------------------------------------------------------------------
def events(q, opt, m, trace, occ):
    """-> dict: fw_jump / fw_fall (forward sweeps entered at depth m / restarted step by step), bw_jump / bw_fall (backward rows with two or more short entries
    decided from one look-up / whose longest short entry dies), margins (min_intv - count of the window, for the sweeps of pass 2)"""
    ev = dict(fw_jump=0, fw_fall=0, bw_jump=0, bw_fall=0, margins=[], margins1=[])
    if m < 2 or opt.min_seed_len <= m:      # (no bit mask of short matches)
        return ev
    n = q.shape[0]
    for sw in trace.sweeps:
        x, min_intv = sw.x, max(sw.min_intv, 1)
        if q[x] > 3:
            continue
        if x + m <= n and (q[x:x + m] < 4).all():
            cnt = occ(x, x + m)
            ev["fw_jump" if cnt >= min_intv else "fw_fall"] += 1
            ev["margins" if sw.pass_ == 2 else "margins1"].append(min_intv - cnt)
        # the forward sweep's change points (bwt.c:304-320), then the rows
        curr, ik, end, i = [], occ(x, x + 1), x + 1, x + 1
        while i < n:
            if q[i] > 3:
                curr.append((end, ik))
                break
            ok = occ(x, i + 1)
            if ok != ik:
                curr.append((end, ik))
                if ok < min_intv:
                    break
            ik, end = ok, i + 1
            i += 1
        if i == n:
            curr.append((end, ik))
        prev = curr[::-1]
        for i in range(x - 1, -1, -1):
            if q[i] > 3:
                break
            shorts = [e for e, _ in prev if e - (i + 1) < m]
            if len(shorts) >= 2:
                ev["bw_jump" if occ(i, shorts[0]) >= min_intv else "bw_fall"] += 1
            curr = []
            for e, _ in prev:
                ok = occ(i, e)
                if ok >= min_intv and (not curr or ok != curr[-1][1]):
                    curr.append((e, ok))
            if not curr:
                break
            prev = curr
    return ev


# ---- crafted reads -------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def crafted(m):
    g, _, lay = X.genome()
    rng = X._rng(f"jump {m}")
    R = X.Reads()
    L = 48
    for j, d in enumerate((-1, 0, 1)):          # a search (and a walk of pass 3) that starts m + 1, m and m - 1 bases before the read's end
        for v in range(3):
            s = 150 + 211 * (3 * j + v)
            x = g[s:s + L].copy()
            x[L - m + d - 1] = 4
            R.add(X.rc(x) if v == 2 else x, f"{L} bases, N at {L - m + d - 1}: a search from len - {m - d}", both=v == 0)
    for j, d in enumerate((0, m - 1, m)):          # N inside and just behind the window of the search that starts at base 12
        for v in range(3):
            s = 2100 + 97 * (3 * j + v)
            x = g[s:s + L].copy()
            x[[11, 12 + d]] = 4
            R.add(x, f"{L} bases, N at 11 and at window base {d}")
    for j in range(4):          # reads that end inside the first window
        R.add(g[400 + 50 * j:400 + 50 * j + m - 1 + j], f"{m - 1 + j} bases")
    for j in range(14):         # random bases: windows the genome does not hold, rows whose longest short entry dies
        R.add(X.rnd(rng, 22 + 2 * j), f"{22 + 2 * j} random bases")
    for j in range(6):
        n = 90
        s = int(rng.integers(0, g.shape[0] - n))
        R.add(X.substitute(rng, g[s:s + n], rng.random(n) < 0.06), f"{n} bases at {s}, 6 %", both=j == 0)
    # pass 2 at its threshold: the last 28 .. 34 bases of an n-copy segment between bases no copy has there -- a pass-1 match with n occurrences, re-seeded from its
    # middle with min_intv = n + 1 -- picked so that the window there occurs n times (the jump falls back) or, by a chance occurrence elsewhere, n + 1 times (it is taken)
    T, found = X.text(), {0: [], 1: []}
    for c in (3, 4, 5, 6, 7, 8, 9, 10):
        s0 = lay.seg[c][1]
        for a in range(26, 33):
            x = np.concatenate([X.rnd(rng, 12), X.other(g[s0 + a - 1]), g[s0 + a:s0 + X.SEG], X.other(g[s0 + X.SEG]), X.rnd(rng, 12)])
            mid = (13 + 13 + X.SEG - a) >> 1
            extra = X.Occ(T, x)(mid, mid + m) - c
            if extra in found and len(found[extra]) < 3:
                found[extra].append(1)
                R.add(x, f"the {c}-copy segment from {a}: the window in the middle occurs {c + extra} times")
    return R.reads, R.tags


@functools.lru_cache(maxsize=None)
def pass2_reads():
    """tables of depth 4, -k 5 -r 1 -y 1000: pass 2 re-seeds every pass-1 match; inside the tandem arrays its min_intv reaches the 4-mers' counts"""
    g, _, lay = X.genome()
    rng = X._rng("jump pass 2")
    R = X.Reads()
    for p in (1, 2, 3):
        a = lay.array[p]
        for n in (5, 6, 7, 8, 9, 12):
            R.add(g[a + 20:a + 20 + n], f"period {p}: {n} bases of the array")
            R.add(np.concatenate([g[a + 30:a + 30 + n], X.rnd(rng, 6)]), f"period {p}: {n} bases of the array, then 6 random")
            R.add(np.concatenate([X.rnd(rng, 5), g[a + 40:a + 40 + n]]), f"period {p}: 5 random bases, then {n} of the array")
    for j in range(10):
        R.add(X.rnd(rng, 30), "30 random bases")
    # ... and the closest this genome has: n bases of an array from the read's first base, then a base after which the match occurs nowhere (a pass-1 match
    # of exactly n bases), two more and a fixed tail; pass 2 starts at base n / 2 with min_intv = the piece's count + 1, on a window that reaches past the piece
    T, found = X.text(), []
    for p in X.PERIODS:
        a = lay.array[p]
        for n in (5, 6, 7, 8, 9):
            for ph in range(min(p, 4)):
                for xb in range(4):
                    for yb in (0, 3):
                        r = np.concatenate([g[a + 20 + ph:a + 20 + ph + n], [xb, yb, 1, 2, 3, 0]]).astype(np.uint8)
                        occ = X.Occ(T, r)
                        if occ(0, n + 1) == 0:
                            found.append((occ(0, n) + 1 - occ(n >> 1, (n >> 1) + 4), len(found), r, f"period {p}: {n} bases of the array from {20 + ph}, then {xb}, {yb} and a tail"))
    jumps, falls = sorted(f for f in found if f[0] <= 0)[-4:], sorted(f for f in found if f[0] > 0)[:4]
    for margin, _, r, tag in jumps + falls:
        R.add(r, f"{tag} (min_intv - count {margin})")
    return R.reads, R.tags


K_OF = lambda m: (m - 1, m, m + 1, 19)


def crafted_opt(k):
    return X.seed_opt(k, split_factor=1.5 if k == 19 else 1.0)


P2_OPT = lambda: X.seed_opt(5, split_factor=1.0, split_width=1000, max_occ=4)      # (max_occ: few SA rows per interval for the stages behind the seeding)


def trace_of(W, opt, read):
    return W.trace_of(opt, read), W.occs[read.tobytes()]


def cover(W):
    tot = {}
    for m in (10, 7):
        opts = [crafted_opt(m + 1), crafted_opt(19)]
        ev = dict(fw_jump=0, fw_fall=0, bw_jump=0, bw_fall=0)
        m1, m2 = [], []
        for r in crafted(m)[0]:
            for opt in opts:
                if r.shape[0] == 0:
                    continue
                t, occ = trace_of(W, opt, r)
                e = events(r, opt, m, t, occ)
                for k in ev:
                    ev[k] += e[k]
                m1 += e["margins1"]; m2 += e["margins"]
        print(f"depth {m}, crafted reads: {ev}")
        assert min(ev.values()) >= 2, (m, ev)
        tot[m] = ev
    reads, _ = pass2_reads()
    opt = P2_OPT()
    ev = dict(fw_jump=0, fw_fall=0, bw_jump=0, bw_fall=0)
    margins = []
    for r in reads:
        t, occ = trace_of(W, opt, r)
        e = events(r, opt, 4, t, occ)
        for k in ev:
            ev[k] += e[k]
        margins += e["margins"]
    below, above = [-x for x in margins if x <= 0], [x for x in margins if x > 0]
    print(f"depth 4, pass 2: {ev}; window count - min_intv of the searches that jump: {sorted(below)[:6]} ...; min_intv - count of those that fall back: {sorted(above)[:6]} ...")
    assert len(below) >= 2 and len(above) >= 2 and min(below) <= 40 and min(above) <= 20, (sorted(below)[:4], sorted(above)[:4])
    assert ev["fw_jump"] >= 2 and ev["fw_fall"] >= 2, ev


# ---- the device side ---------------------------------------------------------------------------------------------------------------------------------------------
def run_reads(W, opt, reads, tags, index_opts, options, what, stats=False):
    dev = W.handle(index_opts)
    truth = [W.truth_of(opt, r) for r in reads]
    seqs, off = testdata.ragged(reads)
    old = {k: dev.get_option(k) for k in options}
    dev.set_taps(True); dev.set_stats(stats)
    try:
        for k, v in options.items():
            dev.set_option(k, v)
        dev.upload(seqs, off); dev.run(opt)
        dev.download()
        n_iv, iv = dev.tap_intervals()
        st = dev.stats()
    finally:
        dev.set_taps(False); dev.set_stats(False)
        for k, v in old.items():
            dev.set_option(k, v)
    bad, k = [], 0
    for i, want in enumerate(truth):
        got = iv[k:k + int(n_iv[i])]
        k += int(n_iv[i])
        if got.shape[0] != want.shape[0] or not all(np.array_equal(got[f], want[f]) for f in ("x0", "x2", "info")):
            n = min(got.shape[0], want.shape[0])
            first = next((j for j in range(n) if any(got[f][j] != want[f][j] for f in ("x0", "x2", "info"))), n)
            show = lambda a: (int(a["info"][first]) >> 32, int(a["info"][first]) & 0xffffffff, int(a["x0"][first]), int(a["x2"][first])) if first < a.shape[0] else None
            bad.append(f"read {i} ({tags[i]}): device {got.shape[0]} intervals, reference {want.shape[0]}; first difference at {first}: device (start, end, x0, x2) {show(got)}, reference {show(want)}")
    assert k == iv.shape[0]
    assert not bad, f"{what}, {index_opts}, {options}: {len(bad)} of {len(truth)} reads differ from mem_collect_intv:\n  " + "\n  ".join(bad[:8])
    return st


def forms_of(thin, turn):
    return [FORMS[turn % len(FORMS)]] if thin else FORMS


def run_family(W, fam, jump, thin):
    for bi, b in enumerate(bb for bb in X.batches().values() if bb.fam == fam):
        idx = b.sim if thin else list(range(len(b.reads)))
        if not idx:
            continue
        for index_opts, options in forms_of(thin, 3 * bi + 5 * jump + fam):
            run_reads(W, b.opt, [b.reads[i] for i in idx], [b.tags[i] for i in idx], index_opts, dict(options, seed_jump=jump), b.name)


def run_crafted(W, m, jump, thin):
    for mi in (m & 1,):
        reads, tags = crafted(m)
        if thin:
            reads, tags = reads[jump % 2::2], tags[jump % 2::2]
        for ki, k in enumerate(K_OF(m)):
            forms = [f for f in FORMS if f[0]["ptab_m"] == m]
            for index_opts, options in ([forms[(ki + jump + mi) % len(forms)]] if thin else forms):
                run_reads(W, crafted_opt(k), reads, tags, index_opts, dict(options, seed_jump=jump), f"crafted, depth {m}, -k {k}")


def run_pass2(W, jump, thin):
    reads, tags = pass2_reads()
    for o in (1, 0):
        for g in ((2, 0)[(jump + o) % 2:][:1] if thin else (2, 0)):
            run_reads(W, P2_OPT(), reads, tags, dict(ptab_m=4, occ32=o), dict(seed_mrg=g, seed_jump=jump), "pass 2 on tables of depth 4")


def check_counters(W):
    """the fast paths ran: fewer table look-ups, the same index blocks (no read is given up: a read redone by the task kernels would count its blocks twice)"""
    for name, index_opts in (("deep", {}), ("depth -k 11", {}), ("depth -k 8", dict(ptab_m=7))):
        b = X.batches()[name]
        st = {j: run_reads(W, b.opt, b.reads, b.tags, index_opts, dict(seed_jump=j, seed_budget=0), name, stats=True) for j in JUMPS}
        tab, blk = {j: st[j]["n_tab_lookups"] for j in JUMPS}, {j: st[j]["n_occ_blocks"] for j in JUMPS}
        print(f"{name}: table look-ups by seed_jump {tab}, index blocks {blk}")
        assert tab[3] < tab[0] and tab[1] < tab[0] and tab[2] < tab[0] and tab[3] < min(tab[1], tab[2]), (name, tab)
        assert len(set(blk.values())) == 1 and blk[0] > 0, (name, blk)


def check_table(W, m):
    """every entry's change bits from the sizes of the record's own prefixes"""
    dev = W.handle(dict(ptab_m=m))
    dev.L.bwagpu_debug_ptab.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    depth, nbytes = C.c_int32(), C.c_uint64()
    assert dev.L.bwagpu_debug_ptab(dev.h, C.byref(depth), C.byref(nbytes), None) == 0
    assert depth.value == m and nbytes.value == 16 * m * 4 ** m
    rec = np.zeros((4 ** m, m, 4), dtype=np.uint32)
    assert dev.L.bwagpu_debug_ptab(dev.h, C.byref(depth), C.byref(nbytes), rec.ctypes.data) == 0
    x2 = ((rec[:, :, 3].astype(np.int64) >> 10) & 31) << 32 | rec[:, :, 2].astype(np.int64)
    assert (x2[:, 1:] <= x2[:, :-1]).all() and x2[:, 0].min() > 0
    chg = (x2[:, 1:] != x2[:, :-1]).astype(np.int64) << np.arange(m - 1)          # [W][k - 1]: depth k + 1 against depth k
    want = np.concatenate([np.zeros((4 ** m, 1), dtype=np.int64), np.cumsum(chg, axis=1)], axis=1)
    got = rec[:, :, 3].astype(np.int64) >> 16
    assert np.array_equal(got, want), f"depth {m}: {int((got != want).sum())} entries with other change bits"
    assert (want[:, -1] == (1 << (m - 1)) - 1).any() and (m < 7 or (want[:, -1] != (1 << (m - 1)) - 1).any())      # (both values of a bit occur; every 4-mer is rarer than its prefixes)
    # records that share a prefix agree on it
    j = m // 2
    key = np.arange(4 ** m) >> (2 * (m - j))
    first = np.searchsorted(key, key)
    assert np.array_equal(rec[:, j - 1], rec[first, j - 1])


# ---- fixtures and tests ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    if not refapi.have_ref():      # (the CPU tests only: the GPU tests' fixture asserts instead)
        pytest.skip("oracle/_ref not built")
    import hostsim_build
    w = S.World(tmp_path_factory.mktemp("seedjump"), lib_path=hostsim_build.build())
    yield w
    w.close()


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    assert refapi.have_ref(), "oracle/_ref (the compiled reference) is missing on the GPU box"
    w = S.World(tmp_path_factory.mktemp("seedjump"))
    yield w
    w.close()


def test_reads_reach_the_fast_paths_and_their_fallbacks(sim):
    cover(sim)


@pytest.mark.parametrize("m", [4, 7])
def test_sim_table(sim, m):
    check_table(sim, m)


def test_sim_counters(sim):
    check_counters(sim)


@pytest.mark.parametrize("jump", JUMPS)
@pytest.mark.parametrize("fam", FAMILIES)
def test_sim_family(sim, fam, jump):
    run_family(sim, fam, jump, thin=True)


@pytest.mark.parametrize("jump", JUMPS)
@pytest.mark.parametrize("m", [10, 7])
def test_sim_crafted(sim, m, jump):
    run_crafted(sim, m, jump, thin=True)


@pytest.mark.parametrize("jump", JUMPS)
def test_sim_pass2(sim, jump):
    run_pass2(sim, jump, thin=True)


@pytest.mark.gpu
def test_gpu_reads_reach_the_fast_paths_and_their_fallbacks(gpu):
    cover(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [4, 7])
def test_gpu_table(gpu, m):
    check_table(gpu, m)


@pytest.mark.gpu
def test_gpu_counters(gpu):
    check_counters(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("jump", JUMPS)
@pytest.mark.parametrize("fam", FAMILIES)
def test_gpu_family(gpu, fam, jump):
    run_family(gpu, fam, jump, thin=False)


@pytest.mark.gpu
@pytest.mark.parametrize("jump", JUMPS)
@pytest.mark.parametrize("m", [10, 7])
def test_gpu_crafted(gpu, m, jump):
    run_crafted(gpu, m, jump, thin=False)


@pytest.mark.gpu
@pytest.mark.parametrize("jump", JUMPS)
def test_gpu_pass2(gpu, jump):
    run_pass2(gpu, jump, thin=False)
