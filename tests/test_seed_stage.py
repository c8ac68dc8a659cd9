"""The seeding stage of the device library -- mem_collect_intv (bwamem.c:140-188) as restated in bwa_amd/csrc/dev_seed.h (k_seed's state machine in all its forms,
k_seed3, k_seed_p2_tasks, k_publish, k_publish_blk) and chosen between in bwagpu_batch_run -- on crafted reads, against the compiled reference.

A case is a read under one option set.  Truth: refapi.RefIndex.intervals(opt, read), mem_collect_intv and the reference's own sort, compared in x0, x2 and info,
order included, with the read's slice of the device's tap_intervals, for every read of every batch under every form (FORMS).  The batch's slot count
(stats()["n_seeds"]) must be what mem_chain's bounds (bwamem.c:304-305) give for the reference's intervals; every batch's first form runs once more with
set_stats(True), which selects the counting instances of the kernels.  The batches of family 8 let chains through, and their chain tap must equal
ref.chains(opt, read, 2) in n, rbeg, qbeg and len: that holds the SA rows k_publish selects and k_sa resolves to the reference; a difference there with equal
intervals is reported as "publish / SA look-up".  All other batches run with min_chain_weight = 2^20, which leaves the later stages without work.

Genome and reads: tests/seed_cases.py (an 18.9 kb genome written and indexed into a temporary directory; eight families, 347 different reads, 1942 pairs of a read
and an option set).  cover() asserts from the replay alone -- seed_cases.replay, a restatement of mem_collect_intv over plain occurrence counts that must
reproduce the reference's (info, x2) list of every read -- that the reads reach the points where the device code changes form (bwagpu_seed_limits):
 1 lengths: every read length 0, 1, k - 1 .. k + 1, 15 .. 17, 31 .. 33, 255, 256; N at bases 0, 15, 16, 17 and the last; clean pieces of k - 1 and k bases;
   the palindrome, the strands' junction; batches whose longest read is 256 (2-bit LDS copy, its N reads byte by byte), 257 and 1100 (4-bit array).
 2 depth: change points at d - 1, d, d + 1 bases, backward rows that grow an entry to d and reads with no match of d bases, for d = 10 and d = 7;
   under ptab_m = 0 / 7 / 10, both index layouts, with and without the bit mask of short matches.
 3 deep: sweeps with <= 2, 6, 7, 10, 11 and >= 30 change points (and as many entries of at least d bases: what the stack holds when the mask is on).  The LDS
   ring holds lds_ent = 10 entries only where the read copy leaves room for them in a lane's 160 bytes: 6 in this batch's default form (its longest read has 221
   bases), 10 without the copy and in long-read batches, 2 by option; run_batch asserts the ring in force of every run (seed_limits()["lds_ent_run"]).
 4 split: pass-1 SMEMs of split_len - 1 .. split_len + 1 bases with x2 = split_width - 1 .. split_width + 1, re-seeded or not; qualifying entries at
   emission index 63, 64 and beyond (reads of 250 random bases under -k 7: up to 265 intervals).
 5 pass 3: bwt_seed_strategy1 deciding at x2 = max_mem_intv - 1, max_mem_intv, max_mem_intv + 1 for 5 and 20; k_seed3 and the inline form.
 6 heavy: every read of families 3 and 4 and reads aimed at the tasks' positions, under -k 19 -r 1.5 and -k 8 -r 1, with seed_budget = 16, 64, 256 (reads given up: asserted) and 0 (none), and a
   pass-2 task list of one entry (n_retries >= 1).
 7 long: families 1 and 3 with reads of 1300 and 1700 bases appended: tasks or the chain, tiny task stacks (second launch: asserted for every batch), either publish
   kernel (a read with more than 256 intervals), interval lists of 24 entries (n_retries >= 1).
 8 publish: x2 = 3, 4, 5, 7, 8, 9, 11, 12 under max_occ = 4 (step 1, 1, 1, 1, 2, 2, 2, 3) and the default.
What the replay counted is printed by cover() (run with -s).

The replay counted (cover() prints it): 14 reads with a backward row that grows an entry to 10 bases (42 to 7), 15 reads with no match of 10 bases (4 of 7); sweeps
of 6 / 7 / 10 / 11 / 30 or more change points in 5 / 21 / 8 / 4 / 22 reads of family 3 (of at least 10 bases: 5 / 3 / 6 / 9 / 16); 8 reads with a qualifying pass-1 entry at emission index
63, at 64 and past it (up to 104 pass-1 entries, 257 intervals a read).
Planted in dev_seed.h and run on the mock runtime, these fail: `len <= virt_m` in push_fw and `L.n0 > n_lds` in push (family 1, then the mock faults in
family 2), `x2 < split_width` in SeedEmit::add and in SS_PASS2 (families 2 and 4) and in k_seed_p2_tasks (family 6), `count <= opt.max_occ` in k_publish
(family 8), the task's L.lo one higher (families 6 and 7).  `n - base <= 64` in SeedEmit::add changes nothing that can be seen: the shift by 64 sets bit 0,
and SS_PASS2 tests again every entry whose bit is set, while entry 64 is read back from the list either way (a bit LOST, `< 63`, is what the reads with a
qualifying entry at index 63 are for).

CPU: on the mock runtime (tests/hostsim): every read of every batch through the batch's first form; through the other forms a subset only -- half of the
batch's `sim` list, which holds every 2nd to 9th read (family 7: all of `sim`, the long read among them) -- and family 2 leaves out the second handle with
tables of depth 10 and takes its last eight forms on every third batch.  The counting repeat takes `sim`.  -m gpu: every read through every form.
Measured, seconds on the mock runtime / on an MI355X: coverage 1.5 / 0.8; families 1: 2.6 / 0.16, 2: 5.6 / 0.29, 3: 1.2 / 0.11, 4: 4.5 / 0.15, 5: 0.4 / 0.03,
6: 4.4 / 0.31, 7: 8.9 / 0.46, 8: 3.2 / 0.03 (the extension module's: coverage 1.3 -- 0.2 s less than this module's, which replays every read --, families
5.9 .. 28.4 on the mock runtime)."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import refapi
import seed_cases as X
import testdata
from bwa_amd import simdata
from bwa_amd.api import BwaGpu

LIMITS = dict(ptab_max=12, ptab_depth=10, lds_ent=10, rd_lds_max_len=256, wave_max_len=1100, cand_bits=64, pub_max=4096, task_stack_cap=140, lane_lds=160)
D7 = 7      # the depth of the second set of prefix tables (option ptab_m)

# family -> (form name, options of the index (a handle of their own), options of the batch).  A form named "fresh ..." gets a handle of its own that is closed again.
INDEX_FORMS = [(f"ptab_m {m}, occ32 {o}", dict(ptab_m=m, occ32=o)) for m in (10, 7, 0) for o in (1, 0)]
FORMS = {
    1: [("default", {}, {}), ("no read copy", {}, dict(seed_rd_lds=0)), ("loads as compiled", {}, dict(seed_mrg=0))],
    2: [(f"{n}, seed_no_virt {v}", ix, dict(seed_no_virt=v)) for n, ix in INDEX_FORMS for v in (0, 1)],
    3: [(f"lds_ent {e}, mrg {m}, rd_lds {r}", {}, dict(seed_lds_ent=e, seed_mrg=m, seed_rd_lds=r)) for e in (-1, 2) for m in (2, 0) for r in (1, 0)],
    4: [("default", {}, {}), ("loads as compiled", {}, dict(seed_mrg=0)), ("never given up", {}, dict(seed_budget=0))],
    5: [("k_seed3", {}, dict(seed_pass3_inline=0)), ("inline", {}, dict(seed_pass3_inline=1)), ("inline, loads as compiled", {}, dict(seed_pass3_inline=1, seed_mrg=0))],
    6: [("budget 16", {}, dict(seed_budget=16)), ("budget 64", {}, dict(seed_budget=64)), ("budget 256", {}, dict(seed_budget=256)), ("budget 0", {}, dict(seed_budget=0)),
        ("budget 64, lds_ent 2", {}, dict(seed_budget=64, seed_lds_ent=2)), ("fresh: budget 64, pass-2 list of 1", {}, dict(seed_budget=64, seed_p2_cap=1))],
    7: [("default", {}, {}), ("chain", {}, dict(seed_tasks=0)), ("chain, loads as compiled", {}, dict(seed_tasks=0, seed_mrg=0)), ("task stacks of 2", {}, dict(seed_task_stack=2)),
        ("task stacks of 2, lds_ent 3", {}, dict(seed_task_stack=2, seed_lds_ent=3)), ("publish by lane", {}, dict(publish_blk=0)), ("chain, publish by lane", {}, dict(seed_tasks=0, publish_blk=0)),
        ("fresh: lists of 24", {}, dict(mem_cap=24))],
    8: [("default", {}, {}), ("never given up", {}, dict(seed_budget=0))],
}


def check_limits(dev):
    got = dev.seed_limits()
    got.pop("lds_ent_run")
    assert got == LIMITS, "a switch point moved: aim the cases at it"


def ring(max_len, rd_lds=True):
    """interval-stack entries per lane in LDS for a batch whose longest read has max_len bases: what the 2-bit read copy (short-read batches: 16 bytes per 64 bases,
    in steps of 16 bytes) leaves of a lane's LDS, lds_ent at the most"""
    if max_len > LIMITS["rd_lds_max_len"] or not rd_lds:
        return LIMITS["lds_ent"]
    rd_words = ((max_len + 15) // 16 + 3) & ~3
    return min(LIMITS["lds_ent"], (LIMITS["lane_lds"] - 4 * rd_words) // 16)


def opt_key(opt):
    return (opt.min_seed_len, round(opt.split_factor * 1000), opt.split_width, opt.max_mem_intv)


class World:
    def __init__(self, d, lib_path=None):
        self.g, self.lens, self.lay = X.genome()
        self.fa = os.path.join(str(d), "seed.fa")
        simdata.write_fasta(self.fa, self.g, self.lens)
        refapi.build_index(self.fa)
        self.lib_path = lib_path
        self.devs = {}
        self.dev = self.handle({})
        self.ref = refapi.RefIndex(self.fa)
        assert self.ref.l_pac == self.g.shape[0] < 20000
        self.truth, self.chain_truth, self.traces, self.occs = {}, {}, {}, {}

    def handle(self, index_opts, fresh=False):
        key = tuple(sorted(index_opts.items()))
        if fresh or key not in self.devs:
            dev = BwaGpu(self.fa, lib_path=self.lib_path, options=dict(index_opts))
            dev.L.bwagpu_debug_prof.argtypes = [C.c_void_p, C.c_void_p]
            if fresh:
                return dev
            self.devs[key] = dev
        return self.devs[key]

    def close(self):
        for d in self.devs.values():
            d.close()
        self.ref.close()

    def truth_of(self, opt, read):
        """the reference's intervals of one read under one option set: computed once, shared and left alone"""
        key = (opt_key(opt), read.tobytes())
        if key not in self.truth:
            self.truth[key] = self.ref.intervals(opt, read)
        return self.truth[key]

    def chains_of(self, opt, read):
        key = (opt_key(opt), opt.max_occ, read.tobytes())
        if key not in self.chain_truth:
            self.chain_truth[key] = self.ref.chains(opt, read, 2)
        return self.chain_truth[key]

    def trace_of(self, opt, read):
        """the replay of one read, validated against the reference's list"""
        key = (opt_key(opt), read.tobytes())
        if key not in self.traces:
            want = self.truth_of(opt, read)
            if key[1] not in self.occs:      # (the occurrence counts of a read's substrings serve all its option sets)
                self.occs[key[1]] = X.Occ(X.text(), read)
            t = X.replay(opt, read, self.occs[key[1]])
            assert t.intv == sorted(zip(want["info"].tolist(), want["x2"].tolist())), "the replay does not reproduce mem_collect_intv"
            self.traces[key] = t
        return self.traces[key]


def n_slots(opt, iv):
    """mem_chain's k-loop bounds (bwamem.c:304-305) over a read's intervals"""
    n = 0
    for x2 in iv["x2"].tolist():
        step = x2 // opt.max_occ if x2 > opt.max_occ else 1
        n += min(opt.max_occ, -(-x2 // step))
    return n


# ---- what the reference did on the reads -------------------------------------------------------------------------------------------------------------------------
def cover(W):
    """the points the families are aimed at, from the replay alone (coverage conditions, not tolerances)"""
    B = X.batches()
    d, ent, bits = LIMITS["ptab_depth"], LIMITS["lds_ent"], LIMITS["cand_bits"]
    fam = lambda f: [b for b in B.values() if b.fam == f]
    traces = lambda b: [W.trace_of(b.opt, r) for r in b.reads]
    for b in B.values():      # every read of every batch: the replay is a validated classifier
        traces(b)
    # 1: lengths, N positions, pieces between N runs, the batches' longest reads
    b1 = B["lengths -k 19"]
    lens = {r.shape[0] for r in b1.reads}
    assert set(X.F1_LENGTHS) <= lens and {k + e for k in (10, 11, 19) for e in (-1, 0, 1)} <= lens, sorted(lens)
    for p in (0, 15, 16, 17):
        assert sum(r.shape[0] > p and r[p] == 4 and (r < 4).any() for r in b1.reads) >= 2, p
    assert sum(r.shape[0] > 0 and r[-1] == 4 and (r < 4).any() for r in b1.reads) >= 2 and sum(r.shape[0] > 0 and (r == 4).all() for r in b1.reads) >= 2
    for k in (10, 11, 19):
        pieces = set()
        for r in B[f"lengths -k {k}"].reads:
            if (r == 4).any():
                pieces |= {len(p) for p in bytes(np.where(r < 4, 65, 78).astype(np.uint8)).split(b"N")}
        assert {k - 1, k} <= pieces, (k, sorted(pieces))
    longest = {name: max(r.shape[0] for r in b.reads) for name, b in B.items()}
    assert {longest[b.name] for b in fam(1)} == {LIMITS["rd_lds_max_len"], LIMITS["rd_lds_max_len"] + 1, LIMITS["wave_max_len"]}
    assert all(longest[b.name] <= LIMITS["rd_lds_max_len"] for f in (2, 3, 4, 5, 6, 8) for b in fam(f)) and all(longest[b.name] > LIMITS["wave_max_len"] for b in fam(7))
    wave = b1.reads[:64]      # reads with N and clean reads in one wavefront
    assert 8 <= sum((r == 4).any() for r in wave) <= 40
    # 2: match lengths around the prefix tables' depth, for both depths
    for dd, name in ((d, "depth -k 11"), (D7, "depth -k 8")):
        T = traces(B[name])
        for ln in (dd - 1, dd, dd + 1):
            assert sum(any(ln in s.lens for s in t.sweeps) for t in T) >= 2, (dd, ln)
        grow = sum(any(dd in s.grown and dd - 1 in s.lens for s in t.sweeps) for t in T)      # an entry of d - 1 bases at a change point, d after a backward row
        short = sum(bool(t.sweeps) and all(max(s.lens, default=0) < dd for s in t.sweeps) for t in T)
        print(f"depth {dd}: {grow} reads with a backward row that grows an entry to {dd} bases, {short} reads with no match of {dd} bases")
        assert grow >= 2 and short >= 2, (dd, grow, short)
    # 3: change points per sweep against the LDS ring
    T = traces(B["deep"])
    ent_rd = ring(longest["deep"])      # the ring of the batch's default form: its reads' LDS copy takes 64 of a lane's 160 bytes
    assert ent_rd == 6
    for what, count in (("change points", lambda s: len(s.lens)), (f"change points of at least {d} bases", lambda s: sum(ln >= d for ln in s.lens))):
        n = {key: sum(any(f(count(s)) for s in t.sweeps) for t in T) for key, f in (("<= 2", lambda c: 1 <= c <= 2), (f"{ent_rd}", lambda c: c == ent_rd), (f"{ent_rd + 1}", lambda c: c == ent_rd + 1), (f"{ent}", lambda c: c == ent), (f"{ent + 1}", lambda c: c == ent + 1), (f">= {3 * ent}", lambda c: c >= 3 * ent))}
        print(f"deep: reads with a sweep of ... {what}: {n}")
        assert min(n.values()) >= 2, (what, n)
    # ... and backward rows that walk entries on both sides of the ring's border: a sweep with more entries than the ring and backward rows
    assert sum(any(sum(ln >= d for ln in s.lens) > ent and s.rows >= 2 for s in t.sweeps) for t in T) >= 2
    # 4: pass 2's thresholds
    for w, f in X.F4_SPLIT:
        b = B[f"split -y {w} -r {f}"]
        sl = int(19 * f + .499)
        seen = {}
        for t in traces(b):
            for s, e, x2, qual in t.p1:
                if (e - s, x2) in seen:
                    assert seen[(e - s, x2)] == qual
                seen[(e - s, x2)] = qual
        for ln in (sl - 1, sl, sl + 1):
            for x2 in (w - 1, w, w + 1):
                if ln >= 19:      # (shorter ones are never reported)
                    assert seen.get((ln, x2)) == (ln >= sl and x2 <= w), (w, f, ln, x2, seen.get((ln, x2)))
        assert f != 1.5 or all((ln, x2) in seen for ln in (sl - 1, sl, sl + 1) for x2 in (w - 1, w, w + 1))      # all nine
        # ... and the re-seeding shows: at the very thresholds pass 2 adds an interval (the 19 bases inside the segment that occur twice more)
        edge = sum(t.n_p2 > 0 and any(qual and x2 == w and e - s <= sl + 1 for s, e, x2, qual in t.p1) for t in traces(b))
        assert edge >= 2, (w, f, edge)
    T = traces(B["many -k 7"])
    at = {k: sum(len(t.p1) > k and t.p1[k][3] for t in T) for k in (bits - 1, bits)}
    past = sum(any(q[3] for q in t.p1[bits + 1:]) for t in T)
    first_not = sum(len(t.p1) > bits and t.p1[bits][3] and not t.p1[0][3] for t in T)
    print(f"many -k 7: reads with a qualifying pass-1 entry at emission index {bits - 1}: {at[bits - 1]}, at {bits}: {at[bits]}, past it: {past}; at {bits} with entry 0 not qualifying: {first_not}; "
          f"most pass-1 entries {max(len(t.p1) for t in T)}, most intervals {max(len(t.intv) for t in T)}")
    assert at[bits - 1] >= 2 and at[bits] >= 2 and past >= 2
    # 5: pass 3's decisions on both sides of max_mem_intv
    for m in (5, 20):
        seen = {}
        for t in traces(B[f"pass 3 -y {m}"]):
            for x2, hit in t.p3:
                seen.setdefault(x2, set()).add(hit)
        assert seen.get(m - 1) == {True} and seen.get(m) == {False} and seen.get(m + 1) == {False}, (m, {k: v for k, v in seen.items() if abs(k - m) < 3})
    assert not any(t.p3 for t in traces(B["pass 3 -y 0"]))
    # 6: matches that start on a pass-1 task's position g = 19 j and at the far end of its range, g - 19 + 1; N on and next to such positions
    bh = B["heavy"]
    starts = [{s % 19 for s, e, x2, qual in t.p1} for t in traces(bh)]
    assert sum(0 in x for x in starts) >= 2 and sum(1 in x for x in starts) >= 2
    n_at = {int(p) % 19 for r in bh.reads if (r < 4).any() for p in np.nonzero(r == 4)[0]}
    assert {18, 0, 1} <= n_at, sorted(n_at)
    # 7: a read that spans several of k_publish_blk's 256-lane strides, none beyond its LDS arrays
    most = max(len(t.intv) for t in traces(B["long, deep -k 8"]))
    assert 256 < most <= LIMITS["pub_max"], most
    # 8: the interval sizes of the SA-row expansion
    x2s = {x2 for t in traces(B["publish -c 4"]) for _, x2 in t.intv}
    assert set(X.F8_COPIES) <= x2s, sorted(x2s)
    n_pairs = sum(len(b.reads) for b in B.values())
    n_reads = len({r.tobytes() for b in B.values() for r in b.reads})
    print(f"{n_reads} different reads, {n_pairs} pairs of a read and an option set")
    assert n_reads == 347 and n_pairs == 1942, (n_reads, n_pairs)


# ---- the device side ---------------------------------------------------------------------------------------------------------------------------------------------
def run_batch(W, b, fname, index_opts, options, idx, stats=False):
    """one batch under one form -> (reads given up, pass-2 tasks, tasks redone by the second launch, retries)"""
    fresh = fname.startswith("fresh")
    dev = W.handle(index_opts, fresh)
    reads = [b.reads[i] for i in idx]
    tags = [b.tags[i] for i in idx]
    opt = b.opt
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
        if b.chains:
            cn, ch, cs = dev.tap_chains()
        st = dev.stats()
        ring_run = dev.seed_limits()["lds_ent_run"]
        prof = (C.c_ulonglong * 16)()
        dev.L.bwagpu_debug_prof(dev.h, prof)
    finally:
        if fresh:
            dev.close()
        else:
            dev.set_taps(False); dev.set_stats(False)
            for k, v in old.items():
                dev.set_option(k, v)
    what = f"{b.name}, form {fname}{', counting' if stats else ''}"
    bad = []
    k = 0
    for i, want in enumerate(truth):
        got = iv[k:k + int(n_iv[i])]
        k += int(n_iv[i])
        if got.shape[0] != want.shape[0] or not all(np.array_equal(got[f], want[f]) for f in ("x0", "x2", "info")):
            m = min(got.shape[0], want.shape[0])
            first = next((j for j in range(m) if any(got[f][j] != want[f][j] for f in ("x0", "x2", "info"))), m)
            show = lambda a: (int(a["info"][first]) >> 32, int(a["info"][first]) & 0xffffffff, int(a["x0"][first]), int(a["x2"][first])) if first < a.shape[0] else None
            bad.append(f"read {idx[i]} ({tags[i]}): device {got.shape[0]} intervals, reference {want.shape[0]}; first difference at {first}: device (start, end, x0, x2) {show(got)}, reference {show(want)}")
    assert k == iv.shape[0]
    assert not bad, f"{what}: {len(bad)} of {len(truth)} reads differ from mem_collect_intv:\n  " + "\n  ".join(bad[:8])
    want_slots = sum(n_slots(opt, t) for r, t in zip(reads, truth) if r.shape[0] >= opt.min_seed_len)
    assert st["n_seeds"] == want_slots, f"{what}: {st['n_seeds']} SA rows reserved, mem_chain's bounds give {want_slots}"
    if stats:
        assert st["n_intv"] == sum(t.shape[0] for t in truth), what
    if b.chains:
        kc = ks = 0
        for i, r in enumerate(reads):
            hdr, seeds = W.chains_of(opt, r)
            n_c = int(cn[i])
            gh = ch[kc:kc + n_c]
            n_s = int(gh["n_seeds"].sum())
            gs = cs[ks:ks + n_s]
            kc += n_c; ks += n_s
            assert n_c == hdr.shape[0] and np.array_equal(gh["n_seeds"], hdr["n"]) and all(np.array_equal(gs[f], seeds[f]) for f in ("rbeg", "qbeg", "len")), \
                f"{what}: read {idx[i]} ({tags[i]}): equal intervals, but the chains differ from mem_chain's ({n_c} chains, reference {hdr.shape[0]}): publish / SA look-up"
        assert kc == ch.shape[0] and ks == cs.shape[0]
    want_ring = options.get("seed_lds_ent", -1)
    if want_ring < 0:
        want_ring = ring(max(r.shape[0] for r in reads), options.get("seed_rd_lds", 1) != 0)
    assert ring_run == want_ring, f"{what}: {ring_run} interval-stack entries per lane in LDS, expected {want_ring}"
    return int(prof[0]), int(prof[1]), int(prof[8]), int(st["n_retries"])


def run_family(W, fam, thin):
    """every batch of a family under each of its forms (thin: the mock runtime's share of reads and forms)"""
    check_limits(W.dev)
    for b in X.batches().values():
        if b.fam != fam:
            continue
        for k, (fname, index_opts, options) in enumerate(FORMS[fam]):
            idx = list(range(len(b.reads)))
            if thin:
                if k > 0:
                    idx = b.sim if fam == 7 else b.sim[k % 2::2]      # (family 7: the batch keeps its long read)
                if fam == 2 and (k in (2, 3) or k >= 4 and (k + (b.opt.min_seed_len & 1)) % 3):      # (twelve forms: not the second handle with tables of depth 10 -- filling
                    continue                                                                          # them is a second of the mock's time --, the later ones on every third batch)
            if not idx:
                continue
            t0 = time.time()
            given_up, p2, redone, retries = run_batch(W, b, fname, index_opts, options, idx)
            if k == 0:      # once more with the counting instances of the kernels
                run_batch(W, b, fname, index_opts, options, b.sim if thin else idx, stats=True)
            print(f"{b.name}, {fname}: {len(idx)} reads, {time.time() - t0:.2f} s; given up {given_up}, pass-2 tasks {p2}, redone {redone}, retries {retries}")
            if fam == 6:
                budget = options["seed_budget"]
                assert (given_up > 0) if budget > 0 else (given_up == 0), (b.name, fname, given_up)
                if "seed_p2_cap" in options:
                    assert retries >= 1 and p2 > 1, (b.name, fname, retries, p2)
            elif options.get("seed_budget") == 0:
                assert given_up == 0, (b.name, fname, given_up)
            if fam == 7:
                assert (redone > 0) if "seed_task_stack" in options else (redone == 0), (b.name, fname, redone)      # (every batch holds a sweep with more change points than a stack of two spilt entries and the LDS ring take)
                if "mem_cap" in options:
                    assert retries >= 1, (b.name, fname, retries)


# ---- fixtures and tests ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    if not refapi.have_ref():      # (the CPU tests only: the GPU tests' fixture asserts instead)
        pytest.skip("oracle/_ref not built")
    import hostsim_build
    w = World(tmp_path_factory.mktemp("seed"), lib_path=hostsim_build.build())
    yield w
    w.close()


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    # on the GPU box the compiled reference must have travelled with the snapshot: a silent skip would turn this module green with nothing run
    assert refapi.have_ref(), "oracle/_ref (the compiled reference) is missing on the GPU box"
    w = World(tmp_path_factory.mktemp("seed"))
    yield w
    w.close()


def test_limits(sim):
    check_limits(sim.dev)
    assert sim.handle(dict(ptab_m=D7)).seed_limits()["ptab_depth"] == D7 and sim.handle(dict(ptab_m=0)).seed_limits()["ptab_depth"] == 0
    assert X.LONG_LEN > LIMITS["wave_max_len"]


def test_families_cover_their_switch_points(sim):
    """the reads of the GPU tests, on the reference's side alone"""
    cover(sim)


@pytest.mark.parametrize("fam", [1, 2, 3, 4, 5, 6, 7, 8])
def test_sim_family(sim, fam):
    run_family(sim, fam, thin=True)


@pytest.mark.gpu
def test_gpu_families_cover_their_switch_points(gpu):
    check_limits(gpu.dev)
    cover(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", [1, 2, 3, 4, 5, 6, 7, 8])
def test_gpu_family(gpu, fam):
    run_family(gpu, fam, thin=False)
