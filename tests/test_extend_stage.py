"""The extension stage of the device library -- mem_chain2aln (bwamem.c:658-812) as restated in bwa_amd/csrc/dev_extw.h (ext_chain_wave, chain_window_wave,
chain_sort_wave, wave_seed_covered), dev_ext.h (k_extend) and dev_extp.h (the plan k_ext_pack leaves for the replay) -- on crafted reads, against the compiled
reference.

A case is a read.  Truth per read: refapi.RefIndex.regs_stage(opt, read, 0), mem_chain2aln over the reference's own chains before de-duplication, compared
byte for byte, order included, with the read's slice of the device's tap_regs_raw.  Before that the read's chain tap must equal ref.chains(opt, read, 2) in n,
rbeg, qbeg and len: the tap is read after the batch has run, when the chains are as mem_flt_chained_seeds leaves them (stage 2; the replay below needs that
stage's seed scores too), so a difference there belongs to seeding or chaining and is reported as such.  Every read of every batch is compared.

Genome and reads: tests/extend_cases.py (a 15.8 kb genome written and indexed into a temporary directory; six families, 481 reads).  Every batch runs through each
kernel form that can take it (FORMS): the short-read form at both occupancies and behind k_ext_pack<4 | 5>, the ring form (one read of 1200 bases
appended: the batch's longest read chooses the form) with four columns and one column per lane, and k_extend (the same batch with opt.w = 500, the
reference run with the same options).  cover() asserts from the reference's output alone -- through extend_cases.replay, a classifier that must consume the
reference's regions exactly -- that the reads reach the points where the control code changes form (bwagpu_ext_limits).

A seed that is covered, and so decided by the "other diagonal" rule, after its chain's 64th extended seed in a short-read batch / 128th in the ring form --
the walk over srt[] with its zero stores -- is what the 12 + 4 islands and the 8400-base read are for: the replay counts 7 such seeds in the short-read
batches and 2 in the ring form's (cover() prints and asserts them).
Family 6 holds the reads on which the rule hangs on a single seed.  Its witnesses are seeds processed earlier, those with a higher score, and where
mem_flt_chained_seeds returns early a seed's score is its length, so that no witness is shorter than the seed and the factor .95 decides nothing: the
"factor" reads run with min_chain_weight = 1, which gives the seeds mem_seed_sw's scores, and place a 10-base seed on another diagonal against a covered one
of 11 bases (.9 * 11 <= 10 < .95 * 11), decided with some 20 seeds extended (from the registers) and with some 70 (in the walk); the "late" reads make the
only witness the 67th or a later extended seed of the chain.  The "bonus" batches of family 5 have the alignment to the read's end cross a deletion one base
longer than the query left of it, inside the band only because pen_clip, as ksw_extend2's end bonus, has widened the band's limit.
k_ext_pack takes queries of at most 127 and w + 1 bases: none on the island reads and none where the indel lies 30 .. 50 bases from the end of a read under
w = 10 or 20 (asserted as 0), some in every other batch (asserted through bwagpu_debug_prof, slot 8).
CPU: on the mock runtime (tests/hostsim), thinned (families 1, 4, 5 and 6: every read through the short-read form, subsets through the others; family 2: one
read; family 3: a subset).  -m gpu: everything."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import extend_cases as X
import refapi
import testdata
from bwa_amd import simdata
from bwa_amd.api import BwaGpu

LIMITS = dict(sort_lane_max=32, kept_short=64, kept_ring=128, covered_step=64, wave_max_len=1100, ring_max=2048)
LANE_W = 500             # 4 w + 132 beyond the widest ring: k_extend
SHORT_FORMS = (("occ 6", dict(ext_occ=6, ext_pack=0)), ("occ 4", dict(ext_occ=4, ext_pack=0)), ("pack 1", dict(ext_pack=1)), ("pack 5", dict(ext_pack=5)))
RING_FORMS = (("ring", dict(ext_blk=-1)), ("ring, a column per lane", dict(ext_blk=0)))
LANE_FORMS = (("lane", dict()),)
NO_PACK = ("band w 10", "band w 20")      # batches without a query k_ext_pack takes: the indels lie 30 .. 50 bases from the end, beyond w + 1


def check_limits(dev):
    assert dev.ext_limits() == LIMITS, "a switch point moved: aim the cases at it"


def ring_cols(w):
    rc = 256
    while rc < 4 * w + 4 + 128:
        rc <<= 1
    return rc


class World:
    def __init__(self, d, lib_path=None):
        self.g, self.lens = X.genome()
        self.fa = os.path.join(str(d), "extend.fa")
        simdata.write_fasta(self.fa, self.g, self.lens)
        refapi.build_index(self.fa)
        self.dev = BwaGpu(self.fa, lib_path=lib_path)
        self.dev.L.bwagpu_debug_prof.argtypes = [C.c_void_p, C.c_void_p]
        self.ref = refapi.RefIndex(self.fa)
        self.l_pac = self.ref.l_pac
        assert self.l_pac == self.g.shape[0] < 20000
        self.long = X.long_read(self.g)
        self.truth = {}

    def close(self):
        self.dev.close(); self.ref.close()

    def truth_of(self, opt, key, read):
        """(chains after mem_flt_chained_seeds, their seeds, raw regions) of one read under one option set: computed once, shared and left alone"""
        if key not in self.truth:
            r = np.ascontiguousarray(read)
            self.truth[key] = self.ref.chains(opt, r, 2) + (self.ref.regs_stage(opt, r, 0),)
        return self.truth[key]


def with_w(opt, w):
    o = type(opt).from_buffer_copy(opt)
    o.w = w
    return o


# ---- what the reference did on the reads -------------------------------------------------------------------------------------------------------------------------
def survey(W, b):
    """the replay over every read of a batch -> a dict of counts and lists"""
    s = dict(chain_n=set(), max_raw=0, skipped=0, ext_cov=0, wide=0, wide_first=0, wide_pack=0, past=[0, 0], cov_past=[0, 0], clamps=set(),
             end5=0, clip5=0, end3=0, clip3=0, qb=[], qe=[],
             f95_reg=0, f95_walk=0, f_late=0, del_in=set())
    opt, L = b.opt, W.l_pac
    off = np.concatenate([[0], np.cumsum(W.lens)])
    for i, rd in enumerate(b.reads):
        hdr, seeds, regs = W.truth_of(opt, (b.name, opt.w, i), rd)
        lq = rd.shape[0]
        info = []
        dec = X.replay(opt, lq, hdr, seeds, regs, info)
        if lq <= LIMITS["wave_max_len"]:      # covered seeds whose fate hangs on the factor .95 (decided from the registers / in the walk) or on an extended seed past the registers
            s["f95_reg"] += sum(f95 and n <= LIMITS["kept_short"] for n, f95, f64, f128 in info)
            s["f95_walk"] += sum(f95 and n > LIMITS["kept_short"] for n, f95, f64, f128 in info)
            s["f_late"] += sum(f64 and n > LIMITS["kept_short"] for n, f95, f64, f128 in info)
        if any(int(r["re"] - r["rb"]) - int(r["qe"] - r["qb"]) >= 7 for r in regs):      # a region with a deletion of 7 or more bases inside (the reads' own: one more than the bases between it and the read's end)
            s["del_in"].add(i)
        s["max_raw"] = max(s["max_raw"], regs.shape[0])
        s["qb"].append(regs["qb"].tolist()); s["qe"].append(regs["qe"].tolist())
        ks = 0
        for c, d in zip(hdr, dec):
            n = int(c["n"])
            sd = seeds[ks:ks + n]
            ks += n
            if n == 0:
                continue
            s["chain_n"].add(n)
            n_ext = 0
            for j, (si, what, at) in enumerate(d):
                for t, kept in enumerate((LIMITS["kept_short"], LIMITS["kept_ring"])):
                    if n_ext > kept and (t == 1 or lq <= LIMITS["wave_max_len"]):      # decided after the list of extended seeds has overflowed
                        s["past"][t] += 1
                        s["cov_past"][t] += what < 2
                s["skipped"] += what == 0
                s["ext_cov"] += what == 1
                if what:
                    n_ext += 1
                    r, t = regs[at], sd[si]
                    if int(r["w"]) == 2 * opt.w:
                        s["wide"] += 1
                        s["wide_first"] += j == 0
                        room = [x for x in (int(t["qbeg"]), lq - int(t["qbeg"]) - int(t["len"])) if x > 0]
                        s["wide_pack"] += j == 0 and min(room) <= opt.w + 1      # (a query k_ext_pack takes: at most w + 1 bases)
                    if int(t["qbeg"]) > 0:
                        s["end5" if int(r["qb"]) == 0 else "clip5"] += 1
                    if int(t["qbeg"]) + int(t["len"]) < lq:
                        s["end3" if int(r["qe"]) == lq else "clip3"] += 1
            # the window before its clamps (bwamem.c:669-683), and the contig of seeds[0] (bntseq.c:426-451)
            (b0, e0), (r0, r1) = X.window(opt, lq, sd, L)
            p = int(sd[0]["rbeg"])
            rev = p >= L
            rid = int(np.searchsorted(off, 2 * L - 1 - p if rev else p, side="right")) - 1
            fb, fe = int(off[rid]), int(off[rid + 1])
            if rev:
                fb, fe = 2 * L - fe, 2 * L - fb
            if b0 < 0: s["clamps"].add("0")
            if e0 > 2 * L: s["clamps"].add("2 l_pac")
            if max(b0, 0) < L < min(e0, 2 * L): s["clamps"].add("l_pac, seeds " + ("reverse" if rev else "forward"))
            if r0 < fb and fb not in (0, L): s["clamps"].add("contig start" + (" rev" if rev else ""))
            if r1 > fe and fe not in (L, 2 * L): s["clamps"].add("contig end" + (" rev" if rev else ""))
    return s


_surveys = {}


def cover(W):
    """the points the families are aimed at, from the reference's output alone (coverage conditions, not tolerances)"""
    B = X.batches()
    for name, b in B.items():
        if name not in _surveys:
            _surveys[name] = survey(W, b)
    S = _surveys
    tot = lambda k, names=None: sum(S[n][k] for n in (names or S))
    fam = lambda f: [n for n in B if B[n].fam == f]
    # the lists of extended seeds overflow, and seeds are decided after that: the short-read form's in family 1, the ring form's in family 2
    assert sum(S[n]["past"][0] for n in fam(1)) >= 2 and sum(S[n]["past"][1] for n in fam(2)) >= 2, [(n, S[n]["past"]) for n in fam(1) + fam(2)]
    cov_past = [sum(S[n]["cov_past"][0] for n in S if "short" in B[n].forms), sum(S[n]["cov_past"][1] for n in S)]
    print(f"covered seeds decided after the list of extended seeds overflowed: short-read form {cov_past[0]}, ring form {cov_past[1]}")
    assert cov_past[0] >= 5 and cov_past[1] >= 2, cov_past
    # the "other diagonal" rule hangs on one seed: .95 against .9 from the registers and in the walk, and a witness that is the 65th or a later extended seed
    assert S["witness factor"]["f95_reg"] >= 2 and S["witness factor"]["f95_walk"] >= 2 and S["witness late"]["f_late"] >= 2, (S["witness factor"], S["witness late"])
    # pen_clip as ksw_extend2's end bonus: alignments to the end across a deletion that only the widened band holds, at the end whose pen_clip is 9
    d09, d90 = S["bonus clip 0/9"]["del_in"], S["bonus clip 9/0"]["del_in"]
    assert len(d09) >= 6 and len(d90) >= 6 and not (d09 & d90), (d09, d90)      # (at least half of the 12 reads with the deletion at that end)
    # chain_sort_wave: lane 0's introsort up to sort_lane_max seeds, the network from one more, on a non-power-of-two beyond a wavefront
    lens = set().union(*(S[n]["chain_n"] for n in S))
    m = LIMITS["sort_lane_max"]
    assert {m - 1, m, m + 1} <= lens and any(n > 64 and n & (n - 1) for n in lens), sorted(lens)
    assert {63, 64, 65} <= lens, sorted(lens)
    # wave_seed_covered's second step
    assert max(S[n]["max_raw"] for n in fam(3)) > LIMITS["covered_step"], [S[n]["max_raw"] for n in fam(3)]
    assert tot("ext_cov") >= 20 and tot("skipped") >= 100, (tot("ext_cov"), tot("skipped"))
    # the second try with the doubled band, also for the seed a chain processes first (the one k_ext_pack answers)
    assert tot("wide", fam(4)) >= 20 and tot("wide_first", fam(4)) >= 5, (tot("wide", fam(4)), tot("wide_first", fam(4)))
    assert S["band pack"]["wide_pack"] >= 8, S["band pack"]["wide_pack"]
    assert any(S[n]["wide"] == 0 for n in fam(5)) and all(S[n]["wide"] < len(B[n].reads) for n in fam(4))
    # to the end or clipped, at either end, under pen_clip5 != pen_clip3 in both orders; and the two sets decide differently on the same reads
    for n in ("edges clip 0/9", "edges clip 9/0"):
        assert min(S[n][k] for k in ("end5", "clip5", "end3", "clip3")) >= 3, (n, [S[n][k] for k in ("end5", "clip5", "end3", "clip3")])
    a, c = S["edges clip 0/9"], S["edges clip 9/0"]
    assert sum(x != y for x, y in zip(a["qb"], c["qb"])) >= 3 and sum(x != y for x, y in zip(a["qe"], c["qe"])) >= 3
    # chain_window_wave's clamps
    clamps = set().union(*(S[n]["clamps"] for n in S))
    want = {"0", "2 l_pac", "l_pac, seeds forward", "l_pac, seeds reverse", "contig start", "contig end", "contig start rev", "contig end rev"}
    assert want <= clamps, want - clamps
    # 481 different reads in all; the tandem, edge and bonus reads run under two or three option sets each: 877 pairs of a read and an option set
    n_pairs = sum(len(b.reads) for b in B.values())
    assert len({r.tobytes() for b in B.values() for r in b.reads}) == 481 and n_pairs == 877, n_pairs


# ---- the device side ---------------------------------------------------------------------------------------------------------------------------------------------
def run_batch(W, b, form, fname, options, idx):
    """one batch under one form -> the number of extensions k_ext_pack answered"""
    dev = W.dev
    reads = [b.reads[i] for i in idx]
    tags = [b.tags[i] for i in idx]
    keys = [(b.name, i) for i in idx]
    opt = b.opt if form != "lane" else with_w(b.opt, LANE_W)
    if form != "short" and max(r.shape[0] for r in reads) <= LIMITS["wave_max_len"]:
        reads.append(W.long); tags.append("the 1200-base read"); keys.append(("long", b.name))
    max_len = max(r.shape[0] for r in reads)
    assert (max_len <= LIMITS["wave_max_len"]) == (form == "short") and (ring_cols(opt.w) <= LIMITS["ring_max"]) == (form != "lane"), (b.name, form)
    truth = [W.truth_of(opt, (k[0], opt.w, k[1]), r) for k, r in zip(keys, reads)]
    seqs, off = testdata.ragged(reads)
    old = {k: dev.get_option(k) for k in options}
    dev.set_taps(True)
    try:
        for k, v in options.items():
            dev.set_option(k, v)
        dev.upload(seqs, off); dev.run(opt)
        dev.download()
        cn, ch, cs = dev.tap_chains()
        rn, rr = dev.tap_regs_raw()
        prof = (C.c_ulonglong * 16)()
        dev.L.bwagpu_debug_prof(dev.h, prof)
    finally:
        dev.set_taps(False)
        for k, v in old.items():
            dev.set_option(k, v)
    what = f"{b.name}, form {fname}"
    bad = []
    kc = ks = kr = 0
    for i, (hdr, seeds, regs) in enumerate(truth):
        n_c, n_r = int(cn[i]), int(rn[i])
        gh = ch[kc:kc + n_c]
        n_s = int(gh["n_seeds"].sum())
        gs, gr = cs[ks:ks + n_s], rr[kr:kr + n_r]
        kc += n_c; ks += n_s; kr += n_r
        assert n_c == hdr.shape[0] and np.array_equal(gh["n_seeds"], hdr["n"]) and all(np.array_equal(gs[f], seeds[f]) for f in ("rbeg", "qbeg", "len")), \
            f"{what}: read {i} ({tags[i]}): the chains differ from mem_flt_chained_seeds' ({n_c} chains, reference {hdr.shape[0]}): a matter of seeding or chaining"
        if n_r != regs.shape[0] or gr.tobytes() != regs.tobytes():
            first = next((j for j in range(min(n_r, regs.shape[0])) if gr[j].tobytes() != regs[j].tobytes()), min(n_r, regs.shape[0]))
            bad.append(f"read {i} ({tags[i]}): device {n_r} raw regions, reference {regs.shape[0]}; first difference at region {first}"
                       + (f": device {gr[first]}, reference {regs[first]}" if first < min(n_r, regs.shape[0]) else ""))
    assert kc == ch.shape[0] and ks == cs.shape[0] and kr == rr.shape[0]
    assert not bad, f"{what}: {len(bad)} of {len(truth)} reads differ from mem_chain2aln:\n  " + "\n  ".join(bad[:8])
    return int(prof[8]) if form == "short" and options.get("ext_pack") else 0


def run_family(W, fam, thin):
    """every batch of a family under each form that can take it (thin: the mock runtime's share of reads and forms)"""
    check_limits(W.dev)
    answered = []
    for b in X.batches().values():
        if b.fam != fam:
            continue
        idx = b.sim if thin else list(range(len(b.reads)))
        for form, forms in (("short", SHORT_FORMS), ("ring", RING_FORMS), ("lane", LANE_FORMS)):
            if form not in b.forms:
                continue
            for k, (fname, options) in enumerate(forms):
                sub = idx
                if thin:
                    if fname in ("occ 4", "pack 5"):      # (the same source as occ 6 / pack 1, instantiated for another occupancy)
                        continue
                    if fam in (4, 5) and (form != "short" or fname != "occ 6"):
                        sub = idx[k::3][:24] if form == "short" else idx[::5][:12]
                    elif form == "ring" and k == 1 or form == "lane":
                        sub = idx[:4]
                    if not sub:
                        continue
                t0 = time.time()
                n = run_batch(W, b, form, fname, options, sub)
                print(f"{b.name}, {fname}: {len(sub)} reads, {time.time() - t0:.2f} s")
                if "pack" in fname:
                    answered.append((b.name, fname, n))
    # extensions were answered ahead by k_ext_pack (bwagpu_debug_prof, slot 8) in every batch it ran on.  It takes queries of up to 127 bases and w + 1, and only
    # the first extensions of a chain: on the island reads (families 1 and 6) that is none
    assert fam == 2 or answered
    for name, fname, n in answered:
        assert (n == 0) if fam in (1, 6) or name in NO_PACK else (n > 0), answered


# ---- fixtures and tests ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    if not refapi.have_ref():      # (the CPU tests only: the GPU tests' fixture asserts instead)
        pytest.skip("oracle/_ref not built")
    import hostsim_build
    w = World(tmp_path_factory.mktemp("extend"), lib_path=hostsim_build.build())
    yield w
    w.close()


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    # on the GPU box the compiled reference must have travelled with the snapshot: a silent skip would turn this module green with nothing run
    assert refapi.have_ref(), "oracle/_ref (the compiled reference) is missing on the GPU box"
    w = World(tmp_path_factory.mktemp("extend"))
    yield w
    w.close()


def test_limits(sim):
    check_limits(sim.dev)
    assert ring_cols(100) <= LIMITS["ring_max"] < ring_cols(LANE_W) and X.LONG_LEN > LIMITS["wave_max_len"]
    assert max(r.shape[0] for b in X.batches().values() if "short" in b.forms for r in b.reads) == LIMITS["wave_max_len"]


def test_families_cover_their_switch_points(sim):
    """the reads of the GPU tests, on the reference's side alone"""
    cover(sim)


@pytest.mark.parametrize("fam", [1, 2, 3, 4, 5, 6])
def test_sim_family(sim, fam):
    run_family(sim, fam, thin=True)


@pytest.mark.gpu
def test_gpu_families_cover_their_switch_points(gpu):
    cover(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", [1, 2, 3, 4, 5, 6])
def test_gpu_family(gpu, fam):
    run_family(gpu, fam, thin=False)
