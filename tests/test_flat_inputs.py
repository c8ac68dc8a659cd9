"""What the *_flat test hooks of the device library share: the handle's one pair of buffers for the caller's reads (FlatReads in bwa_amd/csrc/bwagpu.hip), and
what each hook rejects of malformed reads.

run_shared_buffers: bwagpu_cigars_flat, _sam_flat, _rescue_flat, _dedup_flat, _sampe_flat, _sam_pe_flat and _alns_flat in turn on one handle, on a small, a larger
and the small input again, then in reverse order -- the shared buffers grow, then hold a stale tail -- each result equal to the same call's on a fresh handle.
Record arrays and text are compared byte for byte, timings not at all; CIGAR records are compared decoded (hostapi.decode_cigars), since the order of the
operation array differs between two calls on the device.

run_reads_rejected: the same malformed reads against the six hooks that take reads (bwagpu_alns_flat takes lengths only), through ctypes.  The expectations are
what the entry points did before they shared FlatReads.
CPU: on the mock runtime (tests/hostsim), the larger input with shorter reads.  -m gpu: the same on the device."""
import ctypes as C

import numpy as np
import pytest

import hostapi
import testdata
from bwa_amd import simdata
from bwa_amd.api import BwaGpu
from bwa_amd.structs import PESTAT_DTYPE, PeOut, SamIn, SamOut, default_opt

HOOKS = ("cigars_flat", "sam_flat", "rescue_flat", "dedup_flat", "sampe_flat", "sam_pe_flat", "alns_flat")
PAIR_HOOKS = ("rescue_flat", "sampe_flat", "sam_pe_flat")
SMALL, LARGE, LARGE_SIM = (4, 100), (16, 250), (16, 150)      # (pairs, bases per read); the mock runtime is lane-serial, and the alignment kernels' work grows with the square of the length
SEEDS = (32, 34)      # (batches with few hits per read: mate rescue on the mock runtime takes a second otherwise)


class World:
    def __init__(self, lib_path=None, options=None):
        self.prefix, self.g = testdata.small_index()
        self.make = lambda: BwaGpu(self.prefix, lib_path=lib_path, options=options)
        self.dev = self.make()

    def close(self):
        self.dev.close()


class Inputs:
    """the lists, CIGAR records and operation array a batch of n_pairs simulated pairs leaves on dev, and what else the hooks take"""
    def __init__(self, W, n_pairs, length, seed):
        dev, self.opt = W.dev, default_opt()
        a, b = simdata.make_reads_pe(W.g, n_pairs, length=length, seed=seed, sub=0.02, dele=0.01, ins=0.01)
        self.seqs, self.off = testdata.flat(np.stack([a, b], axis=1).reshape(-1, length))
        dev.upload(self.seqs, self.off); dev.run(self.opt)
        self.counts, self.regs = dev.download()
        self.cigs, self.ops = dev.cigars(self.opt), dev.cigar_ops()
        self.n = self.counts.shape[0]
        self.ids = 100 + np.arange(self.n, dtype=np.int64)
        self.read_len = np.diff(self.off).astype(np.int32)
        self.names = [f"p{r >> 1}" for r in range(self.n)]
        self.quals = bytes(33 + (k * 7) % 40 for k in range(int(self.off[-1])))
        self.pes = np.zeros(4, dtype=PESTAT_DTYPE)      # a fixed window: FR, around make_reads_pe's inserts
        self.pes["failed"] = 1; self.pes["low"] = 1; self.pes["high"] = 1; self.pes["std"] = 1.0
        self.pes[1] = (200, 600, 0, 400.0, 40.0)
        assert self.regs.shape[0] >= self.n // 2, "the simulated batch found too few regions"


def call(dev, hook, I, seqs=None, off=None, quals=True):
    """the hook through bwa_amd.api on I's lists and (unless given) I's reads"""
    seqs, off = (I.seqs, I.off) if seqs is None else (seqs, off)
    q = I.quals if quals else None
    if hook == "cigars_flat":
        return dev.cigars_flat(I.opt, seqs, off, I.counts, I.regs)
    if hook == "sam_flat":
        return dev.sam_flat(I.opt, seqs, off, I.counts, I.regs, I.ids, I.cigs, I.ops, I.names, quals=q)
    if hook == "rescue_flat":
        return dev.rescue_flat(I.opt, I.pes, seqs, off, I.counts, I.regs, I.ids)
    if hook == "dedup_flat":
        return dev.dedup_flat(I.opt, seqs, off, I.counts, I.regs)
    if hook == "sampe_flat":
        return dev.sampe_flat(I.opt, I.pes, seqs, off, I.counts, I.regs, I.ids)
    if hook == "sam_pe_flat":
        return dev.sam_pe_flat(I.opt, I.pes, seqs, off, I.counts, I.regs, I.ids, I.names, quals=q, want_records=True)
    return dev.alns_flat(I.opt, I.counts, I.regs, I.ids, I.read_len, I.cigs, I.ops)


def canon(x):
    """a result without its timings, in a form that compares with ==: arrays as their bytes, CIGAR records with their operations looked up"""
    if isinstance(x, dict):
        d = {k: canon(v) for k, v in x.items() if k not in ("ms", "kernel_ms", "cigs", "ops")}
        if "cigs" in x:
            d["cigars"] = hostapi.decode_cigars(x["cigs"], x["ops"])
        return d
    if isinstance(x, (tuple, list)):
        if len(x) == 2 and isinstance(x[0], np.ndarray) and x[0].dtype.names and "n_cigar" in x[0].dtype.names:      # cigars_flat's (records, operation array)
            return hostapi.decode_cigars(*x)
        return tuple(canon(v) for v in x if not isinstance(v, float))
    if isinstance(x, np.ndarray):
        return (x.dtype.str if x.dtype.names is None else x.dtype.itemsize, x.shape, x.tobytes())
    return x


def fresh_results(W, I, hooks=HOOKS, **kw):
    want = {}
    for hook in hooks:
        dev = W.make()
        try:
            want[hook] = canon(call(dev, hook, I, **kw))
        finally:
            dev.close()
    return want


def run_shared_buffers(W, small, large, seeds):
    dev = W.dev
    S, B = Inputs(W, *small, seeds[0]), Inputs(W, *large, seeds[1])      # (B's batch is the one that stays on the handle)
    assert int(B.off[-1]) >= 3 * int(S.off[-1]) and B.regs.shape[0] >= 3 * S.regs.shape[0] and B.ops.shape[0] > 0
    want = {id(I): fresh_results(W, I) for I in (S, B)}
    assert want[id(B)]["sam_flat"]["text"].count(b"\n") >= B.n and want[id(S)]["sam_pe_flat"]["text"].count(b"\n") >= S.n
    for what, I, order in (("small", S, HOOKS), ("large", B, HOOKS), ("small again", S, HOOKS), ("large, reversed", B, HOOKS[::-1])):
        for hook in order:
            assert canon(call(dev, hook, I)) == want[id(I)][hook], f"{what}: {hook} differs from the same call on a fresh handle"
    # the batch's own results are where they were
    assert dev.cigar_ops().tobytes() == B.ops.tobytes(), "the batch's operation array changed under the *_flat calls"
    assert hostapi.decode_cigars(dev.cigars(B.opt), dev.cigar_ops()) == hostapi.decode_cigars(B.cigs, B.ops)


def raw_calls(dev, I):
    """hook -> f(seqs, off, quals): the C entry point on I's lists with these reads (arrays or None) -> its return value; what a successful call returns is freed"""
    L, h, n, o, P = dev.L, dev.h, I.n, C.byref(I.opt), I.pes.ctypes.data
    ptr = lambda x: None if x is None else x.ctypes.data
    cnt, regs, ids, cigs, ops = (x.ctypes.data for x in (I.counts, I.regs, I.ids, I.cigs, I.ops))
    names = np.frombuffer("".join(I.names).encode(), dtype=np.uint8).copy()
    name_off = np.concatenate([[0], np.cumsum([len(s) for s in I.names])]).astype(np.int64)
    out = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)

    def sam_in(quals):
        return SamIn(names.ctypes.data, name_off.ctypes.data, C.cast(C.c_char_p(quals), C.c_void_p) if quals is not None else None, None, None, None, 0)

    def done(rc, *ptrs):
        for p in ptrs if rc == 0 else ():
            L.bwagpu_free(p)
        return rc

    def cigars_flat(seqs, off, quals):
        p, k, po, ko = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_int64()
        return done(L.bwagpu_cigars_flat(h, o, n, ptr(seqs), ptr(off), cnt, regs, C.byref(p), C.byref(k), C.byref(po), C.byref(ko)), p, po)

    def dedup_flat(seqs, off, quals):
        p, k = C.c_void_p(), C.c_int64()
        return done(L.bwagpu_dedup_flat(h, o, n, ptr(seqs), ptr(off), cnt, regs, out[0].ctypes.data, C.byref(p), C.byref(k), out[1].ctypes.data), p)

    def sam_flat(seqs, off, quals):
        sin, so = sam_in(quals), SamOut()
        return done(L.bwagpu_sam_flat(h, o, n, ptr(seqs), ptr(off), cnt, regs, ids, cigs, ops, I.ops.shape[0], C.byref(sin), C.byref(so)), so.text, so.off, so.flags, so.n_lines)

    def rescue_flat(seqs, off, quals):
        pr, ps, nr, prec, ppri, ppair, ms = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_float()
        return done(L.bwagpu_rescue_flat(h, o, P, n // 2, ptr(seqs), ptr(off), cnt, regs, ids, out[0].ctypes.data, C.byref(pr), C.byref(ps), C.byref(nr), C.byref(prec),
                                         C.byref(ppri), out[1].ctypes.data, C.byref(ppair), C.byref(ms)), pr, ps, prec, ppri, ppair)

    def pe_ptrs(pe):
        return [C.c_void_p(getattr(pe, f)) for f in ("regs", "src", "rescue", "pri", "n_pri", "pairs", "sampe", "cigs", "ops", "alns", "n_aln")]

    def sampe_flat(seqs, off, quals):
        pe = PeOut()
        return done(L.bwagpu_sampe_flat(h, o, P, n // 2, ptr(seqs), ptr(off), cnt, regs, ids, out[0].ctypes.data, C.byref(pe)), *pe_ptrs(pe))

    def sam_pe_flat(seqs, off, quals):
        sin, so, pe = sam_in(quals), SamOut(), PeOut()
        return done(L.bwagpu_sam_pe_flat(h, o, P, n // 2, ptr(seqs), ptr(off), cnt, regs, ids, C.byref(sin), out[0].ctypes.data, C.byref(pe), C.byref(so)),
                    so.text, so.off, so.flags, so.n_lines, *pe_ptrs(pe))

    return dict(cigars_flat=cigars_flat, dedup_flat=dedup_flat, sam_flat=sam_flat, rescue_flat=rescue_flat, sampe_flat=sampe_flat, sam_pe_flat=sam_pe_flat)


def run_reads_rejected(W, small, seed):
    dev = W.dev
    L, h = dev.L, dev.h
    I = Inputs(W, *small, seed)
    want = fresh_results(W, I)
    raw = raw_calls(dev, I)
    seqs, off = I.seqs, I.off
    err = lambda: L.bwagpu_last_error(h).decode()

    def mark():
        """leaves a text of another call in the handle, so that no earlier rejection's text can stand in for the next one's"""
        bad = I.counts.copy(); bad[0] = -1
        assert L.bwagpu_cigars_flat(h, C.byref(I.opt), I.n, seqs.ctypes.data, off.ctypes.data, bad.ctypes.data, I.regs.ctypes.data, *[C.byref(x) for x in (C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_int64())]) == -2
        assert "negative count" in err()

    def rejected(hook, text, s, o):
        mark()
        assert raw[hook](s, o, I.quals) == -2, hook
        if text:
            assert text in err() and f"bwagpu_{hook}" in err(), (hook, text, err())
        assert canon(call(dev, hook, I)) == want[hook], f"{hook}: a valid call after a rejected one"

    descends = off.copy(); descends[2] = descends[1] - 1
    negative = off.copy(); negative[0] = -1
    code5 = seqs.copy(); code5[int(off[1]) + 7] = 5
    has_text = ("cigars_flat", "dedup_flat", "sam_flat")      # (the pair hooks set no text for their reads)
    for hook in raw:
        t = lambda text: text if hook in has_text else None
        rejected(hook, None, seqs, None)
        rejected(hook, None, None, off)
        rejected(hook, t("ascend"), seqs, descends)
        rejected(hook, t("ascend"), seqs, negative)
        if hook == "sam_flat":      # takes the reads as they are: the formatter has a character for every code
            assert raw[hook](code5, off, I.quals) == 0
        else:
            rejected(hook, t("base code"), code5, off)
    # a first offset of 3, three dead bytes in front of the reads (no base codes: they are no part of a read)
    seqs3, off3 = np.concatenate([np.full(3, 9, dtype=np.uint8), seqs]), off + 3
    want.update(fresh_results(W, I, ("sam_pe_flat",), quals=False))      # (without qualities: they sit at the reads' own offsets)
    for hook in raw:
        if hook in PAIR_HOOKS:
            assert canon(call(dev, hook, I, seqs3, off3, quals=False)) == want[hook], f"{hook}: reads that begin at offset 3"
        else:
            rejected(hook, "ascend", seqs3, off3)


# ---- fixtures and tests -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim():
    import hostsim_build
    w = World(lib_path=hostsim_build.build(), options={"ptab_m": 6})
    yield w
    w.close()


@pytest.fixture(scope="module")
def gpu():
    w = World()
    yield w
    w.close()


def test_sim_shared_buffers(sim):
    run_shared_buffers(sim, SMALL, LARGE_SIM, SEEDS)


def test_sim_reads_rejected(sim):
    run_reads_rejected(sim, SMALL, 33)


@pytest.mark.gpu
def test_gpu_shared_buffers(gpu):
    run_shared_buffers(gpu, SMALL, LARGE, SEEDS)


@pytest.mark.gpu
def test_gpu_reads_rejected(gpu):
    run_reads_rejected(gpu, SMALL, 33)
