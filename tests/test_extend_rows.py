"""Crafted cases for the window rows of wave_ksw_extend2 (dev_extw.h: the register-resident one- and two-column row forms of the short-read
extension kernel), through bwagpu_debug_dp kind 0 exactly as test_dp_fuzz.run_extend drives it, against the compiled reference's ksw_extend2
(ksw.c:416), field by field.  Where the fuzz draws its cases, these are built to aim the row loops' corners at each other at the smallest sizes
at which they exist:

  short      queries of 1, 2, 7, 8 and 9 bases (the tail test's first row, qlen - 8, at and below zero) against targets of 1 .. 65 rows
  band       a band that grows by a column a row through 63 -> 64 -> 65 and 127 -> 128 -> 129 live columns and shrinks back the same way: the
             hand-overs one column per lane <-> two columns per lane <-> several passes, with the columns a form leaves behind (stale slots);
             the band's clamps (ksw.c:447-448) bind in every one of these rows
  tlen       targets of 63, 64, 65, 127, 128 and 129 rows: the reload of the reference bases at every 64th row, and the last row
  drop       a good diagonal that turns into mismatches at row K, for every K: the z-drop row (option sets with a z-drop) or the m == 0 row
             (without) moves through the 31st, 32nd and 33rd parked row, the 64th row and the target's last row -- the rows that end a segment
  qend       the band reaches the query's end (ksw.c:486-489) on the very row on which it outgrows 64 columns
  nbases     the `tlen` cases with N in the query (the reference text is 2-bit packed: a target holds no N on the device, bntseq.c:229) and with h0 = 1

each with h0 from 1 to several hundred and under all four option sets of test_dp_fuzz._opts().

Every case reaches the DP: the routine answers an extension whose diagonal loses P < min(o_del + e_del, o_ins + e_ins) (and P < h0, P < zdrop) without
it, so every case is built with two mismatches or a gap, P is computed here from the case and asserted for every one of them, and the device's own count
of shortcut answers must be zero.  (A query of one base cannot lose that much under three of the four option sets -- one mismatch costs a + b --: those
cases reach the DP through h0 <= P, which is asserted instead.)

What the families are said to cover is asserted too, from a numpy restatement of ksw_extend2's band bookkeeping (trace(), checked against the reference's
score and end point in every case it is used on)."""
import numpy as np
import pytest

import refapi
import testdata
from bwa_amd.api import BwaGpu
from test_dp_fuzz import CaseSet, _opts, ref_extend

pytestmark = pytest.mark.skipif(not refapi.have_ref(), reason="oracle/_ref not built")


def _mat(o):
    return np.array([o.mat[i] for i in range(25)], dtype=np.int64).reshape(5, 5)


def diag_loss(o, q, t):
    """P of dev_extw.h's diagonal rule: what the first len(q) diagonal cells lose against an all-match diagonal (None: the target is shorter)."""
    if len(t) < len(q):
        return None
    m = _mat(o)
    return int((m.max() - m[t[:len(q)], q]).sum())


def reaches_dp(o, q, t, h0):
    """(strong, rule): P >= min(oe_del, oe_ins) -- and, weaker, the routine's whole condition for computing rows"""
    P = diag_loss(o, q, t)
    if P is None:
        return True, True
    oe = min(o.o_del + o.e_del, o.o_ins + o.e_ins)
    return P >= oe, not (P < oe and (o.zdrop <= 0 or P < o.zdrop) and h0 > P)


def trace(o, q, t, w, h0, eb):
    """ksw_extend2's rows (ksw.c:430-505) a row at a time in numpy.  Returns (bands, stop, row, (score, qle, tle)): the [beg, end) of every row computed,
    why the loop ended ('m0', 'zdrop' or 'end') and at which row."""
    qlen, tlen = len(q), len(t)
    mat = _mat(o); mx = int(mat.max())
    oe_del, oe_ins = o.o_del + o.e_del, o.o_ins + o.e_ins
    H = np.zeros(qlen + 2, dtype=np.int64); E = np.zeros(qlen + 2, dtype=np.int64)
    H[0] = h0
    if qlen >= 1:
        H[1:qlen + 1] = np.maximum(max(h0 - oe_ins, 0) - np.arange(qlen) * o.e_ins, 0) if h0 > oe_ins else 0
    lim = int((qlen * mx + eb - o.o_ins) / o.e_ins + 1.); w = min(w, max(lim, 1))
    lim = int((qlen * mx + eb - o.o_del) / o.e_del + 1.); w = min(w, max(lim, 1))
    beg, end, mxs, max_i, max_j = 0, qlen, h0, -1, -1
    bands, stop, row = [], "end", tlen
    for i in range(tlen):
        beg = max(beg, i - w); end = min(end, i + w + 1, qlen)
        h1 = max(h0 - (o.o_del + o.e_del * (i + 1)), 0) if beg == 0 else 0
        bands.append((beg, end))
        m, mj = 0, -1
        if end > beg:
            n = end - beg
            Mo, e = H[beg:end].copy(), E[beg:end].copy()
            M = np.where(Mo != 0, Mo + mat[t[i], q[beg:end]], 0)
            a = np.maximum(M - oe_ins, 0)
            k = np.arange(n)
            f = np.zeros(n, dtype=np.int64)
            if n > 1:
                f[1:] = np.maximum.accumulate(a + k * o.e_ins)[:-1] - (k[1:] - 1) * o.e_ins
            h = np.maximum(np.maximum(M, e), f)
            H[beg] = h1; H[beg + 1:end + 1] = h
            E[beg:end] = np.maximum(np.maximum(e - o.e_del, M - oe_del), 0)
            m = int(h.max()); mj = beg + n - 1 - int(np.argmax(h[::-1]))        # the last column wins ties (ksw.c:473-474)
        else:
            H[end] = h1
        E[end] = 0
        if m == 0:
            stop, row = "m0", i
            break
        if m > mxs:
            mxs, max_i, max_j = m, i, mj
        elif o.zdrop > 0:
            di, dj = i - max_i, mj - max_j
            if (di > dj and mxs - m - (di - dj) * o.e_del > o.zdrop) or (di <= dj and mxs - m - (dj - di) * o.e_ins > o.zdrop):
                stop, row = "zdrop", i
                break
        live = (H[beg:end + 1] != 0) | (E[beg:end + 1] != 0)       # ksw.c:502-505
        first = np.nonzero(live[:end - beg])[0]
        nb = beg + int(first[0]) if len(first) else end
        rest = np.nonzero(live[nb - beg:])[0]
        j = nb + int(rest[-1]) if len(rest) else nb - 1
        beg, end = nb, min(j + 2, qlen)
    return bands, stop, row, (mxs, max_j + 1, max_i + 1)


def _add(cs, q, t, w, h0, eb, flags):
    """CaseSet.add for a query and a target given as the routine is to SEE them: the flags' reversals and the complement (test_dp_fuzz._seen) are undone first"""
    q = np.asarray(q, dtype=np.uint8); t = np.asarray(t, dtype=np.uint8)
    if flags & 1:
        q = q[::-1]
    if flags & 2:
        t = t[::-1]
    if flags & 4:
        t = (3 - t[::-1]).astype(np.uint8)
    cs.add(q, t, w, h0, eb, flags)


def _mis(b, k=1):
    return (b + k) % 4 if b < 4 else k % 4


def _copy_with(t, qlen, mism, rng):
    """the target's first qlen bases (random beyond its end) with the bases at `mism` replaced by mismatches"""
    q = np.concatenate([t, rng.integers(0, 4, size=max(0, qlen - len(t))).astype(np.uint8)])[:qlen].copy()
    for n, p in enumerate(mism):
        if 0 <= p < qlen:
            q[p] = _mis(int(q[p]) if p >= len(t) else int(t[p]), 1 + n % 3)
    return q


def fam_short(o, rng):
    cs = CaseSet()
    n = 0
    for qlen in (1, 2, 7, 8, 9):
        for tlen in (1, 2, 5, 9, 20, 63, 64, 65):
            for h0 in (1, 5, 30, 300):
                t = rng.integers(0, 4, size=tlen).astype(np.uint8)
                pat = [(0, 1), (qlen - 2, qlen - 1), (0, qlen - 1)][n % 3]
                q = _copy_with(t, qlen, pat, rng)
                if qlen >= 7 and n % 4 == 3:         # a gap instead: one base of the target missing from the query
                    q = _copy_with(np.delete(t, 1) if tlen > 2 else t, qlen, (qlen - 1, 0), rng)
                if qlen == 1 and h0 > 1:             # one base cannot lose enough: the DP is reached through h0 <= P (see the module's text)
                    h0 = 1
                _add(cs, q, t, (1, 5, 100)[n % 3], h0, (0, 5)[n % 2], n % 8)
                n += 1
    return cs


def fam_band(o, rng):
    """qlen - w - 1 rows of growth (end = i + w + 1 with beg = 0), then, once the band's lower clamp binds (i > w), qlen - (i - w) columns: a large h0 and a
    good diagonal keep every column alive in between, so the widths are the clamps' and pass 63 / 64 / 65 (and 127 / 128 / 129) on the way up and down."""
    cs = CaseSet()
    n = 0
    for qlen, w in ((90, 50), (100, 55), (70, 62), (66, 63), (170, 100), (180, 110), (140, 126), (131, 127), (129, 64), (150, 40)):
        for h0 in (qlen + 120, qlen + 300):
            for var in range(4):
                tlen = qlen + w + 24
                t = rng.integers(0, 4, size=tlen).astype(np.uint8)
                q = _copy_with(t, qlen, (0, 1), rng)
                if var == 1:                         # an unrelated stretch: the zero-trimming works on the band as well
                    a = 20 + 7 * (n % 5); q[a:a + 12] = [_mis(int(x), 2) for x in t[a:a + 12]]
                if var == 2:                         # a deletion from the query in the middle: the band's diagonal shifts
                    a = qlen // 2; q = np.concatenate([q[:a], _copy_with(t[a + 3:], qlen - a, (), rng)])
                if var == 3:
                    q[qlen // 3] = 4                 # N
                _add(cs, q, t, w, h0, (0, 5)[n % 2], n % 8)
                n += 1
    return cs


def fam_tlen(o, rng, with_n=False):
    cs = CaseSet()
    n = 0
    for tlen in (63, 64, 65, 127, 128, 129):
        for dq in (-5, 0, 5, 21):
            for h0 in ((1, 19) if with_n else (1, 20, 60, 400)):
                for w in (5, 100):
                    qlen = tlen + dq
                    t = rng.integers(0, 4, size=tlen).astype(np.uint8)
                    # two mismatches after a run of matches (h0 = 1 survives them), or a one-base gap
                    q = _copy_with(t, qlen, (12, 14), rng) if n % 3 else _copy_with(np.delete(t, 9), qlen, (), rng)
                    if with_n:
                        q[[3 + n % 5, qlen // 2, qlen - 2 - n % 3]] = 4
                    _add(cs, q, t, w, h0, (0, 5, 9)[n % 3], n % 8)
                    n += 1
    return cs


def fam_drop(o, rng):
    """matches up to row K (two mismatches among the first rows), every base a mismatch from there on"""
    cs = CaseSet()
    n = 0
    tlen = 100
    # (band, h0): a band of one column either side leaves no deletion tail to hold the row maximum up -- the score falls by a mismatch a row and the z-drop
    # comes a fixed number of rows after the turn; wider bands and small h0 end in m == 0 instead
    for w, h0, Ks in ((1, 400, range(2, 40)), (1, 150, range(2, 40)), (3, 30, range(2, 72, 2)), (3, 150, range(3, 72, 2)), (8, 30, range(2, 72, 2)),
                      (8, 400, range(3, 72, 2)), (20, 30, range(2, 72, 2)), (100, 150, range(3, 72, 4))):
        for K in Ks:
            t = rng.integers(0, 4, size=tlen).astype(np.uint8)
            q = _copy_with(t, tlen, (1, 3), rng)
            q[K:] = [_mis(int(x), 2) for x in t[K:]]
            if n % 5 == 4 and K > 12:            # the turn comes as a gap
                q = np.concatenate([q[:K], q[K + 2:], q[:2]])
            _add(cs, q, t, w, h0, (0, 5)[n % 2], 0 if n % 3 else n % 8)
            n += 1
    return cs


def fam_qend(o, rng):
    """beg = 0 (a large h0 keeps column 0's left neighbour alive), end = i + w + 1: the band is 64 columns wide at row 63 - w, and with qlen = 64 that is the
    row on which it first touches the query's end; the neighbours on both sides and windows that do not start at column 0 come along."""
    cs = CaseSet()
    n = 0
    for qlen in (62, 63, 64, 65, 66, 67):
        for w in (20, 40, 61, 62, 63):
            for h0 in (qlen + 100, qlen + 350):
                for var in range(2):
                    tlen = qlen + 12
                    t = rng.integers(0, 4, size=tlen).astype(np.uint8)
                    q = _copy_with(t, qlen, (0, 2), rng)
                    if var:                          # an insertion into the query near its start: the window's base moves off column 0 later on
                        q = np.concatenate([q[:6], [_mis(int(q[6]))] * 2, q[6:]])[:qlen].astype(np.uint8)
                    _add(cs, q, t, w, h0, (0, 5)[n % 2], n % 8)
                    n += 1
    # a band of 2 w + 1 = 51 columns moves right by a column a row and the window is re-based every 13 rows or so: over 16 consecutive query lengths the
    # row on which it reaches the query's end falls on every row of that cycle, the one that leaves the window included
    for qlen in range(84, 100):
        for h0 in (qlen + 100, qlen + 350):
            t = rng.integers(0, 4, size=qlen + 12).astype(np.uint8)
            _add(cs, _copy_with(t, qlen, (0, 2), rng), t, 25, h0, (0, 5)[n % 2], n % 8)
            n += 1
    return cs


FAMILIES = {
    "short": fam_short,
    "band": fam_band,
    "tlen": fam_tlen,
    "drop": fam_drop,
    "qend": fam_qend,
    "nbases": lambda o, rng: fam_tlen(o, rng, with_n=True),
}


def _coverage(name, oi, o, cs):
    """what the family claims to reach, from the band trace (the trace itself is held to the reference's result)"""
    if name not in ("band", "drop", "qend", "tlen"):
        return
    grow, shrink, stops, qend_hit, rows_done = set(), set(), {}, False, set()
    for (q, t, w, h0, eb) in cs.py:
        bands, stop, row, res = trace(o, q, t, w, h0, eb)
        assert list(res) == ref_extend(o, q, t, w, h0, eb)[:3], f"{name} opt {oi}: the band trace disagrees with the reference ({res})"
        wd = [e - b for b, e in bands]
        for a, b in zip(wd, wd[1:]):
            if b == a + 1: grow.add(b)
            if b == a - 1: shrink.add(b)
        stops.setdefault(stop, set()).add(row)
        rows_done.add(len(bands))
        for r in range(1, len(bands)):
            if bands[r][1] == len(q) and bands[r - 1][1] < len(q) and wd[r] >= 64 and wd[r - 1] <= 63:
                qend_hit = True
    if name == "band":
        need = {63, 64, 65, 127, 128, 129}
        assert need <= grow and need <= shrink, f"band opt {oi}: widths reached growing {sorted(grow & need)}, shrinking {sorted(shrink & need)}"
    if name == "drop":
        # rows are parked from row 0 on and evaluated every 32: the 31st, 32nd and 33rd parked rows are rows 30, 31, 32 and again 62, 63, 64.  (Under the
        # pacbio set a row loses one point at most, and no z-drop comes within the target.)
        zd, m0 = stops.get("zdrop", set()), stops.get("m0", set())
        if o.zdrop > 0 and oi != 1:
            assert {30, 31, 32} <= zd or {62, 63, 64} <= zd, f"drop opt {oi}: z-drop rows {sorted(zd)}"
        if o.zdrop <= 0 or oi == 0:
            assert {63, 99} <= m0, f"drop opt {oi}: m == 0 rows {sorted(m0)}"       # the 64th row, the target's last row
    if name == "qend":
        # (an option set whose band limit, ksw.c:436-443, keeps a query of 64 bases below 64 columns is left to the sweep of query lengths in fam_qend)
        mx = int(_mat(o).max())
        lim = min(int((64 * mx - o.o_ins) / o.e_ins + 1.), int((64 * mx - o.o_del) / o.e_del + 1.))
        assert qend_hit or lim < 63, f"qend opt {oi}: no case reaches the query's end on the row its band outgrows 64 columns"
    if name == "tlen":
        assert {63, 64, 65, 127, 128, 129} <= rows_done, f"tlen opt {oi}: rows computed {sorted(rows_done)}"


def run_family(dev, name):
    rng = np.random.default_rng(20261020)
    total = 0
    for oi, o in enumerate(_opts()):
        cs = FAMILIES[name](o, rng)
        for k, (q, t, w, h0, eb) in enumerate(cs.py):
            strong, rule = reaches_dp(o, q, t, h0)
            assert rule and (strong or len(q) == 1), f"{name} opt {oi} case {k}: the case would be answered by the diagonal rule (P {diag_loss(o, q, t)}, qlen {len(q)}, h0 {h0})"
        cases, seqs = cs.arrays()
        out = dev.debug_dp(o, 0, cases, seqs)
        assert int(out[:, 6].sum()) == 0, f"{name} opt {oi}: {int(out[:, 6].sum())} cases took the diagonal shortcut"
        for k, (q, t, w, h0, eb) in enumerate(cs.py):
            exp = ref_extend(o, q, t, w, h0, eb)
            assert out[k, :6].tolist() == exp, f"{name} opt {oi} case {k}: device {out[k, :8].tolist()} reference {exp} (qlen {len(q)} tlen {len(t)} w {w} h0 {h0} eb {eb} flags {cases['flags'][k]})"
        _coverage(name, oi, o, cs)
        total += len(cs.py)
    assert total >= 200, f"{name}: only {total} cases"


@pytest.fixture(scope="module")
def sim():
    import hostsim_build
    prefix, _ = testdata.small_index()
    s = BwaGpu(prefix, lib_path=hostsim_build.build())
    yield s
    s.close()


@pytest.fixture(scope="module")
def gpu():
    prefix, _ = testdata.small_index()
    g = BwaGpu(prefix)
    yield g
    g.close()


@pytest.mark.parametrize("name", list(FAMILIES))
def test_sim_extend_rows(sim, name):
    run_family(sim, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FAMILIES))
def test_gpu_extend_rows(gpu, name):
    run_family(gpu, name)
