"""Cases for the sort tests (test_sort_fuzz.py, test_oracle_vs_ref.py::test_introsort_fuzz): key arrangements at which a restatement of klib's
ks_introsort (ksort.h:176-226) goes wrong without a whole-read test noticing -- every size at which a form of the sort changes its method, every tie
pattern, and arrangements that run this particular quicksort out of its depth budget so that the comb sort (ksort.h:152-175) is entered.

A case is first a list of RANKS (small integers; equal ranks = equal keys); key_records() then maps ranks to the key fields of one order (`cls`) by a
mapping that is monotone for that order's comparator, so one arrangement serves every comparator, ascending or descending.  The depth-limit family is
built with McIlroy's adversary ("A killer adversary for quicksort", 1999) run against introsort_model(), a pure-Python restatement that also reports
whether the comb sort ran; generation asserts that it did for every case of that family.

Everything is seeded: the sim, gpu, host and oracle tests see the same cases (the CPU tests a thinned cross product of families and sizes: the stride
of the thinning never exceeds the number of families, so every size keeps a cell in every call of rank_cases, and the tests assert per setting that
every size asked for was compared)."""
import functools

import numpy as np

SORT_KEY_DTYPE = np.dtype([("a", "<i8"), ("b", "<i4"), ("c", "<i4")])

# the sizes at which some form changes its method: n = 2 (one compare), <= 16 (no quicksort pass), DEDUP_KEYSORT_MIN = 24, chain_sort_wave's 32, a
# wave's 64, dd_net's default 129, CW_FLT_LDS = 256, the networks' powers of two, ...
SIZES = (0, 1, 2, 3, 15, 16, 17, 18, 23, 24, 25, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 255, 256, 257, 511, 512, 513, 900, 1023, 1024, 1025)
DEPTH_SIZES = (100, 129, 200, 256, 513, 900, 1024)


# ---- the model ------------------------------------------------------------------------------------------------------------------------------------
def _comb(a, o, n, lt, stat):
    shrink = 1.2473309501039786540366528676643
    gap = n
    while True:
        if gap > 2:
            gap = int(gap / shrink)
            if gap in (9, 10):
                gap = 11
                stat["rule11"] += 1
        sw = False
        i = 0
        while i + gap < n:
            if lt(a[o + i + gap], a[o + i]):
                a[o + i], a[o + i + gap] = a[o + i + gap], a[o + i]
                sw = True
            i += 1
        if not (sw or gap > 2):
            break
    if gap != 1:                                   # (always: the gap never falls below 2)
        for i in range(o + 1, o + n):
            j = i
            while j > o and lt(a[j], a[j - 1]):
                a[j], a[j - 1] = a[j - 1], a[j]
                j -= 1


def introsort_model(a, lt, stat, on_comb=None):
    """ks_introsort on the list a, in place.  stat: comb (times the comb sort ran), sizes (of its ranges), rule11 (gap 9 / 10 -> 11 taken)."""
    n = len(a)
    if n < 1:
        return
    if n == 2:
        if lt(a[1], a[0]):
            a[0], a[1] = a[1], a[0]
        return
    d = 2
    while (1 << d) < n:
        d += 1
    d <<= 1
    stack = []
    s, t = 0, n - 1
    while True:
        if s < t:
            d -= 1
            if d == 0:
                stat["comb"] += 1
                stat["sizes"].append(t - s + 1)
                if on_comb:
                    on_comb(a[s:t + 1])
                _comb(a, s, t - s + 1, lt, stat)
                t = s
                continue
            i, j = s, t
            k = i + ((j - i) >> 1) + 1
            if lt(a[k], a[i]):
                if lt(a[k], a[j]):
                    k = j
            else:
                k = i if lt(a[j], a[i]) else j
            piv = a[k]
            if k != t:
                a[k], a[t] = a[t], a[k]
            while True:
                i += 1
                while lt(a[i], piv):
                    i += 1
                j -= 1
                while i <= j and lt(piv, a[j]):
                    j -= 1
                if j <= i:
                    break
                a[i], a[j] = a[j], a[i]
            a[i], a[t] = a[t], a[i]
            if i - s > t - i:
                if i - s > 16:
                    stack.append((s, i - 1, d))
                s = i + 1 if t - i > 16 else t
            else:
                if t - i > 16:
                    stack.append((i + 1, t, d))
                t = i - 1 if i - s > 16 else s
        else:
            if not stack:
                break
            s, t, d = stack.pop()
    for i in range(1, n):
        j = i
        while j > 0 and lt(a[j], a[j - 1]):
            a[j], a[j - 1] = a[j - 1], a[j]
            j -= 1


def _new_stat():
    return {"comb": 0, "sizes": [], "rule11": 0, "ties_in_comb": 0}


def model_stat(ranks):
    """What introsort_model does with this arrangement (ties_in_comb: comb-sorted ranges that held equal keys)."""
    st = _new_stat()

    def on_comb(rng_):
        if len(set(v for v, _ in rng_)) < len(rng_):
            st["ties_in_comb"] += 1
    a = [(v, i) for i, v in enumerate(ranks)]
    introsort_model(a, lambda x, y: x[0] < y[0], st, on_comb)
    assert [v for v, _ in a] == sorted(ranks)
    return st


@functools.lru_cache(maxsize=None)
def adversary(n):
    """McIlroy's adversary against introsort_model: values are decided only when a comparison needs them, always so that the pivot is poor."""
    gas = n
    val = [gas] * n
    st = {"nsolid": 0, "cand": 0}

    def lt(x, y):
        if val[x] == gas and val[y] == gas:
            if x == st["cand"]:
                val[x] = st["nsolid"]
            else:
                val[y] = st["nsolid"]
            st["nsolid"] += 1
        if val[x] == gas:
            st["cand"] = x
        elif val[y] == gas:
            st["cand"] = y
        return val[x] < val[y]
    introsort_model(list(range(n)), lt, _new_stat())
    for i in range(n):
        if val[i] == gas:
            val[i] = st["nsolid"]
            st["nsolid"] += 1
    return tuple(val)


# ---- arrangements of ranks --------------------------------------------------------------------------------------------------------------------------
def _organ(n):
    return [min(i, n - 1 - i) for i in range(n)]


PATTERNS = {
    "equal": lambda n, r: [0] * n,
    "two": lambda n, r: r.integers(0, 2, size=n).tolist(),
    "three": lambda n, r: r.integers(0, 3, size=n).tolist(),
    "five": lambda n, r: r.integers(0, 5, size=n).tolist(),
    "ties50": lambda n, r: r.integers(0, max(1, n // 2), size=n).tolist(),
    "random": lambda n, r: r.permutation(n).tolist(),
    "asc": lambda n, r: list(range(n)),
    "desc": lambda n, r: list(range(n - 1, -1, -1)),
    "asc_low_last": lambda n, r: list(range(1, n)) + [0] if n else [],
    "asc_high_first": lambda n, r: [n] + list(range(n - 1)) if n else [],
    "organ": lambda n, r: _organ(n),
    "saw2": lambda n, r: [i % 2 for i in range(n)],
    "saw16": lambda n, r: [i % 16 for i in range(n)],
    "saw17": lambda n, r: [i % 17 for i in range(n)],
    "realistic": lambda n, r: np.minimum(r.geometric(0.25, size=n) - 1, 41).tolist(),       # a handful of values, the smallest the commonest
}
FAMILIES = tuple(PATTERNS) + ("depth", "depth_tied")


class Case:
    __slots__ = ("family", "ranks", "stat", "special", "decline", "mode")

    def __init__(self, family, ranks, stat=None, special=None, decline=False, mode=0):
        self.family, self.ranks, self.stat, self.special, self.decline, self.mode = family, ranks, stat, special, decline, mode

    @property
    def n(self):
        return len(self.special) if self.special is not None else len(self.ranks)


@functools.lru_cache(maxsize=None)
def depth_cases(sizes, max_tied=3):
    """Per size: the adversary's arrangement, and up to max_tied tied variants (neighbouring ranks merged) for which the model still enters the comb sort."""
    out = []
    for n in sizes:
        v = list(adversary(n))
        st = model_stat(v)
        assert st["comb"] > 0, f"the adversary does not reach the depth limit at n = {n}"
        out.append(Case("depth", v, st))
        tied = 0
        for div in (3, 2, 5):
            if tied == max_tied:
                break
            vt = [x // div for x in v]
            st = model_stat(vt)
            if st["comb"] > 0:
                out.append(Case("depth_tied", vt, st))
                tied += 1
        assert tied > 0, f"no tied variant of the adversary's arrangement reaches the depth limit at n = {n}"
    return tuple(out)


def rank_cases(seed, sizes=SIZES, depth_sizes=DEPTH_SIZES, thin=1, reps=1, max_tied=3):
    """The cross product of PATTERNS and sizes, `reps` draws of each, and the depth-limit family.  thin > 1: every stride-th cell of the cross product along
    its diagonals, stride = min(thin, number of families) -- so every size keeps at least one family, and (with at least as many sizes as families) every
    family a size.  Case.mode, which key_records() takes, rotates with the cell (size index + 2 * family index) and along the depth-limit cases."""
    rng = np.random.default_rng(seed)
    stride = max(1, min(thin, len(PATTERNS)))
    out = []
    for rep in range(reps):
        for si, n in enumerate(sizes):
            for fi, fam in enumerate(PATTERNS):
                if (si + fi + rep) % stride:
                    continue
                out.append(Case(fam, [int(x) for x in PATTERNS[fam](n, rng)], mode=si + 2 * fi + rep))
    out += [Case(c.family, c.ranks, c.stat, mode=j) for j, c in enumerate(depth_cases(tuple(depth_sizes), max_tied))]
    return out


def requested_sizes(sizes=SIZES, depth_sizes=DEPTH_SIZES):
    return sorted(set(sizes) | set(depth_sizes))


# ---- ranks -> key records -----------------------------------------------------------------------------------------------------------------------------
# orders (cls): "u64" score << 32 | index ascending (b = score); "intv" info ascending (a); "chainw" weight descending (b); "end" re ascending (a);
# "best" score descending, rb, qb ascending (b, a, c); "hash" score descending, is_alt, hash ascending (b, c, a); "hash2" is_alt, score descending, hash
# (c, b, a); "pair" x, y ascending (a, b : c); "u64raw" a ascending
BEST_RB = (0, (1 << 16) - 1, 1 << 16, (1 << 32) - 1, 1 << 32, (1 << 48) - 1)
BEST_QB = (0, 1, 65534, 65535)
BEST_SCORE = (1 << 30, 1, 0, -1, -(1 << 31) + 1)                      # (in sorted order: descending)
END_RE = (0, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 48) - 1, 1 << 62)


N_MODES = {"u64": 2, "intv": 3, "u64raw": 3, "chainw": 2, "end": 4, "best": 5, "hash": 2, "hash2": 1, "pair": 2}      # key_records' modes per order


def key_records(cls, ranks, mode=0):
    """ranks -> SORT_KEY_DTYPE records such that x sorts before y in order `cls` exactly when rank(x) < rank(y).  mode picks which field carries the
    order (and where in its range the values lie)."""
    r = np.asarray(ranks, dtype=np.int64)
    k = np.zeros(r.shape[0], dtype=SORT_KEY_DTYPE)
    top = int(r.max()) if r.shape[0] else 0
    if cls == "u64":
        k["b"] = r if mode % 2 == 0 else r - (top + 1)              # mode 1: scores -top-1 .. -1, keys just below the networks' padding value ~0
        k["a"] = 7
    elif cls in ("intv", "u64raw"):
        # (mode 2: the largest keys there are short of ~0ull, which the networks pad with; a real key of ~0ull cannot occur -- info's low word is a read offset)
        k["a"] = (r, r << 32 | 5, r - (top + 2))[mode % 3]
    elif cls == "chainw":
        k["b"] = ((60 if top <= 41 else top + 19) - r, (1 << 29) - 1 - r)[mode % 2]      # realistic weights 19 .. 60; the bit-field's upper end
    elif cls == "end":
        m = mode % 4
        if m == 3 and top < len(END_RE):
            k["a"] = np.asarray(END_RE, dtype=np.int64)[r]
        else:
            k["a"] = (1000 + r * 37, (1 << 32) - 3 + r, (1 << 48) - 1 - top + r, 1000 + r)[m]     # clustered within max_chain_gap; across bit 32; up to 2^48 - 1
        k["b"] = 50
    elif cls == "best":
        m = mode % 5
        k["b"], k["a"], k["c"] = 60, 123456, 30
        if m == 0:
            k["b"] = 100 - r if top <= 100 else (1 << 30) - r
        elif m == 1:
            k["a"] = (1 << 16) - 1 - min(top, 65535) // 2 + r     # rb differing below bit 16, and across it
        elif m == 2:
            k["a"] = ((1 << 31) - top // 2 + r) << 16 | 0xffff      # rb differing only in bits 16 .. 47
        elif m == 3:
            k["c"] = 65535 - top + r if top <= 65535 else r       # qb up to 65535
        else:                                                        # all three, the two rb halves and qb at their edges
            k["b"] = (1 << 30) - r // 24
            k["a"] = np.asarray(BEST_RB, dtype=np.int64)[(r // 4) % 6]
            k["c"] = np.asarray(BEST_QB, dtype=np.int64)[r % 4]
    elif cls == "hash":
        k["b"] = 1000 - r // 4
        k["c"] = (r // 2) % 2
        k["a"] = (r % 2) * (np.int64(1) << 62) + 5 if mode % 2 else (r % 2)
    elif cls == "hash2":
        half = top // 2 + 1
        k["c"] = r // half
        k["b"] = 1000000 - (r % half) // 2
        k["a"] = (r % half) % 2 * (np.int64(1) << 62) + 9
    elif cls == "pair":
        k["a"] = (r // 4) << (33 if mode % 2 else 0)
        k["b"] = (r // 2) % 2
        k["c"] = r % 2
    else:
        raise ValueError(cls)
    return k


def best_boundary_cases(seed, n_cases):
    """ddp_key_best's field boundaries: draws (with repeats: ties) from the cross product of the edge values of score, rb and qb, runs that differ only in
    rb's low 16 bits, only in its bits above, only in qb -- and the coordinates the packed key cannot hold (rb = 2^48, rb < 0, qb = 65536, qb < 0), for
    which dedup_read_par must decline."""
    rng = np.random.default_rng(seed)
    out = []
    bad = ((1 << 48, 0), (-1, 0), (5, 65536), (5, -1))
    for it in range(n_cases):
        n = int(rng.choice([2, 2, 3, 5, 16, 17, 24, 33, 64, 65, 129, 130, 200]))
        k = np.zeros(n, dtype=SORT_KEY_DTYPE)
        what = it % 6
        k["b"] = rng.choice(BEST_SCORE, size=n) if what in (0, 5) else int(rng.choice(BEST_SCORE))
        k["a"] = rng.choice(BEST_RB, size=n) if what in (0, 5) else int(rng.choice(BEST_RB))
        k["c"] = rng.choice(BEST_QB, size=n) if what in (0, 5) else int(rng.choice(BEST_QB))
        if what == 1:
            k["a"] = (int(rng.choice([0, 1 << 16, 1 << 32, ((1 << 32) - 1) << 16])) | rng.integers(0, 1 << 16, size=n)) if it % 2 else rng.choice([65534, 65535, 65536, 65537], size=n)
        elif what == 2:
            k["a"] = rng.integers(0, 1 << 32, size=n) << 16 | int(rng.integers(0, 1 << 16))
        elif what == 3:
            k["c"] = rng.choice([0, 1, 2, 65533, 65534, 65535], size=n)
        elif what == 4:
            k["b"] = rng.choice([-(1 << 31) + 1, -(1 << 31) + 2, -1, 0, 1, (1 << 30) - 1, 1 << 30], size=n)
        decline = what == 5
        if decline:
            rb, qb = bad[(it // 6) % 4]
            at = int(rng.integers(0, n))
            k["a"][at], k["c"][at] = rb, qb
        out.append(Case("best_decline" if decline else "best_boundary", None, special=k, decline=decline))
    return out


def build(cls, seed, thin=1, reps=1, extra_sizes=(), extra_depth=(), boundary=0, max_tied=3):
    """[(Case, records)] for order `cls`: every rank case through the key_records mode it names, plus (cls "best") the boundary cases."""
    out = []
    cases = rank_cases(seed, tuple(SIZES) + tuple(extra_sizes), tuple(DEPTH_SIZES) + tuple(extra_depth), thin, reps, max_tied)
    for c in cases:
        out.append((c, key_records(cls, c.ranks, mode=c.mode)))
    if cls == "best":
        out += [(c, c.special) for c in best_boundary_cases(seed + 1, boundary)]
    if cls == "end":
        out += end_edge_cases(seed)
    return out


def end_edge_cases(seed):
    """the bias of ddp_key_end (re ^ 1 << 63) at its edge values"""
    rng = np.random.default_rng(seed + 2)
    out = []
    for n in (2, 3, 17, 64, 130):
        r = rng.integers(0, len(END_RE), size=n).tolist()
        out.append((Case("end_edges", r), key_records("end", r, mode=3)))
    return out


def flatten(recs):
    """[(Case, records)] -> (keys, off) as bwagpu_debug_sort takes them"""
    off = np.zeros(len(recs) + 1, dtype=np.int64)
    for i, (_, k) in enumerate(recs):
        off[i + 1] = off[i] + k.shape[0]
    keys = np.concatenate([k for _, k in recs]) if recs else np.zeros(0, dtype=SORT_KEY_DTYPE)
    return np.ascontiguousarray(keys), off
