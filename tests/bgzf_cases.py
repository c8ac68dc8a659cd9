"""BGZF inputs for the device inflate's tests (tests/test_bgzf.py, tests/test_gpu_bgzf.py): a BGZF writer, a DEFLATE bit writer for the
streams zlib's compressor never emits, the corpus of valid and damaged blocks, FASTQ files written as BGZF, and the runs both test files
share.  The oracle is zlib (decompressobj(-15), crc32) behind the block test of the SAM specification 4.1 as BgzfPipe::block_len of
bwa_amd/csrc/host/host_input.h applies it -- never the code under test.  The corpus checks itself against that oracle at import."""
import struct
import zlib

import numpy as np

import fastq_cases

MAX_ISIZE = 65536


# ---- BGZF ------------------------------------------------------------------------------------------------------------------------
def bgzf_block(payload: bytes, isize: int, crc: int, pre: bytes = b"", bc: bool = True, bsize=None) -> bytes:
    """one block: pre = extra subfields ahead of BC; bsize overrides the BSIZE field (total length - 1)"""
    xlen = len(pre) + (6 if bc else 0)
    total = 12 + xlen + len(payload) + 8
    extra = pre + (b"BC\x02\x00" + struct.pack("<H", ((total - 1) if bsize is None else bsize) & 0xffff) if bc else b"")
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra + payload + struct.pack("<II", crc & 0xffffffff, isize & 0xffffffff)


def deflate(text: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY) -> bytes:
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return co.compress(text) + co.flush()


def block_of(text: bytes, payload: bytes = None, level: int = 6, **kw) -> bytes:
    return bgzf_block(deflate(text, level) if payload is None else payload, len(text), zlib.crc32(text), **kw)


EOF_MARKER = block_of(b"")
assert EOF_MARKER == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")      # bgzip's 28 bytes


def block_len(p: bytes) -> int:
    """BgzfPipe::block_len: the total length of the block that starts p, 0 if none lies within p"""
    n = len(p)
    if n < 18 or p[0] != 0x1f or p[1] != 0x8b or p[2] != 8 or not p[3] & 4:
        return 0
    xlen = p[10] | p[11] << 8
    if 12 + xlen > n:
        return 0
    o = 12
    while o + 4 <= 12 + xlen:
        sl = p[o + 2] | p[o + 3] << 8
        if p[o:o + 2] == b"BC" and sl == 2 and o + 6 <= 12 + xlen:
            bs = (p[o + 4] | p[o + 5] << 8) + 1
            return bs if 12 + xlen + 8 <= bs <= n else 0
        o += 4 + sl
    return 0


def oracle_block(p: bytes):
    """the text of the whole block p as BgzfPipe::inflate_group accepts it, or None"""
    xlen = p[10] | p[11] << 8
    crc, isize = struct.unpack("<II", p[-8:])
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(p[12 + xlen:-8])
    except zlib.error:
        return None
    if not d.eof or len(text) != isize or zlib.crc32(text) != crc:      # (unused_data behind the final block is allowed)
        return None
    return text


def oracle_window(comp: bytes, eof: bool = True):
    """(text of the whole blocks, their number, bytes they cover, offset of the first damage or -1): what the library must say of a window"""
    o, texts = 0, []
    while o < len(comp):
        bl = block_len(comp[o:])
        if not bl:
            break
        t = oracle_block(comp[o:o + bl])
        if t is None:
            return None, len(texts), o, o
        texts.append(t)
        o += bl
    if o < len(comp) and eof:
        return None, len(texts), o, o
    return b"".join(texts), len(texts), o, -1


# ---- a DEFLATE bit writer ----------------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):
        """n bits of v, least significant first (header fields, extra bits)"""
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):
        """a Huffman code: most significant bit first"""
        for i in range(n - 1, -1, -1):
            self.put(c >> i & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


def canonical(lens):
    """RFC 1951 3.2.2: symbol -> (code, length)"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l] & ((1 << l) - 1), l)
            nxt[l] += 1
    return out


CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
CL_LENS = [4] * 13 + [5] * 6                 # a complete code over all 19 code-length symbols
CL_EXTRA = {16: 2, 17: 3, 18: 7}
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def _symbols(w, ll, dd, symbols):
    """symbols: (kind, symbol, extra value, extra bits), kind "L" (literal/length alphabet) or "D" (distance alphabet)"""
    for kind, s, xv, xb in symbols:
        c, n = (ll if kind == "L" else dd)[s]
        w.code(c, n)
        w.put(xv, xb)


def lit(b):
    return [("L", x, 0, 0) for x in b]


EOB = ("L", 256, 0, 0)


def stored(w, data, final=1, nlen=None):
    w.put(final, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put((len(data) ^ 0xffff) if nlen is None else nlen, 16)
    for b in data:
        w.put(b, 8)


def fixed(w, symbols, final=1):
    w.put(final, 1)
    w.put(1, 2)
    _symbols(w, canonical(FIXED_LL), canonical(FIXED_D), symbols)


def dynamic(w, ll_lens, d_lens, symbols, final=1, cl_seq=None, hlit=None, hdist=None):
    """a dynamic block from code lengths; cl_seq: the code-length symbols to send, (symbol,) or (16 / 17 / 18, extra value) -- default one per length"""
    w.put(final, 1)
    w.put(2, 2)
    w.put(len(ll_lens) - 257 if hlit is None else hlit, 5)
    w.put(len(d_lens) - 1 if hdist is None else hdist, 5)
    w.put(19 - 4, 4)
    for s in CL_ORDER:
        w.put(CL_LENS[s], 3)
    cl = canonical(CL_LENS)
    for e in (cl_seq if cl_seq is not None else [(l,) for l in list(ll_lens) + list(d_lens)]):
        w.code(*cl[e[0]])
        if e[0] >= 16:
            w.put(e[1], CL_EXTRA[e[0]])
    _symbols(w, canonical(ll_lens), canonical(d_lens), symbols)


def _ll(n, **lens):
    out = [0] * n
    for k, v in lens.items():
        out[int(k[1:])] = v
    return out


# ---- the corpus --------------------------------------------------------------------------------------------------------------------
def _fastq_text(rng, n_bytes):
    out = []
    i = 0
    while sum(len(x) for x in out) < n_bytes:
        l = int(rng.integers(30, 152))
        out.append(b"@read%d/1 BC:Z:%d\n" % (i, i * 7) + fastq_cases._acgt(rng, l) + b"\n+\n" + bytes(rng.integers(33, 74, l).astype(np.uint8)) + b"\n")
        i += 1
    return b"".join(out)[:n_bytes]


def _valid_cases():
    rng = np.random.default_rng(1951)
    fq = _fastq_text(rng, 0xff00)
    small = fq[:3000]
    c = {}

    def z(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
        return text, block_of(text, deflate(text, level, strategy))

    c["stored"] = z(small, 0)
    c["fixed"] = z(small, 6, zlib.Z_FIXED)
    for lv in (1, 6, 9):
        c[f"dynamic_level{lv}"] = z(fq[:20000], lv)
    c["huffman_only"] = z(small, 6, zlib.Z_HUFFMAN_ONLY)
    c["rle"] = z(small + b"A" * 700 + small[:500], 6, zlib.Z_RLE)
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    flushed = co.compress(fq[:1500]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(fq[1500:1600]) + co.flush(zlib.Z_SYNC_FLUSH) + co.flush(zlib.Z_SYNC_FLUSH) + \
        co.compress(fq[1600:5000]) + co.flush(zlib.Z_FULL_FLUSH) + co.flush()
    c["flushes"] = (fq[:5000], block_of(fq[:5000], flushed))
    c["isize_0"] = z(b"")
    c["isize_1"] = z(b"x")
    c["isize_ff00"] = z(fq)
    c["isize_65536"] = z((fq + fq[:256])[:65536])
    # a BGZF block holds 65536 bytes with header and trailer: 65536 bytes that do not compress at all cannot be one.  Random bytes of 192
    # values take 7.6 bits each (Huffman codes, no matches); 60000 random bytes of all values go as stored blocks
    c["random_65536"] = z(bytes(rng.integers(0, 192, 65536).astype(np.uint8)))
    c["random_stored"] = z(bytes(rng.integers(0, 256, 60000).astype(np.uint8)))
    c["run_60000"] = z(b"G" * 60000)
    c["slack_bytes"] = (small, block_of(small, deflate(small) + b"\x07\xff\x00"))
    c["bc_behind_another_subfield"] = (small, block_of(small, pre=b"XY\x03\x00abc"))
    # -- streams from the bit writer
    w = Bits()      # lengths 1, 2, ..., 14, 15, 15 over sixteen symbols: 'a' .. 'o' and 256 (two 15-bit codes: 'o' and 256)
    ll = [0] * 257
    for i in range(15):
        ll[ord("a") + i] = i + 1
    ll[256] = 15
    text = bytes(rng.permutation(np.frombuffer(b"abcdefghijklmno" * 3 + b"aaaaabbbccd", dtype=np.uint8)))
    dynamic(w, ll, [0], lit(text) + [EOB])
    c["codes_of_15_bits"] = (text, block_of(text, w.bytes()))
    w = Bits()      # one distance code of one bit (incomplete, allowed): a literal and a match of 258 at distance 1
    dynamic(w, _ll(286, s65=1, s256=2, s285=2), [1], [("L", 65, 0, 0), ("L", 285, 0, 0), ("D", 0, 0, 0), EOB])
    c["one_distance_code"] = (b"A" * 259, block_of(b"A" * 259, w.bytes()))
    w = Bits()      # a repeat of six that runs from literal/length symbols 256 - 257 into distance symbols 0 - 3
    dynamic(w, _ll(258, s65=2, s255=2, s256=2, s257=2), [2, 2, 2, 2], [("L", 65, 0, 0), ("L", 65, 0, 0), ("L", 257, 0, 0), ("D", 1, 0, 0), EOB],
            cl_seq=[(18, 65 - 11), (2,), (18, 138 - 11), (18, 51 - 11), (2,), (16, 6 - 3)])
    c["repeat_across_alphabets"] = (b"AAAAA", block_of(b"AAAAA", w.bytes()))
    w = Bits()      # 32768 literals, a match at distance 32768 (symbol 29, extra 8191), one at distance 1 behind it
    lits = bytes(rng.integers(0, 144, 32768).astype(np.uint8))
    fixed(w, lit(lits) + [("L", 285, 0, 0), ("D", 29, 8191, 13), ("L", 257, 0, 0), ("D", 0, 0, 0), EOB])
    text = lits + lits[:258] + lits[257:258] * 3
    c["distance_32768"] = (text, block_of(text, w.bytes()))
    return c


def _damaged_cases(valid):
    small, small_block = valid["dynamic_level6"][0][:3000], None
    small_block = block_of(small)
    pay = deflate(small)
    c = {}

    def raw(w, text=b"x"):
        return block_of(text, w.bytes() + b"\0" * 8)

    w = Bits(); w.put(1, 1); w.put(3, 2); c["block_type_3"] = raw(w)
    w = Bits(); stored(w, b"abc", nlen=0xfffd); c["len_nlen_mismatch"] = raw(w, b"abc")
    w = Bits(); w.put(1, 1); w.put(2, 2); w.put(30, 5); w.put(0, 5); w.put(15, 4); c["hlit_287"] = raw(w)
    w = Bits(); w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(30, 5); w.put(15, 4); c["hdist_31"] = raw(w)
    w = Bits(); dynamic(w, _ll(257, s120=1, s121=1, s256=1), [0], [("L", 120, 0, 0), EOB]); c["oversubscribed_literal_code"] = raw(w)
    w = Bits(); dynamic(w, _ll(257, s120=1, s256=1), [2, 2], [("L", 120, 0, 0), EOB]); c["incomplete_distance_code"] = raw(w)
    w = Bits(); dynamic(w, _ll(257, s120=1, s121=1), [0], [("L", 120, 0, 0)]); c["no_symbol_256"] = raw(w)
    w = Bits(); fixed(w, lit(b"x") + [("L", 286, 0, 0), ("D", 0, 0, 0), EOB]); c["fixed_symbol_286"] = raw(w)
    w = Bits(); fixed(w, lit(b"x") + [("L", 257, 0, 0), ("D", 30, 0, 0), EOB]); c["distance_symbol_30"] = raw(w, b"xxxx")
    w = Bits(); fixed(w, lit(b"x") + [("L", 257, 0, 0), ("D", 1, 0, 0), EOB]); c["distance_before_the_start"] = raw(w, b"xxxx")
    c["payload_cut_in_a_symbol"] = block_of(small, pay[:len(pay) - 7])
    c["isize_plus_1_bytes"] = bgzf_block(deflate(small + b"x"), len(small), zlib.crc32(small))
    c["isize_minus_1_bytes"] = bgzf_block(deflate(small[:-1]), len(small), zlib.crc32(small))
    c["crc_off_by_one_bit"] = bgzf_block(pay, len(small), zlib.crc32(small) ^ 0x100)
    c["isize_65537"] = bgzf_block(pay, 65537, zlib.crc32(small))
    c["isize_ffffffff"] = bgzf_block(pay, 0xffffffff, zlib.crc32(small))
    c["bsize_past_the_window"] = block_of(small, bsize=0xffff)
    c["header_without_bc"] = block_of(small, pre=b"XY\x02\x00ab", bc=False)
    assert oracle_block(small_block) == small
    return c


MUTATION_SEED = 7
N_MUTATIONS = 200


def _mutations(valid):
    """single-byte mutations of small valid blocks; the oracle sorts them: {name: block} damaged, {name: (text, block)} still valid"""
    rng = np.random.default_rng(MUTATION_SEED)
    bases = [valid[k][1] for k in ("stored", "fixed", "huffman_only", "rle", "flushes", "codes_of_15_bits", "repeat_across_alphabets", "slack_bytes")]
    bad, good = {}, {}
    for i in range(N_MUTATIONS):
        b = bytearray(bases[i % len(bases)])
        at = int(rng.integers(0, len(b)))
        b[at] ^= int(rng.integers(1, 256))
        b = bytes(b)
        t = oracle_block(b) if block_len(b) == len(b) else None
        if t is None:
            bad[f"mutation_{i}_byte_{at}"] = b
        else:
            good[f"mutation_{i}_byte_{at}"] = (t, b)
    return bad, good


VALID = _valid_cases()
DAMAGED = _damaged_cases(VALID)
_mut_bad, _mut_good = _mutations(VALID)
assert len(_mut_good) <= N_MUTATIONS // 20, f"{len(_mut_good)} of {N_MUTATIONS} mutations are still valid: choose another seed"
DAMAGED.update(_mut_bad)
VALID.update(_mut_good)
FILLER = [VALID[k][1] for k in ("isize_1", "fixed", "isize_0", "huffman_only")]      # small valid blocks around a planted one

# the corpus checks itself
for _name, (_text, _blk) in VALID.items():
    assert len(_blk) <= 65536 and len(_text) <= MAX_ISIZE and block_len(_blk) == len(_blk) and oracle_block(_blk) == _text, _name
for _name, _blk in DAMAGED.items():
    assert oracle_window(_blk, True)[3] == 0, _name
assert zlib.decompressobj(-15).decompress(VALID["slack_bytes"][1][18:-8]) == VALID["slack_bytes"][0]
_d = zlib.decompressobj(-15); _d.decompress(VALID["slack_bytes"][1][18:-8]); assert _d.unused_data == b"\x07\xff\x00"


def planted(name, where):
    """(window, offset of the planted block): DAMAGED[name] as block 0, as block 3 of 5, or as the last of 5"""
    b = DAMAGED[name]
    if where == "first":
        blocks = [b] + FILLER
    elif where == "middle":
        blocks = FILLER[:3] + [b] + FILLER[3:]
    else:
        blocks = FILLER + [b]
    at = sum(len(x) for x in blocks[:blocks.index(b)])
    return b"".join(blocks), at


# ---- FASTQ files as BGZF -------------------------------------------------------------------------------------------------------------
def bgzf_file(text: bytes, sizes="random", seed=0, eof_marker=True, oddities=True) -> bytes:
    """sizes "random": blocks of 1 .. 4000 text bytes, with one-byte and empty blocks in the middle; an int: blocks of that many text bytes"""
    rng = np.random.default_rng(seed)
    out, o, i = [], 0, 0
    while o < len(text):
        n = int(rng.integers(1, 4001)) if sizes == "random" else int(sizes)
        if sizes == "random" and oddities and i % 5 == 2:
            out.append(EOF_MARKER if i % 2 else block_of(b"", level=1))      # an empty block in the middle
            n = 1                                                            # and a block of one byte
        out.append(block_of(text[o:o + n], level=(1, 6, 9)[i % 3]))
        o += n
        i += 1
    if eof_marker:
        out.append(EOF_MARKER)
    return b"".join(out)


def bgzf_case(case, sizes="random", eof_marker=True):
    return [bgzf_file(f, sizes, seed=17 + k, eof_marker=eof_marker) for k, f in enumerate(case["files"])]


# ---- the runs ------------------------------------------------------------------------------------------------------------------------
def check_inflate(parser, comp, eof=True):
    """inflate_bgzf against the oracle on one window"""
    want, n_blocks, used, bad_at = oracle_window(comp, eof)
    text, info = parser.inflate_bgzf(comp, eof=eof)
    assert info["damaged_at"] == bad_at, (info, bad_at)
    if bad_at >= 0:
        assert text is None
        return info
    assert text == want and info["inflated"] == len(want) and info["n_blocks"] == n_blocks and info["used_comp"] == used, info
    return info


def run_chain(parser, case, comp, chunk, window=None, compare_plain=False):
    """batch_bgzf from the start of the files to END, each call's window starting at the virtual offset the call before left: the batches
    are bseq_read's on the plain text, consumed sums to the text's length.  window: compressed bytes per window (doubled on MORE), None: the rest
    of the file.  compare_plain: every call's arrays equal parser.batch's on the plain text of the same window"""
    from bwa_amd import api
    want = fastq_cases.ref_batches(case, chunk)
    files, nf = case["files"], len(case["files"])
    coff, uoff, tpos = [0] * nf, [0] * nf, [0] * nf
    n_more = 0
    for bi in range(len(want) + 1):
        win = window
        while True:
            ends = [len(c) if win is None else min(len(c), o + win) for c, o in zip(comp, coff)]
            eof = tuple(e == len(c) for e, c in zip(ends, comp)) + (True,) * (2 - nf)
            r = parser.batch_bgzf(comp[0][coff[0]:ends[0]], comp[1][coff[1]:ends[1]] if nf > 1 else None, skip=tuple(uoff) + (0,) * (2 - nf), chunk_size=chunk, eof=eof)
            if r["status"] != api.FQ_MORE:
                break
            assert win is not None and not all(eof), "MORE with every file's end in the window"
            n_more += 1
            win *= 2
        assert r["status"] in (api.FQ_CUT, api.FQ_END), (bi, r["status"], r["declined_file"], r["declined_at"], r["bgzf"])
        assert all(i["damaged_at"] == -1 for i in r["bgzf"])
        if compare_plain:
            texts = [oracle_window(c[o:e], False)[0][u:] for c, o, e, u in zip(comp, coff, ends, uoff)]
            assert all(t == f[p:p + len(t)] for t, f, p in zip(texts, files, tpos))
            q = parser.batch(texts[0], texts[1] if nf > 1 else None, chunk_size=chunk, eof=eof)
            assert q["status"] == r["status"] and q["consumed"] == r["consumed"] and q["n_reads"] == r["n_reads"]
            for k in ("seqs", "off", "name_off", "comment_off", "has_comment", "recs"):
                assert np.array_equal(r[k], q[k]), (k, bi)
            assert (r["names"], r["comments"], r["quals"]) == (q["names"], q["comments"], q["quals"])
        if bi == len(want):
            assert r["status"] == api.FQ_END and r["n_reads"] == 0
            break
        assert fastq_cases.device_records(r) == want[bi], f"batch {bi}"
        for k in range(nf):
            i = r["bgzf"][k]
            tpos[k] += r["consumed"][k]
            # the virtual offset is normalised, and it is where the text position says
            assert 0 <= i["next_coff"] <= i["used_comp"] and (i["next_uoff"] == 0 if i["next_coff"] == i["used_comp"] else True), i
            if i["next_coff"] < i["used_comp"]:
                b = comp[k][coff[k] + i["next_coff"]:]
                assert i["next_uoff"] < struct.unpack("<I", b[block_len(b) - 4:block_len(b)])[0], i
            coff[k] += i["next_coff"]
            uoff[k] = i["next_uoff"]
            assert len(oracle_window(comp[k][:coff[k]], False)[0]) + uoff[k] == tpos[k], (k, bi)
        if r["status"] == api.FQ_END:
            assert bi == len(want) - 1
            break
    assert all(p == len(f) for p, f in zip(tpos, files))
    return n_more


def run_irregular(parser, case, comp, chunk):
    """the batches before the planted record are bseq_read's, the batch that holds it is declined at the record's offset in the text window"""
    from bwa_amd import api
    want = fastq_cases.ref_batches(case, chunk)
    files, nf = case["files"], len(case["files"])
    coff, uoff, tpos, taken = [0] * nf, [0] * nf, [0] * nf, 0
    for bi in range(len(want) + 1):
        r = parser.batch_bgzf(comp[0][coff[0]:], comp[1][coff[1]:] if nf > 1 else None, skip=tuple(uoff) + (0,) * (2 - nf), chunk_size=chunk)
        b = want[bi] if bi < len(want) else None
        whole = b is not None and (taken + len(b)) // nf <= case["k"] and len(b) % 2 == 0 and sum(len(x[2]) for x in b) >= chunk
        if not whole:
            assert r["status"] == api.FQ_DECLINED and r["n_reads"] == 0 and "seqs" not in r, (bi, r["status"])
            assert r["declined_file"] == case["file"] and tpos[case["file"]] + r["declined_at"] == case["at"], (r["declined_file"], r["declined_at"], tpos, case["at"])
            return bi
        assert r["status"] == api.FQ_CUT and fastq_cases.device_records(r) == b, f"batch {bi}"
        taken += r["n_reads"]
        for k in range(nf):
            tpos[k] += r["consumed"][k]
            coff[k] += r["bgzf"][k]["next_coff"]
            uoff[k] = r["bgzf"][k]["next_uoff"]
    raise AssertionError("the device never declined")


def run_windows(parser, plain):
    """the result does not depend on the compressed window's length once the window reaches the cut; shorter windows give MORE first"""
    from bwa_amd import api
    rng = np.random.default_rng(9)
    for name, chunk in (("cycle", 1000), ("pairs_cycle", 700)):
        case = plain[name]
        comp = bgzf_case(case)
        nf = len(comp)
        whole = parser.batch_bgzf(comp[0], comp[1] if nf > 1 else None, chunk_size=chunk)
        assert whole["status"] == api.FQ_CUT
        need = [i["next_coff"] + (block_len(c[i["next_coff"]:]) if i["next_uoff"] else 0) for i, c in zip(whole["bgzf"], comp)]      # (the blocks the batch's text lies in)
        for _ in range(6):      # windows that reach the cut and end anywhere behind it, inside a block as a rule
            lens = [int(rng.integers(n, len(c) + 1)) for n, c in zip(need, comp)]
            r = parser.batch_bgzf(comp[0][:lens[0]], comp[1][:lens[1]] if nf > 1 else None, chunk_size=chunk, eof=tuple(n == len(c) for n, c in zip(lens, comp)) + (True,) * (2 - nf))
            assert r["status"] == api.FQ_CUT and r["consumed"] == whole["consumed"], lens
            for k in ("seqs", "off", "name_off", "comment_off", "has_comment", "recs"):
                assert np.array_equal(r[k], whole[k]), (k, lens)
            assert (r["names"], r["comments"], r["quals"]) == (whole["names"], whole["comments"], whole["quals"])
            assert [(i["next_coff"], i["next_uoff"]) for i in r["bgzf"]] == [(i["next_coff"], i["next_uoff"]) for i in whole["bgzf"]]
        for short in (need[0] // 2, 40, 0):      # windows that stop short of the cut: MORE first
            r = parser.batch_bgzf(comp[0][:short], comp[1] if nf > 1 else None, chunk_size=chunk, eof=(False, True))
            assert r["status"] == api.FQ_MORE and r["n_reads"] == 0 and "seqs" not in r, short
        assert run_chain(parser, case, comp, chunk, window=100) > 0


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def write_bgzf(path, text, sizes=0xff00, **kw):
    with open(path, "wb") as f:
        f.write(bgzf_file(text, sizes, **kw))
    return path


def dump_corpus(path):
    """the whole corpus for the stand-alone sanitizer program (tools/bgzf_asan.cpp): per window u32 length, u8 eof, i64 expected damaged_at,
    u32 length of the expected text, the window, the text"""
    with open(path, "wb") as f:
        wins = [b for _, b in VALID.values()] + [b"".join(b for _, b in VALID.values())] + list(DAMAGED.values())
        wins += [planted(n, w)[0] for n in DAMAGED for w in ("middle", "last")]
        for wdw in wins:
            text, _, _, bad = oracle_window(wdw, True)
            text = text or b""
            f.write(struct.pack("<IBqI", len(wdw), 1, bad, len(text)) + wdw + text)
    return len(wins)
