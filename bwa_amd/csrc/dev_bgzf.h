// dev_bgzf.h -- BGZF blocks inflated on the device (included by bwagpu_index.hip; host side: bwagpu_bgzf_inflate, bwagpu_fastq_batch_bgzf).
//
// What it reproduces: zlib's inflate(Z_FINISH) of a raw DEFLATE stream (RFC 1951; inflate.c, inftrees.c) as BgzfPipe::inflate_group of
// host/host_input.h applies it to one BGZF block (SAM specification 4.1), with that function's tests behind it: the text has the length the
// trailer's ISIZE says and the CRC-32 the trailer says.  A block either passes all of it and its text is stored, or it is damaged: the window's
// status word takes the first damaged block and the reason, and nothing of the block is stored.
//
// The rules, as zlib has them:
//   - block type 3, a stored block whose LEN is not ~NLEN, HLIT > 286 or HDIST > 30 are errors;
//   - a set of code lengths is an error when it is over-subscribed, and when it is incomplete -- except that no code at all is allowed
//     (using it is the error then), and except the literal/length and the distance set whose longest code has one bit (inftrees.c: "max != 1");
//     the code-length code must be complete;
//   - a repeat code 16 without a previous length, a repeat that runs past HLIT + HDIST, a literal/length set without symbol 256 are errors;
//     the lengths of both alphabets are one sequence, a repeat may run from the first into the second;
//   - literal/length symbols 286 / 287 and distance symbols 30 / 31 (the fixed code has them), a bit pattern no code has, a distance
//     beyond the bytes produced so far, input that ends inside a symbol, more or fewer bytes than ISIZE are errors;
//   - bytes of the payload behind the final block are ignored.
//
// Shape: one wavefront per BGZF block, one wavefront per workgroup.  The control flow is wave-uniform: every lane keeps the bit reader and
// walks the symbols, the lanes share what is parallel --
//   - the payload is staged in LDS, BZ_STAGE bytes at a time, 16 bytes per lane (coalesced; the only reads of the payload, every one
//     bounded by the payload's ends, zero outside them);
//   - the tables of a set of code lengths: 16 lanes count the lengths, every lane ranks its symbols, every lane fills its entries of the
//     look-up table (BZ_LBITS / BZ_DBITS bits; a longer code takes the canonical walk over the counts, as puff.c does);
//   - a match: lane i takes byte i from out[pos - d + i % d], which is right for overlapping matches too since every source byte lies
//     before pos; a stored block: lane i takes byte i of the payload;
//   - the CRC-32: lane i takes 1028 bytes (257 words: consecutive lanes start on consecutive LDS banks), the lanes' values are combined
//     by multiplication with x^(8 * bytes behind) modulo the CRC polynomial (crc32_combine's arithmetic) and an XOR over the wave;
//   - the store: 16 bytes per lane at 16-byte aligned addresses of the inflated window, after the CRC has been found right.
// The output window is the whole block in LDS (64 KiB + tables = 70 KiB a wavefront): back-references never go through global memory, a
// block needs no flush logic, and CRC and store are one pass at the end.  The price is two wavefronts per CU (160 KiB of LDS), 512 blocks in
// flight on the chip; a 32 KiB ring would double that for a flush every 16 KiB.  profiles/dev_bgzf.md has what the choice costs.
//
// Memory safety: the input is untrusted.  Payload reads go through bz_stage alone; writes to the LDS window are tested against
// min(ISIZE, 65536) first; a distance is tested against the bytes produced; table indices are masked (look-up tables) or tested (sorted
// symbols); every loop ends with the bit budget of the payload (a sticky error once it is overdrawn) or a constant bound.
#pragma once

typedef unsigned short u16;

#define BZ_WAVE 64
#define BZ_MAX_OUT 65536u
#define BZ_STAGE 1024u                         // payload bytes staged at a time: 16 per lane
#define BZ_LBITS 10                            // bits the literal/length look-up table resolves
#define BZ_DBITS 8                             // ... the distance table
#define BZ_CBITS 7                             // ... the code-length code's table (its longest code)
#define BZ_CRC_SEG 1028u                       // bytes per lane of the CRC pass
#define BZ_BIG (1ull << 40)                    // status word of a window: (BZ_BIG - first damaged block) << 8 | its BZ_E_*, 0: every block inflated and stored

// why a block is damaged
enum { BZ_E_TYPE = 1, BZ_E_STORED, BZ_E_COUNTS, BZ_E_CODE, BZ_E_REPEAT, BZ_E_NO_EOB, BZ_E_SYMBOL, BZ_E_DIST, BZ_E_INPUT, BZ_E_LENGTH, BZ_E_ISIZE, BZ_E_CRC };

// one BGZF block of a window: its payload in the compressed bytes, the trailer's words, and where its text goes in the inflated window
struct BzBlock { u64 pay; u32 pay_len, isize, crc, pad; u64 out; };

struct BzLds {
	u32 win[BZ_MAX_OUT / 4 + 4];               // the block's text
	u32 stage[BZ_STAGE / 4];
	u16 ltab[1 << BZ_LBITS], dtab[1 << BZ_DBITS], ctab[1 << BZ_CBITS];      // (symbol << 4 | bits), 0: not resolved by the table
	u16 lsorted[288], dsorted[32], csorted[32];                            // symbols by (length, symbol)
	u16 lcnt[16], dcnt[16], ccnt[16];                                      // symbols per length
	u8 lens[320 + 32], clens[32];
};

IDX_DEVFN void bz_sync()
{	// intra-wave ordering point for LDS data handed from one lane to another
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
}

// the bit reader (the same in every lane)
struct BzIn {
	u64 buf; int cnt;                          // bits not yet taken
	u32 pos, chunk;                            // byte offset (from base) of the next word to load; the staged chunk
	i64 left;                                  // bits of the payload not yet taken: below zero, the stream ran past the payload's end
	int err;                                   // sticky: the first BZ_E_*
	const u8 *comp; u64 base, pay, end;        // base: pay rounded down to 16
	u32 *stage; u32 lane;
};

IDX_DEVFN void bz_fail(BzIn &R, int e) { if (!R.err) R.err = e; }

// the chunk that holds R.pos: lane i loads bytes [16 i, 16 i + 16) of it, zero outside the payload
IDX_DEVFN void bz_stage(BzIn &R)
{
	R.chunk = R.pos / BZ_STAGE;
	const u64 a = R.base + (u64)R.chunk * BZ_STAGE + 16u * R.lane;
	uint4 v = make_uint4(0, 0, 0, 0);
	if (a >= R.pay && a + 16 <= R.end) v = *(const uint4*)(R.comp + a);
	else if (a + 16 > R.pay && a < R.end) {
		u32 w[4] = { 0, 0, 0, 0 };
		for (u32 k = 0; k < 16; ++k) if (a + k >= R.pay && a + k < R.end) w[k >> 2] |= (u32)R.comp[a + k] << ((k & 3) * 8);
		v = make_uint4(w[0], w[1], w[2], w[3]);
	}
	bz_sync();                                 // (every lane is done with the chunk before)
	((uint4*)R.stage)[R.lane] = v;
	bz_sync();
}
IDX_DEVFN void bz_refill(BzIn &R)
{
	if (R.cnt > 32) return;
	if (R.pos / BZ_STAGE != R.chunk) bz_stage(R);
	R.buf |= (u64)R.stage[(R.pos & (BZ_STAGE - 1)) >> 2] << R.cnt;
	R.cnt += 32; R.pos += 4;
}
// n <= 16 bits (the caller has refilled)
IDX_DEVFN u32 bz_take(BzIn &R, int n)
{
	const u32 v = (u32)R.buf & ((1u << n) - 1u);
	R.buf >>= n; R.cnt -= n; R.left -= n;
	if (R.left < 0) bz_fail(R, BZ_E_INPUT);
	return v;
}
// continue at byte `at` of the payload
IDX_DEVFN void bz_seek(BzIn &R, u64 at)
{
	const u64 o = R.pay - R.base + at;
	R.pos = (u32)(o & ~3ull); R.chunk = ~0u; R.buf = 0; R.cnt = 0;
	bz_refill(R);
	const int drop = (int)(o & 3) * 8;
	R.buf >>= drop; R.cnt -= drop;
}

// Tables of the n code lengths at lens (each < 16): cnt, sorted and the look-up table of P bits.  False: the set is over-subscribed or
// incomplete (one_ok: a set whose longest code has one bit may be incomplete)
IDX_DEVFN bool bz_build(const u8 *lens, u32 n, u16 *cnt, u16 *sorted, u16 *tab, int P, bool one_ok, u32 lane)
{
	bz_sync();
	if (lane < 16) { u32 c = 0; for (u32 s = 0; s < n; ++s) c += lens[s] == lane ? 1u : 0u; cnt[lane] = (u16)c; }
	bz_sync();
	int left = 1, longest = 0; bool over = false;
	for (int l = 1; l <= 15; ++l) {
		const int c = cnt[l];
		left = (left << 1) - c;
		if (left < 0) { over = true; left = 0; }
		if (c) longest = l;
	}
	if (over || (left > 0 && longest != 0 && !(one_ok && longest == 1))) return false;
	for (u32 s = lane; s < n; s += BZ_WAVE) {
		const u32 l = lens[s];
		if (!l) continue;
		u32 at = 0;
		for (u32 t = 0; t < s; ++t) at += lens[t] == l ? 1u : 0u;
		for (u32 k = 1; k < l; ++k) at += cnt[k];
		if (at < n) sorted[at] = (u16)s;
	}
	bz_sync();
	for (u32 e = lane; e < (1u << P); e += BZ_WAVE) {
		int code = 0, first = 0, index = 0; u32 v = 0;
		for (int l = 1; l <= P; ++l) {
			code |= (int)(e >> (l - 1)) & 1;
			const int c = cnt[l];
			if (code - c < first) { const u32 at = (u32)(index + code - first); if (at < n) v = (u32)sorted[at] << 4 | (u32)l; break; }
			index += c; first = (first + c) << 1; code <<= 1;
		}
		tab[e] = (u16)v;
	}
	bz_sync();
	return true;
}

// the next symbol of a code (the caller has refilled: 15 bits are there)
IDX_DEVFN u32 bz_symbol(BzIn &R, const u16 *tab, int P, const u16 *cnt, const u16 *sorted, u32 n)
{
	const u32 e = tab[(u32)R.buf & ((1u << P) - 1u)];
	if (e) { (void)bz_take(R, (int)(e & 15)); return e >> 4; }
	u32 bits = (u32)R.buf;
	int code = 0, first = 0, index = 0;
	for (int l = 1; l <= 15; ++l) {
		code |= (int)(bits & 1); bits >>= 1;
		const int c = cnt[l];
		if (code - c < first) {
			const u32 at = (u32)(index + code - first);
			(void)bz_take(R, l);
			if (at < n) return sorted[at];
			break;
		}
		index += c; first = (first + c) << 1; code <<= 1;
	}
	bz_fail(R, BZ_E_SYMBOL);                   // a bit pattern no code has (an incomplete set)
	return 0;
}

// a * b modulo the CRC-32 polynomial, reflected (zlib's multmodp)
IDX_DEVFN u32 bz_mulmod(u32 a, u32 b)
{
	u32 p = 0;
	for (u32 m = 1u << 31; m; m >>= 1) {
		if (a & m) { p ^= b; if (!(a & (m - 1))) break; }
		b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
	}
	return p;
}

// the CRC-32 of the n bytes in win (every lane gets it)
IDX_DEVFN u32 bz_crc(const u32 *win, u32 n, u32 lane)
{
	const u32 s0 = lane * BZ_CRC_SEG;
	u32 c = 0, len = 0;
	if (s0 < n) {
		len = n - s0 < BZ_CRC_SEG ? n - s0 : BZ_CRC_SEG;
		c = ~0u;
		for (u32 o = 0; o < len; o += 4) {
			const u32 nb = len - o < 4 ? len - o : 4;
			c ^= nb == 4 ? win[(s0 + o) >> 2] : win[(s0 + o) >> 2] & ((1u << (8 * nb)) - 1u);
			for (u32 k = 0; k < 8 * nb; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
		}
		c = ~c;
	}
	// crc(A B) = crc(A) * x^(8 |B|) + crc(B): every lane's share of the sum
	u32 m = s0 < n ? n - s0 - len : 0, p = 1u << 31, sq = 1u << 23;
	for (; m; m >>= 1) { if (m & 1) p = bz_mulmod(sq, p); sq = bz_mulmod(sq, sq); }
	c = bz_mulmod(p, c);
	for (int d = 1; d < BZ_WAVE; d <<= 1) c ^= (u32)__shfl_xor((int)c, d);
	return c;
}

struct BzArgs { const u8 *comp; const BzBlock *blk; u32 n_blocks; u8 *out; u64 *bad; };

__global__ void __launch_bounds__(BZ_WAVE) k_bz_inflate(BzArgs A)
{
	__shared__ BzLds S;
	const u32 lane = threadIdx.x & (BZ_WAVE - 1), b = blockIdx.x;
	if (b >= A.n_blocks) return;
	const BzBlock B = A.blk[b];
	u8 *win8 = (u8*)S.win;
	const u32 lim = B.isize < BZ_MAX_OUT ? B.isize : BZ_MAX_OUT;
	u32 op = 0;
	BzIn R;
	R.err = B.isize > BZ_MAX_OUT ? BZ_E_ISIZE : 0;
	R.comp = A.comp; R.pay = B.pay; R.end = B.pay + B.pay_len; R.base = B.pay & ~15ull; R.left = (i64)B.pay_len * 8; R.stage = S.stage; R.lane = lane;
	R.buf = 0; R.cnt = 0; R.pos = 0; R.chunk = ~0u;
	if (!R.err) bz_seek(R, 0);
	bool last = false;
	while (!R.err && !last) {
		bz_refill(R);
		last = bz_take(R, 1) != 0;
		const u32 type = bz_take(R, 2);
		if (type == 3) { bz_fail(R, BZ_E_TYPE); break; }
		if (type == 0) {
			(void)bz_take(R, R.cnt & 7);
			bz_refill(R);
			const u32 len = bz_take(R, 16);
			bz_refill(R);
			const u32 nlen = bz_take(R, 16);
			if (R.err) break;
			if ((len ^ 0xffffu) != nlen) { bz_fail(R, BZ_E_STORED); break; }
			if ((i64)len * 8 > R.left) { bz_fail(R, BZ_E_INPUT); break; }
			if (len > lim - op) { bz_fail(R, BZ_E_LENGTH); break; }
			const u64 at = (u64)B.pay_len - (u64)(R.left >> 3);               // (the reader stands on a byte boundary)
			for (u32 i = lane; i < len; i += BZ_WAVE) win8[op + i] = R.comp[R.pay + at + i];
			op += len;
			const i64 left = R.left - (i64)len * 8;
			bz_seek(R, at + len);
			R.left = left;
			continue;
		}
		u32 nl, nd;
		if (type == 1) {
			nl = 288; nd = 32;
			for (u32 s = lane; s < 320; s += BZ_WAVE) S.lens[s] = (u8)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
		} else {
			bz_refill(R);
			nl = bz_take(R, 5) + 257; nd = bz_take(R, 5) + 1;
			const u32 nc = bz_take(R, 4) + 4;
			if (R.err) break;
			if (nl > 286 || nd > 30) { bz_fail(R, BZ_E_COUNTS); break; }
			const u8 order[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
			for (u32 i = 0; i < 19; ++i) {      // (every lane writes every length: each reads back what it wrote itself)
				u32 v = 0;
				if (i < nc) { bz_refill(R); v = bz_take(R, 3); }
				S.clens[order[i]] = (u8)v;
			}
			if (R.err) break;
			if (!bz_build(S.clens, 19, S.ccnt, S.csorted, S.ctab, BZ_CBITS, false, lane)) { bz_fail(R, BZ_E_CODE); break; }
			u32 have = 0;
			while (have < nl + nd && !R.err) {
				bz_refill(R);
				const u32 sym = bz_symbol(R, S.ctab, BZ_CBITS, S.ccnt, S.csorted, 19);
				if (R.err) break;
				if (sym < 16) { S.lens[have++] = (u8)sym; continue; }
				u32 rep, v = 0;
				if (sym == 16) {
					if (!have) { bz_fail(R, BZ_E_REPEAT); break; }
					v = S.lens[have - 1]; rep = 3 + bz_take(R, 2);
				} else if (sym == 17) rep = 3 + bz_take(R, 3);
				else rep = 11 + bz_take(R, 7);
				if (R.err) break;
				if (have + rep > nl + nd) { bz_fail(R, BZ_E_REPEAT); break; }
				for (u32 i = 0; i < rep; ++i) S.lens[have + i] = (u8)v;
				have += rep;
			}
			if (R.err) break;
			if (!S.lens[256]) { bz_fail(R, BZ_E_NO_EOB); break; }
		}
		if (!bz_build(S.lens, nl, S.lcnt, S.lsorted, S.ltab, BZ_LBITS, true, lane) ||
			!bz_build(S.lens + nl, nd, S.dcnt, S.dsorted, S.dtab, BZ_DBITS, true, lane)) { bz_fail(R, BZ_E_CODE); break; }
		while (!R.err) {
			bz_refill(R);
			const u32 sym = bz_symbol(R, S.ltab, BZ_LBITS, S.lcnt, S.lsorted, nl);
			if (R.err) break;
			if (sym < 256) {
				if (op >= lim) { bz_fail(R, BZ_E_LENGTH); break; }
				win8[op++] = (u8)sym;              // (every lane, the same byte)
				continue;
			}
			if (sym == 256) break;
			if (sym > 285) { bz_fail(R, BZ_E_SYMBOL); break; }
			u32 len;
			if (sym < 265) len = sym - 254;
			else if (sym == 285) len = 258;
			else { const int x = (int)((sym - 261) >> 2); len = 3 + ((4 + ((sym - 261) & 3)) << x) + bz_take(R, x); }
			bz_refill(R);
			const u32 ds = bz_symbol(R, S.dtab, BZ_DBITS, S.dcnt, S.dsorted, nd);
			if (R.err) break;
			if (ds > 29) { bz_fail(R, BZ_E_SYMBOL); break; }
			u32 dist;
			if (ds < 4) dist = ds + 1;
			else { const int x = (int)(ds >> 1) - 1; dist = 1 + ((2 + (ds & 1)) << x) + bz_take(R, x); }
			if (R.err) break;
			if (dist > op) { bz_fail(R, BZ_E_DIST); break; }
			if (len > lim - op) { bz_fail(R, BZ_E_LENGTH); break; }
			bz_sync();                             // (the bytes before op are written)
			if (dist >= len) { for (u32 i = lane; i < len; i += BZ_WAVE) win8[op + i] = win8[op - dist + i]; }
			else for (u32 i = lane; i < len; i += BZ_WAVE) win8[op + i] = win8[op - dist + i % dist];
			op += len;
		}
	}
	if (!R.err && op != B.isize) bz_fail(R, BZ_E_ISIZE);
	bz_sync();
	if (!R.err && bz_crc(S.win, op, lane) != B.crc) bz_fail(R, BZ_E_CRC);
	if (R.err) {
		if (lane == 0) atomicMax(A.bad, (BZ_BIG - (u64)b) << 8 | (u64)R.err);
		return;
	}
	// the store: bytes up to the first 16-byte aligned address one by one, then 16 bytes per lane, then the rest
	u8 *dst = A.out + B.out;
	u32 head = (u32)((16 - ((u64)dst & 15)) & 15);
	if (head > op) head = op;
	const u32 n16 = (op - head) >> 4;
	if (lane < head) dst[lane] = win8[lane];
	for (u32 i = lane; i < n16; i += BZ_WAVE) {
		const u32 t = head + 16 * i, sh = (t & 3) * 8;
		const u32 *w = S.win + (t >> 2);
		uint4 v;
		if (sh) v = make_uint4(w[0] >> sh | w[1] << (32 - sh), w[1] >> sh | w[2] << (32 - sh), w[2] >> sh | w[3] << (32 - sh), w[3] >> sh | w[4] << (32 - sh));
		else v = make_uint4(w[0], w[1], w[2], w[3]);
		*(uint4*)(dst + t) = v;
	}
	const u32 t0 = head + 16 * n16;
	if (t0 + lane < op) dst[t0 + lane] = win8[t0 + lane];
}
