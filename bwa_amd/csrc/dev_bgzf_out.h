// dev_bgzf_out.h -- text compressed into BGZF blocks on the device (included by bwagpu_index.hip behind dev_bgzf.h; host side:
// bwagpu_bgzf_deflate).  The mirror of k_bz_inflate: what it writes is what that kernel, zlib and htslib read.
//
// What it produces: for every slice of at most BO_MAX_TEXT bytes of the text one BGZF block (SAM specification 4.1) -- the 18-byte
// header with the BC subfield and BSIZE, one final raw DEFLATE block (RFC 1951), CRC-32 and ISIZE -- in a slot of BO_SLOT bytes; a scan
// of the sizes and k_bo_gather pack the slots.  A block refers to nothing outside itself.
//
// Shape: one wavefront per BGZF block, one wavefront per workgroup, the block's text in LDS.
//   - match search, BO_TILE positions at a time: a lane hashes the BO_MIN_MATCH bytes at its positions, takes the candidate the head
//     table holds -- the highest earlier position of *earlier tiles* with that hash --, and extends it byte by byte (1 .. BO_MAX_DIST
//     back, up to BO_MAX_MATCH long, overlapping itself if it does).  Then the tile's positions enter the table by atomicMax.  Reads and
//     inserts are separated by a wave barrier and the maximum does not depend on the order of the lanes: the candidates, and with them
//     the compressed bytes, are a function of the text and the block size alone.  A repeat closer than the start of its tile is found
//     through the tile before (period p text matches at a multiple of p).
//   - greedy parse: lane 0 walks the tile's (length, distance) pairs and appends tokens to the block's token array in global memory
//     (a literal: the byte; a match: bit 31, length - 3, distance - 1).
//   - counts of the literal/length and the distance symbols by LDS atomics over the tokens, and the counts of the bare bytes.
//   - code lengths (bo_lengths): the lanes rank the used symbols by (count, symbol), lane 0 runs the two-queue Huffman construction on the
//     sorted counts, limits the depth by moving leaves on the per-length counts (the repair zlib's gen_bitlen applies) and hands the
//     longest lengths to the rarest symbols.  15 bits for both alphabets, 7 for the code-length code.  Codes are canonical.
//     One used symbol gets one bit (the incomplete set zlib allows), no used distance sends one zero length.
//   - block type: the smallest of stored, fixed codes, dynamic codes -- each over the tokens -- and dynamic codes over the bare bytes
//     (no match at all: on text whose matches cost more than their literals, uniform ACGT for one, the greedy choice loses to it).
//     The sizes follow from the counts alone.  Stored is the guarantee: text + 31 bytes, never more than 65536.
//   - emit: every lane takes an equal run of tokens, sums its bits, a wave scan gives the runs their bit offsets.  Lane 0 writes the
//     BGZF header and the code lengths ahead of its run, lane 63 the end-of-block code and the trailer behind its own.  A lane
//     assembles 32-bit words; the first and the last word of a run may be shared with a neighbour and are added atomically to the
//     zeroed slot, the words between are stored.  The CRC-32 is dev_bgzf.h's bz_crc on the text in LDS.
// The code lengths are sent plain (symbols 0..15 of the code-length code, no repeat codes 16..18).
//
// LDS: 64 KiB of text + 32 KiB of heads + tables = ~104 KiB, one wavefront per CU.  profiles/dev_bgzf_out.md has what that costs.
//
// Memory safety: the text is read through [0, n) of its slice alone (n <= BO_MAX_TEXT, the host's cut); LDS reads behind the text stay
// inside 16 zeroed pad bytes; a token array has BO_MAX_TEXT entries and a parse makes at most n tokens; a slot takes at most n + 31
// <= 65311 bytes, and every block type's size is compared with stored's before it is chosen.
#pragma once

#define BO_WAVE 64
#define BO_MAX_TEXT 0xff00u
#define BO_MIN_MATCH 4u
#define BO_MAX_MATCH 258u
#define BO_MAX_DIST 32768u
#define BO_HBITS 12
#define BO_TILE 256u
#define BO_SLOT 65536u
#define BO_MATCH 0x80000000u

enum { BO_STORED = 0, BO_FIXED, BO_DYNAMIC, BO_DYNAMIC_BYTES };

struct BoLds {
	u32 text[BO_MAX_TEXT / 4 + 4];
	u64 head[1 << BO_HBITS];                   // position + 1 (0: none)
	u16 tlen[BO_TILE], tdist[BO_TILE];         // the tile's matches (0: none)
	u32 lfreq[288], dfreq[32], bfreq[288], cfreq[20];
	u32 lcode[288], dcode[32], ccode[20];      // bit-reversed code | length << 16
	u8 llen[288], dlen[32], blen[288], clen[20], zlen[32];      // (zlen: zeros)
	u32 w[576]; u16 par[576], dep[576], sorted[288];      // bo_lengths
	u32 cnt[16], next[16];
	u32 ntok;
};

// literal/length symbol of length - 3, distance symbol of distance - 1, and their extra bits
IDX_DEVFN u32 bo_lsym(u32 l) { if (l < 4) return 257 + l; if (l == 255) return 285; const u32 x = (u32)(31 - __clz((int)l)) - 2; return 261 + 4 * x + ((l >> x) & 3); }
IDX_DEVFN u32 bo_lextra(u32 s) { return s < 265 || s == 285 ? 0 : (s - 261) >> 2; }
IDX_DEVFN u32 bo_dsym(u32 d) { if (d < 4) return d; const u32 n = (u32)(31 - __clz((int)d)); return 2 * n + ((d >> (n - 1)) & 1); }
IDX_DEVFN u32 bo_dextra(u32 s) { return s < 4 ? 0 : (s >> 1) - 1; }
IDX_DEVFN u32 bo_fixed_len(u32 s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

// word k of the 18-byte BGZF header of a block of `size` bytes (MTIME 0, OS 255, as bgzip writes it)
IDX_DEVFN u32 bo_header(u32 k, u32 size) { return k == 0 ? 0x04088b1fu : k == 1 ? 0u : k == 2 ? 0x0006ff00u : k == 3 ? 0x00024342u : (size - 1) & 0xffffu; }

IDX_DEVFN u32 bo_hash(const u8 *T, u32 p)
{
	const u32 v = (u32)T[p] | (u32)T[p + 1] << 8 | (u32)T[p + 2] << 16 | (u32)T[p + 3] << 24;
	return (v * 2654435761u) >> (32 - BO_HBITS);
}

// Code lengths of at most maxbits for the n counts at freq (every lane calls; len is in LDS)
IDX_DEVFN void bo_lengths(const u32 *freq, u32 n, u32 maxbits, u8 *len, BoLds &S, u32 lane)
{
	bz_sync();
	for (u32 s = lane; s < n; s += BO_WAVE) {
		len[s] = 0;
		const u32 f = freq[s];
		if (!f) continue;
		u32 r = 0;
		for (u32 t = 0; t < n; ++t) { const u32 g = freq[t]; r += (g && (g < f || (g == f && t < s))) ? 1u : 0u; }
		S.sorted[r] = (u16)s;
	}
	bz_sync();
	if (lane == 0) {
		u32 m = 0;
		for (u32 t = 0; t < n; ++t) m += freq[t] ? 1u : 0u;
		if (m == 1) len[S.sorted[0]] = 1;
		else if (m >= 2) {
			for (u32 i = 0; i < m; ++i) S.w[i] = freq[S.sorted[i]];
			// leaves 0 .. m-1 by rising count, inner nodes m .. 2m-2 in the order they are made (rising too): two queues
			u32 i = 0, j = m;
			for (u32 k = m; k < 2 * m - 1; ++k) {
				const u32 a = (i < m && (j >= k || S.w[i] <= S.w[j])) ? i++ : j++;
				const u32 b = (i < m && (j >= k || S.w[i] <= S.w[j])) ? i++ : j++;
				S.w[k] = S.w[a] + S.w[b]; S.par[a] = (u16)k; S.par[b] = (u16)k;
			}
			for (u32 b = 0; b < 16; ++b) S.cnt[b] = 0;
			int over = 0;
			S.dep[2 * m - 2] = 0;
			for (u32 v = 2 * m - 2; v-- > 0;) {
				u32 d = (u32)S.dep[S.par[v]] + 1;
				if (d > maxbits) { d = maxbits; ++over; }      // (every node below the limit, inner ones too: each stands for one leaf too many at maxbits)
				S.dep[v] = (u16)d;
				if (v < m) S.cnt[d]++;
			}
			// too deep: a leaf of the deepest level above the limit goes one down and takes one of the clamped leaves as its sibling
			while (over > 0) {
				u32 b = maxbits - 1;
				while (b > 1 && !S.cnt[b]) --b;
				S.cnt[b]--; S.cnt[b + 1] += 2; S.cnt[maxbits]--;
				over -= 2;
			}
			u32 at = 0;
			for (u32 b = maxbits; b >= 1; --b) for (u32 c = S.cnt[b]; c; --c) len[S.sorted[at++]] = (u8)b;
		}
	}
	bz_sync();
}

// canonical codes of n lengths (lane 0 alone; the caller synchronises)
IDX_DEVFN void bo_codes(const u8 *len, u32 n, u32 *code, BoLds &S)
{
	for (u32 b = 0; b < 16; ++b) S.cnt[b] = 0;
	for (u32 s = 0; s < n; ++s) S.cnt[len[s]]++;
	S.cnt[0] = 0;
	u32 c = 0;
	for (u32 b = 1; b < 16; ++b) { c = (c + S.cnt[b - 1]) << 1; S.next[b] = c; }
	for (u32 s = 0; s < n; ++s) {
		const u32 l = len[s];
		u32 r = 0;
		if (l) { u32 v = S.next[l]++; for (u32 k = 0; k < l; ++k) { r = r << 1 | (v & 1); v >>= 1; } }
		code[s] = r | l << 16;
	}
}

// the code-length code of the nl + nd lengths sent plain; returns the bits of HLIT .. the coded lengths, *nc_out: HCLEN + 4
IDX_DEVFN u32 bo_tree(const u8 *ll, u32 nl, const u8 *dl, u32 nd, u32 *nc_out, BoLds &S, u32 lane)
{
	bz_sync();
	if (lane < 20) S.cfreq[lane] = 0;
	bz_sync();
	for (u32 s = lane; s < nl + nd; s += BO_WAVE) atomicAdd(&S.cfreq[s < nl ? ll[s] : dl[s - nl]], 1u);
	bo_lengths(S.cfreq, 19, 7, S.clen, S, lane);
	const u8 order[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
	u32 nc = 4, bits = 0;
	for (u32 i = 0; i < 19; ++i) { const u32 s = order[i]; if (S.clen[s]) nc = i + 1 > nc ? i + 1 : nc; bits += S.cfreq[s] * S.clen[s]; }
	*nc_out = nc;
	return 14 + 3 * nc + bits;
}

// a lane's part of the block's bit stream
struct BoOut { u32 *out; u64 acc; u32 nb, w; bool first; };
IDX_DEVFN void bo_open(BoOut &O, u32 *out, u32 bit) { O.out = out; O.acc = 0; O.nb = bit & 31; O.w = bit >> 5; O.first = true; }
// n <= 32 bits
IDX_DEVFN void bo_put(BoOut &O, u32 v, u32 n)
{
	O.acc |= (u64)v << O.nb; O.nb += n;
	if (O.nb >= 32) {
		if (O.first) atomicAdd(O.out + O.w, (u32)O.acc); else O.out[O.w] = (u32)O.acc;
		O.first = false; O.acc >>= 32; O.nb -= 32; ++O.w;
	}
}
IDX_DEVFN void bo_close(BoOut &O) { if (O.nb && (u32)O.acc) atomicAdd(O.out + O.w, (u32)O.acc); }

// bits of token t under the codes in S / the token itself
IDX_DEVFN u32 bo_token_bits(const BoLds &S, u32 t)
{
	if (!(t & BO_MATCH)) return S.lcode[t] >> 16;
	const u32 ls = bo_lsym((t >> 16) & 255), ds = bo_dsym(t & 32767);
	return (S.lcode[ls] >> 16) + bo_lextra(ls) + (S.dcode[ds] >> 16) + bo_dextra(ds);
}
IDX_DEVFN void bo_token_put(BoOut &O, const BoLds &S, u32 t)
{
	if (!(t & BO_MATCH)) { const u32 c = S.lcode[t]; bo_put(O, c & 0xffff, c >> 16); return; }
	const u32 l = (t >> 16) & 255, d = t & 32767, ls = bo_lsym(l), ds = bo_dsym(d), lx = bo_lextra(ls), dx = bo_dextra(ds);
	const u32 lc = S.lcode[ls], dc = S.dcode[ds];
	bo_put(O, (lc & 0xffff) | ((l & ((1u << lx) - 1u)) << (lc >> 16)), (lc >> 16) + lx);      // (a symbol's first length is a multiple of 1 << its extra bits)
	bo_put(O, (dc & 0xffff) | ((d & ((1u << dx) - 1u)) << (dc >> 16)), (dc >> 16) + dx);
}

struct BoArgs { const u8 *text; u64 text_len; u32 block_size, n_blocks; u32 *tok; u8 *slot; u64 *sizes; };

__global__ void __launch_bounds__(BO_WAVE) k_bo_deflate(BoArgs A)
{
	__shared__ BoLds S;
	const u32 lane = threadIdx.x & (BO_WAVE - 1), b = blockIdx.x;
	if (b >= A.n_blocks) return;
	const u64 t0 = (u64)b * A.block_size;
	const u32 n = A.text_len - t0 < (u64)A.block_size ? (u32)(A.text_len - t0) : A.block_size;
	const u8 *src = A.text + t0;
	u8 *T = (u8*)S.text;
	u32 *tok = A.tok + (u64)b * BO_MAX_TEXT;
	u8 *out8 = A.slot + (u64)b * BO_SLOT;

	// the text, zeros behind it; heads and counts cleared
	if (lane < 4) S.text[(n >> 2) + lane] = 0;
	for (u32 i = lane; i < (1u << BO_HBITS); i += BO_WAVE) S.head[i] = 0;
	for (u32 i = lane; i < 288; i += BO_WAVE) { S.lfreq[i] = 0; S.bfreq[i] = 0; S.llen[i] = 0; S.blen[i] = 0; }
	if (lane < 32) { S.dfreq[lane] = 0; S.dlen[lane] = 0; S.zlen[lane] = 0; }
	bz_sync();
	if (!((u64)src & 3)) {
		for (u32 i = lane; i < (n >> 2); i += BO_WAVE) S.text[i] = ((const u32*)src)[i];
		if (lane < (n & 3)) T[(n & ~3u) + lane] = src[(n & ~3u) + lane];
	} else for (u32 i = lane; i < n; i += BO_WAVE) T[i] = src[i];
	bz_sync();

	// match search and greedy parse, tile by tile
	u32 p = 0, nt = 0;                          // (lane 0's)
	for (u32 s0 = 0; s0 < n; s0 += BO_TILE) {
		u32 hh[BO_TILE / BO_WAVE];
#pragma unroll
		for (u32 k = 0; k < BO_TILE / BO_WAVE; ++k) {
			const u32 at = k * BO_WAVE + lane, pos = s0 + at;
			u32 L = 0, D = 0;
			hh[k] = ~0u;
			if (pos + BO_MIN_MATCH <= n) {
				const u32 h = bo_hash(T, pos);
				hh[k] = h;
				const u32 c = (u32)S.head[h];
				if (c && pos - (c - 1) <= BO_MAX_DIST) {
					const u32 q = c - 1, maxl = n - pos < BO_MAX_MATCH ? n - pos : BO_MAX_MATCH;
					u32 l = 0;
					while (l < maxl && T[q + l] == T[pos + l]) ++l;
					if (l >= BO_MIN_MATCH) { L = l; D = pos - q; }
				}
			}
			S.tlen[at] = (u16)L; S.tdist[at] = (u16)D;
		}
		bz_sync();
#pragma unroll
		for (u32 k = 0; k < BO_TILE / BO_WAVE; ++k) if (hh[k] != ~0u) atomicMax(&S.head[hh[k]], (u64)(s0 + k * BO_WAVE + lane) + 1);
		if (lane == 0) {
			const u32 end = s0 + BO_TILE < n ? s0 + BO_TILE : n;
			while (p < end) {
				const u32 L = S.tlen[p - s0];
				if (L) { tok[nt++] = BO_MATCH | (L - 3) << 16 | ((u32)S.tdist[p - s0] - 1); p += L; }
				else { tok[nt++] = T[p]; ++p; }
			}
		}
		bz_sync();
	}
	if (lane == 0) { S.ntok = nt; S.lfreq[256] = 1; S.bfreq[256] = 1; }
	__threadfence();                            // (lane 0's tokens, read by every lane from here on)
	bz_sync();
	nt = S.ntok;

	// counts
	for (u32 i = lane; i < nt; i += BO_WAVE) {
		const u32 t = tok[i];
		if (t & BO_MATCH) { atomicAdd(&S.lfreq[bo_lsym((t >> 16) & 255)], 1u); atomicAdd(&S.dfreq[bo_dsym(t & 32767)], 1u); }
		else atomicAdd(&S.lfreq[t], 1u);
	}
	for (u32 i = lane; i < n; i += BO_WAVE) atomicAdd(&S.bfreq[T[i]], 1u);
	bz_sync();
	const u32 crc = bz_crc(S.text, n, lane);

	// code lengths and what each block type would take (bits behind the BGZF header, the end-of-block code included)
	bo_lengths(S.lfreq, 286, 15, S.llen, S, lane);
	bo_lengths(S.dfreq, 30, 15, S.dlen, S, lane);
	bo_lengths(S.bfreq, 257, 15, S.blen, S, lane);
	u32 nl = 257, nd = 1, data = 0, fixed = 3, bytes = 0;
	for (u32 s = 0; s < 286; ++s) {
		const u32 f = S.lfreq[s];
		if (f && s >= nl) nl = s + 1;
		data += f * (S.llen[s] + bo_lextra(s)); fixed += f * (bo_fixed_len(s) + bo_lextra(s));
		if (s < 257) bytes += S.bfreq[s] * S.blen[s];
	}
	for (u32 s = 0; s < 30; ++s) {
		const u32 f = S.dfreq[s];
		if (f) nd = s + 1;
		data += f * (S.dlen[s] + bo_dextra(s)); fixed += f * (5 + bo_dextra(s));
	}
	u32 nc = 0, ncb = 0;
	const u32 dyn = 3 + bo_tree(S.llen, nl, S.dlen, nd, &nc, S, lane) + data;
	const u32 dynb = nt == n ? ~0u : 3 + bo_tree(S.blen, 257, S.zlen, 1, &ncb, S, lane) + bytes;
	const u32 stored = (5 + n) * 8;
	u32 mode = BO_STORED, bits = stored;
	if (fixed < bits) { mode = BO_FIXED; bits = fixed; }
	if (dyn < bits) { mode = BO_DYNAMIC; bits = dyn; }
	if (dynb < bits) { mode = BO_DYNAMIC_BYTES; bits = dynb; }
	const u32 size = 18 + ((bits + 7) >> 3) + 8;
	if (lane == 0) A.sizes[b] = size;

	if (mode == BO_STORED) {
		if (lane < 18) out8[lane] = (u8)(bo_header(lane >> 2, size) >> ((lane & 3) * 8));
		if (lane == 18) { out8[18] = 1; out8[19] = (u8)n; out8[20] = (u8)(n >> 8); out8[21] = (u8)~n; out8[22] = (u8)(~n >> 8); }
		for (u32 i = lane; i < n; i += BO_WAVE) out8[23 + i] = T[i];
		if (lane < 4) { out8[23 + n + lane] = (u8)(crc >> (lane * 8)); out8[27 + n + lane] = (u8)(n >> (lane * 8)); }
		return;
	}

	// the codes in use
	if (mode == BO_DYNAMIC_BYTES) {
		nl = 257; nd = 1; nc = ncb; nt = n;
		for (u32 s = lane; s < 288; s += BO_WAVE) S.llen[s] = s < 257 ? S.blen[s] : 0;
		if (lane < 32) S.dlen[lane] = 0;
		(void)bo_tree(S.llen, nl, S.dlen, nd, &nc, S, lane);
	} else if (mode == BO_DYNAMIC) (void)bo_tree(S.llen, nl, S.dlen, nd, &nc, S, lane);
	else {
		for (u32 s = lane; s < 288; s += BO_WAVE) S.llen[s] = (u8)bo_fixed_len(s);
		if (lane < 32) S.dlen[lane] = 5;
	}
	bz_sync();
	if (lane == 0) {
		bo_codes(S.llen, 288, S.lcode, S);
		bo_codes(S.dlen, 32, S.dcode, S);
		if (mode != BO_FIXED) bo_codes(S.clen, 19, S.ccode, S);
	}
	bz_sync();

	// emit
	const u32 head_bits = mode == BO_FIXED ? 3 : 3 + 14 + 3 * nc;
	u32 tree_bits = 0;
	if (mode != BO_FIXED) {
		for (u32 s = 0; s < nl; ++s) tree_bits += S.ccode[S.llen[s]] >> 16;
		for (u32 s = 0; s < nd; ++s) tree_bits += S.ccode[S.dlen[s]] >> 16;
	}
	const u32 per = (nt + BO_WAVE - 1) / BO_WAVE, i0 = lane * per < nt ? lane * per : nt, i1 = i0 + per < nt ? i0 + per : nt;
	u32 mine = 0;
	if (mode == BO_DYNAMIC_BYTES) for (u32 i = i0; i < i1; ++i) mine += S.lcode[T[i]] >> 16;
	else for (u32 i = i0; i < i1; ++i) mine += bo_token_bits(S, tok[i]);
	u32 incl = mine;
	for (int d = 1; d < BO_WAVE; d <<= 1) { const u32 o = (u32)__shfl_up((int)incl, d); if ((int)lane >= d) incl += o; }
	BoOut O;
	u32 *out = (u32*)out8;
	if (lane == 0) {
		bo_open(O, out, 0);
		bo_put(O, bo_header(0, size), 32); bo_put(O, bo_header(1, size), 32); bo_put(O, bo_header(2, size), 32); bo_put(O, bo_header(3, size), 32);
		bo_put(O, bo_header(4, size), 16);
		bo_put(O, mode == BO_FIXED ? 3 : 5, 3);      // BFINAL, BTYPE
		if (mode != BO_FIXED) {
			const u8 order[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
			bo_put(O, nl - 257, 5); bo_put(O, nd - 1, 5); bo_put(O, nc - 4, 4);
			for (u32 i = 0; i < nc; ++i) bo_put(O, S.clen[order[i]], 3);
			for (u32 s = 0; s < nl; ++s) { const u32 c = S.ccode[S.llen[s]]; bo_put(O, c & 0xffff, c >> 16); }
			for (u32 s = 0; s < nd; ++s) { const u32 c = S.ccode[S.dlen[s]]; bo_put(O, c & 0xffff, c >> 16); }
		}
	} else bo_open(O, out, 144 + head_bits + tree_bits + (incl - mine));
	if (mode == BO_DYNAMIC_BYTES) for (u32 i = i0; i < i1; ++i) { const u32 c = S.lcode[T[i]]; bo_put(O, c & 0xffff, c >> 16); }
	else for (u32 i = i0; i < i1; ++i) bo_token_put(O, S, tok[i]);
	if (lane == BO_WAVE - 1) {
		const u32 c = S.lcode[256];
		bo_put(O, c & 0xffff, c >> 16);
		if (O.nb & 7) bo_put(O, 0, 8 - (O.nb & 7));
		bo_put(O, crc, 32); bo_put(O, n, 32);
	}
	bo_close(O);
}

// the slots' blocks, one behind the other
struct BoPack { const u8 *slot; const u64 *sizes, *off; u8 *dst; u32 n_blocks; };

__global__ void __launch_bounds__(256) k_bo_gather(BoPack A)
{
	const u32 b = blockIdx.x;
	if (b >= A.n_blocks) return;
	const u8 *s = A.slot + (u64)b * BO_SLOT;
	u8 *d = A.dst + A.off[b];
	const u32 n = (u32)A.sizes[b];
	for (u32 i = threadIdx.x; i < n; i += 256) d[i] = s[i];
}
