// dev_fasta.h -- the per-byte half of `bwa index`'s FASTA reader on the device (included by bwagpu_index.hip).
//
// What it reproduces: kseq_read (kseq.h:175-215, ks_getuntil2 :95-141) followed by add1 (bntseq.c:232-278) -- which bytes of a
// FASTA stream become bases, their 2-bit codes (nst_nt4_table, bntseq.c:46; every other byte is an ambiguity code replaced by
// lrand48() & 3 after srand48(11)), and the holes of the .amb file.  Header lines are only located here; their text is parsed
// by the host (bwagpu_fasta_*, bwagpu_index.hip).  The host strips the bytes before the first '>' and holds a chunk's trailing
// '\r' back until the byte after it is known, so that every byte seen here lies in a record and has a known successor (or is
// the last byte of the stream).
//
// Rules per byte b at a line start (first byte of the stream after the preamble, or after '\n'):
//   '\n' empty line; '>' header line; '+' / '@' FASTQ structure (rejected); anything else starts a sequence line.
// In a sequence line every byte but '\n' is appended to the record, except a '\r' right before the line end ('\n', or the end of
// the stream when the line has at least two bytes -- ks_getuntil2 returns early on a one-byte last line) when the record then
// holds more than one base, i.e. unless the '\r' is the whole line and the record's first one.  NUL and bytes >= 0x80 in a
// sequence line are rejected (nst_nt4_table[(int)(char)c] reads out of bounds in the reference).  A hole starts at an
// ambiguous base that is its record's first or whose raw byte differs from the previous base's; it ends at the next base that
// starts a new run (or a record), or at the end of the stream.
//
// Method: a chunk is cut into tiles of FA_TILE bytes, a tile into FA_SEG-byte segments, one per lane.  The state a byte needs
// (FaSum: line type, counts, last kept byte) composes associatively over segments, but its parts depend on each other: the
// line type decides which bytes are kept, the kept bytes decide where holes start.  So the chunk is walked in four passes;
// pass p recomputes the tile's in-block prefixes of passes < p from the bytes (kept in registers), reduces the fields of pass
// p per tile, and the tile sums are scanned (rocPRIM) between passes.  Pass 4 writes: one code byte per base, hole starts
// (offset, raw byte), hole ends, and header positions -- each at an index its scan already gave, so outputs are sized exactly
// by the count passes (a chunk of "NnNn..." has as many holes as bases).  k_fa_pack then packs the codes into .pac bytes.
#pragma once

#define FA_BLOCK 256
#define FA_SEG 32                              // bytes per lane: two 16-byte loads
#define FA_TILE (FA_BLOCK * FA_SEG)

enum { FA_LT_HDR = 1, FA_LT_SEQ = 2 };          // line types (0: no header or sequence line start seen)
enum { FA_ERR_FASTQ = 1, FA_ERR_BYTE = 2 };     // kinds of rejected input (error word, see fa_error)

// Summary of a stretch of bytes (or, composed onto the carry, the state after it).  All fields are zero for an empty stretch.
struct FaSum {
	u64 nk, na, nh, ns, ne;   // bases kept, ambiguous bases, header lines, hole starts, hole ends
	u32 pt;                   // type of the last header / sequence line start (0: none)
	u32 lk;                   // 0x100 | raw byte of the last base kept (0: none)
	u32 hs;                   // a header line starts after the last base kept (with no base kept: anywhere)
	u32 pad;
};
struct FaCombine {
	__host__ __device__ FaSum operator()(const FaSum &a, const FaSum &b) const
	{
		FaSum r;
		r.nk = a.nk + b.nk; r.na = a.na + b.na; r.nh = a.nh + b.nh; r.ns = a.ns + b.ns; r.ne = a.ne + b.ne;
		r.pt = b.pt ? b.pt : a.pt;
		r.lk = b.lk ? b.lk : a.lk;
		r.hs = b.lk ? b.hs : (a.hs | b.hs);
		r.pad = 0;
		return r;
	}
};

__host__ __device__ inline FaSum fa_zero() { FaSum z; z.nk = z.na = z.nh = z.ns = z.ne = 0; z.pt = z.lk = z.hs = z.pad = 0; return z; }
IDX_DEVFN bool fa_is_acgt(u32 b) { const u32 u = b & 0xDFu; return u == 'A' || u == 'C' || u == 'G' || u == 'T'; }
IDX_DEVFN u32 fa_code(u32 b) { const u32 u = b & 0xDFu; return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : 3u; }

// where pass 4 writes (indices are relative to the chunk's carry)
struct FaOut {
	u8 *codes;                         // one 2-bit code per base kept
	u64 *hole_off; u8 *hole_chr;       // hole starts
	u64 *hole_end;                     // hole ends (exclusive offsets)
	u64 *hdr_pos, *hdr_off;            // header lines: chunk byte position of the '>', bases before it
	u64 *err;                          // max of fa_error(): the first rejected byte of the chunk
	const u64 *jump;                   // 48 x (a, c): the lrand48 step applied 2^j times
};
IDX_DEVFN u64 fa_error(u64 pos, int kind) { return ((1ull << 40) - pos) << 8 | (u64)kind; }

// X_k of the lrand48 stream after srand48(11): X_0 = 11 << 16 | 0x330E, X_{k+1} = a X_k + c (mod 2^48)
IDX_DEVFN u64 fa_rand_at(const u64 *jump, u64 k)
{
	u64 x = (11ull << 16) | 0x330Eull;
	for (int j = 0; j < 48 && (k >> j); ++j)
		if (k >> j & 1) x = (jump[2 * j] * x + jump[2 * j + 1]) & ((1ull << 48) - 1);
	return x;
}

// One byte b at chunk position pos (nb: the byte after it, -1 at the end of the stream) on top of st composed with d.
template <bool EMIT>
IDX_DEVFN void fa_byte(u32 b, int nb, u64 pos, bool &ls, const FaSum &st, FaSum &d, const FaSum &base, const FaOut &o, u64 &x, bool &have_x)
{
	const bool at_ls = ls;
	ls = b == '\n';
	const u32 pt = d.pt ? d.pt : st.pt;
	if (at_ls) {
		if (b == '\n') return;                                                   // empty line
		if (b == '>') {
			if (EMIT) { const u64 h = st.nh + d.nh - base.nh; o.hdr_pos[h] = pos; o.hdr_off[h] = st.nk + d.nk; }
			d.pt = FA_LT_HDR; ++d.nh; d.hs = 1;
			return;
		}
		if (b == '+' || b == '@') { if (EMIT) atomicMax(o.err, fa_error(pos, FA_ERR_FASTQ)); return; }
		d.pt = FA_LT_SEQ;
	} else if (pt != FA_LT_SEQ || b == '\n') return;                            // header text, or a sequence line's end
	if (b == 0 || b >= 0x80) { if (EMIT) atomicMax(o.err, fa_error(pos, FA_ERR_BYTE)); return; }
	// the line's trailing '\r' (pt: the type of the line before this one when b starts a line)
	if (b == '\r' && (nb == '\n' || (nb < 0 && !at_ls)) && (!at_ls || pt == FA_LT_SEQ)) return;
	// a base: the state before it is st composed with d
	const u32 lk = d.lk ? d.lk : st.lk, hs = d.lk ? d.hs : (st.hs | d.hs);
	const u32 lasts = (hs || !lk) ? 0u : (lk & 0xFFu);                            // previous raw byte of this record (add1's `lasts`)
	const bool prev_amb = lk && !fa_is_acgt(lk & 0xFFu);
	const bool run_break = lasts != b;
	const bool amb = !fa_is_acgt(b);
	const u64 off = st.nk + d.nk;
	if (run_break && prev_amb) { if (EMIT) o.hole_end[st.ne + d.ne - base.ne] = off; ++d.ne; }
	if (amb && run_break) { if (EMIT) { const u64 h = st.ns + d.ns - base.ns; o.hole_off[h] = off; o.hole_chr[h] = (u8)b; } ++d.ns; }
	if (EMIT) {
		u32 c;
		if (amb) {
			x = have_x ? (0x5DEECE66Dull * x + 0xBull) & ((1ull << 48) - 1) : fa_rand_at(o.jump, st.na + d.na + 1);
			have_x = true;
			c = (u32)(x >> 17) & 3u;                                               // lrand48() & 3
		} else c = fa_code(b);
		o.codes[off - base.nk] = (u8)c;
	}
	if (amb) ++d.na;
	++d.nk; d.lk = 0x100u | b; d.hs = 0;
}

// Walk one segment (n bytes at chunk position pos0) from state st; returns what the segment adds (a FaSum to compose onto st).
// ls0: the segment's first byte starts a line; after: the byte after the segment (-1 at the end of the stream).
template <bool EMIT>
IDX_DEVFN FaSum fa_walk(const u8 *seg, int n, u64 pos0, bool ls0, int after, const FaSum &st, const FaSum &base, const FaOut &o)
{
	FaSum d = fa_zero();
	bool ls = ls0;
	u64 x = 0; bool have_x = false;
#pragma unroll
	for (int j = 0; j < FA_SEG; ++j)                  // (unrolled: seg stays in registers)
		if (j < n) fa_byte<EMIT>(seg[j], j + 1 < n ? (int)seg[j + 1 < FA_SEG ? j + 1 : FA_SEG - 1] : after, pos0 + (u64)j, ls, st, d, base, o, x, have_x);
	return d;
}

// exclusive block scan of one FaSum per lane (Hillis-Steele in LDS); *total = the block's sum
IDX_DEVFN FaSum fa_block_scan(FaSum v, FaSum *total)
{
	__shared__ FaSum sh[FA_BLOCK];
	const int t = threadIdx.x;
	const FaCombine op;
	sh[t] = v;
	__syncthreads();
	for (int dlt = 1; dlt < FA_BLOCK; dlt <<= 1) {
		const FaSum w = t >= dlt ? op(sh[t - dlt], sh[t]) : sh[t];
		__syncthreads();
		sh[t] = w;
		__syncthreads();
	}
	const FaSum ex = t ? sh[t - 1] : fa_zero();
	if (total) *total = sh[FA_BLOCK - 1];
	__syncthreads();
	return ex;
}

// Pass P of a chunk (buf[0..n)): tile sums of the fields of pass P into tsum (P < 4), or the outputs (P == 4).
// tscan: inclusive scan of the previous pass's tile sums (P > 1); carry: the state before the chunk; ls0: buf[0] starts a line.
template <int P>
__global__ void __launch_bounds__(FA_BLOCK) k_fa_pass(const u8 *buf, u64 n, int eof, int ls0, FaSum carry, const FaSum *tscan, FaSum *tsum, FaOut o)
{
	const FaCombine op;
	const u64 tile = blockIdx.x;
	const u64 s0 = tile * FA_TILE + (u64)threadIdx.x * FA_SEG;
	u8 seg[FA_SEG];
	int len = 0;
	if (s0 + FA_SEG <= n) {
		const uint4 *p = (const uint4*)(buf + s0);
		const uint4 a = p[0], b = p[1];
		const u32 w[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
#pragma unroll
		for (int k = 0; k < FA_SEG; ++k) seg[k] = (u8)(w[k >> 2] >> ((k & 3) * 8));
		len = FA_SEG;
	} else {
#pragma unroll
		for (int k = 0; k < FA_SEG; ++k) seg[k] = s0 + (u64)k < n ? buf[s0 + k] : 0;
		len = s0 < n ? (int)(n - s0 < FA_SEG ? n - s0 : FA_SEG) : 0;
	}
	const bool ls = s0 == 0 ? ls0 != 0 : (s0 < n && buf[s0 - 1] == '\n');
	const int after = s0 + FA_SEG < n ? (int)buf[s0 + FA_SEG] : (eof ? -1 : 0);   // (a chunk never ends in '\r' unless the stream does)
	const FaSum in = (P > 1 && tile) ? op(carry, tscan[tile - 1]) : carry;
	FaSum x = fa_zero(), tot;
	for (int q = 1; q < P; ++q) {                       // after round q the lane prefixes hold the fields of passes <= q
		const FaSum d = fa_walk<false>(seg, len, s0, ls, after, op(in, x), carry, o);
		x = fa_block_scan(d, nullptr);
	}
	if (P < 4) {
		const FaSum d = fa_walk<false>(seg, len, s0, ls, after, op(in, x), carry, o);
		(void)fa_block_scan(d, &tot);
		if (threadIdx.x == 0) tsum[tile] = tot;
	} else
		(void)fa_walk<true>(seg, len, s0, ls, after, op(in, x), carry, o);
}

// .pac bytes of the bases [l0, l0 + nk): byte q of the output is pac byte (l0 >> 2) + q, holding only this chunk's bases
__global__ void __launch_bounds__(IDX_BLOCK) k_fa_pack(const u8 *codes, u64 l0, u64 nk, u8 *out, u64 n_out)
{
	for (u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x; q < n_out; q += (u64)gridDim.x * blockDim.x) {
		u32 v = 0;
		for (int k = 0; k < 4; ++k) {
			const u64 p = ((l0 >> 2) + q) * 4 + (u64)k;
			if (p >= l0 && p < l0 + nk) v |= (u32)codes[p - l0] << ((3 - k) * 2);
		}
		out[q] = (u8)v;
	}
}
