// dev_fastq.h -- `bwa mem`'s FASTQ reader on the device (included by bwagpu_index.hip; host side: bwagpu_fastq_*).
//
// What it reproduces: kseq_read (kseq.h:175-215, ks_getuntil2 :95-143) followed by bseq_read's batch rule with trim_readno and
// kseq2bseq1 (bwa.c:54-112), and the base recode of mem_align1_core (nst_nt4_table, bntseq.c:46-63) -- for PLAIN records only.
//
// The rule (the one parse_fast_record of host/host_input.h applies on the host).  A record is plain when
//   - it has four lines, all four newlines are there, and the first line starts with '@';
//   - its third line starts with '+';
//   - sequence and quality line have the same non-zero length;
//   - no '\r' stands before the first, second or fourth newline;
//   - the sequence line does not start with '>', '+' or '@';
//   - no byte of the sequence line is <= ' ';
//   - (device only) no byte of the sequence line is >= 0x80: the reference indexes nst_nt4_table with a signed char there.
// For such a record kseq_read delivers: name = the header up to the first isspace() byte (the six C-locale ones), comment = the
// rest of the header line when there was such a byte (it may be empty), bases and qualities = lines two and four.
//
// Why this is exact: a window starts at a record start.  Every record before the first non-plain one is read as kseq_read reads
// it, so by induction each of them starts at a record start too, and the line number mod 4 of every byte before the first
// non-plain record says which field the byte belongs to.  At the first record that is not plain the device stops and says
// where; what lies behind it is never interpreted.
//
// Passes (a window is cut into tiles of FQ_TILE bytes, a tile into FQ_SEG-byte segments, one per lane, two 16-byte loads each):
//   1. k_fq_count: newlines per tile; the tile counts are scanned (rocPRIM).  k_fq_index: the position of newline j goes to
//      nl[j], and the byte-wise checks run on the same loads with the byte's line number mod 4: '\r' before the newline of lines
//      0, 1, 3 and the forbidden bytes of line 1.  A violation lowers the window's first bad record (an atomicMax of its complement).
//   2. k_fq_records: one lane per candidate record (lines 4r .. 4r + 3; for two windows one lane takes record r of both): first
//      bytes, equal lengths, name end, trim_readno; one table entry per record, and the record's (pair's) lengths for the scan.
//   3. The lengths are scanned; k_fq_cut finds the first index at which bseq_read stops (bwa.c:104), k_fq_decide the status.
//   4. k_fq_emit: one wavefront per read copies name, comment and qualities and recodes the bases, at the offsets the scan gave;
//      two windows interleave as reads 2i, 2i + 1.
// nl holds at most n / 2 + 8 positions for a window of n bytes: a plain record has at least 8 bytes and 4 newlines, so a
// window with more newlines than that has a non-plain record among the candidates the array still covers.
#pragma once

#define FQ_BLOCK 256
#define FQ_SEG 32                              // bytes per lane: two 16-byte loads
#define FQ_TILE (FQ_BLOCK * FQ_SEG)
#define FQ_WAVE 64
#define FQ_BIG (1ull << 40)                    // bad word of a window: FQ_BIG - (first non-plain record), 0: none

// one window on the device
struct FqWin {
	const u8 *buf; u32 n;                      // the bytes
	u32 tile0, n_tiles;                        // its tiles among the call's
	u32 *nl; u32 nl_cap;                       // newline positions
	bwagpu_fastq_rec_t *recs; u32 rec_cap;     // candidate records (nl_cap / 4)
	int eof;
};
struct FqArgs { FqWin w[2]; int nw; u32 cap_units; };

// lengths of a record (one window) or of a pair (two), and what the scan makes of them
struct FqSum { u64 seq, name, com; };
struct FqPlus {
	__host__ __device__ FqSum operator()(const FqSum &a, const FqSum &b) const { FqSum r; r.seq = a.seq + b.seq; r.name = a.name + b.name; r.com = a.com + b.com; return r; }
};

// words of the call's state (u64 each; zeroed before the first kernel)
enum { FQ_W_BAD = 0 /* +k */, FQ_W_LINES = 2 /* +k: newlines of window k */, FQ_W_CUT = 4 /* index of the last unit of the batch + 1 */, FQ_N_WORDS = 8 };
// what k_fq_decide leaves for the host
struct FqInfo { i64 status, n_units, consumed[2], declined_file, declined_at; FqSum total; };

IDX_DEVFN bool fq_isspace(u32 c) { return c == ' ' || (c >= '\t' && c <= '\r'); }
IDX_DEVFN u32 fq_nt4(u32 c)
{
	const u32 u = c & 0xDFu;
	return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : c == '-' ? 5u : 4u;
}

// exclusive block scan of one count per lane (Hillis-Steele in LDS); *total = the block's sum
IDX_DEVFN u32 fq_block_scan(u32 v, u32 *total)
{
	__shared__ u32 sh[FQ_BLOCK];
	const int t = threadIdx.x;
	sh[t] = v;
	__syncthreads();
	for (int d = 1; d < FQ_BLOCK; d <<= 1) {
		const u32 w = t >= d ? sh[t - d] + sh[t] : sh[t];
		__syncthreads();
		sh[t] = w;
		__syncthreads();
	}
	const u32 ex = t ? sh[t - 1] : 0u;
	*total = sh[FQ_BLOCK - 1];
	__syncthreads();
	return ex;
}

// the lane's segment of its tile: bytes to seg (zero past the window's end), their number returned
IDX_DEVFN int fq_load(const FqWin &W, u32 s0, u8 *seg)
{
	if (s0 + FQ_SEG <= W.n) {
		const uint4 *p = (const uint4*)(W.buf + s0);
		const uint4 a = p[0], b = p[1];
		const u32 w[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
#pragma unroll
		for (int k = 0; k < FQ_SEG; ++k) seg[k] = (u8)(w[k >> 2] >> ((k & 3) * 8));
		return FQ_SEG;
	}
#pragma unroll
	for (int k = 0; k < FQ_SEG; ++k) seg[k] = s0 + (u32)k < W.n ? W.buf[s0 + k] : 0;
	return s0 < W.n ? (int)(W.n - s0) : 0;
}

// pass 1a: newlines per tile
__global__ void __launch_bounds__(FQ_BLOCK) k_fq_count(FqArgs A, u64 *tcount)
{
	const u32 tile = blockIdx.x;
	const FqWin &W = A.w[(A.nw > 1 && tile >= A.w[1].tile0) ? 1 : 0];
	const u32 s0 = (tile - W.tile0) * FQ_TILE + threadIdx.x * FQ_SEG;
	u8 seg[FQ_SEG];
	const int len = fq_load(W, s0, seg);
	u32 c = 0, tot;
#pragma unroll
	for (int j = 0; j < FQ_SEG; ++j) c += (j < len && seg[j] == '\n') ? 1u : 0u;
	(void)fq_block_scan(c, &tot);
	if (threadIdx.x == 0) tcount[tile] = tot;
}

// pass 1b: newline positions and the byte-wise checks.  tbase: exclusive scan of tcount over all tiles of the call
__global__ void __launch_bounds__(FQ_BLOCK) k_fq_index(FqArgs A, const u64 *tbase, u64 *words)
{
	const u32 tile = blockIdx.x;
	const int k = (A.nw > 1 && tile >= A.w[1].tile0) ? 1 : 0;
	const FqWin &W = A.w[k];
	const u32 s0 = (tile - W.tile0) * FQ_TILE + threadIdx.x * FQ_SEG;
	u8 seg[FQ_SEG];
	const int len = fq_load(W, s0, seg);
	u32 c = 0, tot;
#pragma unroll
	for (int j = 0; j < FQ_SEG; ++j) c += (j < len && seg[j] == '\n') ? 1u : 0u;
	const u32 ex = fq_block_scan(c, &tot);
	const u64 line0 = tbase[tile] - tbase[W.tile0];
	u64 line = line0 + ex;
	u32 prev = (len > 0 && s0 > 0) ? W.buf[s0 - 1] : 0u;
	u64 vmin = ~0ull;
#pragma unroll
	for (int j = 0; j < FQ_SEG; ++j) {
		if (j < len) {
			const u32 b = seg[j];
			if (b == '\n') {
				if (line < W.nl_cap) W.nl[line] = s0 + (u32)j;
				if ((line & 3) != 2 && prev == '\r' && (line >> 2) < vmin) vmin = line >> 2;
				++line;
			} else if ((line & 3) == 1 && (b <= ' ' || b >= 0x80) && (line >> 2) < vmin) vmin = line >> 2;
			prev = b;
		}
	}
	if (vmin != ~0ull) atomicMax(&words[FQ_W_BAD + k], FQ_BIG - vmin);
	if (tile + 1 == W.tile0 + W.n_tiles && threadIdx.x == 0) words[FQ_W_LINES + k] = line0 + tot;
}

// complete candidate records of window k
IDX_DEVFN u64 fq_n_records(const FqArgs &A, const u64 *words, int k)
{
	const u64 L = words[FQ_W_LINES + k];
	return (L < A.w[k].nl_cap ? L : (u64)A.w[k].nl_cap) >> 2;
}
// leading plain records of window k; *has_bad: a complete candidate record behind them is not plain
IDX_DEVFN u64 fq_n_good(const FqArgs &A, const u64 *words, int k, bool *has_bad)
{
	const u64 R = fq_n_records(A, words, k), w = words[FQ_W_BAD + k];
	const u64 bad = w ? FQ_BIG - w : ~0ull;
	const bool hb = bad < R || words[FQ_W_LINES + k] > A.w[k].nl_cap;
	if (has_bad) *has_bad = hb;
	return bad < R ? bad : R;
}
// window offset at which record g of window k starts
IDX_DEVFN u32 fq_start(const FqWin &W, u64 g) { return g ? W.nl[4 * g - 1] + 1u : 0u; }
// how the cut and the status see a window of plain FASTQ records (dev_fasta_reads.h has the FASTA one)
struct FqPlainFmt {
	IDX_DEVFN u64 n_good(const FqArgs &A, const u64 *words, int k, bool *has_bad) const { return fq_n_good(A, words, k, has_bad); }
	IDX_DEVFN u32 start(const FqArgs &A, const u64 *, int k, u64 g) const { return fq_start(A.w[k], g); }
};

// pass 2: one lane per unit (record i of every window).  units[i]: the lengths its records add to the batch (zero past the last
// complete candidate of any window, so that the scan may run over cap_units entries)
__global__ void __launch_bounds__(FQ_BLOCK) k_fq_records(FqArgs A, u64 *words, FqSum *units)
{
	for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < A.cap_units; i += (u64)gridDim.x * blockDim.x) {
		FqSum s; s.seq = s.name = s.com = 0;
		bool all = true;
		for (int k = 0; k < A.nw; ++k) {
			const FqWin &W = A.w[k];
			if (i >= fq_n_records(A, words, k)) { all = false; continue; }
			const uint4 e = *(const uint4*)(W.nl + 4 * i);
			const u32 st = fq_start(W, i), n1 = e.x, n2 = e.y, n3 = e.z, n4 = e.w;
			const u32 sq = n1 + 1, ls = n2 - sq, ql = n3 + 1, lq = n4 - ql;
			const u8 *b = W.buf;
			bool bad = b[st] != '@' || b[n2 + 1] != '+' || ls == 0 || ls != lq;
			if (!bad) { const u32 c = b[sq]; bad = c == '>' || c == '+' || c == '@'; }
			bwagpu_fastq_rec_t r;
			r.file = k; r.has_comment = 0; r.name = (int32_t)st; r.l_name = 0; r.comment = (int32_t)n1; r.l_comment = 0;
			r.seq = (int32_t)sq; r.l_seq = (int32_t)ls; r.qual = (int32_t)ql; r.l_qual = (int32_t)lq;
			if (!bad) {
				const u32 h = st + 1;
				u32 p = h;
				while (p < n1 && !fq_isspace(b[p])) ++p;
				u32 ln = p - h;
				if (p < n1) { r.has_comment = 1; r.comment = (int32_t)(p + 1); r.l_comment = (int32_t)(n1 - p - 1); }
				if (ln > 2 && b[h + ln - 2] == '/' && b[h + ln - 1] >= '0' && b[h + ln - 1] <= '9') ln -= 2;      // trim_readno
				r.name = (int32_t)h; r.l_name = (int32_t)ln;
			} else atomicMax(&words[FQ_W_BAD + k], FQ_BIG - i);
			W.recs[i] = r;
			s.seq += ls; s.name += (u64)r.l_name; s.com += (u64)r.l_comment;
		}
		if (!all) s.seq = s.name = s.com = 0;
		units[i] = s;
	}
}

// pass 3a: the unit behind which bseq_read closes the batch (bwa.c:104): the first one with sum(l_seq) >= chunk -- at an even
// read count, which two windows always have.  uscan: inclusive scan of units.  Sums do not decrease, so exactly one lane finds it.
template <class Fmt>
IDX_DEVFN void fq_cut_unit(const FqArgs &A, const Fmt &F, u64 *words, const FqSum *uscan, u64 chunk)
{
	u64 P = ~0ull;
	for (int k = 0; k < A.nw; ++k) { const u64 g = F.n_good(A, words, k, nullptr); if (g < P) P = g; }
	for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (u64)gridDim.x * blockDim.x) {
		if (uscan[i].seq < chunk || (i && uscan[i - 1].seq >= chunk)) continue;
		const u64 c = (A.nw > 1 || (i & 1)) ? i : i + 1;
		if (c < P) words[FQ_W_CUT] = c + 1;
	}
}
__global__ void __launch_bounds__(FQ_BLOCK) k_fq_cut(FqArgs A, u64 *words, const FqSum *uscan, u64 chunk) { fq_cut_unit(A, FqPlainFmt(), words, uscan, chunk); }

// pass 3b (one lane): status, batch size and totals
template <class Fmt>
IDX_DEVFN void fq_decide_status(const FqArgs &A, const Fmt &F, const u64 *words, const FqSum *uscan, FqInfo *info)
{
	if (blockIdx.x || threadIdx.x) return;
	enum { HAS, BAD, SHORT, ENDED };
	FqInfo o;
	o.status = BWAGPU_FQ_MORE; o.n_units = 0; o.consumed[0] = o.consumed[1] = 0; o.declined_file = -1; o.declined_at = -1;
	o.total.seq = o.total.name = o.total.com = 0;
	u64 good[2] = { 0, 0 }, P = ~0ull;
	for (int k = 0; k < A.nw; ++k) { good[k] = F.n_good(A, words, k, nullptr); if (good[k] < P) P = good[k]; }
	if (words[FQ_W_CUT]) { o.status = BWAGPU_FQ_CUT; o.n_units = (i64)words[FQ_W_CUT]; }
	else {
		int st[2] = { ENDED, ENDED };
		for (int k = 0; k < A.nw; ++k) {
			const FqWin &W = A.w[k];
			bool has_bad = false;
			(void)F.n_good(A, words, k, &has_bad);
			if (good[k] > P) st[k] = HAS;
			else if (has_bad) st[k] = BAD;
			else if (W.n - F.start(A, words, k, P) > 0) st[k] = W.eof ? BAD : SHORT;      // an incomplete last record
			else st[k] = W.eof ? ENDED : SHORT;
		}
		int decl = -1;
		for (int k = A.nw - 1; k >= 0; --k) if (st[k] == BAD) decl = k;
		if (decl < 0 && st[0] != SHORT && st[1] != SHORT && A.nw > 1 && st[0] != st[1]) decl = st[0] == HAS ? 0 : 1;   // one file ended, the other has records left
		if (decl >= 0) { o.status = BWAGPU_FQ_DECLINED; o.declined_file = decl; o.declined_at = (i64)F.start(A, words, decl, P); }
		else if (st[0] == SHORT || (A.nw > 1 && st[1] == SHORT)) o.status = BWAGPU_FQ_MORE;
		else { o.status = BWAGPU_FQ_END; o.n_units = (i64)P; }
	}
	if (o.n_units) {
		o.total = uscan[o.n_units - 1];
		for (int k = 0; k < A.nw; ++k) o.consumed[k] = (i64)F.start(A, words, k, (u64)o.n_units);
	}
	*info = o;
}
__global__ void __launch_bounds__(FQ_WAVE) k_fq_decide(FqArgs A, const u64 *words, const FqSum *uscan, FqInfo *info) { fq_decide_status(A, FqPlainFmt(), words, uscan, info); }

// where pass 4 writes
struct FqOut {
	u8 *seqs; i64 *off; char *names; i64 *name_off; char *quals; char *comments; i64 *comment_off; u8 *has_comment; bwagpu_fastq_rec_t *recs;
};

// pass 4: one wavefront per read
__global__ void __launch_bounds__(FQ_BLOCK) k_fq_emit(FqArgs A, const FqSum *uscan, u64 n_reads, FqSum total, FqOut o)
{
	const u32 lane = threadIdx.x & (FQ_WAVE - 1);
	const u64 wave0 = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / FQ_WAVE, n_waves = (u64)gridDim.x * blockDim.x / FQ_WAVE;
	for (u64 j = wave0; j < n_reads; j += n_waves) {
		const u64 u = A.nw > 1 ? j >> 1 : j;
		const int k = A.nw > 1 ? (int)(j & 1) : 0;
		const FqWin &W = A.w[k];
		const bwagpu_fastq_rec_t r = W.recs[u];
		FqSum at; at.seq = at.name = at.com = 0;
		if (u) at = uscan[u - 1];
		if (k) { const bwagpu_fastq_rec_t m = A.w[0].recs[u]; at.seq += (u64)m.l_seq; at.name += (u64)m.l_name; at.com += (u64)m.l_comment; }
		if (lane == 0) {
			o.off[j] = (i64)at.seq; o.name_off[j] = (i64)at.name; o.comment_off[j] = (i64)at.com; o.has_comment[j] = (u8)r.has_comment; o.recs[j] = r;
			if (j + 1 == n_reads) { o.off[n_reads] = (i64)total.seq; o.name_off[n_reads] = (i64)total.name; o.comment_off[n_reads] = (i64)total.com; }
		}
		const u8 *b = W.buf;
		for (u32 t = lane; t < (u32)r.l_name; t += FQ_WAVE) o.names[at.name + t] = (char)b[(u32)r.name + t];
		for (u32 t = lane; t < (u32)r.l_comment; t += FQ_WAVE) o.comments[at.com + t] = (char)b[(u32)r.comment + t];
		for (u32 t = lane; t < (u32)r.l_seq; t += FQ_WAVE) {
			o.seqs[at.seq + t] = (u8)fq_nt4(b[(u32)r.seq + t]);
			o.quals[at.seq + t] = (char)b[(u32)r.qual + t];
		}
	}
}
