// dev_fasta_reads.h -- `bwa mem`'s reader for FASTA read files on the device (included by bwagpu_index.hip behind dev_fastq.h;
// host side: bwagpu_fastq_batch_fasta*).
//
// What it reproduces: the FASTA half of kseq_read (kseq.h:175-204, ks_getuntil2 :95-143) followed by bseq_read's batch rule with
// trim_readno and kseq2bseq1 (bwa.c:54-112) and the base recode of nst_nt4_table -- dev_fastq.h's job for records without a '+' line.
//
// The rule.  A line is what lies between two '\n', or between a '\n' and the end of the window; the first byte of a line says what it is:
//   '>'         a header: name up to the first isspace() byte, comment the rest of the line when there was such a byte, less one trailing
//               '\r' when the comment is longer than one byte (kseq.h:140); trim_readno on the name;
//   (nothing)   an empty line, skipped (kseq.h:193);
//   '@'         the header of a FASTQ record: that record is declined;
//   '+'         kseq_read would go on to read qualities: the record holding the line is declined;
//   otherwise   a sequence line of the record whose header precedes it.  Its bases are its bytes, less a '\r' at its end when the line has
//               two bytes or more.  A NUL, a byte >= 0x80 or a byte <= ' ' anywhere else in the line declines the record (the reference
//               would keep such a byte as a base, or index nst_nt4_table out of bounds).
// A record reaches from its header line to the next header line, or to the end of the window at eof: empty lines behind its bases are
// its own.  A record without bases is declined (the reference delivers an empty read), and so is a window that does not start with '>'.
// The three corner shapes of a line that is only "\r" (dev_fasta.h:10-17):
//   - behind at least one base of its record and before a '\n': the reference drops the '\r' (the record then holds more than one byte);
//     so does the device -- a CRLF file's empty lines;
//   - as the first sequence line of its record: the reference keeps the '\r' as the record's first base; the record is declined;
//   - as the last line of the stream, without a '\n': ks_getuntil2 returns early and the '\r' stays a base; the record is declined.
// A last line of one base without a '\n' is read as any other line.
//
// Why this is exact: what a line is follows from its first byte alone, and what a record is from the header lines before it, so every
// record before the first declined one is cut and read as kseq_read does it, from any window that starts at a '>'.  A record's end is in
// view when the next header line starts in the window or eof is set; only such records are candidates.
//
// Passes (tiles, segments and loads as in dev_fastq.h; FqWin::nl holds every newline of the window here):
//   1. k_fq_count as it is; k_fr_index: newline positions, and a flag on every line with a byte a sequence line may not hold.
//   2. k_fr_lines: one lane per line: its type, the bases it adds, whether it declines its record.  The (headers, bases, "\r"-only lines)
//      of the lines are scanned (rocPRIM): headers before a line give its record, bases before it its place in the read.
//   3. k_fr_place: header line of every record, the first declined record (atomicMax of a complement).  k_fr_records: one lane per
//      record (per pair of records r of both windows): name, trim_readno, comment, first base line (a binary search in the scan), the
//      lengths for the scan over records.  Cut and status are dev_fastq.h's (fq_cut_unit, fq_decide_status) over FrFmt.
//   4. k_fr_emit: one wavefront per read; names and comments as k_fq_emit copies them; the bases are gathered over the record's body
//      FR_STEP bytes a step: a ballot marks the bytes kept, a lane writes at the step's base plus the kept bytes below it.
#pragma once

#define FR_STEP FQ_WAVE                        // body bytes per emit step: one per lane

enum { FR_W_RECS = 5 /* +k: header lines of window k */ };      // (words 5 and 6 of dev_fastq.h's FQ_N_WORDS)
enum { FR_L_BYTE = 1 /* k_fr_index: a byte no sequence line may hold */, FR_L_HDR = 2, FR_L_BAD = 4 /* the line declines its record */ };

struct FrLine { u32 h, b, c; };                // a line's header (0 / 1), bases, "\r"-only (0 / 1); scanned: counts up to and including it
struct FrLinePlus {
	__host__ __device__ FrLine operator()(const FrLine &a, const FrLine &b) const { FrLine r; r.h = a.h + b.h; r.b = a.b + b.b; r.c = a.c + b.c; return r; }
};
// what a window has on top of its FqWin
struct FrWin {
	u8 *lflag;                                 // per line: FR_L_*
	FrLine *lines, *lscan;                     // per line, and their inclusive scan
	u32 *hline;                                // per record: its header's line; behind the last record: the number of lines
	u32 *bend;                                 // per candidate record: the window offset behind its body
};
struct FrArgs { FrWin x[2]; u32 cap_lines; };

// lines of window k: its newlines, and what lies behind the last one
IDX_DEVFN u32 fr_n_lines(const FqWin &W, const u64 *words, int k)
{
	return (u32)words[FQ_W_LINES + k] + ((W.n && W.buf[W.n - 1] != '\n') ? 1u : 0u);
}
IDX_DEVFN u32 fr_line_start(const FqWin &W, u32 l) { return l ? W.nl[l - 1] + 1u : 0u; }
IDX_DEVFN u32 fr_line_end(const FqWin &W, const u64 *words, int k, u32 l) { return l < (u32)words[FQ_W_LINES + k] ? W.nl[l] : W.n; }

// pass 1b: newline positions and the lines that hold a byte which declines a sequence line
__global__ void __launch_bounds__(FQ_BLOCK) k_fr_index(FqArgs A, FrArgs X, const u64 *tbase, u64 *words)
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
	bool flag = false;
#pragma unroll
	for (int j = 0; j < FQ_SEG; ++j) {
		if (j < len) {
			const u32 b = seg[j];
			if (b == '\n') {
				if (line < W.nl_cap) { W.nl[line] = s0 + (u32)j; if (flag) X.x[k].lflag[line] = FR_L_BYTE; }
				flag = false;
				++line;
			} else if (prev == '\r' || (b <= ' ' && b != '\r') || b >= 0x80) flag = true;      // (a '\r' counts once the byte behind it is known)
			prev = b;
		}
	}
	if (flag && line < W.nl_cap) X.x[k].lflag[line] = FR_L_BYTE;
	if (tile + 1 == W.tile0 + W.n_tiles && threadIdx.x == 0) words[FQ_W_LINES + k] = line0 + tot;
}

// pass 2: one lane per line (line i of every window).  Entries behind a window's last line are zero: the scan runs over cap_lines
__global__ void __launch_bounds__(FQ_BLOCK) k_fr_lines(FqArgs A, FrArgs X, const u64 *words)
{
	for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < X.cap_lines; i += (u64)gridDim.x * blockDim.x) {
		for (int k = 0; k < A.nw; ++k) {
			const FqWin &W = A.w[k];
			if (i >= W.nl_cap) continue;
			FrLine s; s.h = s.b = s.c = 0;
			u32 f = 0;
			if (i < fr_n_lines(W, words, k)) {
				const u32 st = fr_line_start(W, (u32)i), en = fr_line_end(W, words, k, (u32)i), len = en - st;
				const u32 c0 = len ? W.buf[st] : 0u;
				if (c0 == '>' || c0 == '@') { s.h = 1; f = FR_L_HDR | (c0 == '@' ? FR_L_BAD : 0); }
				else if (len) {
					bool bad = (X.x[k].lflag[i] & FR_L_BYTE) || c0 == '+';
					if (len == 1 && c0 == '\r') { s.c = 1; bad = bad || (en == W.n && W.eof); }      // (at the stream's end the reference keeps it)
					else s.b = len - (W.buf[en - 1] == '\r' ? 1u : 0u);
					f = bad ? FR_L_BAD : 0;
				}
			}
			X.x[k].lflag[i] = (u8)f;
			X.x[k].lines[i] = s;
		}
	}
}

// pass 3a: one lane per line: the records' header lines, their number, and the records that a line declines
__global__ void __launch_bounds__(FQ_BLOCK) k_fr_place(FqArgs A, FrArgs X, u64 *words)
{
	for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < X.cap_lines; i += (u64)gridDim.x * blockDim.x) {
		for (int k = 0; k < A.nw; ++k) {
			const FqWin &W = A.w[k];
			const u32 L = fr_n_lines(W, words, k);
			if (i == 0 && L == 0) X.x[k].hline[0] = 0;
			if (i >= L) continue;
			const u32 f = X.x[k].lflag[i], h = X.x[k].lscan[i].h;
			if (f & FR_L_HDR) X.x[k].hline[h - 1] = (u32)i;
			if ((f & FR_L_BAD) || (i == 0 && W.buf[0] != '>')) atomicMax(&words[FQ_W_BAD + k], FQ_BIG - (u64)(h ? h - 1 : 0));
			if (i + 1 == L) { X.x[k].hline[h] = L; words[FR_W_RECS + k] = h; }
		}
	}
}

// how dev_fastq.h's cut and status see a window of FASTA records
struct FrFmt {
	FrArgs X;
	// candidate records of window k: those whose end is in view
	IDX_DEVFN u64 n_records(const FqArgs &A, const u64 *words, int k) const
	{
		const u64 R = words[FR_W_RECS + k];
		return (A.w[k].eof || !R) ? R : R - 1;
	}
	// leading records the device takes; *has_bad: a record in view behind them is declined (a last one without its end included)
	IDX_DEVFN u64 n_good(const FqArgs &A, const u64 *words, int k, bool *has_bad) const
	{
		const u64 R = n_records(A, words, k), w = words[FQ_W_BAD + k];
		const u64 bad = w ? FQ_BIG - w : ~0ull;
		if (has_bad) *has_bad = bad <= R;
		return bad < R ? bad : R;
	}
	// window offset at which record g of window k starts (a window starts at a record start); behind the last record: the window's length
	IDX_DEVFN u32 start(const FqArgs &A, const u64 *words, int k, u64 g) const
	{
		const FqWin &W = A.w[k];
		const u32 l = g ? X.x[k].hline[g] : 0u;
		return l < fr_n_lines(W, words, k) ? fr_line_start(W, l) : W.n;
	}
};

// pass 3b: one lane per unit (record i of every window), as k_fq_records
__global__ void __launch_bounds__(FQ_BLOCK) k_fr_records(FqArgs A, FrFmt F, u64 *words, FqSum *units)
{
	for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < A.cap_units; i += (u64)gridDim.x * blockDim.x) {
		FqSum s; s.seq = s.name = s.com = 0;
		bool all = true;
		for (int k = 0; k < A.nw; ++k) {
			const FqWin &W = A.w[k];
			const FrWin &Y = F.X.x[k];
			if (i >= F.n_records(A, words, k)) { all = false; continue; }
			const u32 H = Y.hline[i], N = Y.hline[i + 1];
			const FrLine at = Y.lscan[H];
			const u32 ls = Y.lscan[N - 1].b - at.b;
			// the first line that adds a base: lscan.b does not decrease
			u32 lo = H + 1, hi = N;
			while (lo < hi) { const u32 m = (lo + hi) >> 1; if (Y.lscan[m].b > at.b) hi = m; else lo = m + 1; }
			bool bad = ls == 0 || Y.lscan[lo].c != at.c;                   // no base, or a "\r"-only line before the first one
			const u8 *b = W.buf;
			const u32 st = fr_line_start(W, H), n1 = fr_line_end(W, words, k, H);
			bad = bad || b[st] != '>';
			bwagpu_fastq_rec_t r;
			r.file = k; r.has_comment = 0; r.name = (int32_t)st; r.l_name = 0; r.comment = (int32_t)n1; r.l_comment = 0;
			r.seq = (int32_t)(ls ? fr_line_start(W, lo) : n1); r.l_seq = (int32_t)ls; r.qual = -1; r.l_qual = 0;
			if (!bad) {
				const u32 h = st + 1;
				u32 p = h;
				while (p < n1 && !fq_isspace(b[p])) ++p;
				u32 ln = p - h;
				if (p < n1) {
					u32 lc = n1 - p - 1;
					if (lc > 1 && b[n1 - 1] == '\r') --lc;                  // ks_getuntil2's trailing '\r'
					r.has_comment = 1; r.comment = (int32_t)(p + 1); r.l_comment = (int32_t)lc;
				}
				if (ln > 2 && b[h + ln - 2] == '/' && b[h + ln - 1] >= '0' && b[h + ln - 1] <= '9') ln -= 2;      // trim_readno
				r.name = (int32_t)h; r.l_name = (int32_t)ln;
			} else atomicMax(&words[FQ_W_BAD + k], FQ_BIG - i);
			W.recs[i] = r;
			Y.bend[i] = F.start(A, words, k, i + 1);
			s.seq += ls; s.name += (u64)r.l_name; s.com += (u64)r.l_comment;
		}
		if (!all) s.seq = s.name = s.com = 0;
		units[i] = s;
	}
}

__global__ void __launch_bounds__(FQ_BLOCK) k_fr_cut(FqArgs A, FrFmt F, u64 *words, const FqSum *uscan, u64 chunk) { fq_cut_unit(A, F, words, uscan, chunk); }
__global__ void __launch_bounds__(FQ_WAVE) k_fr_decide(FqArgs A, FrFmt F, const u64 *words, const FqSum *uscan, FqInfo *info) { fq_decide_status(A, F, words, uscan, info); }

// pass 4: one wavefront per read.  o.quals is not written: a FASTA read has no qualities
__global__ void __launch_bounds__(FQ_BLOCK) k_fr_emit(FqArgs A, FrArgs X, const FqSum *uscan, u64 n_reads, FqSum total, FqOut o)
{
	const u32 lane = threadIdx.x & (FQ_WAVE - 1);
	const u64 below = (1ull << lane) - 1;
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
			o.off[j] = (i64)at.seq; o.name_off[j] = (i64)at.name; o.comment_off[j] = (i64)at.com; o.has_comment[j] = (u8)r.has_comment; o.recs[j] = W.recs[u];
			if (j + 1 == n_reads) { o.off[n_reads] = (i64)total.seq; o.name_off[n_reads] = (i64)total.name; o.comment_off[n_reads] = (i64)total.com; }
		}
		const u8 *b = W.buf;
		for (u32 t = lane; t < (u32)r.l_name; t += FQ_WAVE) o.names[at.name + t] = (char)b[(u32)r.name + t];
		for (u32 t = lane; t < (u32)r.l_comment; t += FQ_WAVE) o.comments[at.com + t] = (char)b[(u32)r.comment + t];
		// the body: every byte of a taken record's sequence lines that is no '\n' and no '\r' is a base
		const u32 e = (k ? X.x[1].bend : X.x[0].bend)[u];
		u64 dst = at.seq;
		for (u32 p0 = (u32)r.seq; p0 < e; p0 += FR_STEP) {
			const u32 p = p0 + lane;
			const u32 c = p < e ? b[p] : (u32)'\n';
			const bool keep = c != '\n' && c != '\r';
			const u64 m = __ballot(keep);
			if (keep) o.seqs[dst + (u64)__popcll(m & below)] = (u8)fq_nt4(c);
			dst += (u64)__popcll(m);
		}
	}
}
