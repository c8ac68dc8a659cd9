// dev_samtext.h -- the SAM text of reads on the device: mem_aln2sam (bwamem.c:851-976, add_cigar :838-849), what mem_reg2sam (bwamem.c:1033-1079) wraps
// around it, and the XA strings of mem_gen_alt (bwamem_extra.c:118-172).  The kernels here are the single-end ones (m == NULL), bwagpu_batch_sam /
// bwagpu_sam_flat (bwagpu.hip); the mate enters sam_line as a type (SamNoMate / SamMate), and the paired-end kernels are in dev_samtext_pe.h.
//
// Everything is read from what the earlier stages left in HBM: the alignment records (dev_alns.h), the marking records (dev_primary.h), the CIGAR records
// with their operation array and packed MD strings (dev_cigar.h), the reads in nt4; besides them the names, qualities and comments of the reads and the
// names and annotations of the contigs.
//
// One routine, sam_read<S, M>, writes all lines of a read into a sink S.  k_sam_size runs it on SamCount, which only counts; a prefix sum of the counts gives
// every read its place in the batch's text; k_sam_write runs the same routine on SamWrite.  The two passes cannot disagree: there is one formatter.
//
// Mapping: one wavefront per read in both passes, and the formatter's control flow is wave-uniform -- every lane runs every statement with the same values.
// SamWrite keeps SAM_STAGE bytes of the line in LDS.  Small pieces (digits, punctuation, tag names) are stored there by lane 0; bulk pieces (name, SEQ, QUAL,
// MD, comment, contig names) by all lanes, 64 bytes a step.  A full staging area goes to HBM with one byte per lane and store, so that a wavefront's stores
// cover consecutive bytes.  A small piece never straddles a flush (the area is flushed early when the piece does not fit); a bulk piece is cut where the
// area ends.  A line longer than the area therefore flushes in its middle, several times.
//
// XA without arrays: only a printed place k shows its XA, so for a printed k the marked list is scanned 64 places a step for the places i with
// secondary_all == k and score_i >= score_k * XA_drop_ratio (get_pri_idx); the population counts of the ballots are cnt[k] and has_alt[k], and when the hit
// limits let the string through a second scan writes the entries in the list's order.
//
// Declined reads (sam_declined): a printed region, or a region listed in a printed XA, without a CIGAR record (BWAGPU_ALN_NOCIGAR).  Zero bytes, bit 0 of the
// read's flag word; the caller formats such a read.
#pragma once
#include <limits.h>
#include "dev_common.h"
#include "dev_extw.h"
#include "dev_alns.h"

#define SAM_STAGE 512           // bytes of a wavefront's staging area in LDS (one wavefront per workgroup)
#define SAM_STEP 64             // places of a marked list a wavefront looks at per step

// what the kernels need besides the lists (device pointers)
struct SamIn {
	const bwagpu_aln_t *alns; const bwagpu_primary_t *pri; const bwagpu_cigar_t *cigs; const u32 *ops;   // records by the lists' offsets (CIGAR records by input index); operation array
	const u8 *seq; const i64 *seq_off;                   // the reads, nt4
	const char *names; const i64 *name_off;
	const char *quals;                                   // at the reads' offsets, or (null: '*')
	const char *comments; const i64 *comment_off;        // or (null: none)
	const char *rg; int rg_len;                          // -R's id, rg_len 0: none
	const char *ctg_text; const i64 *ctg_name_off, *ctg_anno_off;   // contig r: name at ctg_text + ctg_name_off[r], annotation at ctg_text + ctg_anno_off[r] (n_seqs + 1 offsets each)
	i32 extra_flag;
};

// one read as the formatter sees it
struct SamRead {
	const bwagpu_aln_t *alns; const bwagpu_primary_t *pri; const bwagpu_cigar_t *cigs; int n;
	const u8 *seq; const char *qual; int l_seq;
	const char *name; int l_name;
	const char *comment; int l_comment;
};

// ---- the sinks ------------------------------------------------------------------------------------------------------------------------------------------
// reserve(k): the next k <= 24 bytes will be given one by one with byte(place, c) and closed with advance(k); bulk(len, f): bytes f(0) .. f(len - 1)
struct SamCount {
	i64 n;
	DEVFN void reserve(int) {}
	DEVFN void byte(int, char) {}
	DEVFN void advance(int k) { n += k; }
	template <class F> DEVFN void bulk(i64 len, const F &) { if (len > 0) n += len; }
};
struct SamWrite {
	char *out; char *stage; int fill, lane;
	DEVFN void flush()
	{
		wave_sync();
		for (int i = lane; i < fill; i += 64) out[i] = stage[i];
		out += fill; fill = 0;
		wave_sync();      // (the area is read before anybody writes it again)
	}
	DEVFN void reserve(int k) { if (fill + k > SAM_STAGE) flush(); }
	DEVFN void byte(int at, char c) { if (lane == 0) stage[fill + at] = c; }
	DEVFN void advance(int k) { fill += k; }
	template <class F> DEVFN void bulk(i64 len, const F &f)
	{
		for (i64 done = 0; done < len; ) {
			if (fill == SAM_STAGE) flush();
			const i64 left = len - done;
			const int m = left < SAM_STAGE - fill ? (int)left : SAM_STAGE - fill;
			for (int j = lane; j < m; j += 64) stage[fill + j] = f(done + j);
			fill += m; done += m;
		}
	}
};

template <class S> DEVFN void sam_ch(S &s, char c) { s.reserve(1); s.byte(0, c); s.advance(1); }
template <class S, int N> DEVFN void sam_lit(S &s, const char (&z)[N])
{
	s.reserve(N - 1);
	for (int i = 0; i < N - 1; ++i) s.byte(i, z[i]);
	s.advance(N - 1);
}
// decimal text of v (kputw / kputl / "%d")
template <class S, class U> DEVFN void sam_digits(S &s, U u, int neg)
{
	int nd = 1;
	for (U t = u; t >= 10; t /= 10) ++nd;
	s.reserve(nd + neg);
	if (neg) s.byte(0, '-');
	for (int i = nd - 1; i >= 0; --i) { s.byte(neg + i, (char)('0' + (int)(u % 10))); u /= 10; }
	s.advance(nd + neg);
}
template <class S> DEVFN void sam_int(S &s, i64 v)
{
	const u64 u = v < 0 ? 0ull - (u64)v : (u64)v;
	if (u >> 32) sam_digits(s, u, v < 0); else sam_digits(s, (u32)u, v < 0);
}
template <class S> DEVFN void sam_bytes(S &s, const char *p, i64 n) { s.bulk(n, [&](i64 i) { return p[i]; }); }

DEVFN char sam_base(int c, u64 tab) { return (char)(tab >> (8 * (c < 5 ? c : 5))); }      // code 5 and above: the literal's NUL, as in the reference's table
#define SAM_FWD 0x4e54474341ull      // "ACGTN"
#define SAM_REV 0x4e41434754ull      // "TGCAN"
DEVFN char sam_op(int op) { return (char)(0x4e485344494dull >> (8 * (op < 6 ? op : 6))); }      // "MIDSHN"

// pa:f:%.3f of (double)score / alt_sc as glibc prints it: the exact binary value of the quotient rounded to three decimals, ties to even -- by integer
// arithmetic on the mantissa (1000 * M < 2^63).  alt_sc > 0, so the quotient is zero or a normal number below 2^31.
template <class S> DEVFN void sam_pa(S &s, int score, int alt_sc)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
	const double x = (double)score / alt_sc;
	u64 bits;
	__builtin_memcpy(&bits, &x, 8);
	const int e = (int)(bits >> 52 & 0x7ff);
	u64 q = 0;
	if (e != 0) {
		const u64 P = ((bits & ((1ull << 52) - 1)) | 1ull << 52) * 1000;      // |x| * 1000 = P * 2^-sh
		const int sh = 1075 - e;
		if (sh <= 0) q = P;
		else if (sh < 64) {
			q = P >> sh;
			const u64 rem = P & ((1ull << sh) - 1), half = 1ull << (sh - 1);
			if (rem > half || (rem == half && (q & 1))) ++q;
		}
	}
	sam_lit(s, "\tpa:f:");
	if (bits >> 63) sam_ch(s, '-');
	sam_int(s, (i64)(q / 1000));
	const int d = (int)(q % 1000);
	s.reserve(4);
	s.byte(0, '.'); s.byte(1, (char)('0' + d / 100)); s.byte(2, (char)('0' + d / 10 % 10)); s.byte(3, (char)('0' + d % 10));
	s.advance(4);
}

template <class S> DEVFN void sam_ctg_name(S &s, const SamIn &I, int rid)
{
	if (rid < 0) return;
	const i64 b = I.ctg_name_off[rid];
	sam_bytes(s, I.ctg_text + b, I.ctg_name_off[rid + 1] - b);
}

// the CIGAR of record R from the region's CIGAR record: clip5, the operations without a dropped deletion, clip3; the clips print as `clip`
template <class S> DEVFN void sam_cigar(S &s, const SamIn &I, const bwagpu_aln_t &R, const bwagpu_cigar_t *c, char clip)
{
	if (R.clip5) { sam_int(s, R.clip5); sam_ch(s, clip); }
	const int nc = c->n_cigar;
	const u32 *o = nc <= 6 ? c->cigar : I.ops + ((u64)c->cigar[1] << 32 | c->cigar[0]);
	const int lo = (R.flags & BWAGPU_ALN_DEL5) ? 1 : 0, hi = nc - ((R.flags & BWAGPU_ALN_DEL3) ? 1 : 0);
	for (int j = lo; j < hi; ++j) { const u32 x = o[j]; sam_int(s, x >> 4); sam_ch(s, sam_op((int)(x & 0xf))); }
	if (R.clip3) { sam_int(s, R.clip3); sam_ch(s, clip); }
}

template <class S> DEVFN void sam_md(S &s, const SamIn &I, const bwagpu_cigar_t *c)
{
	const int n = c->md_len;
	if (n <= 8) { const u64 w = c->md; s.bulk(n, [&](i64 i) { return (char)(w >> (8 * i)); }); }
	else sam_bytes(s, (const char*)(I.ops + c->md), n);      // (four characters per entry, the first in the low byte)
}

// Place i of the list is listed in the XA of place k: get_pri_idx (bwamem_extra.c:104-110), an int against an int * double product
DEVFN bool sam_xa_lists(const bwagpu_opt_t &opt, const SamRead &Q, int k, int sk, int i)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
	return i < Q.n && Q.pri[i].secondary_all == k && (double)Q.alns[i].score >= sk * (double)opt.XA_drop_ratio;
}

// cnt[k] and has_alt[k] of mem_gen_alt for place k by ballots; true when the hit limits let k's XA through.  *nocig: a listed region has no CIGAR record.
DEVFN bool sam_xa_shown(const bwagpu_opt_t &opt, const SamRead &Q, int k, int lane, bool *nocig)
{
	const int sk = Q.alns[k].score;
	int cnt = 0; bool has_alt = false, noc = false;
	for (int base = 0; base < Q.n; base += SAM_STEP) {
		const int i = base + lane;
		const bool in = sam_xa_lists(opt, Q, k, sk, i);
		const int fl = in ? Q.alns[i].flags : 0;
		cnt += __popcll(__ballot(in));
		has_alt |= __ballot(fl & BWAGPU_ALN_ALT) != 0;
		noc |= __ballot(fl & BWAGPU_ALN_NOCIGAR) != 0;
	}
	*nocig = noc;
	return cnt > 0 && !(cnt > opt.max_XA_hits_alt || (!has_alt && cnt > opt.max_XA_hits));
}

// the read is left to the caller: a printed region, or one listed in a printed XA, has no CIGAR record
DEVFN bool sam_declined(const bwagpu_opt_t &opt, const SamRead &Q, int lane)
{
	bool bad = false;
	for (int base = 0; base < Q.n && !bad; base += SAM_STEP) {
		const int i = base + lane;
		const bool printed = i < Q.n && Q.alns[i].sel >= 0;
		if (__ballot(printed && (Q.alns[i].flags & BWAGPU_ALN_NOCIGAR))) bad = true;
		if (opt.flag & 0x8 /* MEM_F_ALL */) continue;
		for (unsigned long long m = __ballot(printed); m && !bad; m &= m - 1) {
			bool noc;
			if (sam_xa_shown(opt, Q, base + __ffsll(m) - 1, lane, &noc) && noc) bad = true;
		}
	}
	return bad;
}

// The mate as mem_aln2sam's last argument: SamNoMate is m == NULL -- a type, so that the single-end kernels carry nothing of what a mate adds
struct SamNoMate { static constexpr bool present = false; };
struct SamMate {
	static constexpr bool present = true;
	const bwagpu_aln_t *a;        // the mate's record, or (null) mem_reg2aln(.., NULL): no coordinate
	const bwagpu_cigar_t *c;      // its region's CIGAR record
	int mapq;                     // what MQ prints
	int rlen;                     // get_rlen of the mate's final CIGAR
	int flag;                     // 0x40 << end | the pair's extra_flag
};

// get_rlen (bwamem.c:827-836) of record R's final CIGAR: the M and D operations without a dropped deletion (the clips count nothing)
DEVFN int sam_rlen(const SamIn &I, const bwagpu_aln_t &R, const bwagpu_cigar_t *c)
{
	const int nc = c->n_cigar;
	const u32 *o = nc <= 6 ? c->cigar : I.ops + ((u64)c->cigar[1] << 32 | c->cigar[0]);
	const int lo = (R.flags & BWAGPU_ALN_DEL5) ? 1 : 0, hi = nc - ((R.flags & BWAGPU_ALN_DEL3) ? 1 : 0);
	int l = 0;
	for (int j = lo; j < hi; ++j) { const u32 x = o[j]; if ((x & 0xf) == 0 || (x & 0xf) == 2) l += (int)(x >> 4); }
	return l;
}

// One line: place k of the marked list as line `which` of the read, or (k < 0) the unmapped record of mem_reg2aln(.., NULL); mate: mem_aln2sam's m
template <class S, class M> DEVFN void sam_line(S &s, const bwagpu_opt_t &opt, const SamIn &I, const SamRead &Q, int k, int which, int lane, const M &mate)
{
	bwagpu_aln_t R;
	R.pos = -1; R.rid = -1; R.flag = 0x4; R.mapq = 0; R.mapq_out = 0; R.nm = 0; R.n_cigar = 0; R.score = 0; R.sub = 0; R.alt_sc = 0; R.sel = 0; R.clip5 = 0; R.clip3 = 0; R.flags = 0; R.pad_ = 0;
	const bwagpu_cigar_t *c = nullptr;
	if (k >= 0) { R = Q.alns[k]; c = Q.cigs + Q.pri[k].src; }
	bool rev = (R.flags & BWAGPU_ALN_REV) != 0;
	const bool alt = (R.flags & BWAGPU_ALN_ALT) != 0;
	const bool has_cigar = R.rid >= 0 && R.n_cigar > 0;
	const bool hard = which && !(opt.flag & 0x200 /* MEM_F_SOFTCLIP */) && !alt;
	int flag = R.flag | I.extra_flag | (R.rid < 0 ? 0x4 : 0);
	i64 mpos = -1; int mrid = -1; bool mrev = false, mcig = false;      // the mate's columns (:858-866)
	if constexpr (M::present) {
		flag |= 0x1 | mate.flag;
		if (mate.a && mate.a->rid >= 0) { mrid = mate.a->rid; mpos = mate.a->pos; mrev = (mate.a->flags & BWAGPU_ALN_REV) != 0; mcig = mate.a->n_cigar > 0; }
		if (mrid < 0) flag |= 0x8;
		if (R.rid < 0 && mrid >= 0) { R.rid = mrid; R.pos = mpos; rev = mrev; }      // copy mate to alignment: n_cigar = 0, which has_cigar says already
		else if (mrid < 0 && R.rid >= 0) { mrid = R.rid; mpos = R.pos; mrev = rev; }      // copy alignment to mate: n_cigar = 0, as mcig says already
		if (mrev) flag |= 0x20;
	}
	if (rev) flag |= 0x10;
	sam_bytes(s, Q.name, Q.l_name); sam_ch(s, '\t');
	sam_int(s, (flag & 0xffff) | (flag & 0x10000 ? 0x100 : 0)); sam_ch(s, '\t');
	if (R.rid >= 0) {
		sam_ctg_name(s, I, R.rid); sam_ch(s, '\t');
		sam_int(s, R.pos + 1); sam_ch(s, '\t');
		sam_int(s, R.mapq_out); sam_ch(s, '\t');
		if (has_cigar) sam_cigar(s, I, R, c, hard ? 'H' : 'S'); else sam_ch(s, '*');
	} else sam_lit(s, "*\t0\t0\t*");
	if constexpr (M::present) {
		sam_ch(s, '\t');
		if (mrid >= 0) {      // :882-893
			if (R.rid == mrid) sam_ch(s, '='); else sam_ctg_name(s, I, mrid);
			sam_ch(s, '\t'); sam_int(s, mpos + 1); sam_ch(s, '\t');
			if (R.rid == mrid && has_cigar && mcig) {
				const i64 p0 = R.pos + (rev ? sam_rlen(I, R, c) - 1 : 0), p1 = mpos + (mrev ? mate.rlen - 1 : 0);
				sam_int(s, -(p0 - p1 + (p0 > p1 ? 1 : p0 < p1 ? -1 : 0)));
			} else sam_ch(s, '0');
		} else sam_lit(s, "*\t0\t0");
		sam_ch(s, '\t');
	} else sam_lit(s, "\t*\t0\t0\t");
	if (flag & 0x100) sam_lit(s, "*\t*");
	else {
		int qb = 0, qe = Q.l_seq;
		if (has_cigar && hard) { if (rev) { qe -= R.clip5; qb += R.clip3; } else { qb += R.clip5; qe -= R.clip3; } }
		const int len = qe > qb ? qe - qb : 0;
		if (rev) { const u8 *q = Q.seq + qe - 1; s.bulk(len, [&](i64 i) { return sam_base(*(q - i), SAM_REV); }); }
		else { const u8 *q = Q.seq + qb; s.bulk(len, [&](i64 i) { return sam_base(q[i], SAM_FWD); }); }
		sam_ch(s, '\t');
		if (!Q.qual) sam_ch(s, '*');
		else if (rev) { const char *q = Q.qual + qe - 1; s.bulk(len, [&](i64 i) { return *(q - i); }); }
		else sam_bytes(s, Q.qual + qb, len);
	}
	if (has_cigar) { sam_lit(s, "\tNM:i:"); sam_int(s, R.nm); sam_lit(s, "\tMD:Z:"); sam_md(s, I, c); }
	if constexpr (M::present) {
		if (mcig) {      // add_cigar(opt, m, str, which): this line's `which`, the mate's ALT bit
			sam_lit(s, "\tMC:Z:");
			sam_cigar(s, I, *mate.a, mate.c, which && !(opt.flag & 0x200 /* MEM_F_SOFTCLIP */) && !(mate.a->flags & BWAGPU_ALN_ALT) ? 'H' : 'S');
		}
		sam_lit(s, "\tMQ:i:"); sam_int(s, mate.mapq);
	}
	if (R.score >= 0) { sam_lit(s, "\tAS:i:"); sam_int(s, R.score); }
	if (R.sub >= 0) { sam_lit(s, "\tXS:i:"); sam_int(s, R.sub); }
	if (I.rg_len) { sam_lit(s, "\tRG:Z:"); sam_bytes(s, I.rg, I.rg_len); }
	if (!(flag & 0x100)) {
		bool first = true;
		for (int base = 0; base < Q.n; base += SAM_STEP) {      // the other printed records that are not secondary, in the list's order
			const int i = base + lane;
			const bool in = i < Q.n && i != k && Q.alns[i].sel >= 0 && !(Q.alns[i].flag & 0x100);
			for (unsigned long long m = __ballot(in); m; m &= m - 1) {
				const int j = base + __ffsll(m) - 1;
				const bwagpu_aln_t T = Q.alns[j];
				if (first) { sam_lit(s, "\tSA:Z:"); first = false; }
				sam_ctg_name(s, I, T.rid); sam_ch(s, ','); sam_int(s, T.pos + 1); sam_ch(s, ','); sam_ch(s, (T.flags & BWAGPU_ALN_REV) ? '-' : '+'); sam_ch(s, ',');
				if (T.rid >= 0) sam_cigar(s, I, T, Q.cigs + Q.pri[j].src, 'S');
				sam_ch(s, ','); sam_int(s, T.mapq_out); sam_ch(s, ','); sam_int(s, T.nm); sam_ch(s, ';');
			}
		}
		if (R.alt_sc > 0) sam_pa(s, R.score, R.alt_sc);
	}
	bool noc;
	if (k >= 0 && !(opt.flag & 0x8 /* MEM_F_ALL */) && sam_xa_shown(opt, Q, k, lane, &noc)) {
		const bool xb = (opt.flag & 0x2000 /* MEM_F_XB */) != 0;
		if (xb) sam_lit(s, "\tXB:Z:"); else sam_lit(s, "\tXA:Z:");
		for (int base = 0; base < Q.n; base += SAM_STEP) {
			for (unsigned long long m = __ballot(sam_xa_lists(opt, Q, k, R.score, base + lane)); m; m &= m - 1) {
				const int j = base + __ffsll(m) - 1;
				const bwagpu_aln_t T = Q.alns[j];
				sam_ctg_name(s, I, T.rid); sam_ch(s, ','); sam_ch(s, (T.flags & BWAGPU_ALN_REV) ? '-' : '+'); sam_int(s, T.pos + 1); sam_ch(s, ',');
				if (T.rid >= 0) sam_cigar(s, I, T, Q.cigs + Q.pri[j].src, 'S');
				sam_ch(s, ','); sam_int(s, T.nm);
				if (xb) { sam_ch(s, ','); sam_int(s, T.score); sam_ch(s, ','); sam_int(s, T.mapq); }
				sam_ch(s, ';');
			}
		}
	}
	if (Q.l_comment > 0) { sam_ch(s, '\t'); sam_bytes(s, Q.comment, Q.l_comment); }
	if ((opt.flag & 0x100 /* MEM_F_REF_HDR */) && R.rid >= 0 && I.ctg_anno_off) {
		const i64 b = I.ctg_anno_off[R.rid], n = I.ctg_anno_off[R.rid + 1] - b;
		if (n > 0) {
			sam_lit(s, "\tXR:Z:");
			const char *p = I.ctg_text + b;
			s.bulk(n, [&](i64 i) { const char ch = p[i]; return ch == '\t' ? ' ' : ch; });
		}
	}
	sam_ch(s, '\n');
}

// all lines of a read (mem_reg2sam's second loop); returns their number
template <class S, class M> DEVFN int sam_read(S &s, const bwagpu_opt_t &opt, const SamIn &I, const SamRead &Q, int lane, const M &mate)
{
	int which = 0;
	for (int base = 0; base < Q.n || which == 0; base += SAM_STEP) {
		const int i = base + lane;
		unsigned long long m = __ballot(i < Q.n && Q.alns[i].sel >= 0);
		const bool none = base + SAM_STEP >= Q.n && which == 0 && m == 0;      // the list is through and nothing was printed: the unmapped record (one call site for both)
		if (none) m = 1;
		for (; m; m &= m - 1) sam_line(s, opt, I, Q, none ? -1 : base + __ffsll(m) - 1, which++, lane, mate);
	}
	return which;
}

DEVFN SamRead sam_view(const SamIn &I, const i32 *cnt, const i64 *off, int r)
{
	SamRead Q;
	Q.n = cnt[r];
	const i64 o = Q.n > 0 ? off[r] : 0;
	Q.alns = I.alns + o; Q.pri = I.pri + o; Q.cigs = I.cigs + o;
	const i64 sb = I.seq_off[r], nb = I.name_off[r];
	Q.seq = I.seq + sb; Q.l_seq = (int)(I.seq_off[r + 1] - sb); Q.qual = I.quals ? I.quals + sb : nullptr;
	Q.name = I.names + nb; Q.l_name = (int)(I.name_off[r + 1] - nb);
	Q.comment = nullptr; Q.l_comment = 0;
	if (I.comments) { const i64 cb = I.comment_off[r]; Q.comment = I.comments + cb; Q.l_comment = (int)(I.comment_off[r + 1] - cb); }
	return Q;
}

// pass 1: bytes, lines and the declined bit of every read (one wavefront, a workgroup of 64, per read)
__global__ void __launch_bounds__(64) k_sam_size(bwagpu_opt_t opt, int n_reads, const i32 *cnt, const i64 *off, SamIn I, i32 *size, i32 *flags, i32 *n_lines)
{
	const int lane = threadIdx.x & 63;
	for (int r = blockIdx.x; r < n_reads; r += gridDim.x) {
		const SamRead Q = sam_view(I, cnt, off, r);
		SamCount s; s.n = 0;
		int lines = 0;
		const bool declined = sam_declined(opt, Q, lane);
		if (!declined) lines = sam_read(s, opt, I, Q, lane, SamNoMate());
		if (lane == 0) { size[r] = (i32)s.n; flags[r] = declined ? 1 : 0; n_lines[r] = lines; }
	}
}

// pass 2: read r's lines at text + toff[r]
__global__ void __launch_bounds__(64) k_sam_write(bwagpu_opt_t opt, int n_reads, const i32 *cnt, const i64 *off, SamIn I, const i64 *toff, const i32 *flags, char *text)
{
	__shared__ char stage[SAM_STAGE];
	const int lane = threadIdx.x & 63;
	for (int r = blockIdx.x; r < n_reads; r += gridDim.x) {
		if (flags[r] & 1) continue;
		const SamRead Q = sam_view(I, cnt, off, r);
		SamWrite s; s.out = text + toff[r]; s.stage = stage; s.fill = 0; s.lane = lane;
		sam_read(s, opt, I, Q, lane, SamNoMate());
		s.flush();
	}
}
