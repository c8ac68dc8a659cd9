// dev_alns.h -- the alignment list of a read on the device: what mem_reg2aln (bwamem.c:1119-1189) returns for every region of the marked list and what the
// loop of mem_reg2sam (bwamem.c:1045-1062) makes of those results.  bwagpu_batch_alns / bwagpu_alns_flat (bwagpu.hip).
//
// Everything is read from what earlier stages left in HBM: the regions, the marking records (dev_primary.h: place k of the marked list is region `src` of the
// read's k-th record, as in dev_pair.h), the CIGAR records with their operation array (dev_cigar.h) and the contig table.  The CIGAR is not recomputed; of its
// operations only the first and the last are looked at (the leading / trailing deletion rule).
//
// One routine per region, aln_region, and one per read, aln_read<W>, in two forms chosen by the read's number of regions (bwagpu_alns_limits):
//   W = 1   one lane per read, up to ALN_LANE_MAX regions (k_alns_lane);
//   W = 64  one wavefront per read, ALN_STEP regions a step: the place in `aa` is a prefix count of the keep ballot carried across the steps, and the mapQ of
//           aa[0] is broadcast from the first kept lane (k_alns_wave).
// No LDS, no HBM scratch: the loop's only state is the number of records kept so far and aa[0]'s mapQ.
#pragma once
#include <limits.h>
#include "dev_common.h"
#include "dev_fm.h"

#define ALN_LANE_MAX 4          // regions up to which one lane makes a read's list (the marking kernel's value: the reads of k_primary_lane stay lane work)
#define ALN_STEP 64             // regions per step of the wavefront form (one per lane)
#define ALN_LANE_BLOCK 128      // lanes per workgroup of k_alns_lane

static_assert(sizeof(bwagpu_aln_t) == 64, "layout");

// what the kernels need besides the lists
struct AlnIn {
	const bwagpu_primary_t *pri;     // marking records, by the lists' offsets
	const bwagpu_cigar_t *cigs;      // CIGAR records, likewise (by input index of the region)
	const u32 *ops; i64 n_ops;       // operation array
	const i64 *seq_off;              // read r has seq_off[r + 1] - seq_off[r] bases, or (null)
	const i32 *read_len;             // ... read_len[r]
};

// mem_reg2aln of region `a` marked as `p`, with the CIGAR record c; the fields of mem_reg2sam's loop (sel, mapq_out) are left to aln_read
DEVFN bwagpu_aln_t aln_region(const DevIndex &ix, const bwagpu_alnreg_t &a, const bwagpu_primary_t &p, const bwagpu_cigar_t &c, const u32 *ops, i64 n_ops, int l_query)
{
	bwagpu_aln_t r;
	r.pos = -1; r.rid = -1; r.flag = 0; r.mapq = 0; r.mapq_out = 0; r.nm = 0; r.n_cigar = 0; r.score = 0; r.sub = 0; r.alt_sc = 0; r.sel = -1; r.clip5 = 0; r.clip3 = 0; r.flags = 0; r.pad_ = 0;
	const i64 rb = a.rb, re = a.re;
	if (rb < 0 || re < 0) { r.flag = 0x4; return r; }
	const int qb = a.qb, qe = a.qe;
	r.mapq = p.secondary < 0 ? p.mapq : 0;
	if (p.secondary >= 0) r.flag |= 0x100;
	int is_rev;
	i64 pos = dev_depos(ix, rb < ix.l_pac ? rb : re - 1, &is_rev);
	int n = c.n_cigar;
	r.nm = c.nm;
	if (n > 0) {   // squeeze out a leading or trailing deletion
		u32 first = c.cigar[0], last = c.cigar[n <= 6 ? n - 1 : 0];
		if (n > 6) {
			const u64 at = (u64)c.cigar[1] << 32 | c.cigar[0];
			if (at > (u64)n_ops || (u64)n > (u64)n_ops - at) n = -1;      // (a reference outside the operation array: left to the caller)
			else { first = ops[at]; last = ops[at + (u64)n - 1]; }
		}
		if (n > 0) {
			if ((first & 0xf) == 2) { pos += first >> 4; --n; r.flags |= BWAGPU_ALN_DEL5; }
			else if ((last & 0xf) == 2) { --n; r.flags |= BWAGPU_ALN_DEL3; }
		}
	}
	r.clip5 = is_rev ? l_query - qe : qb; r.clip3 = is_rev ? qb : l_query - qe;
	if (n < 0) { r.flags |= BWAGPU_ALN_NOCIGAR; r.n_cigar = -1; r.nm = -1; }
	else r.n_cigar = n + (r.clip5 != 0) + (r.clip3 != 0);
	r.rid = dev_pos2rid(ix, pos);
	r.pos = r.rid >= 0 ? pos - ix.ctg_off[r.rid] : pos;
	r.score = a.score; r.sub = p.sub > a.csub ? p.sub : a.csub;
	r.alt_sc = p.alt_sc;
	if (is_rev) r.flags |= BWAGPU_ALN_REV;
	if (a.is_alt) r.flags |= BWAGPU_ALN_ALT;
	return r;
}

// the three tests of mem_reg2sam's loop (bwamem.c:1048-1050) for place k of a read's marked list; the last one compares an int with an int * float product
DEVFN bool aln_keep(const bwagpu_opt_t &opt, const bwagpu_alnreg_t *a, const bwagpu_primary_t *pri, int n, const bwagpu_alnreg_t &p, const bwagpu_primary_t &m)
{
	if (p.score < opt.T) return false;
	if (m.secondary >= 0 && (p.is_alt || !(opt.flag & 0x8 /* MEM_F_ALL */))) return false;
	if (m.secondary >= 0 && m.secondary < INT_MAX && m.secondary < n) {
		const int s = pri[m.secondary].src;
		if (s >= 0 && s < n && (float)p.score < (float)a[s].score * opt.drop_ratio) return false;
	}
	return true;
}

// One read: regions a[0 .. n), marking records pri[0 .. n), CIGAR records c[0 .. n) (by input index); records to out[0 .. n) in marked order.  Returns aa.n.
template <int W>
DEVFN int aln_read(const DevIndex &ix, const bwagpu_opt_t &opt, const bwagpu_alnreg_t *a, const bwagpu_primary_t *pri, const bwagpu_cigar_t *c, const u32 *ops, i64 n_ops,
				   int l_query, int n, bwagpu_aln_t *out, int lane)
{
	int l = 0, mapq0 = 0;
	for (int base = 0; base < n; base += W) {
		const int k = base + lane;
		bool keep = false;
		bwagpu_aln_t r = {};
		bool sec = false, alt = false;
		if (k < n) {
			const bwagpu_primary_t m = pri[k];
			const int src = m.src >= 0 && m.src < n ? m.src : 0;
			const bwagpu_alnreg_t &p = a[src];
			r = aln_region(ix, p, m, c[src], ops, n_ops, l_query);
			keep = aln_keep(opt, a, pri, n, p, m);
			sec = m.secondary >= 0; alt = p.is_alt != 0;
		}
		int sel = l;
		if (W > 1) {
			const unsigned long long kept = __ballot(keep);
			if (l == 0 && kept) mapq0 = __shfl(r.mapq, __ffsll(kept) - 1);
			sel += __popcll(kept & ((1ull << lane) - 1));
			l += __popcll(kept);
		} else if (keep) { if (l == 0) mapq0 = r.mapq; ++l; }
		if (k < n) {
			r.mapq_out = r.mapq;
			if (keep) {
				r.sel = sel;
				if (sec) r.sub = -1;
				if (sel && !sec) r.flag |= (opt.flag & 0x10 /* MEM_F_NO_MULTI */) ? 0x10000 : 0x800;
				if (!(opt.flag & 0x1000 /* MEM_F_KEEP_SUPP_MAPQ */) && sel && !alt && r.mapq > mapq0) r.mapq_out = mapq0;
			}
			out[k] = r;
		}
	}
	return l;
}

DEVFN int aln_len(const AlnIn &I, int r) { return I.seq_off ? (int)(I.seq_off[r + 1] - I.seq_off[r]) : I.read_len[r]; }

// One lane per read; reads with more than ALN_LANE_MAX regions go to `list` for the wavefront form (tier_push)
__global__ void __launch_bounds__(ALN_LANE_BLOCK) k_alns_lane(DevIndex ix, bwagpu_opt_t opt, int n_reads, const i32 *cnt, const i64 *off, const bwagpu_alnreg_t *regs, AlnIn I,
															   bwagpu_aln_t *out, i32 *n_aln, i32 *list, unsigned int *list_n)
{
	const int lane = threadIdx.x & 63;
	for (i64 r0 = (i64)blockIdx.x * blockDim.x; r0 < n_reads; r0 += (i64)gridDim.x * blockDim.x) {
		const int r = (int)(r0 + threadIdx.x);
		const int n = r < n_reads ? cnt[r] : 0;
		tier_push<1>(n > ALN_LANE_MAX ? 0 : -1, r, n_reads, list, list_n, lane);
		if (r < n_reads && n <= 0) n_aln[r] = 0;
		if (n >= 1 && n <= ALN_LANE_MAX) { const i64 o = off[r]; n_aln[r] = aln_read<1>(ix, opt, regs + o, I.pri + o, I.cigs + o, I.ops, I.n_ops, aln_len(I, r), n, out + o, 0); }
	}
}

// One wavefront (a workgroup of 64) per read of `list`
__global__ void __launch_bounds__(64) k_alns_wave(DevIndex ix, bwagpu_opt_t opt, const i32 *cnt, const i64 *off, const bwagpu_alnreg_t *regs, AlnIn I,
												   bwagpu_aln_t *out, i32 *n_aln, const i32 *list, const unsigned int *list_n)
{
	const int lane = threadIdx.x & 63;
	const int nl = (int)*list_n;
	for (int t = blockIdx.x; t < nl; t += gridDim.x) {
		const int r = list[t], n = cnt[r];
		const i64 o = off[r];
		const int l = aln_read<64>(ix, opt, regs + o, I.pri + o, I.cigs + o, I.ops, I.n_ops, aln_len(I, r), n, out + o, lane);
		if (lane == 0) n_aln[r] = l;
	}
}
