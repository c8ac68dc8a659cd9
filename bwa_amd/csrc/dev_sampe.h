// dev_sampe.h -- a read pair decided on the device: what mem_sam_pe (bwamem_pair.c:276-419) does between mem_pair and the text.  bwagpu_batch_sampe /
// bwagpu_sampe_flat (bwagpu.hip).
//
// Everything is read from what the earlier stages left in HBM: the merged lists of the mate rescue (dev_rescue.h), their marking records (dev_primary.h: place
// k of a marked list is region `src` of the read's k-th record), the pair records (dev_pair.h).  One record per pair, bwagpu_sampe_t, says which way out the
// pair takes -- :311-394 or no_pairing, :397-418 -- and what it prints; the marking records are patched in place as the reference patches its lists:
//   * :335-336: the chosen hit, when it is a secondary, gets the score of its primary as `sub` and secondary = -2; its mapq is recomputed from the new sub;
//   * :350-359: where the chosen hit belongs to the secondary_all group of a primary-assembly hit k, the group is handed to the chosen hit.
// What makes it exact:
//   * raw_mapq (:274) is (int)(6.02 * diff / a + .499) in double, contraction off: the truncation is of a possibly negative value, before the clamp of :327-328;
//   * log(n_sub + 1) (:326) comes from the handle's table of the host's log() values, as the marking's logarithms do (PriLogTab).  An argument outside the table
//     leaves the pair's lists untouched and flags the record (bit 1): the host side of the call runs sampe_path0 again with libm (sampe_host_pair0);
//   * frac_rep is added in float and halved in double (:329); q_se goes through pri_mapq with the patched sub (:337), or is the marking record's mapq of place 0
//     (:347-348: mem_approx_mapq_se of an untouched region is what the marking computed);
//   * h[i].rid of no_pairing (:405-408) is bns_pos2rid of the region's forward position, as aln_region takes it.  A leading deletion moves pos inside the region,
//     and a region lies on one contig, so the rid needs no CIGAR.
//
// Two forms, chosen by the longer of the pair's two lists (bwagpu_sampe_limits; the marking kernel's switch point, so lane work there is lane work here):
//   W = 1   one lane per pair (k_sampe_lane);
//   W = 64  one wavefront per pair (k_sampe_wave): the is_multi scan (:315-319) and the secondary_all rewrite (:354-356), the only loops over a list, take 64
//           places a step -- a ballot, then a store under the lanes' mask.  Everything else is computed by every lane alike and written by lane 0.
// No LDS, no HBM scratch.
#pragma once
#include <limits.h>
#include "dev_common.h"
#include "dev_fm.h"
#include "dev_primary.h"
#include "dev_pair.h"
#include "dev_matesw.h"
#include "dev_alns.h"

#define SAMPE_LANE_MAX PRI_LANE_MAX   // regions of the longer list up to which one lane decides a pair
#define SAMPE_STEP 64                 // places per step of the wavefront form
#define SAMPE_LANE_BLOCK 128          // lanes per workgroup of k_sampe_lane

static_assert(sizeof(bwagpu_sampe_t) == 64, "layout");

// the four windows as mem_sam_pe's proper-pair test reads them (:412)
struct SampeWin { i32 low[4], high[4], failed[4]; };

// what the kernels read besides the options: the merged lists, their marking records (patched in place), n_pri, the pair and rescue records
struct SampeIn {
	const i32 *cnt; const i64 *off; const bwagpu_alnreg_t *regs;
	bwagpu_primary_t *pri; const i32 *npri;
	const bwagpu_pair_t *pairs; const bwagpu_rescue_t *resc;
};

// :274
__host__ __device__ inline int sampe_raw_mapq(int diff, int a)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
	return (int)(6.02 * diff / a + .499);
}

// what :335-359 change in one end's list: the chosen place z; sub and mapq of its record where `fired` (:335-336); grp: the primary whose secondary_all group
// goes to z (:351-352), or -1
struct SampeEnd { int z, fired, sub, mapq, grp; };

// One end of a pair that :311 accepted: q_se (:337-348), the patch of its list, g[i]'s place (:371-373).  a / p: the end's regions and marking records, n / np
// its list length and n_pri.
template <class LG>
__host__ __device__ inline void sampe_end0(const bwagpu_opt_t &opt, const bwagpu_alnreg_t *a, const bwagpu_primary_t *p, int n, int np, int z, bool paired, int q_pe, const LG &lg,
										   int &miss, SampeEnd &E, int &q_se, int &alt)
{
	const bwagpu_primary_t m = p[z];
	const int src = m.src >= 0 && m.src < n ? m.src : 0;
	const bwagpu_alnreg_t &c = a[src];
	E.z = z; E.fired = 0; E.sub = m.sub; E.mapq = m.mapq;
	int q = m.mapq;
	if (paired) {
		if (m.secondary >= 0 && m.secondary < n) {      // :335-336
			const int ps = p[m.secondary].src;
			E.sub = a[ps >= 0 && ps < n ? ps : 0].score; E.fired = 1;
			E.mapq = q = pri_mapq(opt, c, E.sub, m.sub_n, lg, miss);
		}
		q = q > q_pe ? q : q_pe < q + 40 ? q_pe : q + 40;      // :339-340
		const int cap = sampe_raw_mapq(c.score - c.csub, opt.a);      // :343-344
		q = q < cap ? q : cap;
	}
	q_se = q;
	const int k = m.secondary_all;
	E.grp = k >= 0 && k < np ? k : -1;
	alt = -1;
	if (np < n) {      // :371-373
		const bwagpu_primary_t g = p[np];
		const int gs = g.src >= 0 && g.src < n ? g.src : 0;
		if (!(a[gs].score < opt.T || g.secondary >= 0 || !a[gs].is_alt)) alt = np;
	}
}

// :322-349 and :365-378 of a pair that :311 and :320 accepted (n_pri of both ends positive, mem_pair's score positive, no end with several hits): fills s, and
// E0 / E1 with what is to be written into the lists.  Reads the lists, writes nothing.  Returns `miss`: a logarithm outside lg's table -- s is then not final.
template <class LG>
__host__ __device__ inline int sampe_path0(const bwagpu_opt_t &opt, const bwagpu_alnreg_t *a0, const bwagpu_primary_t *p0, int n0, int np0, const bwagpu_alnreg_t *a1, const bwagpu_primary_t *p1,
										   int n1, int np1, const bwagpu_pair_t &pr, const LG &lg, bwagpu_sampe_t &s, SampeEnd &E0, SampeEnd &E1)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
	int miss = 0;
	const int s0 = p0[0].src, s1 = p1[0].src;
	const bwagpu_alnreg_t &b0 = a0[s0 >= 0 && s0 < n0 ? s0 : 0], &b1 = a1[s1 >= 0 && s1 < n1 ? s1 : 0];
	const int o = pr.score, score_un = b0.score + b1.score - opt.pen_unpaired;
	const int subo = pr.sub > score_un ? pr.sub : score_un;
	int q_pe = sampe_raw_mapq(o - subo, opt.a);
	if (pr.n_sub > 0) q_pe -= (int)(4.343 * lg(pr.n_sub + 1, miss) + .499);
	if (q_pe < 0) q_pe = 0;
	if (q_pe > 60) q_pe = 60;
	q_pe = (int)(q_pe * (1. - .5 * (b0.frac_rep + b1.frac_rep)) + .499);
	const bool paired = o > score_un;
	const int z0 = paired && pr.z[0] >= 0 && pr.z[0] < np0 ? pr.z[0] : 0, z1 = paired && pr.z[1] >= 0 && pr.z[1] < np1 ? pr.z[1] : 0;
	s.path = 0; s.why = 0; s.extra_flag = paired ? 3 : 1; s.q_pe = q_pe; s.paired = paired ? 1 : 0;
	sampe_end0(opt, a0, p0, n0, np0, z0, paired, q_pe, lg, miss, E0, s.q_se[0], s.alt[0]);
	sampe_end0(opt, a1, p1, n1, np1, z1, paired, q_pe, lg, miss, E1, s.q_se[1], s.alt[1]);
	s.z[0] = z0; s.z[1] = z1;
	s.n_aa[0] = 1 + (s.alt[0] >= 0); s.n_aa[1] = 1 + (s.alt[1] >= 0);
	return miss;
}

// :335-336 written into the end's list
__host__ __device__ inline void sampe_patch(bwagpu_primary_t *p, const SampeEnd &E)
{
	if (E.fired) { p[E.z].sub = E.sub; p[E.z].secondary = -2; p[E.z].mapq = E.mapq; }
}
// :354-357 for place j of the list
__host__ __device__ inline void sampe_switch(bwagpu_primary_t *p, const SampeEnd &E, int j)
{
	if (p[j].secondary_all == E.grp || j == E.grp) p[j].secondary_all = j == E.z ? -1 : E.z;
}

// The host side of the call for a pair whose record came back with a logarithm missing: the same statements with the host's log()
static inline void sampe_host_pair0(const bwagpu_opt_t &opt, const bwagpu_alnreg_t *a0, bwagpu_primary_t *p0, int n0, int np0, const bwagpu_alnreg_t *a1, bwagpu_primary_t *p1, int n1, int np1,
									const bwagpu_pair_t &pr, bwagpu_sampe_t &s)
{
	SampeEnd E0, E1;
	const int keep = s.flags;
	(void)sampe_path0(opt, a0, p0, n0, np0, a1, p1, n1, np1, pr, PriLogLibm(), s, E0, E1);
	s.flags = keep | 2;
	sampe_patch(p0, E0); sampe_patch(p1, E1);
	if (E0.grp >= 0) for (int j = 0; j < n0; ++j) sampe_switch(p0, E0, j);
	if (E1.grp >= 0) for (int j = 0; j < n1; ++j) sampe_switch(p1, E1, j);
}

// :315-319 for one end: a hit behind the first that is no secondary and reaches T
template <int W>
DEVFN bool sampe_is_multi(const bwagpu_opt_t &opt, const bwagpu_alnreg_t *a, const bwagpu_primary_t *p, int n, int np, int lane)
{
	for (int base = 1; base < np; base += W) {
		const int j = base + lane;
		bool hit = false;
		if (j < np) { const bwagpu_primary_t m = p[j]; hit = m.secondary < 0 && a[m.src >= 0 && m.src < n ? m.src : 0].score >= opt.T; }
		if (W > 1 ? __ballot(hit) != 0 : hit) return true;
	}
	return false;
}

// :398-407 for one end: `which`, h[i].rid and h[i].mapq
DEVFN void sampe_end1(const DevIndex &ix, const bwagpu_opt_t &opt, const bwagpu_alnreg_t *a, const bwagpu_primary_t *p, int n, int np, int &which, int &rid, int &mapq)
{
	which = -1; rid = -1; mapq = 0;
	if (n > 0) {
		const int s0 = p[0].src;
		if (a[s0 >= 0 && s0 < n ? s0 : 0].score >= opt.T) which = 0;
		else if (np < n) { const int s1 = p[np].src; if (a[s1 >= 0 && s1 < n ? s1 : 0].score >= opt.T) which = np; }
	}
	if (which < 0) return;
	const bwagpu_primary_t m = p[which];
	const bwagpu_alnreg_t &c = a[m.src >= 0 && m.src < n ? m.src : 0];
	if (c.rb < 0 || c.re < 0) return;      // (mem_reg2aln's unmapped record, bwamem.c:1125-1130)
	int is_rev;
	rid = dev_pos2rid(ix, dev_depos(ix, c.rb < ix.l_pac ? c.rb : c.re - 1, &is_rev));
	mapq = m.secondary < 0 ? m.mapq : 0;
}

// One pair.  Wave-uniform control flow: every lane of a wavefront form arrives at every ballot.
template <int W>
DEVFN void sampe_pair(const DevIndex &ix, const bwagpu_opt_t &opt, const SampeWin &Wn, const PriLogTab &lg, const SampeIn &I, int pair, bwagpu_sampe_t *out, int lane)
{
	bwagpu_sampe_t s;
	s.path = 0; s.why = 0; s.extra_flag = 0; s.z[0] = s.z[1] = 0; s.q_se[0] = s.q_se[1] = 0; s.alt[0] = s.alt[1] = 0; s.n_aa[0] = s.n_aa[1] = 0; s.q_pe = 0; s.paired = 0; s.flags = 0; s.pad_[0] = s.pad_[1] = 0;
	if (I.resc && (I.resc[pair].flags & 1)) {      // the rescue kernels declined the pair: its lists are the download's, and the caller's to finish
		s.path = -1; s.flags = 1;
		if (lane == 0) out[pair] = s;
		return;
	}
	const int r0 = 2 * pair, r1 = r0 + 1;
	const int n0 = I.cnt[r0], n1 = I.cnt[r1], np0 = I.npri[r0], np1 = I.npri[r1];
	const bwagpu_alnreg_t *a0 = I.regs + I.off[r0], *a1 = I.regs + I.off[r1];
	bwagpu_primary_t *p0 = I.pri + I.off[r0], *p1 = I.pri + I.off[r1];
	const bwagpu_pair_t pr = I.pairs[pair];
	if (pr.flags & 1) s.flags |= 2;
	int why = 0;
	if (opt.flag & 0x4 /* MEM_F_NOPAIRING */) why = 1;
	else if (np0 <= 0 || np1 <= 0 || np0 > n0 || np1 > n1) why = 2;
	else if (pr.score <= 0) why = 4;
	else {
		if (sampe_is_multi<W>(opt, a0, p0, n0, np0, lane)) why |= 8;
		if (sampe_is_multi<W>(opt, a1, p1, n1, np1, lane)) why |= 16;
	}
	if (why == 0) {
		SampeEnd E0, E1;
		int miss = sampe_path0(opt, a0, p0, n0, np0, a1, p1, n1, np1, pr, lg, s, E0, E1);
		if (W > 1) miss = __ballot(miss) != 0;      // (also: every lane has read the lists before one of them writes)
		if (miss) {      // left to the host side of the call, lists untouched
			const int keep = s.flags;
			s.path = 0; s.why = 0; s.extra_flag = 0; s.z[0] = s.z[1] = 0; s.q_se[0] = s.q_se[1] = 0; s.alt[0] = s.alt[1] = 0; s.n_aa[0] = s.n_aa[1] = 0; s.q_pe = 0; s.paired = 0;
			s.flags = keep | 2;
			if (lane == 0) out[pair] = s;
			return;
		}
		if (lane == 0) { sampe_patch(p0, E0); sampe_patch(p1, E1); out[pair] = s; }
		if (E0.grp >= 0)
			for (int base = 0; base < n0; base += W) {
				const int j = base + lane;
				const bool hit = j < n0 && (p0[j].secondary_all == E0.grp || j == E0.grp);
				if (W > 1 && __ballot(hit) == 0) continue;
				if (hit) p0[j].secondary_all = j == E0.z ? -1 : E0.z;
			}
		if (E1.grp >= 0)
			for (int base = 0; base < n1; base += W) {
				const int j = base + lane;
				const bool hit = j < n1 && (p1[j].secondary_all == E1.grp || j == E1.grp);
				if (W > 1 && __ballot(hit) == 0) continue;
				if (hit) p1[j].secondary_all = j == E1.z ? -1 : E1.z;
			}
		return;
	}
	// no_pairing
	int rid0, rid1;
	s.path = 1; s.why = why; s.extra_flag = 1; s.alt[0] = s.alt[1] = -1;
	sampe_end1(ix, opt, a0, p0, n0, np0, s.z[0], rid0, s.q_se[0]);
	sampe_end1(ix, opt, a1, p1, n1, np1, s.z[1], rid1, s.q_se[1]);
	if (!(opt.flag & 0x4) && rid0 == rid1 && rid0 >= 0) {      // :408-413: the first regions of both lists (rid0 >= 0: neither list is empty)
		i64 dist;
		const int f0 = p0[0].src, f1 = p1[0].src;
		const int d = dev_infer_dir(ix.l_pac, a0[f0 >= 0 && f0 < n0 ? f0 : 0].rb, a1[f1 >= 0 && f1 < n1 ? f1 : 0].rb, &dist);
		if (!pair_pick(Wn.failed, d) && dist >= pair_pick(Wn.low, d) && dist <= pair_pick(Wn.high, d)) s.extra_flag |= 2;
	}
	if (lane == 0) out[pair] = s;
}

// One lane per pair; pairs with a list of more than SAMPE_LANE_MAX regions go to `list` for the wavefront form (tier_push)
__global__ void __launch_bounds__(SAMPE_LANE_BLOCK) k_sampe_lane(DevIndex ix, bwagpu_opt_t opt, SampeWin Wn, PriLogTab lg, SampeIn I, int n_pairs, bwagpu_sampe_t *out, i32 *list, unsigned int *list_n)
{
	const int lane = threadIdx.x & 63;
	for (i64 q0 = (i64)blockIdx.x * blockDim.x; q0 < n_pairs; q0 += (i64)gridDim.x * blockDim.x) {
		const int q = (int)(q0 + threadIdx.x);
		int big = 0;
		if (q < n_pairs) { const int n0 = I.cnt[2 * q], n1 = I.cnt[2 * q + 1]; big = n0 > n1 ? n0 : n1; }
		tier_push<1>(big > SAMPE_LANE_MAX ? 0 : -1, q, n_pairs, list, list_n, lane);
		if (q < n_pairs && big <= SAMPE_LANE_MAX) sampe_pair<1>(ix, opt, Wn, lg, I, q, out, 0);
	}
}

// One wavefront (a workgroup of 64) per pair of `list`
__global__ void __launch_bounds__(64) k_sampe_wave(DevIndex ix, bwagpu_opt_t opt, SampeWin Wn, PriLogTab lg, SampeIn I, bwagpu_sampe_t *out, const i32 *list, const unsigned int *list_n)
{
	const int lane = threadIdx.x & 63;
	const int nl = (int)*list_n;
	for (int t = blockIdx.x; t < nl; t += gridDim.x) sampe_pair<64>(ix, opt, Wn, lg, I, list[t], out, lane);
}

// ---- the alignment lists of a decided batch ----------------------------------------------------------------------------------------------------------------
// An end of a pair that :311-394 print: mem_reg2aln of every place; h[i] is place z with q_se as its mapq (:366-367), g[i] place alt with 0x800 (:374-375).
// The rules of mem_reg2sam's loop (sub = -1, the supplementary flag, the mapq cap) do not apply on this path.
template <int W>
DEVFN void aln_read_pair0(const DevIndex &ix, const bwagpu_alnreg_t *a, const bwagpu_primary_t *pri, const bwagpu_cigar_t *c, const u32 *ops, i64 n_ops, int l_query, int n, int z, int alt,
						  int q_se, bwagpu_aln_t *out, int lane)
{
	for (int base = 0; base < n; base += W) {
		const int k = base + lane;
		if (k >= n) continue;
		const bwagpu_primary_t m = pri[k];
		const int src = m.src >= 0 && m.src < n ? m.src : 0;
		bwagpu_aln_t r = aln_region(ix, a[src], m, c[src], ops, n_ops, l_query);
		r.mapq_out = r.mapq;
		if (k == z) { r.sel = 0; r.mapq_out = q_se; }
		else if (k == alt) { r.sel = 1; r.flag |= 0x800; }
		out[k] = r;
	}
}

// read r of the batch is end r & 1 of pair r >> 1
template <int W>
DEVFN int aln_read_pe(const DevIndex &ix, const bwagpu_opt_t &opt, const bwagpu_sampe_t *sampe, int r, const bwagpu_alnreg_t *a, const bwagpu_primary_t *pri, const bwagpu_cigar_t *c,
					  const u32 *ops, i64 n_ops, int l_query, int n, bwagpu_aln_t *out, int lane)
{
	const bwagpu_sampe_t &s = sampe[r >> 1];
	const int i = r & 1;
	if (s.path != 0 || (s.flags & 1)) return aln_read<W>(ix, opt, a, pri, c, ops, n_ops, l_query, n, out, lane);
	aln_read_pair0<W>(ix, a, pri, c, ops, n_ops, l_query, n, i ? s.z[1] : s.z[0], i ? s.alt[1] : s.alt[0], i ? s.q_se[1] : s.q_se[0], out, lane);
	return i ? s.n_aa[1] : s.n_aa[0];
}

// k_alns_lane / k_alns_wave for a decided batch
__global__ void __launch_bounds__(ALN_LANE_BLOCK) k_alns_pe_lane(DevIndex ix, bwagpu_opt_t opt, int n_reads, const i32 *cnt, const i64 *off, const bwagpu_alnreg_t *regs, AlnIn I,
																 const bwagpu_sampe_t *sampe, bwagpu_aln_t *out, i32 *n_aln, i32 *list, unsigned int *list_n)
{
	const int lane = threadIdx.x & 63;
	for (i64 r0 = (i64)blockIdx.x * blockDim.x; r0 < n_reads; r0 += (i64)gridDim.x * blockDim.x) {
		const int r = (int)(r0 + threadIdx.x);
		const int n = r < n_reads ? cnt[r] : 0;
		tier_push<1>(n > ALN_LANE_MAX ? 0 : -1, r, n_reads, list, list_n, lane);
		if (r < n_reads && n <= 0) n_aln[r] = 0;
		if (n >= 1 && n <= ALN_LANE_MAX) { const i64 o = off[r]; n_aln[r] = aln_read_pe<1>(ix, opt, sampe, r, regs + o, I.pri + o, I.cigs + o, I.ops, I.n_ops, aln_len(I, r), n, out + o, 0); }
	}
}

__global__ void __launch_bounds__(64) k_alns_pe_wave(DevIndex ix, bwagpu_opt_t opt, const i32 *cnt, const i64 *off, const bwagpu_alnreg_t *regs, AlnIn I, const bwagpu_sampe_t *sampe,
													  bwagpu_aln_t *out, i32 *n_aln, const i32 *list, const unsigned int *list_n)
{
	const int lane = threadIdx.x & 63;
	const int nl = (int)*list_n;
	for (int t = blockIdx.x; t < nl; t += gridDim.x) {
		const int r = list[t], n = cnt[r];
		const i64 o = off[r];
		const int l = aln_read_pe<64>(ix, opt, sampe, r, regs + o, I.pri + o, I.cigs + o, I.ops, I.n_ops, aln_len(I, r), n, out + o, lane);
		if (lane == 0) n_aln[r] = l;
	}
}

// The region-to-read map of packed lists: region g of read r for off[r] <= g < off[r] + cnt[r].  One wavefront per read.
__global__ void __launch_bounds__(256) k_sampe_reg_read(int n_reads, const i32 *cnt, const i64 *off, i32 *reg_read)
{
	const int lane = threadIdx.x & 63;
	for (i64 r = (i64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n_reads; r += (i64)gridDim.x * (blockDim.x >> 6)) {
		const int n = cnt[r];
		i32 *to = reg_read + off[r];
		for (int k = lane; k < n; k += 64) to[k] = (i32)r;
	}
}
