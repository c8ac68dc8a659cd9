// dev_rescue.h -- the decision loop and merge of mate rescue on the device: what mem_sam_pe does between the download and the marking of a pair
// (bwamem_pair.c:291-302 driving mem_matesw, :137-206).  bwagpu_batch_rescue / bwagpu_rescue_flat (bwagpu.hip).
//
// Per pair: b[i] = the first max_matesw regions of end i within pen_unpaired of its best one, taken from the lists as downloaded (a snapshot: the lists
// change below).  For i = 0, 1 and every anchor b[i][j] in order, mem_matesw against the CURRENT list of the other end: the four orientations some entry
// of that list already satisfies are skipped (:145-150); for each of the others the window (:156-166), the alignment when one is due (:167-177), the
// insertion of a hit before the first entry of strictly lower score (:178-198), and -- after every orientation that was not skipped, once the call has
// aligned anything -- mem_sort_dedup_patch without a reference (:200): introsort by end, the redundancy scan, introsort by (score, rb, qb), removal of
// identical (score, rb, qb).
//
// What makes it exact:
//   * The alignment of (mate, anchor rb, anchor contig, orientation) does not depend on the lists, so it is taken from the task results that k_matesw_tasks /
//     k_matesw_sw (dev_matesw.h) computed from the lists as downloaded: `tix` holds the task of (anchor j of a read, orientation r), or -1.  The initial lists
//     are not a superset of what the replay needs: the redundancy scan can remove an original region that a rescued hit covers, and a later anchor then
//     finds an orientation open that the enumeration saw satisfied.  That alignment is computed in place by the wavefront form (msw_align2, the same code).
//   * The two sorts are ks_introsort as dev_sort.h restates it, run on small key records {keys, index} with the regions moved once along the permutation's
//     cycles (the argument of dev_sort_regs_by_key, dev_dedup.h); `src` travels with its region.  One lane per pair sorts an index array of at most
//     RESC_LANE_MAX + 1 = 17 entries: introsort partitions the whole range once whatever its size, leaves sides of at most 16 to the final insertion sort
//     and so needs no stack there; the wavefront form keeps dev_introsort_stk's stack in LDS.  Neither form has private arrays.
//   * "No alignment was due" (other contig, window shorter than min_seed_len, empty window) is an ordinary outcome; a mate beyond MSW_MAX_Q or a window beyond
//     MSW_MAX_T flags the pair, whose lists are then returned as downloaded.  The two are told apart by msw_window, which k_matesw_sw uses too.
//
// Forms, by the larger of the two ends' capacities cnt + 4 min(|b[other]|, max_matesw) (bwagpu_rescue_limits):
//   one lane per pair, up to RESC_LANE_MAX: the index array in LDS, interleaved by lane (k_rescue_lane);
//   one wavefront per pair, up to RESC_LDS_MAX: the sorts' arrays in LDS (k_rescue_wave<RESC_LDS_MAX>); above that in an HBM scratch area per workgroup (k_rescue_wave<0>).
// In the wavefront form the skip scan, the alignment, the sorts and the redundancy scan use all lanes (dedup_read_par's routines, dev_dedupp.h); lane 0 inserts.  A lane that needs an
// alignment nobody precomputed hands its pair to the wavefront form through the lists, where it starts over from the downloaded lists.
// The merged lists live in an arena (regions and src, capacity per read as above, offsets by a prefix sum on the device) and are then packed.
#pragma once
#include "dev_matesw.h"
#include "dev_dedup.h"
#include "dev_dedupw.h"      // (dev_dedupp.h: the wave routines of dedup_read_par)

#define RESC_LANE_MAX 16        // capacity of the larger end up to which a pair is replayed by one lane
#define RESC_LDS_MAX 256        // ... by a wavefront with its sort keys in LDS (8 KB); above: keys in HBM scratch
#define RESC_LANE_BLOCK 64      // lanes per workgroup of k_rescue_lane: 17 words x 64 lanes = 4.25 KB of LDS

static_assert(sizeof(bwagpu_rescue_t) == 16 && offsetof(bwagpu_alnreg_t, frac_rep) == 76, "layout");

// 4 x the number of anchors of every read: the regions within pen_unpaired of the first, at most max_matesw of them (bwamem_pair.c:291-297); 0 with MEM_F_NO_RESCUE
__global__ void __launch_bounds__(256) k_rescue_count(bwagpu_opt_t opt, int n_reads, const i32 *cnt, const i64 *off, const bwagpu_alnreg_t *regs, i32 *x, unsigned long long *max_cap)
{
	for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n_reads / 2; p += gridDim.x * blockDim.x) {
		int nb[2];
		for (int i = 0; i < 2; ++i) {
			const int ri = 2 * p + i, n = cnt[ri];
			const bwagpu_alnreg_t *a = regs + off[ri];
			int taken = 0;
			if (!(opt.flag & 0x8 /* MEM_F_NO_RESCUE */) && n > 0) {
				const int best = a[0].score;
				for (int j = 0; j < n && taken < opt.max_matesw; ++j) if (a[j].score >= best - opt.pen_unpaired) ++taken;
			}
			if (i == 0) nb[0] = taken; else nb[1] = taken;
			x[ri] = 4 * taken;
		}
		const i64 c0 = (i64)cnt[2 * p] + 4 * nb[1], c1 = (i64)cnt[2 * p + 1] + 4 * nb[0];
		atomicMax(max_cap, (unsigned long long)(c0 > c1 ? c0 : c1));
	}
}

// out[k] = in[0] + .. + in[k - 1] for k = 0 .. n (one workgroup)
__global__ void __launch_bounds__(256) k_rescue_scan(const i32 *in, int n, i64 *out)
{
	__shared__ i64 part[256];
	const int t = (int)threadIdx.x, per = (n + 255) / 256;
	const i64 b = (i64)t * per < n ? (i64)t * per : n, e = b + per < n ? b + per : n;
	i64 s = 0;
	for (i64 k = b; k < e; ++k) s += in[k];
	part[t] = s;
	__syncthreads();
	if (t == 0) {
		i64 run = 0;
		for (int k = 0; k < 256; ++k) { const i64 v = part[k]; part[k] = run; run += v; }
		out[n] = run;
	}
	__syncthreads();
	i64 run = part[t];
	for (i64 k = b; k < e; ++k) { out[k] = run; run += in[k]; }
}

// What a pair's replay works with.  Read ri: downloaded list cnt[ri] regions at regs + off[ri]; tasks of its anchors at tix + toff[ri] (4 per anchor); its
// working list at arena + aoff(ri) with src beside it, where aoff(2p) = off[2p] + toff[2p], aoff(2p + 1) = off[2p + 1] + toff[2p] + (toff[2p + 2] - toff[2p + 1])
// (the extra room of an end is four places per anchor of the other; the sums over whole pairs agree).
struct RescIn {
	const u8 *seq; const i64 *seq_off;
	const i32 *cnt; const i64 *off; const bwagpu_alnreg_t *regs;
	const bwagpu_pes_t *pes;
	const i64 *toff; const i32 *tix; const bwagpu_matesw_t *mres; i64 n_tasks;
	bwagpu_alnreg_t *arena; i32 *asrc; i32 *acnt;
	bwagpu_rescue_t *out;
};
DEVFN i64 resc_aoff(const RescIn &R, int ri) { return (ri & 1) ? R.off[ri] + R.toff[ri - 1] + (R.toff[ri + 1] - R.toff[ri]) : R.off[ri] + R.toff[ri]; }
DEVFN int resc_cap(const RescIn &R, int ri) { return R.cnt[ri] + (int)(R.toff[(ri ^ 1) + 1] - R.toff[ri ^ 1]); }

// a region moved as its eleven 64-bit words (a struct copy with the bit-fields goes through private memory)
struct RescWords { u64 w0, w1, w2, w3, w4, w5, w6, w7, w8, w9, w10; };
static_assert(sizeof(RescWords) == sizeof(bwagpu_alnreg_t), "layout");
DEVFN RescWords resc_load(const bwagpu_alnreg_t *p) { const u64 *q = (const u64*)p; RescWords r = { q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10] }; return r; }
DEVFN void resc_store(bwagpu_alnreg_t *p, const RescWords &r) { u64 *q = (u64*)p; q[0] = r.w0; q[1] = r.w1; q[2] = r.w2; q[3] = r.w3; q[4] = r.w4; q[5] = r.w5; q[6] = r.w6; q[7] = r.w7; q[8] = r.w8; q[9] = r.w9; q[10] = r.w10; }
DEVFN void resc_copy(bwagpu_alnreg_t *to, const bwagpu_alnreg_t *from) { resc_store(to, resc_load(from)); }

// the sorts' working memory.  W = 1: an index array ord[e * st].  W = 64: dedup_read_par's arrays (dev_dedupp.h) for `cap` regions -- the decisions' operands, the
// 16-byte sort keys, the order before and after a compaction -- with the quicksort passes' stack in LDS and a staging area for the records in their final order;
// keys / ord alias them for the in-place routine that takes lists whose coordinates do not fit the 16-byte keys.
struct RescSort {
	i32 *ord; int st; RegKey *keys; SortFrame *stack;
	DdHot *hot; DdKey *dkeys; i32 *ord2; bwagpu_alnreg_t *tmp; i32 *tmp_src;
};

// Position i takes the region that was at idx(i): follow each cycle once (idx < 0: already in place), as dev_sort_regs_by_key does; src travels with its region.
template <class IDX>
DEVFN void resc_permute(bwagpu_alnreg_t *a, i32 *src, int n, IDX idx)
{
	for (int i = 0; i < n; ++i) {
		if (idx(i) < 0 || idx(i) == i) { idx(i) = -1; continue; }
		const RescWords first = resc_load(&a[i]); const i32 fs = src[i];
		int j = i;
		for (;;) {
			const int from = idx(j);
			idx(j) = -1;
			if (from == i) { resc_store(&a[j], first); src[j] = fs; break; }
			resc_copy(&a[j], &a[from]); src[j] = src[from];
			j = from;
		}
	}
}

// ks_introsort of at most 17 elements (dev_introsort, dev_sort.h, for such n: one compare for two; otherwise one partition of the whole range, whose two sides
// are then at most 16 long and left to the insertion sort) on the indices o(0 .. n) of regions that stay where they are
template <class ORD, class LT>
DEVFN void resc_introsort_small(ORD o, int n, const bwagpu_alnreg_t *a, LT lt)
{
	if (n < 2) return;
	if (n == 2) { if (lt(a[o(1)], a[o(0)])) { const i32 t = o(0); o(0) = o(1); o(1) = t; } return; }
	{
		const int t = n - 1;
		int i = 0, j = t, k = i + ((j - i) >> 1) + 1;
		if (lt(a[o(k)], a[o(i)])) { if (lt(a[o(k)], a[o(j)])) k = j; }
		else k = lt(a[o(j)], a[o(i)]) ? i : j;
		const i32 piv = o(k);
		if (k != t) { const i32 x = o(k); o(k) = o(t); o(t) = x; }
		for (;;) {
			do ++i; while (lt(a[o(i)], a[piv]));
			do --j; while (i <= j && lt(a[piv], a[o(j)]));
			if (j <= i) break;
			const i32 x = o(i); o(i) = o(j); o(j) = x;
		}
		{ const i32 x = o(i); o(i) = o(t); o(t) = x; }
	}
	for (int i = 1; i < n; ++i)
		for (int j = i; j > 0 && lt(a[o(j)], a[o(j - 1)]); --j) { const i32 t = o(j); o(j) = o(j - 1); o(j - 1) = t; }
}

// one lane's sort of a list in place.  W = 1: at most 17 regions, indices interleaved by lane.  W = 64 (lane 0, lists outside the 16-byte keys' range only): any
// number -- the introsort moves indices, its temporaries are scalars, and a comparison reads the two records' keys where they lie.
template <int W, bool BEST>
DEVFN void resc_sort(bwagpu_alnreg_t *a, i32 *src, int n, const RescSort &S)
{
	i32 *const ord = S.ord; const int st = S.st;
	auto o = [ord, st](int i) -> i32& { return ord[(size_t)i * st]; };
	for (int i = 0; i < n; ++i) o(i) = i;
	if (W == 1) {
		if (BEST) resc_introsort_small(o, n, a, RegBestLess()); else resc_introsort_small(o, n, a, RegEndLess());
	} else {
		RegKey *k = S.keys;
		for (int i = 0; i < n; ++i) { k[i].a = BEST ? a[i].rb : a[i].re; k[i].b = a[i].score; k[i].c = a[i].qb; k[i].idx = i; k[i].pad_ = 0; }
		if (BEST) dev_introsort_stk(ord, n, [k](i32 x, i32 y) { return KeyBestLess()(k[x], k[y]); }, S.stack);
		else dev_introsort_stk(ord, n, [k](i32 x, i32 y) { return KeyEndLess()(k[x], k[y]); }, S.stack);
	}
	resc_permute(a, src, n, o);
}

// mem_sort_dedup_patch(opt, 0, 0, 0, n, a) (bwamem.c:463-515; mem_patch_reg returns 0 without a reference, :436) by one lane; returns the new length
template <int W>
DEVFN int resc_sort_dedup(const bwagpu_opt_t &opt, bwagpu_alnreg_t *a, i32 *src, int n, const RescSort &S)
{
	if (n <= 1) return n;
	resc_sort<W, false>(a, src, n, S);
	for (int i = 0; i < n; ++i) a[i].n_comp = 1;
	for (int i = 1; i < n; ++i) {
		if (a[i].rid != a[i - 1].rid || a[i].rb >= a[i - 1].re + opt.max_chain_gap) continue;
		const i64 prb = a[i].rb, pre = a[i].re; const int pqb = a[i].qb, pqe = a[i].qe, prid = a[i].rid, psc = a[i].score;
		for (int j = i - 1; j >= 0 && prid == a[j].rid && prb < a[j].re + opt.max_chain_gap; --j) {
			const i64 qrb = a[j].rb, qre = a[j].re; const int qqb = a[j].qb, qqe = a[j].qe;
			if (qqe == qqb) continue;
			const i64 orr = qre - prb, oq = qqb < pqb ? qqe - pqb : pqe - qqb;
			const i64 mr = qre - qrb < pre - prb ? qre - qrb : pre - prb;
			const i64 mq = qqe - qqb < pqe - pqb ? qqe - qqb : pqe - pqb;
			if (orr > opt.mask_level_redun * mr && oq > opt.mask_level_redun * mq) {
				if (psc < a[j].score) { a[i].qe = pqb; break; }
				else a[j].qe = qqb;
			}
		}
	}
	int m = 0;
	for (int i = 0; i < n; ++i) if (a[i].qe > a[i].qb) { if (m != i) { resc_copy(&a[m], &a[i]); src[m] = src[i]; } ++m; }
	n = m;
	resc_sort<W, true>(a, src, n, S);
	for (int i = 1; i < n; ++i)
		if (a[i].score == a[i - 1].score && a[i].rb == a[i - 1].rb && a[i].qb == a[i - 1].qb) a[i].qe = a[i].qb;
	m = n > 0 ? 1 : 0;
	for (int i = 1; i < n; ++i) if (a[i].qe > a[i].qb) { if (m != i) { resc_copy(&a[m], &a[i]); src[m] = src[i]; } ++m; }
	return m;
}

// One of the two sorts by the wave (ddp_order, dev_dedupp.h, with the quicksort passes' stack in LDS): lane 0's passes of ks_introsort on the 16-byte keys, then
// the stable finish by counting.  keys[0 .. n) -> out[place] = index.  (bwagpu_debug_sort's kinds 5-8 hold these pieces to ks_introsort.)
// (records of the LDS / HBM arrays are read and written field by field: a struct copy through a pointer of unknown address space goes through private memory)
DEVFN DdHot resc_hot(const DdHot *p) { DdHot h; h.rb = p->rb; h.re = p->re; h.qb = p->qb; h.qe = p->qe; h.rid = p->rid; h.score = p->score; return h; }
DEVFN void resc_put(DdHot *p, const DdHot &h) { p->rb = h.rb; p->re = h.re; p->qb = h.qb; p->qe = h.qe; p->rid = h.rid; p->score = h.score; }
DEVFN void resc_put(DdKey *p, const DdKey &k) { p->hi = k.hi; p->lo = k.lo; }

// (The passes move indices -- idx, n free words -- and the arrangement they leave is then written out as keys, arr[x] = keys[idx[x]], for the counting: moving
// the 16-byte keys themselves puts the introsort's temporaries into private memory.  The sequence of comparisons, and so the arrangement, is the same.)
template <bool BEST>
DEVFN void resc_order(const DdKey *keys, int n, i32 *out, i32 *idx, DdKey *arr, SortFrame *stack, int lane)
{
	for (int x = lane; x < n; x += 64) idx[x] = x;
	wave_sync();
	if (lane == 0) {
		auto best = [keys](i32 x, i32 y) { return DdKeyLessBest()(keys[x], keys[y]); };
		auto end = [keys](i32 x, i32 y) { return DdKeyLessEnd()(keys[x], keys[y]); };
		if (BEST) dev_introsort_stk<i32, decltype(best), false>(idx, n, best, stack);
		else dev_introsort_stk<i32, decltype(end), false>(idx, n, end, stack);
	}
	wave_sync();
	for (int x = lane; x < n; x += 64) { const DdKey *k = &keys[idx[x]]; arr[x].hi = k->hi; arr[x].lo = k->lo; }
	wave_sync();
	ddp_rank<BEST>(arr, n, out, lane);
}

// mem_sort_dedup_patch(opt, 0, 0, 0, n, a) by the wave: dedup_read_par (dev_dedupp.h) without the patch alignment -- the decisions' operands in S.hot, the records
// where they are until the end, lanes over the regions: the redundancy scan evaluates 64 j at a time (what happens at j depends on earlier j only through p: a
// redundant q of the lower score dies, a redundant q of the higher score kills p and ends the scan), compactions and duplicate marks are prefix counts and
// neighbour compares, and the kept records and their src are gathered in their final order into the staging area and copied back.  n >= 2, wave-uniform.
// Returns the new length, or -1 with nothing changed for a list whose coordinates do not fit the sort keys.
DEVFN int resc_sort_dedup_par(const bwagpu_opt_t &opt, bwagpu_alnreg_t *ga, i32 *src, int n, const RescSort &S, int lane)
{
	DdHot *hot = S.hot; DdKey *keys = S.dkeys; i32 *ord = S.ord, *ord2 = S.ord2;
	wave_sync();
	bool odd = false;
	for (int i = lane; i < n; i += 64) {
		const bwagpu_alnreg_t &g = ga[i];
		DdHot h_; h_.rb = g.rb; h_.re = g.re; h_.qb = g.qb; h_.qe = g.qe; h_.rid = g.rid; h_.score = g.score;
		resc_put(&hot[i], h_);
		resc_put(&keys[i], ddp_key_end(h_, i));
		odd |= ddp_odd(h_) || h_.re < 0;
	}
	if (wave_ballot(odd)) { wave_sync(); return -1; }
	for (int i = lane; i < n; i += 64) ga[i].n_comp = 1;      // bwamem.c:468
	wave_sync();
	resc_order<false>(keys, n, ord, ord2, (DdKey*)S.tmp, S.stack, lane);          // by end position (bwamem.c:467)
	wave_sync();
	const float mlr = opt.mask_level_redun; const int gap = opt.max_chain_gap;
	for (int i = 1; i < n; ++i) {                              // the redundancy scan (bwamem.c:470-497)
		const int pi = uni(ord[i]);
		DdHot p = resc_hot(&hot[pi]);
		p.rb = uni64(p.rb); p.re = uni64(p.re); p.qb = uni(p.qb); p.qe = uni(p.qe); p.rid = uni(p.rid); p.score = uni(p.score);
		for (int jb = i - 1; jb >= 0; jb -= 64) {
			const int j = jb - lane; const bool valid = j >= 0;
			const int qi = valid ? ord[j] : 0;
			const DdHot q = resc_hot(&hot[qi]);
			const bool inwin = valid && q.rid == p.rid && p.rb < q.re + gap;
			const u64 out_m = wave_ballot(!inwin);
			const int nwin = out_m ? (int)__builtin_ctzll(out_m) : 64;      // the scan stops at the first region out of reach
			const bool act = lane < nwin && q.qe != q.qb;
			const i64 orr = q.re - p.rb;
			const i64 oq = q.qb < p.qb ? q.qe - p.qb : p.qe - q.qb;
			const i64 mr = q.re - q.rb < p.re - p.rb ? q.re - q.rb : p.re - p.rb;
			const i64 mq = q.qe - q.qb < p.qe - p.qb ? q.qe - q.qb : p.qe - p.qb;
			const bool red = act && orr > mlr * mr && oq > mlr * mq;
			const u64 lose_m = wave_ballot(red && p.score < q.score);
			const int first = lose_m ? (int)__builtin_ctzll(lose_m) : nwin;
			if (red && lane < first) hot[qi].qe = q.qb;                     // the redundant regions of the lower score, up to the one that ends the scan
			if (lose_m && lane == 0) hot[pi].qe = p.qb;                      // p is the redundant one
			wave_sync();
			if (lose_m || nwin < 64) break;
		}
	}
	wave_sync();
	int m = 0;                                                 // the regions left (bwamem.c:498-502), by score (bwamem.c:504)
	for (int x0 = 0; x0 < n; x0 += 64) {
		const int x = x0 + lane;
		const int id = x < n ? ord[x] : 0;
		const DdHot h_ = resc_hot(&hot[id]);
		const bool keep = x < n && h_.qe > h_.qb;
		const u64 km = wave_ballot(keep);
		if (keep) resc_put(&keys[m + __popcll(km & (((u64)1 << lane) - 1))], ddp_key_best(h_, id));
		m += __popcll(km);
	}
	wave_sync();
	resc_order<true>(keys, m, ord, ord2, (DdKey*)S.tmp, S.stack, lane);
	wave_sync();
	int nf = 0;                                                // identical hits (bwamem.c:505-513): every region that equals the one before it goes
	for (int x0 = 0; x0 < m; x0 += 64) {
		const int x = x0 + lane;
		const int id = x < m ? ord[x] : 0, idp = x > 0 && x < m ? ord[x - 1] : 0;
		const DdHot h_ = resc_hot(&hot[id]), hp = resc_hot(&hot[idp]);
		const bool keep = x < m && (x == 0 || !(h_.score == hp.score && h_.rb == hp.rb && h_.qb == hp.qb));
		const u64 km = wave_ballot(keep);
		if (keep) ord2[nf + __popcll(km & (((u64)1 << lane) - 1))] = id;
		nf += __popcll(km);
	}
	wave_sync();
	u32 *tw = (u32*)S.tmp; const u32 *gw = (const u32*)ga;
	for (int x = lane; x < nf * DDP_REG_WORDS; x += 64) {
		const int k = x / DDP_REG_WORDS, d = x - k * DDP_REG_WORDS;
		tw[x] = gw[(size_t)ord2[k] * DDP_REG_WORDS + d];
	}
	for (int k = lane; k < nf; k += 64) S.tmp_src[k] = src[ord2[k]];
	wave_sync();
	{
		u32 *ow = (u32*)ga;
		for (int x = lane; x < nf * DDP_REG_WORDS; x += 64) ow[x] = tw[x];
		for (int k = lane; k < nf; k += 64) src[k] = S.tmp_src[k];
	}
	wave_sync();
	return nf;
}

// the working lists of pair p as downloaded
template <int W>
DEVFN void resc_reset(const RescIn &R, int p, int lane)
{
	for (int i = 0; i < 2; ++i) {
		const int ri = 2 * p + i, n = R.cnt[ri];
		const i64 ao = resc_aoff(R, ri), o = R.off[ri];
		for (int k = lane; k < n; k += W) { resc_copy(&R.arena[ao + k], &R.regs[o + k]); R.asrc[ao + k] = k; }
		if (W == 1 || lane == 0) R.acnt[ri] = n;
	}
	if (W > 1) wave_sync();
}

enum { RESC_DONE = 0, RESC_HANDOVER = 1, RESC_FLAGGED = 2, RESC_OVERFLOW = 3 };

// One pair.  W = 1: a lane of its own; W = 64: a wavefront, every argument wave-uniform, `runs` the alignment's LDS area.
template <int W>
DEVFN int rescue_pair(const DevIndex &ix, const bwagpu_opt_t &opt, const RescIn &R, int p, const RescSort &S, i32 *runs, int lane)
{
	resc_reset<W>(R, p, lane);
	int n_aligned = 0, n_inline = 0;
	for (int i = 0; i < 2; ++i) {
		const int ri = 2 * p + i, rm = 2 * p + (1 - i);
		const int ni = R.cnt[ri], n_anchor = (int)(R.toff[ri + 1] - R.toff[ri]) >> 2, cap_m = resc_cap(R, rm);
		if (n_anchor == 0) continue;
		const bwagpu_alnreg_t *b = R.regs + R.off[ri];      // (the snapshot: the downloaded list itself)
		bwagpu_alnreg_t *ma = R.arena + resc_aoff(R, rm);
		i32 *msrc = R.asrc + resc_aoff(R, rm);
		const i32 *tix = R.tix + R.toff[ri];
		const u8 *ms = R.seq + R.seq_off[rm];
		const int l_ms_ = (int)(R.seq_off[rm + 1] - R.seq_off[rm]);
		const int best = b[0].score;
		int nm = R.acnt[rm], taken = 0;
		for (int j = 0; j < ni && taken < n_anchor; ++j) {
			if (b[j].score < best - opt.pen_unpaired) continue;
			const int jb = taken++;
			const i64 arb = b[j].rb; const int arid = b[j].rid, aalt = b[j].is_alt;
			int skip = 0;
			for (int r = 0; r < 4; ++r) if (R.pes[r].failed) skip |= 1 << r;
			for (int k = lane; k < nm; k += W) {
				i64 dist;
				const int r = dev_infer_dir(ix.l_pac, arb, ma[k].rb, &dist);
				if (dist >= R.pes[r].low && dist <= R.pes[r].high) skip |= 1 << r;
			}
			if (W > 1) for (int d = 32; d; d >>= 1) skip |= __shfl_xor(skip, d);
			if (skip == 15) continue;
			int n = 0;
			for (int r = 0; r < 4; ++r) {
				if (skip >> r & 1) continue;
				i64 rb, re;
				const int st = msw_window(ix, opt, R.pes, r, arb, arid, l_ms_, rb, re);
				if (st == MSW_BEYOND) return RESC_FLAGGED;
				if (st == MSW_DUE) {
					const int is_rev = (r >> 1) != (r & 1);
					const i64 t = tix[4 * jb + r];
					int score, te, qe, score2, tb, qb;
					if (t >= 0 && t < R.n_tasks) {
						const bwagpu_matesw_t &h = R.mres[t];
						score = h.score; te = h.te; qe = h.qe; score2 = h.score2; tb = h.tb; qb = h.qb;
					} else if (W == 1) return RESC_HANDOVER;
					else {
						const int tlen = uni((int)(re - rb)), l_ms = uni(l_ms_);
						const int xtra = MSW_XSUBO | MSW_XSTART | (l_ms * opt.a < 250 ? MSW_XBYTE : 0) | (opt.min_seed_len * opt.a);
						const i64 wrb = uni64(rb);
						auto Qf = [&](int c) -> int { return is_rev ? (ms[l_ms - 1 - c] < 4 ? 3 - ms[l_ms - 1 - c] : 4) : (int)ms[c]; };
						auto Tf = [&](int c) -> int { return ref_base(ix, wrb + c); };
						int res[7];
						wave_sync();
						msw_align2(opt, l_ms, Qf, tlen, Tf, xtra, runs, res);
						score = res[0]; te = res[1]; qe = res[2]; score2 = res[3]; tb = res[5]; qb = res[6];
						++n_inline;
					}
					if (score >= opt.min_seed_len && qb >= 0) {
						if (nm >= cap_m) return RESC_OVERFLOW;      // (cannot happen: a call adds at most four and the capacity counts four per anchor)
						if (W == 1 || lane == 0) {
							int at = 0;
							while (at < nm && ma[at].score >= score) ++at;      // before the first entry of strictly lower score (:192-196)
							for (int k = nm; k > at; --k) { resc_copy(&ma[k], &ma[k - 1]); msrc[k] = msrc[k - 1]; }
							// (the record is written in place, field by field: a local copy with its bit-fields would live in private memory)
							bwagpu_alnreg_t &g = ma[at];
							g.rb = is_rev ? (ix.l_pac << 1) - (rb + te + 1) : rb + tb;
							g.re = is_rev ? (ix.l_pac << 1) - (rb + tb) : rb + te + 1;
							g.qb = is_rev ? l_ms_ - (qe + 1) : qb;
							g.qe = is_rev ? l_ms_ - qb : qe + 1;
							g.rid = arid; g.score = score; g.truesc = 0; g.sub = 0; g.alt_sc = 0; g.csub = score2; g.sub_n = 0; g.w = 0;
							g.seedcov = (int)((g.re - g.rb < g.qe - g.qb ? g.re - g.rb : g.qe - g.qb) >> 1);
							g.secondary = -1; g.secondary_all = 0; g.seedlen0 = 0; ((i32*)&g)[18] = (i32)((u32)aalt << 30) /* n_comp = 0, is_alt */; g.frac_rep = 0.f; g.hash = 0;
							msrc[at] = -1 - (jb << 2 | r);
						}
						++nm;
						if (W > 1) wave_sync();
					}
					++n;
				}
				if (n) {
					if (W == 1) nm = resc_sort_dedup<1>(opt, ma, msrc, nm, S);
					else if (nm > 1) {
						int m = resc_sort_dedup_par(opt, ma, msrc, nm, S, lane);
						if (m < 0) {      // (coordinates outside the 16-byte keys: lane 0, in place)
							if (lane == 0) m = resc_sort_dedup<64>(opt, ma, msrc, nm, S);
							m = __builtin_amdgcn_readlane(m, 0);
							wave_sync();
						}
						nm = m;
					}
				}
			}
			n_aligned += n;
		}
		if (W == 1 || lane == 0) R.acnt[rm] = nm;
		if (W > 1) wave_sync();
	}
	if (W == 1 || lane == 0) { bwagpu_rescue_t o; o.n_aligned = n_aligned; o.n_inline = n_inline; o.flags = 0; o.pad_ = 0; R.out[p] = o; }
	return RESC_DONE;
}

// a pair that met a mate or a window beyond the alignment kernel (flags 1), or -- an internal error, reported as such -- outgrew its capacity (flags 2)
template <int W>
DEVFN void resc_give_up(const RescIn &R, int p, int why, int lane)
{
	resc_reset<W>(R, p, lane);
	if (W == 1 || lane == 0) { bwagpu_rescue_t o; o.n_aligned = -1; o.n_inline = 0; o.flags = why == RESC_FLAGGED ? 1 : 2; o.pad_ = 0; R.out[p] = o; }
}

// One lane per pair.  Pairs whose larger end has room for more than RESC_LANE_MAX regions, and pairs that need an alignment nobody precomputed, go to the
// wavefront forms: list t of `lists` (n_pairs entries each; 0: keys in LDS, 1: keys in HBM scratch), one atomic per wavefront and list.
__global__ void __launch_bounds__(RESC_LANE_BLOCK) k_rescue_lane(DevIndex ix, bwagpu_opt_t opt, RescIn R, int n_pairs, i32 *lists, unsigned int *list_n)
{
	__shared__ i32 ord[(RESC_LANE_MAX + 1) * RESC_LANE_BLOCK];
	const int lane = threadIdx.x & 63;
	RescSort S = {}; S.ord = ord + threadIdx.x; S.st = RESC_LANE_BLOCK;
	for (i64 p0 = (i64)blockIdx.x * blockDim.x; p0 < n_pairs; p0 += (i64)gridDim.x * blockDim.x) {
		const int p = (int)(p0 + threadIdx.x);
		int tier = -2;      // -2: no pair; -1: this lane's; 0, 1: a list
		if (p < n_pairs) {
			const int c0 = resc_cap(R, 2 * p), c1 = resc_cap(R, 2 * p + 1), c = c0 > c1 ? c0 : c1;
			tier = c <= RESC_LANE_MAX ? -1 : c <= RESC_LDS_MAX ? 0 : 1;
		}
		if (tier == -1) {
			const int rc = rescue_pair<1>(ix, opt, R, p, S, nullptr, 0);
			if (rc == RESC_HANDOVER) tier = 0;
			else if (rc != RESC_DONE) resc_give_up<1>(R, p, rc, 0);
		}
		tier_push<2>(tier, p, n_pairs, lists, list_n, lane);
	}
}

// One wavefront (a workgroup of 64) per pair of `list`.  CAP > 0: the sorts' arrays in LDS; CAP == 0: in the workgroup's part of `scratch` (RESC_WORK_BYTES per region,
// hbm_cap regions).  stage: the workgroup's staging area (RESC_STAGE_BYTES per region, CAP or hbm_cap regions).
#define RESC_WORK_BYTES (sizeof(DdHot) + sizeof(DdKey) + 8)
#define RESC_STAGE_BYTES (sizeof(bwagpu_alnreg_t) + 4)
__host__ __device__ inline size_t resc_stride(size_t per_region, int cap) { return (per_region * (size_t)cap + 15) & ~(size_t)15; }
static_assert(sizeof(RegKey) <= sizeof(DdHot), "the in-place routine's keys alias the decisions' operands");
template <int CAP>
__global__ void __launch_bounds__(64) k_rescue_wave(DevIndex ix, bwagpu_opt_t opt, RescIn R, const i32 *list, const unsigned int *list_n, u8 *scratch, int hbm_cap, u8 *stage)
{
	__shared__ DdHot hot[CAP > 0 ? CAP : 1];
	__shared__ DdKey dkeys[CAP > 0 ? CAP : 1];
	__shared__ i32 ordw[CAP > 0 ? 2 * CAP : 1];
	__shared__ SortFrame stack[DEV_SORT_FRAMES];
	__shared__ i32 runs[MSW_RUN_INTS];
	const int lane = threadIdx.x & 63, cap = CAP > 0 ? CAP : hbm_cap;
	RescSort S; S.st = 1; S.stack = stack;
	if (CAP > 0) { S.hot = hot; S.dkeys = dkeys; S.ord = ordw; S.ord2 = ordw + CAP; }
	else {
		u8 *w = scratch + (size_t)blockIdx.x * resc_stride(RESC_WORK_BYTES, hbm_cap);
		S.hot = (DdHot*)w; S.dkeys = (DdKey*)(w + sizeof(DdHot) * (size_t)hbm_cap); S.ord = (i32*)(w + (sizeof(DdHot) + sizeof(DdKey)) * (size_t)hbm_cap); S.ord2 = S.ord + hbm_cap;
	}
	S.keys = (RegKey*)S.hot;
	{
		u8 *w = stage + (size_t)blockIdx.x * resc_stride(RESC_STAGE_BYTES, cap);
		S.tmp = (bwagpu_alnreg_t*)w; S.tmp_src = (i32*)(w + sizeof(bwagpu_alnreg_t) * (size_t)cap);
	}
	const int nl = (int)*list_n;
	for (int t = blockIdx.x; t < nl; t += gridDim.x) {
		const int p = uni(list[t]);
		const int c0 = resc_cap(R, 2 * p), c1 = resc_cap(R, 2 * p + 1);
		int rc = (c0 > c1 ? c0 : c1) > cap ? RESC_OVERFLOW : RESC_DONE;      // (cannot happen: the host sizes hbm_cap by the batch's largest capacity)
		if (rc == RESC_DONE) rc = rescue_pair<64>(ix, opt, R, p, S, runs, lane);
		if (rc != RESC_DONE) resc_give_up<64>(R, p, rc, lane);
		wave_sync();
	}
}

// The merged lists, packed: read r's acnt[r] regions and src from its place in the arena to poff[r] (poff: k_rescue_scan of acnt).  One wavefront per read,
// a region's 22 words spread over the lanes.
__global__ void __launch_bounds__(256) k_rescue_pack(RescIn R, int n_reads, const i64 *poff, bwagpu_alnreg_t *out, i32 *out_src)
{
	static_assert(sizeof(bwagpu_alnreg_t) == 88, "layout");
	const int lane = threadIdx.x & 63;
	for (i64 r = (i64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n_reads; r += (i64)gridDim.x * (blockDim.x >> 6)) {
		const int n = R.acnt[r];
		const u32 *from = (const u32*)(R.arena + resc_aoff(R, (int)r));
		u32 *to = (u32*)(out + poff[r]);
		for (int k = lane; k < n * 22; k += 64) to[k] = from[k];
		const i32 *sf = R.asrc + resc_aoff(R, (int)r);
		for (int k = lane; k < n; k += 64) out_src[poff[r] + k] = sf[k];
	}
}
