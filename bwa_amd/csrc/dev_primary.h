// dev_primary.h -- primary/secondary marking and mapping quality of a read's regions on the device: what worker2 does first with every read
// (mem_mark_primary_se, bwamem.c:519-584; mem_approx_mapq_se, bwamem.c:982-1006).  bwagpu_batch_primary / bwagpu_primary_flat (bwagpu.hip).
//
// Per read: hash every region with hash_64(id + i) (utils.h:98-109), sort by alnreg_hlt (bwamem.c:423), run the marking loop, then -- when the
// read has hits on ALT contigs -- sort by alnreg_hlt2 (bwamem.c:426), translate the first round's links and run the loop again over the primary-
// assembly hits.  Both orders are total (hash_64 is a bijection, the ids of a read's regions are distinct), so the sorts are rank-by-counting and
// give the reference's permutation whatever ks_introsort does with ties.  The second order is not sorted by key at all: among regions of equal
// (is_alt, score) alnreg_hlt and alnreg_hlt2 both fall back on the hash, so such regions keep the order of the first round and the second round's
// place of a region is its rank by (is_alt, score descending, place in the first round).
//
// One routine, pri_read<W>, in three forms (chosen per read by its number of regions, bwagpu_primary_limits):
//   W = 1   one lane per read, up to PRI_LANE_MAX regions: the working arrays in LDS, interleaved by lane (k_primary_lane);
//   W = 64  one wavefront per read with the arrays in LDS, up to PRI_LDS_SMALL (6 KB per workgroup) or PRI_LDS_BIG regions (48 KB);
//   W = 64  the same with the arrays in an HBM scratch area per workgroup: any number of regions (k_primary_wave<0>).
// In the wavefront forms region i of the marking loop stays serial (the kept list z and sub / sub_n depend on the regions before it); the scan over
// z runs PRI_SCAN entries at a time, and the reference's "first k with a significant overlap" is the lowest set bit of the ballot.
#pragma once
#include <limits.h>
#include <math.h>
#include "dev_common.h"

#define PRI_LANE_MAX 4          // regions up to which a read is marked by one lane
#define PRI_LDS_SMALL 128       // ... by a wavefront with 6 KB of LDS
#define PRI_LDS_BIG 1024        // ... with 48 KB of LDS; reads with more work in HBM scratch
#define PRI_SCAN 64             // entries of the kept list compared per step (one per lane)
#define PRI_LANE_BLOCK 128      // lanes per workgroup of k_primary_lane: 12 words x 4 regions x 128 lanes = 24 KB of LDS
#define PRI_WORDS 12            // 32-bit words of working memory per region

static_assert(sizeof(bwagpu_primary_t) == 32, "layout");

__host__ __device__ inline u64 pri_hash_64(u64 key)
{	// utils.h:98-109
	key += ~(key << 32); key ^= (key >> 22); key += ~(key << 13); key ^= (key >> 8);
	key += (key << 3); key ^= (key >> 15); key += ~(key << 27); key ^= (key >> 31);
	return key;
}

// log(k) of an integer k: on the device from the handle's table of the host's log() values (the device's math library is not the host's libm,
// and (int)(x + .499) turns a last-bit difference into another mapQ); an argument outside the table is reported, not approximated
struct PriLogTab {
	const double *t; int n;
	__host__ __device__ double operator()(int k, int &miss) const { if (k < 0 || k >= n) { miss = 1; return 0.; } return t[k]; }
};
struct PriLogLibm { __host__ __device__ double operator()(int k, int &) const { return log((double)k); } };

// mem_approx_mapq_se (bwamem.c:982-1006) of region `a` with the marked sub / sub_n: the reference's operand types and evaluation order, in double
// precision without contraction (the reference is compiled without FMA; hipcc would fuse `x * y + .499`)
template <class LG>
__host__ __device__ inline int pri_mapq(const bwagpu_opt_t &opt, const bwagpu_alnreg_t &a, int a_sub, int a_sub_n, const LG &lg, int &miss)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
	int mapq, l, sub = a_sub ? a_sub : opt.min_seed_len * opt.a;
	double identity;
	const int score = a.score, csub = a.csub, qb = a.qb, qe = a.qe;
	const i64 rb = a.rb, re = a.re;
	sub = csub > sub ? csub : sub;
	if (sub >= score) return 0;
	l = qe - qb > re - rb ? qe - qb : (int)(re - rb);
	identity = 1. - (double)(l * opt.a - score) / (opt.a + opt.b) / l;
	if (score == 0) mapq = 0;
	else if (opt.mapQ_coef_len > 0) {
		double tmp = l < opt.mapQ_coef_len ? 1. : opt.mapQ_coef_fac / lg(l, miss);
		tmp *= identity * identity;
		mapq = (int)(6.02 * (score - sub) / opt.a * tmp * tmp + .499);
	} else {
		mapq = (int)(30.0 * (1. - (double)sub / score) * lg(a.seedcov, miss) + .499);   // MEM_MAPQ_COEF (bwamem.c:40)
		mapq = identity < 0.95 ? (int)(mapq * identity * identity + .499) : mapq;
	}
	if (a_sub_n > 0) mapq -= (int)(4.343 * lg(a_sub_n + 1, miss) + .499);
	if (mapq > 60) mapq = 60;
	if (mapq < 0) mapq = 0;
	mapq = (int)(mapq * (1. - a.frac_rep) + .499);
	return mapq;
}

// The working arrays of one read; element e of an array is at [e * st] (st = 1, or the lanes of the workgroup when every lane has a read of its own).
// khi / hash (the first sort's keys, by input index) share their memory with sall .. inv, which are first written after that sort: sall[e] and altsc[e]
// are the two halves of khi[e], mp[e] and inv[e] those of hash[e] (element e at [e * 2 * st]: PVA), so that a lane's keys only ever overlap its own arrays.
struct PriView {
	u64 *khi, *hash;
	i32 *sall, *altsc, *mp, *inv;      // secondary_all, alt_sc; place in the first round -> place in the second, and back
	i32 *qb, *qe, *score;              // by place in the first round, as everything below
	u32 *srcalt;                       // input index | (is_alt + 2) << 30
	i32 *sub, *subn, *sec, *z;
	int st;
};
DEVFN PriView pri_view(u64 *raw, int cap, int st, int t)
{
	PriView V; i32 *w = (i32*)raw;
	const size_t a = (size_t)cap * st;
	V.khi = raw + t; V.hash = raw + a + t;
	V.sall = w + 2 * t; V.altsc = w + 2 * t + 1; V.mp = w + 2 * a + 2 * t; V.inv = w + 2 * a + 2 * t + 1;
	V.qb = w + 4 * a + t; V.qe = w + 5 * a + t; V.score = w + 6 * a + t; V.srcalt = (u32*)(w + 7 * a + t);
	V.sub = w + 8 * a + t; V.subn = w + 9 * a + t; V.sec = w + 10 * a + t; V.z = w + 11 * a + t;
	V.st = st;
	return V;
}
#define PV(arr, e) V.arr[(size_t)(e) * V.st]
#define PVA(arr, e) V.arr[(size_t)(e) * 2 * V.st]

DEVFN u64 pri_key_hlt(int score, int alt) { return (u64)(~((u32)score ^ 0x80000000u)) << 2 | (u32)(alt + 2); }      // score descending, then is_alt (the signed two-bit field) ascending
DEVFN u64 pri_key_hlt2(int score, u32 srcalt) { return (u64)(srcalt >> 30) << 32 | (~((u32)score ^ 0x80000000u)); }  // is_alt ascending, then score descending

// the test of mem_mark_primary_se_core (bwamem.c:530-534): an int compared with a float product, in single precision as written
DEVFN bool pri_overlap(int qbi, int qei, int qbj, int qej, float mask_level)
{
	const int b_max = qbj > qbi ? qbj : qbi, e_min = qej < qei ? qej : qei;
	if (e_min <= b_max) return false;
	const int min_l = qei - qbi < qej - qbj ? qei - qbi : qej - qbj;
	return (float)(e_min - b_max) >= (float)min_l * mask_level;
}

// mem_mark_primary_se_core over the first n places of the current order (IND: the second round, place i is element inv[i])
template <int W, bool IND>
DEVFN void pri_core(const PriView &V, float mask_level, int tmp, int n, int lane)
{
	if (n <= 0) return;
	int nz = 1;
	if (lane == 0) PV(z, 0) = 0;
	if (W > 1) __syncthreads();
	for (int i = 1; i < n; ++i) {
		const int ei = IND ? PVA(inv, i) : i;
		const int qbi = PV(qb, ei), qei = PV(qe, ei);
		int found = -1;
		for (int base = 0; base < nz; base += W) {
			const int k = base + lane;
			bool hit = false;
			if (k < nz) {
				const int zj = PV(z, k), ej = IND ? PVA(inv, zj) : zj;
				hit = pri_overlap(qbi, qei, PV(qb, ej), PV(qe, ej), mask_level);
			}
			if (W > 1) {
				const unsigned long long m = __ballot(hit);
				if (m) { found = base + __ffsll(m) - 1; break; }
			} else if (hit) { found = k; break; }
		}
		if (found >= 0) {
			if (lane == 0) {
				const int zj = PV(z, found), ej = IND ? PVA(inv, zj) : zj, si = PV(score, ei);
				if (PV(sub, ej) == 0) PV(sub, ej) = si;
				if (PV(score, ej) - si <= tmp && ((PV(srcalt, ej) >> 30) != 2u || (PV(srcalt, ei) >> 30) == 2u)) ++PV(subn, ej);
				PV(sec, ei) = zj;
			}
		} else {
			if (lane == 0) PV(z, nz) = i;
			++nz;
			if (W > 1) __syncthreads();
		}
	}
	if (W > 1) __syncthreads();
}

// One read: regions a[0 .. n), n >= 1, at most the view's capacity; records to out[0 .. n) in the order mem_mark_primary_se leaves the list.
template <int W>
DEVFN int pri_read(const PriView &V, const bwagpu_opt_t &opt, const PriLogTab &lg, const bwagpu_alnreg_t *a, int n, i64 id, bwagpu_primary_t *out, int lane)
{
	int tmp = opt.a + opt.b;
	tmp = opt.o_del + opt.e_del > tmp ? opt.o_del + opt.e_del : tmp;
	tmp = opt.o_ins + opt.e_ins > tmp ? opt.o_ins + opt.e_ins : tmp;
	// keys of the first order, by input index
	int np = 0;
	for (int i = lane; i < n; i += W) {
		const int alt = a[i].is_alt;
		PV(khi, i) = pri_key_hlt(a[i].score, alt); PV(hash, i) = pri_hash_64((u64)(id + i));
		np += alt == 0;
	}
	if (W > 1) { for (int d = 32; d; d >>= 1) np += __shfl_xor(np, d); __syncthreads(); }
	// rank by counting; the regions' fields go to their places
	for (int i = lane; i < n; i += W) {
		const u64 ki = PV(khi, i), hi = PV(hash, i);
		int r = 0;
		for (int j = 0; j < n; ++j) { const u64 kj = PV(khi, j); r += kj < ki || (kj == ki && PV(hash, j) < hi); }
		PV(qb, r) = a[i].qb; PV(qe, r) = a[i].qe; PV(score, r) = a[i].score; PV(srcalt, r) = (u32)i | (u32)(a[i].is_alt + 2) << 30;
		PV(sub, r) = 0; PV(subn, r) = a[i].sub_n; PV(sec, r) = -1;
	}
	if (W > 1) __syncthreads();
	pri_core<W, false>(V, opt.mask_level, tmp, n, lane);
	// alt_sc (bwamem.c:561-562); the second order, or none (the keys are dead: their memory now holds altsc, mp, inv, sall)
	const bool second = np > 0 && np < n;
	for (int p = lane; p < n; p += W) {
		const int s = PV(sec, p);
		PVA(altsc, p) = ((PV(srcalt, p) >> 30) == 2u && s >= 0 && (PV(srcalt, s) >> 30) != 2u) ? PV(score, s) : 0;
		int r = p;
		if (second) {
			const u64 kp = pri_key_hlt2(PV(score, p), PV(srcalt, p));
			r = 0;
			for (int q = 0; q < n; ++q) { const u64 kq = pri_key_hlt2(PV(score, q), PV(srcalt, q)); r += kq < kp || (kq == kp && q < p); }
		}
		PVA(mp, p) = r; PVA(inv, r) = p;
	}
	if (W > 1) __syncthreads();
	// the first round's links in the second order (bwamem.c:567-573, 579-580)
	for (int p = lane; p < n; p += W) {
		const int s = PV(sec, p);
		if (np < n) {
			if (s >= 0) { PVA(sall, p) = PVA(mp, s); if ((PV(srcalt, p) >> 30) != 2u) PV(sec, p) = INT_MAX; }
			else PVA(sall, p) = -1;
		} else PVA(sall, p) = s;
	}
	if (W > 1) __syncthreads();
	if (second) {   // the primary-assembly hits among themselves (bwamem.c:574-577); sub_n is not reset, as in the reference
		for (int i = lane; i < np; i += W) { const int e = PVA(inv, i); PV(sub, e) = 0; PV(sec, e) = -1; }
		if (W > 1) __syncthreads();
		pri_core<W, true>(V, opt.mask_level, tmp, np, lane);
	}
	for (int i = lane; i < n; i += W) {
		const int e = PVA(inv, i), src = (int)(PV(srcalt, e) & 0x3fffffffu);
		bwagpu_primary_t rec;
		int miss = 0;
		rec.src = src; rec.secondary = PV(sec, e); rec.secondary_all = PVA(sall, e); rec.sub = PV(sub, e); rec.alt_sc = PVA(altsc, e); rec.sub_n = PV(subn, e);
		rec.mapq = pri_mapq(opt, a[src], rec.sub, rec.sub_n, lg, miss);
		rec.flags = miss;
		out[i] = rec;
	}
	if (W > 1) __syncthreads();      // (the workgroup's next read writes the same arrays)
	return np;
}

// One lane per read.  Reads with more than PRI_LANE_MAX regions are handed to the wavefront forms: list t of `lists` (n_reads entries each) takes the reads
// of form t (0: PRI_LDS_SMALL, 1: PRI_LDS_BIG, 2: HBM scratch), one atomic per wavefront and list.
__global__ void __launch_bounds__(PRI_LANE_BLOCK) k_primary_lane(bwagpu_opt_t opt, int n_reads, const i32 *cnt, const i64 *off, const bwagpu_alnreg_t *regs, const i64 *ids, i64 id0,
																  PriLogTab lg, bwagpu_primary_t *out, i32 *n_pri, i32 *lists, unsigned int *list_n)
{
	__shared__ u64 raw[PRI_WORDS / 2 * PRI_LANE_MAX * PRI_LANE_BLOCK];
	const int lane = threadIdx.x & 63;
	const PriView V = pri_view(raw, PRI_LANE_MAX, PRI_LANE_BLOCK, (int)threadIdx.x);
	for (i64 r0 = (i64)blockIdx.x * blockDim.x; r0 < n_reads; r0 += (i64)gridDim.x * blockDim.x) {
		const int r = (int)(r0 + threadIdx.x);
		const int n = r < n_reads ? cnt[r] : 0;
		const int tier = n <= PRI_LANE_MAX ? -1 : n <= PRI_LDS_SMALL ? 0 : n <= PRI_LDS_BIG ? 1 : 2;
		tier_push<3>(tier, r, n_reads, lists, list_n, lane);
		if (r < n_reads && n <= 0) n_pri[r] = 0;
		if (n >= 1 && tier < 0) n_pri[r] = pri_read<1>(V, opt, lg, regs + off[r], n, ids ? ids[r] : id0 + r, out + off[r], 0);
	}
}

// One wavefront (a workgroup of 64) per read of `list`.  CAP > 0: the arrays in LDS; CAP == 0: in the workgroup's part of `scratch` (hbm_cap regions).
template <int CAP>
__global__ void __launch_bounds__(64) k_primary_wave(bwagpu_opt_t opt, const i32 *cnt, const i64 *off, const bwagpu_alnreg_t *regs, const i64 *ids, i64 id0, PriLogTab lg,
													  bwagpu_primary_t *out, i32 *n_pri, const i32 *list, const unsigned int *list_n, u64 *scratch, int hbm_cap)
{
	__shared__ u64 raw[CAP > 0 ? PRI_WORDS / 2 * CAP : 1];
	const int lane = threadIdx.x & 63, cap = CAP > 0 ? CAP : hbm_cap;
	const PriView V = CAP > 0 ? pri_view(raw, CAP, 1, 0) : pri_view(scratch + (size_t)blockIdx.x * (PRI_WORDS / 2) * hbm_cap, hbm_cap, 1, 0);
	const int nl = (int)*list_n;
	for (int t = blockIdx.x; t < nl; t += gridDim.x) {
		const int r = list[t], n = cnt[r];
		if (n > cap) { if (lane == 0) n_pri[r] = -1; continue; }      // (cannot happen: the host sizes hbm_cap by the batch's largest count; reported as an error)
		const int np = pri_read<64>(V, opt, lg, regs + off[r], n, ids ? ids[r] : id0 + r, out + off[r], lane);
		if (lane == 0) n_pri[r] = np;
	}
}
