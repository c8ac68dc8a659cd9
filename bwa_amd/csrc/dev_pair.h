// dev_pair.h -- pairing of the two ends' hits on the device: what worker2 does after it has marked both ends (mem_pair, bwamem_pair.c:208-269).
// bwagpu_batch_pair / bwagpu_pair_flat (bwagpu.hip).  The input of a pair is the first n_pri regions of each end's marked list (the primary-assembly hits).
//
// What makes it exact:
//   * The sort of v is rank by counting.  Key x is rid<<32 | forward position - contig offset (:218-219), key y is score<<32 | i<<2 | strand<<1 | r (:220).
//     The (i, r) are distinct, so the 128-bit order (utils.c:44) is total and a rank computed by counting is the permutation ks_introsort_128 (:224)
//     gives.  The sorted positions themselves matter: p->y = k<<32 | i (:247) is hashed.
//   * The candidate scan depends only on the set.  After the sort dist = x_i - x_k (:239) grows as k falls, so the loop of :233-250 with its
//     `continue`s (:238, :242) and its `break` (:241) visits exactly {k < i : (y_k & 3) == which, low <= x_i - x_k <= high} for each of the two r (:228-232).
//     x carries the contig in its high bits, so hits on another contig are outside every window.  An element k belongs to at most one r of a given i
//     (which = r<<1 | other end, :231), so one walk down from i - 1 serves both r, and it may stop at the largest `high` of the live orientations.
//     Lanes take the i in parallel.
//   * u is never stored or sorted (:258).  Three things are read from it: its largest element by (x, y) gives ret and z[] (:259-262), the second largest
//     q is *sub (:263), and *n_sub is the number of elements other than the largest with sub - q <= tmp (:264-265).  That is a reduction (the two
//     largest, then a count in a second walk when there are at least two candidates); the y of u are distinct, so the maximum is unique.  u.n is kept too.
//   * The score q (:244) must be bit-equal to the host's, and the device's erfc / log are not glibc's: for every orientation that has not failed the host
//     side of the call fills a table T of log(2. * erfc(fabs(ns) * M_SQRT1_2)) for every integer dist in [low, high], ns = (dist - avg) / std as written
//     (:243).  pair_q evaluates (int)((u64)(s_i + s_k) + .721 * T * opt.a + .499) with the reference's operand types and order, in double, contraction
//     off, as pri_mapq does.  A distance outside the table (option pair_tab_cap) flags the pair (bit 0) and the host side of the call recomputes it.
//   * The hash is hash_64(p->y ^ id<<8) with `int id` (:248): the shift is done in 32 bits and then sign-extended.
//   * No candidate (:266): ret = sub = n_sub = 0 and z = {-1, -1} (the reference leaves z untouched).
//
// One routine, pair_read<W>, in three forms chosen per pair by n_pri[0] + n_pri[1] (bwagpu_pair_limits):
//   W = 1   one lane per pair, up to PAIR_LANE_MAX hits: the arrays in LDS, interleaved by lane (k_pair_lane);
//   W = 64  one wavefront per pair with the arrays in LDS, up to PAIR_LDS_SMALL (4 KB per workgroup) or PAIR_LDS_BIG hits (32 KB);
//   W = 64  the same with the arrays in an HBM scratch area per workgroup: any number (k_pair_wave<0>).
#pragma once
#include <limits.h>
#include <math.h>
#include "dev_common.h"
#include "dev_primary.h"

#define PAIR_LANE_MAX 4         // hits of both ends up to which a pair is done by one lane
#define PAIR_LDS_SMALL 128      // ... by a wavefront with 4 KB of LDS
#define PAIR_LDS_BIG 1024       // ... with 32 KB of LDS; pairs with more work in HBM scratch
#define PAIR_LANE_BLOCK 128     // lanes per workgroup of k_pair_lane: 8 words x 4 hits x 128 lanes = 16 KB of LDS
#define PAIR_WORDS 8            // 32-bit words of working memory per hit

static_assert(sizeof(bwagpu_pair_t) == 32 && sizeof(bwagpu_pestat_t) == 32, "layout");

// the four windows and the table of log(2 erfc(|ns| / sqrt 2)): orientation d has tlen[d] entries from t[toff[d]], for dist = low[d] ..
struct PairWin { const double *t; i32 low[4], high[4], failed[4], toff[4], tlen[4]; };

// (the windows are kernel arguments: an index that differs from lane to lane would move them to private memory)
__host__ __device__ inline i32 pair_pick(const i32 (&a)[4], int d) { return d == 0 ? a[0] : d == 1 ? a[1] : d == 2 ? a[2] : a[3]; }

// :244-245 with T = log(2. * erfc(fabs(ns) * M_SQRT1_2)); si, sk = y >> 32 of the two hits
__host__ __device__ inline int pair_q(u64 si, u64 sk, double T, int a)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
	int q = (int)((si + sk) + .721 * T * a + .499);
	return q < 0 ? 0 : q;
}
// :218-220
__host__ __device__ inline void pair_key(const bwagpu_alnreg_t &e, int i, int r, i64 l_pac, i64 ctg_off, u64 &x, u64 &y)
{
	x = (u64)(e.rb < l_pac ? e.rb : (l_pac << 1) - 1 - e.rb);
	x = (u64)(i64)e.rid << 32 | (x - (u64)ctg_off);
	y = (u64)(i64)e.score << 32 | (u64)(i64)(i << 2) | (u64)((e.rb >= l_pac) << 1) | (u64)r;
}
// :247-248
__host__ __device__ inline u64 pair_cand_x(int q, u64 py, int id) { return (u64)(i64)q << 32 | (pri_hash_64(py ^ (u64)(i64)(i32)((u32)id << 8)) & 0xffffffffu); }
__host__ __device__ inline bool pair_lt(u64 ax, u64 ay, u64 bx, u64 by) { return ax < bx || (ax == bx && ay < by); }      // utils.c:44
__host__ __device__ inline int pair_tmp(const bwagpu_opt_t &opt)
{	// :255-257
	int tmp = opt.a + opt.b;
	tmp = tmp > opt.o_del + opt.e_del ? tmp : opt.o_del + opt.e_del;
	tmp = tmp > opt.o_ins + opt.e_ins ? tmp : opt.o_ins + opt.e_ins;
	return tmp;
}

// The working arrays of one pair: keys by input place (kx, ky), then in sorted order (sx, sy); element e of an array is at [e * st].
struct PairView { u64 *kx, *ky, *sx, *sy; int st; };
DEVFN PairView pair_view(u64 *raw, int cap, int st, int t)
{
	PairView V; const size_t a = (size_t)cap * st;
	V.kx = raw + t; V.ky = raw + a + t; V.sx = raw + 2 * a + t; V.sy = raw + 3 * a + t; V.st = st;
	return V;
}
#define QV(arr, e) V.arr[(size_t)(e) * V.st]

// the two largest candidates seen; (0, 0) is below every candidate (a candidate's y = k<<32 | i has i >= 1)
struct PairTop { u64 x1, y1, x2, y2; };
DEVFN void pair_push(PairTop &B, u64 x, u64 y)
{
	if (pair_lt(B.x1, B.y1, x, y)) { B.x2 = B.x1; B.y2 = B.y1; B.x1 = x; B.y1 = y; }
	else if (pair_lt(B.x2, B.y2, x, y)) { B.x2 = x; B.y2 = y; }
}
DEVFN u64 pair_shfl_xor(u64 v, int d) { return (u64)(u32)__shfl_xor((int)(u32)v, d) | (u64)(u32)__shfl_xor((int)(u32)(v >> 32), d) << 32; }

// The candidates of the sorted places i = lane, lane + W, ..: f(x, y) for each.  Returns their number.
template <int W, class F>
DEVFN i64 pair_scan(const PairView &V, const PairWin &P, int n, int a, int id, int max_high, int &miss, int lane, F f)
{
	i64 cnt = 0;
	for (int i = lane; i < n; i += W) {
		const u64 xi = QV(sx, i), yi = QV(sy, i);
		const int strand = (int)(yi >> 1 & 1), end = (int)(yi & 1);
		for (int k = i - 1; k >= 0; --k) {
			const i64 dist = (i64)xi - (i64)QV(sx, k);
			if (dist > max_high) break;
			const u64 yk = QV(sy, k);
			if ((int)(yk & 1) == end) continue;                    // which = r<<1 | the other end (:231)
			const int dir = (int)(yk & 2) | strand;               // r = (y_k & 3) >> 1 (:229)
			if (pair_pick(P.failed, dir) || dist < pair_pick(P.low, dir) || dist > pair_pick(P.high, dir)) continue;
			const i64 at = dist - pair_pick(P.low, dir);
			double T = 0.;
			if (at < pair_pick(P.tlen, dir)) T = P.t[pair_pick(P.toff, dir) + at]; else miss = 1;
			const u64 py = (u64)k << 32 | (u64)i;
			f(pair_cand_x(pair_q(yi >> 32, yk >> 32, T, a), py, id), py);
			++cnt;
		}
	}
	return cnt;
}

// One pair: the first n0 / n1 places of the two ends' marked lists (place i of an end is region src[i].src of its list a, or region i when src is null),
// 1 <= n0, 1 <= n1, n0 + n1 at most the view's capacity.  Every lane returns the record.
template <int W>
DEVFN bwagpu_pair_t pair_read(const PairView &V, const bwagpu_opt_t &opt, const PairWin &P, i64 l_pac, int n_seqs, const i64 *ctg_off, const bwagpu_alnreg_t *a0,
							  const bwagpu_primary_t *src0, int n0, const bwagpu_alnreg_t *a1, const bwagpu_primary_t *src1, int n1, int id, int lane)
{
	const int n = n0 + n1;
	for (int e = lane; e < n; e += W) {
		const int r = e >= n0, i = r ? e - n0 : e;
		const bwagpu_alnreg_t &g = r ? a1[src1 ? src1[i].src : i] : a0[src0 ? src0[i].src : i];
		u64 x, y;
		pair_key(g, i, r, l_pac, g.rid >= 0 && g.rid < n_seqs ? ctg_off[g.rid] : 0, x, y);
		QV(kx, e) = x; QV(ky, e) = y;
	}
	if (W > 1) __syncthreads();
	for (int e = lane; e < n; e += W) {
		const u64 x = QV(kx, e), y = QV(ky, e);
		int r = 0;
		for (int f = 0; f < n; ++f) r += pair_lt(QV(kx, f), QV(ky, f), x, y);
		QV(sx, r) = x; QV(sy, r) = y;
	}
	if (W > 1) __syncthreads();
	int max_high = INT_MIN, miss = 0;
	for (int d = 0; d < 4; ++d) if (!P.failed[d] && P.high[d] > max_high) max_high = P.high[d];
	PairTop B = { 0, 0, 0, 0 };
	i64 cnt = pair_scan<W>(V, P, n, opt.a, id, max_high, miss, lane, [&](u64 x, u64 y) { pair_push(B, x, y); });
	if (W > 1) {
		for (int d = 32; d; d >>= 1) {
			const u64 ox1 = pair_shfl_xor(B.x1, d), oy1 = pair_shfl_xor(B.y1, d), ox2 = pair_shfl_xor(B.x2, d), oy2 = pair_shfl_xor(B.y2, d);
			pair_push(B, ox1, oy1); pair_push(B, ox2, oy2);
			cnt += (i64)pair_shfl_xor((u64)cnt, d);
			miss |= __shfl_xor(miss, d);
		}
	}
	bwagpu_pair_t rec;
	rec.score = rec.sub = rec.n_sub = 0; rec.z[0] = rec.z[1] = -1; rec.flags = miss; rec.n_cand = cnt;
	if (cnt > 0) {
		const u64 yk = QV(sy, B.y1 >> 32), yi = QV(sy, B.y1 & 0xffffffffu);      // :259-262
		const int zk = (int)((yk & 0xffffffffu) >> 2), zi = (int)((yi & 0xffffffffu) >> 2);      // (the two are of different ends; no indexing of the record by a lane's value)
		rec.z[0] = yk & 1 ? zi : zk; rec.z[1] = yk & 1 ? zk : zi;
		rec.score = (int)(B.x1 >> 32);
		if (cnt > 1) {
			const int sub = (int)(B.x2 >> 32), tmp = pair_tmp(opt);
			int ns = 0, miss2 = 0;
			const u64 besty = B.y1;
			pair_scan<W>(V, P, n, opt.a, id, max_high, miss2, lane, [&](u64 x, u64 y) { if (y != besty && sub - (int)(x >> 32) <= tmp) ++ns; });
			if (W > 1) for (int d = 32; d; d >>= 1) ns += __shfl_xor(ns, d);
			rec.sub = sub; rec.n_sub = ns;
		}
	}
	if (W > 1) __syncthreads();      // (the workgroup's next pair writes the same arrays)
	return rec;
}

__host__ __device__ inline bwagpu_pair_t pair_none() { bwagpu_pair_t r; r.score = r.sub = r.n_sub = 0; r.z[0] = r.z[1] = -1; r.flags = 0; r.n_cand = 0; return r; }

// One lane per pair: reads 2p and 2p + 1 (lists at off[] of regs, n_pri[] places each; src: the marking records at the same offsets, or null).  Pair p has id
// ids[p], or id0 + p, truncated to int (:208).  Pairs with more than PAIR_LANE_MAX hits are handed to the wavefront forms: list t of `lists` (n_pairs entries
// each) takes the pairs of form t (0: PAIR_LDS_SMALL, 1: PAIR_LDS_BIG, 2: HBM scratch), one atomic per wavefront and list.
__global__ void __launch_bounds__(PAIR_LANE_BLOCK) k_pair_lane(bwagpu_opt_t opt, PairWin P, i64 l_pac, int n_seqs, const i64 *ctg_off, int n_pairs, const i32 *n_pri, const i64 *off,
																const bwagpu_alnreg_t *regs, const bwagpu_primary_t *src, const i64 *ids, i64 id0, bwagpu_pair_t *out, i32 *lists, unsigned int *list_n)
{
	__shared__ u64 raw[PAIR_WORDS / 2 * PAIR_LANE_MAX * PAIR_LANE_BLOCK];
	const int lane = threadIdx.x & 63;
	const PairView V = pair_view(raw, PAIR_LANE_MAX, PAIR_LANE_BLOCK, (int)threadIdx.x);
	for (i64 p0 = (i64)blockIdx.x * blockDim.x; p0 < n_pairs; p0 += (i64)gridDim.x * blockDim.x) {
		const int p = (int)(p0 + threadIdx.x);
		const int n0 = p < n_pairs ? n_pri[2 * (size_t)p] : 0, n1 = p < n_pairs ? n_pri[2 * (size_t)p + 1] : 0;
		const bool live = n0 > 0 && n1 > 0;
		const i64 n = (i64)n0 + n1;
		const int tier = !live || n <= PAIR_LANE_MAX ? -1 : n <= PAIR_LDS_SMALL ? 0 : n <= PAIR_LDS_BIG ? 1 : 2;
		tier_push<3>(tier, p, n_pairs, lists, list_n, lane);
		if (p < n_pairs && !live) out[p] = pair_none();
		if (live && tier < 0) {
			const i64 o0 = off[2 * (size_t)p], o1 = off[2 * (size_t)p + 1];
			out[p] = pair_read<1>(V, opt, P, l_pac, n_seqs, ctg_off, regs + o0, src ? src + o0 : nullptr, n0, regs + o1, src ? src + o1 : nullptr, n1, (int)(ids ? ids[p] : id0 + p), 0);
		}
	}
}

// One wavefront (a workgroup of 64) per pair of `list`.  CAP > 0: the arrays in LDS; CAP == 0: in the workgroup's part of `scratch` (hbm_cap hits).
template <int CAP>
__global__ void __launch_bounds__(64) k_pair_wave(bwagpu_opt_t opt, PairWin P, i64 l_pac, int n_seqs, const i64 *ctg_off, const i32 *n_pri, const i64 *off, const bwagpu_alnreg_t *regs,
												   const bwagpu_primary_t *src, const i64 *ids, i64 id0, bwagpu_pair_t *out, const i32 *list, const unsigned int *list_n, u64 *scratch, int hbm_cap)
{
	__shared__ u64 raw[CAP > 0 ? PAIR_WORDS / 2 * CAP : 1];
	const int lane = threadIdx.x & 63, cap = CAP > 0 ? CAP : hbm_cap;
	const PairView V = CAP > 0 ? pair_view(raw, CAP, 1, 0) : pair_view(scratch + (size_t)blockIdx.x * (PAIR_WORDS / 2) * hbm_cap, hbm_cap, 1, 0);
	const int nl = (int)*list_n;
	for (int t = blockIdx.x; t < nl; t += gridDim.x) {
		const int p = list[t], n0 = n_pri[2 * (size_t)p], n1 = n_pri[2 * (size_t)p + 1];
		if ((i64)n0 + n1 > cap) { if (lane == 0) { bwagpu_pair_t r = pair_none(); r.flags = 2; out[p] = r; } continue; }      // (cannot happen: the host sizes hbm_cap by the batch's largest pair; reported as an error)
		const i64 o0 = off[2 * (size_t)p], o1 = off[2 * (size_t)p + 1];
		const bwagpu_pair_t rec = pair_read<64>(V, opt, P, l_pac, n_seqs, ctg_off, regs + o0, src ? src + o0 : nullptr, n0, regs + o1, src ? src + o1 : nullptr, n1, (int)(ids ? ids[p] : id0 + p), lane);
		if (lane == 0) out[p] = rec;
	}
}
