// dev_pestat.h -- the insert-size windows of a paired-end batch on the device: mem_pestat (bwamem_pair.c:72-135), the one batch-global step of the
// paired-end path (bwamem.c:1258).  bwagpu_batch_pestat / bwagpu_pestat_flat / bwagpu_batch_pestat_hist / bwagpu_pestat_finish (bwagpu.hip).
//
// k_pestat_collect restates the filter of :78-90, one lane per pair: both ends have a region, cal_sub (:58-70) of either end is at most 0.8 of its first
// region's score, the first regions lie on one contig, and the distance mem_infer_dir (:49-56) gives is in [1, max_ins].  Such a pair adds one to bin
// hist[dir][is]; the list isize[dir] of the reference is that histogram, and everything after :91 reads only the sorted list.  Counts add: the histogram
// of a batch is the sum of its shards' histograms, whichever devices made them.
//
// k_pestat_finish is one workgroup of four wavefronts, wavefront d for orientation d.  What makes it exact:
//   * The order statistics (:103-105) are elements (int)(f * n + .499) of the sorted list, f * n in double as written: the bin at which the running count
//     first exceeds that index.  Every lane first sums one contiguous segment of the bins (their total is n); the wavefront then walks the one segment that
//     holds the index 64 bins a step with a prefix count over the lanes.
//   * avg (:111-114).  The reference adds integers into a double.  Every partial sum is an integer below 2^53 (n < 2^31 elements of at most 2^22), so each
//     of its additions is exact and any order gives the same bits: the sum is reduced in 64-bit integers and converted once; avg = sum / x is one IEEE division.
//   * std (:115-118).  The reference adds (v - avg) * (v - avg) element by element in ascending order, every addition rounded; that is not associative.  Lane 0
//     walks the bins from the lower to the upper outlier bound and adds the bin's term cnt[v] times, one rounded addition each: the same chain of additions
//     (equal elements have equal terms).  The other lanes fetch the bins 64 at a time.  No closed form for a run of equal terms is used.
//   * sqrt and the divisions are the correctly rounded ones (the library is built without fast-math); everything is double, contraction off, with the
//     reference's operand types: (int)(p25 - 2.0 * (p75 - p25) + .499) and so on (:106-108, :120-124).
//   * MIN_DIR_RATIO (:128-134) after a barrier: n_d < max * 0.05 with max an int, in double.
// An orientation with fewer than MIN_DIR_CNT pairs has failed = 1 and every other field 0 (:76, :96-100).  The info record keeps what the scalars were made
// from (and what the reference prints at -v 3).  n >= 2^31 in one orientation (only sums of foreign histograms can get there) is reported, not computed.
#pragma once
#include <math.h>
#include "dev_common.h"
#include "dev_primary.h"

#define PST_MIN_DIR_CNT 10              // MIN_DIR_CNT (bwamem_pair.c:43)
#define PST_MAX_INS (1 << 22)           // the largest max_ins served: 4 x (2^22 + 1) bins are 64 MB
#define PST_BLOCK 256                   // lanes per workgroup of both kernels (k_pestat_finish: four wavefronts, one per orientation)

struct PstOut { bwagpu_pestat_t pes[4]; bwagpu_pestat_info_t info; };      // the handle's result buffer: what the call copies to the host, byte for byte
static_assert(sizeof(bwagpu_pestat_t) == 32 && sizeof(bwagpu_pestat_info_t) == 208 && sizeof(PstOut) == 336, "layout");

// cal_sub (:58-70): the score of the first region after the best that overlaps it significantly on the read, or min_seed_len * a
DEVFN int pst_cal_sub(const bwagpu_alnreg_t *a, int n, float mask_level, int fallback)
{
	const int qb0 = a[0].qb, qe0 = a[0].qe;
	for (int j = 1; j < n; ++j)
		if (pri_overlap(qb0, qe0, a[j].qb, a[j].qe, mask_level)) return a[j].score;      // (the same int >= int * float test as bwamem.c:530-534)
	return fallback;
}

// mem_infer_dir (:49-56)
DEVFN int pst_infer_dir(i64 l_pac, i64 b1, i64 b2, i64 &dist)
{
	const int r1 = b1 >= l_pac, r2 = b2 >= l_pac;
	const i64 p2 = r1 == r2 ? b2 : (l_pac << 1) - 1 - b2;
	dist = p2 > b1 ? p2 - b1 : b1 - p2;
	return (r1 == r2 ? 0 : 1) ^ (p2 > b1 ? 0 : 3);
}

// One lane per pair (reads 2p, 2p + 1: cnt[] regions each from regs[off[]]); hist: 4 x (max_ins + 1) counts, max_ins >= 1.
__global__ void __launch_bounds__(PST_BLOCK) k_pestat_collect(float mask_level, int fallback, int max_ins, i64 l_pac, int n_pairs, const i32 *cnt, const i64 *off,
																  const bwagpu_alnreg_t *regs, unsigned int *hist)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
	for (i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += (i64)gridDim.x * blockDim.x) {
		const int n0 = cnt[2 * p], n1 = cnt[2 * p + 1];
		if (n0 <= 0 || n1 <= 0) continue;
		const bwagpu_alnreg_t *a0 = regs + off[2 * p], *a1 = regs + off[2 * p + 1];
		if (a0[0].rid != a1[0].rid) continue;
		if ((double)pst_cal_sub(a0, n0, mask_level, fallback) > 0.8 * (double)a0[0].score) continue;      // MIN_RATIO: an int against a double
		if ((double)pst_cal_sub(a1, n1, mask_level, fallback) > 0.8 * (double)a1[0].score) continue;
		i64 is;
		const int dir = pst_infer_dir(l_pac, a0[0].rb, a1[0].rb, is);
		if (is != 0 && is <= (i64)max_ins) atomicAdd(&hist[(size_t)dir * ((size_t)max_ins + 1) + (size_t)is], 1u);
	}
}

DEVFN u64 pst_wave_sum(u64 v)
{
	for (int d = 32; d; d >>= 1) {
		const u32 lo = (u32)__shfl_xor((int)(u32)v, d), hi = (u32)__shfl_xor((int)(u32)(v >> 32), d);
		v += (u64)hi << 32 | lo;
	}
	return v;
}
DEVFN u32 pst_wave_scan(u32 v, int lane)      // inclusive prefix sum over the lanes
{
	for (int d = 1; d < 64; d <<= 1) { const u32 t = (u32)__shfl_up((int)v, d); if (lane >= d) v += t; }
	return v;
}

// Element k (from 0) of the sorted list: the bin at which the running count first exceeds k.  incl: the inclusive prefix over the lanes of the segments'
// sums (lane l holds bins [l * seg, (l + 1) * seg)); k is below the total, so a segment and a bin are found.
DEVFN int pst_select(const unsigned int *cnt, int nb, int seg, u32 incl, u32 k, int lane)
{
	const int L = __popcll(__ballot(incl <= k));      // the segments that end at or before k
	u32 base = (u32)__shfl((int)incl, L > 0 ? L - 1 : 0);
	if (L == 0) base = 0;
	const int end = (L + 1) * seg < nb ? (L + 1) * seg : nb;
	for (int b0 = L * seg; b0 < end; b0 += 64) {
		const int b = b0 + lane;
		const u32 sc = pst_wave_scan(b < end ? cnt[b] : 0u, lane), tot = (u32)__shfl((int)sc, 63);
		if (k - base < tot) return b0 + __ffsll(__ballot(base + sc > k)) - 1;
		base += tot;
	}
	return nb - 1;      // (not reached)
}

// hist: 4 x (max_ins + 1) counts, 1 <= max_ins <= PST_MAX_INS; *out zeroed by the caller (the padding of the records stays zero).
__global__ void __launch_bounds__(PST_BLOCK) k_pestat_finish(const unsigned int *hist, int max_ins, PstOut *out)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
	__shared__ unsigned long long s_n[4];
	__shared__ int s_failed[4];
	const int d = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
	const int nb = max_ins + 1, seg = (nb + 63) >> 6;
	const unsigned int *cnt = hist + (size_t)d * nb;
	u64 mine = 0;
	for (int b = lane * seg, e = b + seg < nb ? b + seg : nb; b < e; ++b) mine += cnt[b];
	const u64 n = pst_wave_sum(mine);
	const bool live = n >= PST_MIN_DIR_CNT && n < ((u64)1 << 31);
	if (lane == 0) { s_n[d] = n; s_failed[d] = !live; out->info.n[d] = (i64)n; }
	if (live) {      // (the same for the whole wavefront)
		const u32 incl = pst_wave_scan((u32)mine, lane);
		const int p25 = pst_select(cnt, nb, seg, incl, (u32)(int)(.25 * (double)n + .499), lane);
		const int p50 = pst_select(cnt, nb, seg, incl, (u32)(int)(.50 * (double)n + .499), lane);
		const int p75 = pst_select(cnt, nb, seg, incl, (u32)(int)(.75 * (double)n + .499), lane);
		int low = (int)(p25 - 2.0 * (p75 - p25) + .499);      // OUTLIER_BOUND
		if (low < 1) low = 1;
		int high = (int)(p75 + 2.0 * (p75 - p25) + .499);
		const int lo_out = low, hi_out = high, top = high < nb - 1 ? high : nb - 1;      // (no value lies beyond the last bin)
		u64 sum = 0, x = 0;
		for (int v = low + lane; v <= top; v += 64) { const u32 c = cnt[v]; sum += (u64)v * c; x += c; }
		sum = pst_wave_sum(sum); x = pst_wave_sum(x);
		const double avg = (double)sum / (double)(int)x;      // (x >= 1: the list's element p25 lies within the bounds)
		double sumsq = 0.;
		for (int b0 = low; b0 <= top; b0 += 64) {
			const int v = b0 + lane;
			const u32 c = v <= top ? cnt[v] : 0u;
			for (unsigned long long m = __ballot(c != 0); m; m &= m - 1) {      // the bins of this step that hold something, ascending
				const int j = __ffsll(m) - 1;
				const u32 cj = (u32)__shfl((int)c, j);
				if (lane == 0) {
					const double t = ((double)(u64)(b0 + j) - avg) * ((double)(u64)(b0 + j) - avg);
					for (u32 k = 0; k < cj; ++k) sumsq += t;
				}
			}
		}
		if (lane == 0) {
			const double sd = sqrt(sumsq / (double)(int)x);
			low = (int)(p25 - 3.0 * (p75 - p25) + .499);      // MAPPING_BOUND
			high = (int)(p75 + 3.0 * (p75 - p25) + .499);
			if ((double)low > avg - 4.0 * sd) low = (int)(avg - 4.0 * sd + .499);      // MAX_STDDEV
			if ((double)high < avg + 4.0 * sd) high = (int)(avg + 4.0 * sd + .499);
			if (low < 1) low = 1;
			out->pes[d].low = low; out->pes[d].high = high; out->pes[d].avg = avg; out->pes[d].std = sd;
			out->info.p25[d] = p25; out->info.p50[d] = p50; out->info.p75[d] = p75; out->info.lo_out[d] = lo_out; out->info.hi_out[d] = hi_out;
			out->info.x[d] = (i64)x; out->info.sum[d] = (double)sum; out->info.sumsq[d] = sumsq;
		}
	}
	__syncthreads();
	if (threadIdx.x < 4) {      // MIN_DIR_RATIO (:128-134)
		const int t = (int)threadIdx.x;
		u64 mx = 0;
		for (int k = 0; k < 4; ++k) mx = mx > s_n[k] ? mx : s_n[k];
		int failed = s_failed[t];
		if (!failed && mx < ((u64)1 << 31) && (double)s_n[t] < (int)mx * 0.05) failed = 1;
		out->pes[t].failed = failed;
	}
}
