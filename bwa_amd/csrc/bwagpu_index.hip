// bwagpu_index.hip -- FM-index construction on the device: the BWT/SA half of `bwa index`.
//
// What it replaces in the reference: bwt_bwtgen2 / bwt_pac2bwt (bwtindex.c:64-120, bwt_gen.c: BWT of the forward +
// reverse-complement text by incremental block merging, ~0.5 s/Mbp on one core), bwt_bwtupdate_core (bwtindex.c:150-172:
// interleaving of the Occ checkpoints) and bwt_cal_sa (bwt.c:62-84: the sampled suffix array by an LF walk over the whole
// text).  The outputs are the very arrays those routines leave in bwt_t (bwt.h:48-60), so that bwt_dump_bwt / bwt_dump_sa
// (bwt.c:385-407) -- or our writer -- produce byte-identical .bwt/.sa files (tests/test_index_build.py, -m gpu tests).
//
// Method (not the reference's): the suffix array of T = forward + reverse complement is built outright, in HBM.
//   1. T is packed to 2 bits per base, 32 bases per big-endian u64, so that any 32-mer is two loads and a funnel shift.
//   2. Suffixes are partitioned by their first B bases into 4^B buckets (B chosen so that a bucket is ~10^8 suffixes),
//      and each bucket is radix-sorted (rocPRIM, 64-bit keys) by its next 29 bases + the suffix's valid length (the
//      terminator sorts below A).  After this one pass every suffix whose first B+29 bases are unique -- all but the
//      repeats of the genome -- has its final row.
//   3. The remaining groups are refined by prefix doubling restricted to the unsorted suffixes (Larsson-Sadakane style
//      discarding): a suffix's key is (its group, rank of the suffix h bases further on); one radix sort of the compacted
//      active list per round, h = K, 2K, 4K, ... until no group is left.
//   4. BWT symbols, Occ checkpoints every 128 symbols and the sampled SA are derived from the full SA by streaming kernels.
// Everything is integer work bounded by HBM bandwidth (the sorts) and random 8-byte reads (rank look-ups); no MFMA.
// GRCh38 scale (seq_len 6.2e9): ~110 GB of HBM for SA + rank, which is why this is a 288 GB-per-GPU design.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <hip/hip_runtime.h>
#include <rocprim/functional.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <string>
#include <vector>
#include "../../include/bwagpu.h"

typedef unsigned long long u64;
typedef long long i64;
typedef unsigned int u32;
typedef unsigned char u8;

#define IDX_DEVFN __device__ __forceinline__
#define IDX_BLOCK 256
#define IDX_KEY_BASES 29          // bases of a first-pass sort key (58 bits) + 6 bits of valid length
#define IDX_RANK_BITS 34          // rows < 2^34: l_pac up to 8.5 Gbp

#include "dev_fasta.h"            // FASTA -> .pac / holes (bwagpu_fasta_*)
#include "dev_fastq.h"            // FASTQ windows -> batches (bwagpu_fastq_*)
#include "dev_fasta_reads.h"      // FASTA read windows -> batches (bwagpu_fastq_batch_fasta*)
#include "dev_fastq_smart.h"      // ... classified and split for `mem -p` (bwagpu_fastq_batch_smart*)
#include "dev_bgzf.h"             // BGZF blocks -> text (bwagpu_bgzf_inflate, bwagpu_fastq_batch_bgzf)
#include "dev_bgzf_out.h"         // text -> BGZF blocks (bwagpu_bgzf_deflate)

namespace {

struct Buf {
	void *p = nullptr; size_t cap = 0;
	int ensure(size_t bytes) {
		if (bytes <= cap) return 0;
		release();
		if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) { p = nullptr; return -1; }
		cap = bytes;
		return 0;
	}
	void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
	template <class T> T *as() const { return (T*)p; }
	~Buf() { release(); }
};

// base p of the forward strand from the reference's .pac (bntseq.c:229-230: base l in byte l>>2 at bits (3-(l&3))*2)
IDX_DEVFN int pac_get(const u8 *pac, u64 p) { return pac[p >> 2] >> ((~p & 3) << 1) & 3; }

// 32 bases of T starting at i, first base in the top two bits, 'A' (0) past the end; tw is padded by two zero words
IDX_DEVFN u64 text32(const u64 *tw, u64 i)
{
	const u64 w = i >> 5; const int o = (int)(i & 31) << 1;
	const u64 a = tw[w], b = tw[w + 1];
	return o ? a << o | b >> (64 - o) : a;
}
IDX_DEVFN int text1(const u64 *tw, u64 i) { return (int)(tw[i >> 5] >> ((~i & 31) << 1)) & 3; }

// T = forward strand followed by its reverse complement (bwtindex.c:305-311 / bns_fasta2bntseq with for_only = 0, bntseq.c:299-311)
__global__ void __launch_bounds__(IDX_BLOCK) k_idx_text(const u8 *pac, u64 l_pac, u64 *tw, u64 n_words_pad)
{
	const u64 n = l_pac << 1;
	for (u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x; w < n_words_pad; w += (u64)gridDim.x * blockDim.x) {
		u64 acc = 0;
		for (int j = 0; j < 32; ++j) {
			const u64 p = (w << 5) + (u64)j;
			int c = 0;
			if (p < l_pac) c = pac_get(pac, p);
			else if (p < n) c = 3 - pac_get(pac, n - 1 - p);
			acc = acc << 2 | (u64)c;
		}
		tw[w] = acc;
	}
}

// ---- first pass: buckets by the first B bases ------------------------------------------------------------------------------
__global__ void __launch_bounds__(IDX_BLOCK) k_idx_bucket_count(const u64 *tw, u64 n, int B, u64 *hist)
{
	__shared__ u32 lh[4096];
	const int nb = 1 << (2 * B);
	for (int k = threadIdx.x; k < nb; k += blockDim.x) lh[k] = 0;
	__syncthreads();
	const u64 per_block = (u64)IDX_BLOCK * 64;
	for (u64 base = (u64)blockIdx.x * per_block; base < n; base += (u64)gridDim.x * per_block) {
		for (int k = 0; k < 64; ++k) {
			const u64 i = base + (u64)k * IDX_BLOCK + threadIdx.x;
			if (i < n) atomicAdd(&lh[B ? (u32)(text32(tw, i) >> (64 - 2 * B)) : 0u], 1u);
		}
	}
	__syncthreads();
	for (int k = threadIdx.x; k < nb; k += blockDim.x) if (lh[k]) atomicAdd(&hist[k], (u64)lh[k]);
}

// positions of every bucket, in arbitrary order inside the bucket (the sort that follows orders them), written straight into
// the bucket's row range of the SA: rows[cursor[b] ...)
__global__ void __launch_bounds__(IDX_BLOCK) k_idx_bucket_scatter(const u64 *tw, u64 n, int B, u64 *cursor, u64 *rows)
{
	__shared__ u32 lh[4096];
	__shared__ u64 lbase[4096];
	const int nb = 1 << (2 * B);
	const u64 per_block = (u64)IDX_BLOCK * 16;
	for (u64 base = (u64)blockIdx.x * per_block; base < n; base += (u64)gridDim.x * per_block) {
		for (int k = threadIdx.x; k < nb; k += blockDim.x) lh[k] = 0;
		__syncthreads();
		u32 bk[16], rk[16];
		for (int k = 0; k < 16; ++k) {
			const u64 i = base + (u64)k * IDX_BLOCK + threadIdx.x;
			bk[k] = ~0u; rk[k] = 0;
			if (i < n) { bk[k] = B ? (u32)(text32(tw, i) >> (64 - 2 * B)) : 0u; rk[k] = atomicAdd(&lh[bk[k]], 1u); }
		}
		__syncthreads();
		for (int k = threadIdx.x; k < nb; k += blockDim.x) lbase[k] = lh[k] ? atomicAdd(&cursor[k], (u64)lh[k]) : 0;
		__syncthreads();
		for (int k = 0; k < 16; ++k) {
			const u64 i = base + (u64)k * IDX_BLOCK + threadIdx.x;
			if (bk[k] != ~0u) rows[lbase[bk[k]] + rk[k]] = i;
		}
		__syncthreads();
	}
}

// sort key of suffix i inside its bucket: the 29 bases after the bucket prefix, then the suffix's valid length capped at
// K = B + 29.  Padding bases past the end read as A; among equal padded prefixes the shorter suffix is the smaller one
// (its terminator sorts below A), which is what the length field encodes.  Suffixes with v < K get a unique key.
__global__ void __launch_bounds__(IDX_BLOCK) k_idx_keys(const u64 *tw, u64 n, int B, const u64 *pos, u64 m, u64 *keys)
{
	const u64 K = (u64)B + IDX_KEY_BASES;
	for (u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x; q < m; q += (u64)gridDim.x * blockDim.x) {
		const u64 i = pos[q];
		const u64 v = n - i < K ? n - i : K;
		keys[q] = (text32(tw, i + (u64)B) & ~63ull) | v;
	}
}

// hd[q] = q + 1 at the first element of every run of equal keys, else 0 (an inclusive max-scan turns it into "my run's head + 1")
__global__ void __launch_bounds__(IDX_BLOCK) k_idx_heads(const u64 *keys, u64 m, u64 *hd)
{
	for (u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x; q < m; q += (u64)gridDim.x * blockDim.x)
		hd[q] = (q == 0 || keys[q] != keys[q - 1]) ? q + 1 : 0;
}

// After a bucket's sort: rows and ranks of its suffixes; af[q] = 1 for suffixes whose group has more than one member
__global__ void __launch_bounds__(IDX_BLOCK) k_idx_bucket_finish(const u64 *vals, const u64 *hs, u64 m, u64 row0, u64 *sa, u64 *rank, u64 *af)
{
	for (u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x; q < m; q += (u64)gridDim.x * blockDim.x) {
		const u64 i = vals[q], h = hs[q];
		sa[row0 + q] = i;
		rank[i] = row0 + h - 1;
		const bool head = h == q + 1, next_head = q + 1 == m || hs[q + 1] == q + 2;
		af[q] = (head && next_head) ? 0 : 1;
	}
}

__global__ void __launch_bounds__(IDX_BLOCK) k_idx_bucket_compact(const u64 *vals, const u64 *hs, const u64 *af, const u64 *pos, u64 m, u64 row0,
																  u64 *act_i, u64 *act_head, u64 out0)
{
	for (u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x; q < m; q += (u64)gridDim.x * blockDim.x)
		if (af[q]) { act_i[out0 + pos[q]] = vals[q]; act_head[out0 + pos[q]] = row0 + hs[q] - 1; }
}

// ---- prefix doubling over the unsorted suffixes ---------------------------------------------------------------------------
// active list -> group numbers: gf[a] = 1 where a new group starts
__global__ void __launch_bounds__(IDX_BLOCK) k_idx_group_flags(const u64 *act_head, u64 A, u64 *gf)
{
	for (u64 a = (u64)blockIdx.x * blockDim.x + threadIdx.x; a < A; a += (u64)gridDim.x * blockDim.x)
		gf[a] = (a == 0 || act_head[a] != act_head[a - 1]) ? 1 : 0;
}
__global__ void __launch_bounds__(IDX_BLOCK) k_idx_group_init(const u64 *act_head, const u64 *gsum, u64 A, u64 *gid, u64 *ghead, u64 *gstart)
{
	for (u64 a = (u64)blockIdx.x * blockDim.x + threadIdx.x; a < A; a += (u64)gridDim.x * blockDim.x) {
		const u64 g = gsum[a] - 1;
		gid[a] = g;
		if (a == 0 || act_head[a] != act_head[a - 1]) { ghead[g] = act_head[a]; gstart[g] = a; }
	}
}

// key of one active suffix in the round with step h: (group, rank of the suffix h bases on); the terminator's rank is 0
__global__ void __launch_bounds__(IDX_BLOCK) k_idx_round_keys(const u64 *act_i, const u64 *gid, const u64 *rank, u64 A, u64 n, u64 h, u64 *keys)
{
	for (u64 a = (u64)blockIdx.x * blockDim.x + threadIdx.x; a < A; a += (u64)gridDim.x * blockDim.x) {
		const u64 j = act_i[a] + h;
		keys[a] = gid[a] << IDX_RANK_BITS | (j < n ? rank[j] : 0ull);
	}
}
// fallback when the group number does not fit beside the rank: two stable sorts, by rank first, then by group
__global__ void __launch_bounds__(IDX_BLOCK) k_idx_round_rank_keys(const u64 *act_i, const u64 *rank, u64 A, u64 n, u64 h, u64 *keys)
{
	for (u64 a = (u64)blockIdx.x * blockDim.x + threadIdx.x; a < A; a += (u64)gridDim.x * blockDim.x) {
		const u64 j = act_i[a] + h;
		keys[a] = j < n ? rank[j] : 0ull;
	}
}

// After the round's sort (elements of one group are still contiguous and in the group's old slot range):
//   sf[a] - 1 = index of the first element with the same (group, rank) -> the element's new group head
// writes the new rows and ranks, and flags survivors (members of groups that still have > 1 element) and new group heads.
// `split` form (two-sort fallback): k2 holds the rank keys, gsorted the group numbers; otherwise the group is keys >> 34.
__global__ void __launch_bounds__(IDX_BLOCK) k_idx_round_flags(const u64 *keys, const u64 *gsorted, u64 A, u64 *fk)
{
	for (u64 a = (u64)blockIdx.x * blockDim.x + threadIdx.x; a < A; a += (u64)gridDim.x * blockDim.x) {
		bool head = a == 0 || keys[a] != keys[a - 1];
		if (gsorted && !head) head = gsorted[a] != gsorted[a - 1];
		fk[a] = head ? a + 1 : 0;
	}
}
__global__ void __launch_bounds__(IDX_BLOCK) k_idx_round_apply(const u64 *keys, const u64 *gsorted, const u64 *vals, const u64 *sf, u64 A, const u64 *ghead, const u64 *gstart,
															   u64 *sa, u64 *rank, u64 *surv, u64 *nhead)
{
	for (u64 a = (u64)blockIdx.x * blockDim.x + threadIdx.x; a < A; a += (u64)gridDim.x * blockDim.x) {
		const u64 g = gsorted ? gsorted[a] : keys[a] >> IDX_RANK_BITS;
		const u64 r0 = ghead[g], a0 = gstart[g], i = vals[a];
		sa[r0 + (a - a0)] = i;
		rank[i] = r0 + (sf[a] - 1 - a0);
		const bool head = sf[a] == a + 1, next_head = a + 1 == A || sf[a + 1] == a + 2;
		const u64 s = (head && next_head) ? 0 : 1;
		surv[a] = s; nhead[a] = (s && head) ? 1 : 0;
	}
}
__global__ void __launch_bounds__(IDX_BLOCK) k_idx_round_compact(const u64 *keys, const u64 *gsorted, const u64 *vals, const u64 *sf, const u64 *surv, const u64 *pos, const u64 *ngsum, u64 A,
																 const u64 *ghead, const u64 *gstart, u64 *act_i2, u64 *gid2, u64 *ghead2, u64 *gstart2)
{
	for (u64 a = (u64)blockIdx.x * blockDim.x + threadIdx.x; a < A; a += (u64)gridDim.x * blockDim.x) {
		if (!surv[a]) continue;
		const u64 np = pos[a], ng = ngsum[a] - 1;
		act_i2[np] = vals[a]; gid2[np] = ng;
		if (sf[a] == a + 1) {
			const u64 g = gsorted ? gsorted[a] : keys[a] >> IDX_RANK_BITS;
			ghead2[ng] = ghead[g] + (a - gstart[g]); gstart2[ng] = np;
		}
	}
}

__global__ void __launch_bounds__(IDX_BLOCK) k_idx_iota(u64 *out, u64 A)
{
	for (u64 a = (u64)blockIdx.x * blockDim.x + threadIdx.x; a < A; a += (u64)gridDim.x * blockDim.x) out[a] = a;
}
__global__ void __launch_bounds__(IDX_BLOCK) k_idx_gather(const u64 *src, const u64 *idx, u64 A, u64 *out)
{
	for (u64 a = (u64)blockIdx.x * blockDim.x + threadIdx.x; a < A; a += (u64)gridDim.x * blockDim.x) out[a] = src[idx[a]];
}

// ---- BWT, Occ checkpoints, sampled SA (bwtindex.c:150-172, bwt.c:62-84) --------------------------------------------------------
__global__ void __launch_bounds__(IDX_BLOCK) k_idx_find_primary(const u64 *sa, u64 n_rows, u64 *primary)
{
	for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (u64)gridDim.x * blockDim.x)
		if (sa[r] == 0) *primary = r;
}
// word wi of the $-less BWT string: symbols x = 16 wi .. 16 wi + 15, symbol x = T[SA[row] - 1] with row = x + (x >= primary);
// symbol j of a word sits at bits (15 - j) * 2 (bwt.h:74-80)
__global__ void __launch_bounds__(IDX_BLOCK) k_idx_bwt_words(const u64 *sa, const u64 *tw, u64 n, u64 primary, u32 *words, u64 n_words_pad)
{
	for (u64 wi = (u64)blockIdx.x * blockDim.x + threadIdx.x; wi < n_words_pad; wi += (u64)gridDim.x * blockDim.x) {
		u32 acc = 0;
		for (int j = 0; j < 16; ++j) {
			const u64 x = (wi << 4) + (u64)j;
			u32 c = 0;
			if (x < n) { const u64 row = x + (x >= primary ? 1 : 0); c = (u32)text1(tw, sa[row] - 1); }
			acc = acc << 2 | c;
		}
		words[wi] = acc;
	}
}
// per 128-symbol block: number of A, C, G, T (the last block counts only the symbols that exist)
__global__ void __launch_bounds__(IDX_BLOCK) k_idx_block_counts(const u32 *words, u64 n, u64 n_blk, u64 *c0, u64 *c1, u64 *c2, u64 *c3)
{
	for (u64 b = (u64)blockIdx.x * blockDim.x + threadIdx.x; b < n_blk; b += (u64)gridDim.x * blockDim.x) {
		u32 k1 = 0, k2 = 0, k3 = 0;
		for (int k = 0; k < 8; ++k) {
			const u32 w = words[b * 8 + k], lo = w & 0x55555555u, hi = (w >> 1) & 0x55555555u;
			k3 += __popc(hi & lo); k2 += __popc(hi & ~lo); k1 += __popc(lo & ~hi);
		}
		const u64 len = n - b * 128 < 128 ? n - b * 128 : 128;      // padding symbols are 0 and were never counted as 1..3
		c0[b] = len - k1 - k2 - k3; c1[b] = k1; c2[b] = k2; c3[b] = k3;
	}
}
// the reference's interleaved layout: per block 4 x u64 counts before the block + 8 x u32 symbols; one trailing counts record
__global__ void __launch_bounds__(IDX_BLOCK) k_idx_interleave(const u32 *words, const u64 *o0, const u64 *o1, const u64 *o2, const u64 *o3, u64 n_blk, u32 *out)
{
	for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < n_blk * 16; t += (u64)gridDim.x * blockDim.x) {
		const u64 b = t >> 4; const int k = (int)(t & 15);
		u32 v;
		if (k < 8) { const u64 c = (k >> 1) == 0 ? o0[b] : (k >> 1) == 1 ? o1[b] : (k >> 1) == 2 ? o2[b] : o3[b]; v = (k & 1) ? (u32)(c >> 32) : (u32)c; }
		else v = words[b * 8 + (k - 8)];
		out[t] = v;
	}
}
__global__ void __launch_bounds__(IDX_BLOCK) k_idx_sample_sa(const u64 *sa, u64 n_sa, int intv, u64 *out)
{
	for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n_sa; j += (u64)gridDim.x * blockDim.x)
		out[j] = j == 0 ? ~0ull : sa[j * (u64)intv];          // bwt_cal_sa leaves sa[0] = -1 (bwt.c:79)
}

static unsigned grid_for(u64 items, u64 per_thread = 1)
{
	u64 b = (items + (u64)IDX_BLOCK * per_thread - 1) / ((u64)IDX_BLOCK * per_thread);
	if (b < 1) b = 1;
	if (b > 65536) b = 65536;
	return (unsigned)b;
}

struct Builder {
	hipStream_t st = nullptr;
	std::string err;
	Buf tmp;   // rocPRIM temporary storage
	int verbose = 0;

	int fail(const char *what, hipError_t e) { err = std::string(what) + ": " + hipGetErrorString(e); return BWAGPU_EHIP; }
	int sort_pairs(u64 *k_in, u64 *k_out, u64 *v_in, u64 *v_out, u64 m, int begin_bit, int end_bit)
	{
		size_t bytes = 0;
		hipError_t e = rocprim::radix_sort_pairs(nullptr, bytes, k_in, k_out, v_in, v_out, (size_t)m, (unsigned)begin_bit, (unsigned)end_bit, st);
		if (e != hipSuccess) return fail("radix_sort_pairs(size)", e);
		if (tmp.ensure(bytes)) { err = "hipMalloc failed (sort scratch)"; return BWAGPU_ENOMEM; }
		e = rocprim::radix_sort_pairs(tmp.p, bytes, k_in, k_out, v_in, v_out, (size_t)m, (unsigned)begin_bit, (unsigned)end_bit, st);
		if (e != hipSuccess) return fail("radix_sort_pairs", e);
		return 0;
	}
	int scan_max(u64 *in, u64 *out, u64 m)
	{
		size_t bytes = 0;
		hipError_t e = rocprim::inclusive_scan(nullptr, bytes, in, out, (size_t)m, rocprim::maximum<u64>(), st);
		if (e != hipSuccess) return fail("inclusive_scan(size)", e);
		if (tmp.ensure(bytes)) { err = "hipMalloc failed (scan scratch)"; return BWAGPU_ENOMEM; }
		e = rocprim::inclusive_scan(tmp.p, bytes, in, out, (size_t)m, rocprim::maximum<u64>(), st);
		return e == hipSuccess ? 0 : fail("inclusive_scan", e);
	}
	int scan_sum_incl(u64 *in, u64 *out, u64 m)
	{
		size_t bytes = 0;
		hipError_t e = rocprim::inclusive_scan(nullptr, bytes, in, out, (size_t)m, rocprim::plus<u64>(), st);
		if (e != hipSuccess) return fail("inclusive_scan(size)", e);
		if (tmp.ensure(bytes)) { err = "hipMalloc failed (scan scratch)"; return BWAGPU_ENOMEM; }
		e = rocprim::inclusive_scan(tmp.p, bytes, in, out, (size_t)m, rocprim::plus<u64>(), st);
		return e == hipSuccess ? 0 : fail("inclusive_scan", e);
	}
	int scan_sum_excl(u64 *in, u64 *out, u64 m)
	{
		size_t bytes = 0;
		hipError_t e = rocprim::exclusive_scan(nullptr, bytes, in, out, (u64)0, (size_t)m, rocprim::plus<u64>(), st);
		if (e != hipSuccess) return fail("exclusive_scan(size)", e);
		if (tmp.ensure(bytes)) { err = "hipMalloc failed (scan scratch)"; return BWAGPU_ENOMEM; }
		e = rocprim::exclusive_scan(tmp.p, bytes, in, out, (u64)0, (size_t)m, rocprim::plus<u64>(), st);
		return e == hipSuccess ? 0 : fail("exclusive_scan", e);
	}
	// enlarge a device array that already holds `used` bytes (geometric growth, contents kept)
	int grow(Buf &b, size_t need, size_t used)
	{
		if (need <= b.cap) return 0;
		size_t want = need + need / 2 + 4096;
		void *np = nullptr;
		if (hipMalloc(&np, want) != hipSuccess) {
			want = need;
			if (hipMalloc(&np, want) != hipSuccess) { err = "hipMalloc failed (list of unsorted suffixes)"; return BWAGPU_ENOMEM; }
		}
		if (used) { hipError_t e = hipMemcpyAsync(np, b.p, used, hipMemcpyDeviceToDevice, st); if (e == hipSuccess) e = hipStreamSynchronize(st); if (e != hipSuccess) { (void)hipFree(np); return fail("grow", e); } }
		b.release(); b.p = np; b.cap = want;
		return 0;
	}
	// last element of an exclusive scan + its input = total
	int total_of(const u64 *excl, const u64 *in, u64 m, u64 *out)
	{
		u64 a = 0, b = 0;
		if (m) {
			hipError_t e = hipMemcpyAsync(&a, excl + (m - 1), 8, hipMemcpyDeviceToHost, st);
			if (e == hipSuccess) e = hipMemcpyAsync(&b, in + (m - 1), 8, hipMemcpyDeviceToHost, st);
			if (e == hipSuccess) e = hipStreamSynchronize(st);
			if (e != hipSuccess) return fail("read back scan total", e);
		}
		*out = a + b;
		return 0;
	}
};

static int bits_for(u64 v) { int b = 0; while (b < 64 && (v >> b)) ++b; return b; }

#define IDXCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { rc = bl.fail(#call, e_); goto done; } } while (0)
#define IDXRC(call) do { rc = (call); if (rc) goto done; } while (0)

}  // namespace

extern "C" void bwagpu_built_free(bwagpu_built_t *b)
{
	if (!b) return;
	free(b->bwt); free(b->sa);
	b->bwt = nullptr; b->sa = nullptr;
}

extern "C" int bwagpu_index_build(const uint8_t *pac, int64_t l_pac_, int sa_intv, int device, bwagpu_built_t *out, char *errbuf, size_t errlen)
{
	if (errbuf && errlen) errbuf[0] = 0;
	if (!pac || !out || l_pac_ <= 0 || sa_intv <= 0 || (sa_intv & (sa_intv - 1))) return BWAGPU_EINVAL;
	if ((u64)l_pac_ >= (1ull << (IDX_RANK_BITS - 1)) - 64) return BWAGPU_EUNSUP;
	memset(out, 0, sizeof *out);
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return BWAGPU_ENODEV;
	if (hipSetDevice(device) != hipSuccess) return BWAGPU_ENODEV;
	Builder bl;
	bl.verbose = getenv("BWAGPU_INDEX_VERBOSE") ? atoi(getenv("BWAGPU_INDEX_VERBOSE")) : 0;
	if (hipStreamCreate(&bl.st) != hipSuccess) return BWAGPU_ENODEV;
	int rc = 0;
	const u64 l_pac = (u64)l_pac_, n = l_pac << 1, n_rows = n + 1;
	const u64 n_tw = (n + 31) / 32 + 3;                   // + padding words so that text32 may read past the end
	// bucket prefix: ~2^27 suffixes per bucket (the sort's throughput is flat from ~10^7 elements; its buffers stay small)
	int B = 0;
	if (getenv("BWAGPU_INDEX_BUCKET_BASES")) B = atoi(getenv("BWAGPU_INDEX_BUCKET_BASES"));   // test hook
	else while (B < 6 && (n >> (2 * B)) > (1ull << 27)) ++B;
	if (B < 0) B = 0; if (B > 6) B = 6;
	const int n_bk = 1 << (2 * B);
	const u64 K = (u64)B + IDX_KEY_BASES;
	Buf d_pac, d_tw, d_sa, d_rank, d_hist, d_cursor, d_keys, d_keys2, d_vals2, d_s1, d_s2, d_s3, d_s4;
	Buf d_act_i, d_act_i2, d_gid, d_gid2, d_ghead, d_ghead2, d_gstart, d_gstart2, d_scalar;
	Buf d_words, d_c[4], d_o[4], d_out, d_sas, d_x1, d_x2, d_x3;
	std::vector<u64> hist((size_t)n_bk), base((size_t)n_bk + 1, 0);
	u64 max_bucket = 0, A = 0, primary = 0, n_groups = 0;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	(void)hipEventCreate(&ev0); (void)hipEventCreate(&ev1);
	(void)hipEventRecord(ev0, bl.st);

	if (d_pac.ensure((size_t)(l_pac / 4 + 1)) || d_tw.ensure(n_tw * 8) || d_sa.ensure(n_rows * 8) || d_rank.ensure(n_rows * 8) ||
		d_hist.ensure((size_t)n_bk * 8) || d_cursor.ensure((size_t)n_bk * 8) || d_scalar.ensure(64)) { bl.err = "hipMalloc failed (suffix array)"; rc = BWAGPU_ENOMEM; goto done; }
	IDXCHK(hipMemcpyAsync(d_pac.p, pac, (size_t)(l_pac / 4 + 1), hipMemcpyHostToDevice, bl.st));
	hipLaunchKernelGGL(k_idx_text, dim3(grid_for(n_tw)), dim3(IDX_BLOCK), 0, bl.st, d_pac.as<u8>(), l_pac, d_tw.as<u64>(), n_tw);
	IDXCHK(hipMemsetAsync(d_hist.p, 0, (size_t)n_bk * 8, bl.st));
	hipLaunchKernelGGL(k_idx_bucket_count, dim3(grid_for(n, 64)), dim3(IDX_BLOCK), 0, bl.st, d_tw.as<u64>(), n, B, d_hist.as<u64>());
	IDXCHK(hipMemcpyAsync(hist.data(), d_hist.p, (size_t)n_bk * 8, hipMemcpyDeviceToHost, bl.st));
	IDXCHK(hipStreamSynchronize(bl.st));
	for (int b = 0; b < n_bk; ++b) { base[b + 1] = base[b] + hist[b]; if (hist[b] > max_bucket) max_bucket = hist[b]; }
	if (base[n_bk] != n) { bl.err = "internal: bucket histogram does not add up"; rc = BWAGPU_EHIP; goto done; }
	{	// rows: row 0 is the terminator's suffix; bucket b owns rows [1 + base[b], 1 + base[b+1])
		std::vector<u64> cur((size_t)n_bk);
		for (int b = 0; b < n_bk; ++b) cur[b] = 1 + base[b];
		IDXCHK(hipMemcpyAsync(d_cursor.p, cur.data(), (size_t)n_bk * 8, hipMemcpyHostToDevice, bl.st));
		IDXCHK(hipStreamSynchronize(bl.st));
		hipLaunchKernelGGL(k_idx_bucket_scatter, dim3(grid_for(n, 16)), dim3(IDX_BLOCK), 0, bl.st, d_tw.as<u64>(), n, B, d_cursor.as<u64>(), d_sa.as<u64>());
		const u64 row0v[2] = { n, 0 };                       // SA[0] = n (the empty suffix); rank[n] = 0
		IDXCHK(hipMemcpyAsync(d_sa.p, &row0v[0], 8, hipMemcpyHostToDevice, bl.st));
		IDXCHK(hipMemcpyAsync(d_rank.as<u64>() + n, &row0v[1], 8, hipMemcpyHostToDevice, bl.st));
		IDXCHK(hipStreamSynchronize(bl.st));
	}
	if (d_keys.ensure(max_bucket * 8) || d_keys2.ensure(max_bucket * 8) || d_vals2.ensure(max_bucket * 8) || d_s1.ensure(max_bucket * 8) ||
		d_s2.ensure(max_bucket * 8) || d_s3.ensure(max_bucket * 8)) { bl.err = "hipMalloc failed (bucket sort buffers)"; rc = BWAGPU_ENOMEM; goto done; }
	for (int b = 0; b < n_bk; ++b) {
		const u64 m = hist[b], row0 = 1 + base[b];
		if (m == 0) continue;
		u64 *rows = d_sa.as<u64>() + row0;
		hipLaunchKernelGGL(k_idx_keys, dim3(grid_for(m)), dim3(IDX_BLOCK), 0, bl.st, d_tw.as<u64>(), n, B, rows, m, d_keys.as<u64>());
		IDXRC(bl.sort_pairs(d_keys.as<u64>(), d_keys2.as<u64>(), rows, d_vals2.as<u64>(), m, 0, 64));
		hipLaunchKernelGGL(k_idx_heads, dim3(grid_for(m)), dim3(IDX_BLOCK), 0, bl.st, d_keys2.as<u64>(), m, d_s1.as<u64>());
		IDXRC(bl.scan_max(d_s1.as<u64>(), d_s2.as<u64>(), m));                                          // s2 = hs
		hipLaunchKernelGGL(k_idx_bucket_finish, dim3(grid_for(m)), dim3(IDX_BLOCK), 0, bl.st, d_vals2.as<u64>(), d_s2.as<u64>(), m, row0, d_sa.as<u64>(), d_rank.as<u64>(), d_s3.as<u64>());
		IDXRC(bl.scan_sum_excl(d_s3.as<u64>(), d_s1.as<u64>(), m));                                     // s1 = position among the bucket's unsorted suffixes
		u64 na = 0;
		IDXRC(bl.total_of(d_s1.as<u64>(), d_s3.as<u64>(), m, &na));
		if (na == 0) continue;
		// the list of unsorted suffixes grows bucket by bucket (its final size is only known at the end)
		IDXRC(bl.grow(d_act_i, (A + na) * 8, A * 8)); IDXRC(bl.grow(d_s4, (A + na) * 8, A * 8));
		hipLaunchKernelGGL(k_idx_bucket_compact, dim3(grid_for(m)), dim3(IDX_BLOCK), 0, bl.st, d_vals2.as<u64>(), d_s2.as<u64>(), d_s3.as<u64>(), d_s1.as<u64>(), m, row0,
						   d_act_i.as<u64>(), d_s4.as<u64>(), A);
		A += na;
	}
	if (bl.verbose) fprintf(stderr, "[bwagpu_index] n=%llu B=%d buckets=%d max_bucket=%llu: %llu suffixes (%.2f%%) unsorted after %llu bases\n",
							n, B, n_bk, max_bucket, A, 100.0 * A / n, K);
	IDXCHK(hipStreamSynchronize(bl.st));
	d_keys.release(); d_keys2.release(); d_vals2.release(); d_s1.release(); d_s2.release(); d_s3.release();
	if (A) {
		// group numbers of the active list (d_s4 = head row of every active suffix, non-decreasing)
		if (d_keys.ensure(A * 8) || d_keys2.ensure(A * 8) || d_vals2.ensure(A * 8) || d_s1.ensure(A * 8) || d_s2.ensure(A * 8) || d_s3.ensure(A * 8) ||
			d_act_i2.ensure(A * 8) || d_gid.ensure(A * 8) || d_gid2.ensure(A * 8) || d_ghead.ensure((A / 2 + 1) * 8) || d_ghead2.ensure((A / 2 + 1) * 8) ||
			d_gstart.ensure((A / 2 + 1) * 8) || d_gstart2.ensure((A / 2 + 1) * 8)) { bl.err = "hipMalloc failed (prefix-doubling buffers)"; rc = BWAGPU_ENOMEM; goto done; }
		hipLaunchKernelGGL(k_idx_group_flags, dim3(grid_for(A)), dim3(IDX_BLOCK), 0, bl.st, d_s4.as<u64>(), A, d_s1.as<u64>());
		IDXRC(bl.scan_sum_incl(d_s1.as<u64>(), d_s2.as<u64>(), A));
		hipLaunchKernelGGL(k_idx_group_init, dim3(grid_for(A)), dim3(IDX_BLOCK), 0, bl.st, d_s4.as<u64>(), d_s2.as<u64>(), A, d_gid.as<u64>(), d_ghead.as<u64>(), d_gstart.as<u64>());
		IDXCHK(hipMemcpyAsync(&n_groups, d_s2.as<u64>() + (A - 1), 8, hipMemcpyDeviceToHost, bl.st));
		IDXCHK(hipStreamSynchronize(bl.st));
		u64 *act_i = d_act_i.as<u64>(), *act_i2 = d_act_i2.as<u64>(), *gid = d_gid.as<u64>(), *gid2 = d_gid2.as<u64>();
		u64 *ghead = d_ghead.as<u64>(), *ghead2 = d_ghead2.as<u64>(), *gstart = d_gstart.as<u64>(), *gstart2 = d_gstart2.as<u64>();
		int round = 0;
		for (u64 h = K; A > 0; h <<= 1, ++round) {
			if (h >= (n << 1)) { bl.err = "internal: prefix doubling did not terminate"; rc = BWAGPU_EHIP; goto done; }
			const int gbits = bits_for(n_groups ? n_groups - 1 : 0);
			const u64 *gsorted = nullptr;
			if (gbits + IDX_RANK_BITS <= 64 && !getenv("BWAGPU_INDEX_SPLIT_SORT")) {
				hipLaunchKernelGGL(k_idx_round_keys, dim3(grid_for(A)), dim3(IDX_BLOCK), 0, bl.st, act_i, gid, d_rank.as<u64>(), A, n, h, d_keys.as<u64>());
				IDXRC(bl.sort_pairs(d_keys.as<u64>(), d_keys2.as<u64>(), act_i, d_vals2.as<u64>(), A, 0, IDX_RANK_BITS + (gbits ? gbits : 1)));
			} else {
				// group number and rank do not fit one 64-bit key (> 2^30 groups): order the active indices by rank, then stably by
				// group, and gather suffixes, ranks and groups through the resulting permutation
				if (d_x1.ensure(A * 8) || d_x2.ensure(A * 8) || d_x3.ensure(A * 8)) { bl.err = "hipMalloc failed (split sort)"; rc = BWAGPU_ENOMEM; goto done; }
				hipLaunchKernelGGL(k_idx_round_rank_keys, dim3(grid_for(A)), dim3(IDX_BLOCK), 0, bl.st, act_i, d_rank.as<u64>(), A, n, h, d_keys.as<u64>());   // keys = rank
				hipLaunchKernelGGL(k_idx_iota, dim3(grid_for(A)), dim3(IDX_BLOCK), 0, bl.st, d_x1.as<u64>(), A);
				IDXRC(bl.sort_pairs(d_keys.as<u64>(), d_keys2.as<u64>(), d_x1.as<u64>(), d_x2.as<u64>(), A, 0, IDX_RANK_BITS));                   // x2 = indices by rank
				hipLaunchKernelGGL(k_idx_gather, dim3(grid_for(A)), dim3(IDX_BLOCK), 0, bl.st, gid, d_x2.as<u64>(), A, d_x1.as<u64>());             // x1 = their groups
				IDXRC(bl.sort_pairs(d_x1.as<u64>(), d_x3.as<u64>(), d_x2.as<u64>(), d_vals2.as<u64>(), A, 0, gbits ? gbits : 1));                  // x3 = groups sorted, vals2 = permutation
				hipLaunchKernelGGL(k_idx_gather, dim3(grid_for(A)), dim3(IDX_BLOCK), 0, bl.st, d_keys.as<u64>(), d_vals2.as<u64>(), A, d_keys2.as<u64>());   // keys2 = ranks in (group, rank) order
				hipLaunchKernelGGL(k_idx_gather, dim3(grid_for(A)), dim3(IDX_BLOCK), 0, bl.st, act_i, d_vals2.as<u64>(), A, d_x1.as<u64>());
				IDXCHK(hipMemcpyAsync(d_vals2.p, d_x1.p, A * 8, hipMemcpyDeviceToDevice, bl.st));                                                   // vals2 = suffixes in that order
				gsorted = d_x3.as<u64>();
			}
			hipLaunchKernelGGL(k_idx_round_flags, dim3(grid_for(A)), dim3(IDX_BLOCK), 0, bl.st, d_keys2.as<u64>(), gsorted, A, d_s1.as<u64>());
			IDXRC(bl.scan_max(d_s1.as<u64>(), d_s2.as<u64>(), A));                                       // s2 = sf
			hipLaunchKernelGGL(k_idx_round_apply, dim3(grid_for(A)), dim3(IDX_BLOCK), 0, bl.st, d_keys2.as<u64>(), gsorted, d_vals2.as<u64>(), d_s2.as<u64>(), A, ghead, gstart,
							   d_sa.as<u64>(), d_rank.as<u64>(), d_s1.as<u64>(), d_s3.as<u64>());          // s1 = surv, s3 = new heads
			IDXRC(bl.scan_sum_excl(d_s1.as<u64>(), d_keys.as<u64>(), A));                                // keys = pos
			u64 A2 = 0, G2 = 0;
			IDXRC(bl.total_of(d_keys.as<u64>(), d_s1.as<u64>(), A, &A2));
			if (A2) {
				IDXRC(bl.scan_sum_incl(d_s3.as<u64>(), d_s4.as<u64>(), A));                              // s4 = running count of new heads
				IDXCHK(hipMemcpyAsync(&G2, d_s4.as<u64>() + (A - 1), 8, hipMemcpyDeviceToHost, bl.st));
				IDXCHK(hipStreamSynchronize(bl.st));
				hipLaunchKernelGGL(k_idx_round_compact, dim3(grid_for(A)), dim3(IDX_BLOCK), 0, bl.st, d_keys2.as<u64>(), gsorted, d_vals2.as<u64>(), d_s2.as<u64>(), d_s1.as<u64>(),
								   d_keys.as<u64>(), d_s4.as<u64>(), A, ghead, gstart, act_i2, gid2, ghead2, gstart2);
				{ u64 *t = gid; gid = gid2; gid2 = t; }
				{ u64 *t = act_i; act_i = act_i2; act_i2 = t; }
				{ u64 *t = ghead; ghead = ghead2; ghead2 = t; }
				{ u64 *t = gstart; gstart = gstart2; gstart2 = t; }
			}
			if (bl.verbose) fprintf(stderr, "[bwagpu_index] round %d (h=%llu): %llu -> %llu unsorted suffixes in %llu groups\n", round, h, A, A2, G2);
			A = A2; n_groups = G2;
		}
	}
	IDXCHK(hipStreamSynchronize(bl.st));
	d_rank.release(); d_keys.release(); d_keys2.release(); d_vals2.release(); d_s1.release(); d_s2.release(); d_s3.release(); d_s4.release();
	d_act_i.release(); d_act_i2.release(); d_gid.release(); d_gid2.release(); d_ghead.release(); d_ghead2.release(); d_gstart.release(); d_gstart2.release(); d_x1.release(); d_x2.release(); d_x3.release();
	{	// ---- BWT + Occ checkpoints in the reference's layout, sampled SA --------------------------------------------------------
		const u64 n_blk = (n + 127) / 128, n_words = (n + 15) / 16;
		const u64 bwt_size = n_words + (n_blk + 1) * 8;                // bwtindex.c:154-156
		const u64 n_sa = (n + (u64)sa_intv) / (u64)sa_intv;             // bwt.c:70
		hipLaunchKernelGGL(k_idx_find_primary, dim3(grid_for(n_rows)), dim3(IDX_BLOCK), 0, bl.st, d_sa.as<u64>(), n_rows, d_scalar.as<u64>());
		IDXCHK(hipMemcpyAsync(&primary, d_scalar.p, 8, hipMemcpyDeviceToHost, bl.st));
		IDXCHK(hipStreamSynchronize(bl.st));
		if (d_words.ensure(n_blk * 8 * 4) || d_out.ensure((n_blk + 1) * 16 * 4) || d_sas.ensure(n_sa * 8)) { bl.err = "hipMalloc failed (bwt)"; rc = BWAGPU_ENOMEM; goto done; }
		for (int c = 0; c < 4; ++c) if (d_c[c].ensure(n_blk * 8) || d_o[c].ensure(n_blk * 8)) { bl.err = "hipMalloc failed (occ)"; rc = BWAGPU_ENOMEM; goto done; }
		hipLaunchKernelGGL(k_idx_bwt_words, dim3(grid_for(n_blk * 8)), dim3(IDX_BLOCK), 0, bl.st, d_sa.as<u64>(), d_tw.as<u64>(), n, primary, d_words.as<u32>(), n_blk * 8);
		hipLaunchKernelGGL(k_idx_block_counts, dim3(grid_for(n_blk)), dim3(IDX_BLOCK), 0, bl.st, d_words.as<u32>(), n, n_blk, d_c[0].as<u64>(), d_c[1].as<u64>(), d_c[2].as<u64>(), d_c[3].as<u64>());
		u64 tot[4];
		for (int c = 0; c < 4; ++c) {
			IDXRC(bl.scan_sum_excl(d_c[c].as<u64>(), d_o[c].as<u64>(), n_blk));
			IDXRC(bl.total_of(d_o[c].as<u64>(), d_c[c].as<u64>(), n_blk, &tot[c]));
		}
		if (tot[0] + tot[1] + tot[2] + tot[3] != n) { bl.err = "internal: BWT symbol counts do not add up"; rc = BWAGPU_EHIP; goto done; }
		hipLaunchKernelGGL(k_idx_interleave, dim3(grid_for(n_blk * 16)), dim3(IDX_BLOCK), 0, bl.st, d_words.as<u32>(), d_o[0].as<u64>(), d_o[1].as<u64>(), d_o[2].as<u64>(), d_o[3].as<u64>(),
						   n_blk, d_out.as<u32>());
		hipLaunchKernelGGL(k_idx_sample_sa, dim3(grid_for(n_sa)), dim3(IDX_BLOCK), 0, bl.st, d_sa.as<u64>(), n_sa, sa_intv, d_sas.as<u64>());
		out->bwt = (uint32_t*)malloc((size_t)bwt_size * 4);
		out->sa = (uint64_t*)malloc((size_t)n_sa * 8);
		if (!out->bwt || !out->sa) { bl.err = "malloc failed (host copies of the index)"; rc = BWAGPU_ENOMEM; goto done; }
		// the last block keeps only the words that exist; the trailing record holds the totals (bwtindex.c:158-169)
		const u64 body_words = n_blk * 16 - (n_blk * 8 - n_words);
		IDXCHK(hipMemcpyAsync(out->bwt, d_out.p, (size_t)body_words * 4, hipMemcpyDeviceToHost, bl.st));
		IDXCHK(hipMemcpyAsync(out->sa, d_sas.p, (size_t)n_sa * 8, hipMemcpyDeviceToHost, bl.st));
		IDXCHK(hipStreamSynchronize(bl.st));
		memcpy(out->bwt + body_words, tot, 32);
		out->bwt_size = bwt_size; out->n_sa = n_sa; out->sa_intv = sa_intv; out->primary = primary; out->seq_len = n;
		out->L2[0] = 0; for (int c = 0; c < 4; ++c) out->L2[c + 1] = out->L2[c] + tot[c];
	}
	(void)hipEventRecord(ev1, bl.st); (void)hipEventSynchronize(ev1);
	{ float ms = 0; if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) out->build_ms = ms; }
done:
	if (rc) { bwagpu_built_free(out); if (errbuf && errlen) snprintf(errbuf, errlen, "%s", bl.err.c_str()); }
	if (ev0) (void)hipEventDestroy(ev0);
	if (ev1) (void)hipEventDestroy(ev1);
	(void)hipStreamDestroy(bl.st);
	return rc;
}

// ---- FASTA -> .pac / .ann / .amb (bns_fasta2bntseq, bntseq.c:280-333) ----------------------------------------------------------
// The device walks the bytes (dev_fasta.h); the host strips the bytes before the first record, parses the header lines whose
// positions the device reports, keeps the carry between chunks, and gathers the .pac bytes and the hole list.
struct bwagpu_fasta_parser_s {
	struct Contig { std::string name, anno; u64 offset; };
	hipStream_t st = nullptr;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	size_t chunk = 0;
	u8 *stage = nullptr; size_t n_stage = 0;     // page-locked: chunk + 1 bytes (a held-back '\r' and a full chunk)
	u64 stage_pos = 0;                           // stream offset of stage[0]
	bool started = false;                        // the first '>' has been seen
	u64 skipped = 0;                             // bytes before it
	FaSum carry;
	bool ls = true;                              // the next byte starts a line
	bool in_hdr = false; std::string hdr;        // a header line still open at the end of the last chunk, its text so far
	std::vector<Contig> contigs;
	std::vector<u64> hole_off, hole_end; std::vector<char> hole_chr;
	u8 *pac = nullptr; size_t pac_cap = 0;
	Buf d_buf, d_tsum, d_tscan, d_codes, d_pac, d_hoff, d_hchr, d_hend, d_hpos, d_hdoff, d_err, d_jump, d_tmp;
	std::vector<u8> h_pac, h_hchr; std::vector<u64> h_hoff, h_hend, h_hpos, h_hdoff;
	float parse_ms = 0;
	int rc = 0; std::string err;

	~bwagpu_fasta_parser_s()
	{
		if (stage) (void)hipHostFree(stage);
		free(pac);
		if (ev0) (void)hipEventDestroy(ev0);
		if (ev1) (void)hipEventDestroy(ev1);
		if (st) (void)hipStreamDestroy(st);
	}
	int fail(int code, const std::string &msg) { if (!rc) { rc = code; err = msg; } return rc; }
	int hip(const char *what, hipError_t e) { return e == hipSuccess ? 0 : fail(BWAGPU_EHIP, std::string(what) + ": " + hipGetErrorString(e)); }
	int scan(FaSum *in, FaSum *out, u64 m)
	{
		size_t bytes = 0;
		hipError_t e = rocprim::inclusive_scan(nullptr, bytes, in, out, (size_t)m, FaCombine(), st);
		if (e != hipSuccess) return hip("inclusive_scan(size)", e);
		if (d_tmp.ensure(bytes)) return fail(BWAGPU_ENOMEM, "hipMalloc failed (scan scratch)");
		return hip("inclusive_scan", rocprim::inclusive_scan(d_tmp.p, bytes, in, out, (size_t)m, FaCombine(), st));
	}
	static bool space(u8 c) { return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r'; }
	// a complete header line (the text after '>', without the '\n'): name up to the first white space; the rest of the line is the
	// comment unless that delimiter ended the line (kseq.h:195-196, ks_getuntil2's '\r' rule); strdup stops at a NUL (bntseq.c:241-242)
	void finish_header(Contig &c, const std::string &t)
	{
		size_t i = 0;
		while (i < t.size() && !space((u8)t[i])) ++i;
		c.name = std::string(t.c_str(), strnlen(t.c_str(), i));
		std::string com = i < t.size() ? t.substr(i + 1) : std::string();
		if (com.size() > 1 && com.back() == '\r') com.pop_back();
		c.anno = com.empty() ? std::string("(null)") : std::string(com.c_str());
	}
	int grow_pac(u64 bytes)
	{
		if (bytes <= pac_cap) return 0;
		size_t want = pac_cap ? pac_cap : ((size_t)1 << 20);
		while (want < bytes) want <<= 1;
		u8 *np = (u8*)realloc(pac, want);
		if (!np) return fail(BWAGPU_ENOMEM, "malloc failed (.pac)");
		memset(np + pac_cap, 0, want - pac_cap);
		pac = np; pac_cap = want;
		return 0;
	}
	// parse stage[0..n) (the whole stage when eof, else all but a trailing '\r')
	int process(bool eof)
	{
		size_t n = n_stage;
		if (!eof && n && stage[n - 1] == '\r') --n;
		if (n == 0) return 0;
		const u64 T = (n + FA_TILE - 1) / FA_TILE;
		if (d_buf.ensure(n) || d_tsum.ensure(T * sizeof(FaSum)) || d_tscan.ensure(T * sizeof(FaSum)) || d_err.ensure(8))
			return fail(BWAGPU_ENOMEM, "hipMalloc failed (FASTA chunk)");
		if (hip("copy chunk", hipMemcpyAsync(d_buf.p, stage, n, hipMemcpyHostToDevice, st)) || hip("memset", hipMemsetAsync(d_err.p, 0, 8, st))) return rc;
		(void)hipEventRecord(ev0, st);
		FaOut o; memset(&o, 0, sizeof o);
		o.err = d_err.as<u64>(); o.jump = d_jump.as<u64>();
		const u8 *b = d_buf.as<u8>();
		FaSum *ts = d_tsum.as<FaSum>(), *tc = d_tscan.as<FaSum>();
		hipLaunchKernelGGL(k_fa_pass<1>, dim3((unsigned)T), dim3(FA_BLOCK), 0, st, b, (u64)n, (int)eof, (int)ls, carry, tc, ts, o);
		if (scan(ts, tc, T)) return rc;
		hipLaunchKernelGGL(k_fa_pass<2>, dim3((unsigned)T), dim3(FA_BLOCK), 0, st, b, (u64)n, (int)eof, (int)ls, carry, tc, ts, o);
		if (scan(ts, tc, T)) return rc;
		hipLaunchKernelGGL(k_fa_pass<3>, dim3((unsigned)T), dim3(FA_BLOCK), 0, st, b, (u64)n, (int)eof, (int)ls, carry, tc, ts, o);
		if (scan(ts, tc, T)) return rc;
		FaSum last;
		if (hip("read back chunk totals", hipMemcpyAsync(&last, tc + (T - 1), sizeof last, hipMemcpyDeviceToHost, st)) || hip("sync", hipStreamSynchronize(st))) return rc;
		const FaSum tot = FaCombine()(carry, last);
		const u64 nk = tot.nk - carry.nk, ns = tot.ns - carry.ns, ne = tot.ne - carry.ne, nh = tot.nh - carry.nh;
		const u64 l0 = carry.nk, n_pac = nk ? ((l0 + nk - 1) >> 2) - (l0 >> 2) + 1 : 0;
		if (d_codes.ensure(nk + 1) || d_pac.ensure(n_pac + 1) || d_hoff.ensure(ns * 8 + 8) || d_hchr.ensure(ns + 1) || d_hend.ensure(ne * 8 + 8) ||
			d_hpos.ensure(nh * 8 + 8) || d_hdoff.ensure(nh * 8 + 8)) return fail(BWAGPU_ENOMEM, "hipMalloc failed (FASTA outputs)");
		o.codes = d_codes.as<u8>(); o.hole_off = d_hoff.as<u64>(); o.hole_chr = d_hchr.as<u8>(); o.hole_end = d_hend.as<u64>();
		o.hdr_pos = d_hpos.as<u64>(); o.hdr_off = d_hdoff.as<u64>();
		hipLaunchKernelGGL(k_fa_pass<4>, dim3((unsigned)T), dim3(FA_BLOCK), 0, st, b, (u64)n, (int)eof, (int)ls, carry, tc, ts, o);
		if (n_pac) hipLaunchKernelGGL(k_fa_pack, dim3(grid_for(n_pac)), dim3(IDX_BLOCK), 0, st, d_codes.as<u8>(), l0, nk, d_pac.as<u8>(), n_pac);
		(void)hipEventRecord(ev1, st);
		u64 errw = 0;
		h_pac.resize(n_pac); h_hoff.resize(ns); h_hchr.resize(ns); h_hend.resize(ne); h_hpos.resize(nh); h_hdoff.resize(nh);
		if (hip("download", hipMemcpyAsync(&errw, d_err.p, 8, hipMemcpyDeviceToHost, st)) ||
			(n_pac && hip("download", hipMemcpyAsync(h_pac.data(), d_pac.p, n_pac, hipMemcpyDeviceToHost, st))) ||
			(ns && hip("download", hipMemcpyAsync(h_hoff.data(), d_hoff.p, ns * 8, hipMemcpyDeviceToHost, st))) ||
			(ns && hip("download", hipMemcpyAsync(h_hchr.data(), d_hchr.p, ns, hipMemcpyDeviceToHost, st))) ||
			(ne && hip("download", hipMemcpyAsync(h_hend.data(), d_hend.p, ne * 8, hipMemcpyDeviceToHost, st))) ||
			(nh && hip("download", hipMemcpyAsync(h_hpos.data(), d_hpos.p, nh * 8, hipMemcpyDeviceToHost, st))) ||
			(nh && hip("download", hipMemcpyAsync(h_hdoff.data(), d_hdoff.p, nh * 8, hipMemcpyDeviceToHost, st))) ||
			hip("sync", hipStreamSynchronize(st))) return rc;
		{ float ms = 0; if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) parse_ms += ms; }
		if (errw) {
			const u64 pos = stage_pos + ((1ull << 40) - (errw >> 8));
			char m[200];
			snprintf(m, sizeof m, (errw & 0xFF) == FA_ERR_FASTQ ? "FASTQ record structure ('+' or '@' at the start of a sequence line) at byte offset %llu"
																 : "NUL or non-ASCII byte in a sequence line at byte offset %llu", (unsigned long long)(skipped + pos));
			return fail(BWAGPU_EINVAL, m);
		}
		// header lines: the one left open by the last chunk ends before any that starts here
		size_t hp = 0;
		auto read_line = [&](size_t from) -> bool {        // append stage[from..) up to '\n' to hdr; true when the line ended in this chunk
			const u8 *q = (const u8*)memchr(stage + from, '\n', n - from);
			const size_t e = q ? (size_t)(q - stage) : n;
			hdr.append((const char*)stage + from, e - from);
			return q != nullptr;
		};
		if (in_hdr && read_line(0)) { finish_header(contigs.back(), hdr); in_hdr = false; }
		for (; hp < nh; ++hp) {
			contigs.push_back(Contig());
			contigs.back().offset = h_hdoff[hp];
			hdr.clear();
			if (read_line((size_t)h_hpos[hp] + 1)) finish_header(contigs.back(), hdr);
			else in_hdr = true;
		}
		if (n_pac) {
			if (grow_pac((l0 >> 2) + n_pac + 1)) return rc;
			pac[l0 >> 2] |= h_pac[0];
			if (n_pac > 1) memcpy(pac + (l0 >> 2) + 1, h_pac.data() + 1, n_pac - 1);
		}
		hole_off.insert(hole_off.end(), h_hoff.begin(), h_hoff.end());
		hole_chr.insert(hole_chr.end(), h_hchr.begin(), h_hchr.end());
		hole_end.insert(hole_end.end(), h_hend.begin(), h_hend.end());
		carry = tot;
		ls = stage[n - 1] == '\n';
		memmove(stage, stage + n, n_stage - n);
		n_stage -= n; stage_pos += n;
		return 0;
	}
};

static void fa_err(const bwagpu_fasta_parser_t *p, char *errbuf, size_t errlen)
{
	if (errbuf && errlen) snprintf(errbuf, errlen, "%s", p->err.c_str());
}

extern "C" int bwagpu_fasta_begin(bwagpu_fasta_parser_t **out, int device, int64_t chunk_bytes, char *errbuf, size_t errlen)
{
	if (errbuf && errlen) errbuf[0] = 0;
	if (!out) return BWAGPU_EINVAL;
	*out = nullptr;
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) return BWAGPU_ENODEV;
	bwagpu_fasta_parser_t *p = new bwagpu_fasta_parser_t();
	p->carry = fa_zero();
	p->chunk = chunk_bytes > 0 ? (size_t)chunk_bytes : ((size_t)256 << 20);
	if (hipStreamCreate(&p->st) != hipSuccess || hipEventCreate(&p->ev0) != hipSuccess || hipEventCreate(&p->ev1) != hipSuccess) { delete p; return BWAGPU_ENODEV; }
	if (hipHostMalloc((void**)&p->stage, p->chunk + 1, hipHostMallocDefault) != hipSuccess || p->d_jump.ensure(96 * 8)) {
		p->stage = nullptr; delete p;
		if (errbuf && errlen) snprintf(errbuf, errlen, "allocation of the FASTA staging buffers failed");
		return BWAGPU_ENOMEM;
	}
	u64 jump[96];                 // the lrand48 step x -> a x + c (mod 2^48) applied 2^j times
	u64 a = 0x5DEECE66Dull, c = 0xBull;
	const u64 M = (1ull << 48) - 1;
	for (int j = 0; j < 48; ++j) { jump[2 * j] = a; jump[2 * j + 1] = c; c = (a * c + c) & M; a = (a * a) & M; }
	if (hipMemcpy(p->d_jump.p, jump, sizeof jump, hipMemcpyHostToDevice) != hipSuccess) { delete p; return BWAGPU_EHIP; }
	*out = p;
	return 0;
}

extern "C" int bwagpu_fasta_feed(bwagpu_fasta_parser_t *p, const void *data, int64_t len, char *errbuf, size_t errlen)
{
	if (errbuf && errlen) errbuf[0] = 0;
	if (!p || len < 0 || (len && !data)) return BWAGPU_EINVAL;
	const u8 *s = (const u8*)data;
	size_t left = (size_t)len;
	while (left && !p->rc) {
		if (!p->started) {              // kseq_read: skip to the first '>' or '@' (kseq.h:181-184); '@' would make it FASTQ
			size_t i = 0;
			while (i < left && s[i] != '>' && s[i] != '@') ++i;
			p->skipped += i; s += i; left -= i;
			if (!left) break;
			if (*s == '@') { char m[160]; snprintf(m, sizeof m, "FASTQ input: '@' before the first '>' at byte offset %llu", (unsigned long long)p->skipped); p->fail(BWAGPU_EINVAL, m); break; }
			p->started = true;
		}
		const size_t room = p->chunk + 1 - p->n_stage, k = left < room ? left : room;
		memcpy(p->stage + p->n_stage, s, k);
		p->n_stage += k; s += k; left -= k;
		if (p->n_stage == p->chunk + 1) p->process(false);
	}
	if (p->rc) fa_err(p, errbuf, errlen);
	return p->rc;
}

extern "C" void bwagpu_fasta_free(bwagpu_fasta_t *r)
{
	if (!r) return;
	free(r->pac); free(r->seq_offset); free(r->seq_len); free(r->seq_n_ambs); free(r->names);
	free(r->hole_offset); free(r->hole_len); free(r->hole_amb);
	memset(r, 0, sizeof *r);
}

extern "C" int bwagpu_fasta_end(bwagpu_fasta_parser_t *p, bwagpu_fasta_t *out, char *errbuf, size_t errlen)
{
	if (errbuf && errlen) errbuf[0] = 0;
	if (!p) return BWAGPU_EINVAL;
	if (out) memset(out, 0, sizeof *out);
	if (!p->rc) p->process(true);
	if (!p->rc && p->in_hdr) {
		// a header line at the end of the stream: a '>' with nothing after it makes no record (ks_getuntil returns -1, kseq.h:190)
		if (p->hdr.empty()) p->contigs.pop_back();
		else p->finish_header(p->contigs.back(), p->hdr);
	}
	if (!p->rc && p->contigs.empty()) p->fail(BWAGPU_EINVAL, p->started ? "no FASTA record" : "no FASTA record (no '>' in the input)");
	const u64 l_pac = p->carry.nk;
	if (!p->rc && l_pac == 0) p->fail(BWAGPU_EINVAL, "the FASTA records hold no base");
	if (!p->rc && p->hole_end.size() + 1 == p->hole_off.size()) p->hole_end.push_back(l_pac);       // a hole open at the end
	if (!p->rc && p->hole_end.size() != p->hole_off.size()) p->fail(BWAGPU_EHIP, "internal: hole starts and ends do not pair up");
	const size_t n_seqs = p->contigs.size(), n_holes = p->hole_off.size();
	for (size_t i = 0; !p->rc && i < n_seqs; ++i) {
		const u64 e = i + 1 < n_seqs ? p->contigs[i + 1].offset : l_pac;
		if (e - p->contigs[i].offset >= (1ull << 31)) p->fail(BWAGPU_EINVAL, "contig '" + p->contigs[i].name + "' has 2^31 bases or more (bntann1_t::len is 32-bit)");
	}
	for (size_t i = 0; !p->rc && i < n_holes; ++i)
		if (p->hole_end[i] - p->hole_off[i] >= (1ull << 31)) p->fail(BWAGPU_EINVAL, "a run of ambiguous bases of 2^31 or more (bntamb1_t::len is 32-bit)");
	if (!p->rc && out) {
		size_t nb = 0;
		for (auto &c : p->contigs) nb += c.name.size() + c.anno.size() + 2;
		if (p->grow_pac(l_pac / 4 + 1)) goto done;
		out->pac = p->pac; p->pac = nullptr;
		out->l_pac = (int64_t)l_pac; out->n_seqs = (int32_t)n_seqs; out->n_holes = (int64_t)n_holes; out->names_bytes = (int64_t)nb;
		out->seq_offset = (int64_t*)malloc(n_seqs * 8 + 8); out->seq_len = (int32_t*)malloc(n_seqs * 4 + 4); out->seq_n_ambs = (int32_t*)malloc(n_seqs * 4 + 4);
		out->names = (char*)malloc(nb + 1);
		out->hole_offset = (int64_t*)malloc(n_holes * 8 + 8); out->hole_len = (int32_t*)malloc(n_holes * 4 + 4); out->hole_amb = (char*)malloc(n_holes + 1);
		if (!out->seq_offset || !out->seq_len || !out->seq_n_ambs || !out->names || !out->hole_offset || !out->hole_len || !out->hole_amb) { bwagpu_fasta_free(out); p->fail(BWAGPU_ENOMEM, "malloc failed (FASTA tables)"); goto done; }
		size_t w = 0, h = 0;
		for (size_t i = 0; i < n_seqs; ++i) {
			const auto &c = p->contigs[i];
			const u64 e = i + 1 < n_seqs ? p->contigs[i + 1].offset : l_pac;
			out->seq_offset[i] = (int64_t)c.offset; out->seq_len[i] = (int32_t)(e - c.offset);
			int32_t na = 0;
			while (h < n_holes && p->hole_off[h] < e) { ++na; ++h; }       // (holes never cross contigs and come in offset order)
			out->seq_n_ambs[i] = na;
			memcpy(out->names + w, c.name.c_str(), c.name.size() + 1); w += c.name.size() + 1;
			memcpy(out->names + w, c.anno.c_str(), c.anno.size() + 1); w += c.anno.size() + 1;
		}
		for (size_t i = 0; i < n_holes; ++i) {
			out->hole_offset[i] = (int64_t)p->hole_off[i]; out->hole_len[i] = (int32_t)(p->hole_end[i] - p->hole_off[i]); out->hole_amb[i] = p->hole_chr[i];
		}
		out->parse_ms = p->parse_ms;
	}
done:
	const int rc = p->rc;
	if (rc) fa_err(p, errbuf, errlen);
	delete p;
	return rc;
}

// ---- FASTQ windows -> batches (bseq_read, bwa.c:79-112) -------------------------------------------------------------------------
// The device does everything per byte and per record (dev_fastq.h); the host copies the windows up, waits once for the status, the
// batch size and the total sizes (FqInfo), sizes the result arrays, launches the emit pass and waits once for the copies.
struct bwagpu_fastq_parser_s {
	int device = 0;
	hipStream_t st = nullptr;
	hipEvent_t ev[7] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };      // (4, 5: around the BGZF inflate; 6: behind the classification)
	Buf d_comp[2], d_blk[2], d_bzstat;      // BGZF: compressed windows, block tables, status words + the bad words of both windows
	Buf d_buf[2], d_nl[2], d_recs[2], d_tcount, d_tbase, d_units, d_uscan, d_words, d_tmp;
	Buf o_seqs, o_off, o_names, o_name_off, o_quals, o_com, o_com_off, o_has, o_recs;
	Buf d_eqv, d_runs, d_cls, d_sums, d_sscan, o_idx;      // bwagpu_fastq_batch_smart: dev_fastq_smart.h's arrays
	Buf d_lflag[2], d_lines[2], d_lscan[2], d_hline[2], d_bend[2];      // bwagpu_fastq_batch_fasta: dev_fasta_reads.h's arrays
	Buf d_otext, d_otok, d_oslot, d_osize, d_ooff, d_opack;      // bwagpu_bgzf_deflate: dev_bgzf_out.h's text, tokens, slots, sizes, offsets and packed blocks
	std::string err;

	~bwagpu_fastq_parser_s()
	{
		for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
		if (st) (void)hipStreamDestroy(st);
	}
	int fail(int code, const std::string &msg) { err = msg; return code; }
	int hip(const char *what, hipError_t e) { return e == hipSuccess ? 0 : fail(BWAGPU_EHIP, std::string(what) + ": " + hipGetErrorString(e)); }
	// buffers only grow (Buf::ensure keeps a buffer that is large enough)
	static u32 nl_cap_for(u64 n) { return (u32)(((n >> 1) + 8 + 3) & ~3ull); }
	int ensure_window(int k, u64 n)
	{
		const u64 cap = nl_cap_for(n);
		if (d_buf[k].ensure(n + 16) || d_nl[k].ensure(cap * 4) || d_recs[k].ensure((cap >> 2) * sizeof(bwagpu_fastq_rec_t)))
			return fail(BWAGPU_ENOMEM, "hipMalloc failed (FASTQ window)");
		return 0;
	}
	int ensure_shared(u64 tiles, u64 cap_units)
	{
		if (d_tcount.ensure(tiles * 8 + 8) || d_tbase.ensure(tiles * 8 + 8) || d_units.ensure(cap_units * sizeof(FqSum)) || d_uscan.ensure(cap_units * sizeof(FqSum)) ||
			d_words.ensure(FQ_N_WORDS * 8 + sizeof(FqInfo))) return fail(BWAGPU_ENOMEM, "hipMalloc failed (FASTQ scans)");
		return 0;
	}
	template <class T, class Op> int scan_incl(T *in, T *out, u64 m, Op op)
	{
		size_t bytes = 0;
		hipError_t e = rocprim::inclusive_scan(nullptr, bytes, in, out, (size_t)m, op, st);
		if (e != hipSuccess) return hip("inclusive_scan(size)", e);
		if (d_tmp.ensure(bytes)) return fail(BWAGPU_ENOMEM, "hipMalloc failed (scan scratch)");
		return hip("inclusive_scan", rocprim::inclusive_scan(d_tmp.p, bytes, in, out, (size_t)m, op, st));
	}
	int scan_excl(u64 *in, u64 *out, u64 m)
	{
		size_t bytes = 0;
		hipError_t e = rocprim::exclusive_scan(nullptr, bytes, in, out, (u64)0, (size_t)m, rocprim::plus<u64>(), st);
		if (e != hipSuccess) return hip("exclusive_scan(size)", e);
		if (d_tmp.ensure(bytes)) return fail(BWAGPU_ENOMEM, "hipMalloc failed (scan scratch)");
		return hip("exclusive_scan", rocprim::exclusive_scan(d_tmp.p, bytes, in, out, (u64)0, (size_t)m, rocprim::plus<u64>(), st));
	}
};

extern "C" const char *bwagpu_fastq_last_error(const bwagpu_fastq_parser_t *p) { return p ? p->err.c_str() : ""; }
extern "C" int bwagpu_fastq_rec_size(void) { return (int)sizeof(bwagpu_fastq_rec_t); }

extern "C" int bwagpu_fastq_begin(bwagpu_fastq_parser_t **out, int device, char *errbuf, size_t errlen)
{
	if (errbuf && errlen) errbuf[0] = 0;
	if (!out) return BWAGPU_EINVAL;
	*out = nullptr;
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) return BWAGPU_ENODEV;
	bwagpu_fastq_parser_t *p = new bwagpu_fastq_parser_t();
	p->device = device;
	bool ok = hipStreamCreate(&p->st) == hipSuccess;
	for (hipEvent_t &e : p->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
	if (!ok) { delete p; if (errbuf && errlen) snprintf(errbuf, errlen, "could not create the FASTQ parser's stream and events"); return BWAGPU_ENODEV; }
	*out = p;
	return 0;
}

extern "C" void bwagpu_fastq_end(bwagpu_fastq_parser_t *p) { delete p; }

extern "C" int bwagpu_fastq_reserve(bwagpu_fastq_parser_t *p, int64_t window_bytes)
{
	if (!p || window_bytes < 0 || window_bytes >= ((int64_t)1 << 31)) return BWAGPU_EINVAL;
	if (hipSetDevice(p->device) != hipSuccess) return p->fail(BWAGPU_ENODEV, "hipSetDevice failed");
	const u64 n = (u64)window_bytes, tiles = 2 * ((n + FQ_TILE - 1) / FQ_TILE);
	int rc = p->ensure_window(0, n);
	if (!rc) rc = p->ensure_window(1, n);
	if (!rc) rc = p->ensure_shared(tiles, bwagpu_fastq_parser_s::nl_cap_for(n) >> 2);
	// the outputs of a window's worth of records: the text itself bounds every blob
	if (!rc && (p->o_seqs.ensure(2 * n) || p->o_quals.ensure(2 * n) || p->o_names.ensure(2 * n) || p->o_com.ensure(2 * n))) rc = p->fail(BWAGPU_ENOMEM, "hipMalloc failed (FASTQ outputs)");
	return rc;
}

extern "C" void bwagpu_fastq_out_free(bwagpu_fastq_out_t *o)
{
	if (!o) return;
	bwagpu_free(o->seqs); bwagpu_free(o->off); bwagpu_free(o->names); bwagpu_free(o->name_off); bwagpu_free(o->quals);
	bwagpu_free(o->comments); bwagpu_free(o->comment_off); bwagpu_free(o->has_comment); bwagpu_free(o->recs);
	o->seqs = nullptr; o->off = nullptr; o->names = nullptr; o->name_off = nullptr; o->quals = nullptr;
	o->comments = nullptr; o->comment_off = nullptr; o->has_comment = nullptr; o->recs = nullptr;
}

// the windows of a call: buffers sized, A filled (W.buf: the window buffer's start)
static int fq_setup(bwagpu_fastq_parser_t *p, FqArgs &A, int nw, const u64 len[2], const int eof[2], u32 *n_tiles, u64 *n_units)
{
	memset(&A, 0, sizeof A);
	A.nw = nw;
	u32 tiles = 0; u64 cap_units = ~0ull;
	for (int k = 0; k < A.nw; ++k) {
		if (int rc = p->ensure_window(k, len[k])) return rc;
		FqWin &W = A.w[k];
		W.buf = p->d_buf[k].as<u8>(); W.n = (u32)len[k]; W.tile0 = tiles; W.n_tiles = (u32)((len[k] + FQ_TILE - 1) / FQ_TILE); tiles += W.n_tiles;
		W.nl = p->d_nl[k].as<u32>(); W.nl_cap = bwagpu_fastq_parser_s::nl_cap_for(len[k]); W.recs = p->d_recs[k].as<bwagpu_fastq_rec_t>(); W.rec_cap = W.nl_cap >> 2; W.eof = eof[k];
		if (W.rec_cap < cap_units) cap_units = W.rec_cap;
	}
	A.cap_units = (u32)cap_units;
	*n_tiles = tiles; *n_units = cap_units;
	return p->ensure_shared(tiles, cap_units);
}

// passes 1 to 3 behind the copy-up: the text windows are in place on the device (in stream order).  Events 0, 1, 2 are recorded
static int fq_launch(bwagpu_fastq_parser_t *p, const FqArgs &A, u32 tiles, u64 cap_units, int chunk_size)
{
	u64 *words = p->d_words.as<u64>();
	FqInfo *d_info = (FqInfo*)(words + FQ_N_WORDS);
	FqSum *units = p->d_units.as<FqSum>(), *uscan = p->d_uscan.as<FqSum>();
	if (p->hip("memset", hipMemsetAsync(words, 0, FQ_N_WORDS * 8, p->st))) return BWAGPU_EHIP;
	(void)hipEventRecord(p->ev[0], p->st);
	if (tiles) {
		hipLaunchKernelGGL(k_fq_count, dim3(tiles), dim3(FQ_BLOCK), 0, p->st, A, p->d_tcount.as<u64>());
		if (int rc = p->scan_excl(p->d_tcount.as<u64>(), p->d_tbase.as<u64>(), tiles)) return rc;
		hipLaunchKernelGGL(k_fq_index, dim3(tiles), dim3(FQ_BLOCK), 0, p->st, A, p->d_tbase.as<u64>(), words);
	}
	const unsigned ugrid = grid_for(cap_units) < 1024 ? grid_for(cap_units) : 1024;
	hipLaunchKernelGGL(k_fq_records, dim3(ugrid), dim3(FQ_BLOCK), 0, p->st, A, words, units);
	(void)hipEventRecord(p->ev[1], p->st);
	if (int rc = p->scan_incl(units, uscan, cap_units, FqPlus())) return rc;
	hipLaunchKernelGGL(k_fq_cut, dim3(ugrid), dim3(FQ_BLOCK), 0, p->st, A, words, uscan, (u64)chunk_size);
	hipLaunchKernelGGL(k_fq_decide, dim3(1), dim3(FQ_WAVE), 0, p->st, A, words, uscan, d_info);
	(void)hipEventRecord(p->ev[2], p->st);
	return 0;
}

// FASTA records in the windows fq_setup laid out (dev_fasta_reads.h): a newline slot for every byte, a record slot for every two, and
// the per-line and per-record arrays
static int fr_setup(bwagpu_fastq_parser_t *p, FqArgs &A, FrArgs &X, u64 *n_units)
{
	memset(&X, 0, sizeof X);
	u64 cap_units = ~0ull;
	for (int k = 0; k < A.nw; ++k) {
		FqWin &W = A.w[k];
		const u64 cap_lines = ((u64)W.n + 1 + 3) & ~3ull, cap_recs = ((u64)W.n >> 1) + 2;
		if (p->d_nl[k].ensure(cap_lines * 4) || p->d_recs[k].ensure(cap_recs * sizeof(bwagpu_fastq_rec_t)) || p->d_lflag[k].ensure(cap_lines) ||
			p->d_lines[k].ensure(cap_lines * sizeof(FrLine)) || p->d_lscan[k].ensure(cap_lines * sizeof(FrLine)) || p->d_hline[k].ensure((cap_recs + 1) * 4) ||
			p->d_bend[k].ensure(cap_recs * 4)) return p->fail(BWAGPU_ENOMEM, "hipMalloc failed (FASTA window)");
		W.nl = p->d_nl[k].as<u32>(); W.nl_cap = (u32)cap_lines; W.recs = p->d_recs[k].as<bwagpu_fastq_rec_t>(); W.rec_cap = (u32)cap_recs;
		FrWin &Y = X.x[k];
		Y.lflag = p->d_lflag[k].as<u8>(); Y.lines = p->d_lines[k].as<FrLine>(); Y.lscan = p->d_lscan[k].as<FrLine>(); Y.hline = p->d_hline[k].as<u32>(); Y.bend = p->d_bend[k].as<u32>();
		if (cap_lines > X.cap_lines) X.cap_lines = (u32)cap_lines;
		if (cap_recs < cap_units) cap_units = cap_recs;
	}
	A.cap_units = (u32)cap_units;
	*n_units = cap_units;
	return p->ensure_shared(A.w[A.nw - 1].tile0 + A.w[A.nw - 1].n_tiles, cap_units);
}

// fq_launch for FASTA records
static int fr_launch(bwagpu_fastq_parser_t *p, const FqArgs &A, const FrArgs &X, u32 tiles, u64 cap_units, int chunk_size)
{
	u64 *words = p->d_words.as<u64>();
	FqInfo *d_info = (FqInfo*)(words + FQ_N_WORDS);
	FqSum *units = p->d_units.as<FqSum>(), *uscan = p->d_uscan.as<FqSum>();
	FrFmt F; F.X = X;
	if (p->hip("memset", hipMemsetAsync(words, 0, FQ_N_WORDS * 8, p->st))) return BWAGPU_EHIP;
	for (int k = 0; k < A.nw; ++k) if (p->hip("memset", hipMemsetAsync(X.x[k].lflag, 0, A.w[k].nl_cap, p->st))) return BWAGPU_EHIP;
	(void)hipEventRecord(p->ev[0], p->st);
	if (tiles) {
		hipLaunchKernelGGL(k_fq_count, dim3(tiles), dim3(FQ_BLOCK), 0, p->st, A, p->d_tcount.as<u64>());
		if (int rc = p->scan_excl(p->d_tcount.as<u64>(), p->d_tbase.as<u64>(), tiles)) return rc;
		hipLaunchKernelGGL(k_fr_index, dim3(tiles), dim3(FQ_BLOCK), 0, p->st, A, X, p->d_tbase.as<u64>(), words);
	}
	const unsigned lgrid = grid_for(X.cap_lines) < 1024 ? grid_for(X.cap_lines) : 1024;
	hipLaunchKernelGGL(k_fr_lines, dim3(lgrid), dim3(FQ_BLOCK), 0, p->st, A, X, (const u64*)words);
	for (int k = 0; k < A.nw; ++k) if (int rc = p->scan_incl(X.x[k].lines, X.x[k].lscan, A.w[k].nl_cap, FrLinePlus())) return rc;
	hipLaunchKernelGGL(k_fr_place, dim3(lgrid), dim3(FQ_BLOCK), 0, p->st, A, X, words);
	const unsigned ugrid = grid_for(cap_units) < 1024 ? grid_for(cap_units) : 1024;
	hipLaunchKernelGGL(k_fr_records, dim3(ugrid), dim3(FQ_BLOCK), 0, p->st, A, F, words, units);
	(void)hipEventRecord(p->ev[1], p->st);
	if (int rc = p->scan_incl(units, uscan, cap_units, FqPlus())) return rc;
	hipLaunchKernelGGL(k_fr_cut, dim3(ugrid), dim3(FQ_BLOCK), 0, p->st, A, F, words, uscan, (u64)chunk_size);
	hipLaunchKernelGGL(k_fr_decide, dim3(1), dim3(FQ_WAVE), 0, p->st, A, F, (const u64*)words, uscan, d_info);
	(void)hipEventRecord(p->ev[2], p->st);
	return 0;
}

// everything behind the copy-up.  X: the windows hold FASTA records (fr_setup has run): no qualities, and dev_fasta_reads.h's passes
static int fq_run(bwagpu_fastq_parser_t *p, const FqArgs &A, u32 tiles, u64 cap_units, int chunk_size, bwagpu_fastq_out_t *out, const FrArgs *X = nullptr)
{
	if (int rc = X ? fr_launch(p, A, *X, tiles, cap_units, chunk_size) : fq_launch(p, A, tiles, cap_units, chunk_size)) return rc;
	FqInfo *d_info = (FqInfo*)(p->d_words.as<u64>() + FQ_N_WORDS);
	const FqSum *uscan = p->d_uscan.as<FqSum>();
	FqInfo info;
	// wait 1: status, batch size, total sizes
	if (p->hip("read back the batch's sizes", hipMemcpyAsync(&info, d_info, sizeof info, hipMemcpyDeviceToHost, p->st)) || p->hip("sync", hipStreamSynchronize(p->st))) return BWAGPU_EHIP;
	if (p->hip("FASTQ kernels", hipGetLastError())) return BWAGPU_EHIP;
	{ float ms = 0; if (hipEventElapsedTime(&ms, p->ev[0], p->ev[1]) == hipSuccess) out->kernel_ms[0] = ms; if (hipEventElapsedTime(&ms, p->ev[1], p->ev[2]) == hipSuccess) out->kernel_ms[1] = ms; }
	out->status = (int32_t)info.status;
	if (info.status == BWAGPU_FQ_DECLINED) { out->declined_file = (int32_t)info.declined_file; out->declined_at = info.declined_at; return 0; }
	if (info.status == BWAGPU_FQ_MORE) return 0;
	const u64 n_reads = (u64)info.n_units * (u64)A.nw;
	if (n_reads >= (1ull << 31)) return p->fail(BWAGPU_EUNSUP, "a batch of 2^31 reads or more");
	out->n_reads = (int32_t)n_reads; out->consumed[0] = info.consumed[0]; out->consumed[1] = info.consumed[1];
	const u64 ts = info.total.seq, tn = info.total.name, tc = info.total.com;
	out->seqs = (uint8_t*)bwagpu_alloc_host(ts + 1); out->off = (int64_t*)bwagpu_alloc_host((n_reads + 1) * 8);
	out->names = (char*)bwagpu_alloc_host(tn + 1); out->name_off = (int64_t*)bwagpu_alloc_host((n_reads + 1) * 8);
	out->quals = X ? nullptr : (char*)bwagpu_alloc_host(ts + 1);
	out->comments = (char*)bwagpu_alloc_host(tc + 1); out->comment_off = (int64_t*)bwagpu_alloc_host((n_reads + 1) * 8);
	out->has_comment = (uint8_t*)bwagpu_alloc_host(n_reads + 1); out->recs = (bwagpu_fastq_rec_t*)bwagpu_alloc_host((n_reads + 1) * sizeof(bwagpu_fastq_rec_t));
	int rc = 0;
	if (!out->seqs || !out->off || !out->names || !out->name_off || (!out->quals && !X) || !out->comments || !out->comment_off || !out->has_comment || !out->recs)
		rc = p->fail(BWAGPU_ENOMEM, "out of host memory (FASTQ batch)");
	if (!rc && n_reads == 0) { out->off[0] = out->name_off[0] = out->comment_off[0] = 0; return 0; }
	if (!rc && (p->o_seqs.ensure(ts + 1) || (!X && p->o_quals.ensure(ts + 1)) || p->o_names.ensure(tn + 1) || p->o_com.ensure(tc + 1) || p->o_off.ensure((n_reads + 1) * 8) ||
				p->o_name_off.ensure((n_reads + 1) * 8) || p->o_com_off.ensure((n_reads + 1) * 8) || p->o_has.ensure(n_reads) || p->o_recs.ensure(n_reads * sizeof(bwagpu_fastq_rec_t))))
		rc = p->fail(BWAGPU_ENOMEM, "hipMalloc failed (FASTQ outputs)");
	if (!rc) {
		FqOut o;
		o.seqs = p->o_seqs.as<u8>(); o.off = p->o_off.as<i64>(); o.names = p->o_names.as<char>(); o.name_off = p->o_name_off.as<i64>(); o.quals = p->o_quals.as<char>();
		o.comments = p->o_com.as<char>(); o.comment_off = p->o_com_off.as<i64>(); o.has_comment = p->o_has.as<u8>(); o.recs = p->o_recs.as<bwagpu_fastq_rec_t>();
		const u64 eblocks = (n_reads + FQ_BLOCK / FQ_WAVE - 1) / (FQ_BLOCK / FQ_WAVE);
		const dim3 egrid((unsigned)(eblocks < 65536 ? eblocks : 65536));
		if (X) hipLaunchKernelGGL(k_fr_emit, egrid, dim3(FQ_BLOCK), 0, p->st, A, *X, uscan, n_reads, info.total, o);
		else hipLaunchKernelGGL(k_fq_emit, egrid, dim3(FQ_BLOCK), 0, p->st, A, uscan, n_reads, info.total, o);
		(void)hipEventRecord(p->ev[3], p->st);
		auto down = [&](void *dst, const Buf &src, u64 bytes) { return bytes ? p->hip("download", hipMemcpyAsync(dst, src.p, (size_t)bytes, hipMemcpyDeviceToHost, p->st)) : 0; };
		// wait 2: the copies
		if (down(out->seqs, p->o_seqs, ts) || (!X && down(out->quals, p->o_quals, ts)) || down(out->names, p->o_names, tn) || down(out->comments, p->o_com, tc) ||
			down(out->off, p->o_off, (n_reads + 1) * 8) || down(out->name_off, p->o_name_off, (n_reads + 1) * 8) || down(out->comment_off, p->o_com_off, (n_reads + 1) * 8) ||
			down(out->has_comment, p->o_has, n_reads) || down(out->recs, p->o_recs, n_reads * sizeof(bwagpu_fastq_rec_t)) || p->hip("sync", hipStreamSynchronize(p->st)) ||
			p->hip("FASTQ emit kernel", hipGetLastError())) rc = BWAGPU_EHIP;
		else { float ms = 0; if (hipEventElapsedTime(&ms, p->ev[2], p->ev[3]) == hipSuccess) out->kernel_ms[2] = ms; }
	}
	if (rc) { bwagpu_fastq_out_free(out); out->status = 0; out->n_reads = 0; }
	return rc;
}

// bwagpu_fastq_batch and bwagpu_fastq_batch_fasta: `what` names the call in the error text
static int fq_batch(bwagpu_fastq_parser_t *p, const char *what, bool fasta, const void *raw1, int64_t len1, int eof1, const void *raw2, int64_t len2, int eof2,
					int chunk_size, bwagpu_fastq_out_t *out)
{
	const int64_t lim = (int64_t)1 << 31;
	if (!p) return BWAGPU_EINVAL;
	if (!out || !raw1 || len1 < 0 || len2 < 0 || len1 >= lim || len2 >= lim || chunk_size <= 0 || (!raw2 && len2 != 0))
		return p->fail(BWAGPU_EINVAL, std::string(what) + ": NULL argument, negative length, window of 2^31 bytes or more, chunk_size <= 0, or a length without a second window");
	memset(out, 0, sizeof *out);
	out->declined_file = -1; out->declined_at = -1;
	p->err.clear();
	if (hipSetDevice(p->device) != hipSuccess) return p->fail(BWAGPU_ENODEV, "hipSetDevice failed");      // (the caller's thread may be another one than bwagpu_fastq_begin's)
	FqArgs A; FrArgs X;
	const void *raw[2] = { raw1, raw2 }; const u64 len[2] = { (u64)len1, (u64)len2 }; const int eof[2] = { eof1, eof2 };
	u32 tiles = 0; u64 cap_units = 0;
	if (int rc = fq_setup(p, A, raw2 ? 2 : 1, len, eof, &tiles, &cap_units)) return rc;
	if (fasta) if (int rc = fr_setup(p, A, X, &cap_units)) return rc;
	for (int k = 0; k < A.nw; ++k)
		if (len[k] && p->hip("copy window", hipMemcpyAsync(p->d_buf[k].p, raw[k], (size_t)len[k], hipMemcpyHostToDevice, p->st))) return BWAGPU_EHIP;
	return fq_run(p, A, tiles, cap_units, chunk_size, out, fasta ? &X : nullptr);
}

extern "C" int bwagpu_fastq_batch(bwagpu_fastq_parser_t *p, const void *raw1, int64_t len1, int eof1, const void *raw2, int64_t len2, int eof2,
								  int chunk_size, bwagpu_fastq_out_t *out)
{
	return fq_batch(p, "bwagpu_fastq_batch", false, raw1, len1, eof1, raw2, len2, eof2, chunk_size, out);
}

extern "C" int bwagpu_fastq_batch_fasta(bwagpu_fastq_parser_t *p, const void *raw1, int64_t len1, int eof1, const void *raw2, int64_t len2, int eof2,
										int chunk_size, bwagpu_fastq_out_t *out)
{
	return fq_batch(p, "bwagpu_fastq_batch_fasta", true, raw1, len1, eof1, raw2, len2, eof2, chunk_size, out);
}

extern "C" void bwagpu_fasta_reads_limits(int32_t out[4])
{
	out[0] = FQ_TILE; out[1] = FQ_SEG; out[2] = FR_STEP; out[3] = 0;
}

// ---- BGZF windows -> text (dev_bgzf.h) ---------------------------------------------------------------------------------------------
// The host walks the block headers (BgzfPipe::block_len's test, host/host_input.h) and reads the trailers; the device inflates and tests.
namespace {

// total length of the BGZF block at p (header .. trailer), or 0 if p does not start one that lies within the n bytes in view
size_t bz_block_len(const u8 *p, size_t n)
{
	if (n < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return 0;
	const size_t xlen = p[10] | (size_t)p[11] << 8;
	if (12 + xlen > n) return 0;
	for (size_t o = 12; o + 4 <= 12 + xlen;) {
		const size_t sl = p[o + 2] | (size_t)p[o + 3] << 8;
		if (p[o] == 'B' && p[o + 1] == 'C' && sl == 2 && o + 6 <= 12 + xlen) { const size_t bs = (p[o + 4] | (size_t)p[o + 5] << 8) + 1; return bs >= 12 + xlen + 8 && bs <= n ? bs : 0; }
		o += 4 + sl;
	}
	return 0;
}
u32 bz_le32(const u8 *p) { return p[0] | (u32)p[1] << 8 | (u32)p[2] << 16 | (u32)p[3] << 24; }

// the blocks a call takes from a window
struct BzPlan {
	std::vector<BzBlock> blk, table; std::vector<i64> coff;      // (blk[j].out: offset of the block's text among the taken blocks' text; table: as uploaded)
	i64 used = 0, inflated = 0, host_bad = -1; bool cut_short = false;
};
void bz_walk(const u8 *comp, i64 comp_len, int eof, BzPlan &P)
{
	i64 o = 0;
	while (o < comp_len) {
		const size_t bl = bz_block_len(comp + o, (size_t)(comp_len - o));
		if (!bl) break;
		const size_t xlen = comp[o + 10] | (size_t)comp[o + 11] << 8;
		const u32 isize = bz_le32(comp + o + bl - 4);
		if (isize > BZ_MAX_OUT) { P.host_bad = o; break; }                       // (never size anything from an unbounded ISIZE)
		if (P.inflated + (i64)isize >= ((i64)1 << 31)) { P.cut_short = true; break; }
		BzBlock B; B.pay = (u64)o + 12 + xlen; B.pay_len = (u32)(bl - 12 - xlen - 8); B.isize = isize; B.crc = bz_le32(comp + o + bl - 8); B.pad = 0; B.out = (u64)P.inflated;
		P.blk.push_back(B); P.coff.push_back(o);
		P.inflated += isize; o += (i64)bl;
	}
	P.used = o;
	if (P.host_bad < 0 && !P.cut_short && o < comp_len && eof) P.host_bad = o;   // a partial block, or bytes that are no block, where the input ends
}

// upload window k's taken blocks and their table: a block's text goes to blk.out + shift of the text buffer
int bz_upload(bwagpu_fastq_parser_t *p, int k, const u8 *comp, BzPlan &P, u64 shift)
{
	const size_t nb = P.blk.size();
	if (!nb) return 0;
	if (p->d_comp[k].ensure((size_t)P.used + 32) || p->d_blk[k].ensure(nb * sizeof(BzBlock))) return p->fail(BWAGPU_ENOMEM, "hipMalloc failed (BGZF window)");
	P.table = P.blk;                            // (lives until the caller has waited for the stream)
	for (BzBlock &B : P.table) B.out += shift;
	if (p->hip("copy blocks", hipMemcpyAsync(p->d_comp[k].p, comp, (size_t)P.used, hipMemcpyHostToDevice, p->st)) ||
		p->hip("copy block table", hipMemcpyAsync(p->d_blk[k].p, P.table.data(), nb * sizeof(BzBlock), hipMemcpyHostToDevice, p->st))) return BWAGPU_EHIP;
	return 0;
}
// one wavefront per block of window k
void bz_launch(bwagpu_fastq_parser_t *p, int k, const BzPlan &P, u8 *dst)
{
	const size_t nb = P.blk.size();
	if (!nb) return;
	BzArgs A; A.comp = p->d_comp[k].as<u8>(); A.blk = p->d_blk[k].as<BzBlock>(); A.n_blocks = (u32)nb; A.out = dst; A.bad = p->d_bzstat.as<u64>() + k;
	hipLaunchKernelGGL(k_bz_inflate, dim3((unsigned)nb), dim3(BZ_WAVE), 0, p->st, A);
}

void bz_info(const BzPlan &P, bwagpu_bgzf_info_t *I)
{
	memset(I, 0, sizeof *I);
	I->used_comp = P.used; I->inflated = P.inflated; I->n_blocks = (int32_t)P.blk.size(); I->damaged_at = -1;
}
// the verdict of window k: the first damaged block's offset (device word `bad`), or what the walk found behind the blocks
i64 bz_damage(bwagpu_fastq_parser_t *p, const BzPlan &P, u64 bad)
{
	if (bad) {
		const u64 j = BZ_BIG - (bad >> 8);
		const i64 at = j < P.coff.size() ? P.coff[j] : P.used;
		p->err = "BGZF block at offset " + std::to_string(at) + " of its window is damaged (dev_bgzf.h BZ_E_* " + std::to_string((int)(bad & 255)) + ")";
		return at;
	}
	if (P.host_bad >= 0) p->err = "no whole BGZF block with an ISIZE of at most 65536 at offset " + std::to_string(P.host_bad) + " of its window";
	return P.host_bad;
}

}

extern "C" int bwagpu_bgzf_inflate(bwagpu_fastq_parser_t *p, const void *comp, int64_t comp_len, int eof, void *dst, int64_t dst_cap, bwagpu_bgzf_info_t *info)
{
	if (!p) return BWAGPU_EINVAL;
	if (!comp || comp_len < 0 || !dst || dst_cap < 0 || !info) return p->fail(BWAGPU_EINVAL, "bwagpu_bgzf_inflate: NULL argument or negative length");
	p->err.clear();
	BzPlan P;
	bz_walk((const u8*)comp, comp_len, eof, P);
	bz_info(P, info);
	if (dst_cap < P.inflated) return p->fail(BWAGPU_EINVAL, "bwagpu_bgzf_inflate: dst_cap is smaller than the blocks' summed ISIZE");
	if (hipSetDevice(p->device) != hipSuccess) return p->fail(BWAGPU_ENODEV, "hipSetDevice failed");
	u64 bad[2] = { 0, 0 };
	if (!P.blk.empty()) {
		if (p->d_buf[0].ensure((size_t)P.inflated + 16) || p->d_bzstat.ensure(16)) return p->fail(BWAGPU_ENOMEM, "hipMalloc failed (BGZF text)");
		if (p->hip("memset", hipMemsetAsync(p->d_bzstat.p, 0, 16, p->st))) return BWAGPU_EHIP;
		if (int rc = bz_upload(p, 0, (const u8*)comp, P, 0)) return rc;
		(void)hipEventRecord(p->ev[4], p->st);
		bz_launch(p, 0, P, p->d_buf[0].as<u8>());
		(void)hipEventRecord(p->ev[5], p->st);
		if (p->hip("read back the verdict", hipMemcpyAsync(bad, p->d_bzstat.p, 16, hipMemcpyDeviceToHost, p->st)) || p->hip("sync", hipStreamSynchronize(p->st)) ||
			p->hip("BGZF kernel", hipGetLastError())) return BWAGPU_EHIP;
		float ms = 0; if (hipEventElapsedTime(&ms, p->ev[4], p->ev[5]) == hipSuccess) info->inflate_ms = ms;
	}
	info->damaged_at = bz_damage(p, P, bad[0]);
	info->next_coff = P.used; info->next_uoff = 0;
	if (info->damaged_at >= 0 || !P.inflated) return 0;
	if (p->hip("download", hipMemcpyAsync(dst, p->d_buf[0].p, (size_t)P.inflated, hipMemcpyDeviceToHost, p->st)) || p->hip("sync", hipStreamSynchronize(p->st))) return BWAGPU_EHIP;
	return 0;
}

// ---- text -> BGZF blocks (dev_bgzf_out.h) ---------------------------------------------------------------------------------------------
// The host cuts the text into blocks and launches of BO_LAUNCH blocks; per launch the device compresses every block into its slot, scans
// the sizes and packs the slots, and the host waits twice: for the packed length, then for the bytes.
#define BO_LAUNCH 1024

extern "C" void bwagpu_bgzf_out_limits(int32_t out[4])
{
	out[0] = (int32_t)BO_MAX_TEXT; out[1] = (int32_t)BO_MIN_MATCH; out[2] = (int32_t)BO_MAX_MATCH; out[3] = (int32_t)BO_MAX_DIST;
}

extern "C" int bwagpu_bgzf_deflate(bwagpu_fastq_parser_t *p, const void *text, int64_t text_len, int block_size, int eof_marker, void **comp, bwagpu_bgzf_out_info_t *info)
{
	static const u8 eof_block[28] = { 0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
	if (!p) return BWAGPU_EINVAL;
	if (comp) *comp = nullptr;
	if (!text || text_len < 0 || !comp || !info || block_size < 0 || block_size > (int)BO_MAX_TEXT)
		return p->fail(BWAGPU_EINVAL, "bwagpu_bgzf_deflate: NULL argument, negative length or block_size outside 0..0xff00");
	p->err.clear();
	memset(info, 0, sizeof *info);
	const u64 bs = block_size ? (u64)block_size : BO_MAX_TEXT, n = (u64)text_len, nb_all = (n + bs - 1) / bs;
	const u64 cap = n + 31 * nb_all + sizeof eof_block;          // (no block is larger than its stored form)
	u8 *dst = (u8*)bwagpu_alloc_host(cap);
	if (!dst) return p->fail(BWAGPU_ENOMEM, "bwagpu_bgzf_deflate: no host memory for the blocks");
	if (hipSetDevice(p->device) != hipSuccess) { bwagpu_free(dst); return p->fail(BWAGPU_ENODEV, "hipSetDevice failed"); }
	u64 at = 0;
	int rc = 0;
	for (u64 b0 = 0; b0 < nb_all && !rc; b0 += BO_LAUNCH) {
		const u64 nb = nb_all - b0 < BO_LAUNCH ? nb_all - b0 : BO_LAUNCH, t0 = b0 * bs, tn = n - t0 < nb * bs ? n - t0 : nb * bs;
		if (p->d_otext.ensure(tn + 16) || p->d_otok.ensure(nb * BO_MAX_TEXT * 4) || p->d_oslot.ensure(nb * BO_SLOT) || p->d_osize.ensure(nb * 8 + 8) ||
			p->d_ooff.ensure(nb * 8 + 8) || p->d_opack.ensure(tn + 31 * nb)) { rc = p->fail(BWAGPU_ENOMEM, "hipMalloc failed (BGZF output)"); break; }
		BoArgs A; A.text = p->d_otext.as<u8>(); A.text_len = tn; A.block_size = (u32)bs; A.n_blocks = (u32)nb; A.tok = p->d_otok.as<u32>(); A.slot = p->d_oslot.as<u8>(); A.sizes = p->d_osize.as<u64>();
		BoPack G; G.slot = A.slot; G.sizes = A.sizes; G.off = p->d_ooff.as<u64>(); G.dst = p->d_opack.as<u8>(); G.n_blocks = (u32)nb;
		if (p->hip("copy text", hipMemcpyAsync(p->d_otext.p, (const u8*)text + t0, tn, hipMemcpyHostToDevice, p->st)) ||
			p->hip("memset", hipMemsetAsync(p->d_oslot.p, 0, nb * BO_SLOT, p->st))) { rc = BWAGPU_EHIP; break; }
		(void)hipEventRecord(p->ev[4], p->st);
		hipLaunchKernelGGL(k_bo_deflate, dim3((unsigned)nb), dim3(BO_WAVE), 0, p->st, A);
		(void)hipEventRecord(p->ev[5], p->st);
		if ((rc = p->scan_excl(A.sizes, p->d_ooff.as<u64>(), nb))) break;
		hipLaunchKernelGGL(k_bo_gather, dim3((unsigned)nb), dim3(256), 0, p->st, G);
		u64 last[2] = { 0, 0 };
		if (p->hip("read back the packed length", hipMemcpyAsync(&last[0], p->d_ooff.as<u64>() + nb - 1, 8, hipMemcpyDeviceToHost, p->st)) ||
			p->hip("read back the packed length", hipMemcpyAsync(&last[1], A.sizes + nb - 1, 8, hipMemcpyDeviceToHost, p->st)) ||
			p->hip("sync", hipStreamSynchronize(p->st)) || p->hip("BGZF output kernels", hipGetLastError())) { rc = BWAGPU_EHIP; break; }
		const u64 packed = last[0] + last[1];
		if (packed > tn + 31 * nb || at + packed + sizeof eof_block > cap) { rc = p->fail(BWAGPU_EHIP, "bwagpu_bgzf_deflate: the device reported blocks larger than their stored form"); break; }
		if (p->hip("download", hipMemcpyAsync(dst + at, p->d_opack.p, packed, hipMemcpyDeviceToHost, p->st)) || p->hip("sync", hipStreamSynchronize(p->st))) { rc = BWAGPU_EHIP; break; }
		float ms = 0; if (hipEventElapsedTime(&ms, p->ev[4], p->ev[5]) == hipSuccess) info->deflate_ms += ms;
		at += packed;
	}
	if (rc) { bwagpu_free(dst); return rc; }
	if (eof_marker) { memcpy(dst + at, eof_block, sizeof eof_block); at += sizeof eof_block; }
	info->n_blocks = (int64_t)nb_all; info->text_len = text_len; info->comp_len = (int64_t)at;
	*comp = dst;
	return 0;
}

// bwagpu_fastq_batch_bgzf's work around the parse: the walk, the inflate into the window buffers and its verdict, then run(A, tiles,
// cap_units) -- the parse, which leaves *status and consumed[] --, then the virtual offsets.  info: two entries
template <class Run>
static int bz_batch(bwagpu_fastq_parser_t *p, const bwagpu_bgzf_win_t *const w[2], int nw, bwagpu_bgzf_info_t info[2], int32_t *status, const int64_t *consumed, Run run)
{
	BzPlan P[2];
	memset(info, 0, 2 * sizeof info[0]);
	info[1].damaged_at = -1;
	for (int k = 0; k < nw; ++k) {
		bz_walk((const u8*)w[k]->comp, w[k]->comp_len, w[k]->eof, P[k]);
		bz_info(P[k], &info[k]);
	}
	for (int k = 0; k < nw; ++k) {
		if (P[k].blk.empty() && w[k]->skip > 0 && !w[k]->eof && P[k].host_bad < 0) { *status = BWAGPU_FQ_MORE; return 0; }      // (the first block is not in view yet)
		if ((u32)w[k]->skip > (P[k].blk.empty() ? 0u : P[k].blk[0].isize)) return p->fail(BWAGPU_EINVAL, "bwagpu_fastq_batch_bgzf: skip is larger than the first block's ISIZE");
	}
	if (hipSetDevice(p->device) != hipSuccess) return p->fail(BWAGPU_ENODEV, "hipSetDevice failed");
	// the text windows: buffers first (they may move), then the inflate into them.  Block text starts `pad` bytes into the buffer so that the
	// text window -- skip bytes further on -- starts at a 16-byte boundary, as an uploaded window does
	u64 len[2] = { 0, 0 }, pad[2] = { 0, 0 }; int eof[2] = { 1, 1 };
	for (int k = 0; k < nw; ++k) {
		len[k] = (u64)P[k].inflated - (u64)w[k]->skip; pad[k] = (16 - ((u64)w[k]->skip & 15)) & 15; eof[k] = w[k]->eof && !P[k].cut_short;
		if (p->d_buf[k].ensure((size_t)(pad[k] + (u64)P[k].inflated + 16))) return p->fail(BWAGPU_ENOMEM, "hipMalloc failed (BGZF text)");
	}
	FqArgs A;
	u32 tiles = 0; u64 cap_units = 0;
	if (int rc = fq_setup(p, A, nw, len, eof, &tiles, &cap_units)) return rc;
	if (p->d_bzstat.ensure(16)) return p->fail(BWAGPU_ENOMEM, "hipMalloc failed (BGZF status)");
	if (p->hip("memset", hipMemsetAsync(p->d_bzstat.p, 0, 16, p->st))) return BWAGPU_EHIP;
	for (int k = 0; k < nw; ++k) if (int rc = bz_upload(p, k, (const u8*)w[k]->comp, P[k], pad[k])) return rc;
	(void)hipEventRecord(p->ev[4], p->st);
	for (int k = 0; k < nw; ++k) {
		bz_launch(p, k, P[k], p->d_buf[k].as<u8>());
		A.w[k].buf = p->d_buf[k].as<u8>() + pad[k] + (u64)w[k]->skip;
	}
	(void)hipEventRecord(p->ev[5], p->st);
	u64 bad[2] = { 0, 0 };
	// the wait for the inflate's verdict
	if (p->hip("read back the verdict", hipMemcpyAsync(bad, p->d_bzstat.p, 16, hipMemcpyDeviceToHost, p->st)) || p->hip("sync", hipStreamSynchronize(p->st)) ||
		p->hip("BGZF kernel", hipGetLastError())) return BWAGPU_EHIP;
	{ float ms = 0; if (hipEventElapsedTime(&ms, p->ev[4], p->ev[5]) == hipSuccess) info[0].inflate_ms = info[1].inflate_ms = ms; }
	bool damaged = false;
	for (int k = 0; k < nw; ++k) { info[k].damaged_at = bz_damage(p, P[k], bad[k]); damaged = damaged || info[k].damaged_at >= 0; info[k].next_coff = 0; info[k].next_uoff = w[k]->skip; }
	if (damaged) { *status = BWAGPU_FQ_DAMAGED; return 0; }
	if (int rc = run(A, tiles, cap_units)) return rc;
	if (*status == BWAGPU_FQ_CUT || *status == BWAGPU_FQ_END)
		for (int k = 0; k < nw; ++k) {
			const u64 t = (u64)w[k]->skip + (u64)consumed[k];
			info[k].next_coff = P[k].used; info[k].next_uoff = 0;
			// the first block whose text reaches beyond t (empty blocks at t are stepped over)
			size_t lo = 0, hi = P[k].blk.size();
			while (lo < hi) { const size_t m = (lo + hi) >> 1; if (P[k].blk[m].out + P[k].blk[m].isize > t) hi = m; else lo = m + 1; }
			if (lo < P[k].blk.size()) { info[k].next_coff = P[k].coff[lo]; info[k].next_uoff = (int32_t)(t - P[k].blk[lo].out); }
		}
	return 0;
}

// bwagpu_fastq_batch_bgzf and bwagpu_fastq_batch_fasta_bgzf
static int fq_batch_bgzf(bwagpu_fastq_parser_t *p, const char *what, bool fasta, const bwagpu_bgzf_win_t *w1, const bwagpu_bgzf_win_t *w2, int chunk_size,
						 bwagpu_fastq_out_t *out, bwagpu_bgzf_info_t info[2])
{
	if (!p) return BWAGPU_EINVAL;
	const bwagpu_bgzf_win_t *w[2] = { w1, w2 };
	const int nw = w2 ? 2 : 1;
	bool ok = w1 && out && info && chunk_size > 0;
	for (int k = 0; ok && k < nw; ++k) ok = w[k]->comp && w[k]->comp_len >= 0 && w[k]->skip >= 0;
	if (!ok) return p->fail(BWAGPU_EINVAL, std::string(what) + ": NULL argument, negative length or skip, or chunk_size <= 0");
	memset(out, 0, sizeof *out);
	out->declined_file = -1; out->declined_at = -1;
	p->err.clear();
	return bz_batch(p, w, nw, info, &out->status, out->consumed, [&](const FqArgs &A, u32 tiles, u64 cap_units) {
		if (!fasta) return fq_run(p, A, tiles, cap_units, chunk_size, out);
		FqArgs B = A; FrArgs X;
		if (int rc = fr_setup(p, B, X, &cap_units)) return rc;
		return fq_run(p, B, tiles, cap_units, chunk_size, out, &X);
	});
}

extern "C" int bwagpu_fastq_batch_bgzf(bwagpu_fastq_parser_t *p, const bwagpu_bgzf_win_t *w1, const bwagpu_bgzf_win_t *w2, int chunk_size,
									   bwagpu_fastq_out_t *out, bwagpu_bgzf_info_t info[2])
{
	return fq_batch_bgzf(p, "bwagpu_fastq_batch_bgzf", false, w1, w2, chunk_size, out, info);
}

extern "C" int bwagpu_fastq_batch_fasta_bgzf(bwagpu_fastq_parser_t *p, const bwagpu_bgzf_win_t *w1, const bwagpu_bgzf_win_t *w2, int chunk_size,
											 bwagpu_fastq_out_t *out, bwagpu_bgzf_info_t info[2])
{
	return fq_batch_bgzf(p, "bwagpu_fastq_batch_fasta_bgzf", true, w1, w2, chunk_size, out, info);
}

// ---- one window of interleaved reads -> single reads and pairs (dev_fastq_smart.h) ------------------------------------------------
extern "C" void bwagpu_fastq_smart_free(bwagpu_fastq_smart_t *o)
{
	if (!o) return;
	bwagpu_free(o->cls); o->cls = nullptr;
	for (int k = 0; k < 2; ++k) { bwagpu_free(o->idx[k]); o->idx[k] = nullptr; bwagpu_fastq_out_free(&o->sub[k]); }
}

static void fqs_init(bwagpu_fastq_smart_t *out)
{
	memset(out, 0, sizeof *out);
	out->declined_at = -1;
	for (int k = 0; k < 2; ++k) { out->sub[k].declined_file = -1; out->sub[k].declined_at = -1; }
}

// fq_run for one window, with passes 5 to 7 in the place of pass 4
static int fqs_run(bwagpu_fastq_parser_t *p, const FqArgs &A, u32 tiles, u64 cap_units, int chunk_size, bwagpu_fastq_smart_t *out)
{
	if (p->d_eqv.ensure(cap_units * 4) || p->d_runs.ensure(cap_units * 4) || p->d_cls.ensure(cap_units) || p->d_sums.ensure(cap_units * sizeof(FqsSum)) ||
		p->d_sscan.ensure(cap_units * sizeof(FqsSum))) return p->fail(BWAGPU_ENOMEM, "hipMalloc failed (FASTQ classification)");
	if (int rc = fq_launch(p, A, tiles, cap_units, chunk_size)) return rc;
	FqInfo *d_info = (FqInfo*)(p->d_words.as<u64>() + FQ_N_WORDS);
	u32 *eqv = p->d_eqv.as<u32>(), *runs = p->d_runs.as<u32>();
	FqsSum *sums = p->d_sums.as<FqsSum>(), *sscan = p->d_sscan.as<FqsSum>();
	const unsigned ugrid = grid_for(cap_units) < 1024 ? grid_for(cap_units) : 1024;
	hipLaunchKernelGGL(k_fqs_eq, dim3(ugrid), dim3(FQ_BLOCK), 0, p->st, A, (const FqInfo*)d_info, eqv);
	if (int rc = p->scan_incl(eqv, runs, cap_units, rocprim::maximum<u32>())) return rc;
	hipLaunchKernelGGL(k_fqs_class, dim3(ugrid), dim3(FQ_BLOCK), 0, p->st, A, (const FqInfo*)d_info, (const u32*)runs, p->d_cls.as<u8>(), sums);
	if (int rc = p->scan_incl(sums, sscan, cap_units, FqsPlus())) return rc;
	(void)hipEventRecord(p->ev[6], p->st);
	FqInfo info; FqsSum tot;
	// wait 1: status, batch size, total sizes -- and the sub-batches' (entries past the batch add nothing: the scan's last element)
	if (p->hip("read back the batch's sizes", hipMemcpyAsync(&info, d_info, sizeof info, hipMemcpyDeviceToHost, p->st)) ||
		p->hip("read back the sub-batches' sizes", hipMemcpyAsync(&tot, sscan + (cap_units - 1), sizeof tot, hipMemcpyDeviceToHost, p->st)) || p->hip("sync", hipStreamSynchronize(p->st))) return BWAGPU_EHIP;
	if (p->hip("FASTQ kernels", hipGetLastError())) return BWAGPU_EHIP;
	{
		float ms = 0;
		if (hipEventElapsedTime(&ms, p->ev[0], p->ev[1]) == hipSuccess) out->kernel_ms[0] = ms;
		if (hipEventElapsedTime(&ms, p->ev[1], p->ev[2]) == hipSuccess) out->kernel_ms[1] = ms;
		if (hipEventElapsedTime(&ms, p->ev[2], p->ev[6]) == hipSuccess) out->kernel_ms[2] = ms;
	}
	out->status = (int32_t)info.status;
	if (info.status == BWAGPU_FQ_DECLINED) { out->declined_at = info.declined_at; return 0; }
	if (info.status == BWAGPU_FQ_MORE) return 0;
	const u64 n_reads = (u64)info.n_units;
	if (n_reads >= (1ull << 31)) return p->fail(BWAGPU_EUNSUP, "a batch of 2^31 reads or more");
	if ((u64)tot.n[0] + tot.n[1] != n_reads || (u64)tot.seq[0] + tot.seq[1] != info.total.seq || (u64)tot.name[0] + tot.name[1] != info.total.name ||
		(u64)tot.com[0] + tot.com[1] != info.total.com || (tot.n[1] & 1)) return p->fail(BWAGPU_EHIP, "internal: the sub-batches do not add up to the batch");
	out->n_reads = (int32_t)n_reads; out->consumed = info.consumed[0];
	out->sub[0].status = out->sub[1].status = out->status;
	int rc = 0;
	out->cls = (uint8_t*)bwagpu_alloc_host(n_reads + 1);
	if (!out->cls) rc = p->fail(BWAGPU_ENOMEM, "out of host memory (FASTQ batch)");
	// device side: sub-batch 1's arrays lie behind sub-batch 0's in the parser's output buffers
	const u64 ts = info.total.seq, tn = info.total.name, tc = info.total.com;
	if (!rc && (p->o_seqs.ensure(ts + 1) || p->o_quals.ensure(ts + 1) || p->o_names.ensure(tn + 1) || p->o_com.ensure(tc + 1) || p->o_off.ensure((n_reads + 2) * 8) ||
				p->o_name_off.ensure((n_reads + 2) * 8) || p->o_com_off.ensure((n_reads + 2) * 8) || p->o_has.ensure(n_reads + 1) || p->o_recs.ensure((n_reads + 1) * sizeof(bwagpu_fastq_rec_t)) ||
				p->o_idx.ensure((n_reads + 1) * 4))) rc = p->fail(BWAGPU_ENOMEM, "hipMalloc failed (FASTQ outputs)");
	FqsOut O; memset(&O, 0, sizeof O);
	for (int k = 0; !rc && k < 2; ++k) {
		bwagpu_fastq_out_t &s = out->sub[k];
		const u64 m = tot.n[k], b_seq = k ? tot.seq[0] : 0, b_name = k ? tot.name[0] : 0, b_com = k ? tot.com[0] : 0, b_n = k ? tot.n[0] : 0;
		out->n_sub[k] = s.n_reads = (int32_t)m;
		out->idx[k] = (int32_t*)bwagpu_alloc_host((m + 1) * 4);
		s.seqs = (uint8_t*)bwagpu_alloc_host((u64)tot.seq[k] + 1); s.off = (int64_t*)bwagpu_alloc_host((m + 1) * 8);
		s.names = (char*)bwagpu_alloc_host((u64)tot.name[k] + 1); s.name_off = (int64_t*)bwagpu_alloc_host((m + 1) * 8);
		s.quals = (char*)bwagpu_alloc_host((u64)tot.seq[k] + 1);
		s.comments = (char*)bwagpu_alloc_host((u64)tot.com[k] + 1); s.comment_off = (int64_t*)bwagpu_alloc_host((m + 1) * 8);
		s.has_comment = (uint8_t*)bwagpu_alloc_host(m + 1); s.recs = (bwagpu_fastq_rec_t*)bwagpu_alloc_host((m + 1) * sizeof(bwagpu_fastq_rec_t));
		if (!out->idx[k] || !s.seqs || !s.off || !s.names || !s.name_off || !s.quals || !s.comments || !s.comment_off || !s.has_comment || !s.recs) { rc = p->fail(BWAGPU_ENOMEM, "out of host memory (FASTQ batch)"); break; }
		s.off[0] = s.name_off[0] = s.comment_off[0] = 0;      // (an empty sub-batch: nothing else comes down)
		FqOut &o = O.sub[k];
		o.seqs = p->o_seqs.as<u8>() + b_seq; o.quals = p->o_quals.as<char>() + b_seq; o.names = p->o_names.as<char>() + b_name; o.comments = p->o_com.as<char>() + b_com;
		o.off = p->o_off.as<i64>() + b_n + k; o.name_off = p->o_name_off.as<i64>() + b_n + k; o.comment_off = p->o_com_off.as<i64>() + b_n + k;
		o.has_comment = p->o_has.as<u8>() + b_n; o.recs = p->o_recs.as<bwagpu_fastq_rec_t>() + b_n; O.idx[k] = p->o_idx.as<int32_t>() + b_n;
	}
	if (!rc && n_reads) {
		const u64 eblocks = (n_reads + FQ_BLOCK / FQ_WAVE - 1) / (FQ_BLOCK / FQ_WAVE);
		hipLaunchKernelGGL(k_fqs_emit, dim3((unsigned)(eblocks < 65536 ? eblocks : 65536)), dim3(FQ_BLOCK), 0, p->st, A, (const u8*)p->d_cls.as<u8>(), (const FqsSum*)sscan, n_reads, tot, O);
		(void)hipEventRecord(p->ev[3], p->st);
		auto down = [&](void *dst, const void *src, u64 bytes) { return bytes ? p->hip("download", hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, p->st)) : 0; };
		bool bad = down(out->cls, p->d_cls.p, n_reads) != 0;
		for (int k = 0; !bad && k < 2; ++k) {
			const bwagpu_fastq_out_t &s = out->sub[k]; const FqOut &o = O.sub[k];
			const u64 m = tot.n[k];
			if (!m) continue;
			bad = down(s.seqs, o.seqs, tot.seq[k]) || down(s.quals, o.quals, tot.seq[k]) || down(s.names, o.names, tot.name[k]) || down(s.comments, o.comments, tot.com[k]) ||
				  down(s.off, o.off, (m + 1) * 8) || down(s.name_off, o.name_off, (m + 1) * 8) || down(s.comment_off, o.comment_off, (m + 1) * 8) ||
				  down(s.has_comment, o.has_comment, m) || down(s.recs, o.recs, m * sizeof(bwagpu_fastq_rec_t)) || down(out->idx[k], O.idx[k], m * 4);
		}
		// wait 2: the copies
		if (bad || p->hip("sync", hipStreamSynchronize(p->st)) || p->hip("FASTQ emit kernel", hipGetLastError())) rc = BWAGPU_EHIP;
		else { float ms = 0; if (hipEventElapsedTime(&ms, p->ev[6], p->ev[3]) == hipSuccess) out->kernel_ms[3] = ms; }
	}
	if (rc) { bwagpu_fastq_smart_free(out); fqs_init(out); }
	return rc;
}

extern "C" int bwagpu_fastq_batch_smart(bwagpu_fastq_parser_t *p, const void *raw, int64_t len, int eof, int chunk_size, bwagpu_fastq_smart_t *out)
{
	if (!p) return BWAGPU_EINVAL;
	if (!out || !raw || len < 0 || len >= ((int64_t)1 << 31) || chunk_size <= 0)
		return p->fail(BWAGPU_EINVAL, "bwagpu_fastq_batch_smart: NULL argument, negative length, window of 2^31 bytes or more, or chunk_size <= 0");
	fqs_init(out);
	p->err.clear();
	if (hipSetDevice(p->device) != hipSuccess) return p->fail(BWAGPU_ENODEV, "hipSetDevice failed");
	FqArgs A;
	const u64 lens[2] = { (u64)len, 0 }; const int eofs[2] = { eof, 1 };
	u32 tiles = 0; u64 cap_units = 0;
	if (int rc = fq_setup(p, A, 1, lens, eofs, &tiles, &cap_units)) return rc;
	if (len && p->hip("copy window", hipMemcpyAsync(p->d_buf[0].p, raw, (size_t)len, hipMemcpyHostToDevice, p->st))) return BWAGPU_EHIP;
	return fqs_run(p, A, tiles, cap_units, chunk_size, out);
}

extern "C" int bwagpu_fastq_batch_smart_bgzf(bwagpu_fastq_parser_t *p, const bwagpu_bgzf_win_t *w1, int chunk_size, bwagpu_fastq_smart_t *out, bwagpu_bgzf_info_t *info)
{
	if (!p) return BWAGPU_EINVAL;
	if (!(w1 && out && info && chunk_size > 0 && w1->comp && w1->comp_len >= 0 && w1->skip >= 0))
		return p->fail(BWAGPU_EINVAL, "bwagpu_fastq_batch_smart_bgzf: NULL argument, negative length or skip, or chunk_size <= 0");
	fqs_init(out);
	p->err.clear();
	const bwagpu_bgzf_win_t *w[2] = { w1, nullptr };
	bwagpu_bgzf_info_t both[2]; memset(both, 0, sizeof both);
	int64_t consumed[2] = { 0, 0 };
	const int rc = bz_batch(p, w, 1, both, &out->status, consumed, [&](const FqArgs &A, u32 tiles, u64 cap_units) {
		const int r = fqs_run(p, A, tiles, cap_units, chunk_size, out);
		consumed[0] = out->consumed;
		return r;
	});
	*info = both[0];
	return rc;
}
