// dev_debug.h -- bwagpu_debug_dp: one wavefront of a device DP routine on caller-supplied sequences (differential tests); bwagpu_debug_sort (at the
// end): the device's restatements of ks_introsort on caller-supplied keys.
//
// The whole-read parity tests feed the DP routines a narrow distribution of (h0, band, lengths); this entry lets a test drive
// wave_ksw_extend2 (k_extend_wave, both modes), wave_ksw_global2 (k_cigar), wave_global2_score_ring (k_dedup_wave) and the
// ksw_align2 restatement of k_matesw_sw with adversarial inputs and compare them with the reference's exported ksw_extend2
// (ksw.c:416), ksw_global2 (ksw.c:540) and ksw_align2 (ksw.c:379).  The routines read their target from 2-bit packed reference
// text (ref_base), so the caller's sequence array is packed into a scratch "pac" and the kernels run on a DevIndex that points
// at it; everything else is the product code, called exactly as the product kernels call it.
#pragma once
#include "dev_extw.h"
#include "dev_extp.h"
#include "dev_cigar.h"
#include "dev_dedupw.h"
#include "dev_matesw.h"
#include "dev_seed.h"
#include "dev_chainw.h"

#define DBG_OUT_INTS 72

DEVFN void dbg_case_geometry(const bwagpu_dp_case_t &c, i64 l_pac, int &q0, int &qdir, i64 &t0, int &tdir)
{
	q0 = (c.flags & 1) ? c.q_len - 1 : 0; qdir = (c.flags & 1) ? -1 : 1;       // bit 0: the query is presented back to front
	if (c.flags & 4) {                                                        // bit 2: the target's complement, through the reverse-strand half of the text
		if (c.flags & 2) { t0 = (l_pac << 1) - 1 - c.t_off; tdir = -1; }       //   ... read back to front at that (complement of the reversed target)
		else { t0 = (l_pac << 1) - 1 - (c.t_off + c.t_len - 1); tdir = 1; }
	} else if (c.flags & 2) { t0 = c.t_off + c.t_len - 1; tdir = -1; }         // bit 1: the target is presented back to front
	else { t0 = c.t_off; tdir = 1; }
}

// kind 0 / 1: wave_ksw_extend2 as k_extend_wave sets it up (columns + read profile in LDS / ring mode)
template <bool RING> __global__ void __launch_bounds__(64) k_debug_extend(DevIndex ix, bwagpu_opt_t opt, int n_cases, const bwagpu_dp_case_t *cases, const u8 *seqs,
																			 int max_q, int ring_cols, i32 *out, int blk)
{
	HIP_DYNAMIC_SHARED(unsigned char, dbg_lds)
	const int lane = threadIdx.x & 63;
	WaveLds L;
	L.stat = nullptr; L.blk = RING ? blk : 0;
	L.eh = (int2*)dbg_lds;
	if (RING) {
		int8_t *m = (int8_t*)(dbg_lds + (size_t)8 * ring_cols);
		if (lane < 25) m[lane] = opt.mat[lane];
		L.mat = m; L.ring_mask = ring_cols - 1; L.qp = nullptr; L.qstride = 0;
	} else {
		L.qstride = (max_q + 64 + 3) & ~3;
		L.qp = (int8_t*)(dbg_lds + (size_t)8 * (max_q + 2 + 64));
		int8_t *m = L.qp + 5 * L.qstride;
		if (lane < 25) m[lane] = opt.mat[lane];
		L.mat = m; L.ring_mask = 0;
	}
	wave_sync();
	const int mat_max = opt_mat_max(opt);
	for (int k = blockIdx.x; k < n_cases; k += gridDim.x) {
		const bwagpu_dp_case_t c = cases[k];
		const u8 *q = seqs + c.q_off;
		int q0, qdir, tdir; i64 t0;
		dbg_case_geometry(c, ix.l_pac, q0, qdir, t0, tdir);
		if (!RING) {      // the read's profile (ext_read_wave builds it once per read)
			for (int j = lane; j < c.q_len; j += 64) { const int qc = q[j]; for (int b = 0; b < 5; ++b) L.qp[b * L.qstride + j] = L.mat[b * 5 + qc]; }
			wave_sync();
		}
		u64 cells = 0, fast = 0;
		const ExtRes r = wave_ksw_extend2<RING>(ix, opt, mat_max, q, q0, qdir, c.q_len, t0, tdir, c.t_len, c.w, c.end_bonus, c.h0, L, cells, fast);
		wave_sync();
		if (lane == 0) {
			i32 *o = out + (size_t)k * DBG_OUT_INTS;
			o[0] = r.score; o[1] = r.qle; o[2] = r.tle; o[3] = r.gtle; o[4] = r.gscore; o[5] = r.max_off; o[6] = (i32)fast; o[7] = (i32)cells;
		}
	}
}

// kind 6 / 7: the packed extension routine of k_ext_pack (dev_extp.h), four cases per wavefront, four / eight columns per lane.  out[0..5] as kind 0,
// out[6]: answered by the diagonal rule, out[7]: 1 = the routine vouches for the result (0: outside its conditions -- the product then runs kind 0's routine)
template <int CPL> __global__ void __launch_bounds__(64) k_debug_extpack(DevIndex ix, bwagpu_opt_t opt, int n_cases, const bwagpu_dp_case_t *cases, const u8 *seqs, i32 *out)
{
	HIP_DYNAMIC_SHARED(unsigned char, dbg_lds)
	const int lane = threadIdx.x & 63, grp = lane >> 4;
	int8_t *mat = (int8_t*)dbg_lds;
	if (lane < 25) mat[lane] = opt.mat[lane];
	wave_sync();
	PackConst C;
	C.o_del = opt.o_del; C.e_del = opt.e_del; C.o_ins = opt.o_ins; C.e_ins = opt.e_ins; C.oe_del = opt.o_del + opt.e_del; C.oe_ins = opt.o_ins + opt.e_ins;
	C.zdrop = opt.zdrop; C.mat = mat; C.prof = (int8_t*)(dbg_lds + 32); C.mat_max = opt_mat_max(opt);
	for (int base = blockIdx.x * 4; base < n_cases; base += gridDim.x * 4) {
		const int k = base + grp;
		PackState<CPL> S;
		#pragma unroll
		for (int c = 0; c < CPL; ++c) { S.H[c] = 0; S.E[c] = 0; }
		S.run = 0; S.done = 0; S.valid = 0; S.i = 0; S.end = 0; S.qlen = 1; S.tlen = 0; S.w = 0; S.h0 = 1; S.max = 0; S.max_i = S.max_j = S.max_ie = -1; S.gscore = -1; S.max_off = 0;
		S.tdir = 1; S.t0 = 0; S.tpack = 0; S.tnext = 0; S.lq = 0; S.sq = 0;
		u64 fast = 0;
		{
			const bwagpu_dp_case_t c = cases[k < n_cases ? k : n_cases - 1];
			PackTask T;
			T.q = seqs + c.q_off; T.qlen = c.q_len; T.tlen = c.t_len; T.w = c.w; T.end_bonus = c.end_bonus; T.h0 = c.h0;
			dbg_case_geometry(c, ix.l_pac, T.q0, T.qdir, T.t0, T.tdir);
			pack_init<CPL>(ix, C, T, S, k < n_cases, fast);
		}
		while (__ballot(S.run != 0)) pack_row<CPL, true>(ix, C, S);
		if (k < n_cases && (lane & 15) == 0) {
			const ExtRes r = pack_result(S);
			i32 *o = out + (size_t)k * DBG_OUT_INTS;
			o[0] = r.score; o[1] = r.qle; o[2] = r.tle; o[3] = r.gtle; o[4] = r.gscore; o[5] = r.max_off; o[6] = (i32)fast; o[7] = S.valid;
		}
		wave_sync();
	}
}

// kind 2: wave_ksw_global2 with traceback as k_cigar sets it up (second tier's LDS); out: score, n_ops (-1: more than 64, -2: outside
// the kernel's limits), then the operations in alignment order
__global__ void __launch_bounds__(64) k_debug_global(DevIndex ix, bwagpu_opt_t opt, int n_cases, const bwagpu_dp_case_t *cases, const u8 *seqs, i32 *out)
{
	HIP_DYNAMIC_SHARED(unsigned char, dbg_lds)
	const int lane = threadIdx.x & 63;
	CigLds L;
	L.hd = (i32*)dbg_lds; L.e = L.hd + (CIG_MAX_LEN + 2 + 64);
	L.qstride = CIG_MAX_LEN + 64; L.z_cells = CIG_Z_BIG;
	L.qp = (int8_t*)(L.e + (CIG_MAX_LEN + 2 + 64));
	L.z = (u8*)(L.qp + 5 * L.qstride);
	L.ops = (u32*)(L.z + CIG_Z_BIG / 2 + CIG_MAX_COLS);
	L.md = (u8*)(L.ops + CIG_TMP_OPS);
	for (int k = blockIdx.x; k < n_cases; k += gridDim.x) {
		const bwagpu_dp_case_t c = cases[k];
		const u8 *q = seqs + c.q_off;
		int q0, qdir, tdir; i64 t0;
		dbg_case_geometry(c, ix.l_pac, q0, qdir, t0, tdir);
		i32 *o = out + (size_t)k * DBG_OUT_INTS;
		const int n_col = c.q_len < 2 * c.w + 1 ? c.q_len : 2 * c.w + 1;
		if (c.q_len > CIG_MAX_LEN || c.t_len > CIG_MAX_LEN || n_col > CIG_MAX_COLS || n_col * ((c.t_len + 1) & ~1) > CIG_Z_BIG) { if (lane == 0) { o[0] = 0; o[1] = -2; } continue; }
		int n_ops = 0;
		const int score = wave_ksw_global2(ix, opt, q, q0, qdir, c.q_len, t0, tdir, c.t_len, c.w, L, &n_ops);
		if (lane == 0) { o[0] = score; o[1] = n_ops; for (int j = 0; j < n_ops; ++j) o[2 + j] = (i32)L.ops[n_ops - 1 - j]; }
		wave_sync();
	}
}

// kind 3: the score-only ring form of k_dedup_wave
template <bool BLK = false> __global__ void __launch_bounds__(64) k_debug_global_ring(DevIndex ix, bwagpu_opt_t opt, int n_cases, const bwagpu_dp_case_t *cases, const u8 *seqs, int ring_cols, i32 *out, int q_cap)
{
	HIP_DYNAMIC_SHARED(unsigned char, dbg_lds)
	const int lane = threadIdx.x & 63;
	DedupLds L;
	L.hd = (i32*)dbg_lds; L.e = L.hd + ring_cols; L.ring_mask = ring_cols - 1; L.H = nullptr; L.E = nullptr; L.qbuf = dbg_lds + (size_t)8 * ring_cols + 32; L.qcap = q_cap;
	int8_t *m = (int8_t*)(dbg_lds + (size_t)8 * ring_cols);
	if (lane < 25) m[lane] = opt.mat[lane];
	L.mat = m;
	wave_sync();
	for (int k = blockIdx.x; k < n_cases; k += gridDim.x) {
		const bwagpu_dp_case_t c = cases[k];
		int q0, qdir, tdir; i64 t0;
		dbg_case_geometry(c, ix.l_pac, q0, qdir, t0, tdir);
		i32 *o = out + (size_t)k * DBG_OUT_INTS;
		if (2 * c.w + 4 + 128 > ring_cols) { if (lane == 0) { o[0] = 0; o[1] = -2; } continue; }
		u64 cells = 0;
		const int score = BLK && L.qcap >= c.q_len ? wave_global2_score_ring_blk(ix, opt, seqs + c.q_off, q0, qdir, c.q_len, t0, tdir, c.t_len, c.w, L, cells)
													   : wave_global2_score_ring(ix, opt, seqs + c.q_off, q0, qdir, c.q_len, t0, tdir, c.t_len, c.w, L, cells);
		if (lane == 0) { o[0] = score; o[1] = 0; o[7] = (i32)cells; }
		wave_sync();
	}
}

// kind 4: ksw_align2 as k_matesw_sw runs it (one wavefront per case; h0 carries the xtra word); out: score, te, qe, score2, te2, tb, qb
__global__ void __launch_bounds__(64) k_debug_align2(DevIndex ix, bwagpu_opt_t opt, int n_cases, const bwagpu_dp_case_t *cases, const u8 *seqs, i32 *out)
{
	__shared__ i32 dbg_runs[MSW_RUN_INTS];
	const int lane = threadIdx.x & 63;
	for (int k = blockIdx.x; k < n_cases; k += gridDim.x) {
		const bwagpu_dp_case_t c = cases[k];
		i32 *o = out + (size_t)k * DBG_OUT_INTS;
		if (c.q_len > MSW_MAX_Q || c.t_len > MSW_MAX_T) { if (lane == 0) { o[0] = 0; o[1] = -2; } continue; }
		const u8 *q = seqs + c.q_off;
		int q0, qdir, tdir; i64 t0;
		dbg_case_geometry(c, ix.l_pac, q0, qdir, t0, tdir);
		auto Qf = [&](int j) -> int { return (int)q[q0 + j * qdir]; };
		auto Tf = [&](int i) -> int { return ref_base(ix, t0 + (i64)i * tdir); };
		int res[7];
		msw_align2(opt, c.q_len, Qf, c.t_len, Tf, c.h0, dbg_runs, res);
		if (lane == 0) for (int j = 0; j < 7; ++j) o[j] = res[j];
		wave_sync();
	}
}

// kind 5: wave_ksw_global2_long as k_cigar_long sets it up; out: score, n_ops (-1: too many, -2: outside the limits), the first 70 operations
__global__ void __launch_bounds__(64) k_debug_global_long(DevIndex ix, bwagpu_opt_t opt, int n_cases, const bwagpu_dp_case_t *cases, const u8 *seqs, u8 *z_all, i64 z_cap, u32 *ops_all, i32 *out)
{
	HIP_DYNAMIC_SHARED(unsigned char, dbg_lds)
	const int lane = threadIdx.x & 63;
	CigLongLds L;
	cigl_lds_setup(dbg_lds, L);
	if (lane < 25) L.mat[lane] = opt.mat[lane];
	CigLongScratch S;
	S.z = z_all + (i64)blockIdx.x * z_cap; S.z_cap = z_cap; S.ops = ops_all + (size_t)blockIdx.x * CIGL_MAX_OPS; S.md = nullptr;
	wave_sync();
	for (int k = blockIdx.x; k < n_cases; k += gridDim.x) {
		const bwagpu_dp_case_t c = cases[k];
		int q0, qdir, tdir; i64 t0;
		dbg_case_geometry(c, ix.l_pac, q0, qdir, t0, tdir);
		i32 *o = out + (size_t)k * DBG_OUT_INTS;
		const int n_col = c.q_len < 2 * c.w + 1 ? c.q_len : 2 * c.w + 1;
		if (n_col > CIGL_MAX_COLS || (i64)c.t_len * ((n_col + 15) & ~15) > z_cap) { if (lane == 0) { o[0] = 0; o[1] = -2; } continue; }
		int n_ops = 0;
		const int score = wave_ksw_global2_long(ix, opt, seqs + c.q_off, q0, qdir, c.q_len, t0, tdir, c.t_len, c.w, L, S, &n_ops);
		if (lane == 0) { o[0] = score; o[1] = n_ops; for (int j = 0; j < n_ops && j < DBG_OUT_INTS - 2; ++j) o[2 + j] = (i32)S.ops[n_ops - 1 - j]; }
		wave_sync();
	}
}

// 2-bit packing of the case array's bases (codes > 3 are stored as their low two bits: targets hold 0..3 only)
__global__ void __launch_bounds__(256) k_debug_pack(const u8 *seqs, i64 n, u8 *pac)
{
	for (i64 b = (i64)blockIdx.x * blockDim.x + threadIdx.x; b < (n + 3) / 4; b += (i64)gridDim.x * blockDim.x) {
		u32 v = 0;
		for (int k = 0; k < 4; ++k) { const i64 l = b * 4 + k; const u32 c = l < n ? seqs[l] & 3u : 0u; v |= c << ((3 - k) << 1); }   // _set_pac (bntseq.c:229)
		pac[b] = (u8)v;
	}
}

// ---- bwagpu_debug_sort: every form in which the device restates ks_introsort (ksort.h:176-226), on caller-supplied keys ---------------------------
// BWA-MEM's output depends on the tie behaviour of that unstable sort, and several of the forms below are not its sequence of steps but an argument
// that the result is the same; whole reads feed them only the key distributions that reads happen to produce (the depth limit's comb sort needs an
// adversarial arrangement to run at all).  Each kernel calls the product's routine where the product calls it, with the arrays in the memory the product
// keeps them in, and returns the permutation it produced: perm[place] = the element's index in the case.
#define DBG_SORT_U64 0          // dev_ext.h's seed order: one lane's introsort of score << 32 | index
#define DBG_SORT_CHAIN_SEEDS 1  // chain_sort_wave (dev_extw.h): lane 0's introsort up to 32 seeds, wave_sort_u64 above
#define DBG_SORT_INTV 2         // k_publish: one lane's introsort of Intv3 records by info
#define DBG_SORT_INTV_BLK 3     // k_publish_blk: the workgroup's network up to PUB_MAX intervals, one lane's introsort above
#define DBG_SORT_CHAIN_W 4      // k_chain_wave: quicksort passes over {weight, index} pairs in LDS or HBM, the stable finish by counting
#define DBG_SORT_REG_END 5      // k_dedup: one lane's sort of the 88-byte records (fewer than DEDUP_KEYSORT_MIN) or of their RegKey records, by end
#define DBG_SORT_REG_BEST 6     //          ... by score, rb, qb
#define DBG_SORT_PAR_END 7      // dedup_read_par: passes over DdKey in LDS, finish by counting or by the network (dd_net, par_cap), by end
#define DBG_SORT_PAR_BEST 8     //          ... by score, rb, qb
#define DBG_SORT_PAR_CAP_MAX 1100     // (DDP_LDS_PER_REG bytes of LDS each: within the 64 KB a launch gets without asking for more)

// kinds 0, 2, 5, 6: a lane per case, as the product's lane-per-read kernels run these sorts (all arrays in HBM)
template <int KIND> __global__ void __launch_bounds__(256) k_debug_sort_lane(int n_cases, const bwagpu_sort_key_t *keys, const i64 *off, u64 *srt_all, Intv3 *iv_all,
																			 bwagpu_alnreg_t *reg_all, RegKey *rk_all, i32 *perm, i32 *status)
{
	for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n_cases; k += gridDim.x * blockDim.x) {
		const i64 o = off[k]; const int n = (int)(off[k + 1] - o);
		const bwagpu_sort_key_t *kk = keys + o; i32 *pm = perm + o;
		if (KIND == DBG_SORT_U64) {
			u64 *srt = srt_all + o;
			for (int i = 0; i < n; ++i) { bwagpu_seed_t s_; s_.rbeg = kk[i].a; s_.qbeg = kk[i].c; s_.len = 0; s_.score = kk[i].b; srt[i] = seed_order_key(s_, i); }   // dev_ext.h: the seeds by score
			dev_introsort(srt, n, U64Less());
			for (int i = 0; i < n; ++i) pm[i] = (i32)(u32)srt[i];
		} else if (KIND == DBG_SORT_INTV) {
			Intv3 *iv = iv_all + o;
			for (int i = 0; i < n; ++i) { iv[i].x0 = (u64)i; iv[i].x2 = 0; iv[i].info = (u64)kk[i].a; }
			if (n > 0) dev_introsort(iv, n, IntvInfoLess());
			for (int i = 0; i < n; ++i) pm[i] = (i32)iv[i].x0;
		} else {
			bwagpu_alnreg_t *a = reg_all + o;
			for (int i = 0; i < n; ++i) {
				bwagpu_alnreg_t g; memset(&g, 0, sizeof g);
				g.rb = kk[i].a; g.re = kk[i].a; g.score = kk[i].b; g.qb = kk[i].c; g.qe = kk[i].c + 1; g.seedlen0 = i;
				a[i] = g;
			}
			if (n > 1) dedup_sort_regs<KIND == DBG_SORT_REG_BEST>(a, n, n >= DEDUP_KEYSORT_MIN ? rk_all + o : nullptr);     // (dedup_read: n > 1)
			for (int i = 0; i < n; ++i) pm[i] = a[i].seedlen0;
		}
		status[k] = 0;
	}
}

// kinds 1, 4, 7, 8: a wavefront per case
template <int KIND> __global__ void __launch_bounds__(64) k_debug_sort_wave(int n_cases, const bwagpu_sort_key_t *keys, const i64 *off, bwagpu_seed_t *seed_all, u64 *srt_all, i32 *ord_all,
																			int dd_net, int par_cap, int chain_flt_lds, i32 *perm, i32 *status)
{
	HIP_DYNAMIC_SHARED(unsigned char, dbg_lds)
	const int lane = threadIdx.x & 63;
	for (int k = blockIdx.x; k < n_cases; k += gridDim.x) {
		const i64 o = off[k]; const int n = (int)(off[k + 1] - o);
		const bwagpu_sort_key_t *kk = keys + o; i32 *pm = perm + o;
		int st = 0;
		wave_sync();                                             // (the LDS arrays' last readers: the case before)
		if (KIND == DBG_SORT_CHAIN_SEEDS) {
			bwagpu_seed_t *seeds = seed_all + o; u64 *srt = srt_all + o;
			for (int i = lane; i < n; i += 64) { bwagpu_seed_t s_; s_.rbeg = kk[i].a; s_.qbeg = kk[i].c; s_.len = 0; s_.score = kk[i].b; seeds[i] = s_; }
			wave_sync();
			chain_sort_wave(seeds, srt, n);
			wave_sync();
			for (int i = lane; i < n; i += 64) pm[i] = (i32)(u32)srt[i];
		} else if (KIND == DBG_SORT_CHAIN_W) {
			// chain_read_wave's storage: the pairs in the wave's LDS area up to CW_PW_LDS of them, else in HBM; the sorted order in LDS up to chain_flt_lds chains
			int2 *pw = cw_pw_place(n, chain_flt_lds, cw_area(dbg_lds), srt_all + o);
			i32 *sord = cw_sord_place(n, chain_flt_lds, dbg_lds, ord_all + o);
			for (int i = lane; i < n; i += 64) pw[i] = make_int2(kk[i].b, i);
			wave_sync();
			if (n > 0) cw_weight_order(pw, n, sord, lane);        // (chain_read_wave returns before its sort when no chain is left)
			wave_sync();
			for (int i = lane; i < n; i += 64) pm[i] = sord[i];
		} else {
			constexpr bool BEST = KIND == DBG_SORT_PAR_BEST;
			DdHot *hot = (DdHot*)dbg_lds; DdKey *dk = (DdKey*)(hot + par_cap); i32 *ord = (i32*)(dk + par_cap);        // k_dedup_wave's layout: hot, keys, ord, ord2
			if (n > par_cap) st = -2;                              // (k_dedup_wave takes such a read in place)
			else if (n <= 1) { if (lane == 0 && n == 1) pm[0] = 0; }   // (dedup_read_par: nothing to sort)
			else {
				bool odd = false;
				for (int i = lane; i < n; i += 64) {
					DdHot h_; h_.rb = BEST ? kk[i].a : 0; h_.re = BEST ? 0 : kk[i].a; h_.qb = BEST ? kk[i].c : 0; h_.qe = h_.qb + 1; h_.rid = 0; h_.score = kk[i].b;
					hot[i] = h_;
					dk[i] = BEST ? ddp_key_best(h_, i) : ddp_key_end(h_, i);
					odd |= ddp_odd(h_);                             // (rb and qb are the BEST order's: an END case carries its key in re alone)
				}
				if (wave_ballot(odd)) st = 1;
				else {
					wave_sync();
					ddp_order<BEST>(dk, n, ord, dd_net, par_cap + par_cap / 2, lane);
					wave_sync();
					for (int i = lane; i < n; i += 64) pm[i] = ord[i];
				}
			}
		}
		if (lane == 0) status[k] = st;
	}
}

// kind 3: a workgroup of 256 per case
__global__ void __launch_bounds__(256) k_debug_sort_blk(int n_cases, const bwagpu_sort_key_t *keys, const i64 *off, Intv3 *iv_all, Intv3 *tmp_all, i32 *perm, i32 *status)
{
	__shared__ u64 s_key[PUB_MAX];
	__shared__ unsigned short s_idx[PUB_MAX];
	const int tid = threadIdx.x;
	Intv3 *tmp = tmp_all + (size_t)blockIdx.x * PUB_MAX;
	for (int k = blockIdx.x; k < n_cases; k += gridDim.x) {
		const i64 o = off[k]; const int n = (int)(off[k + 1] - o);
		Intv3 *iv = iv_all + o;
		for (int i = tid; i < n; i += blockDim.x) { iv[i].x0 = (u64)i; iv[i].x2 = 0; iv[i].info = (u64)keys[o + i].a; }
		__syncthreads();
		if (n > 0) publish_sort_blk(iv, n, tmp, (size_t)PUB_MAX, s_key, s_idx);      // (k_publish_blk skips a read without intervals)
		__syncthreads();
		for (int i = tid; i < n; i += blockDim.x) perm[o + i] = (i32)iv[i].x0;
		if (tid == 0) status[k] = 0;
		__syncthreads();
	}
}
