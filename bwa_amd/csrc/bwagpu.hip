// bwagpu.hip -- host side of libbwagpu.so: index upload, batch arenas, kernel sequencing, the C-ABI of
// include/bwagpu.h.  Device code lives in the dev_*.h headers included below (one translation unit so that the
// per-lane routines inline into their kernels).
//
// Pipeline of one batch (all on one HIP stream, no host round-trips between stages):
//   k_seed    one lane/read   SMEM seeding (3 passes) -> SA intervals; reserves slot space, B-tree nodes
//   k_sa      one lane/seed   suffix-array lookups (LF walk to a sampled row)
//   k_chain   one lane/read   B-tree chaining, chain weights, chain filter -> kept chains + flattened seeds
//   k_seedsw  one lane/read   (long reads only) mem_flt_chained_seeds: local SW re-scoring of short seeds
//   k_extend  one lane/read   banded extension of seeds (ksw_extend2) -> raw alignment regions
//   k_dedup   one lane/read   sort / redundancy removal / patching (ksw_global2 score) -> final regions
// Arenas are sized from the batch's base count and grown (whole batch re-run) if a stage reports overflow.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <algorithm>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include <chrono>

#include "bwagpu_config.h"
#include "dev_common.h"
#include "dev_fm.h"
#include "dev_sort.h"
#include "dev_seed.h"
#include "dev_chain.h"
#include "dev_chainw.h"
#include "dev_ext.h"
#include "dev_extw.h"
#include "dev_extp.h"
#include "dev_dedup.h"
#include "dev_seedsw.h"
#include "dev_cigar.h"
#include "dev_dedupw.h"
#include "dev_matesw.h"
#include "dev_primary.h"
#include "dev_pair.h"
#include "dev_rescue.h"
#include "dev_pestat.h"
#include "dev_alns.h"
#include "dev_sampe.h"
#include "dev_samtext.h"
#include "dev_samtext_pe.h"
#include "dev_debug.h"

#define BWAGPU_VERSION "bwagpu 0.1 (gfx950)"

// bwagpu_batch_footprint: the allocation code itself run "dry" -- ensure() adds what it would allocate to *g_dry_sum and allocates nothing --, so that the
// estimate cannot drift away from what bwagpu_batch_reserve / alloc_batch really ask for.
static thread_local size_t *g_dry_sum = nullptr;
struct DevBuf {
	void *p = nullptr; size_t cap = 0;
	int ensure(size_t bytes) {
		if (bytes <= cap) return 0;
		if (g_dry_sum) { *g_dry_sum += bytes + (bytes >> 3) + 256 - cap; return 0; }
		if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
		size_t want = bytes + (bytes >> 3) + 256;
		if (hipMalloc(&p, want) != hipSuccess) { p = nullptr; return -1; }
		cap = want;
		return 0;
	}
	void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
	template <class T> T *as() const { return (T*)p; }
};

struct bwagpu_s {
	int device = 0;
	hipStream_t stream = nullptr;
	hipEvent_t ev[8] = {};
	void *reserved[3] = {nullptr, nullptr, nullptr};   // page-locked result blocks of bwagpu_batch_reserve, held until the handle's first download
	hipEvent_t ev_wait = nullptr;    // blocking-sync event: waiting for the stream must not spin on a host core (see wait_stream)
	std::string err;
	BwagpuConfig cfg;               // tuning and test options (bwagpu_config.h): environment read once at creation, then bwagpu_set_option
	// index
	DevIndex ix = {};
	struct IndexBufs {
		DevBuf d_bwt, d_sa, d_pac, d_ctg_off, d_ctg_len, d_ctg_alt, d_ptab, d_occ32, d_occ_sb; std::atomic<int> refs{1};
		std::atomic<int> busy{0};      // handles on this index that are inside a call that launches kernels (share auto)
		// per-base arena needs learnt by any handle on this index (a re-run for arena growth doubles a batch's device time, so a
		// cloned handle should not have to learn them again); written and read under `m`
		std::mutex m; double need_slot = 0, need_node = 0, need_reg = 0; int need_mem = 0;
		long batches = 0, mem_events = 0;      // batches run on this index; those that had to be redone with longer interval lists (see the end of bwagpu_batch_run)
		// contig names and annotations (bwagpu_set_contig_names; from .ann): one blob, names first, and n_seqs + 1 offsets into it for either; the same in HBM
		// (offsets: names', then annotations').  Set before the handles on this index format text.
		std::string ctg_text; std::vector<i64> ctg_name_off, ctg_anno_off; DevBuf d_ctg_text, d_ctg_toff; bool have_names = false;
	};
	IndexBufs *ibuf = nullptr;      // shared by bwagpu_clone()d handles
	i64 l_pac = 0; int n_seqs = 0; u64 seq_len = 0; int sa_intv = 0;
	u64 bwt_blocks = 0, bwt_bytes = 0, sa_bytes = 0, pac_bytes = 0, bwt_size = 0, n_sa = 0;
	std::vector<i64> h_ctg_off; std::vector<i32> h_ctg_len, h_ctg_alt;
	// batch
	int n_reads = 0, max_len = 0; i64 n_bases = 0;
	bool have_batch = false, ran = false;
	int cigar_filter = 0;           // bwagpu_set_cigar_filter
	int stats_on = 0, taps_on = 0;       // stage taps cost a second region arena and a copy per batch: off unless a test asks (bwagpu_set_taps)
	bwagpu_stats_t stats = {};
	volatile int phase = 0;       // progress marker for bwagpu_debug_phase (diagnostics of a stuck call)
	i64 packed_tot = -1;          // regions packed by the last bwagpu_batch_download (-1: none)
	int packed_max = 0; bool downloaded = false;   // ... the largest count of a read among them; a download has happened for this run (a batch without reads packs nothing)
	DevBuf d_pri_out, d_pri_npri, d_pri_lists, d_pri_ctr, d_pri_scratch, d_pri_log;      // bwagpu_batch_primary / bwagpu_primary_flat: records, return values, the wavefront forms' read lists and their lengths, HBM working arrays, the table of logarithms
	DevBuf d_pair_out, d_pair_lists, d_pair_ctr, d_pair_scratch, d_pair_tab, d_pair_npri;      // bwagpu_batch_pair / bwagpu_pair_flat: records, the wavefront forms' pair lists and their lengths, HBM working arrays, the table of log(2 erfc) values, bwagpu_pair_flat's n_pri
	std::vector<double> pair_tab; bwagpu_pestat_t pair_tab_pes[4] = {}; i64 pair_tab_cap = -1; i32 pair_toff[4] = {}, pair_tlen[4] = {}; bool pair_tab_dev = false;   // the table as last filled: for these windows and this capacity; resident in d_pair_tab
	DevBuf d_pst_hist, d_pst_out;                                                         // bwagpu_batch_pestat and its kin (dev_pestat.h): the histogram of insert sizes, four windows and the info record (PstOut) -- resident for the next device-side consumer
	DevBuf d_aln_out, d_aln_n, d_aln_list, d_aln_ctr, d_aln_cigs, d_aln_ops, d_aln_len;                  // bwagpu_batch_alns / bwagpu_alns_flat (dev_alns.h): records, aa.n per read, the wavefront form's read list and its length; bwagpu_alns_flat's CIGAR records, operation array and read lengths
	enum { ST_NAMES, ST_NAMEOFF, ST_QUAL, ST_COMM, ST_COMMOFF, ST_RG, ST_SIZE, ST_TOFF, ST_FLAGS, ST_LINES, ST_TEXT, ST_N };
	DevBuf d_st[ST_N];      // bwagpu_batch_sam / bwagpu_sam_flat (dev_samtext.h): the reads' names, qualities, comments with their offsets, -R's id; bytes per read, their prefix sums, flag words, lines per read, the text
	DevBuf d_pf_regs, d_pf_cnt, d_pf_off, d_pf_ids, d_pf_seq, d_pf_seqoff;                // ... and the uploaded lists (FlatLists) and reads (FlatReads) of the *_flat calls
	std::vector<double> pri_log; i64 pri_log_dev = 0;                                      // log((double)k) by the host's libm for k < size; entries resident in d_pri_log
	DevBuf d_msw_tasks, d_msw_out, d_msw_pes, d_msw_scratch;
	enum { RS_X, RS_TOFF, RS_TIX, RS_ARENA, RS_ASRC, RS_ACNT, RS_POFF, RS_REGS, RS_SRC, RS_OUT, RS_LISTS, RS_CTR, RS_KEYS, RS_STAGE, RS_PAIRIDS, RS_N };
	DevBuf d_rs[RS_N];      // bwagpu_batch_rescue / bwagpu_rescue_flat (dev_rescue.h): anchors x 4 per read and their prefix sums, the task table, the arena of working lists (regions, src, lengths), the packed merged lists (offsets, regions, src), records, the wavefront forms' pair lists and their lengths, HBM sort keys; the pairs' ids
	enum { SP_OUT, SP_LIST, SP_CTR, SP_READ, SP_CIGS, SP_EXT, SP_N };
	DevBuf d_sp[SP_N];      // bwagpu_batch_sampe / bwagpu_sampe_flat (dev_sampe.h): the pair records, the wavefront form's pair list and its length, the merged lists' region-to-read map, their CIGAR records and operation array
	enum { CF_READ, CF_CIGS, CF_EXT, CF_N };
	DevBuf d_cf[CF_N];      // bwagpu_cigars_flat: the region-to-read map, the CIGAR records and the operation array (none of them a batch's)
	enum { DF_REGS, DF_REGOFF, DF_NRAW, DF_CNT, DF_FORM, DF_BLOB, DF_DPH, DF_DPE, DF_CTR, DF_N };
	DevBuf d_df[DF_N];     // bwagpu_dedup_flat: the caller's regions, their offsets and counts, the counts left, the routine per read, the sorts' key scratch, DP scratch, counters (none of them a batch's)
	i64 cigl_z_cap = 0;                          // bytes per direction matrix of the long CIGAR tier's scratch (grows with the batches)
	DevBuf d_cigl_z, d_cigl_ops, d_cigl_md, d_cigl_list;      // scratch of the long-segment CIGAR tier (k_cigar_long): direction matrices, operations, MD strings per workgroup
	DevBuf d_cig_ext; i64 cig_ext_n = -1;   // operation array of the last bwagpu_batch_cigars (records with 7..64 operations point into it)
	DevBuf d_dd_tmp;                            // short-read batches: staging areas of k_dedup_wave<.., LIST>'s waves (the kept records of a read in their final order)
	DevBuf d_heavy;                             // short-read batches: the reads the lane-per-read seeding kernel gave up (their passes 1-2 run as tasks)
	DevBuf d_p2_tasks; double p2_factor = 1.;   // pass-2 tasks of a short-read batch's heavy reads (grown on overflow bit 5)
	DevBuf d_vr_tab, d_vr_ovf, d_intv_n3;   // pass 1 of long-read batches as tasks (k_seed<LR>): the reads' first tasks, the list of tasks to redo on full-size stacks, pass 3's entries per read
	DevBuf d_seq_2b, d_seq_flags; int rd_words = 0; int seed_lds_run = 0;   // per-read 2-bit copies for k_seed's LDS (k_pack_reads2b)
	DevBuf d_pack_off, d_regs_packed, d_pack_read, d_cigs, d_seq, d_seq_nib, d_off, d_ctr, d_tmp_intv, d_intv_n, d_intv_off, d_intv, d_seed_n, d_seed_off;
	DevBuf d_slot_pos, d_slot_qbeg, d_slot_len, d_slot_rid, d_slot_blob;
	DevBuf d_order, d_bin_cnt, d_seed_w, d_seed_order, d_chain_n, d_node_off, d_nodes, d_reg_off, d_reg_cap_r, d_reg_n_raw, d_reg_n, d_regs, d_regs_raw, d_dp_h, d_dp_e, d_minhsp;
	i64 slot_cap = 0, node_cap = 0, reg_cap = 0; int mem_cap = 0;
	double need_slot = 0, need_node = 0, need_reg = 0; int need_mem = 0;   // per-base arena needs learnt from earlier batches of this handle
	std::vector<i64> h_off;
};

// Wait for the handle's stream without burning a host core: hipStreamSynchronize busy-waits, and a process that keeps several
// batches in flight from several host threads would spend that many cores spinning -- cores the finalize stage needs.
#define wait_stream(h) ((h)->ev_wait ? (hipEventRecord((h)->ev_wait, (h)->stream) == hipSuccess ? hipEventSynchronize((h)->ev_wait) : hipStreamSynchronize((h)->stream)) : hipStreamSynchronize((h)->stream))

#define HIPCHK(h, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { (h)->err = std::string(#call) + ": " + hipGetErrorString(e_); return BWAGPU_EHIP; } } while (0)

extern "C" const char *bwagpu_version(void) { return BWAGPU_VERSION; }
// sizeof of the public structs as this library was compiled (bindings check their mirrors against it)
extern "C" void bwagpu_abi_sizes(int32_t out[8])
{
	out[0] = (int32_t)sizeof(bwagpu_opt_t); out[1] = (int32_t)sizeof(bwagpu_alnreg_t); out[2] = (int32_t)sizeof(bwagpu_stats_t); out[3] = (int32_t)sizeof(bwagpu_index_desc_t);
	out[4] = (int32_t)sizeof(bwagpu_cigar_t); out[5] = (int32_t)sizeof(bwagpu_matesw_t); out[6] = (int32_t)sizeof(bwagpu_bseq1_t); out[7] = (int32_t)sizeof(bwagpu_built_t);
}

extern "C" const char *bwagpu_strerror(int code)
{
	switch (code) {
	case BWAGPU_OK: return "ok";
	case BWAGPU_ENODEV: return "no usable HIP device";
	case BWAGPU_EINVAL: return "invalid argument";
	case BWAGPU_ENOMEM: return "out of memory";
	case BWAGPU_EIO: return "index files missing or inconsistent";
	case BWAGPU_EHIP: return "HIP runtime error";
	case BWAGPU_EUNSUP: return "unsupported option on the device path";
	default: return "unknown error";
	}
}
extern "C" const char *bwagpu_last_error(const bwagpu_t *h) { return h ? h->err.c_str() : ""; }
// ---- result buffers ------------------------------------------------------------------------------------------------
// The large per-batch results (regions, CIGAR records, operation array, mate-rescue records: ~300 MB per 667 k reads) are copied out of the
// device with hipMemcpyAsync.  Into malloc'ed memory the runtime stages such a copy through bounce buffers; into page-locked memory it is one
// DMA at the link's rate.  Page-locking itself costs more than the copy, so the blocks are kept: bwagpu_free puts a pooled block back,
// result_alloc hands out the smallest free block that fits (sizes are rounded up so that consecutive batches find each other's blocks).
// Results under 1 MiB (BWAGPU_PINNED_MIN_KB), and everything when BWAGPU_PINNED_RESULTS=0, come from malloc as before.  The pool is bounded (4 GiB page-locked).
namespace {
struct ResultPool {
	std::mutex m;
	std::map<void*, size_t> live;                   // blocks handed out -> capacity
	std::multimap<size_t, void*> idle;              // capacity -> block
	size_t pinned = 0;
	std::atomic<long long> on{1}, min_kb{1024}, cap_mb{16384};
	std::atomic<bool> warned{false};
	std::atomic<bool> inited{false};                // settings taken from a handle's options (init_config) or, for a block asked for before any handle exists, from the environment
	void *get(size_t bytes)
	{
		if (!inited.exchange(true)) { BwagpuConfig c; c.from_env(); on = c.pinned_results; min_kb = c.pinned_min_kb < 0 ? 0 : c.pinned_min_kb; cap_mb = c.pinned_cap_mb < 0 ? 0 : c.pinned_cap_mb; }
		const size_t cap_total = (size_t)cap_mb.load() << 20;
		const bool enabled = on.load() != 0;                       // (options pinned_results / pinned_min_kb: process-wide, set whenever a handle is created or the option is set)
		const size_t min_bytes = (size_t)min_kb.load() << 10;
		if (!enabled || bytes < min_bytes) return malloc(bytes ? bytes : 1);
		size_t step = (size_t)1 << 20;                 // block sizes: multiples of 1 MiB up to 8 MiB, then of a quarter of the power of two below
		while (step * 8 <= bytes) step <<= 1;
		const size_t want = (bytes + step - 1) / step * step;
		{
			std::lock_guard<std::mutex> l(m);
			auto it = idle.lower_bound(bytes);
			if (it != idle.end() && it->first <= want * 2) { void *p = it->second; live[p] = it->first; idle.erase(it); return p; }
			if (pinned + want > cap_total) {           // make room: drop idle blocks, smallest first
				while (!idle.empty() && pinned + want > cap_total) { auto b = idle.begin(); (void)hipHostFree(b->second); pinned -= b->first; idle.erase(b); }
				if (pinned + want > cap_total) {
					if (!warned.exchange(true)) fprintf(stderr, "[W::bwagpu] the page-locked result pool is full (%lld MiB, option pinned_cap_mb): further results are copied through pageable memory\n", cap_mb.load());
					return malloc(bytes);
				}
			}
			pinned += want;
		}
		void *p = nullptr;
		if (hipHostMalloc(&p, want, hipHostMallocPortable) != hipSuccess || !p) {     // (portable: a block may serve another device's handle next time)
			(void)hipGetLastError();
			std::lock_guard<std::mutex> l(m); pinned -= want;
			return malloc(bytes);
		}
		std::lock_guard<std::mutex> l(m);
		live[p] = want;
		return p;
	}
	// release the idle blocks (bwagpu_trim; also when the process's last handle is destroyed: an embedding program gets the page-locked
	// memory back with the device)
	void trim()
	{
		std::lock_guard<std::mutex> l(m);
		for (auto &b : idle) { (void)hipHostFree(b.second); pinned -= b.first; }
		idle.clear();
	}
	void put(void *p)
	{
		if (!p) return;
		{
			std::lock_guard<std::mutex> l(m);
			auto it = live.find(p);
			if (it != live.end()) { idle.emplace(it->second, p); live.erase(it); return; }
		}
		free(p);
	}
};
ResultPool g_results;
}
static void *result_alloc(size_t bytes) { return g_results.get(bytes); }
extern "C" void bwagpu_free(void *p) { g_results.put(p); }
extern "C" void *bwagpu_alloc_host(size_t bytes) { return g_results.get(bytes); }
extern "C" void bwagpu_trim(void) { g_results.trim(); }
static std::atomic<int> g_live_handles{0};

static int upload(bwagpu_t *h, DevBuf &b, const void *src, size_t bytes)
{
	if (b.ensure(bytes ? bytes : 16)) { h->err = "hipMalloc failed"; return BWAGPU_ENOMEM; }
	if (bytes) HIPCHK(h, hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
	return 0;
}

// ---- options (bwagpu_config.h) ----------------------------------------------------------------------------------------------
namespace {
std::mutex g_cfg_m;
std::map<std::string, long long> g_cfg_defaults;     // bwagpu_set_default_option: applied to handles created afterwards, on top of the environment
}
// Ranges of the options (one test for all three ways in -- bwagpu_set_option, bwagpu_set_default_option, the environment): sizes and counts that the
// batch calls cast to int or multiply, and the options with a fixed set of kernel instances behind them (-1 = auto where the list says so).
// seed_lds_ent: 16 entries x 16 B x 256 lanes is the whole 64 KiB a workgroup's dynamic LDS may take.
static bool option_in_range(const BwagpuConfig &c, const long long *f, long long value)
{
	auto in = [&](long long lo, long long hi) { return value >= lo && value <= hi; };
	if (f == &c.ext_occ) return value == 4 || value == 6;
	if (f == &c.seed_mrg) return value == -1 || value == 0 || value == 2;
	if (f == &c.share) return in(-1, 100);
	if (f == &c.seed_task_stack || f == &c.seed_p2_cap || f == &c.mem_cap || f == &c.seed_grid || f == &c.cig_ops_cap || f == &c.idx_desc_max_mb || f == &c.pri_log_cap || f == &c.pair_tab_cap) return in(0, 0x3fffffff);
	if (f == &c.seed_budget || f == &c.dedup_heavy) return in(-1, 0x3fffffff);
	if (f == &c.dedup_stage || f == &c.dedup_big || f == &c.dedup_net) return in(-1, 1024);
	if (f == &c.seed_lds_ent) return in(-1, 16);
	if (f == &c.dedup_ring) return value == 0 || (in(256, 4096) && (value & (value - 1)) == 0);
	if (f == &c.cigl_mib) return in(0, 1 << 20);
	if (f == &c.cig_tiers || f == &c.chain_regs) return in(0, 2);
	if (f == &c.seed_jump) return in(-1, 3);
	if (f == &c.chain_flt_lds) return in(0, CW_FLT_LDS);
	if (f == &c.ptab_m) return in(0, PTAB_MAX);
	if (f == &c.occ32_sb_shift) return in(8, 32);
	return true;
}
static void init_config(BwagpuConfig &c)
{
	c = BwagpuConfig();
	const BwagpuConfig dflt;
	c.from_env();
	// a value from the environment that is out of range is dropped with a warning (the handle keeps the compiled-in default); bwagpu_set_default_option
	// refuses such values when they are set
#define X(name, d) if (!option_in_range(c, &c.name, c.name)) { fprintf(stderr, "[W::bwagpu] BWAGPU_%s=%lld is out of range: ignored\n", #name, c.name); c.name = dflt.name; }
	BWAGPU_OPTION_LIST(X)
#undef X
	std::lock_guard<std::mutex> l(g_cfg_m);
	for (auto &kv : g_cfg_defaults) if (long long *f = c.field(kv.first.c_str())) *f = kv.second;
	g_results.on = c.pinned_results; g_results.min_kb = c.pinned_min_kb < 0 ? 0 : c.pinned_min_kb; g_results.cap_mb = c.pinned_cap_mb < 0 ? 0 : c.pinned_cap_mb; g_results.inited = true;
}
extern "C" int bwagpu_set_default_option(const char *key, long long value)
{
	BwagpuConfig probe;
	const long long *f = probe.field(key);
	if (!f || !option_in_range(probe, f, value)) return BWAGPU_EINVAL;
	std::lock_guard<std::mutex> l(g_cfg_m);
	g_cfg_defaults[key] = value;
	return BWAGPU_OK;
}
extern "C" void bwagpu_clear_default_options(void) { std::lock_guard<std::mutex> l(g_cfg_m); g_cfg_defaults.clear(); }
extern "C" int bwagpu_set_option(bwagpu_t *h, const char *key, long long value)
{
	if (!h) return BWAGPU_EINVAL;
	long long *f = h->cfg.field(key);
	if (!f) return BWAGPU_EINVAL;
	// the index-side options shape what bwagpu_create / bwagpu_index_ready derive from the index: per handle they can only be set before that
	// happens (a handle created with NULL arrays, ahead of the broadcast); otherwise use bwagpu_set_default_option before creating the handle
	if ((f == &h->cfg.occ32 || f == &h->cfg.occ32_sb_shift || f == &h->cfg.ptab_m) && (h->ix.occ32 || h->ix.ptab) && *f != value) return BWAGPU_EINVAL;
	if (!option_in_range(h->cfg, f, value)) return BWAGPU_EINVAL;
	*f = value;
	if (f == &h->cfg.pinned_results) g_results.on = value;
	if (f == &h->cfg.pinned_min_kb) g_results.min_kb = value < 0 ? 0 : value;
	if (f == &h->cfg.pinned_cap_mb) g_results.cap_mb = value < 0 ? 0 : value;
	return BWAGPU_OK;
}
extern "C" int bwagpu_get_option(const bwagpu_t *h, const char *key, long long *value)
{
	if (!h || !value) return BWAGPU_EINVAL;
	const long long *f = const_cast<bwagpu_t*>(h)->cfg.field(key);
	if (!f) return BWAGPU_EINVAL;
	*value = *f;
	return BWAGPU_OK;
}
extern "C" int bwagpu_option_name(int i, const char **name)
{
	static const char *const names[] = {
#define X(n, d) #n,
		BWAGPU_OPTION_LIST(X)
#undef X
	};
	if (!name || i < 0 || i >= (int)(sizeof names / sizeof names[0])) return BWAGPU_EINVAL;
	*name = names[i];
	return BWAGPU_OK;
}

// ---- prefix tables (DevIndex::ptab): level j from level j-1 with the sweep's own extension ----------------------------------
__global__ void __launch_bounds__(256) k_ptab_level(DevIndex ix, u64 *tab, int j)
{
	const u64 n = (u64)1 << (2 * j);
	for (u64 c = (u64)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (u64)gridDim.x * blockDim.x) {
		BiIntv out;
		if (j == 1) fm_init(ix, (int)c, out);                          // bwt_set_intv (bwt.h:82)
		else {
			const u64 *pe = tab + ((((u64)1 << (2 * (j - 1))) - 4) / 3 + (c >> 2)) * 3;
			BiIntv par; par.x0 = pe[0]; par.x1 = pe[1]; par.x2 = pe[2]; par.info = 0;
			// forward extension by base c&3 (bwt.c:307-308).  Empty parents are extended too, by the same arithmetic:
			// bwt_seed_strategy1 keeps extending an interval that has become empty until min_seed_len is reached (bwt.c:364-377)
			fm_extend1(ix, par, 3 - (int)(c & 3), 0, out);
		}
		u64 *e = tab + ((n - 4) / 3 + c) * 3;
		e[0] = out.x0; e[1] = out.x1; e[2] = out.x2;
	}
}

// records: for every m-mer W the packed bi-intervals of its m prefixes, gathered from the level tables.  The entry of the j-base prefix
// carries, in the 16 bits the packing leaves for `info`, the CHANGE BITS of its own prefixes: bit k-1 = the (k+1)-base prefix has another
// interval size than the k-base one, 1 <= k < j.  Sizes never grow with depth, so two depths have equal sizes exactly when no change bit
// lies between them: what a sweep's steps below the tables' depth ask of the index (dev_seed.h, option seed_jump), from one entry.
__global__ void __launch_bounds__(256) k_ptab_records(const u64 *tab, uint4 *rec, int m)
{
	const u64 n = ((u64)1 << (2 * m)) * (u64)m;
	for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (u64)gridDim.x * blockDim.x) {
		const u64 w = t / (u64)m; const int j = (int)(t % (u64)m) + 1;
		const u64 *e = tab + ((((u64)1 << (2 * j)) - 4) / 3 + (w >> (2 * (m - j)))) * 3;
		BiIntv v; v.x0 = e[0]; v.x1 = e[1]; v.x2 = e[2]; v.info = 0;
		u64 deeper = v.x2;
		for (int k = j - 1; k >= 1; --k) {
			const u64 x2 = tab[((((u64)1 << (2 * k)) - 4) / 3 + (w >> (2 * (m - k)))) * 3 + 2];
			if (x2 != deeper) v.info |= (u64)1 << (k - 1);
			deeper = x2;
		}
		rec[t] = SeedStack::pack(v);
	}
}

// ---- the 32-byte block layout of the BWT (DevIndex::occ32) --------------------------------------------------------------------
// counts of the four symbols at the start of 64-base block j, from the reference-format block it is half of
DEVFN void occ32_start_counts(const DevIndex &ix, u64 j, u64 cnt[4])
{
	const uint4 *src = ix.bwt + (j >> 1) * 4;
	const uint4 c01 = src[0], c23 = src[1];
	cnt[0] = (u64)c01.y << 32 | c01.x; cnt[1] = (u64)c01.w << 32 | c01.z; cnt[2] = (u64)c23.y << 32 | c23.x; cnt[3] = (u64)c23.w << 32 | c23.z;
	if (j & 1) {                           // second half: add the first 64 bases of the block
		const uint4 w0 = src[2];
		u32 c1 = 0, c2 = 0, c3 = 0;
		count_pair(w0.x, w0.y, 32, c1, c2, c3); count_pair(w0.z, w0.w, 32, c1, c2, c3);
		cnt[0] += 64 - c1 - c2 - c3; cnt[1] += c1; cnt[2] += c2; cnt[3] += c3;
	}
}
__global__ void __launch_bounds__(256) k_occ32_sb(DevIndex ix, u64 *sb, u64 n_sb, u64 n_new, int sh /* log2 of 64-base blocks per superblock */)
{
	for (u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x; s < n_sb; s += (u64)gridDim.x * blockDim.x) {
		u64 cnt[4] = { 0, 0, 0, 0 };
		if ((s << sh) < n_new) occ32_start_counts(ix, s << sh, cnt);   // (the table has one spare entry past the end)
		for (int k = 0; k < 4; ++k) sb[s * 4 + k] = cnt[k];
	}
}
// Second form of the superblock table for the one-trip rank routine (dev_fm.h, occ32x_*): entry [s][c] = { count of c, sum of the counts of
// the symbols above c } -- what an extension by c needs from a position's superblock in ONE 16-byte load instead of the whole 32-byte row
__global__ void __launch_bounds__(256) k_occ32_sbx(const u64 *sb, uint4 *out, u64 n_sb)
{
	for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < n_sb * 4; t += (u64)gridDim.x * blockDim.x) {
		const u64 *row = sb + (t >> 2) * 4; const int c = (int)(t & 3);
		u64 above = 0;
		for (int i = c + 1; i < 4; ++i) above += row[i];
		out[t] = make_uint4((u32)row[c], (u32)(row[c] >> 32), (u32)above, (u32)(above >> 32));
	}
}
__global__ void __launch_bounds__(256) k_occ32_blocks(DevIndex ix, const u64 *sb, uint4 *out, u64 n_new, int sh)
{
	for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n_new; j += (u64)gridDim.x * blockDim.x) {
		u64 cnt[4];
		occ32_start_counts(ix, j, cnt);
		const u64 *base = sb + (j >> sh) * 4;
		uint4 rel; rel.x = (u32)(cnt[0] - base[0]); rel.y = (u32)(cnt[1] - base[1]); rel.z = (u32)(cnt[2] - base[2]); rel.w = (u32)(cnt[3] - base[3]);
		out[j * 2] = rel;
		out[j * 2 + 1] = ix.bwt[(j >> 1) * 4 + 2 + (j & 1)];
	}
}
// The seeding and SA kernels read this layout (default; BWAGPU_OCC32=0 keeps them on the reference-format blocks): built from the resident
// reference-format blocks, which stay the interchange format (files, index broadcast, bwagpu_index_buffers).  Measured at 3.1 Gbp
// (profiles/r03_seed_variants.md): k_seed 94.6 ms on the 64-byte blocks, 84.6 ms on these -- and 134.5 ms with the 64-byte blocks fetched
// quad-cooperatively (a round-3 variant, deleted in round 4), although that fetch pattern moves the chip's random-block ceiling from 22.9e9 to
// 51.3e9 per second (tools/randbw3.hip): the cooperative form adds instructions and registers (3 waves per SIMD) in front of every trip.
static int build_occ32(bwagpu_t *h)
{
	h->ix.occ32 = nullptr; h->ix.occ_sb = nullptr; h->ix.occ_sbx = nullptr; h->ix.occ_sb_shift = 32; h->ix.occ32_bytes = h->ix.occ_sbx_bytes = 0;
	if (h->cfg.occ32 == 0 || h->bwt_blocks == 0) return 0;   // (option occ32 = 0: keep to the reference-format blocks)
	int shift = (int)h->cfg.occ32_sb_shift;      // (tests: small superblocks on small genomes)
	if (shift < 8) shift = 8; if (shift > 32) shift = 32;
	const int sh = shift - 6;
	const u64 n_new = (u64)h->bwt_blocks * 2, n_sb = (n_new >> sh) + 1;
	if (h->ibuf->d_occ32.ensure((size_t)n_new * 32) || h->ibuf->d_occ_sb.ensure((size_t)n_sb * (32 + 64))) { h->err = "hipMalloc failed (32-byte blocks)"; return BWAGPU_ENOMEM; }   // (both forms of the superblock table, one after the other)
	hipLaunchKernelGGL(k_occ32_sb, dim3((unsigned)((n_sb + 255) / 256 < 1024 ? (n_sb + 255) / 256 : 1024)), dim3(256), 0, h->stream, h->ix, h->ibuf->d_occ_sb.as<u64>(), n_sb, n_new, sh);
	hipLaunchKernelGGL(k_occ32_blocks, dim3((unsigned)((n_new + 255) / 256 < 65536 ? (n_new + 255) / 256 : 65536)), dim3(256), 0, h->stream, h->ix, h->ibuf->d_occ_sb.as<u64>(), h->ibuf->d_occ32.as<uint4>(), n_new, sh);
	hipLaunchKernelGGL(k_occ32_sbx, dim3((unsigned)((n_sb * 4 + 255) / 256 < 1024 ? (n_sb * 4 + 255) / 256 : 1024)), dim3(256), 0, h->stream, h->ibuf->d_occ_sb.as<u64>(), (uint4*)(h->ibuf->d_occ_sb.as<u64>() + n_sb * 4), n_sb);
	hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(h->stream);
	HIPCHK(h, e1); HIPCHK(h, e2);
	h->ix.occ32 = h->ibuf->d_occ32.as<uint4>(); h->ix.occ_sb = h->ibuf->d_occ_sb.as<u64>(); h->ix.occ_sb_shift = shift;
	h->ix.occ_sbx = (const uint4*)(h->ibuf->d_occ_sb.as<u64>() + n_sb * 4);
	h->ix.occ32_bytes = n_new * 32; h->ix.occ_sbx_bytes = n_sb * 64;
	return 0;
}

static int build_prefix_tables(bwagpu_t *h, int m)
{
	// the packed entries hold 37-bit interval bounds (as do the LDS interval stacks)
	h->ix.ptab_bytes = 0;
	if (m < 2 || h->ix.seq_len >= ((u64)1 << 36)) { h->ix.ptab = nullptr; h->ix.ptab_m = 0; return 0; }
	if (m > PTAB_MAX) m = PTAB_MAX;
	size_t entries = ((((size_t)1 << (2 * (m + 1))) - 4) / 3);
	DevBuf levels;
	if (levels.ensure(entries * 24) || h->ibuf->d_ptab.ensure(((size_t)1 << (2 * m)) * m * sizeof(uint4))) { levels.release(); h->err = "hipMalloc failed (prefix tables)"; return BWAGPU_ENOMEM; }
	DevIndex ix = h->ix; ix.ptab = nullptr; ix.ptab_m = 0;
	for (int j = 1; j <= m; ++j) {
		u64 n = (u64)1 << (2 * j);
		unsigned nb = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
		hipLaunchKernelGGL(k_ptab_level, dim3(nb), dim3(256), 0, h->stream, ix, levels.as<u64>(), j);
	}
	const u64 n_rec = ((u64)1 << (2 * m)) * (u64)m;
	hipLaunchKernelGGL(k_ptab_records, dim3((unsigned)((n_rec + 255) / 256 < 8192 ? (n_rec + 255) / 256 : 8192)), dim3(256), 0, h->stream, levels.as<u64>(), h->ibuf->d_ptab.as<uint4>(), m);
	hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(h->stream);
	levels.release();
	HIPCHK(h, e1); HIPCHK(h, e2);
	h->ix.ptab = h->ibuf->d_ptab.as<uint4>(); h->ix.ptab_m = m; h->ix.ptab_bytes = n_rec * sizeof(uint4);
	return 0;
}

extern "C" int bwagpu_create(bwagpu_t **out, const bwagpu_index_desc_t *d, int device)
{
	if (!out || !d || d->n_seqs <= 0 || !d->ctg_offset || !d->ctg_len || !d->ctg_is_alt) return BWAGPU_EINVAL;
	const bool alloc_only = !d->bwt && !d->sa && !d->pac;   // receiving side of an index broadcast
	if (!alloc_only && (!d->bwt || !d->sa || !d->pac)) return BWAGPU_EINVAL;
	if (d->sa_intv <= 0 || (d->sa_intv & (d->sa_intv - 1))) return BWAGPU_EINVAL;
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return BWAGPU_ENODEV;
	if (hipSetDevice(device) != hipSuccess) return BWAGPU_ENODEV;
	bwagpu_t *h = new bwagpu_s(); ++g_live_handles;
	h->device = device;
	h->ibuf = new bwagpu_s::IndexBufs();
	init_config(h->cfg);
	int rc;
	if (hipStreamCreate(&h->stream) != hipSuccess) { h->stream = nullptr; bwagpu_destroy(h); return BWAGPU_ENODEV; }
	for (int i = 0; i < 8; ++i) if (hipEventCreate(&h->ev[i]) != hipSuccess) { h->ev[i] = nullptr; bwagpu_destroy(h); return BWAGPU_ENODEV; }
	if (hipEventCreateWithFlags(&h->ev_wait, hipEventBlockingSync | hipEventDisableTiming) != hipSuccess) h->ev_wait = nullptr;
	// the last Occ record of the .bwt is a trailing 32-byte half block; pad the upload to whole 64-byte blocks
	u64 nblk = (d->bwt_size + 15) / 16;
	std::vector<uint32_t> padded;
	const uint32_t *src = d->bwt;
	if (!alloc_only && d->bwt_size % 16) { padded.assign(nblk * 16, 0); memcpy(padded.data(), d->bwt, d->bwt_size * 4); src = padded.data(); }
	h->bwt_bytes = nblk * 64; h->sa_bytes = d->n_sa * 8; h->pac_bytes = (u64)(d->l_pac / 4 + 1);
	h->bwt_size = d->bwt_size; h->n_sa = d->n_sa;
	if (alloc_only) {
		if (h->ibuf->d_bwt.ensure(h->bwt_bytes) || h->ibuf->d_sa.ensure(h->sa_bytes) || h->ibuf->d_pac.ensure(h->pac_bytes)) { rc = BWAGPU_ENOMEM; goto fail; }
	} else {
		if ((rc = upload(h, h->ibuf->d_bwt, src, nblk * 64))) goto fail;
		if ((rc = upload(h, h->ibuf->d_sa, d->sa, d->n_sa * 8))) goto fail;
		if ((rc = upload(h, h->ibuf->d_pac, d->pac, (size_t)(d->l_pac / 4 + 1)))) goto fail;
	}
	if ((rc = upload(h, h->ibuf->d_ctg_off, d->ctg_offset, (size_t)d->n_seqs * 8))) goto fail;
	if ((rc = upload(h, h->ibuf->d_ctg_len, d->ctg_len, (size_t)d->n_seqs * 4))) goto fail;
	if ((rc = upload(h, h->ibuf->d_ctg_alt, d->ctg_is_alt, (size_t)d->n_seqs * 4))) goto fail;
	h->bwt_blocks = nblk;
	h->ix.bwt = h->ibuf->d_bwt.as<uint4>();
	h->ix.primary = d->primary; for (int i = 0; i < 5; ++i) h->ix.L2[i] = d->L2[i];
	h->ix.seq_len = d->seq_len;
	h->ix.sa = h->ibuf->d_sa.as<u64>(); h->ix.sa_mask = (u64)d->sa_intv - 1;
	h->ix.sa_shift = 0; while ((1 << h->ix.sa_shift) < d->sa_intv) ++h->ix.sa_shift;
	h->ix.pac = h->ibuf->d_pac.as<u8>(); h->ix.l_pac = d->l_pac;
	h->ix.n_seqs = d->n_seqs; h->ix.ctg_off = h->ibuf->d_ctg_off.as<i64>(); h->ix.ctg_len = h->ibuf->d_ctg_len.as<i32>(); h->ix.ctg_alt = h->ibuf->d_ctg_alt.as<i32>();
	h->l_pac = d->l_pac; h->n_seqs = d->n_seqs; h->seq_len = d->seq_len; h->sa_intv = d->sa_intv;
	h->h_ctg_off.assign(d->ctg_offset, d->ctg_offset + d->n_seqs);
	h->h_ctg_len.assign(d->ctg_len, d->ctg_len + d->n_seqs);
	h->h_ctg_alt.assign(d->ctg_is_alt, d->ctg_is_alt + d->n_seqs);
	h->ix.ptab = nullptr; h->ix.ptab_m = 0; h->ix.ptab_bytes = 0; h->ix.occ32 = nullptr; h->ix.occ_sb = nullptr; h->ix.occ_sbx = nullptr; h->ix.occ32_bytes = h->ix.occ_sbx_bytes = 0;
	if (!alloc_only) {   // (a handle that receives its index by broadcast builds them in bwagpu_index_ready)
		if ((rc = build_occ32(h))) goto fail;
		if ((rc = build_prefix_tables(h, (int)h->cfg.ptab_m))) goto fail;
	}
	*out = h;
	return BWAGPU_OK;
fail:
	bwagpu_destroy(h);
	return rc;
}

extern "C" void bwagpu_destroy(bwagpu_t *h)
{
	if (!h) return;
	struct LastOut { ~LastOut() { if (--g_live_handles == 0) g_results.trim(); } } last_out;      // (after the handle's own buffers are gone)
	for (void *&p_ : h->reserved) { if (p_) bwagpu_free(p_); p_ = nullptr; }
	if (h->ibuf && --h->ibuf->refs == 0) {
		DevBuf *ib[] = { &h->ibuf->d_bwt, &h->ibuf->d_sa, &h->ibuf->d_pac, &h->ibuf->d_ctg_off, &h->ibuf->d_ctg_len, &h->ibuf->d_ctg_alt, &h->ibuf->d_ptab, &h->ibuf->d_occ32, &h->ibuf->d_occ_sb, &h->ibuf->d_ctg_text, &h->ibuf->d_ctg_toff };
		for (DevBuf *b : ib) b->release();
		delete h->ibuf;
	}
	DevBuf *all[] = { &h->d_pst_hist, &h->d_pst_out, &h->d_pair_out, &h->d_pair_lists, &h->d_pair_ctr, &h->d_pair_scratch, &h->d_pair_tab, &h->d_pair_npri, &h->d_pri_out, &h->d_pri_npri, &h->d_pri_lists, &h->d_pri_ctr, &h->d_pri_scratch, &h->d_pri_log, &h->d_aln_out, &h->d_aln_n, &h->d_aln_list, &h->d_aln_ctr, &h->d_aln_cigs, &h->d_aln_ops, &h->d_aln_len, &h->d_pf_regs, &h->d_pf_cnt, &h->d_pf_off, &h->d_pf_ids, &h->d_pf_seq, &h->d_pf_seqoff, &h->d_heavy, &h->d_dd_tmp, &h->d_p2_tasks, &h->d_vr_tab, &h->d_vr_ovf, &h->d_intv_n3, &h->d_cigl_list, &h->d_cigl_z, &h->d_cigl_ops, &h->d_cigl_md, &h->d_seq_2b, &h->d_seq_flags, &h->d_cig_ext, &h->d_msw_tasks, &h->d_msw_out, &h->d_msw_pes, &h->d_msw_scratch, &h->d_pack_off, &h->d_regs_packed, &h->d_pack_read, &h->d_cigs, &h->d_seq, &h->d_seq_nib, &h->d_off, &h->d_ctr, &h->d_tmp_intv,
		&h->d_intv_n, &h->d_intv_off, &h->d_intv, &h->d_seed_n, &h->d_seed_off, &h->d_slot_pos, &h->d_slot_qbeg, &h->d_slot_len, &h->d_slot_rid, &h->d_slot_blob, &h->d_chain_n, &h->d_node_off,
		&h->d_order, &h->d_bin_cnt, &h->d_seed_w, &h->d_seed_order, &h->d_nodes, &h->d_reg_off, &h->d_reg_cap_r, &h->d_reg_n_raw, &h->d_reg_n, &h->d_regs, &h->d_regs_raw, &h->d_dp_h, &h->d_dp_e, &h->d_minhsp };
	for (DevBuf *b : all) b->release();
	for (DevBuf &b : h->d_rs) b.release();
	for (DevBuf &b : h->d_sp) b.release();
	for (DevBuf &b : h->d_cf) b.release();
	for (DevBuf &b : h->d_df) b.release();
	for (DevBuf &b : h->d_st) b.release();
	for (int i = 0; i < 8; ++i) if (h->ev[i]) (void)hipEventDestroy(h->ev[i]);
	if (h->ev_wait) (void)hipEventDestroy(h->ev_wait);
	if (h->stream) (void)hipStreamDestroy(h->stream);
	delete h;
}

// ---- index files (formats: bwt.c:385-462, bntseq.c:97-211, bwa.c:300-312) -------------------------------------
static bool read_file(const std::string &fn, std::vector<char> &out)
{
	FILE *fp = fopen(fn.c_str(), "rb");
	if (!fp) return false;
	fseek(fp, 0, SEEK_END); long sz = ftell(fp); fseek(fp, 0, SEEK_SET);
	out.resize((size_t)sz);
	bool ok = sz == 0 || fread(out.data(), 1, (size_t)sz, fp) == (size_t)sz;
	fclose(fp);
	return ok;
}

extern "C" int bwagpu_create_from_files(bwagpu_t **out, const char *prefix, int device)
{
	if (!out || !prefix) return BWAGPU_EINVAL;
	std::string pre(prefix);
	std::vector<char> fb, fs, fp;
	if (!read_file(pre + ".bwt", fb) || fb.size() < 40 || !read_file(pre + ".sa", fs) || fs.size() < 56 || !read_file(pre + ".pac", fp)) return BWAGPU_EIO;
	bwagpu_index_desc_t d; memset(&d, 0, sizeof d);
	const u64 *hb = (const u64*)fb.data();
	d.primary = hb[0]; d.L2[0] = 0; for (int i = 0; i < 4; ++i) d.L2[i + 1] = hb[1 + i];
	d.seq_len = d.L2[4];
	d.bwt = (const uint32_t*)(fb.data() + 40); d.bwt_size = (fb.size() - 40) / 4;
	const u64 *hs = (const u64*)fs.data();
	if (hs[0] != d.primary || hs[6] != d.seq_len) return BWAGPU_EIO;
	d.sa_intv = (int)hs[5];
	if (d.sa_intv <= 0) return BWAGPU_EIO;
	d.n_sa = (d.seq_len + d.sa_intv) / d.sa_intv;
	if (fs.size() < 56 + (d.n_sa - 1) * 8) return BWAGPU_EIO;
	std::vector<u64> sa(d.n_sa);
	sa[0] = (u64)-1;                                   // bwt_restore_sa forces sa[0] = -1 (bwt.c:437)
	memcpy(sa.data() + 1, fs.data() + 56, (d.n_sa - 1) * 8);
	d.sa = sa.data();
	// .ann: "l_pac n_seqs seed" then per contig "gi name [anno]" / "offset len n_ambs"
	FILE *fa = fopen((pre + ".ann").c_str(), "r");
	if (!fa) return BWAGPU_EIO;
	long long xx; int n_seqs; unsigned seed;
	if (fscanf(fa, "%lld%d%u", &xx, &n_seqs, &seed) != 3 || n_seqs <= 0) { fclose(fa); return BWAGPU_EIO; }
	d.l_pac = xx; d.n_seqs = n_seqs;
	std::vector<i64> coff(n_seqs); std::vector<i32> clen(n_seqs), calt(n_seqs, 0); std::vector<std::string> names(n_seqs), annos(n_seqs);
	for (int i = 0; i < n_seqs; ++i) {
		char name[8192]; unsigned gi; int c, n_ambs, len;
		if (fscanf(fa, "%u%8191s", &gi, name) != 2) { fclose(fa); return BWAGPU_EIO; }
		names[i] = name;
		std::string rest;
		while ((c = fgetc(fa)) != '\n' && c != EOF) if (rest.size() < 8190) rest += (char)c;
		if (rest.size() > 1 && rest != " (null)") annos[i] = rest.substr(1);      // bntseq.c:128-129
		if (fscanf(fa, "%lld%d%d", &xx, &len, &n_ambs) != 3) { fclose(fa); return BWAGPU_EIO; }
		coff[i] = xx; clen[i] = len;
	}
	fclose(fa);
	if (FILE *fl = fopen((pre + ".alt").c_str(), "r")) {   // first column of each non-@ line names an ALT contig (bns_restore, bntseq.c:185-205)
		std::string name; int ch;
		while ((ch = fgetc(fl)) != EOF) {            // lines of any length; like the reference, a last line without a line end is not seen
			if (ch == '\t' || ch == '\n' || ch == '\r') {
				if (!name.empty() && name[0] != '@') for (int i = 0; i < n_seqs; ++i) if (names[i] == name) calt[i] = 1;
				while (ch != '\n' && ch != EOF) ch = fgetc(fl);
				name.clear();
			} else name += (char)ch;
		}
		fclose(fl);
	}
	if ((i64)fp.size() < d.l_pac / 4 + 1) return BWAGPU_EIO;
	d.pac = (const u8*)fp.data();
	d.ctg_offset = coff.data(); d.ctg_len = clen.data(); d.ctg_is_alt = calt.data();
	const int rc = bwagpu_create(out, &d, device);
	if (rc != BWAGPU_OK) return rc;
	std::string nb, ab; std::vector<i64> no(1, 0), ao(1, 0);
	for (int i = 0; i < n_seqs; ++i) { nb += names[i]; no.push_back((i64)nb.size()); ab += annos[i]; ao.push_back((i64)ab.size()); }
	const int rn = bwagpu_set_contig_names(*out, nb.data(), no.data(), ab.data(), ao.data());
	if (rn != BWAGPU_OK) { bwagpu_destroy(*out); *out = nullptr; }
	return rn;
}

// The host's copy of the contigs' names and annotations into h's HBM (h->ibuf->m is held)
static int ctg_names_upload(bwagpu_t *h)
{
	bwagpu_s::IndexBufs &B = *h->ibuf;
	std::vector<i64> toff(B.ctg_name_off);
	toff.insert(toff.end(), B.ctg_anno_off.begin(), B.ctg_anno_off.end());
	if (int rc = upload(h, B.d_ctg_text, B.ctg_text.data(), B.ctg_text.size())) return rc;
	return upload(h, B.d_ctg_toff, toff.data(), toff.size() * 8);
}

extern "C" int bwagpu_set_contig_names(bwagpu_t *h, const char *names, const int64_t *name_off, const char *annos, const int64_t *anno_off)
{
	if (!h || !names || !name_off || (annos && !anno_off)) return BWAGPU_EINVAL;
	const int n = h->n_seqs;
	for (int i = 0; i < n; ++i)
		if (name_off[0] < 0 || name_off[i] > name_off[i + 1] || (annos && (anno_off[0] < 0 || anno_off[i] > anno_off[i + 1]))) { h->err = "bwagpu_set_contig_names: offsets that do not ascend"; return BWAGPU_EINVAL; }
	HIPCHK(h, hipSetDevice(h->device));
	bwagpu_s::IndexBufs &B = *h->ibuf;
	std::lock_guard<std::mutex> l(B.m);
	B.ctg_text.assign(names + name_off[0], names + name_off[n]);
	B.ctg_name_off.resize((size_t)n + 1); B.ctg_anno_off.resize((size_t)n + 1);
	const i64 nn = (i64)B.ctg_text.size();
	for (int i = 0; i <= n; ++i) { B.ctg_name_off[i] = name_off[i] - name_off[0]; B.ctg_anno_off[i] = nn + (annos ? anno_off[i] - anno_off[0] : 0); }
	if (annos) B.ctg_text.append(annos + anno_off[0], annos + anno_off[n]);
	const int rc = ctg_names_upload(h);
	B.have_names = rc == BWAGPU_OK;
	return rc;
}

// A second handle on the same device that shares the index already resident in HBM (no copy) but has its own stream and
// batch arenas: two handles driven from two host threads keep two batches in flight, so the latency-bound tails of one
// batch (chaining of repeat-rich reads) overlap with the throughput-bound kernels of the other.
extern "C" int bwagpu_clone(bwagpu_t *src, bwagpu_t **out)
{
	if (!src || !out) return BWAGPU_EINVAL;
	if (hipSetDevice(src->device) != hipSuccess) return BWAGPU_ENODEV;
	bwagpu_t *h = new bwagpu_s(); ++g_live_handles;
	h->device = src->device;
	h->ibuf = src->ibuf; ++h->ibuf->refs;     // (bwagpu_destroy drops the reference again on every failure path below)
	if (hipStreamCreate(&h->stream) != hipSuccess) { h->stream = nullptr; bwagpu_destroy(h); return BWAGPU_ENODEV; }
	for (int i = 0; i < 8; ++i) if (hipEventCreate(&h->ev[i]) != hipSuccess) { h->ev[i] = nullptr; bwagpu_destroy(h); return BWAGPU_ENODEV; }
	if (hipEventCreateWithFlags(&h->ev_wait, hipEventBlockingSync | hipEventDisableTiming) != hipSuccess) h->ev_wait = nullptr;
	h->ix = src->ix; h->l_pac = src->l_pac; h->n_seqs = src->n_seqs; h->seq_len = src->seq_len; h->sa_intv = src->sa_intv;
	h->bwt_blocks = src->bwt_blocks; h->bwt_bytes = src->bwt_bytes; h->sa_bytes = src->sa_bytes; h->pac_bytes = src->pac_bytes;
	h->bwt_size = src->bwt_size; h->n_sa = src->n_sa;
	h->h_ctg_off = src->h_ctg_off; h->h_ctg_len = src->h_ctg_len; h->h_ctg_alt = src->h_ctg_alt;
	h->stats_on = src->stats_on; h->taps_on = src->taps_on; h->cigar_filter = src->cigar_filter; h->cfg = src->cfg;
	*out = h;
	return BWAGPU_OK;
}

// A handle on ANOTHER device of the node holding a copy of src's resident index: the three index buffers, the
// (possibly densified) SA, the contig table and the prefix tables travel device to device with hipMemcpyPeer -- point to point
// over xGMI, the single-process counterpart of the RCCL broadcast that bwa_amd/dist.py does between processes.  The new handle
// owns its copy; bwagpu_clone() on it gives further streams on that device.
static int clone_to_device_impl(bwagpu_t *src, int device, bwagpu_t **out)
{
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return BWAGPU_ENODEV;
	if (device == src->device) return bwagpu_clone(src, out);
	if (hipSetDevice(device) != hipSuccess) return BWAGPU_ENODEV;
	bwagpu_t *h = new bwagpu_s(); ++g_live_handles;
	h->device = device;
	h->ibuf = new bwagpu_s::IndexBufs();
	h->cfg = src->cfg;
	if (hipStreamCreate(&h->stream) != hipSuccess) { h->stream = nullptr; bwagpu_destroy(h); return BWAGPU_ENODEV; }
	for (int i = 0; i < 8; ++i) if (hipEventCreate(&h->ev[i]) != hipSuccess) { h->ev[i] = nullptr; bwagpu_destroy(h); return BWAGPU_ENODEV; }
	if (hipEventCreateWithFlags(&h->ev_wait, hipEventBlockingSync | hipEventDisableTiming) != hipSuccess) h->ev_wait = nullptr;
	struct { DevBuf *dst; const DevBuf *from; size_t bytes; } parts[] = {
		{ &h->ibuf->d_bwt, &src->ibuf->d_bwt, (size_t)src->bwt_bytes }, { &h->ibuf->d_sa, &src->ibuf->d_sa, (size_t)src->sa_bytes },
		{ &h->ibuf->d_pac, &src->ibuf->d_pac, (size_t)src->pac_bytes }, { &h->ibuf->d_ctg_off, &src->ibuf->d_ctg_off, (size_t)src->n_seqs * 8 },
		{ &h->ibuf->d_ctg_len, &src->ibuf->d_ctg_len, (size_t)src->n_seqs * 4 }, { &h->ibuf->d_ctg_alt, &src->ibuf->d_ctg_alt, (size_t)src->n_seqs * 4 },
		{ &h->ibuf->d_ptab, &src->ibuf->d_ptab, src->ix.ptab ? ((size_t)1 << (2 * src->ix.ptab_m)) * src->ix.ptab_m * sizeof(uint4) : 0 } };
	for (auto &pt : parts) {
		if (pt.bytes == 0) continue;
		if (pt.dst->ensure(pt.bytes)) { h->err = "hipMalloc failed (index copy)"; bwagpu_destroy(h); return BWAGPU_ENOMEM; }
		if (hipMemcpyPeer(pt.dst->p, device, pt.from->p, src->device, pt.bytes) != hipSuccess) { bwagpu_destroy(h); return BWAGPU_EHIP; }
	}
	h->ix = src->ix;
	h->ix.bwt = h->ibuf->d_bwt.as<uint4>(); h->ix.sa = h->ibuf->d_sa.as<u64>(); h->ix.pac = h->ibuf->d_pac.as<u8>();
	h->ix.ctg_off = h->ibuf->d_ctg_off.as<i64>(); h->ix.ctg_len = h->ibuf->d_ctg_len.as<i32>(); h->ix.ctg_alt = h->ibuf->d_ctg_alt.as<i32>();
	h->ix.ptab = src->ix.ptab ? h->ibuf->d_ptab.as<uint4>() : nullptr;
	h->bwt_blocks = src->bwt_blocks;
	if (src->ix.occ32) { if (int rc = build_occ32(h)) { bwagpu_destroy(h); return rc; } } else { h->ix.occ32 = nullptr; h->ix.occ_sb = nullptr; h->ix.occ_sbx = nullptr; h->ix.occ32_bytes = h->ix.occ_sbx_bytes = 0; }   // (rebuilt here rather than copied)
	h->l_pac = src->l_pac; h->n_seqs = src->n_seqs; h->seq_len = src->seq_len; h->sa_intv = src->sa_intv;
	h->bwt_blocks = src->bwt_blocks; h->bwt_bytes = src->bwt_bytes; h->sa_bytes = src->sa_bytes; h->pac_bytes = src->pac_bytes;
	h->bwt_size = src->bwt_size; h->n_sa = src->n_sa;
	h->h_ctg_off = src->h_ctg_off; h->h_ctg_len = src->h_ctg_len; h->h_ctg_alt = src->h_ctg_alt;
	h->stats_on = src->stats_on; h->taps_on = src->taps_on; h->cigar_filter = src->cigar_filter;
	{
		std::lock_guard<std::mutex> ls(src->ibuf->m);
		if (src->ibuf->have_names) {
			std::lock_guard<std::mutex> ld(h->ibuf->m);
			h->ibuf->ctg_text = src->ibuf->ctg_text; h->ibuf->ctg_name_off = src->ibuf->ctg_name_off; h->ibuf->ctg_anno_off = src->ibuf->ctg_anno_off;
			if (int rc = ctg_names_upload(h)) { bwagpu_destroy(h); return rc; }
			h->ibuf->have_names = true;
		}
	}
	*out = h;
	return BWAGPU_OK;
}

extern "C" int bwagpu_clone_to_device(bwagpu_t *src, int device, bwagpu_t **out)
{
	if (!src || !out) return BWAGPU_EINVAL;
	int prev = -1;
	if (hipGetDevice(&prev) != hipSuccess) prev = -1;
	const int rc = clone_to_device_impl(src, device, out);
	if (prev >= 0) (void)hipSetDevice(prev);      // the calling thread's current device is left as it was
	return rc;
}

extern "C" int bwagpu_index_buffers(bwagpu_t *h, void **bwt, uint64_t *bwt_bytes, void **sa, uint64_t *sa_bytes, void **pac, uint64_t *pac_bytes)
{
	if (!h || !bwt || !bwt_bytes || !sa || !sa_bytes || !pac || !pac_bytes) return BWAGPU_EINVAL;
	*bwt = h->ibuf->d_bwt.p; *bwt_bytes = h->bwt_bytes; *sa = h->ibuf->d_sa.p; *sa_bytes = h->sa_bytes; *pac = h->ibuf->d_pac.p; *pac_bytes = h->pac_bytes;
	return BWAGPU_OK;
}

// call on a handle created with NULL arrays once its buffers have been filled by the broadcast
extern "C" int bwagpu_index_ready(bwagpu_t *h)
{
	if (!h) return BWAGPU_EINVAL;
	HIPCHK(h, hipSetDevice(h->device));
	if (int rc = build_occ32(h)) return rc;
	return build_prefix_tables(h, (int)h->cfg.ptab_m);
}

extern "C" int bwagpu_index_export(const bwagpu_t *h, bwagpu_index_desc_t *d, int64_t *ctg_offset, int32_t *ctg_len, int32_t *ctg_is_alt)
{
	if (!h || !d) return BWAGPU_EINVAL;
	memset(d, 0, sizeof *d);
	d->bwt_size = h->bwt_size; d->primary = h->ix.primary; for (int i = 0; i < 5; ++i) d->L2[i] = h->ix.L2[i];
	d->seq_len = h->seq_len; d->n_sa = h->n_sa; d->sa_intv = h->sa_intv; d->l_pac = h->l_pac; d->n_seqs = h->n_seqs;
	if (ctg_offset) memcpy(ctg_offset, h->h_ctg_off.data(), (size_t)h->n_seqs * 8);
	if (ctg_len) memcpy(ctg_len, h->h_ctg_len.data(), (size_t)h->n_seqs * 4);
	if (ctg_is_alt) memcpy(ctg_is_alt, h->h_ctg_alt.data(), (size_t)h->n_seqs * 4);
	return BWAGPU_OK;
}

extern "C" int bwagpu_index_info(const bwagpu_t *h, int64_t *l_pac, int32_t *n_seqs, uint64_t *seq_len, int *sa_intv)
{
	if (!h) return BWAGPU_EINVAL;
	if (l_pac) *l_pac = h->l_pac;
	if (n_seqs) *n_seqs = h->n_seqs;
	if (seq_len) *seq_len = h->seq_len;
	if (sa_intv) *sa_intv = h->sa_intv;
	return BWAGPU_OK;
}

extern "C" int bwagpu_debug_phase(const bwagpu_t *h) { return h ? h->phase : -1; }
// diagnostic counters of the last batch_run (Counters::prof)
extern "C" int bwagpu_debug_prof(bwagpu_t *h, unsigned long long out[16])
{
	if (!h || !out || !h->d_ctr.p) return BWAGPU_EINVAL;
	Counters c;
	if (hipMemcpy(&c, h->d_ctr.p, sizeof c, hipMemcpyDeviceToHost) != hipSuccess) return BWAGPU_EHIP;
	for (int i = 0; i < 16; ++i) out[i] = c.prof[i];
	out[8] = c.n_vr_ovf + c.prof[8];       // long-read batches: tasks of pass 1 that were redone on full-size interval stacks; short-read batches: extensions k_ext_pack answered (the one is 0 where the other counts)
	out[0] = c.n_heavy; out[1] = c.n_p2_tasks;       // short-read batches: reads whose passes 1-2 ran as tasks, and their pass-2 searches
	return BWAGPU_OK;
}

// the prefix tables as the kernels read them (DevIndex::ptab): *m = their depth, *bytes = their size; with `out` given, that many bytes are copied there
extern "C" int bwagpu_debug_ptab(bwagpu_t *h, int32_t *m, uint64_t *bytes, void *out)
{
	if (!h || !m || !bytes) return BWAGPU_EINVAL;
	*m = h->ix.ptab ? h->ix.ptab_m : 0; *bytes = h->ix.ptab ? h->ix.ptab_bytes : 0;
	if (out && *bytes && hipMemcpy(out, h->ix.ptab, *bytes, hipMemcpyDeviceToHost) != hipSuccess) return BWAGPU_EHIP;
	return BWAGPU_OK;
}

// ... its index look-ups by interval size (Counters::seed_x2)
extern "C" int bwagpu_debug_seed_x2(bwagpu_t *h, unsigned long long out[8])
{
	if (!h || !out || !h->d_ctr.p) return BWAGPU_EINVAL;
	Counters c;
	if (hipMemcpy(&c, h->d_ctr.p, sizeof c, hipMemcpyDeviceToHost) != hipSuccess) return BWAGPU_EHIP;
	for (int i = 0; i < 8; ++i) out[i] = c.seed_x2[i];
	return BWAGPU_OK;
}
// ... and the histogram of k_seed's iterations per read (stats runs): out[b] = reads that took [2^(b-1), 2^b) iterations, out[32 + b] = their iterations summed
extern "C" int bwagpu_debug_hist(bwagpu_t *h, unsigned long long out[256])
{
	if (!h || !out || !h->d_ctr.p) return BWAGPU_EINVAL;
	Counters c;
	if (hipMemcpy(&c, h->d_ctr.p, sizeof c, hipMemcpyDeviceToHost) != hipSuccess) return BWAGPU_EHIP;
	for (int i = 0; i < 64; ++i) out[i] = c.seed_hist[i];
	for (int i = 0; i < 96; ++i) { out[64 + i] = c.wave_hist[0][i]; out[160 + i] = c.wave_hist[1][i]; }
	return BWAGPU_OK;
}
// ... and of the chaining tiers: out[t * 64 + b] = reads that finished in tier t with 16 b .. 16 b + 15 chains (b = 31: more), out[t * 64 + 32 + b] = with 32 b .. 32 b + 31 seeds
extern "C" int bwagpu_debug_chain_hist(bwagpu_t *h, unsigned long long out[192])
{
	if (!h || !out || !h->d_ctr.p) return BWAGPU_EINVAL;
	Counters c;
	if (hipMemcpy(&c, h->d_ctr.p, sizeof c, hipMemcpyDeviceToHost) != hipSuccess) return BWAGPU_EHIP;
	for (int t = 0; t < 3; ++t) for (int i = 0; i < 32; ++i) { out[t * 64 + i] = c.chain_hist[t][i]; out[t * 64 + 32 + i] = c.chain_seeds[t][i]; }
	return BWAGPU_OK;
}
extern "C" int bwagpu_set_stats(bwagpu_t *h, int enable) { if (!h) return BWAGPU_EINVAL; h->stats_on = enable ? 1 : 0; return BWAGPU_OK; }
extern "C" int bwagpu_set_cigar_filter(bwagpu_t *h, int enable) { if (!h) return BWAGPU_EINVAL; h->cigar_filter = enable ? 1 : 0; return BWAGPU_OK; }
extern "C" int bwagpu_set_taps(bwagpu_t *h, int enable) { if (!h) return BWAGPU_EINVAL; h->taps_on = enable ? 1 : 0; return BWAGPU_OK; }
extern "C" int bwagpu_get_stats(const bwagpu_t *h, bwagpu_stats_t *out) { if (!h || !out) return BWAGPU_EINVAL; *out = h->stats; return BWAGPU_OK; }

// ---- SA densification ---------------------------------------------------------------------------------------
// SA[next(k)] = SA[k] - 1 for next(k) = (k == primary ? 0 : LF(k)) (bwt_sa, bwt.c:91-103, read backwards), and `next` runs through all rows in
// one cycle.  So every row's value follows from ONE walk around that cycle: a lane starts at a row the old sampling holds, steps with LF and
// writes the rows on its way that the new sampling keeps, until it reaches the next row of the old sampling -- seq_len LF steps in all,
// where a walk per new sample (fm_sa) took old_intv - 1 steps on average for each of them (6.8x as many for 32 -> 4).  Row 0 is stored as
// -1 (bwtindex.c:bwt_cal_sa); the walk that starts there counts down from seq_len.  A lane takes its next start when its walk ends, not
// when the wave's longest one does: the loop is one LF step per lane and turn.
__global__ void __launch_bounds__(256) k_densify(DevIndex ix, u64 *out, u64 n_chains, int new_shift, u64 seq_len)
{
	const u64 stride = (u64)gridDim.x * blockDim.x, new_mask = ((u64)1 << new_shift) - 1;
	u64 c = (u64)blockIdx.x * blockDim.x + threadIdx.x, k = 0, v = 0;
	auto start = [&]() {
		k = c << ix.sa_shift;
		v = c == 0 ? seq_len : ix.sa[c];
		out[k >> new_shift] = c == 0 ? ~0ull : v;
	};
	if (c < n_chains) start();
	while (c < n_chains) {
		k = k == ix.primary ? 0 : fm_lf(ix, k);
		--v;
		if ((k & ix.sa_mask) == 0) { c += stride; if (c < n_chains) start(); }
		else if ((k & new_mask) == 0) out[k >> new_shift] = v;
	}
}

extern "C" int bwagpu_densify_sa(bwagpu_t *h, int new_intv)
{
	if (!h || new_intv <= 0 || (new_intv & (new_intv - 1)) || new_intv > h->sa_intv) return BWAGPU_EINVAL;
	if (new_intv == h->sa_intv) return BWAGPU_OK;
	if (h->ibuf->refs > 1) { h->err = "densify the SA before cloning the handle"; return BWAGPU_EINVAL; }
	HIPCHK(h, hipSetDevice(h->device));
	int sh = 0; while ((1 << sh) < new_intv) ++sh;
	u64 n_out = (h->seq_len + new_intv) / new_intv;
	DevBuf nb;
	if (nb.ensure(n_out * 8)) { h->err = "hipMalloc failed (dense SA)"; return BWAGPU_ENOMEM; }
	hipLaunchKernelGGL(k_densify, dim3((unsigned)((h->n_sa + 255) / 256 < 8192 ? (h->n_sa + 255) / 256 : 8192)), dim3(256), 0, h->stream, h->ix, nb.as<u64>(), (u64)h->n_sa, sh, (u64)h->seq_len);
	HIPCHK(h, hipGetLastError());
	HIPCHK(h, hipStreamSynchronize(h->stream));
	h->ibuf->d_sa.release();
	h->ibuf->d_sa = nb;
	h->ix.sa = h->ibuf->d_sa.as<u64>(); h->ix.sa_mask = (u64)new_intv - 1; h->ix.sa_shift = sh; h->sa_intv = new_intv;
	h->n_sa = n_out; h->sa_bytes = n_out * 8;
	return BWAGPU_OK;
}

static int sc_max_all(const bwagpu_opt_t *opt) { int m = 1; for (int k = 0; k < 25; ++k) if (opt->mat[k] > m) m = opt->mat[k]; return m; }

// ---- batches -------------------------------------------------------------------------------------------------
static const int BLOCK = 256;
static const int MAX_RESIDENT_THREADS = 256 * 2048;   // 256 CUs x 32 waves x 64 lanes
static const int WAVE_EXT_MAX_LEN = 1100;
static const int EXT_RING_MAX = 2048;      // the widest ring of {H,E} columns k_extend_wave<true> takes (bands beyond it: k_extend)
// the extension stage's switch points, as compiled (dev_extw.h, bwagpu_batch_run)
extern "C" void bwagpu_ext_limits(int32_t out[6])
{
	out[0] = CHAIN_SORT_LANE_MAX; out[1] = EXT_KEPT_SHORT * 64; out[2] = EXT_KEPT_RING * 64; out[3] = SEED_COVERED_STEP; out[4] = WAVE_EXT_MAX_LEN; out[5] = EXT_RING_MAX;
}
static const int SEED_LDS_ENT = 10;                     // 10 x 16 B x 256 lanes = 40 KiB of LDS per block -> 4 blocks (16 waves) per CU; measured best of {4,7,10,15}               // 4 waves x (8+5) B/column must fit the 64 KiB dynamic-LDS limit

static const int SEED_RD_MAX_LEN = 256;                 // the longest read of a batch whose reads get a 2-bit copy for k_seed's LDS (four 16-byte pieces per read)
static const int TASK_STACK_DFLT = 128;                 // BiIntv-sized entries of a task lane's spill area beyond PTAB_MAX (option seed_task_stack = 0)
// the seeding stage's switch points, as compiled and -- the prefix tables' depth -- as in force for the handle's index (h may be null: the option's default)
static const int SEED_LANE_LDS = 160;                   // LDS bytes per lane of k_seed at four blocks per CU: the read's 2-bit copy first, interval-stack entries with the rest
extern "C" void bwagpu_seed_limits(const bwagpu_t *h, int32_t out[10])
{
	out[0] = PTAB_MAX; out[1] = h ? h->ix.ptab_m : (int32_t)BwagpuConfig().ptab_m; out[2] = SEED_LDS_ENT; out[3] = SEED_RD_MAX_LEN; out[4] = WAVE_EXT_MAX_LEN;
	out[5] = SEED_CAND_BITS; out[6] = PUB_MAX; out[7] = PTAB_MAX + TASK_STACK_DFLT; out[8] = SEED_LANE_LDS; out[9] = h ? h->seed_lds_run : 0;
}

// first guess of a batch's arena sizes from its shape (n_reads, n_bases, max_len); grown on overflow
static void size_arenas(bwagpu_t *h)
{
	const int n = h->n_reads;
	i64 nb = h->n_bases > 1024 ? h->n_bases : 1024;
	h->slot_cap = nb / 3 + 4096;     // (a 3.1 Gbp repeat-rich genome needs ~0.26 slots and ~0.15 region records per base)
	h->node_cap = h->slot_cap / 4 + 2 * (i64)n + 64;
	h->reg_cap = nb / 5 + 4096;
	// capacity of one read's interval list: reads keep ~10-30 intervals whatever their length class; grown x4 on overflow
	// (256 at least: with 64, one read in ten thousand of a repeat-rich genome -- a 150 bp read inside a tandem array leaves well over a hundred
	// intervals -- made the first batch of every handle run twice, profiles/r04_e2e_split.log)
	h->mem_cap = h->max_len / 3 < 256 ? 256 : h->max_len / 3;
	// what earlier batches -- of this handle or of another handle on the same index -- turned out to need carries over
	{
		std::lock_guard<std::mutex> l(h->ibuf->m);
		if (h->ibuf->need_slot > h->need_slot) h->need_slot = h->ibuf->need_slot;
		if (h->ibuf->need_node > h->need_node) h->need_node = h->ibuf->need_node;
		if (h->ibuf->need_reg > h->need_reg) h->need_reg = h->ibuf->need_reg;
		if (h->ibuf->need_mem > h->need_mem) h->need_mem = h->ibuf->need_mem;
	}
	if ((i64)(h->need_slot * nb) > h->slot_cap) h->slot_cap = (i64)(h->need_slot * nb);
	if ((i64)(h->need_node * nb) > h->node_cap) h->node_cap = (i64)(h->need_node * nb);
	if ((i64)(h->need_reg * nb) > h->reg_cap) h->reg_cap = (i64)(h->need_reg * nb);
	if (h->need_mem > h->mem_cap) h->mem_cap = h->need_mem;
	if (h->cfg.mem_cap > 0) h->mem_cap = (int)h->cfg.mem_cap;   // test hook: force the overflow/retry path
}

// resident lanes of the lane-per-read kernels: enough to fill the chip, bounded by the seeding scratch budget (2 interval stacks per lane)
static int resident_threads(const bwagpu_t *h)
{
	const int BLOCK_ = 256;
	size_t per_lane = (size_t)(h->max_len + 1 + PTAB_MAX) * sizeof(BiIntv) + (size_t)2 * (h->max_len + 2) * 4;
	size_t budget = (size_t)12 << 30;
	i64 max_thr = (i64)(budget / per_lane);
	if (max_thr > 256 * 2048) max_thr = 256 * 2048;
	if (max_thr < BLOCK_) max_thr = BLOCK_;
	int n_threads = (int)(((i64)h->n_reads + BLOCK_ - 1) / BLOCK_ * BLOCK_);
	if (n_threads > max_thr) n_threads = (int)(max_thr / BLOCK_ * BLOCK_);
	return n_threads;
}

extern "C" int bwagpu_batch_upload(bwagpu_t *h, int n, const uint8_t *seqs, const int64_t *off)
{
	if (!h || n < 0 || (n > 0 && (!seqs || !off))) return BWAGPU_EINVAL;
	HIPCHK(h, hipSetDevice(h->device));
	h->have_batch = false; h->ran = false; h->packed_tot = -1; h->downloaded = false; h->cig_ext_n = -1; h->phase = 10;
	h->n_reads = n; h->max_len = 0; h->n_bases = n ? off[n] - off[0] : 0;
	if (n && off[0] != 0) return BWAGPU_EINVAL;
	for (int i = 0; i < n; ++i) {
		i64 l = off[i + 1] - off[i];
		if (l < 0 || l > 0x3fffffff) return BWAGPU_EINVAL;
		if (l > h->max_len) h->max_len = (int)l;
	}
	h->h_off.assign(off, off + n + 1);
	const u64 n_words = ((u64)h->n_bases + 15) / 16;
	h->phase = 11;
	if (h->d_seq.ensure((size_t)h->n_bases + 16) || h->d_seq_nib.ensure((size_t)(n_words + 1) * 8) || h->d_off.ensure((size_t)(n + 1) * 8)) { h->err = "hipMalloc failed (reads)"; return BWAGPU_ENOMEM; }
	if (n) {
		HIPCHK(h, hipMemcpyAsync(h->d_seq.p, seqs, (size_t)h->n_bases, hipMemcpyHostToDevice, h->stream));
		HIPCHK(h, hipMemcpyAsync(h->d_off.p, off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, h->stream));
		h->phase = 12;
		Batch P = {}; P.seq = h->d_seq.as<u8>(); P.seq_nib = h->d_seq_nib.as<u64>();
		u64 pb = (n_words + BLOCK - 1) / BLOCK;
		hipLaunchKernelGGL(k_pack_reads, dim3((unsigned)(pb < 65536 ? pb : 65536)), dim3(BLOCK), 0, h->stream, P, n_words);
		HIPCHK(h, hipGetLastError());
		// reads of up to 256 bases: a 2-bit copy per read for the seeding kernel's LDS
		h->rd_words = (h->max_len <= SEED_RD_MAX_LEN && h->cfg.seed_rd_lds != 0) ? (((h->max_len + 15) / 16 + 3) & ~3) : 0;
		if (h->rd_words) {
			if (h->d_seq_2b.ensure((size_t)n * h->rd_words * 4 + 64) || h->d_seq_flags.ensure((size_t)n + 16)) { h->err = "hipMalloc failed (reads)"; return BWAGPU_ENOMEM; }
			HIPCHK(h, hipMemsetAsync(h->d_seq_flags.p, 0, (size_t)n, h->stream));
			P.off = h->d_off.as<i64>(); P.n_reads = n; P.rd_words = h->rd_words; P.seq_2b = h->d_seq_2b.as<u32>(); P.seq_flags = h->d_seq_flags.as<u8>();
			const u64 tb = ((u64)n * h->rd_words + BLOCK - 1) / BLOCK;
			hipLaunchKernelGGL(k_pack_reads2b, dim3((unsigned)(tb < 65536 ? tb : 65536)), dim3(BLOCK), 0, h->stream, P);
			HIPCHK(h, hipGetLastError());
		}
		HIPCHK(h, wait_stream(h));
	}
	size_arenas(h);
	h->have_batch = true;
	return BWAGPU_OK;
}

// Waves that own a DP scratch region (dp_h / dp_e).  The lane-per-read kernels need one per wave of the seeding grid; the wave-per-read
// kernels of long-read batches (k_seedsw_wave, k_dedup_wave) should fill the chip whatever that grid is -- for 10 kb reads the seeding
// scratch limits it to a few dozen waves, which left 2000 reads to 32 waves (measured: 3.1 of a batch's 4.8 s) -- so they get up to 1024.
static int dp_wave_count(const bwagpu_t *h, int n_threads)
{
	int w = (n_threads + 63) / 64;
	if (h->max_len > WAVE_EXT_MAX_LEN) { int want = h->n_reads < 1024 ? h->n_reads : 1024; if (want > w) w = want; }
	return w;
}

static int alloc_batch(bwagpu_t *h, int n_threads, int seed_lanes)
{
	int n = h->n_reads; size_t sc = (size_t)h->slot_cap + 8;   // +8: chunked readers may touch a few slots past the last read's range
	int bad = 0;
	bad |= h->d_ctr.ensure(sizeof(Counters));
	bad |= h->d_tmp_intv.ensure((size_t)(seed_lanes > n_threads ? seed_lanes : n_threads) * (h->max_len + 1 + PTAB_MAX) * sizeof(BiIntv));
	bad |= h->d_intv_n.ensure((size_t)n * 4 + 16); bad |= h->d_intv_off.ensure((size_t)n * 8 + 16);
	bad |= h->d_intv.ensure(((size_t)n * h->mem_cap + 16) * sizeof(Intv3));
	bad |= h->d_seed_n.ensure((size_t)n * 4 + 16); bad |= h->d_seed_off.ensure((size_t)n * 8 + 16);
	bad |= h->d_slot_pos.ensure(sc * 8); bad |= h->d_slot_qbeg.ensure(sc * 4); bad |= h->d_slot_len.ensure(sc * 4); bad |= h->d_slot_rid.ensure(sc * 4); bad |= h->d_slot_blob.ensure(sc * SLOT_BLOB_BYTES);
	bad |= h->d_chain_n.ensure((size_t)n * 4 + 16); bad |= h->d_node_off.ensure((size_t)n * 8 + 16);
	bad |= h->d_nodes.ensure((size_t)h->node_cap * BT_NODE_INTS * 4);
	bad |= h->d_reg_off.ensure((size_t)n * 8 + 16); bad |= h->d_reg_cap_r.ensure((size_t)n * 4 + 16);
	bad |= h->d_reg_n_raw.ensure((size_t)n * 4 + 16); bad |= h->d_reg_n.ensure((size_t)n * 4 + 16);
	bad |= h->d_regs.ensure((size_t)h->reg_cap * sizeof(bwagpu_alnreg_t));
	if (h->taps_on) bad |= h->d_regs_raw.ensure((size_t)h->reg_cap * sizeof(bwagpu_alnreg_t));
	int n_waves = dp_wave_count(h, n_threads);
	bad |= h->d_dp_h.ensure((size_t)n_waves * (h->max_len + 2) * DPS * 4);
	bad |= h->d_dp_e.ensure((size_t)n_waves * (h->max_len + 2) * DPS * 4);
	bad |= h->d_minhsp.ensure((size_t)(h->max_len + 2) * 4);
	bad |= h->d_order.ensure((size_t)n * 4 + 16); bad |= h->d_bin_cnt.ensure(2 * ORDER_BINS * 4); bad |= h->d_seed_w.ensure((size_t)n * 4 + 16); bad |= h->d_seed_order.ensure((size_t)n * 4 + 16);
	if (bad) { h->err = "hipMalloc failed (batch arenas)"; return BWAGPU_ENOMEM; }
	return 0;
}

// heavy-first processing order of the batch by a per-read weight array (device)
static int order_reads(bwagpu_t *h, const Batch &B, const i32 *weight)
{
	HIPCHK(h, hipMemsetAsync(B.bin_cnt, 0, 2 * ORDER_BINS * 4, h->stream));
	int nb = (B.n_reads + BLOCK - 1) / BLOCK; if (nb > 1024) nb = 1024;
	int chunk = (B.n_reads + nb - 1) / nb;
	hipLaunchKernelGGL(k_order_count, dim3(nb), dim3(BLOCK), 0, h->stream, B, weight);
	hipLaunchKernelGGL(k_order_scan, dim3(1), dim3(64), 0, h->stream, B);
	hipLaunchKernelGGL(k_order_fill, dim3(nb), dim3(BLOCK), 0, h->stream, B, weight, chunk);
	return 0;
}

static void release_reserved(bwagpu_t *h) { for (void *&p : h->reserved) { if (p) bwagpu_free(p); p = nullptr; } }

// Allocate now what a batch of this shape will need -- read arrays, arenas, scratch, packed results: device buffers are only ever grown, so
// the first real batch of the handle finds them in place instead of spending ~0.4 s in hipMalloc inside the pipeline.
extern "C" int bwagpu_batch_reserve(bwagpu_t *h, int n_reads, int64_t n_bases, int max_len)
{
	if (!h || n_reads <= 0 || n_bases <= 0 || max_len <= 0 || max_len > 0x3fffffff) return BWAGPU_EINVAL;
	HIPCHK(h, hipSetDevice(h->device));
	const int n0 = h->n_reads, m0 = h->max_len; const i64 b0 = h->n_bases; const bool have0 = h->have_batch, ran0 = h->ran;
	const i64 sc0 = h->slot_cap, nc0 = h->node_cap, rc0 = h->reg_cap; const int mc0 = h->mem_cap;
	h->n_reads = n_reads; h->n_bases = n_bases; h->max_len = max_len;
	size_arenas(h);
	int bad = alloc_batch(h, resident_threads(h), 0) != 0;
	const u64 n_words = ((u64)n_bases + 15) / 16;
	const int rdw = max_len <= SEED_RD_MAX_LEN ? (((max_len + 15) / 16 + 3) & ~3) : 0;
	bad |= h->d_seq.ensure((size_t)n_bases + 16); bad |= h->d_seq_nib.ensure((size_t)(n_words + 1) * 8); bad |= h->d_off.ensure((size_t)(n_reads + 1) * 8);
	if (rdw) { bad |= h->d_seq_2b.ensure((size_t)n_reads * rdw * 4 + 64); bad |= h->d_seq_flags.ensure((size_t)n_reads + 16); }
	const i64 tot = (i64)n_reads * 4;        // (packed results: ~3.2 regions per read on a repeat-rich genome)
	bad |= h->d_pack_off.ensure((size_t)n_reads * 8); bad |= h->d_regs_packed.ensure((size_t)tot * sizeof(bwagpu_alnreg_t)); bad |= h->d_pack_read.ensure((size_t)tot * 4);
	bad |= h->d_cigs.ensure((size_t)tot * sizeof(bwagpu_cigar_t)); bad |= h->d_cig_ext.ensure((size_t)(tot * 4 + 65536) * 4);
	// ... and the page-locked blocks its results will be copied into (regions, CIGAR records, operation array: ~0.4 GB per 667 k reads; page-locking costs
	// more than the copy -- ~0.2 ms per MB -- and the pool keeps what it is given back, so the handle's first batch finds them)
	if (h->cfg.reserve_results && !g_dry_sum) {
		// (held by the handle until its first download asks for blocks: handles that reserve one after another would otherwise all be handed the same three idle blocks)
		release_reserved(h);
		h->reserved[0] = result_alloc((size_t)tot * sizeof(bwagpu_alnreg_t)); h->reserved[1] = result_alloc((size_t)tot * sizeof(bwagpu_cigar_t)); h->reserved[2] = result_alloc((size_t)tot * 2 * 4);
	}
	h->n_reads = n0; h->n_bases = b0; h->max_len = m0; h->have_batch = have0; h->ran = ran0;
	h->slot_cap = sc0; h->node_cap = nc0; h->reg_cap = rc0; h->mem_cap = mc0;
	if (bad) { h->err = "hipMalloc failed (reserve)"; return BWAGPU_ENOMEM; }
	return BWAGPU_OK;
}

// Device memory a handle's buffers would GROW by for a batch of this shape (bytes; what bwagpu_batch_reserve would allocate now), and the device's
// free / total memory: what a caller needs to decide how much HBM it can spend on a denser suffix array before the batches arrive.
extern "C" int64_t bwagpu_batch_footprint(bwagpu_t *h, int n_reads, int64_t n_bases, int max_len)
{
	if (!h || n_reads <= 0 || n_bases <= 0 || max_len <= 0 || max_len > 0x3fffffff) return -1;
	size_t sum = 0;
	g_dry_sum = &sum;
	const int rc = bwagpu_batch_reserve(h, n_reads, n_bases, max_len);
	g_dry_sum = nullptr;
	return rc == BWAGPU_OK ? (int64_t)sum : -1;
}
extern "C" int bwagpu_mem_info(bwagpu_t *h, uint64_t *free_bytes, uint64_t *total_bytes)
{
	if (!h) return BWAGPU_EINVAL;
	HIPCHK(h, hipSetDevice(h->device));
	size_t f = 0, t = 0;
	HIPCHK(h, hipMemGetInfo(&f, &t));
	if (free_bytes) *free_bytes = f;
	if (total_bytes) *total_bytes = t;
	return BWAGPU_OK;
}

namespace { struct BusyGuard { std::atomic<int> &c; int others; explicit BusyGuard(std::atomic<int> &c_) : c(c_), others(c_.fetch_add(1)) {} ~BusyGuard() { --c; } }; }
// ---- the de-duplication stage's plan and launches (bwagpu_batch_run and bwagpu_dedup_flat) ----------------------------------------------------------------
// heavy_min: regions from which k_dedup leaves a read to the wave-per-read launches (0: it does every read itself); rc, q_cap, lds0: the patch alignments' ring,
// query room and their LDS bytes; cap_m / cap_b: regions the LDS arrays of the two list launches hold; blk_m / blk_b: their workgroups
#define DEDUP_HEAVY_DEFAULT 3      // options dedup_heavy and dedup_stage left at auto
#define DEDUP_STAGE_DEFAULT 128
#define DEDUP_RING_MIN 256         // columns of the patch alignments' smallest ring
struct DedupPlan { int heavy_min = 0, rc = 0, q_cap = 0, cap_m = 0, cap_b = 0; size_t lds0 = 0; long long blk_m = 0, blk_b = 0; };
static long long share_of(long long g, bool long_batch, long long share_pct)      // option share (see bwagpu_batch_run): g workgroups fill the chip; a short-read batch launches share_pct percent of them
{
	if (long_batch || share_pct >= 100 || share_pct <= 0) return g;
	const long long v = g * share_pct / 100; return v < 1 ? 1ll : v;
}
// The plan for n reads of up to max_len bases; dp_waves: the scratch regions dp_h / dp_e will hold.  Sizes the handle's list and staging buffers.
static int dedup_plan(bwagpu_t *h, const bwagpu_opt_t *opt, const BwagpuConfig &cfg, int max_len, int n, bool long_batch, long long share_pct, long long dp_waves, DedupPlan &dd)
{
	dd = DedupPlan();
	// k_dedup's list of the reads it leaves to the wave-per-read kernel: the seeding kernels' list of heavy reads, free again by then
	dd.heavy_min = long_batch || cfg.dedup_wave || h->seq_len >= ((u64)1 << 47) || max_len >= (1 << 16) ? 0 : (int)(cfg.dedup_heavy < 0 ? DEDUP_HEAVY_DEFAULT : cfg.dedup_heavy);     // (the bounds: DdKey, dev_dedupp.h)
	if (dd.heavy_min > 0) {
		int need = 8 * opt->w + 4 + 128; if (need < max_len / 4 + 132) need = max_len / 4 + 132;
		dd.rc = DEDUP_RING_MIN; while (dd.rc < need && dd.rc < 4096) dd.rc <<= 1;
		dd.q_cap = (max_len + 15) & ~15;
		if (8 * dd.rc + 32 + dd.q_cap > 65536) dd.q_cap = 0;
		dd.lds0 = (size_t)8 * dd.rc + 32 + dd.q_cap;
		const long long room = (65536 - (long long)dd.lds0) / (long long)DDP_LDS_PER_REG;       // regions a workgroup's LDS holds next to the ring
		dd.cap_m = (int)(cfg.dedup_stage < 0 ? DEDUP_STAGE_DEFAULT : cfg.dedup_stage); if (dd.cap_m > room) dd.cap_m = (int)(room > 0 ? room : 0);
		dd.cap_b = (int)(cfg.dedup_big < 0 ? room : cfg.dedup_big); if (dd.cap_b > room) dd.cap_b = (int)(room > 0 ? room : 0);
		const long long wpc_m = (160 * 1024) / (long long)(dd.lds0 + DDW_PAR_BYTES(dd.cap_m)), wpc_b = (160 * 1024) / (long long)(dd.lds0 + DDW_PAR_BYTES(dd.cap_b));
		dd.blk_m = share_of(256 * (wpc_m > 12 ? 12 : wpc_m), long_batch, share_pct); dd.blk_b = share_of(256 * (wpc_b > 12 ? 12 : wpc_b), long_batch, share_pct);
		const long long cap = dp_waves > 0 ? dp_waves : 1;       // (dp_h / dp_e hold one scratch region per wave)
		if (dd.blk_m > cap) dd.blk_m = cap; if (dd.blk_b > cap) dd.blk_b = cap;
		if (dd.blk_m > n) dd.blk_m = n; if (dd.blk_b > n) dd.blk_b = n;
		if (h->d_heavy.ensure((size_t)n * 4 + 16) || h->d_dd_tmp.ensure(((size_t)dd.blk_m * dd.cap_m + (size_t)dd.blk_b * dd.cap_b) * sizeof(bwagpu_alnreg_t) + 16)) { h->err = "hipMalloc failed (de-duplication lists)"; return BWAGPU_ENOMEM; }
	}
	return BWAGPU_OK;
}
// The stage's kernels on batch B (n reads of up to max_len bases; lane_blocks: workgroups of the lane-per-read kernel); sets B's dd_* fields.
static void dedup_launch(bwagpu_t *h, const bwagpu_opt_t *opt, const BwagpuConfig &cfg, Batch &B, int max_len, int n, bool long_batch, long long share_pct, unsigned lane_blocks, const DedupPlan &dd)
{
	const dim3 block(BLOCK);
	if (long_batch || cfg.dedup_wave) {     // long reads: few reads, long patch alignments -> one wavefront per read
		// Ring of {H,E} columns for the patch alignments' band: 2 w + 132 columns, where w = max(min(.., 4 opt.w), |rlen - l_query| + 3) (bwa.c:180-187)
		// and the length difference of two merged regions of a 10 kb read with 13 % indels runs to several hundred bases.  A band the ring
		// cannot hold falls back to one lane with its columns in HBM -- 10^7 cells at one lane's pace: measured 0.6 s per call, 58 s of a
		// 100-read batch's 59 (profiles/r03_longread_probe.md) -- so the ring is sized for 1/8 of the longest read and capped by what one
		// wave's LDS share allows; wider rings mean fewer waves per workgroup (the dynamic LDS of a workgroup is 64 KiB).
		int need = 8 * opt->w + 4 + 128; if (need < max_len / 4 + 132) need = max_len / 4 + 132;
		int rc_ = DEDUP_RING_MIN; while (rc_ < need && rc_ < 4096) rc_ <<= 1;
		if (cfg.dedup_ring > 0) rc_ = (int)cfg.dedup_ring;      // test hook: a power of two, 256..4096
		if (rc_ < DEDUP_RING_MIN || rc_ > 4096 || (rc_ & (rc_ - 1))) rc_ = 1024;
		const bool dedup_blk = (cfg.dedup_blk >= 0 ? cfg.dedup_blk : 1) != 0;   // four columns per lane in the patch alignments (wave_global2_score_ring_blk: 381 -> 207 ms per 6000 x 10 kb reads, BENCH_r03 variants); needs the segment in LDS
		int q_cap = dedup_blk ? (max_len + 15) & ~15 : 0;      // room for a patch alignment's query segment next to the ring
		if (8 * rc_ + 32 + q_cap > 65536) q_cap = 0;
		int wpb = rc_ <= 1024 ? 4 : (rc_ <= 2048 ? 2 : 1);
		while (wpb > 1 && (8 * rc_ + 32 + q_cap) * wpb > 65536) wpb >>= 1;
		i64 nblk = ((i64)n + wpb - 1) / wpb, cap = B.dp_waves / wpb > 0 ? B.dp_waves / wpb : 1;   // dp_h/dp_e hold one scratch region per wave
		if (dedup_blk && q_cap) hipLaunchKernelGGL(k_dedup_wave<true>, dim3((unsigned)(nblk < cap ? nblk : cap)), dim3(64 * wpb), (size_t)(8 * rc_ + 32 + q_cap) * wpb, h->stream, h->ix, *opt, B, rc_, q_cap, 0, 0, (bwagpu_alnreg_t*)nullptr);
		else hipLaunchKernelGGL(k_dedup_wave<false>, dim3((unsigned)(nblk < cap ? nblk : cap)), dim3(64 * wpb), (size_t)(8 * rc_ + 32 + q_cap) * wpb, h->stream, h->ix, *opt, B, rc_, q_cap, 0, 0, (bwagpu_alnreg_t*)nullptr);
	} else {
		// Lane per read for the reads with one or two regions (nine in ten of the headline's); the others are listed by k_dedup and done by two more
		// launches, one wavefront per read with the decisions' operands in LDS (dedup_read_par, dev_dedupp.h): the reads of up to dedup_stage regions
		// (16.6 KB of LDS per wave, nine to a CU), then the few with more (up to dedup_big regions in 64 KB; beyond that, in place in HBM).
		B.dd_heavy_min = dd.heavy_min; B.dd_list = h->d_heavy.as<i32>(); B.dd_prio = cfg.dedup_prio != 0; B.dd_net = (int)(cfg.dedup_net < 0 ? DEDUP_NET_DEFAULT : cfg.dedup_net);
		B.dd_stage_cap = dd.cap_m > 0 ? dd.cap_m : 0x3fffffff;      // (no LDS arrays: one list, every read in place)
		hipLaunchKernelGGL(k_dedup, dim3((unsigned)share_of(lane_blocks, long_batch, share_pct)), block, 0, h->stream, h->ix, *opt, B);
		if (B.dd_heavy_min > 0) {
			bwagpu_alnreg_t *tmp = h->d_dd_tmp.as<bwagpu_alnreg_t>();
			const size_t lds_m = dd.lds0 + DDW_PAR_BYTES(dd.cap_m), lds_b = dd.lds0 + DDW_PAR_BYTES(dd.cap_b);
			if (dd.q_cap) hipLaunchKernelGGL((k_dedup_wave<true, true>), dim3((unsigned)dd.blk_m), dim3(64), lds_m, h->stream, h->ix, *opt, B, dd.rc, dd.q_cap, dd.cap_m, 0, tmp);
			else hipLaunchKernelGGL((k_dedup_wave<false, true>), dim3((unsigned)dd.blk_m), dim3(64), lds_m, h->stream, h->ix, *opt, B, dd.rc, dd.q_cap, dd.cap_m, 0, tmp);
			if (dd.cap_m > 0) {
				tmp += (size_t)dd.blk_m * dd.cap_m;
				if (dd.q_cap) hipLaunchKernelGGL((k_dedup_wave<true, true>), dim3((unsigned)dd.blk_b), dim3(64), lds_b, h->stream, h->ix, *opt, B, dd.rc, dd.q_cap, dd.cap_b, 1, tmp);
				else hipLaunchKernelGGL((k_dedup_wave<false, true>), dim3((unsigned)dd.blk_b), dim3(64), lds_b, h->stream, h->ix, *opt, B, dd.rc, dd.q_cap, dd.cap_b, 1, tmp);
			}
		}
	}
}

extern "C" int bwagpu_batch_run(bwagpu_t *h, const bwagpu_opt_t *opt)
{
	if (!h || !opt || !h->have_batch) return BWAGPU_EINVAL;
	const BusyGuard busy(h->ibuf->busy);
	if (opt->e_del <= 0 || opt->e_ins <= 0 || opt->max_occ <= 0 || opt->min_seed_len <= 0 || opt->w < 0) return BWAGPU_EINVAL;
	HIPCHK(h, hipSetDevice(h->device));
	memset(&h->stats, 0, sizeof h->stats);
	h->stats.n_reads = h->n_reads; h->stats.n_bases = h->n_bases;
	h->ran = false; h->packed_tot = -1; h->downloaded = false; h->cig_ext_n = -1;      // regions packed by an earlier download (and their CIGAR operations) belong to the previous run
	if (h->n_reads == 0) { h->ran = true; return BWAGPU_OK; }
	int n = h->n_reads;
	// resident lanes: enough to fill the chip, bounded by the seeding scratch budget (2 interval stacks per lane)
	const int n_threads = resident_threads(h);
	// mem_flt_chained_seeds thresholds per read length (bwamem.c:626-628); log() stays on the host
	std::vector<i32> minhsp(h->max_len + 2, -1);
	bool any_seedsw = false;
	for (int l = 1; l <= h->max_len; ++l) {
		double min_l = opt->min_chain_weight ? 1.1f * opt->min_chain_weight : 5.5f * log((double)l);
		if (!(min_l > 0.05f * l)) { minhsp[l] = (int)(opt->a * min_l + .499); any_seedsw = true; }
	}
	const BwagpuConfig &cfg = h->cfg;            // (no batch call reads the environment: bwagpu_config.h)
	const bool dbg_sync = cfg.debug_sync != 0;   // diagnostics: wait and report after every stage
	// Long-read batches (a read beyond the short-read extension kernel's columns) default to the kernel forms BENCH_r03's `variants` measured
	// fastest for them, identical regions: seeding by chunks with one memory round trip per iteration, workgroup-per-read interval sort, LDS
	// seed re-scoring, four columns per lane in the patch alignments.  An explicit option (>= 0) overrides either way.
	const bool long_batch = h->max_len > WAVE_EXT_MAX_LEN;
	// Option share (percent; short-read batches): the persistent kernels of the hot path launch with that share of the workgroups that would fill
	// the chip.  A kernel whose workgroups live until its work runs out holds every slot it got: launched to fill the chip, the kernels of the
	// batches in flight take turns; launched for a share, kernels of different batches -- the memory-bound seeding of one, the issue-bound
	// extension of another -- run side by side.
	// auto (-1): half the chip per kernel when at least three handles share this index -- three batches in flight, the way `bwa-amd mem` and the bench's timed loop
	// drive a device -- and another of them has kernels in flight as this run starts; else all of it (a lone handle; the first batch of a pipeline, which has
	// the chip to itself while the reader is still parsing the second: 151 -> ~90 ms, `profiles/r05_e2e_reserve_results.log`).  Measured with three batches in flight (profiles/r05_share_ab.log): 108.3 ms per step at 100, 105.2-105.7 at 50 (105.1 at 40,
	// 107.1 at 60), i.e. -2.7 %, for +10 % on a batch that has the chip to itself (131.8 -> 144.8 ms) -- round 4 measured nothing; the kernels' balance has moved.
	const long long share_pct = cfg.share >= 0 ? cfg.share : (h->ibuf->refs.load() >= 3 && busy.others > 0 ? 50 : 100);
	auto share = [&](long long g) { return share_of(g, long_batch, share_pct); };
	auto pick = [&](long long v, long long dflt_long) { return v >= 0 ? v : (long_batch ? dflt_long : 0); };
	// Pass 1 of long-read batches as independent tasks (option seed_tasks; dev_seed.h, k_seed's LR): one task per read and min_seed_len-th
	// position.  The host only says where each read's tasks begin; a task finds its read by bisection.
	bool seed_tasks = pick(cfg.seed_tasks, 1) != 0;
	int n_vreads = 0, task_lanes = 0;
	const int TASK_STACK_CAP = PTAB_MAX + (cfg.seed_task_stack > 0 ? (int)((cfg.seed_task_stack + 1) / 2) : TASK_STACK_DFLT);          // BiIntv-sized entries of a task lane's spill area (default: 256 packed entries; a full stack hands the task to the second launch)
	if (!long_batch || h->max_len >= 65536 || h->seq_len >= ((u64)1 << 37) || h->ix.occ32 == nullptr || h->ix.ptab == nullptr || h->rd_words != 0 || opt->min_seed_len < 1 || cfg.seed_pass3_inline) seed_tasks = false;
	if (seed_tasks) {
		std::vector<i32> first((size_t)n + 1);
		i64 tot = 0;
		for (int r = 0; r < n; ++r) { first[r] = (i32)tot; tot += (h->h_off[r + 1] - h->h_off[r] + opt->min_seed_len - 1) / opt->min_seed_len; }
		first[n] = (i32)tot;
		if (tot <= 0 || tot > 0x7fffffff) seed_tasks = false;
		else {
			n_vreads = (int)tot;
			task_lanes = (int)((tot + BLOCK - 1) / BLOCK * BLOCK); if (task_lanes > 256 * 3 * BLOCK) task_lanes = 256 * 3 * BLOCK;   // persistent lanes (three workgroups per CU), tasks drawn from a counter
			if (h->d_vr_tab.ensure(((size_t)n + 1) * 4) || h->d_vr_ovf.ensure((size_t)n_vreads * 4 + 16) || h->d_intv_n3.ensure((size_t)n * 4 + 16)) { h->err = "hipMalloc failed (seeding tasks)"; return BWAGPU_ENOMEM; }
			HIPCHK(h, hipMemcpyAsync(h->d_vr_tab.p, first.data(), first.size() * 4, hipMemcpyHostToDevice, h->stream));   // (pageable source: staged before the call returns)
		}
	}
	if (dbg_sync) fprintf(stderr, "[bwagpu] pass 1 by tasks: %d tasks on %d lanes (max_len %d, step %d)\n", n_vreads, task_lanes, h->max_len, opt->min_seed_len);
	// Short-read batches: a read on which a lane of the lane-per-read kernel has spent more than option seed_budget iterations (default 8192: 0.15 % of
	// the bench's reads -- and the whole of that kernel's critical path; measured over budgets 2048..8192: profiles/r04_seed_budget_ab.jsonl) is given up there and seeded by the task kernels afterwards (dev_seed.h, LR).
	// Round 6 (profiles/r06_seed_budget.md): alone on the chip the stage is shortest at ~6 k iterations (50.5 ms against 55.5 at 8192, 59.8 at 12288: the main
	// kernel's tail of nearly empty waves ends sooner); with other batches' kernels on the chip that tail costs nothing -- they fill it -- and the step is best
	// with fewer reads handed to the chip-filling task kernels (86.3-87.6 ms at 12288 against 87.1-89.1 at 8192).  So auto follows the same signal as `share`.
	const int seed_budget = (int)(cfg.seed_budget < 0 ? (share_pct < 100 ? 12288 : 6144) : cfg.seed_budget);
	const int heavy_tpr = opt->min_seed_len > 0 ? (h->max_len + opt->min_seed_len - 1) / opt->min_seed_len : 0;
	// The one-trip seeding kernels (MRG = 2) address the index through buffer descriptors: 32-bit byte offsets into tables of less than 4 GiB.  The heavy
	// reads' task kernels exist in that form only, so an index beyond a descriptor's reach (occ32 above 4 GiB: a genome of more than ~4.3 Gbp; a deep
	// prefix table) keeps every read on the lane-per-read kernel, without a budget (option idx_desc_max_mb lowers the limit: test hook).
	const u64 desc_max = cfg.idx_desc_max_mb > 0 && ((u64)cfg.idx_desc_max_mb << 20) < BUF_MAX_BYTES ? (u64)cfg.idx_desc_max_mb << 20 : BUF_MAX_BYTES;
	const bool idx_in_desc = h->ix.occ32 != nullptr && h->ix.ptab != nullptr && h->ix.occ32_bytes <= desc_max && h->ix.ptab_bytes <= desc_max;
	const bool heavy_tasks = !long_batch && h->rd_words != 0 && seed_budget > 0 && heavy_tpr > 0 && idx_in_desc &&
							 h->seq_len < ((u64)1 << 37) && !cfg.seed_pass3_inline && opt->max_mem_intv > 0;
	const int heavy_lanes = heavy_tasks ? (int)(((i64)n * heavy_tpr + BLOCK - 1) / BLOCK * BLOCK < 256 * 3 * BLOCK ? ((i64)n * heavy_tpr + BLOCK - 1) / BLOCK * BLOCK : 256 * 3 * BLOCK) : 0;
	if (heavy_tasks && (h->d_intv_n3.ensure((size_t)n * 4 + 16) || h->d_heavy.ensure((size_t)n * 4 + 16))) { h->err = "hipMalloc failed (seeding tasks)"; return BWAGPU_ENOMEM; }
	// k_dedup's list of the reads it leaves to the wave-per-read kernel: the seeding kernels' list of heavy reads, free again by then
	DedupPlan dd;
	if (int rc = dedup_plan(h, opt, cfg, h->max_len, n, long_batch, share_pct, dp_wave_count(h, n_threads), dd)) return rc;
	for (int attempt = 0; attempt < 12; ++attempt) {
		h->phase = 20 + attempt * 100;
		int rc = alloc_batch(h, n_threads, seed_tasks ? (int)(((size_t)task_lanes * TASK_STACK_CAP + (size_t)(h->max_len + PTAB_MAX)) / (size_t)(h->max_len + 1 + PTAB_MAX))   // (the tasks' small spill areas, in units of a full-size one)
											: heavy_lanes);      // (the heavy reads' task lanes use the spill area after the lane-per-read kernel)
		if (rc) return rc;
		HIPCHK(h, hipMemcpyAsync(h->d_minhsp.p, minhsp.data(), minhsp.size() * 4, hipMemcpyHostToDevice, h->stream));
		HIPCHK(h, hipMemsetAsync(h->d_ctr.p, 0, sizeof(Counters), h->stream));
		Batch B; memset(&B, 0, sizeof B);
		B.n_reads = n; B.max_len = h->max_len; B.stats = h->stats_on;
		B.seq = h->d_seq.as<u8>(); B.seq_nib = h->d_seq_nib.as<u64>(); B.off = h->d_off.as<i64>(); B.ctr = h->d_ctr.as<Counters>();
		B.tmp_intv = h->d_tmp_intv.as<BiIntv>(); B.mem_cap = h->mem_cap;
		B.rd_words = h->rd_words; B.seq_2b = h->d_seq_2b.as<u32>(); B.seq_flags = h->d_seq_flags.as<u8>();
		// LDS per lane: 160 bytes at four blocks per CU -- the read's 2-bit copy first, interval-stack entries with the rest
		const int lane_lds = SEED_LANE_LDS, ent_max = SEED_LDS_ENT;
		const int lds_ent_dflt = h->rd_words ? ((lane_lds - 4 * h->rd_words) / 16 < ent_max ? (lane_lds - 4 * h->rd_words) / 16 : ent_max) : ent_max;
		B.seed_lds_ent = (h->seq_len < ((u64)1 << 37) && h->max_len < 65536) ? (cfg.seed_lds_ent >= 0 ? (int)cfg.seed_lds_ent : lds_ent_dflt) : 0;
		h->seed_lds_run = B.seed_lds_ent;
		if (((size_t)(B.seed_lds_ent ? B.seed_lds_ent : 1) * 16 + (size_t)B.rd_words * 4) * BLOCK > 65536) B.rd_words = 0;   // (an LDS_ENT override too large for both)
		B.intv_n = h->d_intv_n.as<i32>(); B.intv_off = h->d_intv_off.as<i64>(); B.intv = h->d_intv.as<Intv3>();
		B.seed_n = h->d_seed_n.as<i32>(); B.seed_off = h->d_seed_off.as<i64>(); B.slot_cap = h->slot_cap;
		B.slot_pos = h->d_slot_pos.as<u64>(); B.slot_qbeg = h->d_slot_qbeg.as<i32>(); B.slot_len = h->d_slot_len.as<i32>(); B.slot_rid = h->d_slot_rid.as<i32>(); B.slot_blob = h->d_slot_blob.as<u8>();
		B.chain_n = h->d_chain_n.as<i32>(); B.node_off = h->d_node_off.as<i64>(); B.nodes = h->d_nodes.as<i32>(); B.node_cap = h->node_cap;
		B.reg_off = h->d_reg_off.as<i64>(); B.reg_cap_r = h->d_reg_cap_r.as<i32>(); B.reg_n_raw = h->d_reg_n_raw.as<i32>(); B.reg_n = h->d_reg_n.as<i32>();
		B.regs = h->d_regs.as<bwagpu_alnreg_t>(); B.reg_cap = h->reg_cap;
		B.regs_raw = h->taps_on ? h->d_regs_raw.as<bwagpu_alnreg_t>() : nullptr;
		B.dp_h = h->d_dp_h.as<i32>(); B.dp_e = h->d_dp_e.as<i32>(); B.dp_waves = dp_wave_count(h, n_threads);
		B.seedsw_minhsp = h->d_minhsp.as<i32>();
		B.order = h->d_order.as<i32>(); B.bin_cnt = h->d_bin_cnt.as<u32>(); B.seed_w = h->d_seed_w.as<i32>(); B.seed_order = nullptr;
		B.seed_prio = cfg.seed_prio != 0;
		B.ext_blk = cfg.ext_blk != 0;
		B.seed_no_virt = cfg.seed_no_virt != 0;
		B.seed_jump = cfg.seed_jump < 0 ? 3 : (int)cfg.seed_jump;
		B.seed_pass3_inline = cfg.seed_pass3_inline != 0;
		B.task_step = opt->min_seed_len; B.n_vreads = n_vreads; B.vr_ovf_run = 0; B.vr_room = 0; B.seed_stack_cap = 0; B.intv_n3 = nullptr;
		if (seed_tasks) { B.vr_first = h->d_vr_tab.as<i32>(); B.vr_ovf = h->d_vr_ovf.as<i32>(); B.intv_n3 = h->d_intv_n3.as<i32>(); }
		B.task_tpr = 0; B.p2_tasks = nullptr; B.p2_cap = 0; B.heavy_list = nullptr; B.seed_budget = 0;
		if (heavy_tasks) {
			const i64 p2_cap = cfg.seed_p2_cap > 0 ? cfg.seed_p2_cap * (i64)h->p2_factor : (i64)((double)n * .5 * h->p2_factor) + 4096;      // (grown fourfold when a batch overflows it)
			B.heavy_list = h->d_heavy.as<i32>(); B.seed_budget = seed_budget;
			if (h->d_p2_tasks.ensure((size_t)p2_cap * 8)) { h->err = "hipMalloc failed (seeding tasks)"; return BWAGPU_ENOMEM; }
			B.intv_n3 = h->d_intv_n3.as<i32>(); B.p2_tasks = h->d_p2_tasks.as<i64>(); B.p2_cap = p2_cap;
		}
		// memory round trips per iteration of the seeding kernels (dev_seed.h, k_seed's MRG): 0 = as compiled, 2 = table entries, whole index
		// blocks and the next interval-stack entry in one trip (any other non-zero value selects 2 as well)
		int seed_mrg = (cfg.seed_mrg >= 0 ? cfg.seed_mrg : 2) ? 2 : 0;      // (auto: 2 for every batch since round 4 -- 2 % faster in step time for short reads as well, every time it was measured)
		if (!idx_in_desc) seed_mrg = 0;   // (its loads address 32-bit offsets into buffers of < 4 GiB: an index beyond that keeps the plain kernels, see idx_in_desc above)
		B.seq_nib_bytes = (((u64)h->n_bases + 15) / 16) * 8;
		dim3 grid(n_threads / BLOCK), block(BLOCK);
		HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
		if (dbg_sync) { hipError_t e_ = hipStreamSynchronize(h->stream); fprintf(stderr, "[bwagpu] attempt %d: %s done (%s)\n", attempt, "start", hipGetErrorString(e_)); }
		if (!B.seed_pass3_inline) {   // pass 3 first (cheap), then passes 1-2 on the reads ordered by the repetitiveness it measured
			if (h->ix.occ32 != nullptr && seed_mrg) hipLaunchKernelGGL((k_seed3<1, true>), grid, block, 0, h->stream, h->ix, *opt, B);
			else if (h->ix.occ32 != nullptr) hipLaunchKernelGGL(k_seed3<1>, grid, block, 0, h->stream, h->ix, *opt, B);
			else hipLaunchKernelGGL(k_seed3<0>, grid, block, 0, h->stream, h->ix, *opt, B);
			if (!cfg.seed_input_order) {
				i32 *keep = B.order; B.order = h->d_seed_order.as<i32>();
				if (int rc2 = order_reads(h, B, B.seed_w)) return rc2;
				B.seed_order = B.order; B.order = keep;
			}
		}
		const size_t seed_lds = ((size_t)(B.seed_lds_ent ? B.seed_lds_ent : 1) * sizeof(uint4) + (size_t)B.rd_words * 4) * BLOCK;
		dim3 sgrid = grid;                    // (option seed_grid, measurements: fewer resident workgroups of the seeding kernel; it stays within 5 % down to two per CU -- it is bound by memory requests, not by waves -- but step time with three batches in flight did not move either, nor did making the batches' seeding kernels take turns)
		if (cfg.seed_grid > 0 && (unsigned long long)cfg.seed_grid < grid.x) sgrid = dim3((unsigned)cfg.seed_grid);
		else if (!long_batch) sgrid = dim3((unsigned)share(grid.x));
		// (instances: with/without the LDS copy of the reads, the work counters -- which cost registers --, the two index layouts, one or several trips per iteration)
#define SEED_LAUNCH(RD_, ST_, B_, O_, M_) hipLaunchKernelGGL((k_seed<RD_, ST_, B_, O_, M_>), sgrid, block, seed_lds, h->stream, h->ix, *opt, B)
#define SEED_LAUNCH_B(RD_, ST_) do { if (blk == 1 && mrg == 2) SEED_LAUNCH(RD_, ST_, 1, (RD_ ? 4 : 3), 2);   /* (no LDS copy of the reads: long reads, few lanes -- registers instead of spills) */ \
		else if (blk == 1) SEED_LAUNCH(RD_, ST_, 1, 4, 0); else SEED_LAUNCH(RD_, ST_, 0, 4, 0); } while (0)
		{
			const bool rd = B.rd_words != 0, st = B.stats != 0;
			const int blk = h->ix.occ32 != nullptr ? 1 : 0;
			const int mrg = seed_mrg;
			if (seed_tasks && blk == 1 && !rd) {
				// long reads: pass 1 as independent tasks on small interval stacks; the few tasks whose stack filled up once more, on full-size
				// stacks (its work list is known on the device only: the launch is sized for the lane-per-read kernel and usually finds nothing);
				// then the lane-per-read kernel from pass 2 on
				Batch BA = B; BA.seed_order = nullptr; BA.seed_stack_cap = TASK_STACK_CAP; BA.vr_room = B.seed_lds_ent + 2 * (TASK_STACK_CAP - PTAB_MAX) - 2;
				Batch BO = B; BO.seed_order = nullptr; BO.vr_ovf_run = 1; BO.vr_room = 0x7fffffff;
				const dim3 agrid((unsigned)(task_lanes / BLOCK));
#define SEED_LAUNCH_LR(ST_, M_) do { hipLaunchKernelGGL((k_seed<false, ST_, 1, 3, M_, 1>), agrid, block, seed_lds, h->stream, h->ix, *opt, BA); \
					hipLaunchKernelGGL((k_seed<false, ST_, 1, 3, M_, 1>), sgrid, block, seed_lds, h->stream, h->ix, *opt, BO); \
					hipLaunchKernelGGL((k_seed<false, ST_, 1, 3, M_, 2>), sgrid, block, seed_lds, h->stream, h->ix, *opt, B); } while (0)
				if (mrg == 2) { if (st) SEED_LAUNCH_LR(true, 2); else SEED_LAUNCH_LR(false, 2); }
				else { if (st) SEED_LAUNCH_LR(true, 0); else SEED_LAUNCH_LR(false, 0); }
#undef SEED_LAUNCH_LR
			}
			else {
				if (rd) { if (st) SEED_LAUNCH_B(true, true); else SEED_LAUNCH_B(true, false); }
				else { if (st) SEED_LAUNCH_B(false, true); else SEED_LAUNCH_B(false, false); }
				if (heavy_tasks && blk == 1) {
					// the reads the kernel above gave up: pass-1 tasks, the list of their pass-2 searches, those searches (all sized on the device)
					Batch BT = B; BT.rd_words = 0; BT.seed_order = nullptr; BT.task_tpr = heavy_tpr; BT.vr_room = 0x7fffffff; BT.seed_stack_cap = 0; BT.seed_budget = 0;
					const size_t lds_t = (size_t)(B.seed_lds_ent ? B.seed_lds_ent : 1) * sizeof(uint4) * BLOCK;
					const dim3 hgrid((unsigned)(heavy_lanes / BLOCK));
					if (st) hipLaunchKernelGGL((k_seed<false, true, 1, 3, 2, 1>), hgrid, block, lds_t, h->stream, h->ix, *opt, BT);
					else hipLaunchKernelGGL((k_seed<false, false, 1, 3, 2, 1>), hgrid, block, lds_t, h->stream, h->ix, *opt, BT);
					hipLaunchKernelGGL(k_seed_p2_tasks, dim3((unsigned)(n < 256 * 64 ? (n + BLOCK - 1) / BLOCK : 64)), block, 0, h->stream, *opt, BT);
					if (st) hipLaunchKernelGGL((k_seed<false, true, 1, 3, 2, 3>), hgrid, block, lds_t, h->stream, h->ix, *opt, BT);
					else hipLaunchKernelGGL((k_seed<false, false, 1, 3, 2, 3>), hgrid, block, lds_t, h->stream, h->ix, *opt, BT);
				}
			}
		}
#undef SEED_LAUNCH_B
#undef SEED_LAUNCH
		HIPCHK(h, hipEventRecord(h->ev[7], h->stream));
		if (dbg_sync) { hipError_t e_ = hipStreamSynchronize(h->stream); fprintf(stderr, "[bwagpu] attempt %d: %s done (%s)\n", attempt, "k_seed3+k_seed", hipGetErrorString(e_)); }
		if (long_batch && pick(cfg.publish_blk, 1))    // long reads: one workgroup per read sorts, counts and expands (167 -> 47 ms per 6000 x 10 kb reads, BENCH_r03 variants)
		{
			size_t pb = h->d_tmp_intv.cap / ((size_t)PUB_MAX * sizeof(Intv3));      // workgroups the spill area has scratch for (PUB_MAX records each)
			if (pb > 2048) pb = 2048; if (pb > (size_t)n) pb = (size_t)n; if (pb < 1) pb = 1;
			hipLaunchKernelGGL(k_publish_blk, dim3((unsigned)pb), block, 0, h->stream, *opt, B);
		}
		else {
			hipLaunchKernelGGL(k_publish, grid, block, 0, h->stream, *opt, B);      // (sorts, reserves and expands: k_expand's loop is its last step)
		}
		HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
		if (dbg_sync) { hipError_t e_ = hipStreamSynchronize(h->stream); fprintf(stderr, "[bwagpu] attempt %d: %s done (%s)\n", attempt, "publish+expand", hipGetErrorString(e_)); }
		i64 sa_blocks = (h->slot_cap + BLOCK - 1) / BLOCK;
		if (sa_blocks > MAX_RESIDENT_THREADS / BLOCK) sa_blocks = MAX_RESIDENT_THREADS / BLOCK;
		hipLaunchKernelGGL(k_sa, dim3((unsigned)sa_blocks), block, 0, h->stream, h->ix, B);
		HIPCHK(h, hipEventRecord(h->ev[2], h->stream));
		if (dbg_sync) { hipError_t e_ = hipStreamSynchronize(h->stream); fprintf(stderr, "[bwagpu] attempt %d: %s done (%s)\n", attempt, "k_sa", hipGetErrorString(e_)); }
		B.chain_regs = (int)cfg.chain_regs; B.chain_flt_lds = (int)(cfg.chain_flt_lds < CW_FLT_LDS ? cfg.chain_flt_lds : CW_FLT_LDS);
		{	// wave per read, heaviest reads (most seeds) first
			if (int rc2 = order_reads(h, B, B.seed_n)) return rc2;
			i64 nblk = ((i64)n + 3) / 4, cap = share(256 * 5);   // (5 workgroups per CU: __launch_bounds__ of k_chain_wave)
			hipLaunchKernelGGL(k_chain_wave, dim3((unsigned)(nblk < cap ? nblk : cap)), block, (size_t)CW_LDS_BYTES * 4, h->stream, h->ix, *opt, B);
		}
		HIPCHK(h, hipEventRecord(h->ev[3], h->stream));
		if (dbg_sync) { hipError_t e_ = hipStreamSynchronize(h->stream); fprintf(stderr, "[bwagpu] attempt %d: %s done (%s)\n", attempt, "k_chain", hipGetErrorString(e_)); }
		if (any_seedsw && h->max_len > WAVE_EXT_MAX_LEN) {   // long reads: one wavefront per read, one lane per seed
			int sc_max = 0; for (int k = 0; k < 25; ++k) if (opt->mat[k] > sc_max) sc_max = opt->mat[k];
			const i64 wcap = B.dp_waves > 0 ? B.dp_waves : 1;
			if (pick(cfg.seedsw_lds, 1) && SEEDSW_LDS_COLS * sc_max < 65536) {
				// the cell loop's state in LDS (dev_local_score_lds), one wave per workgroup (165 -> 26 ms per 6000 x 10 kb reads, BENCH_r03 variants)
				if (SEEDSW_LDS_COLS * sc_max < 256) hipLaunchKernelGGL((k_seedsw_wave<8>), dim3((unsigned)(n < wcap ? n : wcap)), dim3(64), (size_t)SEEDSW_LDS_COLS * 64 * 3, h->stream, h->ix, *opt, B);
				else hipLaunchKernelGGL((k_seedsw_wave<16>), dim3((unsigned)(n < wcap ? n : wcap)), dim3(64), (size_t)SEEDSW_LDS_COLS * 64 * 5, h->stream, h->ix, *opt, B);
			} else {
				i64 nblk = ((i64)n + 3) / 4, cap = wcap / 4 > 0 ? wcap / 4 : 1;      // (one DP scratch region per wave)
				hipLaunchKernelGGL((k_seedsw_wave<0>), dim3((unsigned)(nblk < cap ? nblk : cap)), block, 0, h->stream, h->ix, *opt, B);
			}
		} else if (any_seedsw) hipLaunchKernelGGL(k_seedsw, grid, block, 0, h->stream, h->ix, *opt, B);
		HIPCHK(h, hipEventRecord(h->ev[4], h->stream));
		if (dbg_sync) { hipError_t e_ = hipStreamSynchronize(h->stream); fprintf(stderr, "[bwagpu] attempt %d: %s done (%s)\n", attempt, "k_seedsw", hipGetErrorString(e_)); }
		if (int rc2 = order_reads(h, B, B.reg_cap_r)) return rc2;   // heaviest reads (most seeds in kept chains) first
		// wave-per-read extension with the DP columns in LDS; its row-max scan packs (score << 6 | lane) into 31 bits
		i64 max_score = (i64)h->max_len * (opt->a > 0 ? opt->a : 1) * 2 + 1024;
		int ring_cols = 256;                     // long reads: ring of {H,E} columns wide enough for the widest band (2 * opt.w, bwamem.c:742)
		while (ring_cols < 4 * opt->w + 4 + 128) ring_cols <<= 1;
		if (h->max_len <= WAVE_EXT_MAX_LEN && max_score < (1 << 24)) {
			int lds_wave = (8 * (h->max_len + 2 + 64) + 5 * ((h->max_len + 64 + 3) & ~3) + 64 + 15) & ~15;   // {H,E} columns, query profile, scoring matrix, the stats runs' counters
			i64 nblk = ((i64)n + 3) / 4, cap = share(256 * 6);       // (six workgroups per CU are resident at 6 waves per SIMD)
			const int occ = (int)cfg.ext_occ;   // waves per SIMD the register allocation aims at (measured at 3.1 Gbp in round 2: 4 -> 63 ms, 5 -> 58 ms, 6 -> 56 ms; round 4, with the window rows: 4 -> 37.9, 5 -> 37.0-38.3, 6 -> 35.4-36.1 ms; the instance for 5 is not built -- one state of the source made hipcc 7.2 fail on it with an unaligned 64-bit spill reload, and it never won)
			const dim3 g((unsigned)(nblk < cap ? nblk : cap));
			// the chains' first extensions -- most of the stage's DP cells -- four to a wavefront, ahead of the kernel that replays mem_chain2aln's order-dependent
			// logic over them (dev_extp.h).  Not in stats runs: the work counters stay the one-wave routine's.
			if (cfg.ext_pack && !h->stats_on && h->max_len < 65536 && opt->w > 0 && (i64)h->max_len * sc_max_all(opt) < (1 << 21)) {
				B.ext_plan = 1;
				const i64 pcap = share(256 * 5);
				if (cfg.ext_pack == 5) hipLaunchKernelGGL((k_ext_pack<5>), dim3((unsigned)(nblk < pcap ? nblk : pcap)), block, (size_t)XP_LDS_BYTES * 4, h->stream, h->ix, *opt, B);
				else hipLaunchKernelGGL((k_ext_pack<4>), dim3((unsigned)(nblk < share(256 * 4) ? nblk : share(256 * 4))), block, (size_t)XP_LDS_BYTES * 4, h->stream, h->ix, *opt, B);
			}
			if (occ == 4) hipLaunchKernelGGL((k_extend_wave<false, 4>), g, block, (size_t)lds_wave * 4, h->stream, h->ix, *opt, B, lds_wave, 0);
			else hipLaunchKernelGGL((k_extend_wave<false, 6>), g, block, (size_t)lds_wave * 4, h->stream, h->ix, *opt, B, lds_wave, 0);
		} else if (max_score < (1 << 24) && ring_cols <= EXT_RING_MAX) {
			// the band's columns only: independent of the read length
			const int lds_wave = 8 * ring_cols + 64;      // (the ring, the scoring matrix, the stats runs' counters)
			int wpb = 4; while (wpb > 1 && lds_wave * wpb > 65536) wpb >>= 1;
			i64 nblk = ((i64)n + wpb - 1) / wpb, cap = 256 * 8 * (4 / wpb);
			hipLaunchKernelGGL((k_extend_wave<true, 4>), dim3((unsigned)(nblk < cap ? nblk : cap)), dim3(64 * wpb), (size_t)lds_wave * wpb, h->stream, h->ix, *opt, B, lds_wave, ring_cols);
		} else                                  // very wide bands: lane-per-read scalar DP with the columns in HBM scratch
			hipLaunchKernelGGL(k_extend, grid, block, 0, h->stream, h->ix, *opt, B);
		HIPCHK(h, hipEventRecord(h->ev[5], h->stream));
		if (dbg_sync) { hipError_t e_ = hipStreamSynchronize(h->stream); fprintf(stderr, "[bwagpu] attempt %d: %s done (%s)\n", attempt, "k_extend", hipGetErrorString(e_)); }
		dedup_launch(h, opt, cfg, B, h->max_len, n, long_batch, share_pct, grid.x, dd);
		HIPCHK(h, hipEventRecord(h->ev[6], h->stream));
		if (dbg_sync) { hipError_t e_ = hipStreamSynchronize(h->stream); fprintf(stderr, "[bwagpu] attempt %d: %s done (%s)\n", attempt, "k_dedup", hipGetErrorString(e_)); }
		HIPCHK(h, hipGetLastError());
		h->phase = 22 + attempt * 100;
		Counters c;
		HIPCHK(h, hipMemcpyAsync(&c, h->d_ctr.p, sizeof c, hipMemcpyDeviceToHost, h->stream));
		HIPCHK(h, wait_stream(h));
		if (c.overflow) {   // grow what overflowed and redo the batch; nothing of the failed attempt is kept
			// the bump counters kept counting past the arenas' ends: grow to what was asked for (+10 %) in one step rather than by doubling
			if (c.overflow & 2) { const i64 want = (i64)(c.seed_used + c.seed_used / 10) + 4096; h->slot_cap = want > h->slot_cap * 5 / 4 ? want : h->slot_cap * 2; }
			if (c.overflow & 6) {
				i64 want = h->slot_cap / 4 + 2 * (i64)n + 64; const i64 asked = (i64)(c.node_used + c.node_used / 10) + 64;
				if (asked > want) want = asked;
				h->node_cap = want > h->node_cap * 5 / 4 ? want : h->node_cap * 2;
			}
			if (c.overflow & 8) { const i64 want = (i64)(c.reg_used + c.reg_used / 10) + 4096; h->reg_cap = (c.overflow & 2) || want <= h->reg_cap * 5 / 4 ? h->reg_cap * 2 : want; }
			if (c.overflow & 16) h->mem_cap = h->mem_cap * 4;
			if (c.overflow & 32) h->p2_factor *= 4.;
			++h->stats.n_retries; h->stats.retry_mask |= (int32_t)c.overflow;
			continue;
		}
		{	// remember the sizes that sufficed, per base
			const double nbd = (double)(h->n_bases > 1024 ? h->n_bases : 1024);
			if (h->slot_cap / nbd > h->need_slot) h->need_slot = h->slot_cap / nbd;
			if (h->node_cap / nbd > h->need_node) h->need_node = h->node_cap / nbd;
			if (h->reg_cap / nbd > h->need_reg) h->need_reg = h->reg_cap / nbd;
			std::lock_guard<std::mutex> l(h->ibuf->m);
			// The interval lists' capacity is a stride (read r's list sits at r * mem_cap), so a longer one costs every read of every later batch: four times the
			// arena, and k_publish / k_chain_wave walking lists 24 KB apart (measured after one retry in a 20 M-read run: k_publish 2.5 -> 20 ms in the batches that
			// followed, 16 GB per handle).  One read in ~20 million of the bench's genome leaves more than 256 intervals; redoing that one batch is the cheaper
			// answer, so the longer lists are only kept once overflows recur (two or more, and more often than one batch in sixteen).
			++h->ibuf->batches;
			if (h->stats.retry_mask & 16) ++h->ibuf->mem_events;
			const bool keep_mem = h->ibuf->mem_events >= 2 && h->ibuf->mem_events * 16 > h->ibuf->batches;
			if (h->mem_cap > h->need_mem && cfg.mem_cap <= 0 && (keep_mem || !(h->stats.retry_mask & 16))) h->need_mem = h->mem_cap;
			if (h->need_slot > h->ibuf->need_slot) h->ibuf->need_slot = h->need_slot;
			if (h->need_node > h->ibuf->need_node) h->ibuf->need_node = h->need_node;
			if (h->need_reg > h->ibuf->need_reg) h->ibuf->need_reg = h->need_reg;
			if (h->need_mem > h->ibuf->need_mem) h->ibuf->need_mem = h->need_mem;
		}
		float ms[6];
		for (int i = 0; i < 6; ++i) HIPCHK(h, hipEventElapsedTime(&ms[i], h->ev[i], h->ev[i + 1]));
		HIPCHK(h, hipEventElapsedTime(&h->stats.ms_publish, h->ev[7], h->ev[1]));
		ms[0] -= h->stats.ms_publish;
		h->stats.ms_seed = ms[0]; h->stats.ms_sa = ms[1]; h->stats.ms_chain = ms[2]; h->stats.ms_seedsw = ms[3]; h->stats.ms_extend = ms[4]; h->stats.ms_dedup = ms[5];
		HIPCHK(h, hipEventElapsedTime(&h->stats.ms_total, h->ev[0], h->ev[6]));
		h->stats.n_seeds = (i64)c.seed_used;
		h->stats.n_intv = (i64)c.n_intv;
		h->stats.n_chains = (i64)c.n_chains; h->stats.n_regs_raw = (i64)c.n_regs_raw; h->stats.n_regs = (i64)c.n_regs;
		h->stats.n_tab_lookups = (i64)c.tab_lookups; h->stats.n_bt_nodes = (i64)c.bt_nodes; h->stats.n_chain_recs = (i64)c.chain_recs;
		h->stats.n_occ_blocks = (i64)c.occ_blocks; h->stats.n_lf_steps = (i64)c.lf_steps;
		h->stats.n_ext_calls = (i64)c.ext_calls; h->stats.n_ext_cells = (i64)c.ext_cells; h->stats.n_ext_fast = (i64)c.ext_fast;
		h->stats.n_glb_calls = (i64)c.glb_calls; h->stats.n_glb_cells = (i64)c.glb_cells; h->stats.ref_bases = (i64)c.ref_bases;
		h->stats.n_sw_calls = (i64)c.sw_calls; h->stats.n_sw_cells = (i64)c.sw_cells;
		h->ran = true;
		return BWAGPU_OK;
	}
	h->err = "arena growth did not converge";
	return BWAGPU_ENOMEM;
}

// gather per-read variable-length device records into read order on the host
template <class T>
static int gather(bwagpu_t *h, const DevBuf &d_n, const DevBuf &d_off, const DevBuf &d_rec, i64 rec_cap, int32_t *counts, T **out, int64_t *n_out)
{
	int n = h->n_reads;
	std::vector<i32> cnt(n); std::vector<i64> off(n);
	if (n) {
		HIPCHK(h, hipMemcpy(cnt.data(), d_n.p, (size_t)n * 4, hipMemcpyDeviceToHost));
		HIPCHK(h, hipMemcpy(off.data(), d_off.p, (size_t)n * 8, hipMemcpyDeviceToHost));
	}
	i64 tot = 0, hi = 0;
	for (int i = 0; i < n; ++i) { tot += cnt[i]; if (cnt[i] && off[i] + cnt[i] > hi) hi = off[i] + cnt[i]; }
	if (hi > rec_cap) { h->err = "internal: record range beyond arena"; return BWAGPU_EHIP; }
	std::vector<T> all((size_t)hi);
	if (hi) HIPCHK(h, hipMemcpy(all.data(), d_rec.p, (size_t)hi * sizeof(T), hipMemcpyDeviceToHost));
	T *res = (T*)malloc((size_t)(tot ? tot : 1) * sizeof(T));
	if (!res) return BWAGPU_ENOMEM;
	i64 k = 0;
	for (int i = 0; i < n; ++i) {
		if (counts) counts[i] = cnt[i];
		if (cnt[i]) memcpy(res + k, all.data() + off[i], (size_t)cnt[i] * sizeof(T));
		k += cnt[i];
	}
	*out = res; *n_out = tot;
	return BWAGPU_OK;
}

// The region arena is sparse (every read owns a range sized for its worst case); pack the used records on the device so
// that only they cross PCIe.  One lane per read, 88-byte records copied as 11 x u64.
__global__ void __launch_bounds__(256) k_pack_regs(int n, const i32 *reg_n, const i64 *reg_off, const bwagpu_alnreg_t *regs, const i64 *dst_off, bwagpu_alnreg_t *dst, i32 *dst_read)
{
	static_assert(sizeof(bwagpu_alnreg_t) == 88, "layout");
	for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
		const int c = reg_n[r];
		const u64 *src = (const u64*)(regs + reg_off[r]); u64 *d = (u64*)(dst + dst_off[r]);
		for (int k = 0; k < c * 11; ++k) d[k] = src[k];
		for (int k = 0; k < c; ++k) dst_read[dst_off[r] + k] = r;
	}
}

extern "C" int bwagpu_batch_download(bwagpu_t *h, int32_t *counts, bwagpu_alnreg_t **regs_out, int64_t *n_regs_out)
{
	if (!h || !h->ran || !regs_out || !n_regs_out) return BWAGPU_EINVAL;
	HIPCHK(h, hipSetDevice(h->device));
	const int n = h->n_reads;
	h->cig_ext_n = -1;
	if (n == 0) { *regs_out = (bwagpu_alnreg_t*)malloc(sizeof(bwagpu_alnreg_t)); *n_regs_out = 0; h->downloaded = true; h->packed_max = 0; return BWAGPU_OK; }
	h->phase = 30;
	std::vector<i32> cnt((size_t)n); std::vector<i64> dst((size_t)n);
	HIPCHK(h, hipMemcpyAsync(cnt.data(), h->d_reg_n.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(h, wait_stream(h));
	i64 tot = 0; int cnt_max = 0;
	for (int i = 0; i < n; ++i) { dst[i] = tot; tot += cnt[i]; if (cnt[i] > cnt_max) cnt_max = cnt[i]; if (counts) counts[i] = cnt[i]; }
	release_reserved(h);      // (the blocks bwagpu_batch_reserve page-locked for this handle go back to the pool, where the next lines find them)
	bwagpu_alnreg_t *res = (bwagpu_alnreg_t*)result_alloc((size_t)(tot ? tot : 1) * sizeof(bwagpu_alnreg_t));
	if (!res) return BWAGPU_ENOMEM;
	h->phase = 31;
	if (tot) {
		if (h->d_pack_off.ensure((size_t)n * 8) || h->d_regs_packed.ensure((size_t)tot * sizeof(bwagpu_alnreg_t)) || h->d_pack_read.ensure((size_t)tot * 4)) { bwagpu_free(res); h->err = "hipMalloc failed (packed regions)"; return BWAGPU_ENOMEM; }
		h->phase = 32;
		(void)hipEventRecord(h->ev[0], h->stream);
		hipError_t e = hipMemcpyAsync(h->d_pack_off.p, dst.data(), (size_t)n * 8, hipMemcpyHostToDevice, h->stream);
		if (e == hipSuccess) {
			int nb = (n + BLOCK - 1) / BLOCK; if (nb > 8192) nb = 8192;
			hipLaunchKernelGGL(k_pack_regs, dim3(nb), dim3(BLOCK), 0, h->stream, n, h->d_reg_n.as<i32>(), h->d_reg_off.as<i64>(), h->d_regs.as<bwagpu_alnreg_t>(),
							   h->d_pack_off.as<i64>(), h->d_regs_packed.as<bwagpu_alnreg_t>(), h->d_pack_read.as<i32>());
			e = hipGetLastError();
		}
		(void)hipEventRecord(h->ev[1], h->stream);
		if (e == hipSuccess) e = hipMemcpyAsync(res, h->d_regs_packed.p, (size_t)tot * sizeof(bwagpu_alnreg_t), hipMemcpyDeviceToHost, h->stream);
		(void)hipEventRecord(h->ev[2], h->stream);
		if (e == hipSuccess) e = wait_stream(h);
		if (e != hipSuccess) { bwagpu_free(res); HIPCHK(h, e); }
		(void)hipEventElapsedTime(&h->stats.ms_pack, h->ev[0], h->ev[1]); (void)hipEventElapsedTime(&h->stats.ms_download_copy, h->ev[1], h->ev[2]);
	}
	h->packed_tot = tot; h->packed_max = cnt_max; h->downloaded = true; h->phase = 39;
	*regs_out = res; *n_regs_out = tot;
	return BWAGPU_OK;
}

// What the CIGAR kernels read and where they leave their records: tot regions `regs`, region g of read reg_read[g], the reads' lists starting at off[] (the filter's
// "best region of the read"); the reads' bases seq / seq_off; the records go to *d_cigs and the operation array to *d_ext (grown here).
struct CigLists {
	i64 tot; const bwagpu_alnreg_t *regs; const i32 *reg_read; const i64 *off;
	const u8 *seq; const i64 *seq_off; int n_reads, max_len; i64 n_bases;
	DevBuf *d_cigs, *d_ext;
};
// The kernels of bwagpu_batch_cigars on the regions C describes (tot > 0): the LDS tiers, the long tier, a second attempt when the operation array was too small.
// res (may be null): the records' host copy; *ext_n: entries of the operation array in use; ms[0] / ms[1]: device time of the kernels and of the copy.
static int cigars_run(bwagpu_t *h, const bwagpu_opt_t *opt, const CigLists &C, bwagpu_cigar_t *res, i64 *ext_n, float ms[2])
{
	const i64 tot = C.tot;
	static_assert(sizeof(bwagpu_cigar_t) == 48, "layout");
	{
		if (C.d_cigs->ensure((size_t)tot * sizeof(bwagpu_cigar_t)) || h->d_ctr.ensure(sizeof(Counters))) { h->err = "hipMalloc failed (cigars)"; return BWAGPU_ENOMEM; }
		Batch B = {}; B.seq = const_cast<u8*>(C.seq); B.off = const_cast<i64*>(C.seq_off); B.n_reads = C.n_reads; B.max_len = C.max_len;
		B.ctr = h->d_ctr.as<Counters>(); B.stats = h->stats_on;      // (stats: the fills' DP cells, counted in glb_cells / glb_calls -- the batch's run is over, its counters have been read)
		unsigned long long *next = &h->d_ctr.as<Counters>()->next_ext, *ext_used = &h->d_ctr.as<Counters>()->cig_ext_used;
		const int zc[2] = { CIG_Z_SMALL, CIG_Z_BIG };
		const int n_tier = (int)h->cfg.cig_tiers;   // diagnostics
		// operation array: sized for a typical batch; one that needs more (gap-rich reads) reports the total it reserved and is
		// redone once with exactly that much
		i64 ext_cap = tot * 4 + 65536;
		if (C.max_len > CIG_MAX_LEN && C.n_bases / 2 + 65536 > ext_cap) ext_cap = C.n_bases / 2 + 65536;   // (long reads: ~0.37 entries per base at 13 % indels -- operations and MD characters)
		if (h->cfg.cig_ops_cap > 0) ext_cap = h->cfg.cig_ops_cap;   // (tests of the second attempt)
		if (ext_cap < 1) ext_cap = 1;
		// third tier (k_cigar_long): segments, bands and operation counts beyond the LDS tiers' limits; one 64-thread workgroup per region at a time,
		// each with a direction matrix of its own in HBM.  A sizing pass (k_cigar_long_plan) counts the regions the LDS tiers left and the largest
		// matrix any of them can ask for; the scratch is as many such matrices as there are regions, at most 1024 and at most option cigl_mib (32 GiB).
		const bool long_tier = h->cfg.cig_long != 0;
		const i64 cigl_budget = (i64)h->cfg.cigl_mib << 20;
		const bool cig_trace = h->cfg.cig_trace != 0;
		auto t_last = std::chrono::steady_clock::now();
		auto lap = [&](const char *what) {
			if (!cig_trace) return;
			(void)wait_stream(h);
			auto t = std::chrono::steady_clock::now();
			fprintf(stderr, "[bwagpu] cigars: %s %.1f ms\n", what, std::chrono::duration<double, std::milli>(t - t_last).count());
			t_last = t;
		};
		unsigned long long used = 0;
		hipError_t e = hipSuccess;
		(void)hipEventRecord(h->ev[0], h->stream);
		for (int attempt = 0; attempt < 2; ++attempt) {
			if (C.d_ext->ensure((size_t)ext_cap * 4)) { h->err = "hipMalloc failed (cigars)"; return BWAGPU_ENOMEM; }
			e = hipMemsetAsync(ext_used, 0, sizeof(unsigned long long), h->stream);
			if (e == hipSuccess && h->stats_on) e = hipMemsetAsync(&h->d_ctr.as<Counters>()->glb_calls, 0, 2 * sizeof(unsigned long long), h->stream);      // (glb_calls, glb_cells: adjacent)
			for (int tier = 0; tier < n_tier && e == hipSuccess; ++tier) {   // narrow bands at high occupancy, then the deferred wide ones
				e = hipMemsetAsync(next, 0, sizeof(unsigned long long), h->stream);
				if (e != hipSuccess) break;
				h->phase = 41 + tier;
				// tier 0: the diag form only (bands of up to 64 columns whose direction nibbles fit CIG_Z_SMALL; no {H,E} columns in LDS: 6.3 KB per wave);
				// tier 1: both forms with CIG_Z_BIG nibbles, for what tier 0 deferred
				const int lds_wave = tier == 0 ? CIG_LDS_BYTES_DIAG(zc[tier]) : CIG_LDS_BYTES(zc[tier]);
				const int wpb = tier == 0 ? 4 : 2;                 // waves per workgroup: the wide tier stays below 64 KiB of LDS per group
				i64 nblk = (tot + wpb - 1) / wpb, cap = 256 * 6;
				if (tier == 0) hipLaunchKernelGGL(k_cigar<true>, dim3((unsigned)(nblk < cap ? nblk : cap)), dim3(64 * wpb), (size_t)lds_wave * wpb, h->stream, h->ix, *opt, B, tot,
								   C.regs, C.reg_read, C.d_cigs->as<bwagpu_cigar_t>(), next, zc[tier], tier,
								   C.d_ext->as<u32>(), ext_used, ext_cap, h->cigar_filter ? C.off : (const i64*)nullptr);
				else hipLaunchKernelGGL(k_cigar<false>, dim3((unsigned)(nblk < cap ? nblk : cap)), dim3(64 * wpb), (size_t)lds_wave * wpb, h->stream, h->ix, *opt, B, tot,
								   C.regs, C.reg_read, C.d_cigs->as<bwagpu_cigar_t>(), next, zc[tier], tier,
								   C.d_ext->as<u32>(), ext_used, ext_cap, h->cigar_filter ? C.off : (const i64*)nullptr);
				e = hipGetLastError();
			}
			lap("LDS tiers");
			if (e == hipSuccess && long_tier) {
				unsigned long long *plan_d = h->d_ctr.as<Counters>()->cigl_plan, plan[2] = { 0, 0 };
				if (h->d_cigl_list.ensure((size_t)tot * 4)) { h->err = "hipMalloc failed (cigars)"; return BWAGPU_ENOMEM; }
				e = hipMemsetAsync(plan_d, 0, sizeof plan, h->stream);
				if (e == hipSuccess) {
					h->phase = 43;
					i64 nb = (tot + 255) / 256; if (nb > 2048) nb = 2048;
					hipLaunchKernelGGL(k_cigar_long_plan, dim3((unsigned)nb), dim3(256), 0, h->stream, h->ix, *opt, tot, C.regs, C.d_cigs->as<bwagpu_cigar_t>(), plan_d, h->d_cigl_list.as<i32>());
					e = hipGetLastError();
				}
				if (e == hipSuccess) e = hipMemcpyAsync(plan, plan_d, sizeof plan, hipMemcpyDeviceToHost, h->stream);
				if (e == hipSuccess) e = wait_stream(h);
				if (e == hipSuccess && plan[0] > 0 && plan[1] > 0) {
					// matrices a quarter larger than this batch's largest and a multiple of 1 MiB, so that the next batches rarely re-allocate
					i64 z_cap = (i64)plan[1] + (i64)plan[1] / 4; z_cap = (z_cap + ((i64)1 << 20) - 1) & ~(((i64)1 << 20) - 1);
					if (h->cigl_z_cap > z_cap) z_cap = h->cigl_z_cap;
					i64 n_long = cigl_budget / z_cap; if (n_long > 1024) n_long = 1024; if (n_long > (i64)plan[0]) n_long = (i64)plan[0]; if (n_long < 1) n_long = 1;
					if (h->d_cigl_z.ensure((size_t)z_cap * n_long) || h->d_cigl_ops.ensure((size_t)n_long * CIGL_MAX_OPS * 4) || h->d_cigl_md.ensure((size_t)n_long * CIGL_MD_CAP)) {
						h->err = "hipMalloc failed (cigars)"; return BWAGPU_ENOMEM; }
					h->cigl_z_cap = z_cap;
					if (cig_trace) fprintf(stderr, "[bwagpu] cigars: long tier: %llu regions, largest matrix %.1f MB, %lld workgroups x %.1f MB\n", plan[0], plan[1] / 1e6, (long long)n_long, z_cap / 1e6);
					lap("long tier plan + scratch");
					e = hipMemsetAsync(next, 0, sizeof(unsigned long long), h->stream);
					if (e == hipSuccess) {
						h->phase = 44;
						hipLaunchKernelGGL(k_cigar_long, dim3((unsigned)n_long), dim3(64), (size_t)CIGL_LDS_BYTES, h->stream, h->ix, *opt, B, (i64)plan[0], h->d_cigl_list.as<i32>(),
										   C.regs, C.reg_read, C.d_cigs->as<bwagpu_cigar_t>(), next,
										   h->d_cigl_z.as<u8>(), z_cap, h->d_cigl_ops.as<u32>(), h->d_cigl_md.as<u8>(), C.d_ext->as<u32>(), ext_used, ext_cap);
						e = hipGetLastError();
					}
					lap("k_cigar_long");
				}
			}
			if (e == hipSuccess) e = hipMemcpyAsync(&used, ext_used, sizeof used, hipMemcpyDeviceToHost, h->stream);
			if (e == hipSuccess) e = wait_stream(h);
			if (e != hipSuccess || (i64)used <= ext_cap) break;
			ext_cap = (i64)used;
		}
		h->phase = 45;
		(void)hipEventRecord(h->ev[1], h->stream);
		if (e == hipSuccess && h->stats_on) {
			unsigned long long cc[2] = { 0, 0 };
			e = hipMemcpyAsync(cc, &h->d_ctr.as<Counters>()->glb_calls, sizeof cc, hipMemcpyDeviceToHost, h->stream);
			if (e == hipSuccess) e = wait_stream(h);
			h->stats.n_cig_dp = (i64)cc[0]; h->stats.n_cig_cells = (i64)cc[1];
		}
		if (e == hipSuccess && res) e = hipMemcpyAsync(res, C.d_cigs->p, (size_t)tot * sizeof(bwagpu_cigar_t), hipMemcpyDeviceToHost, h->stream);
		(void)hipEventRecord(h->ev[2], h->stream);
		if (e == hipSuccess) e = wait_stream(h);
		HIPCHK(h, e);
		(void)hipEventElapsedTime(&ms[0], h->ev[0], h->ev[1]); (void)hipEventElapsedTime(&ms[1], h->ev[1], h->ev[2]);     // (kernels: includes the plan's small D2H and, after an overflow, the second attempt)
		*ext_n = (i64)used < ext_cap ? (i64)used : ext_cap;
	}
	return BWAGPU_OK;
}

extern "C" int bwagpu_batch_cigars(bwagpu_t *h, const bwagpu_opt_t *opt, bwagpu_cigar_t **out, int64_t *n_out)
{
	if (!h || !opt || !h->ran || h->packed_tot < 0 || !out || !n_out) return BWAGPU_EINVAL;
	const BusyGuard busy(h->ibuf->busy);
	if (opt->e_del <= 0 || opt->e_ins <= 0) return BWAGPU_EINVAL;
	HIPCHK(h, hipSetDevice(h->device));
	const i64 tot = h->packed_tot;
	h->phase = 40; h->cig_ext_n = -1;
	bwagpu_cigar_t *res = (bwagpu_cigar_t*)result_alloc((size_t)(tot ? tot : 1) * sizeof(bwagpu_cigar_t));
	if (!res) return BWAGPU_ENOMEM;
	if (tot) {
		const CigLists C = { tot, h->d_regs_packed.as<bwagpu_alnreg_t>(), h->d_pack_read.as<i32>(), h->d_pack_off.as<i64>(), h->d_seq.as<u8>(), h->d_off.as<i64>(), h->n_reads, h->max_len, h->n_bases,
							 &h->d_cigs, &h->d_cig_ext };
		i64 ext_n = -1; float ms[2] = { 0.f, 0.f };
		const int rc = cigars_run(h, opt, C, res, &ext_n, ms);
		if (rc != BWAGPU_OK) { bwagpu_free(res); return rc; }
		h->stats.ms_cigar_kernels = ms[0]; h->stats.ms_cigar_copy = ms[1];
		h->cig_ext_n = ext_n;
	}
	if (tot == 0) h->cig_ext_n = 0;
	*out = res; *n_out = tot;
	return BWAGPU_OK;
}

extern "C" int bwagpu_batch_cigar_ops(bwagpu_t *h, uint32_t **ops, int64_t *n_ops)
{
	if (!h || !ops || !n_ops || h->cig_ext_n < 0) return BWAGPU_EINVAL;
	HIPCHK(h, hipSetDevice(h->device));
	const i64 n = h->cig_ext_n;
	uint32_t *res = (uint32_t*)result_alloc((size_t)(n ? n : 1) * 4);
	if (!res) return BWAGPU_ENOMEM;
	if (n) {
		(void)hipEventRecord(h->ev[0], h->stream);
		hipError_t e = hipMemcpyAsync(res, h->d_cig_ext.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream);
		(void)hipEventRecord(h->ev[1], h->stream);
		if (e == hipSuccess) e = wait_stream(h);
		if (e != hipSuccess) { bwagpu_free(res); HIPCHK(h, e); }
		float ms = 0; (void)hipEventElapsedTime(&ms, h->ev[0], h->ev[1]); h->stats.ms_cigar_copy += ms;
	}
	*ops = res; *n_ops = n;
	return BWAGPU_OK;
}

// ---- what the post-alignment stages share (mate rescue, marking, pairing, insert sizes) ------------------------------------------------------------
// A result block until it goes to the caller (`*out = r.release()`, the last statement that can fail behind it): every other way out of a function hands it
// back through bwagpu_free, so HIPCHK and plain returns work while one is held.
struct ResultFree { void operator()(void *p) const { bwagpu_free(p); } };
template <class T> using ResultBlock = std::unique_ptr<T[], ResultFree>;
template <class T> static ResultBlock<T> result_block(size_t n) { return ResultBlock<T>((T*)result_alloc((n ? n : 1) * sizeof(T))); }

// The region lists of n reads, tot regions in all, the longest of max_cnt.  On the device: counts d_cnt, offsets d_off into d_regs, read i's id d_ids[i] or (null)
// id0 + i.  h_*: the same arrays on the host, each null where the host has none -- ListsMirror then brings it over for the records that come back flagged.
struct RegLists {
	int n = 0, max_cnt = 0; i64 tot = 0;
	const i32 *d_cnt = nullptr; const i64 *d_off = nullptr; const bwagpu_alnreg_t *d_regs = nullptr; const i64 *d_ids = nullptr; i64 id0 = 0;
	const i32 *h_cnt = nullptr; const i64 *h_off = nullptr; const bwagpu_alnreg_t *h_regs = nullptr; const i64 *h_ids = nullptr;
};
// the packed regions of the last download
static RegLists lists_of_batch(const bwagpu_t *h, i64 id0)
{
	RegLists L; L.n = h->n_reads; L.tot = h->packed_tot < 0 ? 0 : h->packed_tot; L.max_cnt = h->packed_max; L.id0 = id0;
	L.d_cnt = h->d_reg_n.as<i32>(); L.d_off = h->d_pack_off.as<i64>(); L.d_regs = h->d_regs_packed.as<bwagpu_alnreg_t>();
	return L;
}
// Counts, offsets and regions of L that are not on the host, fetched into vectors of this object (one wait); L.h_* then point at them.
struct ListsMirror {
	std::vector<i32> cnt; std::vector<i64> off; std::vector<bwagpu_alnreg_t> regs;
	hipError_t fetch(bwagpu_t *h, RegLists &L)
	{
		hipError_t e = hipSuccess;
		if (!L.h_cnt) { cnt.resize((size_t)L.n); e = hipMemcpyAsync(cnt.data(), L.d_cnt, (size_t)L.n * 4, hipMemcpyDeviceToHost, h->stream); L.h_cnt = cnt.data(); }
		if (e == hipSuccess && !L.h_off) { off.resize((size_t)L.n); e = hipMemcpyAsync(off.data(), L.d_off, (size_t)L.n * 8, hipMemcpyDeviceToHost, h->stream); L.h_off = off.data(); }
		if (e == hipSuccess && !L.h_regs) { regs.resize((size_t)(L.tot ? L.tot : 1)); if (L.tot) e = hipMemcpyAsync(regs.data(), L.d_regs, (size_t)L.tot * sizeof(bwagpu_alnreg_t), hipMemcpyDeviceToHost, h->stream); L.h_regs = regs.data(); }
		return e == hipSuccess ? wait_stream(h) : e;
	}
};
// The lists of a *_flat call: n counts and the regions back to back.  scan(): what all these calls require of them -- counts of 0 .. 2^30 - 1, regions where a
// count is positive and, where the call checks contigs (rid_n, or null), the first rid_n[i] <= counts[i] regions of list i on a contig of the index -- and the
// offsets, the total, the largest count; false: BWAGPU_EINVAL.  upload(): into the handle's d_pf_* buffers (with n_ids ids, or none), waits -- `off` is this
// object's --, and describes them in L with the caller's arrays as the host mirror.  `what` names the call in the error text.
struct FlatLists {
	std::vector<i64> off; size_t n = 0; i64 tot = 0; int max_cnt = 0;
	bool scan(const bwagpu_t *h, size_t n_, const i32 *counts, const bwagpu_alnreg_t *regs, const i32 *rid_n)
	{
		n = n_; off.assign(n + 1, 0);
		for (size_t i = 0; i < n; ++i) {
			if (counts[i] < 0 || counts[i] > 0x3fffffff || (counts[i] > 0 && !regs)) return false;
			for (int k = 0; rid_n && k < rid_n[i]; ++k) if (regs[tot + k].rid < 0 || regs[tot + k].rid >= h->n_seqs) return false;
			if (counts[i] > max_cnt) max_cnt = counts[i];
			off[i] = tot; tot += counts[i];
		}
		off[n] = tot;
		return true;
	}
	int upload(bwagpu_t *h, const char *what, const i32 *counts, const bwagpu_alnreg_t *regs, const i64 *ids, size_t n_ids, RegLists &L)
	{
		L = RegLists(); L.n = (int)n; L.tot = tot; L.max_cnt = max_cnt;
		if (n == 0) return BWAGPU_OK;
		if (h->d_pf_cnt.ensure(n * 4) || h->d_pf_off.ensure((n + 1) * 8) || (ids && h->d_pf_ids.ensure(n_ids * 8)) || h->d_pf_regs.ensure((size_t)(tot ? tot : 1) * sizeof(bwagpu_alnreg_t))) {
			h->err = std::string("hipMalloc failed (") + what + ")"; return BWAGPU_ENOMEM;
		}
		HIPCHK(h, hipMemcpyAsync(h->d_pf_cnt.p, counts, n * 4, hipMemcpyHostToDevice, h->stream));
		HIPCHK(h, hipMemcpyAsync(h->d_pf_off.p, off.data(), (n + 1) * 8, hipMemcpyHostToDevice, h->stream));
		if (ids) HIPCHK(h, hipMemcpyAsync(h->d_pf_ids.p, ids, n_ids * 8, hipMemcpyHostToDevice, h->stream));
		if (tot) HIPCHK(h, hipMemcpyAsync(h->d_pf_regs.p, regs, (size_t)tot * sizeof(bwagpu_alnreg_t), hipMemcpyHostToDevice, h->stream));
		HIPCHK(h, wait_stream(h));
		L.d_cnt = h->d_pf_cnt.as<i32>(); L.d_off = h->d_pf_off.as<i64>(); L.d_regs = h->d_pf_regs.as<bwagpu_alnreg_t>(); L.d_ids = ids ? h->d_pf_ids.as<i64>() : nullptr;
		L.h_cnt = counts; L.h_off = off.data(); L.h_regs = regs; L.h_ids = ids;
		return BWAGPU_OK;
	}
};
// The reads of a *_flat call: base codes back to back, read i at seqs[off[i] .. off[i + 1]).  scan(): what all these calls require of them -- offsets that are not
// negative and ascend, no read of more than 2^30 - 1 bases, sequences where there are bases -- and the first offset, the end of the last read, the longest read;
// false: BWAGPU_EINVAL.  codes_ok(): no base code above 4 in a read; false: BWAGPU_EINVAL.  upload(): seqs[0 .. n_bases) (padded as a batch's d_seq is) and the
// offsets into the handle's d_pf_seq / d_pf_seqoff, enqueued only -- ahead of FlatLists::upload, whose wait covers them, or of a wait of the caller's.  `what`
// names the entry point in the error text, `tag` in upload()'s as FlatLists::upload's does.
struct FlatReads {
	const u8 *seqs = nullptr; const i64 *off = nullptr; size_t n = 0; i64 first = 0, n_bases = 0; int max_len = 0;
	static bool bad_offsets(bwagpu_t *h, const char *what) { h->err = std::string(what) + ": offsets that do not ascend"; return false; }
	bool scan(bwagpu_t *h, const char *what, size_t n_, const u8 *seqs_, const i64 *off_)
	{
		n = n_; seqs = seqs_; off = off_;
		if (n == 0) return true;
		if (off[0] < 0) return bad_offsets(h, what);
		for (size_t i = 0; i < n; ++i) {
			if (off[i + 1] < off[i] || off[i + 1] - off[i] > 0x3fffffff) return bad_offsets(h, what);
			max_len = std::max(max_len, (int)(off[i + 1] - off[i]));
		}
		first = off[0]; n_bases = off[n];
		return n_bases == 0 || seqs;
	}
	bool codes_ok(bwagpu_t *h, const char *what) const
	{
		for (i64 k = first; k < n_bases; ++k) if (seqs[k] > 4) { h->err = std::string(what) + ": a base code above 4"; return false; }
		return true;
	}
	int upload(bwagpu_t *h, const char *tag) const
	{
		if (n == 0) return BWAGPU_OK;
		if (h->d_pf_seq.ensure((size_t)n_bases + 16) || h->d_pf_seqoff.ensure((n + 1) * 8)) { h->err = std::string("hipMalloc failed (") + tag + ")"; return BWAGPU_ENOMEM; }
		if (n_bases) HIPCHK(h, hipMemcpyAsync(h->d_pf_seq.p, seqs, (size_t)n_bases, hipMemcpyHostToDevice, h->stream));
		HIPCHK(h, hipMemcpyAsync(h->d_pf_seqoff.p, off, (n + 1) * 8, hipMemcpyHostToDevice, h->stream));
		return BWAGPU_OK;
	}
};
// ---- the CIGAR kernels on lists of the caller (test hook) ------------------------------------------------------------------------------------------------
extern "C" void bwagpu_cigar_limits(int32_t out[10])
{
	const int32_t v[10] = { CIG_MAX_LEN, CIG_Z_SMALL, CIG_Z_BIG, CIG_MAX_COLS, CIG_MAX_OPS, CIG_TMP_OPS, CIG_MD_CAP, CIGL_MAX_COLS, CIGL_MAX_OPS, CIGL_QCAP };
	memcpy(out, v, sizeof v);
}

extern "C" int bwagpu_cigars_flat(bwagpu_t *h, const bwagpu_opt_t *opt, int n_reads, const uint8_t *seqs, const int64_t *seq_off, const int32_t *counts, const bwagpu_alnreg_t *regs,
								  bwagpu_cigar_t **cigs, int64_t *n_cigs, uint32_t **ops, int64_t *n_ops)
{
	if (!h || !opt || n_reads < 0 || !cigs || !n_cigs || !ops || !n_ops || (n_reads > 0 && (!counts || !seq_off))) return BWAGPU_EINVAL;
	if (opt->e_del <= 0 || opt->e_ins <= 0) { h->err = "bwagpu_cigars_flat: e_del and e_ins must be positive"; return BWAGPU_EINVAL; }
	for (int i = 0; i < n_reads; ++i) if (counts[i] < 0) { h->err = "bwagpu_cigars_flat: a negative count"; return BWAGPU_EINVAL; }
	FlatLists F; RegLists L;
	if (!F.scan(h, (size_t)n_reads, counts, regs, nullptr)) { h->err = "bwagpu_cigars_flat: a count outside [0, 2^30), or counts without regions"; return BWAGPU_EINVAL; }
	if (F.tot > 0x7fffffff) { h->err = "bwagpu_cigars_flat: more than 2^31 - 1 regions"; return BWAGPU_EINVAL; }
	FlatReads R;
	if (!R.scan(h, "bwagpu_cigars_flat", (size_t)n_reads, seqs, seq_off) || (R.first != 0 && !R.bad_offsets(h, "bwagpu_cigars_flat"))) return BWAGPU_EINVAL;      // R.first: this call's reads begin at seqs[0] (the pair calls take any first offset)
	if (!R.codes_ok(h, "bwagpu_cigars_flat")) return BWAGPU_EINVAL;
	for (int i = 0; i < n_reads; ++i) {
		const i64 len = seq_off[i + 1] - seq_off[i];
		for (i64 k = F.off[(size_t)i]; k < F.off[(size_t)i + 1]; ++k) {
			const bwagpu_alnreg_t &a = regs[k];
			if (a.qb < 0 || a.qe > len) { h->err = "bwagpu_cigars_flat: region " + std::to_string(k) + ": qb < 0 or qe beyond the read"; return BWAGPU_EINVAL; }
			if (a.rb < 0 || a.re > 2 * h->l_pac) { h->err = "bwagpu_cigars_flat: region " + std::to_string(k) + ": rb < 0 or re beyond 2 l_pac"; return BWAGPU_EINVAL; }
		}
	}
	const BusyGuard busy(h->ibuf->busy);
	HIPCHK(h, hipSetDevice(h->device));
	*cigs = nullptr; *ops = nullptr; *n_cigs = 0; *n_ops = 0;
	ResultBlock<bwagpu_cigar_t> res = result_block<bwagpu_cigar_t>((size_t)F.tot);
	if (!res) return BWAGPU_ENOMEM;
	i64 ext_n = 0;
	DevBuf *D = h->d_cf;
	if (F.tot > 0) {
		if (int rc = R.upload(h, "cigars_flat")) return rc;
		if (int rc = F.upload(h, "cigars_flat", counts, regs, nullptr, 0, L)) return rc;
		if (D[bwagpu_s::CF_READ].ensure((size_t)F.tot * 4)) { h->err = "hipMalloc failed (cigars_flat)"; return BWAGPU_ENOMEM; }
		int nb = (n_reads + 3) / 4; if (nb > 8192) nb = 8192;
		hipLaunchKernelGGL(k_sampe_reg_read, dim3(nb), dim3(BLOCK), 0, h->stream, n_reads, L.d_cnt, L.d_off, D[bwagpu_s::CF_READ].as<i32>());
		HIPCHK(h, hipGetLastError());
		// (the filter's table is the lists' offsets: a read's first region is its best)
		const CigLists C = { F.tot, L.d_regs, D[bwagpu_s::CF_READ].as<i32>(), L.d_off, h->d_pf_seq.as<u8>(), h->d_pf_seqoff.as<i64>(), n_reads, R.max_len, R.n_bases,
							 &D[bwagpu_s::CF_CIGS], &D[bwagpu_s::CF_EXT] };
		float ms[2] = { 0.f, 0.f };
		const int rcc = cigars_run(h, opt, C, res.get(), &ext_n, ms);
		if (rcc != BWAGPU_OK) return rcc;
	}
	ResultBlock<uint32_t> res_ops = result_block<uint32_t>((size_t)ext_n);
	if (!res_ops) return BWAGPU_ENOMEM;
	if (ext_n) {
		HIPCHK(h, hipMemcpyAsync(res_ops.get(), D[bwagpu_s::CF_EXT].p, (size_t)ext_n * 4, hipMemcpyDeviceToHost, h->stream));
		HIPCHK(h, wait_stream(h));
	}
	*n_cigs = F.tot; *n_ops = ext_n;
	*cigs = res.release(); *ops = res_ops.release();
	return BWAGPU_OK;
}

// ---- the de-duplication stage on lists of the caller (test hook) ------------------------------------------------------------------------------------------
extern "C" void bwagpu_dedup_limits(int32_t out[8])
{
	const int32_t v[8] = { DEDUP_HEAVY_DEFAULT, DEDUP_STAGE_DEFAULT, DEDUP_NET_DEFAULT, DEDUP_KEYSORT_MIN, 64 /* regions dedup_read_par's scan takes at once: a wavefront */,
						   64 /* reads k_dedup draws at once */, DEDUP_RING_MIN, (int32_t)DDP_LDS_PER_REG };
	memcpy(out, v, sizeof v);
}

// bwagpu_batch_run's de-duplication stage -- dedup_plan and dedup_launch, as for a batch -- on the caller's reads and raw region lists, in buffers of its own: a
// batch on the handle keeps its results (the stage's list and staging buffers are scratch there as well).
extern "C" int bwagpu_dedup_flat(bwagpu_t *h, const bwagpu_opt_t *opt, int n_reads, const uint8_t *seqs, const int64_t *seq_off, const int32_t *counts, const bwagpu_alnreg_t *regs,
								 int32_t *counts_out, bwagpu_alnreg_t **regs_out, int64_t *n_out, int32_t *form)
{
	if (!h || !opt || n_reads < 0 || !regs_out || !n_out || (n_reads > 0 && (!counts || !seq_off || !counts_out))) return BWAGPU_EINVAL;
	if (opt->e_del <= 0 || opt->e_ins <= 0 || opt->w < 0) { h->err = "bwagpu_dedup_flat: e_del and e_ins must be positive, w not negative"; return BWAGPU_EINVAL; }
	for (int i = 0; i < n_reads; ++i) if (counts[i] < 0) { h->err = "bwagpu_dedup_flat: a negative count"; return BWAGPU_EINVAL; }
	FlatLists F; RegLists L;
	if (!F.scan(h, (size_t)n_reads, counts, regs, nullptr)) { h->err = "bwagpu_dedup_flat: a count outside [0, 2^30), or counts without regions"; return BWAGPU_EINVAL; }
	if (F.tot > 0x7fffffff) { h->err = "bwagpu_dedup_flat: more than 2^31 - 1 regions"; return BWAGPU_EINVAL; }
	FlatReads R;
	if (!R.scan(h, "bwagpu_dedup_flat", (size_t)n_reads, seqs, seq_off) || (R.first != 0 && !R.bad_offsets(h, "bwagpu_dedup_flat"))) return BWAGPU_EINVAL;      // R.first: this call's reads begin at seqs[0] (the pair calls take any first offset)
	if (!R.codes_ok(h, "bwagpu_dedup_flat")) return BWAGPU_EINVAL;
	const int max_len = R.max_len;
	for (int i = 0; i < n_reads; ++i) {
		const i64 len = seq_off[i + 1] - seq_off[i];
		for (i64 k = F.off[(size_t)i]; k < F.off[(size_t)i + 1]; ++k) {
			const bwagpu_alnreg_t &a = regs[k];
			if (a.qb < 0 || a.qe < a.qb || a.qe > len) { h->err = "bwagpu_dedup_flat: region " + std::to_string(k) + ": qb < 0, qe < qb or qe beyond the read"; return BWAGPU_EINVAL; }
			if (a.rb < 0 || a.re <= a.rb || a.re > 2 * h->l_pac) { h->err = "bwagpu_dedup_flat: region " + std::to_string(k) + ": rb < 0, re <= rb or re beyond 2 l_pac"; return BWAGPU_EINVAL; }
			if (a.rb < h->l_pac && a.re > h->l_pac) { h->err = "bwagpu_dedup_flat: region " + std::to_string(k) + ": bridges l_pac"; return BWAGPU_EINVAL; }
			if (a.rid >= h->n_seqs) { h->err = "bwagpu_dedup_flat: region " + std::to_string(k) + ": rid beyond the index's contigs"; return BWAGPU_EINVAL; }      // (the stage looks its alt flag up)
		}
	}
	const BusyGuard busy(h->ibuf->busy);
	HIPCHK(h, hipSetDevice(h->device));
	*regs_out = nullptr; *n_out = 0;
	if (n_reads == 0) {
		ResultBlock<bwagpu_alnreg_t> none = result_block<bwagpu_alnreg_t>(0);
		if (!none) return BWAGPU_ENOMEM;
		*regs_out = none.release();
		return BWAGPU_OK;
	}
	const int n = n_reads;
	const BwagpuConfig &cfg = h->cfg;
	const bool long_batch = max_len > WAVE_EXT_MAX_LEN;      // (as bwagpu_batch_run)
	const long long share_pct = cfg.share >= 0 ? cfg.share : (h->ibuf->refs.load() >= 3 && busy.others > 0 ? 50 : 100);
	// lanes of the lane-per-read kernel and the waves that own a DP scratch region (resident_threads / dp_wave_count, for these reads)
	i64 lanes = ((i64)n + BLOCK - 1) / BLOCK * BLOCK; if (lanes > 256 * BLOCK) lanes = 256 * BLOCK;
	int dp_waves = (int)(lanes / 64);
	if (long_batch) { const int want = n < 1024 ? n : 1024; if (want > dp_waves) dp_waves = want; }
	DedupPlan dd;
	if (int rc = dedup_plan(h, opt, cfg, max_len, n, long_batch, share_pct, dp_waves, dd)) return rc;
	DevBuf *D = h->d_df;
	const size_t dp_bytes = (size_t)dp_waves * ((size_t)max_len + 2) * DPS * 4;
	if (D[bwagpu_s::DF_REGS].ensure((size_t)(F.tot ? F.tot : 1) * sizeof(bwagpu_alnreg_t)) ||
		D[bwagpu_s::DF_REGOFF].ensure(((size_t)n + 1) * 8) || D[bwagpu_s::DF_NRAW].ensure((size_t)n * 4 + 16) || D[bwagpu_s::DF_CNT].ensure((size_t)n * 4 + 16) || D[bwagpu_s::DF_FORM].ensure((size_t)n * 4 + 16) ||
		D[bwagpu_s::DF_BLOB].ensure(((size_t)F.tot + 8) * SLOT_BLOB_BYTES) || D[bwagpu_s::DF_DPH].ensure(dp_bytes) || D[bwagpu_s::DF_DPE].ensure(dp_bytes) || D[bwagpu_s::DF_CTR].ensure(sizeof(Counters))) {
		h->err = "hipMalloc failed (dedup_flat)"; return BWAGPU_ENOMEM;
	}
	if (int rc = R.upload(h, "dedup_flat")) return rc;      // (this call's wait below covers the copies)
	if (F.tot) HIPCHK(h, hipMemcpyAsync(D[bwagpu_s::DF_REGS].p, regs, (size_t)F.tot * sizeof(bwagpu_alnreg_t), hipMemcpyHostToDevice, h->stream));
	HIPCHK(h, hipMemcpyAsync(D[bwagpu_s::DF_REGOFF].p, F.off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, h->stream));
	HIPCHK(h, hipMemcpyAsync(D[bwagpu_s::DF_NRAW].p, counts, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
	HIPCHK(h, hipMemsetAsync(D[bwagpu_s::DF_CNT].p, 0, (size_t)n * 4, h->stream));
	HIPCHK(h, hipMemsetAsync(D[bwagpu_s::DF_FORM].p, 0xff, (size_t)n * 4, h->stream));
	HIPCHK(h, hipMemsetAsync(D[bwagpu_s::DF_CTR].p, 0, sizeof(Counters), h->stream));
	HIPCHK(h, wait_stream(h));      // (the caller's arrays are pageable)
	Batch B; memset(&B, 0, sizeof B);
	B.n_reads = n; B.max_len = max_len; B.stats = h->stats_on;
	B.seq = h->d_pf_seq.as<u8>(); B.off = h->d_pf_seqoff.as<i64>(); B.ctr = D[bwagpu_s::DF_CTR].as<Counters>();
	B.regs = D[bwagpu_s::DF_REGS].as<bwagpu_alnreg_t>(); B.reg_cap = F.tot; B.reg_off = D[bwagpu_s::DF_REGOFF].as<i64>();
	B.reg_n_raw = D[bwagpu_s::DF_NRAW].as<i32>(); B.reg_n = D[bwagpu_s::DF_CNT].as<i32>(); B.regs_raw = nullptr;
	// the sorts' key scratch (dev_sort_regs_by_key): read i's block of the blob begins at slot reg_off[i] and has counts[i] slots, one 64-byte chain record -- room for a RegKey -- each
	B.slot_blob = D[bwagpu_s::DF_BLOB].as<u8>(); B.seed_off = B.reg_off; B.seed_n = B.reg_n_raw; B.slot_cap = F.tot;
	B.dp_h = D[bwagpu_s::DF_DPH].as<i32>(); B.dp_e = D[bwagpu_s::DF_DPE].as<i32>(); B.dp_waves = dp_waves;
	B.dd_form = D[bwagpu_s::DF_FORM].as<i32>();
	dedup_launch(h, opt, cfg, B, max_len, n, long_batch, share_pct, (unsigned)(lanes / BLOCK), dd);
	HIPCHK(h, hipGetLastError());
	std::vector<bwagpu_alnreg_t> all((size_t)(F.tot ? F.tot : 1));
	std::vector<i32> forms((size_t)n);
	if (F.tot) HIPCHK(h, hipMemcpyAsync(all.data(), D[bwagpu_s::DF_REGS].p, (size_t)F.tot * sizeof(bwagpu_alnreg_t), hipMemcpyDeviceToHost, h->stream));
	HIPCHK(h, hipMemcpyAsync(counts_out, D[bwagpu_s::DF_CNT].p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(h, hipMemcpyAsync(forms.data(), D[bwagpu_s::DF_FORM].p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(h, wait_stream(h));
	i64 tot_out = 0;
	for (int i = 0; i < n; ++i) {
		if (counts_out[i] < 0 || counts_out[i] > counts[i] || forms[(size_t)i] < 0) { h->err = "bwagpu_dedup_flat: read " + std::to_string(i) + " was not finished"; return BWAGPU_EHIP; }
		tot_out += counts_out[i];
	}
	ResultBlock<bwagpu_alnreg_t> res = result_block<bwagpu_alnreg_t>((size_t)tot_out);
	if (!res) return BWAGPU_ENOMEM;
	i64 k = 0;
	for (int i = 0; i < n; ++i) for (int j = 0; j < counts_out[i]; ++j) res[(size_t)k++] = all[(size_t)(F.off[(size_t)i] + j)];
	if (form) memcpy(form, forms.data(), (size_t)n * 4);
	*n_out = tot_out; *regs_out = res.release();
	return BWAGPU_OK;
}

// the largest argument a logarithm of the marking can get: a region's longer side, its seed coverage, its incoming sub_n plus the increments of both rounds plus one
static i64 pri_log_need(const i32 *counts, const bwagpu_alnreg_t *regs, int n)
{
	i64 need = 0, k = 0;
	for (int i = 0; i < n; ++i)
		for (int j = 0; j < counts[i]; ++j, ++k) {
			const bwagpu_alnreg_t &a = regs[k];
			const i64 lq = (i64)a.qe - a.qb, lr = a.re - a.rb, sn = (i64)a.sub_n + 2 * (i64)counts[i] + 1;
			need = std::max(std::max(need, lq), std::max(std::max(lr, sn), (i64)a.seedcov));
		}
	return need;
}
// the largest n_pri[2p] + n_pri[2p + 1]: sizes the pairing kernels' HBM form
static i64 max_pair_sum(const i32 *npri, int np)
{
	i64 m = 0;
	for (int p = 0; p < np; ++p) m = std::max(m, (i64)npri[2 * (size_t)p] + npri[2 * (size_t)p + 1]);
	return m;
}
static bwagpu_pes_t pes_of(const bwagpu_pestat_t &pe) { bwagpu_pes_t r; r.low = pe.low; r.high = pe.high; r.failed = pe.failed; r.pad_ = 0; return r; }

// The task kernels of mate rescue on the reads of L (reads 2p, 2p + 1 mates; sequences d_seq / d_seqoff): k_matesw_tasks, then k_matesw_sw on the *nt tasks it
// found, results in d_msw_out.  d_toff / d_tix: the table of dev_rescue.h, or null.  Returns with the alignment kernel in the stream.
static int matesw_launch(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pes_t pes[4], const RegLists &L, const u8 *d_seq, const i64 *d_seqoff, const i64 *d_toff, i32 *d_tix,
						 i64 task_cap, unsigned long long *n_tasks_out)
{
	const int waves = 1024, n = L.n;
	if (h->d_msw_tasks.ensure((size_t)task_cap * sizeof(MateTask)) || h->d_msw_out.ensure((size_t)task_cap * sizeof(bwagpu_matesw_t)) ||
		h->d_msw_pes.ensure(4 * sizeof(bwagpu_pes_t)) || h->d_ctr.ensure(sizeof(Counters))) {
		h->err = "hipMalloc failed (mate rescue)"; return BWAGPU_ENOMEM;
	}
	unsigned long long *n_tasks = &h->d_ctr.as<Counters>()->next_chain, *next = &h->d_ctr.as<Counters>()->next_dedup;   // idle counters at this point
	HIPCHK(h, hipMemsetAsync(n_tasks, 0, 8, h->stream));
	HIPCHK(h, hipMemsetAsync(next, 0, 8, h->stream));
	HIPCHK(h, hipMemcpyAsync(h->d_msw_pes.p, pes, 4 * sizeof(bwagpu_pes_t), hipMemcpyHostToDevice, h->stream));
	int nb = (n / 2 + BLOCK - 1) / BLOCK; if (nb > 8192) nb = 8192; if (nb < 1) nb = 1;
	(void)hipEventRecord(h->ev[4], h->stream);      // (ev[4] .. ev[5]: the task kernel; ev[6]: ahead of the alignment kernel -- rescue_run's kernel time is the sum of its segments, not a span over its host waits)
	hipLaunchKernelGGL(k_matesw_tasks, dim3(nb), dim3(BLOCK), 0, h->stream, h->ix, *opt, n, L.d_cnt, L.d_off, L.d_regs,
					   h->d_msw_pes.as<bwagpu_pes_t>(), h->d_msw_tasks.as<MateTask>(), n_tasks, task_cap, d_toff, d_tix);
	HIPCHK(h, hipGetLastError());
	(void)hipEventRecord(h->ev[5], h->stream);
	unsigned long long nt = 0;
	HIPCHK(h, hipMemcpyAsync(&nt, n_tasks, 8, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(h, wait_stream(h));
	if ((i64)nt > task_cap) nt = (unsigned long long)task_cap;
	(void)hipEventRecord(h->ev[6], h->stream);
	if (nt) {
		Batch B = {}; B.seq = const_cast<u8*>(d_seq); B.off = const_cast<i64*>(d_seqoff); B.n_reads = n;      // (k_matesw_sw reads the sequences and their offsets, nothing else of the batch)
		const i64 want = ((i64)nt + 3) / 4;           // one wavefront per alignment, four per workgroup
		hipLaunchKernelGGL(k_matesw_sw, dim3((unsigned)(want < waves / 4 * 8 ? want : waves / 4 * 8)), dim3(BLOCK), 0, h->stream, h->ix, *opt, B, h->d_msw_pes.as<bwagpu_pes_t>(), h->d_msw_tasks.as<MateTask>(), (i64)nt,
						   h->d_msw_out.as<bwagpu_matesw_t>(), next);
		HIPCHK(h, hipGetLastError());
	}
	*n_tasks_out = nt;
	return BWAGPU_OK;
}

extern "C" int bwagpu_batch_matesw(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pes_t pes[4], bwagpu_matesw_t **out, int64_t *n_out)
{
	if (!h || !opt || !pes || !h->ran || h->packed_tot < 0 || !out || !n_out) return BWAGPU_EINVAL;
	if (opt->e_del <= 0 || opt->e_ins <= 0 || (h->n_reads & 1)) return BWAGPU_EINVAL;
	const BusyGuard busy(h->ibuf->busy);
	static_assert(sizeof(bwagpu_matesw_t) == 56 && sizeof(MateTask) == 24 && sizeof(bwagpu_pes_t) == 16, "layout");
	HIPCHK(h, hipSetDevice(h->device));
	const int n = h->n_reads;
	*out = nullptr; *n_out = 0;
	if (n == 0 || h->packed_tot == 0) { *out = (bwagpu_matesw_t*)malloc(sizeof(bwagpu_matesw_t)); return *out ? BWAGPU_OK : BWAGPU_ENOMEM; }
	unsigned long long nt = 0;
	const int rc = matesw_launch(h, opt, pes, lists_of_batch(h, 0), h->d_seq.as<u8>(), h->d_off.as<i64>(), nullptr, nullptr, (i64)n * 2 + 1024 /* more candidates than this are simply left to the host */, &nt);
	if (rc != BWAGPU_OK) { (void)wait_stream(h); return rc; }
	ResultBlock<bwagpu_matesw_t> res = result_block<bwagpu_matesw_t>((size_t)nt);
	if (!res) { (void)wait_stream(h); return BWAGPU_ENOMEM; }
	if (nt) {
		HIPCHK(h, hipMemcpyAsync(res.get(), h->d_msw_out.p, (size_t)nt * sizeof(bwagpu_matesw_t), hipMemcpyDeviceToHost, h->stream));
		HIPCHK(h, wait_stream(h));
	}
	*out = res.release(); *n_out = (int64_t)nt;
	return BWAGPU_OK;
}

// ---- primary/secondary marking + mapQ on the device (dev_primary.h) ---------------------------------------------------------------------------
extern "C" void bwagpu_primary_limits(int32_t out[4]) { out[0] = PRI_LANE_MAX; out[1] = PRI_LDS_SMALL; out[2] = PRI_LDS_BIG; out[3] = PRI_SCAN; }

static const i64 PRI_LOG_MAX = (i64)1 << 22;      // entries the table of logarithms is grown to at most (32 MB); arguments beyond it are the host's
// the marking records whose mapQ needs the host's logarithm (flags bit 0), counted: a caller that leaves the records on the device asks this instead of reading them
__global__ void __launch_bounds__(256) k_primary_misses(const bwagpu_primary_t *recs, i64 tot, unsigned int *n_miss)
{
	for (i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x; k < tot; k += (i64)gridDim.x * blockDim.x) if (recs[k].flags & 1) atomicAdd(n_miss, 1u);
}
// The kernels of both entry points on the lists L (its largest count sizes the HBM form): records to a result block (*out), return values to n_pri.
// log_need = the largest argument of a logarithm to expect.  resident: the records are wanted in d_pri_out only (out may be null) -- they come to the host
// only if one of them needs the host's logarithm (k_primary_misses counts those), and go back completed.
static int primary_run(bwagpu_t *h, const bwagpu_opt_t *opt, RegLists L, i64 log_need, bwagpu_primary_t **out, int32_t *n_pri, float *kernel_ms, bool resident = false)
{
	const int n_reads = L.n, max_cnt = L.max_cnt;
	const i64 tot = L.tot;
	if (kernel_ms) *kernel_ms = 0.f;
	ResultBlock<bwagpu_primary_t> res = result_block<bwagpu_primary_t>(resident ? 0 : (size_t)tot);
	if (!res) return BWAGPU_ENOMEM;
	if (n_reads == 0) { if (out) *out = res.release(); return BWAGPU_OK; }
	// the table of logarithms: the host's log() of every integer a mapQ of this batch can ask for (option pri_log_cap: a table of exactly that many entries, for tests)
	i64 log_n = log_need + 1 < 4096 ? 4096 : log_need + 1;
	if (log_n > PRI_LOG_MAX) log_n = PRI_LOG_MAX;
	if (h->cfg.pri_log_cap > 0) log_n = h->cfg.pri_log_cap < PRI_LOG_MAX ? h->cfg.pri_log_cap : PRI_LOG_MAX;
	if ((i64)h->pri_log.size() < log_n) { const size_t was = h->pri_log.size(); h->pri_log.resize((size_t)log_n); for (size_t k = was; k < (size_t)log_n; ++k) h->pri_log[k] = log((double)k); }
	const int n_hbm = max_cnt > PRI_LDS_BIG ? (n_reads < 64 ? n_reads : 64) : 0;      // workgroups of the HBM form
	const void *log_was = h->d_pri_log.p;
	if (h->d_pri_out.ensure((size_t)(tot ? tot : 1) * sizeof(bwagpu_primary_t)) || h->d_pri_npri.ensure((size_t)n_reads * 4) || h->d_pri_lists.ensure((size_t)n_reads * 3 * 4) ||
		h->d_pri_ctr.ensure(4 * sizeof(unsigned int)) || h->d_pri_log.ensure((size_t)log_n * 8) || (n_hbm && h->d_pri_scratch.ensure((size_t)n_hbm * max_cnt * PRI_WORDS * 4))) {
		h->err = "hipMalloc failed (primary)"; return BWAGPU_ENOMEM;
	}
	hipError_t e = hipSuccess;
	if (h->pri_log_dev < log_n || h->d_pri_log.p != log_was) { /* (a buffer that had to grow is a new one) */ e = hipMemcpyAsync(h->d_pri_log.p, h->pri_log.data(), (size_t)log_n * 8, hipMemcpyHostToDevice, h->stream); h->pri_log_dev = log_n; }
	if (e == hipSuccess) e = hipMemsetAsync(h->d_pri_ctr.p, 0, 4 * sizeof(unsigned int), h->stream);
	const PriLogTab lg = { h->d_pri_log.as<double>(), (int)log_n };
	bwagpu_primary_t *d_out = h->d_pri_out.as<bwagpu_primary_t>();
	i32 *d_npri = h->d_pri_npri.as<i32>(), *lists = h->d_pri_lists.as<i32>();
	unsigned int *list_n = h->d_pri_ctr.as<unsigned int>();
	(void)hipEventRecord(h->ev[0], h->stream);
	if (e == hipSuccess) {
		int nb = (n_reads + PRI_LANE_BLOCK - 1) / PRI_LANE_BLOCK; if (nb > 256 * 12) nb = 256 * 12;
		hipLaunchKernelGGL(k_primary_lane, dim3(nb), dim3(PRI_LANE_BLOCK), 0, h->stream, *opt, n_reads, L.d_cnt, L.d_off, L.d_regs, L.d_ids, L.id0, lg, d_out, d_npri, lists, list_n);
		e = hipGetLastError();
	}
	// the wavefront forms draw their reads from the lists the first kernel left (their lengths stay on the device); a form no read of the batch can need is not launched
	if (e == hipSuccess && max_cnt > PRI_LANE_MAX) {
		const int nb = n_reads < 256 * 16 ? n_reads : 256 * 16;
		hipLaunchKernelGGL(k_primary_wave<PRI_LDS_SMALL>, dim3(nb), dim3(64), 0, h->stream, *opt, L.d_cnt, L.d_off, L.d_regs, L.d_ids, L.id0, lg, d_out, d_npri, lists, list_n, (u64*)nullptr, 0);
		e = hipGetLastError();
	}
	if (e == hipSuccess && max_cnt > PRI_LDS_SMALL) {
		const int nb = n_reads < 256 * 3 ? n_reads : 256 * 3;
		hipLaunchKernelGGL(k_primary_wave<PRI_LDS_BIG>, dim3(nb), dim3(64), 0, h->stream, *opt, L.d_cnt, L.d_off, L.d_regs, L.d_ids, L.id0, lg, d_out, d_npri, lists + n_reads, list_n + 1, (u64*)nullptr, 0);
		e = hipGetLastError();
	}
	if (e == hipSuccess && n_hbm) {
		hipLaunchKernelGGL(k_primary_wave<0>, dim3(n_hbm), dim3(64), 0, h->stream, *opt, L.d_cnt, L.d_off, L.d_regs, L.d_ids, L.id0, lg, d_out, d_npri, lists + (size_t)2 * n_reads, list_n + 2, h->d_pri_scratch.as<u64>(), max_cnt);
		e = hipGetLastError();
	}
	if (e == hipSuccess && resident && tot) {      // (list_n[3]: no list of the wavefront forms)
		hipLaunchKernelGGL(k_primary_misses, dim3((unsigned)((tot + 255) / 256 < 1024 ? (tot + 255) / 256 : 1024)), dim3(256), 0, h->stream, d_out, tot, list_n + 3);
		e = hipGetLastError();
	}
	(void)hipEventRecord(h->ev[1], h->stream);
	std::vector<i32> np((size_t)n_reads);
	unsigned int n_miss = 0;
	if (e == hipSuccess && tot && !resident) e = hipMemcpyAsync(res.get(), d_out, (size_t)tot * sizeof(bwagpu_primary_t), hipMemcpyDeviceToHost, h->stream);
	if (e == hipSuccess && resident) e = hipMemcpyAsync(&n_miss, list_n + 3, sizeof n_miss, hipMemcpyDeviceToHost, h->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(np.data(), d_npri, (size_t)n_reads * 4, hipMemcpyDeviceToHost, h->stream);
	if (e == hipSuccess) e = wait_stream(h);
	HIPCHK(h, e);
	if (kernel_ms) (void)hipEventElapsedTime(kernel_ms, h->ev[0], h->ev[1]);
	for (int i = 0; i < n_reads; ++i) if (np[i] < 0) { h->err = "internal: a read outgrew the marking kernel's working arrays"; return BWAGPU_EHIP; }
	if (n_pri) memcpy(n_pri, np.data(), (size_t)n_reads * 4);
	if (resident) {
		if (n_miss == 0) return BWAGPU_OK;
		res = result_block<bwagpu_primary_t>((size_t)tot);
		if (!res) return BWAGPU_ENOMEM;
		HIPCHK(h, hipMemcpyAsync(res.get(), d_out, (size_t)tot * sizeof(bwagpu_primary_t), hipMemcpyDeviceToHost, h->stream));
		HIPCHK(h, wait_stream(h));
	}
	// records whose mapQ needed a logarithm outside the table: the same function with the host's log()
	bool any = false;
	for (i64 k = 0; k < tot && !any; ++k) any = (res[k].flags & 1) != 0;
	if (any) {
		ListsMirror M;
		HIPCHK(h, M.fetch(h, L));
		i64 base = 0;
		for (int i = 0; i < n_reads; ++i) {
			for (int k = 0; k < L.h_cnt[i]; ++k) {
				bwagpu_primary_t &r = res[base + k];
				int miss = 0;
				if (r.flags & 1) r.mapq = pri_mapq(*opt, L.h_regs[base + r.src], r.sub, r.sub_n, PriLogLibm(), miss);
			}
			base += L.h_cnt[i];
		}
	}
	if (resident) {
		HIPCHK(h, hipMemcpyAsync(d_out, res.get(), (size_t)tot * sizeof(bwagpu_primary_t), hipMemcpyHostToDevice, h->stream));
		HIPCHK(h, wait_stream(h));      // (the block goes back to the pool when this returns)
		return BWAGPU_OK;
	}
	*out = res.release();
	return BWAGPU_OK;
}

// primary_run's log_need for the last download: a logarithm's argument is at most the longer side of a region (the read, or the read and the gaps its band
// allows), its seed coverage (at most the read), or the read's number of regions plus one
static i64 batch_log_need(const bwagpu_t *h, const bwagpu_opt_t *opt)
{
	const i64 need = 2 * (i64)h->max_len + 4 * (i64)(opt->w > 0 ? opt->w : 0) + 64;
	return h->packed_max + 2 > need ? h->packed_max + 2 : need;
}

extern "C" int bwagpu_batch_primary(bwagpu_t *h, const bwagpu_opt_t *opt, int64_t id0, bwagpu_primary_t **out, int64_t *n_out, int32_t *n_pri, float *kernel_ms)
{
	if (!h || !opt || !h->ran || !h->downloaded || !out || !n_out) return BWAGPU_EINVAL;
	const BusyGuard busy(h->ibuf->busy);
	HIPCHK(h, hipSetDevice(h->device));
	const i64 tot = h->packed_tot < 0 ? 0 : h->packed_tot;
	const i64 log_need = batch_log_need(h, opt);
	*out = nullptr; *n_out = 0;
	if (tot == 0) {      // no region in the whole batch: nothing to run (and the packed arrays may not exist)
		ResultBlock<bwagpu_primary_t> res = result_block<bwagpu_primary_t>(0);
		if (!res) return BWAGPU_ENOMEM;
		if (n_pri) for (int i = 0; i < h->n_reads; ++i) n_pri[i] = 0;
		if (kernel_ms) *kernel_ms = 0.f;
		*out = res.release();
		return BWAGPU_OK;
	}
	const int rc = primary_run(h, opt, lists_of_batch(h, id0), log_need, out, n_pri, kernel_ms);
	if (rc == BWAGPU_OK) *n_out = tot;
	return rc;
}

extern "C" int bwagpu_primary_flat(bwagpu_t *h, const bwagpu_opt_t *opt, int n_reads, const int32_t *counts, const bwagpu_alnreg_t *regs, const int64_t *ids,
								   bwagpu_primary_t **out, int32_t *n_pri, float *kernel_ms)
{
	if (!h || !opt || n_reads < 0 || !out || (n_reads > 0 && (!counts || !ids))) return BWAGPU_EINVAL;
	FlatLists F; RegLists L;
	if (!F.scan(h, (size_t)n_reads, counts, regs, nullptr)) return BWAGPU_EINVAL;
	const BusyGuard busy(h->ibuf->busy);
	HIPCHK(h, hipSetDevice(h->device));
	*out = nullptr;
	const int rc = F.upload(h, "primary", counts, regs, ids, (size_t)n_reads, L);
	return rc != BWAGPU_OK ? rc : primary_run(h, opt, L, pri_log_need(counts, regs, n_reads), out, n_pri, kernel_ms);
}

// ---- pairing on the device (dev_pair.h) ------------------------------------------------------------------------------------------------------------
extern "C" void bwagpu_pair_limits(int32_t out[3]) { out[0] = PAIR_LANE_MAX; out[1] = PAIR_LDS_SMALL; out[2] = PAIR_LDS_BIG; }

static const i64 PAIR_TAB_DEFAULT = (i64)1 << 18;      // entries of the table of log(2 erfc) values unless option pair_tab_cap says otherwise (2 MB)
// bwamem_pair.c:243-244: the term of q that depends on the distance alone, by the host's libm
static double pair_tab_value(i64 dist, const bwagpu_pestat_t &pe)
{
	const double ns = (dist - pe.avg) / pe.std;
	return log(2. * erfc(fabs(ns) * M_SQRT1_2));
}

// mem_pair of one pair on the host, with the host's erfc / log: the records of pairs that met a distance outside the table.  The same statement of the
// function as pair_read (dev_pair.h): sort by (x, y), the candidate set of every i, the two largest candidates, the count.
static bwagpu_pair_t pair_host(const bwagpu_opt_t &opt, const bwagpu_pestat_t pes[4], i64 l_pac, const std::vector<i64> &ctg_off, const bwagpu_alnreg_t *a0, const bwagpu_primary_t *s0, int n0,
							   const bwagpu_alnreg_t *a1, const bwagpu_primary_t *s1, int n1, int id)
{
	bwagpu_pair_t rec = pair_none(); rec.flags = 1;
	std::vector<std::pair<u64, u64>> v;
	for (int r = 0; r < 2; ++r)
		for (int i = 0; i < (r ? n1 : n0); ++i) {
			const bwagpu_alnreg_t &g = r ? a1[s1 ? s1[i].src : i] : a0[s0 ? s0[i].src : i];
			u64 x, y;
			pair_key(g, i, r, l_pac, g.rid >= 0 && (size_t)g.rid < ctg_off.size() ? ctg_off[(size_t)g.rid] : 0, x, y);
			v.emplace_back(x, y);
		}
	std::sort(v.begin(), v.end());      // (a total order: the (i, r) are distinct)
	u64 bx = 0, by = 0, cx = 0, cy = 0;      // the largest and the second largest candidate
	std::vector<int> qs; std::vector<u64> ys;
	for (int i = 0; i < (int)v.size(); ++i)
		for (int k = i - 1; k >= 0; --k) {
			const i64 dist = (i64)v[i].first - (i64)v[k].first;
			if (((v[k].second ^ v[i].second) & 1) == 0) continue;
			const int dir = (int)(v[k].second & 2) | (int)(v[i].second >> 1 & 1);
			if (pes[dir].failed || dist < pes[dir].low || dist > pes[dir].high) continue;
			const int q = pair_q(v[i].second >> 32, v[k].second >> 32, pair_tab_value(dist, pes[dir]), opt.a);
			const u64 py = (u64)k << 32 | (u64)i, px = pair_cand_x(q, py, id);
			if (pair_lt(bx, by, px, py)) { cx = bx; cy = by; bx = px; by = py; }
			else if (pair_lt(cx, cy, px, py)) { cx = px; cy = py; }
			qs.push_back(q); ys.push_back(py);
		}
	rec.n_cand = (i64)qs.size();
	if (qs.empty()) return rec;
	const u64 yk = v[(size_t)(by >> 32)].second, yi = v[(size_t)(by & 0xffffffffu)].second;
	rec.z[yk & 1] = (int)((yk & 0xffffffffu) >> 2); rec.z[yi & 1] = (int)((yi & 0xffffffffu) >> 2);
	rec.score = (int)(bx >> 32);
	if (qs.size() > 1) {
		const int tmp = pair_tmp(opt);
		rec.sub = (int)(cx >> 32);
		for (size_t j = 0; j < qs.size(); ++j) if (ys[j] != by && rec.sub - qs[j] <= tmp) ++rec.n_sub;
	}
	return rec;
}

// What pairing reads besides the lists, on the device and (always) on the host: the first npri[] places of each list take part; src: the marking records at the
// lists' offsets, or null on both sides; pair p has id ids[p], or (null on both sides) id0 + p -- the lists' own ids are the reads'.
struct PairSel { const i32 *d_npri, *h_npri; const bwagpu_primary_t *d_src, *h_src; const i64 *d_ids, *h_ids; i64 id0; };
// The kernels of both entry points on the L.n / 2 pairs of the lists L (reads 2p, 2p + 1) as S selects them: records to a result block (*out).
static int pair_run(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pestat_t pes[4], RegLists L, const PairSel &S, bwagpu_pair_t **out, float *kernel_ms)
{
	const int n_pairs = L.n / 2;
	const i64 max_sum = max_pair_sum(S.h_npri, n_pairs);
	if (kernel_ms) *kernel_ms = 0.f;
	ResultBlock<bwagpu_pair_t> res = result_block<bwagpu_pair_t>((size_t)n_pairs);
	if (!res) return BWAGPU_ENOMEM;
	if (n_pairs == 0) { *out = res.release(); return BWAGPU_OK; }
	// the table: for every orientation that has not failed, the distances low .. high as far as the capacity goes, in the order of the orientations
	const i64 cap = h->cfg.pair_tab_cap > 0 ? h->cfg.pair_tab_cap : PAIR_TAB_DEFAULT;
	if (!h->pair_tab_dev || h->pair_tab_cap != cap || memcmp(h->pair_tab_pes, pes, sizeof h->pair_tab_pes) != 0) {
		i64 used = 0;
		for (int d = 0; d < 4; ++d) {
			i64 len = pes[d].failed || pes[d].high < pes[d].low ? 0 : (i64)pes[d].high - pes[d].low + 1;
			if (len > cap - used) len = cap - used;
			h->pair_toff[d] = (i32)used; h->pair_tlen[d] = (i32)len; used += len;
		}
		h->pair_tab.resize((size_t)(used ? used : 1));
		for (int d = 0; d < 4; ++d)
			for (i64 k = 0; k < h->pair_tlen[d]; ++k) h->pair_tab[(size_t)(h->pair_toff[d] + k)] = pair_tab_value((i64)pes[d].low + k, pes[d]);
		memcpy(h->pair_tab_pes, pes, sizeof h->pair_tab_pes); h->pair_tab_cap = cap; h->pair_tab_dev = false;
	}
	const int n_hbm = max_sum > PAIR_LDS_BIG ? (n_pairs < 64 ? n_pairs : 64) : 0;      // workgroups of the HBM form
	if (max_sum > 0x3fffffff) return BWAGPU_EINVAL;
	const void *tab_was = h->d_pair_tab.p;
	if (h->d_pair_out.ensure((size_t)n_pairs * sizeof(bwagpu_pair_t)) || h->d_pair_lists.ensure((size_t)n_pairs * 3 * 4) || h->d_pair_ctr.ensure(4 * sizeof(unsigned int)) ||
		h->d_pair_tab.ensure(h->pair_tab.size() * 8) || (n_hbm && h->d_pair_scratch.ensure((size_t)n_hbm * (size_t)max_sum * PAIR_WORDS * 4))) {
		h->err = "hipMalloc failed (pair)"; return BWAGPU_ENOMEM;
	}
	hipError_t e = hipSuccess;
	if (!h->pair_tab_dev || h->d_pair_tab.p != tab_was) { e = hipMemcpyAsync(h->d_pair_tab.p, h->pair_tab.data(), h->pair_tab.size() * 8, hipMemcpyHostToDevice, h->stream); h->pair_tab_dev = true; }
	if (e == hipSuccess) e = hipMemsetAsync(h->d_pair_ctr.p, 0, 4 * sizeof(unsigned int), h->stream);
	PairWin P; P.t = h->d_pair_tab.as<double>();
	for (int d = 0; d < 4; ++d) { P.low[d] = pes[d].low; P.high[d] = pes[d].high; P.failed[d] = pes[d].failed || pes[d].high < pes[d].low; P.toff[d] = h->pair_toff[d]; P.tlen[d] = h->pair_tlen[d]; }
	bwagpu_pair_t *d_out = h->d_pair_out.as<bwagpu_pair_t>();
	i32 *lists = h->d_pair_lists.as<i32>();
	unsigned int *list_n = h->d_pair_ctr.as<unsigned int>();
	const i64 *ctg = h->ix.ctg_off;
	(void)hipEventRecord(h->ev[0], h->stream);
	if (e == hipSuccess) {
		int nb = (n_pairs + PAIR_LANE_BLOCK - 1) / PAIR_LANE_BLOCK; if (nb > 256 * 12) nb = 256 * 12;
		hipLaunchKernelGGL(k_pair_lane, dim3(nb), dim3(PAIR_LANE_BLOCK), 0, h->stream, *opt, P, h->l_pac, h->n_seqs, ctg, n_pairs, S.d_npri, L.d_off, L.d_regs, S.d_src, S.d_ids, S.id0, d_out, lists, list_n);
		e = hipGetLastError();
	}
	// the wavefront forms draw their pairs from the lists the first kernel left; a form no pair of the batch can need is not launched
	if (e == hipSuccess && max_sum > PAIR_LANE_MAX) {
		const int nb = n_pairs < 256 * 16 ? n_pairs : 256 * 16;
		hipLaunchKernelGGL(k_pair_wave<PAIR_LDS_SMALL>, dim3(nb), dim3(64), 0, h->stream, *opt, P, h->l_pac, h->n_seqs, ctg, S.d_npri, L.d_off, L.d_regs, S.d_src, S.d_ids, S.id0, d_out, lists, list_n, (u64*)nullptr, 0);
		e = hipGetLastError();
	}
	if (e == hipSuccess && max_sum > PAIR_LDS_SMALL) {
		const int nb = n_pairs < 256 * 4 ? n_pairs : 256 * 4;
		hipLaunchKernelGGL(k_pair_wave<PAIR_LDS_BIG>, dim3(nb), dim3(64), 0, h->stream, *opt, P, h->l_pac, h->n_seqs, ctg, S.d_npri, L.d_off, L.d_regs, S.d_src, S.d_ids, S.id0, d_out, lists + n_pairs, list_n + 1, (u64*)nullptr, 0);
		e = hipGetLastError();
	}
	if (e == hipSuccess && n_hbm) {
		hipLaunchKernelGGL(k_pair_wave<0>, dim3(n_hbm), dim3(64), 0, h->stream, *opt, P, h->l_pac, h->n_seqs, ctg, S.d_npri, L.d_off, L.d_regs, S.d_src, S.d_ids, S.id0, d_out, lists + (size_t)2 * n_pairs, list_n + 2,
						   h->d_pair_scratch.as<u64>(), (int)max_sum);
		e = hipGetLastError();
	}
	(void)hipEventRecord(h->ev[1], h->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(res.get(), d_out, (size_t)n_pairs * sizeof(bwagpu_pair_t), hipMemcpyDeviceToHost, h->stream);
	if (e == hipSuccess) e = wait_stream(h);
	HIPCHK(h, e);
	if (kernel_ms) (void)hipEventElapsedTime(kernel_ms, h->ev[0], h->ev[1]);
	bool any = false;
	for (int p = 0; p < n_pairs; ++p) {
		if (res[p].flags & 2) { h->err = "internal: a pair outgrew the pairing kernel's working arrays"; return BWAGPU_EHIP; }
		any |= (res[p].flags & 1) != 0;
	}
	if (any) {      // pairs that met a distance outside the table: the same function with the host's erfc / log
		ListsMirror M;
		HIPCHK(h, M.fetch(h, L));
		for (int p = 0; p < n_pairs; ++p) {
			if (!(res[p].flags & 1)) continue;
			const i64 o0 = L.h_off[2 * (size_t)p], o1 = L.h_off[2 * (size_t)p + 1];
			res[p] = pair_host(*opt, pes, h->l_pac, h->h_ctg_off, L.h_regs + o0, S.h_src ? S.h_src + o0 : nullptr, S.h_npri[2 * (size_t)p], L.h_regs + o1, S.h_src ? S.h_src + o1 : nullptr,
							   S.h_npri[2 * (size_t)p + 1], (int)(S.h_ids ? S.h_ids[p] : S.id0 + p));
		}
	}
	*out = res.release();
	return BWAGPU_OK;
}

extern "C" int bwagpu_batch_pair(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pestat_t pes[4], int64_t id0, bwagpu_pair_t **pairs, int64_t *n_pairs,
								 bwagpu_primary_t **pri, int64_t *n_pri_recs, int32_t *n_pri, float *kernel_ms)
{
	if (!h || !opt || !pes || !h->ran || !h->downloaded || !pairs || !n_pairs) return BWAGPU_EINVAL;
	if ((h->n_reads & 1) || (id0 & 1) || (opt->flag & 0x800 /* MEM_F_PRIMARY5 */)) return BWAGPU_EINVAL;
	*pairs = nullptr; *n_pairs = 0;
	if (pri) *pri = nullptr;
	if (n_pri_recs) *n_pri_recs = 0;
	const int np = h->n_reads / 2;
	bwagpu_primary_t *recs_ = nullptr; int64_t n_recs = 0; float ms_pri = 0.f, ms_pair = 0.f;
	std::vector<i32> npri((size_t)h->n_reads);
	int rc = bwagpu_batch_primary(h, opt, id0, &recs_, &n_recs, npri.data(), &ms_pri);
	if (rc != BWAGPU_OK) return rc;
	ResultBlock<bwagpu_primary_t> recs(recs_);
	const BusyGuard busy(h->ibuf->busy);
	if (hipSetDevice(h->device) != hipSuccess) { h->err = "hipSetDevice failed"; return BWAGPU_EHIP; }
	ResultBlock<bwagpu_pair_t> res;
	if (n_recs == 0) {      // no region in the whole batch: every pair is without a candidate (and the packed arrays may not exist)
		res = result_block<bwagpu_pair_t>((size_t)np);
		if (!res) return BWAGPU_ENOMEM;
		for (int p = 0; p < np; ++p) res[p] = pair_none();
	} else {      // the marking's records and return values are still in its buffers
		const PairSel S = { h->d_pri_npri.as<i32>(), npri.data(), h->d_pri_out.as<bwagpu_primary_t>(), recs.get(), nullptr, nullptr, id0 >> 1 };
		bwagpu_pair_t *r = nullptr;
		rc = pair_run(h, opt, pes, lists_of_batch(h, id0), S, &r, &ms_pair);
		if (rc != BWAGPU_OK) return rc;
		res.reset(r);
	}
	*pairs = res.release(); *n_pairs = np;
	if (n_pri) memcpy(n_pri, npri.data(), (size_t)h->n_reads * 4);
	if (kernel_ms) *kernel_ms = ms_pri + ms_pair;
	if (pri) { *pri = recs.release(); if (n_pri_recs) *n_pri_recs = n_recs; }
	return BWAGPU_OK;
}

extern "C" int bwagpu_pair_flat(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pestat_t pes[4], int n_pairs, const int32_t *counts, const int32_t *n_pri,
								const bwagpu_alnreg_t *regs, const int64_t *ids, bwagpu_pair_t **pairs, float *kernel_ms)
{
	if (!h || !opt || !pes || n_pairs < 0 || n_pairs > 0x3fffffff || !pairs || (n_pairs > 0 && (!counts || !n_pri || !ids))) return BWAGPU_EINVAL;
	const size_t n_reads = (size_t)n_pairs * 2;
	for (size_t i = 0; i < n_reads; ++i) if (n_pri[i] < 0 || n_pri[i] > counts[i]) return BWAGPU_EINVAL;
	FlatLists F; RegLists L;
	if (!F.scan(h, n_reads, counts, regs, n_pri)) return BWAGPU_EINVAL;
	const BusyGuard busy(h->ibuf->busy);
	HIPCHK(h, hipSetDevice(h->device));
	*pairs = nullptr;
	const int rc = F.upload(h, "pair", counts, regs, ids, (size_t)n_pairs, L);
	if (rc != BWAGPU_OK) return rc;
	if (n_pairs) {
		if (h->d_pair_npri.ensure(n_reads * 4)) { h->err = "hipMalloc failed (pair)"; return BWAGPU_ENOMEM; }
		HIPCHK(h, hipMemcpyAsync(h->d_pair_npri.p, n_pri, n_reads * 4, hipMemcpyHostToDevice, h->stream));      // (the caller's array, in the stream ahead of the kernels)
	}
	const PairSel S = { h->d_pair_npri.as<i32>(), n_pri, nullptr, nullptr, L.d_ids, ids, 0 };
	L.d_ids = L.h_ids = nullptr;      // (the ids given are the pairs')
	return pair_run(h, opt, pes, L, S, pairs, kernel_ms);
}

// ---- the merge of mate-rescue hits on the device (dev_rescue.h) -----------------------------------------------------------------------------------
extern "C" void bwagpu_rescue_limits(int32_t out[4]) { out[0] = RESC_LANE_MAX; out[1] = RESC_LDS_MAX; out[2] = 0; out[3] = 0; }

// The kernels of both entry points on the L.n = 2 n_pairs reads of the lists L (sequences d_seq / d_seqoff): the task kernels, the replay, the packing, then -- for
// pri / pairs -- the marking and pairing kernels on the packed merged lists.
static int rescue_run(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pestat_t pes[4], const RegLists &L, const u8 *d_seq, const i64 *d_seqoff, int32_t *counts, bwagpu_alnreg_t **regs,
					  int32_t **src, int64_t *n_regs, bwagpu_rescue_t **rescue, bwagpu_primary_t **pri, int32_t *n_pri, bwagpu_pair_t **pairs, float *kernel_ms,
					  const bwagpu_opt_t *opt_count = nullptr /* the options k_rescue_count reads, where they differ from opt (sampe_run) */, float *ms_parts = nullptr /* rescue, marking, pairing */)
{
	const int n_reads = L.n, np = n_reads / 2;
	if (!opt_count) opt_count = opt;
	const i64 tot = L.tot;
	*regs = nullptr; *src = nullptr; *n_regs = 0; *rescue = nullptr;
	if (pri) *pri = nullptr;
	if (pairs) *pairs = nullptr;
	if (kernel_ms) *kernel_ms = 0.f;
	ResultBlock<bwagpu_alnreg_t> res_regs; ResultBlock<int32_t> res_src; ResultBlock<bwagpu_primary_t> res_pri; ResultBlock<bwagpu_pair_t> res_pair;
	ResultBlock<bwagpu_rescue_t> res_rec = result_block<bwagpu_rescue_t>((size_t)np);
	if (!res_rec) return BWAGPU_ENOMEM;
	std::vector<i32> npri((size_t)n_reads, 0);
	i64 mtot = 0;
	float ms_resc = 0.f, ms_pri = 0.f, ms_pair = 0.f;
	if (tot == 0) {      // no region in the whole batch: nothing to rescue from (and the packed arrays may not exist)
		for (int i = 0; i < n_reads; ++i) counts[i] = 0;
		for (int p = 0; p < np; ++p) { res_rec[p].n_aligned = res_rec[p].n_inline = res_rec[p].flags = res_rec[p].pad_ = 0; }
		res_regs = result_block<bwagpu_alnreg_t>(0); res_src = result_block<int32_t>(0);
		if (!res_regs || !res_src) return BWAGPU_ENOMEM;
	} else {
		const bwagpu_pes_t pes4[4] = { pes_of(pes[0]), pes_of(pes[1]), pes_of(pes[2]), pes_of(pes[3]) };
		DevBuf *D = h->d_rs;
		if (D[bwagpu_s::RS_X].ensure((size_t)n_reads * 4) || D[bwagpu_s::RS_TOFF].ensure(((size_t)n_reads + 1) * 8) || D[bwagpu_s::RS_CTR].ensure(64) || D[bwagpu_s::RS_ACNT].ensure((size_t)n_reads * 4) ||
			D[bwagpu_s::RS_POFF].ensure(((size_t)n_reads + 1) * 8) || D[bwagpu_s::RS_OUT].ensure((size_t)np * sizeof(bwagpu_rescue_t)) || D[bwagpu_s::RS_LISTS].ensure((size_t)np * 2 * 4)) {
			h->err = "hipMalloc failed (rescue)"; return BWAGPU_ENOMEM;
		}
		i32 *d_x = D[bwagpu_s::RS_X].as<i32>(), *d_acnt = D[bwagpu_s::RS_ACNT].as<i32>();
		i64 *d_toff = D[bwagpu_s::RS_TOFF].as<i64>(), *d_poff = D[bwagpu_s::RS_POFF].as<i64>();
		unsigned int *list_n = D[bwagpu_s::RS_CTR].as<unsigned int>();
		unsigned long long *d_maxcap = (unsigned long long*)(list_n + 2);
		HIPCHK(h, hipMemsetAsync(D[bwagpu_s::RS_CTR].p, 0, 64, h->stream));
		(void)hipEventRecord(h->ev[2], h->stream);
		int nb = (np + BLOCK - 1) / BLOCK; if (nb > 8192) nb = 8192;
		hipLaunchKernelGGL(k_rescue_count, dim3(nb), dim3(BLOCK), 0, h->stream, *opt_count, n_reads, L.d_cnt, L.d_off, L.d_regs, d_x, d_maxcap);
		HIPCHK(h, hipGetLastError());
		hipLaunchKernelGGL(k_rescue_scan, dim3(1), dim3(256), 0, h->stream, d_x, n_reads, d_toff);
		HIPCHK(h, hipGetLastError());
		(void)hipEventRecord(h->ev[3], h->stream);
		i64 extra = 0; unsigned long long max_cap = 0;
		HIPCHK(h, hipMemcpyAsync(&extra, d_toff + n_reads, 8, hipMemcpyDeviceToHost, h->stream));
		HIPCHK(h, hipMemcpyAsync(&max_cap, d_maxcap, 8, hipMemcpyDeviceToHost, h->stream));
		HIPCHK(h, wait_stream(h));
		if (max_cap > 0x3fffffffull) return BWAGPU_EINVAL;
		const int n_lds = np < 1024 ? np : 1024;      // workgroups of the form with its arrays in LDS (each has a staging area of RESC_LDS_MAX regions)
		const int n_hbm = (i64)max_cap > RESC_LDS_MAX ? (np < 64 ? np : 64) : 0;      // workgroups of the form with its keys in HBM
		if (D[bwagpu_s::RS_TIX].ensure((size_t)(extra ? extra : 1) * 4) || D[bwagpu_s::RS_ARENA].ensure((size_t)(tot + extra) * sizeof(bwagpu_alnreg_t)) || D[bwagpu_s::RS_ASRC].ensure((size_t)(tot + extra) * 4) ||
			(n_hbm && D[bwagpu_s::RS_KEYS].ensure((size_t)n_hbm * resc_stride(RESC_WORK_BYTES, (int)max_cap))) ||
			D[bwagpu_s::RS_STAGE].ensure(std::max((size_t)n_lds * resc_stride(RESC_STAGE_BYTES, RESC_LDS_MAX), (size_t)n_hbm * resc_stride(RESC_STAGE_BYTES, (int)max_cap)))) {
			h->err = "hipMalloc failed (rescue)"; return BWAGPU_ENOMEM;
		}
		i32 *d_tix = D[bwagpu_s::RS_TIX].as<i32>();
		HIPCHK(h, hipMemsetAsync(d_tix, 0xff, (size_t)(extra ? extra : 1) * 4, h->stream));
		unsigned long long nt = 0;
		if (extra) {
			const int rc = matesw_launch(h, opt, pes4, L, d_seq, d_seqoff, d_toff, d_tix, extra /* four per anchor: every task has its record */, &nt);
			if (rc != BWAGPU_OK) { (void)wait_stream(h); return rc; }
		} else {      // (no anchor in the batch: the replay copies the lists and reads neither windows nor tasks)
			if (h->d_msw_pes.ensure(4 * sizeof(bwagpu_pes_t)) || h->d_msw_out.ensure(sizeof(bwagpu_matesw_t))) { h->err = "hipMalloc failed (rescue)"; return BWAGPU_ENOMEM; }
			HIPCHK(h, hipMemcpyAsync(h->d_msw_pes.p, pes4, sizeof pes4, hipMemcpyHostToDevice, h->stream));
			(void)hipEventRecord(h->ev[6], h->stream);
		}
		RescIn R;
		R.seq = d_seq; R.seq_off = d_seqoff; R.cnt = L.d_cnt; R.off = L.d_off; R.regs = L.d_regs; R.pes = h->d_msw_pes.as<bwagpu_pes_t>();
		R.toff = d_toff; R.tix = d_tix; R.mres = h->d_msw_out.as<bwagpu_matesw_t>(); R.n_tasks = (i64)nt;
		R.arena = D[bwagpu_s::RS_ARENA].as<bwagpu_alnreg_t>(); R.asrc = D[bwagpu_s::RS_ASRC].as<i32>(); R.acnt = d_acnt; R.out = D[bwagpu_s::RS_OUT].as<bwagpu_rescue_t>();
		i32 *lists = D[bwagpu_s::RS_LISTS].as<i32>();
		nb = (np + RESC_LANE_BLOCK - 1) / RESC_LANE_BLOCK; if (nb > 256 * 16) nb = 256 * 16;
		hipLaunchKernelGGL(k_rescue_lane, dim3(nb), dim3(RESC_LANE_BLOCK), 0, h->stream, h->ix, *opt, R, np, lists, list_n);
		HIPCHK(h, hipGetLastError());
		// the wavefront forms draw their pairs from the lists the first kernel left; the first also takes what the lanes handed over, so it always runs
		hipLaunchKernelGGL(k_rescue_wave<RESC_LDS_MAX>, dim3(n_lds), dim3(64), 0, h->stream, h->ix, *opt, R, lists, list_n, (u8*)nullptr, 0, D[bwagpu_s::RS_STAGE].as<u8>());
		HIPCHK(h, hipGetLastError());
		if (n_hbm) {
			hipLaunchKernelGGL(k_rescue_wave<0>, dim3(n_hbm), dim3(64), 0, h->stream, h->ix, *opt, R, lists + np, list_n + 1, D[bwagpu_s::RS_KEYS].as<u8>(), (int)max_cap, D[bwagpu_s::RS_STAGE].as<u8>());
			HIPCHK(h, hipGetLastError());
		}
		hipLaunchKernelGGL(k_rescue_scan, dim3(1), dim3(256), 0, h->stream, d_acnt, n_reads, d_poff);
		HIPCHK(h, hipGetLastError());
		(void)hipEventRecord(h->ev[7], h->stream);
		HIPCHK(h, hipMemcpyAsync(&mtot, d_poff + n_reads, 8, hipMemcpyDeviceToHost, h->stream));
		HIPCHK(h, hipMemcpyAsync(counts, d_acnt, (size_t)n_reads * 4, hipMemcpyDeviceToHost, h->stream));
		HIPCHK(h, hipMemcpyAsync(res_rec.get(), R.out, (size_t)np * sizeof(bwagpu_rescue_t), hipMemcpyDeviceToHost, h->stream));
		HIPCHK(h, wait_stream(h));
		if (mtot < 0 || mtot > tot + extra) { h->err = "internal: merged lists larger than their arena"; return BWAGPU_EHIP; }
		for (int p = 0; p < np; ++p) if (res_rec[p].flags & 2) { h->err = "internal: a pair outgrew the rescue kernel's working lists"; return BWAGPU_EHIP; }
		if (D[bwagpu_s::RS_REGS].ensure((size_t)(mtot ? mtot : 1) * sizeof(bwagpu_alnreg_t)) || D[bwagpu_s::RS_SRC].ensure((size_t)(mtot ? mtot : 1) * 4)) { h->err = "hipMalloc failed (rescue)"; return BWAGPU_ENOMEM; }
		res_regs = result_block<bwagpu_alnreg_t>((size_t)mtot); res_src = result_block<int32_t>((size_t)mtot);
		if (!res_regs || !res_src) return BWAGPU_ENOMEM;
		nb = (n_reads + 3) / 4; if (nb > 8192) nb = 8192;
		(void)hipEventRecord(h->ev[0], h->stream);
		hipLaunchKernelGGL(k_rescue_pack, dim3(nb), dim3(BLOCK), 0, h->stream, R, n_reads, d_poff, D[bwagpu_s::RS_REGS].as<bwagpu_alnreg_t>(), D[bwagpu_s::RS_SRC].as<i32>());
		HIPCHK(h, hipGetLastError());
		(void)hipEventRecord(h->ev[1], h->stream);
		if (mtot) {
			HIPCHK(h, hipMemcpyAsync(res_regs.get(), D[bwagpu_s::RS_REGS].p, (size_t)mtot * sizeof(bwagpu_alnreg_t), hipMemcpyDeviceToHost, h->stream));
			HIPCHK(h, hipMemcpyAsync(res_src.get(), D[bwagpu_s::RS_SRC].p, (size_t)mtot * 4, hipMemcpyDeviceToHost, h->stream));
		}
		HIPCHK(h, wait_stream(h));
		{	// the kernels' segments between the call's host waits: count + scan, the task kernel, alignments + replay + scan, packing
			float a = 0.f, b = 0.f, c = 0.f, d = 0.f;
			(void)hipEventElapsedTime(&a, h->ev[2], h->ev[3]);
			if (extra) (void)hipEventElapsedTime(&b, h->ev[4], h->ev[5]);
			(void)hipEventElapsedTime(&c, h->ev[6], h->ev[7]);
			(void)hipEventElapsedTime(&d, h->ev[0], h->ev[1]);
			ms_resc = a + b + c + d;
		}
	}
	// marking and pairing of the merged lists: the kernels of bwagpu_batch_primary / bwagpu_batch_pair, pointed at the packed merged lists (k_rescue_pack's; on
	// the host the call's own results; the offsets stay on the device) under the ids of L
	RegLists M; M.n = n_reads; M.tot = mtot; M.d_ids = L.d_ids; M.id0 = L.id0; M.h_ids = L.h_ids; M.h_cnt = counts; M.h_regs = res_regs.get();
	M.d_cnt = h->d_rs[bwagpu_s::RS_ACNT].as<i32>(); M.d_off = h->d_rs[bwagpu_s::RS_POFF].as<i64>(); M.d_regs = h->d_rs[bwagpu_s::RS_REGS].as<bwagpu_alnreg_t>();
	for (int i = 0; i < n_reads; ++i) M.max_cnt = std::max(M.max_cnt, counts[i]);
	if (pri || pairs) {
		if (mtot == 0) { res_pri = result_block<bwagpu_primary_t>(0); if (!res_pri) return BWAGPU_ENOMEM; }
		else {
			bwagpu_primary_t *r = nullptr;
			const int rc = primary_run(h, opt, M, pri_log_need(counts, res_regs.get(), n_reads), &r, npri.data(), &ms_pri);
			if (rc != BWAGPU_OK) return rc;
			res_pri.reset(r);
		}
	}
	if (pairs) {
		if (mtot == 0) {
			res_pair = result_block<bwagpu_pair_t>((size_t)np);
			if (!res_pair) return BWAGPU_ENOMEM;
			for (int p = 0; p < np; ++p) res_pair[p] = pair_none();
		} else {
			PairSel S = { h->d_pri_npri.as<i32>(), npri.data(), h->d_pri_out.as<bwagpu_primary_t>(), res_pri.get(), nullptr, nullptr, L.id0 >> 1 };
			std::vector<i64> pid;
			if (L.h_ids) {      // a pair's id is its first read's id >> 1 (bwamem_pair.c:349-354)
				pid.resize((size_t)np);
				for (int p = 0; p < np; ++p) pid[(size_t)p] = L.h_ids[2 * (size_t)p] >> 1;
				if (h->d_rs[bwagpu_s::RS_PAIRIDS].ensure((size_t)np * 8)) { h->err = "hipMalloc failed (rescue)"; return BWAGPU_ENOMEM; }
				HIPCHK(h, hipMemcpyAsync(h->d_rs[bwagpu_s::RS_PAIRIDS].p, pid.data(), (size_t)np * 8, hipMemcpyHostToDevice, h->stream));
				HIPCHK(h, wait_stream(h));
				S.d_ids = h->d_rs[bwagpu_s::RS_PAIRIDS].as<i64>(); S.h_ids = pid.data();
			}
			bwagpu_pair_t *r = nullptr;
			const int rc = pair_run(h, opt, pes, M, S, &r, &ms_pair);
			if (rc != BWAGPU_OK) return rc;
			res_pair.reset(r);
		}
	}
	*regs = res_regs.release(); *src = res_src.release(); *n_regs = mtot; *rescue = res_rec.release();
	if (pri) *pri = res_pri.release();
	if (pairs) *pairs = res_pair.release();
	if (n_pri) memcpy(n_pri, npri.data(), (size_t)n_reads * 4);
	if (kernel_ms) *kernel_ms = ms_resc + ms_pri + ms_pair;
	if (ms_parts) { ms_parts[0] = ms_resc; ms_parts[1] = ms_pri; ms_parts[2] = ms_pair; }
	return BWAGPU_OK;
}

extern "C" int bwagpu_batch_rescue(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pestat_t pes[4], int64_t id0, int32_t *counts, bwagpu_alnreg_t **regs, int32_t **src, int64_t *n_regs,
								   bwagpu_rescue_t **rescue, bwagpu_primary_t **pri, int32_t *n_pri, bwagpu_pair_t **pairs, float *kernel_ms)
{
	if (!h || !opt || !pes || !h->ran || !h->downloaded || !regs || !src || !n_regs || !rescue || (h->n_reads > 0 && !counts)) return BWAGPU_EINVAL;
	if ((h->n_reads & 1) || (id0 & 1) || opt->e_del <= 0 || opt->e_ins <= 0 || (pairs && (opt->flag & 0x800 /* MEM_F_PRIMARY5 */))) return BWAGPU_EINVAL;
	const BusyGuard busy(h->ibuf->busy);
	HIPCHK(h, hipSetDevice(h->device));
	return rescue_run(h, opt, pes, lists_of_batch(h, id0), h->d_seq.as<u8>(), h->d_off.as<i64>(), counts, regs, src, n_regs, rescue, pri, n_pri, pairs, kernel_ms);
}

extern "C" int bwagpu_rescue_flat(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pestat_t pes[4], int n_pairs, const uint8_t *seqs, const int64_t *off, const int32_t *counts_in,
								  const bwagpu_alnreg_t *regs_in, const int64_t *ids, int32_t *counts, bwagpu_alnreg_t **regs, int32_t **src, int64_t *n_regs, bwagpu_rescue_t **rescue,
								  bwagpu_primary_t **pri, int32_t *n_pri, bwagpu_pair_t **pairs, float *kernel_ms)
{
	if (!h || !opt || !pes || n_pairs < 0 || n_pairs > 0x1fffffff || !regs || !src || !n_regs || !rescue) return BWAGPU_EINVAL;
	if (n_pairs > 0 && (!seqs || !off || !counts_in || !counts || ((pri || pairs) && !ids))) return BWAGPU_EINVAL;
	if (opt->e_del <= 0 || opt->e_ins <= 0 || (pairs && (opt->flag & 0x800 /* MEM_F_PRIMARY5 */))) return BWAGPU_EINVAL;
	FlatReads R; FlatLists F; RegLists L;
	if (!R.scan(h, "bwagpu_rescue_flat", 2 * (size_t)n_pairs, seqs, off) || !F.scan(h, 2 * (size_t)n_pairs, counts_in, regs_in, counts_in) || !R.codes_ok(h, "bwagpu_rescue_flat")) return BWAGPU_EINVAL;
	const BusyGuard busy(h->ibuf->busy);
	HIPCHK(h, hipSetDevice(h->device));
	if (int rc = R.upload(h, "rescue")) return rc;
	const int rc = F.upload(h, "rescue", counts_in, regs_in, ids, F.n, L);
	return rc != BWAGPU_OK ? rc : rescue_run(h, opt, pes, L, h->d_pf_seq.as<u8>(), h->d_pf_seqoff.as<i64>(), counts, regs, src, n_regs, rescue, pri, n_pri, pairs, kernel_ms);
}

// ---- insert-size statistics on the device (dev_pestat.h) ------------------------------------------------------------------------------------------
extern "C" void bwagpu_pestat_limits(int32_t out[2]) { out[0] = PST_MIN_DIR_CNT; out[1] = PST_MAX_INS; }

static i64 pestat_bins(int max_ins) { return max_ins >= 0 ? 4 * ((i64)max_ins + 1) : 0; }
static void pestat_none(bwagpu_pestat_t pes[4], bwagpu_pestat_info_t *info)      // no pair can qualify: :76 and :96-100 for every orientation
{
	memset(pes, 0, 4 * sizeof(bwagpu_pestat_t));
	for (int d = 0; d < 4; ++d) pes[d].failed = 1;
	if (info) memset(info, 0, sizeof *info);
}
static int pestat_max_ins_ok(bwagpu_t *h, const bwagpu_opt_t *opt)
{
	if (opt->max_ins <= PST_MAX_INS) return 1;
	h->err = "max_ins " + std::to_string(opt->max_ins) + " is beyond the device histogram's " + std::to_string(PST_MAX_INS) + " (bwagpu_pestat_limits): mem_pestat of this batch is the host's";
	return 0;
}
// k_pestat_collect over the L.n / 2 pairs of the lists L into the handle's histogram (cleared first), in the stream; 1 <= max_ins <= PST_MAX_INS
static int pestat_collect(bwagpu_t *h, const bwagpu_opt_t *opt, const RegLists &L)
{
	const size_t bytes = (size_t)pestat_bins(opt->max_ins) * 4;
	if (h->d_pst_hist.ensure(bytes)) { h->err = "hipMalloc failed (pestat)"; return BWAGPU_ENOMEM; }
	HIPCHK(h, hipMemsetAsync(h->d_pst_hist.p, 0, bytes, h->stream));
	const int n_pairs = L.n >> 1;
	if (n_pairs == 0) return BWAGPU_OK;
	int nb = (n_pairs + PST_BLOCK - 1) / PST_BLOCK; if (nb > 256 * 8) nb = 256 * 8;
	hipLaunchKernelGGL(k_pestat_collect, dim3(nb), dim3(PST_BLOCK), 0, h->stream, opt->mask_level, opt->min_seed_len * opt->a, opt->max_ins, h->l_pac, n_pairs, L.d_cnt, L.d_off, L.d_regs, h->d_pst_hist.as<unsigned int>());
	HIPCHK(h, hipGetLastError());
	return BWAGPU_OK;
}
// k_pestat_finish on the handle's histogram into its result buffer, in the stream
static int pestat_finish(bwagpu_t *h, const bwagpu_opt_t *opt)
{
	if (h->d_pst_out.ensure(sizeof(PstOut))) { h->err = "hipMalloc failed (pestat)"; return BWAGPU_ENOMEM; }
	HIPCHK(h, hipMemsetAsync(h->d_pst_out.p, 0, sizeof(PstOut), h->stream));
	hipLaunchKernelGGL(k_pestat_finish, dim3(1), dim3(PST_BLOCK), 0, h->stream, h->d_pst_hist.as<unsigned int>(), opt->max_ins, h->d_pst_out.as<PstOut>());
	HIPCHK(h, hipGetLastError());
	return BWAGPU_OK;
}
// the result buffer to the host: the call's one wait
static int pestat_fetch(bwagpu_t *h, bwagpu_pestat_t pes[4], bwagpu_pestat_info_t *info, float *kernel_ms)
{
	PstOut o;
	HIPCHK(h, hipMemcpyAsync(&o, h->d_pst_out.p, sizeof o, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(h, wait_stream(h));
	if (kernel_ms) (void)hipEventElapsedTime(kernel_ms, h->ev[0], h->ev[1]);
	for (int d = 0; d < 4; ++d) if (o.info.n[d] >= ((i64)1 << 31)) { h->err = "2^31 or more pairs in one orientation: beyond mem_pestat's int arithmetic"; return BWAGPU_EINVAL; }
	memcpy(pes, o.pes, sizeof o.pes);
	if (info) *info = o.info;
	return BWAGPU_OK;
}
// both kernels as one timed segment, then the fetch
static int pestat_run(bwagpu_t *h, const bwagpu_opt_t *opt, const RegLists &L, bwagpu_pestat_t pes[4], bwagpu_pestat_info_t *info, float *kernel_ms)
{
	(void)hipEventRecord(h->ev[0], h->stream);
	int rc = pestat_collect(h, opt, L);
	if (rc == BWAGPU_OK) rc = pestat_finish(h, opt);
	(void)hipEventRecord(h->ev[1], h->stream);
	return rc == BWAGPU_OK ? pestat_fetch(h, pes, info, kernel_ms) : rc;
}

extern "C" int bwagpu_batch_pestat(bwagpu_t *h, const bwagpu_opt_t *opt, bwagpu_pestat_t pes[4], bwagpu_pestat_info_t *info, float *kernel_ms)
{
	if (!h || !opt || !pes || !h->ran || !h->downloaded) return BWAGPU_EINVAL;
	if (!pestat_max_ins_ok(h, opt)) return BWAGPU_EINVAL;
	const BusyGuard busy(h->ibuf->busy);
	HIPCHK(h, hipSetDevice(h->device));
	if (kernel_ms) *kernel_ms = 0.f;
	if (h->packed_tot <= 0 || h->n_reads < 2 || opt->max_ins <= 0) { pestat_none(pes, info); return BWAGPU_OK; }      // (without a region the packed arrays may not exist)
	return pestat_run(h, opt, lists_of_batch(h, 0), pes, info, kernel_ms);
}

extern "C" int bwagpu_pestat_flat(bwagpu_t *h, const bwagpu_opt_t *opt, int n_reads, const int32_t *counts, const bwagpu_alnreg_t *regs,
								  bwagpu_pestat_t pes[4], bwagpu_pestat_info_t *info, float *kernel_ms)
{
	if (!h || !opt || !pes || n_reads < 0 || (n_reads > 0 && !counts)) return BWAGPU_EINVAL;
	FlatLists F; RegLists L;
	if (!F.scan(h, (size_t)n_reads, counts, regs, nullptr)) return BWAGPU_EINVAL;
	if (!pestat_max_ins_ok(h, opt)) return BWAGPU_EINVAL;
	const BusyGuard busy(h->ibuf->busy);
	HIPCHK(h, hipSetDevice(h->device));
	if (kernel_ms) *kernel_ms = 0.f;
	if (F.tot == 0 || n_reads < 2 || opt->max_ins <= 0) { pestat_none(pes, info); return BWAGPU_OK; }
	const int rc = F.upload(h, "pestat", counts, regs, nullptr, 0, L);
	return rc != BWAGPU_OK ? rc : pestat_run(h, opt, L, pes, info, kernel_ms);
}

extern "C" int bwagpu_batch_pestat_hist(bwagpu_t *h, const bwagpu_opt_t *opt, uint32_t **hist, int64_t *n_bins, float *kernel_ms)
{
	if (!h || !opt || !hist || !n_bins || !h->ran || !h->downloaded) return BWAGPU_EINVAL;
	if (!pestat_max_ins_ok(h, opt)) return BWAGPU_EINVAL;
	const BusyGuard busy(h->ibuf->busy);
	HIPCHK(h, hipSetDevice(h->device));
	if (kernel_ms) *kernel_ms = 0.f;
	const i64 nbins = pestat_bins(opt->max_ins);
	ResultBlock<uint32_t> res = result_block<uint32_t>((size_t)nbins);
	if (!res) return BWAGPU_ENOMEM;
	*hist = nullptr; *n_bins = 0;
	if (h->packed_tot <= 0 || h->n_reads < 2 || opt->max_ins <= 0) memset(res.get(), 0, (size_t)(nbins ? nbins : 1) * 4);      // nothing to count
	else {
		(void)hipEventRecord(h->ev[0], h->stream);
		const int rc = pestat_collect(h, opt, lists_of_batch(h, 0));
		(void)hipEventRecord(h->ev[1], h->stream);
		if (rc != BWAGPU_OK) return rc;
		HIPCHK(h, hipMemcpyAsync(res.get(), h->d_pst_hist.p, (size_t)nbins * 4, hipMemcpyDeviceToHost, h->stream));
		HIPCHK(h, wait_stream(h));
		if (kernel_ms) (void)hipEventElapsedTime(kernel_ms, h->ev[0], h->ev[1]);
	}
	*hist = res.release(); *n_bins = nbins;
	return BWAGPU_OK;
}

extern "C" int bwagpu_pestat_finish(bwagpu_t *h, const bwagpu_opt_t *opt, const uint32_t *hist, int64_t n_bins, bwagpu_pestat_t pes[4], bwagpu_pestat_info_t *info, float *kernel_ms)
{
	if (!h || !opt || !pes) return BWAGPU_EINVAL;
	if (!pestat_max_ins_ok(h, opt)) return BWAGPU_EINVAL;
	if (n_bins != pestat_bins(opt->max_ins) || (n_bins > 0 && !hist)) { h->err = "bwagpu_pestat_finish: the histogram does not have 4 * (max_ins + 1) bins"; return BWAGPU_EINVAL; }
	const BusyGuard busy(h->ibuf->busy);
	HIPCHK(h, hipSetDevice(h->device));
	if (kernel_ms) *kernel_ms = 0.f;
	if (opt->max_ins <= 0) { pestat_none(pes, info); return BWAGPU_OK; }
	if (h->d_pst_hist.ensure((size_t)n_bins * 4)) { h->err = "hipMalloc failed (pestat)"; return BWAGPU_ENOMEM; }
	HIPCHK(h, hipMemcpyAsync(h->d_pst_hist.p, hist, (size_t)n_bins * 4, hipMemcpyHostToDevice, h->stream));
	(void)hipEventRecord(h->ev[0], h->stream);
	const int rc = pestat_finish(h, opt);
	(void)hipEventRecord(h->ev[1], h->stream);
	return rc == BWAGPU_OK ? pestat_fetch(h, pes, info, kernel_ms) : rc;
}

// ---- the alignment list of every read on the device (dev_alns.h) -------------------------------------------------------------------------------------
extern "C" void bwagpu_alns_limits(int32_t out[2]) { out[0] = ALN_LANE_MAX; out[1] = ALN_STEP; }
extern "C" int bwagpu_aln_size(void) { return (int)sizeof(bwagpu_aln_t); }

// The kernels of both entry points on the lists L: the marking (primary_run: its records stay in d_pri_out), then k_alns_lane / k_alns_wave with the CIGAR
// records, operation array and read lengths of I (I.pri is set here).  resident (a caller that wants text, sam_run): the records of both stages stay in
// d_aln_out / d_pri_out and nothing comes to the host; the kernels of this stage run between ev[0] and ev[1], *kernel_ms is the marking's time alone.
static int alns_run(bwagpu_t *h, const bwagpu_opt_t *opt, const RegLists &L, i64 log_need, AlnIn I, bwagpu_aln_t **alns, int32_t *n_aln, bwagpu_primary_t **pri, int32_t *n_pri, float *kernel_ms,
					bool resident = false)
{
	const int n_reads = L.n;
	const i64 tot = L.tot;
	if (kernel_ms) *kernel_ms = 0.f;
	ResultBlock<bwagpu_aln_t> res = result_block<bwagpu_aln_t>(resident ? 0 : (size_t)tot);
	if (!res) return BWAGPU_ENOMEM;
	if (resident && (n_reads == 0 || tot == 0)) return BWAGPU_OK;
	if (n_reads == 0 || tot == 0) {
		ResultBlock<bwagpu_primary_t> none = result_block<bwagpu_primary_t>(0);
		if (!none) return BWAGPU_ENOMEM;
		for (int i = 0; i < n_reads; ++i) { if (n_aln) n_aln[i] = 0; if (n_pri) n_pri[i] = 0; }
		if (pri) *pri = none.release();
		*alns = res.release();
		return BWAGPU_OK;
	}
	bwagpu_primary_t *recs_ = nullptr;
	float ms_pri = 0.f, ms = 0.f;
	const int rc = primary_run(h, opt, L, log_need, &recs_, n_pri, &ms_pri, resident);
	if (rc != BWAGPU_OK) return rc;
	ResultBlock<bwagpu_primary_t> recs(recs_);
	if (h->d_aln_out.ensure((size_t)tot * sizeof(bwagpu_aln_t)) || h->d_aln_n.ensure((size_t)n_reads * 4) || h->d_aln_list.ensure((size_t)n_reads * 4) || h->d_aln_ctr.ensure(sizeof(unsigned int))) {
		h->err = "hipMalloc failed (alns)"; return BWAGPU_ENOMEM;
	}
	// a mapQ the host side of the marking had to compute (a logarithm outside the table) is not in the device's copy of the records yet
	bool any = false;
	for (i64 k = 0; !resident && k < tot && !any; ++k) any = (recs[k].flags & 1) != 0;
	if (any) HIPCHK(h, hipMemcpyAsync(h->d_pri_out.p, recs.get(), (size_t)tot * sizeof(bwagpu_primary_t), hipMemcpyHostToDevice, h->stream));
	HIPCHK(h, hipMemsetAsync(h->d_aln_ctr.p, 0, sizeof(unsigned int), h->stream));
	I.pri = h->d_pri_out.as<bwagpu_primary_t>();
	bwagpu_aln_t *d_out = h->d_aln_out.as<bwagpu_aln_t>();
	i32 *d_n = h->d_aln_n.as<i32>(), *list = h->d_aln_list.as<i32>();
	unsigned int *list_n = h->d_aln_ctr.as<unsigned int>();
	(void)hipEventRecord(h->ev[0], h->stream);
	int nb = (n_reads + ALN_LANE_BLOCK - 1) / ALN_LANE_BLOCK; if (nb > 256 * 12) nb = 256 * 12;
	hipLaunchKernelGGL(k_alns_lane, dim3(nb), dim3(ALN_LANE_BLOCK), 0, h->stream, h->ix, *opt, n_reads, L.d_cnt, L.d_off, L.d_regs, I, d_out, d_n, list, list_n);
	HIPCHK(h, hipGetLastError());
	if (L.max_cnt > ALN_LANE_MAX) {      // (the list's length stays on the device)
		hipLaunchKernelGGL(k_alns_wave, dim3(n_reads < 256 * 16 ? n_reads : 256 * 16), dim3(64), 0, h->stream, h->ix, *opt, L.d_cnt, L.d_off, L.d_regs, I, d_out, d_n, list, list_n);
		HIPCHK(h, hipGetLastError());
	}
	(void)hipEventRecord(h->ev[1], h->stream);
	if (resident) { if (kernel_ms) *kernel_ms = ms_pri; return BWAGPU_OK; }
	std::vector<i32> na((size_t)n_reads);
	HIPCHK(h, hipMemcpyAsync(res.get(), d_out, (size_t)tot * sizeof(bwagpu_aln_t), hipMemcpyDeviceToHost, h->stream));
	HIPCHK(h, hipMemcpyAsync(na.data(), d_n, (size_t)n_reads * 4, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(h, wait_stream(h));
	(void)hipEventElapsedTime(&ms, h->ev[0], h->ev[1]);
	if (kernel_ms) *kernel_ms = ms_pri + ms;
	if (n_aln) memcpy(n_aln, na.data(), (size_t)n_reads * 4);
	if (pri) *pri = recs.release();
	*alns = res.release();
	return BWAGPU_OK;
}

// the CIGAR records and operation array of the last bwagpu_batch_cigars, the batch's read offsets
static AlnIn alnin_of_batch(const bwagpu_t *h)
{
	AlnIn I = {}; I.cigs = h->d_cigs.as<bwagpu_cigar_t>(); I.ops = h->d_cig_ext.as<u32>(); I.n_ops = h->cig_ext_n; I.seq_off = h->d_off.as<i64>();
	return I;
}

extern "C" int bwagpu_batch_alns(bwagpu_t *h, const bwagpu_opt_t *opt, int64_t id0, bwagpu_aln_t **alns, int64_t *n_alns, int32_t *n_aln, bwagpu_primary_t **pri, int32_t *n_pri, float *kernel_ms)
{
	if (!h || !opt || !h->ran || !h->downloaded || h->cig_ext_n < 0 || !alns || !n_alns) return BWAGPU_EINVAL;
	if (opt->flag & 0x800 /* MEM_F_PRIMARY5 */) return BWAGPU_EINVAL;
	const BusyGuard busy(h->ibuf->busy);
	HIPCHK(h, hipSetDevice(h->device));
	*alns = nullptr; *n_alns = 0; if (pri) *pri = nullptr;
	const RegLists L = lists_of_batch(h, id0);
	const int rc = alns_run(h, opt, L, batch_log_need(h, opt), alnin_of_batch(h), alns, n_aln, pri, n_pri, kernel_ms);
	if (rc == BWAGPU_OK) *n_alns = L.tot;
	return rc;
}

// The CIGAR records of a *_flat call, one per region (tot in all), and the operation array of n_ops words they point into.  flat_cigs_ok(): an n_cigar of
// -1 .. 32768, operations -- and, with_md, MD strings -- that are kept in the array inside it; false: BWAGPU_EINVAL (`what` names the entry point in the text).
// flat_cigs_upload(): into d_aln_cigs / d_aln_ops and I, enqueued only: the wait is the caller's.
static bool flat_cigs_ok(bwagpu_t *h, const char *what, const bwagpu_cigar_t *cigs, i64 tot, i64 n_ops, bool with_md)
{
	if (tot > 0 && !cigs) return false;
	for (i64 k = 0; k < tot; ++k) {
		const bwagpu_cigar_t &c = cigs[k];
		if (c.n_cigar < -1 || c.n_cigar > 32768) { h->err = std::string(what) + ": n_cigar outside [-1, 32768]"; return false; }
		if (c.n_cigar > 6) {
			const u64 at = (u64)c.cigar[1] << 32 | c.cigar[0];
			if (at > (u64)n_ops || (u64)c.n_cigar > (u64)n_ops - at) { h->err = std::string(what) + ": a CIGAR record points outside the operation array"; return false; }
		}
		if (with_md && c.n_cigar >= 0 && (c.md_len < 0 || (c.md_len > 8 && (c.md > (u64)n_ops || ((u64)c.md_len + 3) / 4 > (u64)n_ops - c.md)))) {
			h->err = std::string(what) + ": an MD string outside the operation array"; return false;
		}
	}
	return true;
}
static int flat_cigs_upload(bwagpu_t *h, const char *tag, const bwagpu_cigar_t *cigs, i64 tot, const uint32_t *ops, i64 n_ops, AlnIn &I)
{
	if (h->d_aln_cigs.ensure((size_t)(tot ? tot : 1) * sizeof(bwagpu_cigar_t)) || h->d_aln_ops.ensure((size_t)(n_ops ? n_ops : 1) * 4)) { h->err = std::string("hipMalloc failed (") + tag + ")"; return BWAGPU_ENOMEM; }
	if (tot) HIPCHK(h, hipMemcpyAsync(h->d_aln_cigs.p, cigs, (size_t)tot * sizeof(bwagpu_cigar_t), hipMemcpyHostToDevice, h->stream));
	if (n_ops) HIPCHK(h, hipMemcpyAsync(h->d_aln_ops.p, ops, (size_t)n_ops * 4, hipMemcpyHostToDevice, h->stream));
	I.cigs = h->d_aln_cigs.as<bwagpu_cigar_t>(); I.ops = h->d_aln_ops.as<u32>();
	return BWAGPU_OK;
}

extern "C" int bwagpu_alns_flat(bwagpu_t *h, const bwagpu_opt_t *opt, int n_reads, const int32_t *counts, const bwagpu_alnreg_t *regs, const int64_t *ids, const int32_t *read_len,
								const bwagpu_cigar_t *cigs, const uint32_t *ops, int64_t n_ops, bwagpu_aln_t **alns, int32_t *n_aln, bwagpu_primary_t **pri, int32_t *n_pri, float *kernel_ms)
{
	if (!h || !opt || n_reads < 0 || !alns || n_ops < 0 || (n_ops > 0 && !ops) || (n_reads > 0 && (!counts || !ids || !read_len))) return BWAGPU_EINVAL;
	if (opt->flag & 0x800 /* MEM_F_PRIMARY5 */) return BWAGPU_EINVAL;
	FlatLists F; RegLists L;
	if (!F.scan(h, (size_t)n_reads, counts, regs, counts)) return BWAGPU_EINVAL;
	for (int i = 0; i < n_reads; ++i) if (read_len[i] < 0) return BWAGPU_EINVAL;
	if (!flat_cigs_ok(h, "bwagpu_alns_flat", cigs, F.tot, n_ops, false)) return BWAGPU_EINVAL;
	const BusyGuard busy(h->ibuf->busy);
	HIPCHK(h, hipSetDevice(h->device));
	*alns = nullptr; if (pri) *pri = nullptr;
	if (int rc = F.upload(h, "alns", counts, regs, ids, (size_t)n_reads, L)) return rc;
	AlnIn I = {}; I.n_ops = n_ops;
	if (F.tot > 0) {
		if (int rc = flat_cigs_upload(h, "alns", cigs, F.tot, ops, n_ops, I)) return rc;
		if (h->d_aln_len.ensure((size_t)n_reads * 4)) { h->err = "hipMalloc failed (alns)"; return BWAGPU_ENOMEM; }
		HIPCHK(h, hipMemcpyAsync(h->d_aln_len.p, read_len, (size_t)n_reads * 4, hipMemcpyHostToDevice, h->stream));
		HIPCHK(h, wait_stream(h));      // (the caller's arrays are pageable: the copies are done when they return, the wait keeps that independent of the runtime)
		I.read_len = h->d_aln_len.as<i32>();
	}
	return alns_run(h, opt, L, pri_log_need(counts, regs, n_reads), I, alns, n_aln, pri, n_pri, kernel_ms);
}

// ---- single-end SAM text on the device (dev_samtext.h) ------------------------------------------------------------------------------------------------
extern "C" void bwagpu_sam_limits(int32_t out[2]) { out[0] = SAM_STAGE; out[1] = SAM_STEP; }

// what both entry points require of the caller's names, comments and of the handle
static int sam_in_check(bwagpu_t *h, int n_reads, const bwagpu_sam_in_t *in, const char *what)
{
	if (!h->ibuf->have_names) { h->err = std::string(what) + ": the handle has no contig names (bwagpu_set_contig_names)"; return BWAGPU_EINVAL; }
	if (n_reads > 0 && (!in->names || !in->name_off || (in->comments && !in->comment_off))) return BWAGPU_EINVAL;
	for (int i = 0; i < n_reads; ++i)
		if (in->name_off[0] < 0 || in->name_off[i] > in->name_off[i + 1] || (in->comments && (in->comment_off[0] < 0 || in->comment_off[i] > in->comment_off[i + 1]))) {
			h->err = std::string(what) + ": offsets that do not ascend"; return BWAGPU_EINVAL;
		}
	return BWAGPU_OK;
}

// the text of a call without reads
static int sam_none(bwagpu_sam_out_t *out)
{
	ResultBlock<i64> off = result_block<i64>(1);
	ResultBlock<i32> flags = result_block<i32>(0), lines = result_block<i32>(0);
	ResultBlock<char> text = result_block<char>(0);
	if (!off || !flags || !lines || !text) return BWAGPU_ENOMEM;
	off[0] = 0;
	out->text = text.release(); out->off = off.release(); out->flags = flags.release(); out->n_lines = lines.release();
	return BWAGPU_OK;
}

// The names, qualities and comments of n > 0 reads (n_bases bases in all) and -R's id go to the device; S gets them and the handle's contig names.  Also sizes
// the per-read arrays of sam_passes.
static int sam_upload(bwagpu_t *h, int n, i64 n_bases, const bwagpu_sam_in_t *in, SamIn &S)
{
	DevBuf *B = h->d_st;
	const size_t n_names = (size_t)in->name_off[n], n_comm = in->comments ? (size_t)in->comment_off[n] : 0, n_rg = in->rg_id ? strlen(in->rg_id) : 0;
	if (B[bwagpu_s::ST_NAMES].ensure(n_names + 1) || B[bwagpu_s::ST_NAMEOFF].ensure(((size_t)n + 1) * 8) || (in->quals && B[bwagpu_s::ST_QUAL].ensure((size_t)n_bases + 1)) ||
		(in->comments && (B[bwagpu_s::ST_COMM].ensure(n_comm + 1) || B[bwagpu_s::ST_COMMOFF].ensure(((size_t)n + 1) * 8))) || B[bwagpu_s::ST_RG].ensure(n_rg + 1) ||
		B[bwagpu_s::ST_SIZE].ensure((size_t)n * 4) || B[bwagpu_s::ST_TOFF].ensure(((size_t)n + 1) * 8) || B[bwagpu_s::ST_FLAGS].ensure((size_t)n * 4) || B[bwagpu_s::ST_LINES].ensure((size_t)n * 4)) {
		h->err = "hipMalloc failed (sam)"; return BWAGPU_ENOMEM;
	}
	if (n_names) HIPCHK(h, hipMemcpyAsync(B[bwagpu_s::ST_NAMES].p, in->names, n_names, hipMemcpyHostToDevice, h->stream));
	HIPCHK(h, hipMemcpyAsync(B[bwagpu_s::ST_NAMEOFF].p, in->name_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, h->stream));
	if (in->quals && n_bases) HIPCHK(h, hipMemcpyAsync(B[bwagpu_s::ST_QUAL].p, in->quals, (size_t)n_bases, hipMemcpyHostToDevice, h->stream));
	if (in->comments) {
		if (n_comm) HIPCHK(h, hipMemcpyAsync(B[bwagpu_s::ST_COMM].p, in->comments, n_comm, hipMemcpyHostToDevice, h->stream));
		HIPCHK(h, hipMemcpyAsync(B[bwagpu_s::ST_COMMOFF].p, in->comment_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, h->stream));
	}
	if (n_rg) HIPCHK(h, hipMemcpyAsync(B[bwagpu_s::ST_RG].p, in->rg_id, n_rg, hipMemcpyHostToDevice, h->stream));
	S.names = B[bwagpu_s::ST_NAMES].as<char>(); S.name_off = B[bwagpu_s::ST_NAMEOFF].as<i64>();
	S.quals = in->quals ? B[bwagpu_s::ST_QUAL].as<char>() : nullptr;
	S.comments = in->comments ? B[bwagpu_s::ST_COMM].as<char>() : nullptr; S.comment_off = in->comments ? B[bwagpu_s::ST_COMMOFF].as<i64>() : nullptr;
	S.rg = B[bwagpu_s::ST_RG].as<char>(); S.rg_len = (int)n_rg;
	S.ctg_text = h->ibuf->d_ctg_text.as<char>(); S.ctg_name_off = h->ibuf->d_ctg_toff.as<i64>(); S.ctg_anno_off = S.ctg_name_off + h->n_seqs + 1;
	S.extra_flag = in->extra_flag;
	return BWAGPU_OK;
}

// The two passes of the formatter on n > 0 reads whose lists are d_cnt / d_off and whose records S names, and the final copies; d_sampe: the pair records of
// a paired-end call (the kernels of dev_samtext_pe.h), or null.  e: the four events the passes run between (kernel_ms[1], [2]).  Host waits: one for the
// total size, one for the final copies.
static int sam_passes(bwagpu_t *h, const bwagpu_opt_t *opt, int n, const i32 *d_cnt, const i64 *d_off, const SamIn &S, const bwagpu_sampe_t *d_sampe, const int e[4], bwagpu_sam_out_t *out)
{
	DevBuf *B = h->d_st;
	ResultBlock<i64> off = result_block<i64>((size_t)n + 1);
	ResultBlock<i32> flags = result_block<i32>((size_t)n), lines = result_block<i32>((size_t)n);
	if (!off || !flags || !lines) return BWAGPU_ENOMEM;
	i32 *d_size = B[bwagpu_s::ST_SIZE].as<i32>(), *d_flags = B[bwagpu_s::ST_FLAGS].as<i32>(), *d_lines = B[bwagpu_s::ST_LINES].as<i32>();
	i64 *d_toff = B[bwagpu_s::ST_TOFF].as<i64>();
	const int nb = n < 256 * 16 ? n : 256 * 16;
	(void)hipEventRecord(h->ev[e[0]], h->stream);
	if (d_sampe) hipLaunchKernelGGL(k_sam_pe_size, dim3(nb), dim3(64), 0, h->stream, *opt, n, d_cnt, d_off, S, d_sampe, d_size, d_flags, d_lines);
	else hipLaunchKernelGGL(k_sam_size, dim3(nb), dim3(64), 0, h->stream, *opt, n, d_cnt, d_off, S, d_size, d_flags, d_lines);
	HIPCHK(h, hipGetLastError());
	hipLaunchKernelGGL(k_rescue_scan, dim3(1), dim3(256), 0, h->stream, d_size, n, d_toff);
	HIPCHK(h, hipGetLastError());
	(void)hipEventRecord(h->ev[e[1]], h->stream);
	i64 total = 0;
	HIPCHK(h, hipMemcpyAsync(&total, d_toff + n, 8, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(h, wait_stream(h));
	if (total < 0) { h->err = "internal: a negative text size"; return BWAGPU_EHIP; }
	ResultBlock<char> text = result_block<char>((size_t)total);
	if (!text) return BWAGPU_ENOMEM;
	if (B[bwagpu_s::ST_TEXT].ensure((size_t)total + 1)) { h->err = "hipMalloc failed (sam)"; return BWAGPU_ENOMEM; }
	(void)hipEventRecord(h->ev[e[2]], h->stream);
	if (d_sampe) hipLaunchKernelGGL(k_sam_pe_write, dim3(nb), dim3(64), 0, h->stream, *opt, n, d_cnt, d_off, S, d_sampe, d_toff, d_flags, B[bwagpu_s::ST_TEXT].as<char>());
	else hipLaunchKernelGGL(k_sam_write, dim3(nb), dim3(64), 0, h->stream, *opt, n, d_cnt, d_off, S, d_toff, d_flags, B[bwagpu_s::ST_TEXT].as<char>());
	HIPCHK(h, hipGetLastError());
	(void)hipEventRecord(h->ev[e[3]], h->stream);
	if (total) HIPCHK(h, hipMemcpyAsync(text.get(), B[bwagpu_s::ST_TEXT].p, (size_t)total, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(h, hipMemcpyAsync(off.get(), d_toff, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(h, hipMemcpyAsync(flags.get(), d_flags, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(h, hipMemcpyAsync(lines.get(), d_lines, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
	HIPCHK(h, wait_stream(h));
	(void)hipEventElapsedTime(&out->kernel_ms[1], h->ev[e[0]], h->ev[e[1]]);
	(void)hipEventElapsedTime(&out->kernel_ms[2], h->ev[e[2]], h->ev[e[3]]);
	for (int i = 0; i < n; ++i) out->n_declined += flags[i] & 1;
	out->n_text = total;
	out->text = text.release(); out->off = off.release(); out->flags = flags.release(); out->n_lines = lines.release();
	return BWAGPU_OK;
}

// The kernels of both entry points on the lists L of reads d_seq / d_seqoff (n_bases in all): alns_run with its records left on the device, then the two
// passes of the formatter.  Host waits: the marking's, one for the total size, one for the final copies.
static int sam_run(bwagpu_t *h, const bwagpu_opt_t *opt, const RegLists &L, i64 log_need, AlnIn I, const u8 *d_seq, const i64 *d_seqoff, i64 n_bases, const bwagpu_sam_in_t *in, bwagpu_sam_out_t *out)
{
	if (L.n == 0) return sam_none(out);
	SamIn S = {};
	if (int rc = sam_upload(h, L.n, n_bases, in, S)) return rc;
	float ms_pri = 0.f, ms = 0.f;
	const int rc = alns_run(h, opt, L, log_need, I, nullptr, nullptr, nullptr, nullptr, &ms_pri, true);
	if (rc != BWAGPU_OK) return rc;
	S.alns = h->d_aln_out.as<bwagpu_aln_t>(); S.pri = h->d_pri_out.as<bwagpu_primary_t>(); S.cigs = I.cigs; S.ops = I.ops;
	S.seq = d_seq; S.seq_off = d_seqoff;
	const int e[4] = { 2, 3, 4, 5 };
	const int rcp = sam_passes(h, opt, L.n, L.d_cnt, L.d_off, S, nullptr, e, out);
	if (rcp != BWAGPU_OK) return rcp;
	if (L.tot > 0) (void)hipEventElapsedTime(&ms, h->ev[0], h->ev[1]);
	out->kernel_ms[0] = ms_pri + ms;
	return BWAGPU_OK;
}

extern "C" int bwagpu_batch_sam(bwagpu_t *h, const bwagpu_opt_t *opt, int64_t id0, const bwagpu_sam_in_t *in, bwagpu_sam_out_t *out)
{
	if (!h || !opt || !h->ran || !h->downloaded || h->cig_ext_n < 0 || !in || !out) return BWAGPU_EINVAL;
	if (opt->flag & 0x800 /* MEM_F_PRIMARY5 */) return BWAGPU_EINVAL;
	memset(out, 0, sizeof *out);
	if (int rc = sam_in_check(h, h->n_reads, in, "bwagpu_batch_sam")) return rc;
	const BusyGuard busy(h->ibuf->busy);
	HIPCHK(h, hipSetDevice(h->device));
	return sam_run(h, opt, lists_of_batch(h, id0), batch_log_need(h, opt), alnin_of_batch(h), h->d_seq.as<u8>(), h->d_off.as<i64>(), h->n_bases, in, out);
}

extern "C" int bwagpu_sam_flat(bwagpu_t *h, const bwagpu_opt_t *opt, int n_reads, const uint8_t *seqs, const int64_t *seq_off, const int32_t *counts, const bwagpu_alnreg_t *regs,
							   const int64_t *ids, const bwagpu_cigar_t *cigs, const uint32_t *ops, int64_t n_ops, const bwagpu_sam_in_t *in, bwagpu_sam_out_t *out)
{
	if (!h || !opt || n_reads < 0 || !in || !out || n_ops < 0 || (n_ops > 0 && !ops) || (n_reads > 0 && (!counts || !ids || !seq_off))) return BWAGPU_EINVAL;
	if (opt->flag & 0x800 /* MEM_F_PRIMARY5 */) return BWAGPU_EINVAL;
	memset(out, 0, sizeof *out);
	if (int rc = sam_in_check(h, n_reads, in, "bwagpu_sam_flat")) return rc;
	FlatLists F; RegLists L;
	if (!F.scan(h, (size_t)n_reads, counts, regs, counts)) return BWAGPU_EINVAL;
	FlatReads R;      // (no codes_ok(): the formatter has a character for every code, sam_base in dev_samtext.h)
	if (!R.scan(h, "bwagpu_sam_flat", (size_t)n_reads, seqs, seq_off) || (R.first != 0 && !R.bad_offsets(h, "bwagpu_sam_flat"))) return BWAGPU_EINVAL;      // R.first: this call's reads begin at seqs[0] (the pair calls take any first offset)
	if (!flat_cigs_ok(h, "bwagpu_sam_flat", cigs, F.tot, n_ops, true)) return BWAGPU_EINVAL;
	const BusyGuard busy(h->ibuf->busy);
	HIPCHK(h, hipSetDevice(h->device));
	if (int rc = R.upload(h, "sam")) return rc;
	if (int rc = F.upload(h, "sam", counts, regs, ids, (size_t)n_reads, L)) return rc;
	AlnIn I = {}; I.n_ops = n_ops;
	if (n_reads > 0) {
		if (int rc = flat_cigs_upload(h, "sam", cigs, F.tot, ops, n_ops, I)) return rc;
		HIPCHK(h, wait_stream(h));      // (the caller's arrays are pageable, as in bwagpu_alns_flat)
		I.seq_off = h->d_pf_seqoff.as<i64>();
	}
	return sam_run(h, opt, L, pri_log_need(counts, regs, n_reads), I, h->d_pf_seq.as<u8>(), h->d_pf_seqoff.as<i64>(), R.n_bases, in, out);
}

// ---- a read pair decided on the device (dev_sampe.h) ----------------------------------------------------------------------------------------------------
extern "C" void bwagpu_sampe_limits(int32_t out[2]) { out[0] = SAMPE_LANE_MAX; out[1] = SAMPE_STEP; }
extern "C" int bwagpu_sampe_size(void) { return (int)sizeof(bwagpu_sampe_t); }

// The kernels of both entry points on the L.n = 2 n_pairs reads of the lists L (sequences d_seq / d_seqoff, the longest of max_len bases, n_bases in all):
// rescue_run with marking and pairing; the decision kernels on its resident records; the CIGAR kernels on the merged lists; the alignment lists from the patched
// marking records.  Host waits: rescue_run's, cigars_run's, one for the final copies.  resident (a caller that wants text and no records, sam_pe_run): alignment
// records, patched marking records and operation array stay in d_aln_out / d_pri_out / d_sp and do not come to the host -- out->alns, out->ops are empty, out->pri is
// rescue_run's, n_aln and the path-1 n_aa are not filled, there is no final wait and kernel_ms[5] is the caller's to read from ev[5], ev[6] behind a wait of its own.
static int sampe_run(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pestat_t pes[4], const RegLists &L, const u8 *d_seq, const i64 *d_seqoff, int max_len, i64 n_bases, int32_t *counts,
					 bwagpu_pe_out_t *out, bool resident = false)
{
	const int n_reads = L.n, np = n_reads / 2;
	// MEM_F_NO_RESCUE is 0x20 (bwamem.h:44); k_rescue_count reads bit 0x8 for it, so this call hands it the bit where the reference would look
	bwagpu_opt_t oc = *opt; oc.flag = (opt->flag & ~0x8) | ((opt->flag & 0x20) ? 0x8 : 0);
	ResultBlock<int32_t> res_npri = result_block<int32_t>((size_t)n_reads), res_naln = result_block<int32_t>((size_t)n_reads);
	ResultBlock<bwagpu_sampe_t> res_s = result_block<bwagpu_sampe_t>((size_t)np);
	if (!res_npri || !res_naln || !res_s) return BWAGPU_ENOMEM;
	bwagpu_alnreg_t *regs_ = nullptr; int32_t *src_ = nullptr; int64_t mtot = 0; bwagpu_rescue_t *resc_ = nullptr; bwagpu_primary_t *pri_ = nullptr; bwagpu_pair_t *pairs_ = nullptr;
	float ms[6] = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
	const int rc = rescue_run(h, opt, pes, L, d_seq, d_seqoff, counts, &regs_, &src_, &mtot, &resc_, &pri_, res_npri.get(), &pairs_, nullptr, &oc, ms);
	if (rc != BWAGPU_OK) return rc;
	ResultBlock<bwagpu_alnreg_t> res_regs(regs_); ResultBlock<int32_t> res_src(src_); ResultBlock<bwagpu_rescue_t> res_resc(resc_); ResultBlock<bwagpu_primary_t> res_pri(pri_);
	ResultBlock<bwagpu_pair_t> res_pairs(pairs_);
	ResultBlock<bwagpu_cigar_t> res_cigs = result_block<bwagpu_cigar_t>((size_t)mtot);
	ResultBlock<bwagpu_aln_t> res_alns = result_block<bwagpu_aln_t>(resident ? 0 : (size_t)mtot);
	ResultBlock<uint32_t> res_ops;
	if (!res_cigs || !res_alns) return BWAGPU_ENOMEM;
	i64 ext_n = 0;
	if (mtot == 0) {      // no region in the whole batch: every pair prints two unmapped records (and the device arrays may not exist)
		for (int p = 0; p < np; ++p) {
			bwagpu_sampe_t &s = res_s[p];
			memset(&s, 0, sizeof s);
			s.path = 1; s.why = (opt->flag & 0x4 /* MEM_F_NOPAIRING */) ? 1 : 2; s.extra_flag = 1; s.z[0] = s.z[1] = -1; s.alt[0] = s.alt[1] = -1;
		}
		for (int i = 0; i < n_reads; ++i) res_naln[i] = 0;
		res_ops = result_block<uint32_t>(0);
		if (!res_ops) return BWAGPU_ENOMEM;
	} else {
		// records the host side of the marking or of the pairing computed are not in the device's copies yet
		bool any_pri = false, any_pair = false;
		for (i64 k = 0; k < mtot && !any_pri; ++k) any_pri = (res_pri[k].flags & 1) != 0;
		for (int p = 0; p < np && !any_pair; ++p) any_pair = (res_pairs[p].flags & 1) != 0;
		if (any_pri) HIPCHK(h, hipMemcpyAsync(h->d_pri_out.p, res_pri.get(), (size_t)mtot * sizeof(bwagpu_primary_t), hipMemcpyHostToDevice, h->stream));
		if (any_pair) HIPCHK(h, hipMemcpyAsync(h->d_pair_out.p, res_pairs.get(), (size_t)np * sizeof(bwagpu_pair_t), hipMemcpyHostToDevice, h->stream));
		DevBuf *S = h->d_sp, *D = h->d_rs;
		if (S[bwagpu_s::SP_OUT].ensure((size_t)np * sizeof(bwagpu_sampe_t)) || S[bwagpu_s::SP_LIST].ensure((size_t)np * 4) || S[bwagpu_s::SP_CTR].ensure(sizeof(unsigned int)) ||
			S[bwagpu_s::SP_READ].ensure((size_t)mtot * 4)) { h->err = "hipMalloc failed (sampe)"; return BWAGPU_ENOMEM; }
		int max_cnt = 0;
		for (int i = 0; i < n_reads; ++i) max_cnt = std::max(max_cnt, counts[i]);
		SampeWin Wn;
		for (int d = 0; d < 4; ++d) { Wn.low[d] = pes[d].low; Wn.high[d] = pes[d].high; Wn.failed[d] = pes[d].failed; }
		i64 log_n = h->pri_log_dev;      // the marking's table, as the marking of this call used it
		if (h->cfg.pri_log_cap > 0 && h->cfg.pri_log_cap < log_n) log_n = h->cfg.pri_log_cap;
		const PriLogTab lg = { h->d_pri_log.as<double>(), (int)log_n };
		SampeIn I;
		I.cnt = D[bwagpu_s::RS_ACNT].as<i32>(); I.off = D[bwagpu_s::RS_POFF].as<i64>(); I.regs = D[bwagpu_s::RS_REGS].as<bwagpu_alnreg_t>();
		I.pri = h->d_pri_out.as<bwagpu_primary_t>(); I.npri = h->d_pri_npri.as<i32>(); I.pairs = h->d_pair_out.as<bwagpu_pair_t>(); I.resc = D[bwagpu_s::RS_OUT].as<bwagpu_rescue_t>();
		bwagpu_sampe_t *d_s = S[bwagpu_s::SP_OUT].as<bwagpu_sampe_t>();
		i32 *list = S[bwagpu_s::SP_LIST].as<i32>();
		unsigned int *list_n = S[bwagpu_s::SP_CTR].as<unsigned int>();
		HIPCHK(h, hipMemsetAsync(list_n, 0, sizeof(unsigned int), h->stream));
		(void)hipEventRecord(h->ev[3], h->stream);
		int nb = (np + SAMPE_LANE_BLOCK - 1) / SAMPE_LANE_BLOCK; if (nb > 256 * 12) nb = 256 * 12;
		hipLaunchKernelGGL(k_sampe_lane, dim3(nb), dim3(SAMPE_LANE_BLOCK), 0, h->stream, h->ix, *opt, Wn, lg, I, np, d_s, list, list_n);
		HIPCHK(h, hipGetLastError());
		if (max_cnt > SAMPE_LANE_MAX) {      // (the list's length stays on the device)
			hipLaunchKernelGGL(k_sampe_wave, dim3(np < 256 * 16 ? np : 256 * 16), dim3(64), 0, h->stream, h->ix, *opt, Wn, lg, I, d_s, list, list_n);
			HIPCHK(h, hipGetLastError());
		}
		(void)hipEventRecord(h->ev[4], h->stream);
		nb = (n_reads + 3) / 4; if (nb > 8192) nb = 8192;
		hipLaunchKernelGGL(k_sampe_reg_read, dim3(nb), dim3(BLOCK), 0, h->stream, n_reads, I.cnt, I.off, S[bwagpu_s::SP_READ].as<i32>());
		HIPCHK(h, hipGetLastError());
		HIPCHK(h, hipMemcpyAsync(res_s.get(), d_s, (size_t)np * sizeof(bwagpu_sampe_t), hipMemcpyDeviceToHost, h->stream));      // (there after cigars_run's first wait)
		// CIGAR records of every merged region
		const CigLists C = { mtot, I.regs, S[bwagpu_s::SP_READ].as<i32>(), I.off, d_seq, d_seqoff, n_reads, max_len, n_bases, &S[bwagpu_s::SP_CIGS], &S[bwagpu_s::SP_EXT] };
		float msc[2] = { 0.f, 0.f };
		const int rcc = cigars_run(h, opt, C, res_cigs.get(), &ext_n, msc);
		if (rcc != BWAGPU_OK) return rcc;
		ms[4] = msc[0];
		(void)hipEventElapsedTime(&ms[3], h->ev[3], h->ev[4]);
		res_ops = result_block<uint32_t>(resident ? 0 : (size_t)ext_n);
		if (!res_ops) return BWAGPU_ENOMEM;
		// pairs that met a logarithm outside the table: the same statements with the host's log(), on the call's own copies; their records go back to the device
		std::vector<i64> hoff;
		for (int p = 0; p < np; ++p) {
			bwagpu_sampe_t &s = res_s[p];
			if (!(s.path == 0 && s.extra_flag == 0 && (s.flags & 2))) continue;
			if (hoff.empty()) { hoff.resize((size_t)n_reads + 1); hoff[0] = 0; for (int i = 0; i < n_reads; ++i) hoff[(size_t)i + 1] = hoff[(size_t)i] + counts[i]; }
			const int r0 = 2 * p, r1 = r0 + 1;
			const i64 o0 = hoff[(size_t)r0], o1 = hoff[(size_t)r1];
			sampe_host_pair0(*opt, res_regs.get() + o0, res_pri.get() + o0, counts[r0], res_npri[r0], res_regs.get() + o1, res_pri.get() + o1, counts[r1], res_npri[r1], res_pairs[p], s);
			HIPCHK(h, hipMemcpyAsync(I.pri + o0, res_pri.get() + o0, (size_t)(counts[r0] + counts[r1]) * sizeof(bwagpu_primary_t), hipMemcpyHostToDevice, h->stream));
			HIPCHK(h, hipMemcpyAsync(d_s + p, &s, sizeof s, hipMemcpyHostToDevice, h->stream));
		}
		// the alignment lists
		if (h->d_aln_out.ensure((size_t)mtot * sizeof(bwagpu_aln_t)) || h->d_aln_n.ensure((size_t)n_reads * 4) || h->d_aln_list.ensure((size_t)n_reads * 4) || h->d_aln_ctr.ensure(sizeof(unsigned int))) {
			h->err = "hipMalloc failed (sampe)"; return BWAGPU_ENOMEM;
		}
		AlnIn A = {}; A.pri = I.pri; A.cigs = S[bwagpu_s::SP_CIGS].as<bwagpu_cigar_t>(); A.ops = S[bwagpu_s::SP_EXT].as<u32>(); A.n_ops = ext_n; A.seq_off = d_seqoff;
		bwagpu_aln_t *d_out = h->d_aln_out.as<bwagpu_aln_t>();
		i32 *d_n = h->d_aln_n.as<i32>(), *alist = h->d_aln_list.as<i32>();
		unsigned int *alist_n = h->d_aln_ctr.as<unsigned int>();
		HIPCHK(h, hipMemsetAsync(alist_n, 0, sizeof(unsigned int), h->stream));
		(void)hipEventRecord(h->ev[5], h->stream);
		nb = (n_reads + ALN_LANE_BLOCK - 1) / ALN_LANE_BLOCK; if (nb > 256 * 12) nb = 256 * 12;
		hipLaunchKernelGGL(k_alns_pe_lane, dim3(nb), dim3(ALN_LANE_BLOCK), 0, h->stream, h->ix, *opt, n_reads, I.cnt, I.off, I.regs, A, d_s, d_out, d_n, alist, alist_n);
		HIPCHK(h, hipGetLastError());
		if (max_cnt > ALN_LANE_MAX) {
			hipLaunchKernelGGL(k_alns_pe_wave, dim3(n_reads < 256 * 16 ? n_reads : 256 * 16), dim3(64), 0, h->stream, h->ix, *opt, I.cnt, I.off, I.regs, A, d_s, d_out, d_n, alist, alist_n);
			HIPCHK(h, hipGetLastError());
		}
		(void)hipEventRecord(h->ev[6], h->stream);
		if (!resident) {
			HIPCHK(h, hipMemcpyAsync(res_alns.get(), d_out, (size_t)mtot * sizeof(bwagpu_aln_t), hipMemcpyDeviceToHost, h->stream));
			HIPCHK(h, hipMemcpyAsync(res_naln.get(), d_n, (size_t)n_reads * 4, hipMemcpyDeviceToHost, h->stream));
			HIPCHK(h, hipMemcpyAsync(res_pri.get(), I.pri, (size_t)mtot * sizeof(bwagpu_primary_t), hipMemcpyDeviceToHost, h->stream));      // (as the decision kernels left them)
			if (ext_n) HIPCHK(h, hipMemcpyAsync(res_ops.get(), S[bwagpu_s::SP_EXT].p, (size_t)ext_n * 4, hipMemcpyDeviceToHost, h->stream));
			HIPCHK(h, wait_stream(h));
			(void)hipEventElapsedTime(&ms[5], h->ev[5], h->ev[6]);
			for (int p = 0; p < np; ++p) if (res_s[p].path == 1) { res_s[p].n_aa[0] = res_naln[2 * (size_t)p]; res_s[p].n_aa[1] = res_naln[2 * (size_t)p + 1]; }
		}
	}
	out->regs = res_regs.release(); out->src = res_src.release(); out->n_regs = mtot; out->rescue = res_resc.release(); out->pri = res_pri.release(); out->n_pri = res_npri.release();
	out->pairs = res_pairs.release(); out->sampe = res_s.release(); out->cigs = res_cigs.release(); out->ops = res_ops.release(); out->n_ops = ext_n; out->alns = res_alns.release();
	out->n_aln = res_naln.release();
	memcpy(out->kernel_ms, ms, sizeof ms);
	return BWAGPU_OK;
}

extern "C" int bwagpu_batch_sampe(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pestat_t pes[4], int64_t id0, int32_t *counts, bwagpu_pe_out_t *out)
{
	if (out) memset(out, 0, sizeof *out);
	if (!h || !opt || !pes || !h->ran || !h->downloaded || !out || (h->n_reads > 0 && !counts)) return BWAGPU_EINVAL;
	if ((h->n_reads & 1) || (id0 & 1) || opt->e_del <= 0 || opt->e_ins <= 0 || (opt->flag & 0x800 /* MEM_F_PRIMARY5 */)) return BWAGPU_EINVAL;
	const BusyGuard busy(h->ibuf->busy);
	HIPCHK(h, hipSetDevice(h->device));
	return sampe_run(h, opt, pes, lists_of_batch(h, id0), h->d_seq.as<u8>(), h->d_off.as<i64>(), h->max_len, h->n_bases, counts, out);
}

extern "C" int bwagpu_sampe_flat(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pestat_t pes[4], int n_pairs, const uint8_t *seqs, const int64_t *off, const int32_t *counts_in,
								 const bwagpu_alnreg_t *regs_in, const int64_t *ids, int32_t *counts, bwagpu_pe_out_t *out)
{
	if (out) memset(out, 0, sizeof *out);
	if (!h || !opt || !pes || n_pairs < 0 || n_pairs > 0x1fffffff || !out) return BWAGPU_EINVAL;
	if (n_pairs > 0 && (!seqs || !off || !counts_in || !counts || !ids)) return BWAGPU_EINVAL;
	if (opt->e_del <= 0 || opt->e_ins <= 0 || (opt->flag & 0x800 /* MEM_F_PRIMARY5 */)) return BWAGPU_EINVAL;
	FlatReads R; FlatLists F; RegLists L;
	if (!R.scan(h, "bwagpu_sampe_flat", 2 * (size_t)n_pairs, seqs, off) || !F.scan(h, 2 * (size_t)n_pairs, counts_in, regs_in, counts_in) || !R.codes_ok(h, "bwagpu_sampe_flat")) return BWAGPU_EINVAL;
	const BusyGuard busy(h->ibuf->busy);
	HIPCHK(h, hipSetDevice(h->device));
	if (int rc = R.upload(h, "sampe")) return rc;
	const int rc = F.upload(h, "sampe", counts_in, regs_in, ids, F.n, L);
	return rc != BWAGPU_OK ? rc : sampe_run(h, opt, pes, L, h->d_pf_seq.as<u8>(), h->d_pf_seqoff.as<i64>(), R.max_len, R.n_bases - R.first, counts, out);
}

// ---- paired-end SAM text on the device (dev_samtext_pe.h) ---------------------------------------------------------------------------------------------
extern "C" void bwagpu_sam_pe_limits(int32_t out[2]) { out[0] = SAM_STAGE; out[1] = SAM_STEP; }

// mates carry one name (the reference dies on a pair that does not, bwamem_pair.c:386, :416)
static int sam_pe_names_check(bwagpu_t *h, int n_pairs, const bwagpu_sam_in_t *in, const char *what)
{
	for (int p = 0; p < n_pairs; ++p) {
		const i64 a = in->name_off[2 * (size_t)p], b = in->name_off[2 * (size_t)p + 1], c = in->name_off[2 * (size_t)p + 2];
		if (b - a != c - b || memcmp(in->names + a, in->names + b, (size_t)(b - a)) != 0) {
			h->err = std::string(what) + ": paired reads have different names (pair " + std::to_string(p) + ")"; return BWAGPU_EINVAL;
		}
	}
	return BWAGPU_OK;
}

static void pe_out_free(bwagpu_pe_out_t *o)
{
	bwagpu_free(o->regs); bwagpu_free(o->src); bwagpu_free(o->rescue); bwagpu_free(o->pri); bwagpu_free(o->n_pri); bwagpu_free(o->pairs); bwagpu_free(o->sampe); bwagpu_free(o->cigs);
	bwagpu_free(o->ops); bwagpu_free(o->alns); bwagpu_free(o->n_aln);
	memset(o, 0, sizeof *o);
}

// Both entry points: sampe_run (its arguments), then the two passes of the formatter on the records it left on the device.  q_bases: bytes of in->quals.
// Without pe, sampe_run leaves alignment records, patched marking records and the operation array where they are.
static int sam_pe_run(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pestat_t pes[4], const RegLists &L, const u8 *d_seq, const i64 *d_seqoff, int max_len, i64 n_bases, i64 q_bases,
					  const bwagpu_sam_in_t *in, int32_t *counts, bwagpu_pe_out_t *pe, bwagpu_sam_out_t *out)
{
	const int n = L.n;
	bwagpu_pe_out_t own; memset(&own, 0, sizeof own);
	bwagpu_pe_out_t *P = pe ? pe : &own;
	int rc = sampe_run(h, opt, pes, L, d_seq, d_seqoff, max_len, n_bases, counts, P, pe == nullptr);
	if (rc != BWAGPU_OK) return rc;
	if (n == 0) rc = sam_none(out);
	else {
		SamIn S = {};
		rc = sam_upload(h, n, q_bases, in, S);
		DevBuf *D = h->d_rs, *Sp = h->d_sp;
		if (rc == BWAGPU_OK && P->n_regs == 0) {      // no region in the whole batch: the lists and pair records are the host's only
			if (D[bwagpu_s::RS_ACNT].ensure((size_t)n * 4) || D[bwagpu_s::RS_POFF].ensure(((size_t)n + 1) * 8) || Sp[bwagpu_s::SP_OUT].ensure((size_t)(n / 2) * sizeof(bwagpu_sampe_t))) {
				h->err = "hipMalloc failed (sam_pe)"; rc = BWAGPU_ENOMEM;
			} else if (hipMemsetAsync(D[bwagpu_s::RS_ACNT].p, 0, (size_t)n * 4, h->stream) != hipSuccess || hipMemsetAsync(D[bwagpu_s::RS_POFF].p, 0, ((size_t)n + 1) * 8, h->stream) != hipSuccess ||
					   hipMemcpyAsync(Sp[bwagpu_s::SP_OUT].p, P->sampe, (size_t)(n / 2) * sizeof(bwagpu_sampe_t), hipMemcpyHostToDevice, h->stream) != hipSuccess) {
				h->err = "hipMemcpy failed (sam_pe)"; rc = BWAGPU_EHIP;
			}
		}
		if (rc == BWAGPU_OK) {
			S.alns = h->d_aln_out.as<bwagpu_aln_t>(); S.pri = h->d_pri_out.as<bwagpu_primary_t>(); S.cigs = Sp[bwagpu_s::SP_CIGS].as<bwagpu_cigar_t>(); S.ops = Sp[bwagpu_s::SP_EXT].as<u32>();
			S.seq = d_seq; S.seq_off = d_seqoff;
			const int e[4] = { 0, 1, 2, 3 };      // (ev[5], ev[6] hold sampe_run's last segment)
			rc = sam_passes(h, opt, n, D[bwagpu_s::RS_ACNT].as<i32>(), D[bwagpu_s::RS_POFF].as<i64>(), S, Sp[bwagpu_s::SP_OUT].as<bwagpu_sampe_t>(), e, out);
		}
		if (rc == BWAGPU_OK) {
			if (!pe && P->n_regs > 0) (void)hipEventElapsedTime(&P->kernel_ms[5], h->ev[5], h->ev[6]);
			for (int k = 0; k < 6; ++k) out->kernel_ms[0] += P->kernel_ms[k];
		}
	}
	if (!pe || rc != BWAGPU_OK) pe_out_free(P);
	return rc;
}

extern "C" int bwagpu_batch_sam_pe(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pestat_t pes[4], int64_t id0, const bwagpu_sam_in_t *in, int32_t *counts, bwagpu_pe_out_t *pe,
								   bwagpu_sam_out_t *out)
{
	if (pe) memset(pe, 0, sizeof *pe);
	if (out) memset(out, 0, sizeof *out);
	if (!h || !opt || !pes || !h->ran || !h->downloaded || !in || !out || (h->n_reads > 0 && !counts)) return BWAGPU_EINVAL;
	if ((h->n_reads & 1) || (id0 & 1) || opt->e_del <= 0 || opt->e_ins <= 0 || (opt->flag & 0x800 /* MEM_F_PRIMARY5 */)) return BWAGPU_EINVAL;
	if (int rc = sam_in_check(h, h->n_reads, in, "bwagpu_batch_sam_pe")) return rc;
	if (int rc = sam_pe_names_check(h, h->n_reads / 2, in, "bwagpu_batch_sam_pe")) return rc;
	const BusyGuard busy(h->ibuf->busy);
	HIPCHK(h, hipSetDevice(h->device));
	return sam_pe_run(h, opt, pes, lists_of_batch(h, id0), h->d_seq.as<u8>(), h->d_off.as<i64>(), h->max_len, h->n_bases, h->n_bases, in, counts, pe, out);
}

extern "C" int bwagpu_sam_pe_flat(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pestat_t pes[4], int n_pairs, const uint8_t *seqs, const int64_t *off, const int32_t *counts_in,
								  const bwagpu_alnreg_t *regs_in, const int64_t *ids, const bwagpu_sam_in_t *in, int32_t *counts, bwagpu_pe_out_t *pe, bwagpu_sam_out_t *out)
{
	if (pe) memset(pe, 0, sizeof *pe);
	if (out) memset(out, 0, sizeof *out);
	if (!h || !opt || !pes || n_pairs < 0 || n_pairs > 0x1fffffff || !in || !out) return BWAGPU_EINVAL;
	if (n_pairs > 0 && (!seqs || !off || !counts_in || !counts || !ids)) return BWAGPU_EINVAL;
	if (opt->e_del <= 0 || opt->e_ins <= 0 || (opt->flag & 0x800 /* MEM_F_PRIMARY5 */)) return BWAGPU_EINVAL;
	if (int rc = sam_in_check(h, 2 * n_pairs, in, "bwagpu_sam_pe_flat")) return rc;
	if (int rc = sam_pe_names_check(h, n_pairs, in, "bwagpu_sam_pe_flat")) return rc;
	FlatReads R; FlatLists F; RegLists L;
	if (!R.scan(h, "bwagpu_sam_pe_flat", 2 * (size_t)n_pairs, seqs, off) || !F.scan(h, 2 * (size_t)n_pairs, counts_in, regs_in, counts_in) || !R.codes_ok(h, "bwagpu_sam_pe_flat")) return BWAGPU_EINVAL;
	const BusyGuard busy(h->ibuf->busy);
	HIPCHK(h, hipSetDevice(h->device));
	if (int rc = R.upload(h, "sam_pe")) return rc;
	const int rc = F.upload(h, "sam_pe", counts_in, regs_in, ids, F.n, L);
	if (rc != BWAGPU_OK) return rc;
	return sam_pe_run(h, opt, pes, L, h->d_pf_seq.as<u8>(), h->d_pf_seqoff.as<i64>(), R.max_len, R.n_bases - R.first, R.n_bases, in, counts, pe, out);
}

extern "C" int bwagpu_align_flat(bwagpu_t *h, const bwagpu_opt_t *opt, int n, const uint8_t *seqs, const int64_t *off,
								 int32_t *counts, bwagpu_alnreg_t **regs_out, int64_t *n_regs_out)
{
	int rc;
	if ((rc = bwagpu_batch_upload(h, n, seqs, off))) return rc;
	if ((rc = bwagpu_batch_run(h, opt))) return rc;
	return bwagpu_batch_download(h, counts, regs_out, n_regs_out);
}

// nst_nt4_table (bntseq.c:46-63) as a function: A/a C/c G/g T/t -> 0..3, '-' -> 5, everything else 4
static inline uint8_t nt4(unsigned char c)
{
	switch (c) {
	case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3;
	case '-': return 5;
	default: return 4;
	}
}

extern "C" int bwagpu_align_bseq(bwagpu_t *h, const bwagpu_opt_t *opt, int n, bwagpu_bseq1_t *seqs, bwagpu_alnreg_v *regs)
{
	if (!h || !opt || n < 0 || (n > 0 && (!seqs || !regs))) return BWAGPU_EINVAL;
	std::vector<i64> off((size_t)n + 1, 0);
	for (int i = 0; i < n; ++i) off[i + 1] = off[i] + seqs[i].l_seq;
	std::vector<u8> flat((size_t)off[n] + 1);
	for (int i = 0; i < n; ++i) {   // in-place nt4 encoding, the contract of mem_align1_core (bwamem.c:1087-1088)
		char *s = seqs[i].seq;
		for (int j = 0; j < seqs[i].l_seq; ++j) { unsigned char c = (unsigned char)s[j]; s[j] = (char)(c < 4 ? c : nt4(c)); }
		memcpy(flat.data() + off[i], s, (size_t)seqs[i].l_seq);
	}
	std::vector<int32_t> counts((size_t)n);
	bwagpu_alnreg_t *all = nullptr; int64_t tot = 0;
	int rc = bwagpu_align_flat(h, opt, n, flat.data(), off.data(), counts.data(), &all, &tot);
	if (rc) return rc;
	i64 k = 0;
	for (int i = 0; i < n; ++i) {
		regs[i].n = regs[i].m = (size_t)counts[i];
		regs[i].a = (bwagpu_alnreg_t*)malloc((size_t)(counts[i] ? counts[i] : 1) * sizeof(bwagpu_alnreg_t));
		if (!regs[i].a) {   // leave no half-filled output behind
			for (int j = 0; j < i; ++j) { free(regs[j].a); regs[j].a = nullptr; regs[j].n = regs[j].m = 0; }
			regs[i].n = regs[i].m = 0;
			bwagpu_free(all);
			return BWAGPU_ENOMEM;
		}
		memcpy(regs[i].a, all + k, (size_t)counts[i] * sizeof(bwagpu_alnreg_t));
		k += counts[i];
	}
	bwagpu_free(all);
	return BWAGPU_OK;
}

// ---- differential tests of the DP routines (dev_debug.h) ---------------------------------------------------------------------
extern "C" int bwagpu_debug_dp(bwagpu_t *h, const bwagpu_opt_t *opt, int kind, int n_cases, const bwagpu_dp_case_t *cases, const uint8_t *seqs, int64_t n_seq_bytes, int32_t *out)
{
	if (!h || !opt || n_cases < 0 || kind < 0 || kind > 7 || (n_cases > 0 && (!cases || !seqs || !out)) || n_seq_bytes < 0) return BWAGPU_EINVAL;
	if (opt->e_del <= 0 || opt->e_ins <= 0) return BWAGPU_EINVAL;
	if (n_cases == 0) return BWAGPU_OK;
	static_assert(sizeof(bwagpu_dp_case_t) == 32, "layout");
	int max_q = 1, max_w = 1;
	for (int i = 0; i < n_cases; ++i) {
		const bwagpu_dp_case_t &c = cases[i];
		if (c.q_len < 0 || c.t_len < 0 || c.q_off < 0 || c.t_off < 0 || (i64)c.q_off + c.q_len > n_seq_bytes || (i64)c.t_off + c.t_len > n_seq_bytes || c.w < 0) return BWAGPU_EINVAL;
		if ((kind == 0 || kind == 1 || kind >= 6) && c.h0 <= 0) return BWAGPU_EINVAL;      // ksw_extend2 asserts h0 > 0 (ksw.c:420)
		if (c.q_len > max_q) max_q = c.q_len;
		if (c.w > max_w) max_w = c.w;
	}
	HIPCHK(h, hipSetDevice(h->device));
	DevBuf d_seq, d_pac, d_cases, d_out, d_scr, d_pac2;
	int rc = BWAGPU_OK;
	const int grid = n_cases < 2048 ? n_cases : 2048;
	const bool dbg_blk = (h->cfg.dedup_blk >= 0 ? h->cfg.dedup_blk : 1) != 0;      // kind 3 in its four-columns-per-lane form (the product's default) or, option dedup_blk = 0, one column per lane
	hipError_t e = hipSuccess;
	if (d_seq.ensure((size_t)n_seq_bytes + 16) || d_pac.ensure((size_t)n_seq_bytes / 4 + 16) || d_cases.ensure((size_t)n_cases * sizeof(bwagpu_dp_case_t)) || d_out.ensure((size_t)n_cases * DBG_OUT_INTS * 4)) { h->err = "hipMalloc failed (debug)"; rc = BWAGPU_ENOMEM; goto done; }
	e = hipMemcpyAsync(d_seq.p, seqs, (size_t)n_seq_bytes, hipMemcpyHostToDevice, h->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(d_cases.p, cases, (size_t)n_cases * sizeof(bwagpu_dp_case_t), hipMemcpyHostToDevice, h->stream);
	if (e == hipSuccess) e = hipMemsetAsync(d_out.p, 0, (size_t)n_cases * DBG_OUT_INTS * 4, h->stream);
	if (e == hipSuccess) {
		hipLaunchKernelGGL(k_debug_pack, dim3(256), dim3(256), 0, h->stream, d_seq.as<u8>(), (i64)n_seq_bytes, d_pac.as<u8>());
		DevIndex ix = h->ix; ix.pac = d_pac.as<u8>(); ix.l_pac = n_seq_bytes;
		if (kind == 0) {
			if (max_q > WAVE_EXT_MAX_LEN) { rc = BWAGPU_EINVAL; goto done; }
			const size_t lds = (8 * (size_t)(max_q + 2 + 64) + 5 * (size_t)((max_q + 64 + 3) & ~3) + 32 + 15) & ~(size_t)15;
			hipLaunchKernelGGL((k_debug_extend<false>), dim3(grid), dim3(64), lds, h->stream, ix, *opt, n_cases, d_cases.as<bwagpu_dp_case_t>(), d_seq.as<u8>(), max_q, 0, d_out.as<i32>(), 0);
		} else if (kind == 1) {
			int ring_cols = 256; while (ring_cols < 2 * max_w + 4 + 128) ring_cols <<= 1;
			if (ring_cols > 4096) { rc = BWAGPU_EINVAL; goto done; }
			hipLaunchKernelGGL((k_debug_extend<true>), dim3(grid), dim3(64), (size_t)8 * ring_cols + 32, h->stream, ix, *opt, n_cases, d_cases.as<bwagpu_dp_case_t>(), d_seq.as<u8>(), max_q, ring_cols, d_out.as<i32>(), (int)(h->cfg.ext_blk != 0));
		} else if (kind == 2) {
			hipLaunchKernelGGL(k_debug_global, dim3(grid), dim3(64), (size_t)CIG_LDS_BYTES(CIG_Z_BIG), h->stream, ix, *opt, n_cases, d_cases.as<bwagpu_dp_case_t>(), d_seq.as<u8>(), d_out.as<i32>());
		} else if (kind == 3) {
			int ring_cols = 256; while (ring_cols < 2 * max_w + 4 + 128) ring_cols <<= 1;
			if (ring_cols > 4096) { rc = BWAGPU_EINVAL; goto done; }
			const int q_cap = dbg_blk && 8 * ring_cols + 32 + ((max_q + 15) & ~15) <= 65536 ? (max_q + 15) & ~15 : 0;
			if (dbg_blk) hipLaunchKernelGGL(k_debug_global_ring<true>, dim3(grid), dim3(64), (size_t)8 * ring_cols + 32 + q_cap, h->stream, ix, *opt, n_cases, d_cases.as<bwagpu_dp_case_t>(), d_seq.as<u8>(), ring_cols, d_out.as<i32>(), q_cap);
			else hipLaunchKernelGGL(k_debug_global_ring<false>, dim3(grid), dim3(64), (size_t)8 * ring_cols + 32 + q_cap, h->stream, ix, *opt, n_cases, d_cases.as<bwagpu_dp_case_t>(), d_seq.as<u8>(), ring_cols, d_out.as<i32>(), q_cap);
		} else if (kind == 6 || kind == 7) {
			const int g4 = (n_cases + 3) / 4 < 2048 ? (n_cases + 3) / 4 : 2048;
			if (kind == 6) hipLaunchKernelGGL((k_debug_extpack<4>), dim3(g4), dim3(64), (size_t)XP_LDS_BYTES, h->stream, ix, *opt, n_cases, d_cases.as<bwagpu_dp_case_t>(), d_seq.as<u8>(), d_out.as<i32>());
			else hipLaunchKernelGGL((k_debug_extpack<8>), dim3(g4), dim3(64), (size_t)XP_LDS_BYTES, h->stream, ix, *opt, n_cases, d_cases.as<bwagpu_dp_case_t>(), d_seq.as<u8>(), d_out.as<i32>());
		} else if (kind == 5) {
			int max_t = 1; for (int i = 0; i < n_cases; ++i) if (cases[i].t_len > max_t) max_t = cases[i].t_len;
			i64 z_cap = ((i64)max_t + 16) * ((CIGL_MAX_COLS + 15) & ~15); z_cap = (z_cap + 15) & ~(i64)15;
			const int blocks = grid < 64 ? grid : 64;
			if (d_scr.ensure((size_t)blocks * z_cap) || d_pac2.ensure((size_t)blocks * CIGL_MAX_OPS * 4)) { h->err = "hipMalloc failed (debug)"; rc = BWAGPU_ENOMEM; goto done; }
			hipLaunchKernelGGL(k_debug_global_long, dim3(blocks), dim3(64), (size_t)CIGL_LDS_BYTES, h->stream, ix, *opt, n_cases, d_cases.as<bwagpu_dp_case_t>(), d_seq.as<u8>(), d_scr.as<u8>(), z_cap, d_pac2.as<u32>(), d_out.as<i32>());
		} else {
			hipLaunchKernelGGL(k_debug_align2, dim3(grid), dim3(64), 0, h->stream, ix, *opt, n_cases, d_cases.as<bwagpu_dp_case_t>(), d_seq.as<u8>(), d_out.as<i32>());
		}
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpyAsync(out, d_out.p, (size_t)n_cases * DBG_OUT_INTS * 4, hipMemcpyDeviceToHost, h->stream);
	if (e == hipSuccess) e = wait_stream(h);
	if (e != hipSuccess) { h->err = std::string("bwagpu_debug_dp: ") + hipGetErrorString(e); rc = BWAGPU_EHIP; }
done:
	(void)hipStreamSynchronize(h->stream);
	d_seq.release(); d_pac.release(); d_cases.release(); d_out.release(); d_scr.release(); d_pac2.release();
	return rc;
}

// ---- differential tests of the sorts (dev_debug.h) ----------------------------------------------------------------------------
extern "C" int bwagpu_debug_sort(bwagpu_t *h, int kind, int n_cases, const bwagpu_sort_key_t *keys, const int64_t *off, int dd_net, int par_cap, int chain_flt_lds, int32_t *perm, int32_t *status)
{
	if (!h || kind < 0 || kind > DBG_SORT_PAR_BEST || n_cases < 0 || (n_cases > 0 && (!off || !status))) return BWAGPU_EINVAL;
	if (n_cases == 0) return BWAGPU_OK;
	static_assert(sizeof(bwagpu_sort_key_t) == 16, "layout");
	if (off[0] != 0) return BWAGPU_EINVAL;
	for (int i = 0; i < n_cases; ++i) if (off[i + 1] < off[i] || off[i + 1] - off[i] > (1 << 20)) return BWAGPU_EINVAL;
	const size_t tot = (size_t)off[n_cases];
	if (tot > 0 && (!keys || !perm)) return BWAGPU_EINVAL;
	const bool par = kind == DBG_SORT_PAR_END || kind == DBG_SORT_PAR_BEST;
	if (par && (par_cap < 2 || par_cap > DBG_SORT_PAR_CAP_MAX || dd_net < 0)) return BWAGPU_EINVAL;
	if (kind == DBG_SORT_CHAIN_W && chain_flt_lds < 0) return BWAGPU_EINVAL;
	if (chain_flt_lds > CW_FLT_LDS) chain_flt_lds = CW_FLT_LDS;                  // (as the option is read, batch_run)
	HIPCHK(h, hipSetDevice(h->device));
	DevBuf d_keys, d_off, d_perm, d_st, d_a, d_b;      // d_a: the records a kind sorts (or its seeds), d_b: its second array (key scratch, srt[], the block kernel's staging records)
	int rc = BWAGPU_OK;
	hipError_t e = hipSuccess;
	const bool lane_kind = kind == DBG_SORT_U64 || kind == DBG_SORT_INTV || kind == DBG_SORT_REG_END || kind == DBG_SORT_REG_BEST;
	const int blk_grid = n_cases < 128 ? n_cases : 128;
	size_t bytes_a = 16, bytes_b = 16;
	if (kind == DBG_SORT_U64) bytes_a = tot * 8;
	else if (kind == DBG_SORT_INTV) bytes_a = tot * sizeof(Intv3);
	else if (kind == DBG_SORT_INTV_BLK) { bytes_a = tot * sizeof(Intv3); bytes_b = (size_t)blk_grid * PUB_MAX * sizeof(Intv3); }
	else if (kind == DBG_SORT_REG_END || kind == DBG_SORT_REG_BEST) { bytes_a = tot * sizeof(bwagpu_alnreg_t); bytes_b = tot * sizeof(RegKey); }
	else if (kind == DBG_SORT_CHAIN_SEEDS) { bytes_a = tot * sizeof(bwagpu_seed_t); bytes_b = tot * 8; }
	else if (kind == DBG_SORT_CHAIN_W) { bytes_a = tot * 4; bytes_b = tot * 8; }
	if (d_keys.ensure(tot * sizeof(bwagpu_sort_key_t) + 16) || d_off.ensure((size_t)(n_cases + 1) * 8) || d_perm.ensure(tot * 4 + 16) || d_st.ensure((size_t)n_cases * 4) || d_a.ensure(bytes_a + 16) || d_b.ensure(bytes_b + 16)) {
		h->err = "hipMalloc failed (debug)"; rc = BWAGPU_ENOMEM; goto done;
	}
	if (tot) e = hipMemcpyAsync(d_keys.p, keys, tot * sizeof(bwagpu_sort_key_t), hipMemcpyHostToDevice, h->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(d_off.p, off, (size_t)(n_cases + 1) * 8, hipMemcpyHostToDevice, h->stream);
	if (e == hipSuccess) e = hipMemsetAsync(d_perm.p, 0xff, tot * 4 + 16, h->stream);           // -1: a place nothing was written to
	if (e == hipSuccess) e = hipMemsetAsync(d_st.p, 0xff, (size_t)n_cases * 4, h->stream);
	if (e == hipSuccess) {
		const bwagpu_sort_key_t *dk = d_keys.as<bwagpu_sort_key_t>(); const i64 *dof = d_off.as<i64>(); i32 *dp = d_perm.as<i32>(), *ds = d_st.as<i32>();
		if (lane_kind) {
			const dim3 grid((unsigned)((n_cases + 255) / 256 < 1024 ? (n_cases + 255) / 256 : 1024)), blk(256);
			if (kind == DBG_SORT_U64) hipLaunchKernelGGL((k_debug_sort_lane<DBG_SORT_U64>), grid, blk, 0, h->stream, n_cases, dk, dof, d_a.as<u64>(), (Intv3*)nullptr, (bwagpu_alnreg_t*)nullptr, (RegKey*)nullptr, dp, ds);
			else if (kind == DBG_SORT_INTV) hipLaunchKernelGGL((k_debug_sort_lane<DBG_SORT_INTV>), grid, blk, 0, h->stream, n_cases, dk, dof, (u64*)nullptr, d_a.as<Intv3>(), (bwagpu_alnreg_t*)nullptr, (RegKey*)nullptr, dp, ds);
			else if (kind == DBG_SORT_REG_END) hipLaunchKernelGGL((k_debug_sort_lane<DBG_SORT_REG_END>), grid, blk, 0, h->stream, n_cases, dk, dof, (u64*)nullptr, (Intv3*)nullptr, d_a.as<bwagpu_alnreg_t>(), d_b.as<RegKey>(), dp, ds);
			else hipLaunchKernelGGL((k_debug_sort_lane<DBG_SORT_REG_BEST>), grid, blk, 0, h->stream, n_cases, dk, dof, (u64*)nullptr, (Intv3*)nullptr, d_a.as<bwagpu_alnreg_t>(), d_b.as<RegKey>(), dp, ds);
		} else if (kind == DBG_SORT_INTV_BLK) {
			hipLaunchKernelGGL(k_debug_sort_blk, dim3(blk_grid), dim3(256), 0, h->stream, n_cases, dk, dof, d_a.as<Intv3>(), d_b.as<Intv3>(), dp, ds);
		} else {
			const dim3 grid((unsigned)(n_cases < 2048 ? n_cases : 2048)), blk(64);
			if (kind == DBG_SORT_CHAIN_SEEDS) hipLaunchKernelGGL((k_debug_sort_wave<DBG_SORT_CHAIN_SEEDS>), grid, blk, 0, h->stream, n_cases, dk, dof, d_a.as<bwagpu_seed_t>(), d_b.as<u64>(), (i32*)nullptr, 0, 0, 0, dp, ds);
			else if (kind == DBG_SORT_CHAIN_W) hipLaunchKernelGGL((k_debug_sort_wave<DBG_SORT_CHAIN_W>), grid, blk, (size_t)CW_LDS_BYTES, h->stream, n_cases, dk, dof, (bwagpu_seed_t*)nullptr, d_b.as<u64>(), d_a.as<i32>(), 0, 0, chain_flt_lds, dp, ds);
			else if (kind == DBG_SORT_PAR_END) hipLaunchKernelGGL((k_debug_sort_wave<DBG_SORT_PAR_END>), grid, blk, DDW_PAR_BYTES(par_cap), h->stream, n_cases, dk, dof, (bwagpu_seed_t*)nullptr, (u64*)nullptr, (i32*)nullptr, dd_net, par_cap, 0, dp, ds);
			else hipLaunchKernelGGL((k_debug_sort_wave<DBG_SORT_PAR_BEST>), grid, blk, DDW_PAR_BYTES(par_cap), h->stream, n_cases, dk, dof, (bwagpu_seed_t*)nullptr, (u64*)nullptr, (i32*)nullptr, dd_net, par_cap, 0, dp, ds);
		}
		e = hipGetLastError();
	}
	if (e == hipSuccess && tot) e = hipMemcpyAsync(perm, d_perm.p, tot * 4, hipMemcpyDeviceToHost, h->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(status, d_st.p, (size_t)n_cases * 4, hipMemcpyDeviceToHost, h->stream);
	if (e == hipSuccess) e = wait_stream(h);
	if (e != hipSuccess) { h->err = std::string("bwagpu_debug_sort: ") + hipGetErrorString(e); rc = BWAGPU_EHIP; }
done:
	(void)hipStreamSynchronize(h->stream);
	d_keys.release(); d_off.release(); d_perm.release(); d_st.release(); d_a.release(); d_b.release();
	return rc;
}

extern "C" void bwagpu_debug_sort_limits(int32_t out[8])
{
	out[0] = PUB_MAX; out[1] = CW_PW_LDS; out[2] = CW_FLT_LDS; out[3] = DEDUP_KEYSORT_MIN; out[4] = DBG_SORT_PAR_CAP_MAX; out[5] = CHAIN_SORT_LANE_MAX; out[6] = DEDUP_NET_DEFAULT; out[7] = 0;
}

// ---- stage taps ----------------------------------------------------------------------------------------------
extern "C" int bwagpu_tap_intervals(bwagpu_t *h, int32_t *counts, bwagpu_intv_t **out, int64_t *n_out)
{
	if (!h || !h->ran || !out || !n_out) return BWAGPU_EINVAL;
	static_assert(sizeof(bwagpu_intv_t) == sizeof(Intv3), "layout");
	return gather<bwagpu_intv_t>(h, h->d_intv_n, h->d_intv_off, h->d_intv, (i64)h->n_reads * h->mem_cap, counts, out, n_out);
}

extern "C" int bwagpu_tap_chains(bwagpu_t *h, int32_t *counts, bwagpu_chain_t **chains, int64_t *n_chains, bwagpu_seed_t **seeds, int64_t *n_seeds)
{
	if (!h || !h->ran || !chains || !n_chains || !seeds || !n_seeds) return BWAGPU_EINVAL;
	HIPCHK(h, hipSetDevice(h->device));
	const int n = h->n_reads;
	std::vector<i32> cn((size_t)n), sn((size_t)n); std::vector<i64> off((size_t)n);
	if (n) {
		HIPCHK(h, hipMemcpy(cn.data(), h->d_chain_n.p, (size_t)n * 4, hipMemcpyDeviceToHost));
		HIPCHK(h, hipMemcpy(sn.data(), h->d_seed_n.p, (size_t)n * 4, hipMemcpyDeviceToHost));
		HIPCHK(h, hipMemcpy(off.data(), h->d_seed_off.p, (size_t)n * 8, hipMemcpyDeviceToHost));
	}
	std::vector<bwagpu_chain_t> vc; std::vector<bwagpu_seed_t> vs; std::vector<bwagpu_chain_t> tc; std::vector<bwagpu_seed_t> ts;
	for (int i = 0; i < n; ++i) {   // per-read regions: kept chain headers at +80n, their seeds at +112n (RegionView)
		if (counts) counts[i] = cn[i];
		if (cn[i] == 0) continue;
		const u8 *base = h->d_slot_blob.as<u8>() + off[i] * SLOT_BLOB_BYTES;
		tc.resize((size_t)cn[i]);
		HIPCHK(h, hipMemcpy(tc.data(), base + (size_t)80 * sn[i], (size_t)cn[i] * sizeof(bwagpu_chain_t), hipMemcpyDeviceToHost));
		int ks = 0; for (auto &c : tc) ks += c.n_seeds;
		ts.resize((size_t)ks);
		if (ks) HIPCHK(h, hipMemcpy(ts.data(), base + (size_t)112 * sn[i], (size_t)ks * sizeof(bwagpu_seed_t), hipMemcpyDeviceToHost));
		vc.insert(vc.end(), tc.begin(), tc.end()); vs.insert(vs.end(), ts.begin(), ts.end());
	}
	*chains = (bwagpu_chain_t*)malloc((vc.size() + 1) * sizeof(bwagpu_chain_t)); *seeds = (bwagpu_seed_t*)malloc((vs.size() + 1) * sizeof(bwagpu_seed_t));
	if (!*chains || !*seeds) return BWAGPU_ENOMEM;
	if (!vc.empty()) memcpy(*chains, vc.data(), vc.size() * sizeof(bwagpu_chain_t));
	if (!vs.empty()) memcpy(*seeds, vs.data(), vs.size() * sizeof(bwagpu_seed_t));
	*n_chains = (int64_t)vc.size(); *n_seeds = (int64_t)vs.size();
	return BWAGPU_OK;
}

extern "C" int bwagpu_tap_regs_raw(bwagpu_t *h, int32_t *counts, bwagpu_alnreg_t **out, int64_t *n_out)
{
	if (!h || !h->ran || !h->taps_on || !out || !n_out) return BWAGPU_EINVAL;
	return gather<bwagpu_alnreg_t>(h, h->d_reg_n_raw, h->d_reg_off, h->d_regs_raw, h->reg_cap, counts, out, n_out);
}
