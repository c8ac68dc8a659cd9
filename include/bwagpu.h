/* include/bwagpu.h -- C-ABI of the MI355X-native BWA-MEM alignment core (libbwagpu.so).
 *
 * The library replaces exactly one thing in lh3/bwa: the first parallel loop of mem_process_seqs()
 *     kt_for(opt->n_threads, worker1, &w, n)                       (reference bwamem.c:1252)
 * i.e. "for every read i: regs[i] = mem_align1_core(opt, bwt, bns, pac, l_seq, seq, aux)"
 * (reference bwamem.c:1081-1117, 1203-1215).  Everything it computes on the way -- SMEM seeding over the
 * FM-index (bwt.c:189-379), suffix-array lookup (bwt.c:53-96), chaining and chain filtering
 * (bwamem.c:216-411), banded seed extension (ksw.c:416-515 via bwamem.c:658-812) and region
 * de-duplication/patching (bwamem.c:432-515, ksw.c:540-642) -- runs as HIP kernels on gfx950 with the index
 * resident in HBM.  Results (mem_alnreg_t records) are bit-identical to the reference's.
 *
 * Conventions
 *   - plain C, plain pointers and sizes; no C++/torch types cross this boundary;
 *   - every function returns 0 on success or a negative BWAGPU_E* code (the reference itself has no error
 *     returns on this path: it exit()s via err_fatal, utils.c:90-122; a drop-in wrapper prints
 *     bwagpu_strerror() and exits to mimic that);
 *   - a handle is single-caller / non-reentrant, like step 1 of the reference's kt_pipeline
 *     (kthread.c:93-104 guarantees one batch at a time in mem_process_seqs);
 *   - there is NO CPU fallback: without a HIP device bwagpu_create() fails with BWAGPU_ENODEV.
 *
 * Struct layouts below are byte-for-byte those of the reference (checked by tests against the compiled
 * reference): bwagpu_opt_t == mem_opt_t (bwamem.h:52-84, 168 B), bwagpu_alnreg_t == mem_alnreg_t
 * (bwamem.h:86-104, 88 B), bwagpu_alnreg_v == mem_alnreg_v (bwamem.h:106), bwagpu_bseq1_t == bseq1_t
 * (bwa.h:58-61, 48 B).  A reference-side caller may pass its own structs through a pointer cast.
 */
#ifndef BWAGPU_H
#define BWAGPU_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BWAGPU_OK        0
#define BWAGPU_ENODEV   -1  /* no usable HIP device / HIP runtime error at start-up */
#define BWAGPU_EINVAL   -2  /* bad argument */
#define BWAGPU_ENOMEM   -3  /* host or device allocation failed */
#define BWAGPU_EIO      -4  /* index files missing or inconsistent */
#define BWAGPU_EHIP     -5  /* HIP runtime error during a batch (see bwagpu_last_error) */
#define BWAGPU_EUNSUP   -6  /* option combination not implemented on the device path yet */

typedef struct bwagpu_s bwagpu_t;

/* == mem_opt_t, reference bwamem.h:52-84 */
typedef struct {
	int a, b;
	int o_del, e_del;
	int o_ins, e_ins;
	int pen_unpaired;
	int pen_clip5, pen_clip3;
	int w;
	int zdrop;
	uint64_t max_mem_intv;
	int T;
	int flag;
	int min_seed_len;
	int min_chain_weight;
	int max_chain_extend;
	float split_factor;
	int split_width;
	int max_occ;
	int max_chain_gap;
	int n_threads;
	int chunk_size;
	float mask_level;
	float drop_ratio;
	float XA_drop_ratio;
	float mask_level_redun;
	float mapQ_coef_len;
	int mapQ_coef_fac;
	int max_ins;
	int max_matesw;
	int max_XA_hits, max_XA_hits_alt;
	int8_t mat[25];
} bwagpu_opt_t;

/* == mem_alnreg_t, reference bwamem.h:86-104 */
typedef struct {
	int64_t rb, re;
	int qb, qe;
	int rid;
	int score;
	int truesc;
	int sub;
	int alt_sc;
	int csub;
	int sub_n;
	int w;
	int seedcov;
	int secondary;
	int secondary_all;
	int seedlen0;
	int n_comp:30, is_alt:2;
	float frac_rep;
	uint64_t hash;
} bwagpu_alnreg_t;

/* Banded global alignment of one region as mem_reg2aln's band-doubling loop around bwa_gen_cigar2 leaves it
 * (bwamem.c:1143-1152, bwa.c:148-234): score, BAM-style CIGAR (len << 4 | op, op M=0 I=1 D=2) before clipping and before
 * the leading/trailing-deletion squeeze, and the NM / MD values computed from it (bwa.c:196-226).  n_cigar 1..6: the operations are
 * in cigar[]; n_cigar > 6 (up to 32768: a 10 kb read with 13 % indels has ~2500): they are entries [at, at + n_cigar) of the batch's
 * operation array (bwagpu_batch_cigar_ops), at = cigar[1] << 32 | cigar[0].  MD: md_len characters; up to 8 of them are the bytes of `md` (first character in the low byte),
 * longer strings are packed four to an entry (first character in the low byte) at entries [md, md + (md_len + 3) / 4) of the
 * operation array.  n_cigar == -1: not computed on the device (region below opt->T; a band of more than 2048 columns, more than 32768
 * operations or an MD string of more than 96 KiB; `score` then holds the reason 1/2/3, nm is -1) -- the caller runs bwa_gen_cigar2 itself. */
typedef struct {
	int32_t score;
	int32_t n_cigar;
	uint32_t cigar[6];
	int32_t nm;
	int32_t md_len;
	uint64_t md;
} bwagpu_cigar_t;

/* Insert-size window of one orientation as mem_matesw uses it: mem_pestat_t::low/high/failed (bwamem.h:108-112). */
typedef struct { int32_t low, high, failed, pad_; } bwagpu_pes_t;

/* One precomputed mate-rescue alignment: the kswr_t that mem_matesw's ksw_align2 call (bwamem_pair.c:177) returns for
 * aligning read `read` (or its reverse complement) inside the window that anchor position `anchor_rb` on contig
 * `anchor_rid` and orientation r imply.  r == -1: no alignment was due for this task (empty window, other contig, window
 * shorter than min_seed_len or beyond the kernel's limits). */
typedef struct {
	int32_t read, r;
	int64_t anchor_rb;
	int32_t anchor_rid;
	int32_t score, te, qe, score2, te2, tb, qb;
	int32_t pad_, pad2_;     /* zero */
} bwagpu_matesw_t;

/* == mem_alnreg_v, reference bwamem.h:106 */
typedef struct { size_t n, m; bwagpu_alnreg_t *a; } bwagpu_alnreg_v;

/* == bseq1_t, reference bwa.h:58-61 */
typedef struct {
	int l_seq, id;
	char *name, *comment, *seq, *qual, *sam;
} bwagpu_bseq1_t;

/* The reference index as plain arrays.  A reference-side caller fills it from bwt_t (bwt.h:48-60), bntseq_t
 * (bntseq.h:41-64) and the pac pointer of bwaidx_t (bwa.h:48-56); see INTEGRATION.md for the 15-line stub. */
typedef struct {
	/* FM-index: interleaved Occ/BWT words exactly as in bwt_t::bwt (bwtindex.c:150-172) */
	const uint32_t *bwt;     /* bwt_t::bwt      */
	uint64_t bwt_size;       /* bwt_t::bwt_size (number of uint32 words) */
	uint64_t primary;        /* bwt_t::primary  */
	uint64_t L2[5];          /* bwt_t::L2       */
	uint64_t seq_len;        /* bwt_t::seq_len  */
	/* sampled suffix array */
	const uint64_t *sa;      /* bwt_t::sa (sa[0] == (uint64_t)-1) */
	uint64_t n_sa;           /* bwt_t::n_sa     */
	int sa_intv;             /* bwt_t::sa_intv (power of two) */
	/* 2-bit packed forward reference */
	const uint8_t *pac;      /* bwaidx_t::pac, l_pac/4+1 bytes */
	int64_t l_pac;           /* bntseq_t::l_pac */
	/* contig table */
	int32_t n_seqs;          /* bntseq_t::n_seqs */
	const int64_t *ctg_offset;  /* anns[i].offset */
	const int32_t *ctg_len;     /* anns[i].len    */
	const int32_t *ctg_is_alt;  /* anns[i].is_alt */
} bwagpu_index_desc_t;

/* Counters of one batch (for the roofline denominator) and per-stage device times. */
typedef struct {
	int64_t n_reads, n_bases;
	int64_t n_intv;          /* SA intervals kept by mem_collect_intv          */
	int64_t n_seeds;         /* bwt_sa calls (N_sa)                            */
	int64_t n_chains;        /* chains after mem_chain_flt                     */
	int64_t n_regs_raw;      /* regions before mem_sort_dedup_patch            */
	int64_t n_regs;          /* regions returned                               */
	/* filled only when stats collection is enabled (bwagpu_set_stats): */
	int64_t n_occ_blocks;    /* N_blk: 64-byte index blocks touched by seeding */
	int64_t n_lf_steps;      /* N_lf : bwt_invPsi steps inside bwt_sa          */
	int64_t n_ext_calls;     /* ksw_extend2 calls                              */
	int64_t n_ext_cells;     /* ksw_extend2 DP cells                           */
	int64_t n_glb_calls;     /* ksw_global2 (score-only) calls                 */
	int64_t n_glb_cells;     /* ksw_global2 DP cells                           */
	int64_t ref_bases;       /* W_ref: reference bases covered by extension windows */
	int64_t n_sw_calls;      /* mem_seed_sw local alignments (long reads)      */
	int64_t n_sw_cells;
	/* device time per stage, milliseconds (HIP events on the library's stream) */
	float ms_seed, ms_sa, ms_chain, ms_seedsw, ms_extend, ms_dedup, ms_total;
	int32_t n_retries;       /* arena-growth reruns */
	float ms_publish;        /* k_publish + k_expand (interval sort, slot reservation); ms_seed is the k_seed kernel alone */
	int64_t n_tab_lookups;   /* 16-byte prefix-table entries read by seeding in place of index blocks (stats only) */
	int64_t n_bt_nodes;      /* B-tree nodes (160 B) visited by chaining's look-ups (stats only)               */
	int64_t n_chain_recs;    /* chain records (64 B) read or created by chaining (stats only)                  */
	int64_t n_chain_deferred;/* (rounds 2-4: reads whose chaining outgrew the first LDS tier; 0 since round 5 -- one chaining kernel, no tiers) */
	int64_t n_ext_fast;      /* ksw_extend2 calls answered without DP (diagonal rule, dev_extw.h)              */
	int64_t n_chain_deferred2;/* (likewise: always 0)                                                               */
	/* the calls after bwagpu_batch_run, filled by them (HIP events on the handle's stream; 0 until the call has run for this batch): */
	float ms_pack;           /* bwagpu_batch_download: packing the used region records on the device          */
	float ms_download_copy;  /* ... and their device-to-host copy                                              */
	float ms_cigar_kernels;  /* bwagpu_batch_cigars: all its launches (the three tiers, NM/MD)                 */
	float ms_cigar_copy;     /* ... and the copies of the records and (bwagpu_batch_cigar_ops) the operation array */
	int64_t n_cig_cells;     /* bwagpu_batch_cigars (stats only): DP cells of the ksw_global2 fills with traceback, every band-doubling attempt counted */
	int64_t n_cig_dp;        /* ... and the number of such fills (regions answered by the gap-free comparison, bwa.c:171-174, do not count) */
	int32_t retry_mask;      /* OR of the overflow bits that made bwagpu_batch_run redo the batch: 2 slots, 4 B-tree nodes, 8 regions, 16 interval lists, 32 pass-2 task list */
	int32_t reserved_;
} bwagpu_stats_t;

/* Diagnostics: a marker of the step the handle's current (or last) batch call has reached; safe to call from another
 * thread while a call is in progress.  10-12 upload, 20+100*attempt run launched, 22+100*attempt run waiting, 30-39 download,
 * 40-45 cigars. */
int bwagpu_debug_phase(const bwagpu_t *h);
/* Diagnostics: sixteen event counters of the last batch_run; with stats on, [13..15] = wave iterations of the seeding kernel, those that
 * ran its bookkeeping code, and the lanes extending summed over iterations (tools/seed_iter_probe.py). */
int bwagpu_debug_prof(bwagpu_t *h, unsigned long long out[16]);
/* Diagnostics (stats on): where three kernels' time goes, read by read.  out[0..64): the seeding kernel -- out[b] = reads that took [2^(b-1), 2^b)
 * wave iterations, out[32 + b] = their iterations summed (tools/seed_iter_probe.py).  out[64..160): the wave-per-read extension kernel -- reads by
 * the time their wave spent on them (bin b: [2^(b-1), 2^b) x 10 ns), then per bin the ksw_extend2 calls and the DP cells (>> 10) of those reads;
 * out[160..256): the same for the wave-per-read de-duplication kernel (long reads) and its patch alignments. */
int bwagpu_debug_hist(bwagpu_t *h, unsigned long long out[256]);
/* Diagnostics (stats on): the seeding kernel's index-block look-ups by interval size.  out[0] / out[1] = forward / backward extension steps that read
 * index blocks, out[2] / out[3] = those whose interval is a single row (a unique match), out[4] / out[5] = maximal runs of such steps. */
int bwagpu_debug_seed_x2(bwagpu_t *h, unsigned long long out[8]);
/* Diagnostics: the prefix tables as the seeding kernels read them.  *m = their depth (0: none), *bytes = 16 m 4^m; with `out` non-NULL the entries are
 * copied there: entry [W * m + j - 1] = the j-base prefix of m-mer W (first base most significant) as four 32-bit words -- the low words of x0, x1, x2, then
 * their bits 32..36 in 5-bit fields and, in the top 16 bits, the prefix's change bits (bit k-1: its (k+1)-base prefix has another size than its k-base one). */
int bwagpu_debug_ptab(bwagpu_t *h, int32_t *m, uint64_t *bytes, void *out);
/* Diagnostics (stats on): the chaining kernel's reads by size and form.  out[t * 64 + b] = reads whose seeds were chained in form t (0: in registers,
 * 1: in the B-tree) with 16 b .. 16 b + 15 chains (before the chain filter) (b = 31: more); out[t * 64 + 32 + b] = with 32 b .. 32 b + 31 seeds.
 * out[128 .. 136] = the kernel's wave time in 10 ns ticks by phase (seed loop in registers, in the tree, repeat fraction + in-order list, weights, sort,
 * pairwise filter, publishing), the longest read, and the reads counted (tools/seed_iter_probe.py prints all of it). */
int bwagpu_debug_chain_hist(bwagpu_t *h, unsigned long long out[192]);

/* ---- differential tests of the device DP routines ----------------------------------------------------------------------- */
/* One case of bwagpu_debug_dp.  Sequences are nt4 codes in the call's `seqs` array: the query may hold 0..4, the target 0..3 (the
 * device reads targets from 2-bit packed reference text).  flags: bit 0 = present the query back to front, bit 1 = present the
 * target back to front, bit 2 = present the target's complement (read through the reverse-strand half of the text). */
typedef struct {
	int32_t q_off, q_len, t_off, t_len;
	int32_t w;               /* band width */
	int32_t h0;              /* kinds 0,1: ksw_extend2's h0; kind 4: ksw_align2's xtra word */
	int32_t end_bonus;       /* kinds 0,1 */
	int32_t flags;
} bwagpu_dp_case_t;
/* Runs one wavefront of a device DP routine per case, set up exactly as the product kernel sets it up, and returns 72 ints per
 * case.  kind 0: ksw_extend2 as k_extend_wave runs it for short reads (ksw.c:416; columns and read profile in LDS), kind 1: the
 * same in ring mode (long reads) -> {score, qle, tle, gtle, gscore, max_off, answered-without-DP, cells}; kind 2: ksw_global2 with
 * traceback as k_cigar runs it (ksw.c:540) -> {score, n_ops, ops...} (n_ops -1: more than 64 operations, -2: outside the kernel's
 * limits); kind 3: the score-only ksw_global2 of k_dedup_wave -> {score}; kind 4: ksw_align2 as k_matesw_sw runs it (ksw.c:379)
 * -> {score, te, qe, score2, te2, tb, qb}; kind 5: ksw_global2 with traceback as the long-segment kernel k_cigar_long runs it (columns
 * in an LDS ring, direction bytes in HBM, tiled traceback) -> {score, n_ops, up to 70 ops...} (n_ops may exceed 70: the first 70 are returned).  opt supplies the scoring (mat, gap costs, zdrop). */
int bwagpu_debug_dp(bwagpu_t *h, const bwagpu_opt_t *opt, int kind, int n_cases, const bwagpu_dp_case_t *cases, const uint8_t *seqs, int64_t n_seq_bytes, int32_t *out);

/* ---- differential tests of the device sorts ------------------------------------------------------------------------------ */
/* One element of a bwagpu_debug_sort case: a = the 64-bit part of the key (a region's end or start, an interval's info), b = score or weight,
 * c = query start.  A kind reads the fields its order is made of. */
typedef struct { int64_t a; int32_t b, c; } bwagpu_sort_key_t;
/* Runs one of the device's restatements of klib's ks_introsort (ksort.h:176-226) on n_cases cases -- case k is keys[off[k] .. off[k + 1]), off[0] = 0 --
 * where and as the product runs it, and returns per case the permutation it produced (perm[off[k] + place] = index of the element within its case;
 * -1 where nothing was written) and status[k]: 0 sorted, 1 the routine declined the case (dedup_read_par: a coordinate outside its packed keys),
 * -2 outside the entry's limits (kinds 7, 8: more than par_cap elements).
 * kind 0: one lane's introsort of b << 32 | index (mem_chain2aln's seed order, bwamem.c:684); 1: the same order by the wave-per-read kernel's routine (one
 * lane up to 32 seeds, a wave-wide network above); 2: k_publish's sort of intervals by a (bwamem.c:187); 3: k_publish_blk's (workgroup network up to 4096
 * intervals, one lane above); 4: chains by weight b, heaviest first (bwamem.c:367), pairs in LDS or HBM by size and chain_flt_lds; 5 / 6: regions by end a
 * (bwamem.c:467) / by (b descending, a, c) (bwamem.c:504) as the lane-per-read kernel sorts them; 7 / 8: the same two orders as dedup_read_par sorts them,
 * with its switches: dd_net (elements from which a network finishes the sort; 0: never) and par_cap (2 .. 1100: the elements its LDS arrays hold). */
/* The sizes at which the forms above change their method, as compiled: out[0] intervals up to which k_publish_blk sorts by its network, [1] chains whose
 * weight pairs fit the LDS area, [2] the largest chain_flt_lds, [3] regions from which the lane-per-read kernel sorts key records, [4] the largest par_cap,
 * [5] seeds up to which chain_sort_wave sorts on one lane, [6] the default of option dedup_net (dd_net), [7] 0. */
void bwagpu_debug_sort_limits(int32_t out[8]);
int bwagpu_debug_sort(bwagpu_t *h, int kind, int n_cases, const bwagpu_sort_key_t *keys, const int64_t *off, int dd_net, int par_cap, int chain_flt_lds, int32_t *perm, int32_t *status);

/* ---- optional widening past mem_process_seqs' first loop ---- */
/* After bwagpu_batch_download: one bwagpu_cigar_t per downloaded region, in the same order, computed on the device.  They
 * are what worker2's mem_reg2aln (bwamem.c:1119-1152) would compute on the host for that region; a finalize stage can use
 * them instead of calling bwa_gen_cigar2 (the records carry NM and the MD string as well, bwa.c:196-238).  Free with bwagpu_free. */
int bwagpu_batch_cigars(bwagpu_t *h, const bwagpu_opt_t *opt, bwagpu_cigar_t **out, int64_t *n_out);
/* Enable (1) / disable (0, default) a filter in bwagpu_batch_cigars: regions that overlap their read's best region (by mask_level, as
 * mem_mark_primary_se judges overlap, bwamem.c:519-545) and score below XA_drop_ratio times its score are not computed (reason 1).  Such a
 * region is neither printed nor listed in an XA tag (bwamem_extra.c:118-134) unless a third region stands between the two, so a finalize stage
 * that treats the records as hints loses nothing but the rare recomputation -- and the device skips its most expensive alignments. */
int bwagpu_set_cigar_filter(bwagpu_t *h, int enable);
/* The operation array of the last bwagpu_batch_cigars call (records with more than 6 operations point into it).  Free with bwagpu_free. */
int bwagpu_batch_cigar_ops(bwagpu_t *h, uint32_t **ops, int64_t *n_ops);
/* Test hook: the kernels of bwagpu_batch_cigars on reads (nt4 codes 0..4, n_reads + 1 offsets starting at 0) and region lists of the caller (read i: counts[i]
 * records of regs; with the filter of bwagpu_set_cigar_filter on, the first of them is the read's best region).  *cigs: one record per region, in the regions'
 * order; *ops: the operation array they point into, *n_ops entries.  Free both with bwagpu_free.  Needs no batch and leaves the records and operation array of
 * bwagpu_batch_cigars / bwagpu_batch_cigar_ops on the same handle alone.  BWAGPU_EINVAL (with bwagpu_last_error text): negative counts, offsets that do not
 * ascend, base codes above 4, qb < 0 or qe > the read's length, rb < 0 or re > 2 l_pac, e_del <= 0 or e_ins <= 0.  Shapes the kernels classify themselves come
 * back as records that were not computed: qe <= qb, rb >= re, rb < l_pac < re (reason 2), score below opt->T (reason 1). */
int bwagpu_cigars_flat(bwagpu_t *h, const bwagpu_opt_t *opt, int n_reads, const uint8_t *seqs, const int64_t *seq_off, const int32_t *counts, const bwagpu_alnreg_t *regs,
					   bwagpu_cigar_t **cigs, int64_t *n_cigs, uint32_t **ops, int64_t *n_ops);
/* The constants of the CIGAR kernels, as compiled: CIG_MAX_LEN, CIG_Z_SMALL, CIG_Z_BIG, CIG_MAX_COLS, CIG_MAX_OPS, CIG_TMP_OPS, CIG_MD_CAP (the LDS tiers: longest
 * segment, direction nibbles of the first and second tier, widest band, operations kept in a record, operations and MD characters a wavefront stages);
 * CIGL_MAX_COLS, CIGL_MAX_OPS, CIGL_QCAP (the long tier: widest band, most operations, query bases staged in LDS). */
void bwagpu_cigar_limits(int32_t out[10]);
/* Test hook: the de-duplication stage of bwagpu_batch_run (mem_sort_dedup_patch, bwamem.c:463-515) on reads (nt4 codes 0..4, n_reads + 1 offsets starting at
 * 0) and raw region lists of the caller (read i: counts[i] records of regs).  counts_out[i]: the regions read i is left with; *regs_out: those regions, read by
 * read in the stage's output order, *n_out of them (free with bwagpu_free); form[i] (may be NULL): the routine that finished read i -- 0 one lane (dedup_read),
 * 1 one wavefront on the records in place (dedup_read_wave), 2 one wavefront with the regions spread over its lanes (dedup_read_par).  The routine is chosen as
 * for a batch of these reads, from the handle's options (dedup_heavy, dedup_stage, dedup_big, dedup_net, dedup_wave, dedup_blk, dedup_ring).  Needs no batch
 * and leaves a batch's results on the same handle alone.  BWAGPU_EINVAL (with bwagpu_last_error text): negative counts, offsets that do not ascend, base codes
 * above 4, a region without 0 <= qb <= qe <= the read's length or 0 <= rb < re <= 2 l_pac, one that bridges l_pac, a rid beyond the index's contigs (negative
 * ones pass), e_del <= 0, e_ins <= 0 or w < 0. */
int bwagpu_dedup_flat(bwagpu_t *h, const bwagpu_opt_t *opt, int n_reads, const uint8_t *seqs, const int64_t *seq_off, const int32_t *counts, const bwagpu_alnreg_t *regs,
					  int32_t *counts_out, bwagpu_alnreg_t **regs_out, int64_t *n_out, int32_t *form);
/* The stage's switch points, as compiled: the defaults of options dedup_heavy, dedup_stage and dedup_net, DEDUP_KEYSORT_MIN (regions from which the in-place
 * sorts move keys), the regions dedup_read_par's scan takes at once, the reads k_dedup draws at once, the smallest ring of the patch alignments,
 * DDP_LDS_PER_REG (LDS bytes per region of dedup_read_par). */
void bwagpu_dedup_limits(int32_t out[8]);
/* The switch points of the extension stage (mem_chain2aln), as compiled: out[0] seeds up to which one lane sorts a chain's seeds (longer chains: the wavefront's
 * sorting network), [1] / [2] extended seeds of a chain kept in registers for the "other diagonal" rule by the short-read / the ring form (one more: the walk
 * over the sorted keys), [3] earlier regions of the read tested per step of the "already covered" rule, [4] the longest read of a batch that takes the
 * short-read form, [5] the widest ring of the ring form (4 w + 132 columns, rounded up to a power of two, beyond it: the lane-per-read kernel). */
void bwagpu_ext_limits(int32_t out[6]);
/* The switch points of the seeding stage (mem_collect_intv), as compiled: out[0] the deepest prefix table, [1] the depth in force for h's index (0: no tables; h may be
 * NULL: the default of option ptab_m) -- shorter matches are a bit mask of the lane when min_seed_len exceeds it --, [2] the most interval-stack entries per lane in LDS (the
 * default of option seed_lds_ent where the read copy leaves room: see [8], [9]), [3] the longest read of a batch whose reads are copied to LDS at 2 bits per base, [4] the longest read of a short-read batch,
 * [5] pass-1 entries whose pass-2 test the emitter remembers (later ones are read back from the list), [6] intervals of a read the workgroup-per-read sort takes,
 * [7] entries of a pass-1 task's interval stack in HBM, prefix-table depth included (the default of option seed_task_stack, in 32-byte units), [8] LDS bytes per lane of the seeding kernel: a short-read batch's 2-bit read copy (16 bytes per 64 bases of its
 * longest read, in steps of 16 bytes) comes first and 16-byte stack entries, [2] at the most, take the rest, [9] the entries in force in h's last bwagpu_batch_run
 * (0: none yet, or the stack wholly in HBM). */
void bwagpu_seed_limits(const bwagpu_t *h, int32_t out[10]);

/* After bwagpu_batch_download of a paired batch (mates interleaved 2i, 2i+1): the local alignments mem_matesw
 * (bwamem_pair.c:137-206) would run for every (anchor region, orientation) that the downloaded region lists do not already
 * satisfy, given the batch's insert-size windows.  A finalize stage looks results up by (read, anchor_rb, anchor_rid, r)
 * and runs ksw_align2 itself where there is none.  Free with bwagpu_free. */
int bwagpu_batch_matesw(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pes_t pes[4], bwagpu_matesw_t **out, int64_t *n_out);

/* Primary/secondary marking and mapping quality on the device: what worker2 does first with a read's regions,
 * mem_mark_primary_se (bwamem.c:519-584) followed by mem_approx_mapq_se (bwamem.c:982-1006).  One record per region, in the order
 * mem_mark_primary_se leaves the read's list; `hash` is not stored (it is hash_64(id + src), utils.h:98-109). */
typedef struct {
	int32_t src;            /* index of this region in the read's list as given / as downloaded */
	int32_t secondary, secondary_all, sub, alt_sc, sub_n;   /* as the reference leaves them (INT_MAX for an ALT hit's `secondary`, bwamem.c:571) */
	int32_t mapq;           /* mem_approx_mapq_se of the marked region, for every region (callers apply `secondary < 0 ? mapq : 0` themselves, bwamem.c:1061) */
	int32_t flags;          /* bit 0: a logarithm's argument was outside the handle's table; mapq was then computed by the host side of the call (it is right either way) */
} bwagpu_primary_t;
/* After bwagpu_batch_download: the records of every read of the batch, concatenated in read order with the download's counts.  Read i of the
 * batch has id id0 + i -- what mem_reg2sam (n_processed + i, bwamem.c:1227) and mem_sam_pe (id << 1 | r, bwamem_pair.c:349-350) pass for an even
 * n_processed.  n_pri[i] (may be NULL) = mem_mark_primary_se's return value for read i; *kernel_ms (may be NULL) = device time of the kernels
 * (HIP events).  Free *out with bwagpu_free.  BWAGPU_EINVAL before a download. */
int bwagpu_batch_primary(bwagpu_t *h, const bwagpu_opt_t *opt, int64_t id0, bwagpu_primary_t **out, int64_t *n_out, int32_t *n_pri, float *kernel_ms);
/* The same kernels on region lists the caller supplies (read i: counts[i] regions, concatenated in regs; ids[i] its id) -- for a finalize stage
 * that marks after it has merged mate-rescue hits on the host (bwamem_pair.c -> mem_sam_pe).  The regions' sub_n, csub, seedcov, frac_rep and
 * is_alt are read as given (the reference does not reset sub_n either).  *out: sum of counts records, free with bwagpu_free. */
int bwagpu_primary_flat(bwagpu_t *h, const bwagpu_opt_t *opt, int n_reads, const int32_t *counts, const bwagpu_alnreg_t *regs, const int64_t *ids,
						bwagpu_primary_t **out, int32_t *n_pri, float *kernel_ms);
/* The sizes at which the kernels change their method, as compiled: out[0] regions up to which one lane marks a read, [1] up to which a wavefront
 * does with its small LDS area, [2] with its large one (reads with more work in HBM scratch), [3] entries of the kept list compared per step. */
void bwagpu_primary_limits(int32_t out[4]);

/* Pairing of the two ends' hits on the device: mem_pair (bwamem_pair.c:208-269), the next thing worker2 does with a pair once both ends are marked. */
typedef struct { int32_t low, high, failed; double avg, std; } bwagpu_pestat_t;   /* == mem_pestat_t (bwamem.h:108-112), 32 bytes */
typedef struct {
	int32_t score, sub, n_sub;  /* mem_pair's return value, *sub and *n_sub */
	int32_t z[2];               /* places of the best pair's hits in the two ends' marked lists; {-1, -1} when there is no candidate (the reference leaves z untouched) */
	int32_t flags;              /* bit 0: a distance was outside the handle's table of log(2 erfc) values (option pair_tab_cap); the host side of the call then computed the record (it is right either way) */
	int64_t n_cand;             /* number of candidate pairs (u.n) */
} bwagpu_pair_t;
/* After bwagpu_batch_download of a batch whose reads 2p and 2p + 1 are mates: the marking kernels of bwagpu_batch_primary on the downloaded lists (read i
 * has id id0 + i; id0 must be even), then mem_pair of every pair on the device-resident records: place i of a read is region `src` of its i-th record, the
 * first n_pri places of each end take part, and pair p has id (id0 >> 1) + p truncated to int, as mem_sam_pe passes it (bwamem_pair.c:349-354).
 * *pairs: *n_pairs records, free with bwagpu_free.  pri / n_pri_recs (may be NULL) receive bwagpu_batch_primary's records (free with bwagpu_free), n_pri
 * (may be NULL) its return values, *kernel_ms (may be NULL) the device time of all kernels.  A pair one of whose ends has no primary-assembly hit gets the
 * no-candidate record (mem_sam_pe does not call mem_pair then).  BWAGPU_EINVAL: before a download, an odd number of reads, an odd id0, MEM_F_PRIMARY5 in
 * opt->flag (mem_reorder_primary5 between marking and pairing is not on the device), NULL h / opt / pes / pairs / n_pairs. */
int bwagpu_batch_pair(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pestat_t pes[4], int64_t id0, bwagpu_pair_t **pairs, int64_t *n_pairs,
					  bwagpu_primary_t **pri, int64_t *n_pri_recs, int32_t *n_pri, float *kernel_ms);
/* The same kernels on lists the caller has already marked (reads 2p, 2p + 1: counts[] regions each, concatenated in regs; the first n_pri[] of each take
 * part, the rest are ignored; ids[p] the pair's id) -- for a finalize stage that pairs after it has merged rescued hits.  Of a region rb, rid and score are
 * read.  *pairs: n_pairs records, free with bwagpu_free.  BWAGPU_EINVAL also for n_pri outside [0, counts] and a rid outside the index. */
int bwagpu_pair_flat(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pestat_t pes[4], int n_pairs, const int32_t *counts, const int32_t *n_pri,
					 const bwagpu_alnreg_t *regs, const int64_t *ids, bwagpu_pair_t **pairs, float *kernel_ms);
/* The numbers of hits of both ends at which the pairing kernels change their form, as compiled: out[0] up to which one lane does a pair, [1] up to which a
 * wavefront does with its small LDS area, [2] with its large one (pairs with more work in HBM scratch). */
void bwagpu_pair_limits(int32_t out[3]);

/* The merge of mate-rescue hits on the device: mem_matesw's decision loop as mem_sam_pe drives it (bwamem_pair.c:137-206, :291-302), between the download and
 * the marking.  For every pair (reads 2p, 2p + 1) the anchors are taken from the lists as downloaded, every rescue alignment the loop asks for is looked up among
 * the results of bwagpu_batch_matesw's kernels (or computed in place when the initial lists did not foresee it), hits are inserted and the list is sorted and
 * made non-redundant exactly as mem_sort_dedup_patch does without a reference. */
typedef struct {
	int32_t n_aligned;   /* mem_sam_pe's n for this pair (alignments run); -1 when flagged */
	int32_t n_inline;    /* of those, computed inside the rescue kernel (no precomputed record) */
	int32_t flags;       /* bit 0: a mate longer than the SW kernel's limit or a window beyond it: lists returned as downloaded, caller rescues itself */
	int32_t pad_;
} bwagpu_rescue_t;
/* After bwagpu_batch_download of a batch whose reads 2p and 2p + 1 are mates (read i has id id0 + i, id0 even).  counts[i]: the length of read i's merged list;
 * *regs: the merged lists, concatenated, in the order mem_sam_pe has them when it reaches mem_mark_primary_se (every byte as the reference's: a rescued hit is
 * zero outside rid, is_alt, qb, qe, rb, re, score, csub, secondary = -1, seedcov, and n_comp, which is 1 once a sort of two or more regions has run over the list and 0 for a hit put into an empty list); *src: one entry per merged region, its index
 * in that read's downloaded list, or -1 - (j << 2 | r) for a hit rescued from anchor j of the other end (the j-th of its regions within pen_unpaired of its best)
 * in orientation r; *rescue: n / 2 records.  pri / n_pri (may be NULL): what bwagpu_primary_flat returns for the merged lists; pairs (may be NULL): what
 * bwagpu_pair_flat returns for those records (pair p has id (id0 >> 1) + p).  A flagged pair's lists, and its records, are those of the download.
 * MEM_F_NO_RESCUE in opt->flag: the lists come back unchanged with n_aligned = 0.  Everything returned is freed with bwagpu_free.  BWAGPU_EINVAL: before a
 * download, an odd number of reads, an odd id0, a NULL h / opt / pes / counts / regs / src / n_regs / rescue, MEM_F_PRIMARY5 together with pairs. */
int  bwagpu_batch_rescue(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pestat_t pes[4], int64_t id0,
		int32_t *counts /* n reads: merged list lengths */, bwagpu_alnreg_t **regs, int32_t **src, int64_t *n_regs,
		bwagpu_rescue_t **rescue /* n/2 */,
		bwagpu_primary_t **pri, int32_t *n_pri,      /* may be NULL: marking of the merged lists */
		bwagpu_pair_t **pairs,                       /* may be NULL: mem_pair on those records */
		float *kernel_ms);
/* The same kernels on reads and lists of the caller: 2 n_pairs reads (nt4 codes 0..4, read i at seqs[off[i] .. off[i + 1])), counts_in[i] regions each,
 * concatenated in regs_in (rid inside the index); ids: one per read (a pair's id is ids[2p] >> 1), may be NULL when pri and pairs are. */
int  bwagpu_rescue_flat(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pestat_t pes[4], int n_pairs,
		const uint8_t *seqs, const int64_t *off,                       /* 2 n_pairs reads, nt4 */
		const int32_t *counts_in, const bwagpu_alnreg_t *regs_in, const int64_t *ids /* per read; may be NULL when pri and pairs are */,
		int32_t *counts, bwagpu_alnreg_t **regs, int32_t **src, int64_t *n_regs, bwagpu_rescue_t **rescue,
		bwagpu_primary_t **pri, int32_t *n_pri, bwagpu_pair_t **pairs, float *kernel_ms);
/* The sizes at which the kernels change their form, as compiled: out[0] the capacity of a pair's larger end (its regions plus four per anchor of the other end) up to
 * which one lane replays the pair, [1] up to which a wavefront does with its sort keys in LDS (larger pairs: keys in HBM scratch); [2], [3] are zero. */
void bwagpu_rescue_limits(int32_t out[4]);

/* The insert-size windows on the device: mem_pestat (bwamem_pair.c:72-135), the step of the paired-end path that needs the whole batch (bwamem.c:1258) and
 * whose result, pes[4], every call above takes.  A kernel with one lane per pair (reads 2p, 2p + 1; a trailing unpaired read is ignored) applies the filter of
 * :78-90 and counts the insert sizes into a histogram of 4 x (max_ins + 1) bins; a second kernel reads the order statistics, the mean, the standard deviation and
 * the windows off the histogram.  pes is byte for byte the reference's mem_pestat_t[4], padding zero.  The histograms of several shards add, bin by bin. */
typedef struct {            /* what mem_pestat prints and what its scalars were made from */
	int64_t n[4];           /* candidate unique pairs per orientation (isize[d].n) */
	int32_t p25[4], p50[4], p75[4];
	int32_t lo_out[4], hi_out[4];   /* bounds used for mean and std.dev (:106-108) */
	int64_t x[4];           /* values inside them */
	double  sum[4], sumsq[4];       /* avg = sum / x, std = sqrt(sumsq / x) */
} bwagpu_pestat_info_t;     /* (fields of an orientation with fewer than MIN_DIR_CNT pairs are zero, n apart) */
/* After bwagpu_batch_download (the preconditions of bwagpu_batch_primary): mem_pestat of the downloaded lists.  info and kernel_ms (device time of both kernels,
 * HIP events) may be NULL.  A batch without any region, fewer than two reads, or opt->max_ins <= 0: four failed orientations, nothing is launched.  The result
 * also stays in a device buffer of the handle.  BWAGPU_EINVAL: before a download, NULL h / opt / pes, opt->max_ins above the limit (bwagpu_pestat_limits; see
 * bwagpu_last_error -- the caller keeps its host function for that case). */
int  bwagpu_batch_pestat(bwagpu_t *h, const bwagpu_opt_t *opt, bwagpu_pestat_t pes[4], bwagpu_pestat_info_t *info, float *kernel_ms);
/* The same kernels on lists of the caller (read i: counts[i] regions, concatenated in regs; of a region qb, qe, score, rid and rb are read). */
int  bwagpu_pestat_flat (bwagpu_t *h, const bwagpu_opt_t *opt, int n_reads, const int32_t *counts, const bwagpu_alnreg_t *regs,
                         bwagpu_pestat_t pes[4], bwagpu_pestat_info_t *info, float *kernel_ms);
/* The first kernel alone, for a batch cut over several handles: *hist receives the 4 * (max_ins + 1) counts of this handle's downloaded lists, orientation by
 * orientation (*n_bins of them; 0 for a negative max_ins); free with bwagpu_free.  Preconditions and errors as bwagpu_batch_pestat. */
int  bwagpu_batch_pestat_hist(bwagpu_t *h, const bwagpu_opt_t *opt, uint32_t **hist, int64_t *n_bins, float *kernel_ms);  /* 4 * (max_ins + 1) counts; bwagpu_free */
/* The second kernel alone on a histogram of the caller -- the element-wise sum of the shards' -- on any handle, before or after a run.  BWAGPU_EINVAL also for
 * n_bins other than 4 * (max_ins + 1) and for 2^31 or more pairs in one orientation.  _hist followed by _finish on one handle is bwagpu_batch_pestat. */
int  bwagpu_pestat_finish(bwagpu_t *h, const bwagpu_opt_t *opt, const uint32_t *hist, int64_t n_bins,
                          bwagpu_pestat_t pes[4], bwagpu_pestat_info_t *info, float *kernel_ms);
void bwagpu_pestat_limits(int32_t out[2]);   /* MIN_DIR_CNT, largest max_ins served (1 << 22) */

/* The alignment list of a read on the device: per region of the marked list what mem_reg2aln (bwamem.c:1119-1189) returns for it, and per read what the loop
 * of mem_reg2sam (bwamem.c:1045-1062) makes of those results.  The CIGAR is not recomputed: from a record and the region's bwagpu_cigar_t a caller writes the
 * final CIGAR (clip5, then the record's operations without the dropped deletion, then clip3), NM, MD, AS, XS and the SA / XA fields. */
#define BWAGPU_ALN_NOCIGAR 0x1   /* the region's CIGAR record has n_cigar == -1: pos, n_cigar and nm are not final, the caller runs mem_reg2aln for this region */
#define BWAGPU_ALN_REV     0x2   /* is_rev */
#define BWAGPU_ALN_ALT     0x4   /* is_alt */
#define BWAGPU_ALN_DEL5    0x8   /* the CIGAR record's first operation, a deletion, is dropped (pos has moved by its length) */
#define BWAGPU_ALN_DEL3    0x10  /* the CIGAR record's last operation, a deletion, is dropped */
typedef struct {
	int64_t pos;            /* on contig rid; -1 for an unmapped region (rb < 0 || re < 0: rid -1, flag 0x4) */
	int32_t rid;
	int32_t flag;           /* 0x100 for a secondary; 0x800 or (MEM_F_NO_MULTI) 0x10000 for every printed non-secondary after the first; the caller ORs its extra_flag */
	int32_t mapq;           /* mem_reg2aln's (0 for a secondary): what an XA entry of the region prints */
	int32_t mapq_out;       /* what the region's own line prints: mapq capped by aa[0]'s unless MEM_F_KEEP_SUPP_MAPQ is set or the hit is ALT */
	int32_t nm;             /* of the CIGAR record */
	int32_t n_cigar;        /* final: the record's operations without a dropped deletion, plus the clips */
	int32_t score, sub;     /* sub = max(sub, csub); -1 for a printed secondary */
	int32_t alt_sc;
	int32_t sel;            /* place of the region in mem_reg2sam's list `aa`, or -1 where one of its three tests skips the region */
	int32_t clip5, clip3;   /* by strand; 0: none */
	int32_t flags;          /* BWAGPU_ALN_* */
	int32_t pad_;           /* zero */
} bwagpu_aln_t;             /* 64 bytes */
/* After bwagpu_batch_download AND bwagpu_batch_cigars of the same batch: the marking kernels of bwagpu_batch_primary on the downloaded lists (read i has id
 * id0 + i), then one record per downloaded region, in marked order per read (record k of a read belongs to region `src` of its k-th marking record).
 * n_aln[i] (may be NULL) = aa.n of read i; 0: the caller writes the unmapped record.  pri / n_pri (may be NULL) receive bwagpu_batch_primary's records and
 * return values; *kernel_ms (may be NULL) the device time of all kernels (HIP events, summed over the segments).  Free *alns and *pri with bwagpu_free.
 * BWAGPU_EINVAL: before a download, without CIGAR records for this download, MEM_F_PRIMARY5 in opt->flag (mem_reorder_primary5 between marking and
 * mem_reg2sam is not on the device), NULL h / opt / alns / n_alns. */
int bwagpu_batch_alns(bwagpu_t *h, const bwagpu_opt_t *opt, int64_t id0, bwagpu_aln_t **alns, int64_t *n_alns, int32_t *n_aln,
					  bwagpu_primary_t **pri, int32_t *n_pri, float *kernel_ms);
/* The same kernels on unmarked lists of the caller (as bwagpu_primary_flat: read i has counts[i] regions in regs and id ids[i]) with read_len[i] bases; cigs:
 * one CIGAR record per region, in the regions' order, pointing into the n_ops entries of ops (the layout bwagpu_batch_cigars / bwagpu_batch_cigar_ops
 * deliver).  *alns: sum of counts records.  BWAGPU_EINVAL also for a region's rid outside the index, an n_cigar outside [-1, 32768], a reference to
 * operations outside [0, n_ops) and a negative read_len. */
int bwagpu_alns_flat(bwagpu_t *h, const bwagpu_opt_t *opt, int n_reads, const int32_t *counts, const bwagpu_alnreg_t *regs, const int64_t *ids, const int32_t *read_len,
					 const bwagpu_cigar_t *cigs, const uint32_t *ops, int64_t n_ops, bwagpu_aln_t **alns, int32_t *n_aln, bwagpu_primary_t **pri, int32_t *n_pri, float *kernel_ms);
/* out[0] regions up to which one lane makes a read's list, out[1] regions a wavefront takes per step */
void bwagpu_alns_limits(int32_t out[2]);
int  bwagpu_aln_size(void);   /* sizeof(bwagpu_aln_t) as compiled */

/* The SAM text of single-end reads on the device: mem_aln2sam (bwamem.c:851-976) of every record mem_reg2sam lists for a read (m == NULL), the XA / XB strings
 * of mem_gen_alt included, written by one kernel straight from the resident alignment, marking and CIGAR records.  The handle needs the contigs' names:
 * bwagpu_create_from_files takes them (and the annotations) from .ann; a caller of bwagpu_create sets them once, before it clones the handle. */
/* names / annos: the bytes of all names / annotations back to back, without terminators; contig i's are [name_off[i], name_off[i + 1]), n_seqs + 1 ascending
 * offsets each.  annos may be NULL (no annotations: no XR tag).  bwagpu_clone shares them, bwagpu_clone_to_device copies them. */
int bwagpu_set_contig_names(bwagpu_t *h, const char *names, const int64_t *name_off, const char *annos, const int64_t *anno_off);
typedef struct {
	const char *names;    const int64_t *name_off;     /* n_reads + 1 ascending offsets; no terminators */
	const char *quals;                                  /* NULL: '*'; else one byte per base at the reads' own offsets */
	const char *comments; const int64_t *comment_off;   /* NULL: none; an empty comment prints nothing (bseq_read leaves it NULL) */
	const char *rg_id;                                  /* NULL or "": none */
	int32_t extra_flag;
} bwagpu_sam_in_t;
typedef struct {
	char *text;           int64_t n_text;               /* the batch's text: the lines of read i are text[off[i] .. off[i + 1]), in read order */
	int64_t *off;                                       /* n_reads + 1 */
	int32_t *flags;                                     /* per read; bit 0: declined -- no bytes, the caller formats the read */
	int32_t *n_lines;     int64_t n_declined;           /* lines per read (0 for a declined one) */
	float kernel_ms[3];                                 /* device time: marking + alignment lists, sizing + prefix sum, writing */
} bwagpu_sam_out_t;                                     /* text, off, flags and n_lines are freed with bwagpu_free, each */
/* After bwagpu_batch_download and bwagpu_batch_cigars of the same batch (bwagpu_batch_alns' preconditions): the kernels of bwagpu_batch_alns, whose records
 * stay on the device, then two passes of one formatter -- bytes per read, a prefix sum, the text.  Read i has id id0 + i.  A read is declined when a region it
 * prints, or one it lists in a printed XA, has no CIGAR record (BWAGPU_ALN_NOCIGAR); nothing else is.  A read without regions prints the unmapped record.
 * Host waits: those of the marking, one for the total size, one for the final copy.  BWAGPU_EINVAL: bwagpu_batch_alns' cases, a handle without contig names
 * (see bwagpu_last_error), NULL in / out / names / name_off, comments without comment_off, offsets that do not ascend. */
int bwagpu_batch_sam(bwagpu_t *h, const bwagpu_opt_t *opt, int64_t id0, const bwagpu_sam_in_t *in, bwagpu_sam_out_t *out);
/* The same on reads (nt4, n_reads + 1 offsets: `quals` follows them), lists, ids, CIGAR records and operation array of the caller: bwagpu_alns_flat's
 * arguments and checks, and an MD string outside the operation array is BWAGPU_EINVAL too. */
int bwagpu_sam_flat(bwagpu_t *h, const bwagpu_opt_t *opt, int n_reads, const uint8_t *seqs, const int64_t *seq_off, const int32_t *counts, const bwagpu_alnreg_t *regs,
					const int64_t *ids, const bwagpu_cigar_t *cigs, const uint32_t *ops, int64_t n_ops, const bwagpu_sam_in_t *in, bwagpu_sam_out_t *out);
/* out[0] bytes of a wavefront's staging area (a longer line is flushed in its middle), out[1] places of a marked list a wavefront takes per step */
void bwagpu_sam_limits(int32_t out[2]);

/* A read pair decided on the device: everything mem_sam_pe (bwamem_pair.c:276-419) does behind mem_pair except the text.  The merge of the mate-rescue hits,
 * the marking and the pairing are bwagpu_batch_rescue's; then one record per pair says which of the two ways out the pair takes and what it prints, the marking
 * records are patched as mem_sam_pe patches the lists (:335-336, :350-359), every merged region gets its CIGAR record (bwagpu_batch_cigars' kernels) and its
 * bwagpu_aln_t.  What is left to the caller is the CIGAR / MD / XA text and mem_aln2sam. */
typedef struct {
	int32_t path;           /* 0: printed by :311-394 (the pair is taken from the lists by z / alt); 1: by no_pairing, :397-418 (two mem_reg2sam lists); -1: not decided (flags bit 0) */
	int32_t why;            /* path 1: the reason, in the reference's order of evaluation -- 1: MEM_F_NOPAIRING; 2: an end has n_pri == 0; 4: mem_pair returned <= 0;
	                         * 8 / 16: is_multi[0] / is_multi[1] (these two may come together; a later reason is not looked for once an earlier one holds) */
	int32_t extra_flag;     /* 1 or 3: the reference's variable on either path */
	int32_t z[2];           /* path 0: place of h[i] in end i's marked list (0 where the unpaired alignment is preferred, :346); path 1: `which` of :399-404, -1: the unmapped record */
	int32_t q_se[2];        /* path 0: h[i].mapq as :337-348 leave it; path 1: mem_reg2aln's mapq of `which` (0: unmapped) -- what the mate's MQ tag prints */
	int32_t alt[2];         /* path 0: place of g[i] (n_pri[i]) where :371-377 print it, else -1; path 1: -1 */
	int32_t n_aa[2];        /* lines the end prints.  path 0: 1 or 2; path 1: aa.n of mem_reg2sam's loop, 0 = the unmapped line */
	int32_t q_pe;           /* after :329; 0 on path 1 */
	int32_t paired;         /* path 0: 1 where o > score_un (:331) */
	int32_t flags;          /* bit 0: bwagpu_batch_rescue declined the pair (its flags & 1): every other field but path is zero, the caller runs mem_sam_pe itself on the download's lists;
	                         * bit 1: the host side of the call computed this record or the pair record it was made from (a logarithm outside the handle's table, a distance outside the pairing table); it is right either way */
	int32_t pad_[2];        /* zero */
} bwagpu_sampe_t;          /* 64 bytes */
/* What the two calls below return.  Every array is freed with bwagpu_free; after a failure all of them are NULL. */
typedef struct {
	bwagpu_alnreg_t *regs; int32_t *src; int64_t n_regs;   /* the merged lists, as bwagpu_batch_rescue returns them */
	bwagpu_rescue_t *rescue;                                /* n / 2 */
	bwagpu_primary_t *pri;                                  /* n_regs marking records of the merged lists AS mem_sam_pe LEAVES THE LISTS: bwagpu_batch_rescue's except for the chosen hit's
	                                                         * sub, secondary = -2 and mapq (recomputed from the new sub) where :335-336 fired, and the switched group's secondary_all (:350-359) */
	int32_t *n_pri;                                         /* n */
	bwagpu_pair_t *pairs;                                   /* n / 2 */
	bwagpu_sampe_t *sampe;                                  /* n / 2 */
	bwagpu_cigar_t *cigs;                                   /* one per merged region, in the merged lists' order */
	uint32_t *ops; int64_t n_ops;                           /* the operation array of cigs */
	bwagpu_aln_t *alns;                                     /* one per merged region, in marked order.  An end of a path-1 pair: as bwagpu_batch_alns (the caller ORs 0x40 << i | extra_flag).  An end of a
	                                                         * path-0 pair: sel = 0 at place z[i] with mapq_out = q_se[i], sel = 1 and flag |= 0x800 at alt[i], sel = -1 elsewhere; sub as mem_reg2aln leaves it */
	int32_t *n_aln;                                         /* n: lines per read (= sampe's n_aa) */
	float kernel_ms[6];                                     /* device time (HIP events, summed per segment) of rescue, marking, pairing, decision, CIGAR and alignment-list kernels.  [4] is what bwagpu_batch_cigars reports as ms_cigar_kernels:
	                                                         * one span over its tiers, which contains the long tier's sizing copy with its host wait and, after an overflow of the operation array, the second attempt */
} bwagpu_pe_out_t;
/* After bwagpu_batch_download of a batch whose reads 2p, 2p + 1 are mates (read i has id id0 + i, id0 even); needs no bwagpu_batch_cigars call and leaves the records of an earlier
 * one (and what bwagpu_batch_alns makes of them) alone.  counts[i]: the length of read i's merged list.  BWAGPU_EINVAL: bwagpu_batch_rescue's cases, MEM_F_PRIMARY5 in opt->flag, a NULL out.
 * MEM_F_NO_RESCUE in opt->flag (bwamem.h:44) is honoured as the reference honours it: the lists pass unchanged. */
int  bwagpu_batch_sampe(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pestat_t pes[4], int64_t id0, int32_t *counts, bwagpu_pe_out_t *out);
/* The same kernels on reads and lists of the caller: the inputs of bwagpu_rescue_flat, ids required. */
int  bwagpu_sampe_flat(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pestat_t pes[4], int n_pairs, const uint8_t *seqs, const int64_t *off,
		const int32_t *counts_in, const bwagpu_alnreg_t *regs_in, const int64_t *ids, int32_t *counts, bwagpu_pe_out_t *out);
/* out[0] regions of a pair's longer list up to which one lane decides the pair (the marking kernel's value), out[1] places a wavefront takes per step */
void bwagpu_sampe_limits(int32_t out[2]);
int  bwagpu_sampe_size(void);   /* sizeof(bwagpu_sampe_t) as compiled */

/* The SAM text of read pairs on the device: what mem_sam_pe prints (bwamem_pair.c:360-385, :397-415) -- mem_aln2sam with a mate: flag bits 0x1 / 0x8 / 0x20 /
 * 0x40 / 0x80 and the pair's extra_flag, the two copy rules for an unmapped end, RNEXT / PNEXT / TLEN, MC:Z: and MQ:i:.  The kernels of bwagpu_batch_sampe run
 * first; the formatter of bwagpu_batch_sam then reads their resident records (alignment, patched marking and CIGAR records, the pair records), one wavefront per
 * read.  `in` describes all 2 * n_pairs reads; in->extra_flag is ORed into every line.  With pe == NULL the alignment records, the marking records and the
 * operation array do not come to the host; with pe the pair output is exactly bwagpu_batch_sampe's.  A pair is declined as a whole (no bytes, bit 0 of both reads'
 * flag words; the caller runs mem_sam_pe's text for it): its bwagpu_sampe_t has flags & 1 or path < 0, or an end is declined by bwagpu_batch_sam's rule, or
 * an end's mate place (z[1 - i]) has BWAGPU_ALN_NOCIGAR; nothing else is.  out->kernel_ms[0] is the sum of bwagpu_batch_sampe's six segments.
 * BWAGPU_EINVAL: bwagpu_batch_sampe's cases, bwagpu_batch_sam's (contig names, offsets), and mates whose names differ (bwagpu_last_error names the pair; the
 * reference dies on them) -- all checked before anything is launched. */
int  bwagpu_batch_sam_pe(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pestat_t pes[4], int64_t id0, const bwagpu_sam_in_t *in, int32_t *counts,
		bwagpu_pe_out_t *pe /* may be NULL */, bwagpu_sam_out_t *out);
/* The same on reads and lists of the caller: bwagpu_sampe_flat's inputs; in->quals follows `off`. */
int  bwagpu_sam_pe_flat(bwagpu_t *h, const bwagpu_opt_t *opt, const bwagpu_pestat_t pes[4], int n_pairs, const uint8_t *seqs, const int64_t *off,
		const int32_t *counts_in, const bwagpu_alnreg_t *regs_in, const int64_t *ids, const bwagpu_sam_in_t *in, int32_t *counts,
		bwagpu_pe_out_t *pe /* may be NULL */, bwagpu_sam_out_t *out);
/* as bwagpu_sam_limits */
void bwagpu_sam_pe_limits(int32_t out[2]);

/* ---- index construction on the device -------------------------------------------------------- */
/* The arrays `bwa index` leaves in bwt_t after bwt_bwtgen2/bwt_pac2bwt + bwt_bwtupdate_core + bwt_cal_sa
 * (bwtindex.c:64-120, 150-172; bwt.c:62-84), built from the 2-bit packed forward strand by a suffix sort in HBM
 * (bwagpu_index.hip).  bwt/sa are malloc()ed; free with bwagpu_built_free.  Written with the 40/56-byte headers of
 * bwt_dump_bwt / bwt_dump_sa (bwt.c:385-407) they are byte-identical to the reference's .bwt/.sa files. */
typedef struct {
	uint32_t *bwt;           /* bwt_t::bwt: Occ checkpoints interleaved with 2-bit symbols, bwt_size words */
	uint64_t bwt_size;
	uint64_t *sa;            /* bwt_t::sa: n_sa entries, sa[0] = (uint64_t)-1 */
	uint64_t n_sa;
	int sa_intv;
	uint64_t primary, L2[5], seq_len;
	float build_ms;          /* device time of the whole construction (HIP events) */
} bwagpu_built_t;
/* pac: the reference's .pac layout (bntseq.c:229-230), forward strand, l_pac bases, no ambiguity codes (bns_fasta2bntseq
 * replaces them before packing, bntseq.c:266,295-296).  sa_intv: power of two (the reference uses 32, bwtindex.c:316).
 * On failure a message is copied to errbuf (may be NULL). */
int bwagpu_index_build(const uint8_t *pac, int64_t l_pac, int sa_intv, int device, bwagpu_built_t *out, char *errbuf, size_t errlen);
void bwagpu_built_free(bwagpu_built_t *b);

/* ---- FASTA -> .pac/.ann/.amb on the device (what bns_fasta2bntseq computes, bntseq.c:280-333) ------------------------------- */
/* A streaming parser: begin, feed the FASTA text (uncompressed) in pieces of any size, end.  The per-byte work -- which bytes
 * are bases, their codes (ambiguity codes replaced by the lrand48() stream after srand48(11), as bwa index does), the holes --
 * runs on the device in chunks of chunk_bytes (<= 0: 256 MiB); the host parses the header lines.  Input that the reference
 * reads as FASTQ or does not define (an '@' before the first '>', a sequence line starting with '+' or '@', a NUL or a byte
 * >= 0x80 in a sequence line, no record, no base, a contig or hole of 2^31 bases or more) fails with BWAGPU_EINVAL and a
 * message naming the byte offset.  After a failure the parser only accepts bwagpu_fasta_end (which reports it again).
 * bwagpu_fasta_end always releases the parser and its device memory; the result's arrays are freed with bwagpu_fasta_free
 * (each is also freeable with bwagpu_free).  result.pac goes to bwagpu_index_build unchanged. */
typedef struct bwagpu_fasta_parser_s bwagpu_fasta_parser_t;
typedef struct {
	uint8_t *pac;            /* forward strand, l_pac / 4 + 1 bytes in the .pac layout (bntseq.c:229) */
	int64_t l_pac;
	int32_t n_seqs;
	int64_t *seq_offset;     /* per contig: bntann1_t offset, len, n_ambs */
	int32_t *seq_len, *seq_n_ambs;
	char *names;             /* per contig: name NUL anno NUL (anno "(null)" for an empty comment, as bntann1_t::anno) */
	int64_t names_bytes;
	int64_t n_holes;
	int64_t *hole_offset;    /* per hole: bntamb1_t offset, len, amb */
	int32_t *hole_len;
	char *hole_amb;
	float parse_ms;          /* device time of the parse kernels */
} bwagpu_fasta_t;
int bwagpu_fasta_begin(bwagpu_fasta_parser_t **p, int device, int64_t chunk_bytes, char *errbuf, size_t errlen);
int bwagpu_fasta_feed(bwagpu_fasta_parser_t *p, const void *data, int64_t len, char *errbuf, size_t errlen);
int bwagpu_fasta_end(bwagpu_fasta_parser_t *p, bwagpu_fasta_t *out, char *errbuf, size_t errlen);
void bwagpu_fasta_free(bwagpu_fasta_t *r);

/* ---- FASTQ batches on the device (what bseq_read delivers, bwa.c:79-112 over kseq.h:175-215) --------------------------------- */
/* A parser of its own (no index, no bwagpu_t).  A call takes a window of the uncompressed FASTQ text of one file, or of two files
 * of mates, each starting at a record start, and returns the batch bseq_read(chunk_size) would cut from there: records parsed as
 * kseq_read parses them, trim_readno applied, bases recoded by nst_nt4_table, two files interleaved as reads 2i, 2i + 1 -- in the
 * layouts bwagpu_batch_upload (seqs, off) and bwagpu_sam_in_t (names, name_off, quals, comments, comment_off) take.
 * The device reads PLAIN records only: four lines with all four newlines, '@' first, the third line starting with '+', sequence and
 * quality of the same non-zero length, no '\r' before the first, second or fourth newline, a sequence line that does not start with
 * '>', '+' or '@' and holds no byte <= ' ' and none >= 0x80.  Every record before the first one that is not plain is read exactly
 * as the reference reads it (dev_fastq.h has the argument); at that record the device stops and says where.
 *   BWAGPU_FQ_CUT       the cut was reached: the batch is complete.  A non-plain record behind the cut does not matter.
 *   BWAGPU_FQ_END       every eof flag is set, every byte of every window became a record and (two windows) both hold the same number
 *                       of records: the batch is the rest of the input (n_reads == 0 for empty windows; arrays are still delivered).
 *   BWAGPU_FQ_MORE      a window without eof ran out before the cut and held no non-plain record: nothing is delivered, the caller
 *                       repeats the call from the same start with a longer window.
 *   BWAGPU_FQ_DECLINED  before the cut there is a non-plain record, an incomplete last record at eof (a missing final newline included),
 *                       or one window ends at eof while the other has records left (the reference's "fewer sequences" cases): n_reads == 0,
 *                       no arrays; declined_file / declined_at: the window and the byte offset in it of the first record not taken.  The
 *                       caller reads this batch with a reader of its own.
 * consumed[k]: bytes of window k that became the batch's records (CUT, END); the next call's window starts there.
 * Host waits: one for the counts and total sizes, one for the final copies.  Device buffers only grow.  The arrays come from the
 * result pool: release them with bwagpu_fastq_out_free (or bwagpu_free, each).
 * BWAGPU_EINVAL: NULL p / raw1 / out, a negative length, a window of 2^31 bytes or more, chunk_size <= 0, raw2 == NULL with len2 != 0. */
typedef struct bwagpu_fastq_parser_s bwagpu_fastq_parser_t;
enum { BWAGPU_FQ_CUT = 0, BWAGPU_FQ_END = 1, BWAGPU_FQ_MORE = 2, BWAGPU_FQ_DECLINED = 3 };
typedef struct {
	int32_t file, has_comment;      /* window index (0 / 1); the header had a delimiter behind the name */
	int32_t name, l_name;           /* window offsets and lengths: the name (trim_readno applied), */
	int32_t comment, l_comment;     /* the comment (l_comment may be 0 with has_comment set), */
	int32_t seq, l_seq;             /* the bases, */
	int32_t qual, l_qual;           /* the qualities (l_qual == l_seq) */
} bwagpu_fastq_rec_t;              /* 40 bytes */
typedef struct {
	int32_t status, n_reads;
	int64_t consumed[2];            /* bytes of window k that became this batch's records */
	int32_t declined_file; int64_t declined_at;   /* DECLINED: which window, byte offset of the first record not taken */
	uint8_t *seqs;  int64_t *off;                  /* nt4, n_reads + 1: what bwagpu_batch_upload reads; seqs from bwagpu_alloc_host's pool */
	char *names;    int64_t *name_off;             /* bwagpu_sam_in_t's layouts, trim_readno applied */
	char *quals;                                   /* at the reads' own offsets */
	char *comments; int64_t *comment_off; uint8_t *has_comment;   /* has_comment[i]: the header had a delimiter (the comment may be empty) */
	bwagpu_fastq_rec_t *recs;                      /* per read: window index, offsets and lengths of its four fields in the window */
	float kernel_ms[3];                            /* newline + check passes, cut, emit */
} bwagpu_fastq_out_t;
int  bwagpu_fastq_begin(bwagpu_fastq_parser_t **p, int device, char *errbuf, size_t errlen);
/* device buffers for two windows of window_bytes each, ahead of the first call (BWAGPU_ENOMEM leaves the parser usable) */
int  bwagpu_fastq_reserve(bwagpu_fastq_parser_t *p, int64_t window_bytes);
int  bwagpu_fastq_batch(bwagpu_fastq_parser_t *p, const void *raw1, int64_t len1, int eof1,
                        const void *raw2 /* NULL: one file */, int64_t len2, int eof2,
                        int chunk_size, bwagpu_fastq_out_t *out);
const char *bwagpu_fastq_last_error(const bwagpu_fastq_parser_t *p);
void bwagpu_fastq_out_free(bwagpu_fastq_out_t *out);
void bwagpu_fastq_end(bwagpu_fastq_parser_t *p);
int  bwagpu_fastq_rec_size(void);   /* sizeof(bwagpu_fastq_rec_t) as compiled */

/* ---- BGZF input inflated on the device (bgzip's block-compressed gzip, SAM specification 4.1), on the same parser ------------- */
/* A window here is COMPRESSED bytes that start at a BGZF block start.  The library walks the block headers on the host: a block is a
 * gzip member (magic 1f 8b, CM 8, FEXTRA set) with a `BC' subfield of length 2 anywhere among its extra subfields whose BSIZE is
 * consistent with XLEN and lies within the bytes in view; its trailer holds CRC-32 and ISIZE.  Whole blocks are taken for as long as
 * their ISIZEs sum to less than 2^31; what was not taken is as if it were not in the window (eof then does not apply to this call).
 * A trailing partial block without eof is left for the next call; with eof, it -- or bytes that are no block -- is damage.  Empty
 * blocks (bgzip's 28-byte end-of-file marker, anywhere) are ordinary.  The compressed bytes and a table of the blocks go up, every
 * block is inflated by one wavefront (dev_bgzf.h) and tested as zlib's inflate(Z_FINISH) plus the trailer test it: all three block
 * types, any number of deflate blocks, unused payload bytes behind the final one allowed; block type 3, LEN != ~NLEN, HLIT > 286,
 * HDIST > 30, an over-subscribed or (but for zlib's one-bit exception) incomplete code, no end-of-block code, symbols 286 / 287 / 30 /
 * 31, a distance before the block's own text, a stream that runs past the payload, text longer or shorter than ISIZE, ISIZE above
 * 65536 and a CRC-32 that differs are damage.  A damaged block ends in a status, never in an access outside its buffers.
 *
 * bwagpu_bgzf_inflate: the decoder alone.  The text of the blocks taken goes to dst (host memory, dst_cap bytes): info->inflated bytes.
 * When a block is damaged (info->damaged_at >= 0) nothing is written to dst.  Returns BWAGPU_EINVAL for NULL p / comp / dst / info, a
 * negative length, and a dst_cap below the blocks' summed ISIZE.
 *
 * bwagpu_fastq_batch_bgzf: bwagpu_fastq_batch over the text of one or two BGZF windows.  The text never exists on the host: the
 * blocks are inflated into the parser's window buffer and the text window the parse sees begins `skip' bytes into it -- skip is the
 * part of the first block's text that earlier batches consumed, 0 <= skip <= that block's ISIZE (0 when the window holds no block), else
 * BWAGPU_EINVAL; a window without eof that is too short for its first block is BWAGPU_FQ_MORE whatever skip is.  From there it is bwagpu_fastq_batch: the same kernels, statuses, outputs, and its two host waits behind one for the
 * inflate's verdict.  consumed[k], declined_at and the offsets in recs are in the text window's coordinates (recs: offsets into
 * device-side text; the blobs names / quals / comments / seqs are the content).  eof of a text window: the window's eof, unless blocks
 * were left out by the 2^31 rule.
 *   BWAGPU_FQ_MORE      as before: repeat the call from the same start with more compressed bytes.
 *   BWAGPU_FQ_DAMAGED   a block taken from either window is damaged, or eof is set and the window does not end with a whole block:
 *                       n_reads == 0, no arrays, damaged_at set in that window's info (the other's is -1 unless it is damaged too).
 *                       DAMAGED wins over DECLINED: nothing of a window with a damaged block is interpreted.
 * info[k] (k = 0, 1; info[1] is zeroed with damaged_at -1 for one window):
 *   next_coff / next_uoff (CUT, END): the BGZF virtual offset of the first byte not consumed -- the block's start in comp and the byte
 *   in that block's text; next_uoff is below that block's ISIZE, or next_coff == used_comp with next_uoff == 0 when all the text taken
 *   was consumed.  The next call's window starts at comp + next_coff with skip = next_uoff.
 * BWAGPU_EINVAL: NULL p / w1 / w1->comp / out / info, w2 with a NULL comp, a negative comp_len or skip, skip beyond the first block's
 * ISIZE, chunk_size <= 0. */
enum { BWAGPU_FQ_DAMAGED = 4 };
typedef struct { const void *comp; int64_t comp_len; int32_t skip, eof; } bwagpu_bgzf_win_t;
typedef struct {
	int64_t used_comp;     /* bytes of comp covered by the whole blocks this call took */
	int64_t inflated;      /* their ISIZEs summed */
	int32_t n_blocks;
	int64_t next_coff; int32_t next_uoff;   /* CUT / END: virtual offset of the first byte not consumed */
	int64_t damaged_at;    /* offset in comp of the first block that is not a BGZF block or does not inflate to its ISIZE and CRC; else -1 */
	float inflate_ms;      /* device time of the inflate kernel (batch_bgzf: of both windows' launches, in both infos) */
} bwagpu_bgzf_info_t;
int  bwagpu_bgzf_inflate(bwagpu_fastq_parser_t *p, const void *comp, int64_t comp_len, int eof,
                         void *dst, int64_t dst_cap, bwagpu_bgzf_info_t *info);
int  bwagpu_fastq_batch_bgzf(bwagpu_fastq_parser_t *p, const bwagpu_bgzf_win_t *w1, const bwagpu_bgzf_win_t *w2 /* NULL: one file */,
                             int chunk_size, bwagpu_fastq_out_t *out, bwagpu_bgzf_info_t info[2]);

/* bwagpu_bgzf_deflate: the other direction -- text (host memory) compressed into a BGZF stream (SAM specification 4.1) that bgzip -d,
 * samtools, htslib and bwagpu_bgzf_inflate read.  The text is cut into blocks of block_size bytes (1..0xff00; 0: 0xff00, bgzip's), each
 * compressed on its own by one wavefront (dev_bgzf_out.h: hash-based match search, greedy parse, length-limited canonical codes; the
 * smallest of dynamic, fixed and stored per block) and never larger than its text + 31 bytes.  The compressed bytes depend on the text
 * and block_size alone.  eof_marker: bgzip's 28-byte end-of-file block behind the last block (text_len == 0: that block alone, or
 * nothing).  *comp: info->comp_len bytes, free with bwagpu_free; text of 2^31 bytes or more takes several launches.  BWAGPU_EINVAL:
 * NULL p / text / comp / info, text_len < 0, block_size outside 0..0xff00. */
typedef struct { int64_t n_blocks, text_len, comp_len; float deflate_ms; } bwagpu_bgzf_out_info_t;
int  bwagpu_bgzf_deflate(bwagpu_fastq_parser_t *p, const void *text, int64_t text_len, int block_size /* 1..0xff00, 0: 0xff00 */,
                         int eof_marker, void **comp /* bwagpu_free */, bwagpu_bgzf_out_info_t *info);
void bwagpu_bgzf_out_limits(int32_t out[4]);   /* largest block text, min match, max match, max distance the kernel uses */

/* ---- interleaved input: `mem -p' ("smart pairing"), on the same parser ------------------------------------------------------------ */
/* ---- FASTA read files on the same parser (the FASTA half of kseq_read, kseq.h:175-204) ---------------------------------------- */
/* bwagpu_fastq_batch_fasta: bwagpu_fastq_batch for windows of FASTA text -- the same arguments, BWAGPU_EINVAL cases, statuses,
 * consumed, declined_file / declined_at, result pool and two host waits; bwagpu_fastq_batch_fasta_bgzf is its BGZF twin, with
 * bwagpu_fastq_batch_bgzf's arguments, BWAGPU_FQ_DAMAGED and third wait.  A window starts at a record start, a '>'; the call returns the
 * batch bseq_read(chunk_size) would cut from there.  The existing entry points are unchanged: they decline every '>' record.
 * The rule for FASTA records.  A line is what lies between two '\n', or between one '\n' and the end of the window; its first byte
 * says what it is:
 *   '>'        a header: the name up to the first isspace() byte (trim_readno applied); when there is such a byte, the comment is the
 *              rest of the line, less one trailing '\r' if it is longer than one byte (ks_getuntil2, kseq.h:140);
 *   no byte    an empty line: skipped (kseq.h:193);
 *   '@'        the start of a FASTQ record: that record is declined;
 *   '+'        the record holding the line is declined;
 *   any other  a sequence line of the record whose header precedes it: its bytes are bases, less a '\r' at its end when the line has two
 *              bytes or more.  A NUL, a byte >= 0x80 or a byte <= ' ' anywhere else in it declines the record.
 * A record ends where the next header line starts, or at the window's end with eof; empty lines behind its bases belong to it, so that
 * consumed at BWAGPU_FQ_END is the window's length.  Declined as well: a record without bases (a '>' with nothing behind it at eof
 * included) and a window that does not start with '>' (at offset 0).  A line that is only "\r": behind a base of its record and before a
 * '\n' it adds nothing, as in the reference (a CRLF file's empty line); as its record's first sequence line, or as the stream's last
 * line without a '\n', the reference keeps the '\r' as a base, and the device declines the record.  A last line of one base without a
 * '\n' is read like any other line.
 * BWAGPU_FQ_CUT needs the end of the batch's last record in view -- the next header line's first byte, or eof -- otherwise the status is
 * BWAGPU_FQ_MORE.  Two windows must both be FASTA.
 * Output: bwagpu_fastq_out_t as it is, with quals == NULL (bseq_read leaves qual NULL, SAM prints '*').  In recs, qual = -1 and
 * l_qual = 0; seq is the window offset of the read's first base byte and l_seq the number of bases: the bases are the window's bytes
 * from seq on, line ends skipped.  kernel_ms: line passes, cut, emit.
 * bwagpu_fasta_reads_limits: bytes per tile, bytes per lane of the byte passes, body bytes per step of the emit pass, 0. */
int  bwagpu_fastq_batch_fasta(bwagpu_fastq_parser_t *p, const void *raw1, int64_t len1, int eof1,
                              const void *raw2 /* NULL: one file */, int64_t len2, int eof2,
                              int chunk_size, bwagpu_fastq_out_t *out);
int  bwagpu_fastq_batch_fasta_bgzf(bwagpu_fastq_parser_t *p, const bwagpu_bgzf_win_t *w1, const bwagpu_bgzf_win_t *w2 /* NULL: one file */,
                                   int chunk_size, bwagpu_fastq_out_t *out, bwagpu_bgzf_info_t info[2]);
void bwagpu_fasta_reads_limits(int32_t out[4]);

/* bwagpu_fastq_batch_smart: bwagpu_fastq_batch on ONE window, followed on the device by bseq_classify (bwa.c:114-130) and the split
 * fastmap.c:94-105 makes of the batch: reads whose name equals the next or the last read's form pairs, the others are single, and
 * mem_process_seqs runs on the single reads first and on the pairs second.  The whole batch is the one a one-window bwagpu_fastq_batch
 * reports -- the same kernels and statuses, status / n_reads / consumed / declined_at with the same meaning (BWAGPU_FQ_MORE: nothing is
 * delivered; BWAGPU_FQ_DECLINED: no arrays) -- and for BWAGPU_FQ_CUT and BWAGPU_FQ_END the call delivers
 *   cls[n_reads]       0: single, 1: first of a pair, 2: second of a pair.  Classification starts anew with every batch, as the
 *                      reference's does: a run of equal names that the cut divides is classified in two parts.
 *   n_sub[k], idx[k]   k = 0: the single reads, k = 1: the reads of pairs (mates at 2j, 2j + 1), both in input order; idx[k][j] is the
 *                      place in the batch of sub-batch k's read j.
 *   sub[k]             sub-batch k complete, in bwagpu_fastq_out_t's layouts and from the same pool: seqs, off, names, name_off, quals,
 *                      comments, comment_off, has_comment, recs (n_reads == n_sub[k], status as the whole batch's; consumed, declined_*
 *                      and kernel_ms are not used).  An empty sub-batch has valid arrays with off[0] == name_off[0] == comment_off[0] == 0.
 *                      The first read of sub-batch 0 has the batch's first read number, the first of sub-batch 1 that number + n_sub[0].
 * Names are compared after trim_readno and as strcmp compares them: a name may hold a NUL byte (it is no white space to kseq), and two
 * names are equal when they agree up to and including the first NUL of either, the end of a name counting as one.  The names
 * delivered keep all their bytes, as the reference's do.
 * Host waits: bwagpu_fastq_batch's two and no other -- the classes are computed before the first one, whose copy brings the sub-batches'
 * sizes along with the batch's.
 * bwagpu_fastq_batch_smart_bgzf: the same over the text of one BGZF window (bwagpu_fastq_batch_bgzf's rules: skip, MORE for a first
 * block not in view, BWAGPU_FQ_DAMAGED wins, next_coff / next_uoff in *info).
 * BWAGPU_EINVAL: NULL p / raw / out, a negative length, a window of 2^31 bytes or more, chunk_size <= 0; for BGZF: NULL p / w / w->comp /
 * out / info, a negative comp_len or skip, skip beyond the first block's ISIZE, chunk_size <= 0. */
typedef struct {
	int32_t status, n_reads;
	int64_t consumed;                  /* bytes of the window that became this batch's records */
	int64_t declined_at;               /* DECLINED: byte offset of the first record not taken, else -1 */
	uint8_t *cls;                      /* n_reads classes */
	int32_t n_sub[2];
	int32_t *idx[2];                   /* n_sub[k] each */
	bwagpu_fastq_out_t sub[2];
	float kernel_ms[4];                /* newline + check passes, cut, classification, emit */
} bwagpu_fastq_smart_t;
int  bwagpu_fastq_batch_smart(bwagpu_fastq_parser_t *p, const void *raw, int64_t len, int eof, int chunk_size, bwagpu_fastq_smart_t *out);
int  bwagpu_fastq_batch_smart_bgzf(bwagpu_fastq_parser_t *p, const bwagpu_bgzf_win_t *w, int chunk_size, bwagpu_fastq_smart_t *out,
                                   bwagpu_bgzf_info_t *info);
void bwagpu_fastq_smart_free(bwagpu_fastq_smart_t *out);   /* releases every array; idempotent */

/* ---- lifetime ------------------------------------------------------------------------------------------ */

/* Create a handle on HIP device `device` and upload the index once (replaces nothing in the reference; it is
 * the extra call a drop-in adds after bwa_idx_load, fastmap.c:362-368).  The descriptor's arrays are copied to
 * HBM; the caller keeps ownership of its host copies. */
int bwagpu_create(bwagpu_t **h, const bwagpu_index_desc_t *idx, int device);

/* Multi-GPU start-up: the index is uploaded once by one rank and broadcast to the others over
 * RCCL/xGMI.  A receiving rank calls bwagpu_create() with bwt = sa = pac = NULL (sizes, scalars and the small contig
 * table filled in): the HBM buffers are allocated but left for the collective to fill.  bwagpu_index_buffers() exposes
 * the three device buffers (pointer + byte size) on both sides; bwagpu_index_export() returns the scalars and contig
 * table of a loaded handle so that they can be sent to the other ranks. */
int bwagpu_index_buffers(bwagpu_t *h, void **bwt, uint64_t *bwt_bytes, void **sa, uint64_t *sa_bytes, void **pac, uint64_t *pac_bytes);
int bwagpu_index_export(const bwagpu_t *h, bwagpu_index_desc_t *scalars, int64_t *ctg_offset, int32_t *ctg_len, int32_t *ctg_is_alt);
/* After the broadcast has filled a receiving handle's buffers: derive the device-side acceleration tables from them. */
int bwagpu_index_ready(bwagpu_t *h);

/* Same, reading <prefix>.bwt/.sa/.pac/.ann/.amb/.alt from disk in the reference's on-disk formats
 * (replaces bwa_idx_load_from_disk(hint, BWA_IDX_ALL), bwa.c:289-321, for a stand-alone host). */
int bwagpu_create_from_files(bwagpu_t **h, const char *prefix, int device);

/* Another handle on the same GPU sharing the resident index (no copy), with its own stream and batch arenas.  Two handles
 * driven from two host threads keep two batches in flight (the kt_pipeline of the reference overlaps I/O the same way,
 * kthread.c:119).  Clone after bwagpu_densify_sa, not before.  Each handle is destroyed separately. */
int bwagpu_clone(bwagpu_t *src, bwagpu_t **out);
/* A handle on another device of the node with its own copy of src's index, copied device to device over xGMI (hipMemcpyPeer): the
 * single-process counterpart of the RCCL index broadcast between processes.  Densify the SA on src first. */
int bwagpu_clone_to_device(bwagpu_t *src, int device, bwagpu_t **out);
void bwagpu_destroy(bwagpu_t *h);
const char *bwagpu_strerror(int code);
const char *bwagpu_last_error(const bwagpu_t *h);
const char *bwagpu_version(void);
/* sizeof of bwagpu_opt_t, _alnreg_t, _stats_t, _index_desc_t, _cigar_t, _matesw_t, _bseq1_t, _built_t in this build of the library */
void bwagpu_abi_sizes(int32_t out[8]);

/* Index facts (for callers that loaded from files). */
int bwagpu_index_info(const bwagpu_t *h, int64_t *l_pac, int32_t *n_seqs, uint64_t *seq_len, int *sa_intv);

/* Optional: replace the sampled SA (interval sa_intv, ~31 dependent index reads per lookup, bwt.c:86-96) by a
 * denser one built on the device (new_intv in {1,2,4,8,16}; values identical by definition of the SA).  Spends
 * HBM capacity to delete dependent loads. */
int bwagpu_densify_sa(bwagpu_t *h, int new_intv);

/* ---- options ------------------------------------------------------------------------------------------------
 * Tuning and test options of a handle, by name (the list with defaults and meanings: bwa_amd/csrc/bwagpu_config.h; bwagpu_option_name(i)
 * enumerates it).  None of them changes a result -- they pick between kernel forms that the tests hold to identical output, size scratch
 * areas, or force the overflow/retry paths.  A handle's options are fixed when it is created: compiled-in defaults, then the environment
 * (BWAGPU_<NAME IN CAPITALS>, read once per bwagpu_create*), then bwagpu_set_default_option(); bwagpu_clone*() copies them;
 * bwagpu_set_option() changes one between batches.  No batch call reads the environment.  (The reference has no counterpart: its tuning
 * lives in mem_opt_t, which this library takes as it is.)
 *   bwagpu_set_default_option: for handles created afterwards by this process -- the way to set the options that shape what is derived from
 *   the index at load time (occ32, occ32_sb_shift, ptab_m); bwagpu_clear_default_options() forgets them all.
 *   Unknown name -> BWAGPU_EINVAL.  -1 means "automatic" for the options that have such a setting. */
int bwagpu_set_option(bwagpu_t *h, const char *name, long long value);
int bwagpu_get_option(const bwagpu_t *h, const char *name, long long *value);
int bwagpu_set_default_option(const char *name, long long value);
void bwagpu_clear_default_options(void);
int bwagpu_option_name(int i, const char **name);    /* i = 0, 1, ... until BWAGPU_EINVAL */

/* Enable (1) / disable (0) collection of the algorithmic work counters in bwagpu_stats_t. */
int bwagpu_set_stats(bwagpu_t *h, int enable);
int bwagpu_get_stats(const bwagpu_t *h, bwagpu_stats_t *out);

/* ---- the hot path -------------------------------------------------------------------------------------- */

/* Drop-in replacement for the worker1 loop (reference bwamem.c:1203-1215, 1252).
 *   seqs[i].seq holds ASCII bases or 0..4 codes; on return it holds 0..4 codes (the in-place mutation
 *   contract of mem_align1_core, bwamem.c:1087-1088).  regs[i] receives {n, m, a} with a malloc()ed array
 *   the caller free()s, exactly as worker2 does (bwamem.c:1227,1231).  With MEM_F_PE set in opt->flag nothing
 *   changes on this path: both mates are aligned independently (bwamem.c:1209-1213).
 *   With n = 1 it is also the device half of mem_align1 (bwamem_extra.c:102-112; example.c:40): the binding copies the sequence,
 *   calls this and then the reference's own mem_mark_primary_se (integration/mem_process_seqs_gpu.c, __wrap_mem_align1). */
int bwagpu_align_bseq(bwagpu_t *h, const bwagpu_opt_t *opt, int n, bwagpu_bseq1_t *seqs, bwagpu_alnreg_v *regs);

/* Flat form of the same call: reads are nt4 codes (0..4) concatenated in `seqs`, read i = seqs[off[i]..off[i+1]).
 *   counts[i] = number of regions of read i; *regs_out = array of all regions in read order
 *   (caller frees with bwagpu_free -- NOT free(): large results are page-locked blocks of a pool that bwagpu_free refills,
 *   BWAGPU_PINNED_RESULTS=0 turns that off); *n_regs_out = total. */
int bwagpu_align_flat(bwagpu_t *h, const bwagpu_opt_t *opt, int n, const uint8_t *seqs, const int64_t *off,
					  int32_t *counts, bwagpu_alnreg_t **regs_out, int64_t *n_regs_out);
/* A host buffer for a batch's base codes (what bwagpu_batch_upload reads): page-locked when the runtime grants it, from the same pool as
 * the result arrays, so that the upload is one DMA instead of a staged copy; plain memory otherwise.  Release with bwagpu_free.
 * (No counterpart in the reference: bseq1_t::seq is malloc'ed by bseq_read, bwa.c:79-112.) */
void *bwagpu_alloc_host(size_t bytes);
void bwagpu_free(void *p);   /* releases any array an entry point of this library returned through an out-pointer (thread-safe) */
/* The pool behind bwagpu_alloc_host and the large result arrays keeps up to 4 GiB of page-locked blocks for re-use (options pinned_results,
 * pinned_min_kb).  bwagpu_trim() gives the idle ones back to the system; it happens by itself when the process's last handle is destroyed.
 * Blocks are pinned under the calling thread's current device (the batch calls set their handle's); they are portable across devices. */
void bwagpu_trim(void);

/* Split form for callers that overlap transfers with compute, and for measuring the device path with the batch
 * already resident in HBM: upload -> run (device only, asynchronous kernels + one final sync) -> download. */
int bwagpu_batch_upload(bwagpu_t *h, int n, const uint8_t *seqs, const int64_t *off);
/* Optional, any time: allocate the device buffers a batch of about this shape will need (they are only ever grown), so that the handle's
 * first batch does not pay for them inside a pipeline.  Unless option reserve_results is 0 it also page-locks the result blocks of such a batch
 * (about 150 bytes per region at 4 regions per read) and hands them to the pool bwagpu_free() feeds, where the batch's downloads find them. */
int bwagpu_batch_reserve(bwagpu_t *h, int n_reads, int64_t n_bases, int max_len);
/* Bytes of device memory the handle's buffers would grow by for a batch of this shape (what bwagpu_batch_reserve would allocate now; -1 on bad
 * arguments), and the device's free / total memory (hipMemGetInfo).  `bwa-amd mem` sizes the dense suffix array with them: it takes the smallest
 * SA interval that leaves room for its handles' batches. */
int64_t bwagpu_batch_footprint(bwagpu_t *h, int n_reads, int64_t n_bases, int max_len);
int bwagpu_mem_info(bwagpu_t *h, uint64_t *free_bytes, uint64_t *total_bytes);
int bwagpu_batch_run(bwagpu_t *h, const bwagpu_opt_t *opt);
int bwagpu_batch_download(bwagpu_t *h, int32_t *counts, bwagpu_alnreg_t **regs_out, int64_t *n_regs_out);

/* ---- stage taps (parity tests; device results of the last batch_run, read order) ------------------------ */
/* Taps are on by default; switching them off (0) skips the copy of the pre-dedup regions kept for
 * bwagpu_tap_regs_raw (a benchmark setting). */
int bwagpu_set_taps(bwagpu_t *h, int enable);
/* SA intervals after mem_collect_intv (bwamem.c:140-188): per read counts + records {x0, x2, info}. */
typedef struct { uint64_t x0, x2, info; } bwagpu_intv_t;
int bwagpu_tap_intervals(bwagpu_t *h, int32_t *counts, bwagpu_intv_t **out, int64_t *n_out);
/* Chains after mem_chain_flt (+ mem_flt_chained_seeds): per read chain counts, chain headers, flat seeds. */
typedef struct { int32_t n_seeds, rid, w, kept, is_alt; float frac_rep; int64_t pos; } bwagpu_chain_t;
typedef struct { int64_t rbeg; int32_t qbeg, len, score, pad_; } bwagpu_seed_t;
int bwagpu_tap_chains(bwagpu_t *h, int32_t *counts, bwagpu_chain_t **chains, int64_t *n_chains,
					  bwagpu_seed_t **seeds, int64_t *n_seeds);
/* Regions after mem_chain2aln, before mem_sort_dedup_patch. */
int bwagpu_tap_regs_raw(bwagpu_t *h, int32_t *counts, bwagpu_alnreg_t **out, int64_t *n_out);

#ifdef __cplusplus
}
#endif
#endif
