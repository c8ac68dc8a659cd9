// dev_samtext_pe.h -- the SAM text of read pairs on the device: what mem_sam_pe (bwamem_pair.c:360-385 and :397-415) prints once bwagpu_batch_sampe's kernels have
// decided the pairs.  bwagpu_batch_sam_pe / bwagpu_sam_pe_flat (bwagpu.hip).
//
// The formatter is dev_samtext.h's, with a SamMate where the single-end kernels pass SamNoMate.  Read r is end r & 1 of pair r >> 1; what it prints is in the
// `sel` fields of its alignment records on either path (dev_sampe.h: place z and place alt on path 0, mem_reg2sam's list on path 1), so sam_read walks both alike.
// The mate is place z[1 - i] of the other end's marked list -- `which` on path 1, which need not be a printed place -- or, where that is -1, the unmapped record;
// MQ prints q_se[1 - i] on both paths.
//
// Mapping: one wavefront per READ, as in the single-end kernels, so the two ends of a pair may run in different workgroups; each computes the pair's declined bit
// for itself (sam_pe_declined: both ends' lists are scanned by both).  A pair is declined as a whole: its bwagpu_sampe_t has flags & 1 or path < 0, an end is
// declined by the single-end rule, or an end's mate place has no CIGAR record.
#pragma once
#include "dev_samtext.h"
#include "dev_sampe.h"

// the mate of end i of pair P: Qm is the other end
DEVFN SamMate sam_mate(const SamIn &I, const bwagpu_sampe_t &P, int i, const SamRead &Qm)
{
	SamMate m;
	const int z = i ? P.z[0] : P.z[1];
	m.a = nullptr; m.c = nullptr; m.rlen = 0;
	m.mapq = i ? P.q_se[0] : P.q_se[1];
	m.flag = (0x40 << i) | P.extra_flag;
	if (z >= 0 && z < Qm.n) {
		m.a = Qm.alns + z; m.c = Qm.cigs + Qm.pri[z].src;
		if (m.a->rid >= 0 && m.a->n_cigar > 0 && (m.a->flags & BWAGPU_ALN_REV)) m.rlen = sam_rlen(I, *m.a, m.c);      // (read only for a reverse mate)
	}
	return m;
}

// the pair is left to the caller
DEVFN bool sam_pe_declined(const bwagpu_opt_t &opt, const bwagpu_sampe_t &P, const SamRead &Q0, const SamRead &Q1, int lane)
{
	if ((P.flags & 1) || P.path < 0) return true;
	if (P.z[0] >= 0 && P.z[0] < Q0.n && (Q0.alns[P.z[0]].flags & BWAGPU_ALN_NOCIGAR)) return true;
	if (P.z[1] >= 0 && P.z[1] < Q1.n && (Q1.alns[P.z[1]].flags & BWAGPU_ALN_NOCIGAR)) return true;
	return sam_declined(opt, Q0, lane) || sam_declined(opt, Q1, lane);
}

// pass 1: bytes, lines and the declined bit of every read (one wavefront, a workgroup of 64, per read)
__global__ void __launch_bounds__(64) k_sam_pe_size(bwagpu_opt_t opt, int n_reads, const i32 *cnt, const i64 *off, SamIn I, const bwagpu_sampe_t *sampe, i32 *size, i32 *flags, i32 *n_lines)
{
	const int lane = threadIdx.x & 63;
	for (int r = blockIdx.x; r < n_reads; r += gridDim.x) {
		const bwagpu_sampe_t P = sampe[r >> 1];
		const SamRead Q = sam_view(I, cnt, off, r), Qm = sam_view(I, cnt, off, r ^ 1);
		SamCount s; s.n = 0;
		int lines = 0;
		const bool declined = (r & 1) ? sam_pe_declined(opt, P, Qm, Q, lane) : sam_pe_declined(opt, P, Q, Qm, lane);
		if (!declined) lines = sam_read(s, opt, I, Q, lane, sam_mate(I, P, r & 1, Qm));
		if (lane == 0) { size[r] = (i32)s.n; flags[r] = declined ? 1 : 0; n_lines[r] = lines; }
	}
}

// pass 2: read r's lines at text + toff[r]
__global__ void __launch_bounds__(64) k_sam_pe_write(bwagpu_opt_t opt, int n_reads, const i32 *cnt, const i64 *off, SamIn I, const bwagpu_sampe_t *sampe, const i64 *toff, const i32 *flags, char *text)
{
	__shared__ char stage[SAM_STAGE];
	const int lane = threadIdx.x & 63;
	for (int r = blockIdx.x; r < n_reads; r += gridDim.x) {
		if (flags[r] & 1) continue;
		const bwagpu_sampe_t P = sampe[r >> 1];
		const SamRead Q = sam_view(I, cnt, off, r), Qm = sam_view(I, cnt, off, r ^ 1);
		SamWrite s; s.out = text + toff[r]; s.stage = stage; s.fill = 0; s.lane = lane;
		sam_read(s, opt, I, Q, lane, sam_mate(I, P, r & 1, Qm));
		s.flush();
	}
}
