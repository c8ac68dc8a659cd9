// dev_fastq_smart.h -- `bwa mem -p` ("smart pairing") on the device FASTQ reader's batch (included by bwagpu_index.hip behind
// dev_fastq.h; host side: bwagpu_fastq_batch_smart*).
//
// What it reproduces: bseq_classify (bwa.c:114-130) on the batch bseq_read cut from ONE window, and the two arrays it fills --
// sep[0], the reads without a mate, and sep[1], the pairs at 2k, 2k + 1, both in input order -- as two sub-batches in
// bwagpu_fastq_out_t's layouts, which is what fastmap.c:94-105 calls mem_process_seqs on.
//
// The rule.  eq[i] = (strcmp(name[i], name[i - 1]) == 0) for 1 <= i < n, eq[0] = 0, names after trim_readno.  The reference's loop
// with has_last is the recurrence paired[i] = eq[i] && !paired[i - 1], paired[0] = 0: within a maximal run of eq ones that starts at
// i0 (eq[i0 - 1] == 0), paired[i] = ((i - i0) & 1) == 0.  Read j is the second of a pair iff paired[j], the first iff paired[j + 1]
// (paired[n] = 0), else it is single.  i0 is the last j <= i with eq[j] == 0, plus one: an inclusive maximum scan of
// (eq[j] ? 0 : j + 1), whose result does not depend on how the scan cuts the array into blocks.
//
// Names compare as strcmp compares them: a header byte '\0' is not isspace(), so a name may hold one, and strcmp stops there while
// the name that is delivered keeps all its bytes.  Two names are equal iff they agree up to and including the first NUL of either,
// the terminator behind the name's last byte counting as one.
//
// Passes, all behind k_fq_decide and before the host's first wait (the batch size n is read from the FqInfo on the device; lanes
// past n write neutral elements, so that the scans may run over cap_units entries as the existing ones do):
//   5. k_fqs_eq: one lane per read, (eq ? 0 : i + 1) -> scanned with maximum (rocPRIM).
//   6. k_fqs_class: one lane per read: class 0 / 1 / 2 and the lengths the read adds to its sub-batch -> scanned with plus.
//   7. k_fqs_emit: k_fq_emit's work into two sub-batches: one wavefront per read, the place in the sub-batch and the offsets of the
//      read's name, comment and bases from the exclusive scan.
#pragma once

// what a read adds to the sub-batches (k: 0 single, 1 paired): a read, its bases, name and comment bytes.  (32-bit: a window has
// less than 2^31 bytes, and every sum counts bytes of it)
struct FqsSum { u32 n[2], seq[2], name[2], com[2]; };
struct FqsPlus {
	__host__ __device__ FqsSum operator()(const FqsSum &a, const FqsSum &b) const
	{
		FqsSum r;
		for (int k = 0; k < 2; ++k) { r.n[k] = a.n[k] + b.n[k]; r.seq[k] = a.seq[k] + b.seq[k]; r.name[k] = a.name[k] + b.name[k]; r.com[k] = a.com[k] + b.com[k]; }
		return r;
	}
};

IDX_DEVFN u64 fqs_load8(const u8 *p) { u64 w; __builtin_memcpy(&w, p, 8); return w; }
// the lowest set bit marks the first zero byte of w (bits above it may be set for bytes that are not zero)
IDX_DEVFN u64 fqs_zero_bytes(u64 w) { return (w - 0x0101010101010101ull) & ~w & 0x8080808080808080ull; }

// strcmp(a, b) == 0 for names of la and lb bytes in the window, each followed by a terminator that is not in the window.  Eight
// bytes per step (a name lies at any offset; a load may run up to 7 bytes past the shorter name's end, which is inside the record:
// behind the header line a plain record has at least 7 bytes)
IDX_DEVFN bool fqs_name_eq(const u8 *a, u32 la, const u8 *b, u32 lb)
{
	const u32 m = la < lb ? la : lb;
	for (u32 t = 0; t < m; t += 8) {
		const u32 left = m - t;
		const u64 mask = left >= 8 ? ~0ull : (1ull << (8 * left)) - 1;
		const u64 wa = fqs_load8(a + t), x = (wa ^ fqs_load8(b + t)) & mask, z = fqs_zero_bytes(wa | ~mask);
		if (x | z) {
			const int fd = x ? __ffsll((unsigned long long)x) - 1 : 64, fz = z ? __ffsll((unsigned long long)z) - 1 : 64;
			return (fz >> 3) < (fd >> 3);      // a NUL in both before the first difference: equal; else they differ
		}
	}
	if (la == lb) return true;
	return (la < lb ? b[m] : a[m]) == 0;      // the shorter name's terminator against the longer one's next byte
}

// reads of the batch the passes before left in info (0: no batch)
IDX_DEVFN u64 fqs_n(const FqInfo *info) { return (info->status == BWAGPU_FQ_CUT || info->status == BWAGPU_FQ_END) ? (u64)info->n_units : 0; }

// pass 5: adjacent names.  v[i] = 0 when read i's name equals read i - 1's, else i + 1
__global__ void __launch_bounds__(FQ_BLOCK) k_fqs_eq(FqArgs A, const FqInfo *info, u32 *v)
{
	const u64 n = fqs_n(info);
	const FqWin &W = A.w[0];
	for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < A.cap_units; i += (u64)gridDim.x * blockDim.x) {
		bool eq = false;
		if (i && i < n) {
			const bwagpu_fastq_rec_t r = W.recs[i], q = W.recs[i - 1];
			eq = fqs_name_eq(W.buf + (u32)r.name, (u32)r.l_name, W.buf + (u32)q.name, (u32)q.l_name);
		}
		v[i] = eq ? 0u : (u32)i + 1u;
	}
}

// paired[i] from the scanned run starts (rs[i]: i0 of the run read i is in; i + 1 when eq[i] == 0)
IDX_DEVFN bool fqs_paired(const u32 *rs, u64 i, u64 n) { return i < n && rs[i] != (u32)i + 1u && (((u32)i - rs[i]) & 1u) == 0; }

// pass 6: classes and what every read adds to its sub-batch
__global__ void __launch_bounds__(FQ_BLOCK) k_fqs_class(FqArgs A, const FqInfo *info, const u32 *rs, u8 *cls, FqsSum *sums)
{
	const u64 n = fqs_n(info);
	const FqWin &W = A.w[0];
	for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < A.cap_units; i += (u64)gridDim.x * blockDim.x) {
		FqsSum s;
		for (int k = 0; k < 2; ++k) s.n[k] = s.seq[k] = s.name[k] = s.com[k] = 0;
		if (i < n) {
			const u32 c = fqs_paired(rs, i, n) ? 2u : fqs_paired(rs, i + 1, n) ? 1u : 0u;
			const bwagpu_fastq_rec_t r = W.recs[i];
			const int k = c ? 1 : 0;
			cls[i] = (u8)c;
			s.n[k] = 1; s.seq[k] = (u32)r.l_seq; s.name[k] = (u32)r.l_name; s.com[k] = (u32)r.l_comment;
		}
		sums[i] = s;
	}
}

// where pass 7 writes: the two sub-batches, and the place in the input batch of every read of theirs
struct FqsOut { FqOut sub[2]; int32_t *idx[2]; };

// pass 7: one wavefront per read.  sscan: inclusive scan of sums; total: its last element
__global__ void __launch_bounds__(FQ_BLOCK) k_fqs_emit(FqArgs A, const u8 *cls, const FqsSum *sscan, u64 n_reads, FqsSum total, FqsOut O)
{
	const u32 lane = threadIdx.x & (FQ_WAVE - 1);
	const u64 wave0 = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / FQ_WAVE, n_waves = (u64)gridDim.x * blockDim.x / FQ_WAVE;
	const FqWin &W = A.w[0];
	for (u64 j = wave0; j < n_reads; j += n_waves) {
		const int k = cls[j] ? 1 : 0;
		const bwagpu_fastq_rec_t r = W.recs[j];
		u64 at = 0, a_seq = 0, a_name = 0, a_com = 0;
		if (j) { const FqsSum &e = sscan[j - 1]; at = e.n[k]; a_seq = e.seq[k]; a_name = e.name[k]; a_com = e.com[k]; }
		const FqOut &o = O.sub[k];
		if (lane == 0) {
			o.off[at] = (i64)a_seq; o.name_off[at] = (i64)a_name; o.comment_off[at] = (i64)a_com; o.has_comment[at] = (u8)r.has_comment; o.recs[at] = r;
			O.idx[k][at] = (int32_t)j;
			if (at + 1 == total.n[k]) { o.off[at + 1] = (i64)total.seq[k]; o.name_off[at + 1] = (i64)total.name[k]; o.comment_off[at + 1] = (i64)total.com[k]; }
		}
		const u8 *b = W.buf;
		for (u32 t = lane; t < (u32)r.l_name; t += FQ_WAVE) o.names[a_name + t] = (char)b[(u32)r.name + t];
		for (u32 t = lane; t < (u32)r.l_comment; t += FQ_WAVE) o.comments[a_com + t] = (char)b[(u32)r.comment + t];
		for (u32 t = lane; t < (u32)r.l_seq; t += FQ_WAVE) {
			o.seqs[a_seq + t] = (u8)fq_nt4(b[(u32)r.seq + t]);
			o.quals[a_seq + t] = (char)b[(u32)r.qual + t];
		}
	}
}
