// bgzf_asan.cpp -- the BGZF inflate (bwa_amd/csrc/dev_bgzf.h and its host side in bwagpu_index.hip) under AddressSanitizer and
// UndefinedBehaviorSanitizer, on the CPU: a stand-alone program linked with the library sources compiled against the mock HIP runtime
// (tests/hostsim).  It reads the corpus tests/bgzf_cases.py dumps -- every valid and every damaged window -- and hands each window to
// bwagpu_bgzf_inflate and to bwagpu_fastq_batch_bgzf from a heap copy of exactly the window's size, with a text buffer of exactly the
// expected size: device buffers are heap blocks under the mock, so any read or write outside a window, a table or a text is reported.
// tools/bgzf_asan.sh builds and runs it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../include/bwagpu.h"

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: bgzf_asan <corpus dump>\n"); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	bwagpu_fastq_parser_t *p = nullptr;
	char eb[256];
	if (bwagpu_fastq_begin(&p, 0, eb, sizeof eb) != 0) { fprintf(stderr, "bwagpu_fastq_begin: %s\n", eb); return 2; }
	long n = 0, n_bad = 0, failed = 0;
	for (;;) {
		uint32_t len, tlen; uint8_t eof; int64_t bad;
		if (fread(&len, 4, 1, f) != 1) break;
		if (fread(&eof, 1, 1, f) != 1 || fread(&bad, 8, 1, f) != 1 || fread(&tlen, 4, 1, f) != 1) { fprintf(stderr, "short dump\n"); return 2; }
		unsigned char *win = (unsigned char*)malloc(len ? len : 1), *want = (unsigned char*)malloc(tlen ? tlen : 1), *dst = (unsigned char*)malloc(tlen ? tlen : 1);
		if ((len && fread(win, 1, len, f) != len) || (tlen && fread(want, 1, tlen, f) != tlen)) { fprintf(stderr, "short dump\n"); return 2; }
		bwagpu_bgzf_info_t info;
		int rc = bwagpu_bgzf_inflate(p, win, len, eof, dst, tlen, &info);
		if (bad >= 0) {      // (a damaged window's text buffer is too small for the blocks' claims, or the damage is reported)
			++n_bad;
			if (!(rc == BWAGPU_EINVAL || (rc == 0 && info.damaged_at == bad))) { fprintf(stderr, "window %ld: rc %d damaged_at %lld, expected %lld\n", n, rc, (long long)info.damaged_at, (long long)bad); ++failed; }
		} else if (rc != 0 || info.damaged_at != -1 || info.inflated != (int64_t)tlen || memcmp(dst, want, tlen)) { fprintf(stderr, "window %ld: rc %d, text differs\n", n, rc); ++failed; }
		bwagpu_bgzf_win_t w = { win, (int64_t)len, 0, eof };
		bwagpu_fastq_out_t out; bwagpu_bgzf_info_t inf[2];
		rc = bwagpu_fastq_batch_bgzf(p, &w, nullptr, 1000, &out, inf);
		if (rc != 0 || (bad >= 0) != (out.status == BWAGPU_FQ_DAMAGED) || inf[0].damaged_at != bad) { fprintf(stderr, "window %ld: batch rc %d status %d damaged_at %lld, expected %lld\n", n, rc, out.status, (long long)inf[0].damaged_at, (long long)bad); ++failed; }
		bwagpu_fastq_out_free(&out);
		free(win); free(want); free(dst);
		++n;
	}
	bwagpu_fastq_end(p);
	fclose(f);
	printf("%ld windows (%ld damaged), %ld disagreements\n", n, n_bad, failed);
	return failed ? 1 : 0;
}
