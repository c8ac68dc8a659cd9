// bgzf_out_asan.cpp -- the BGZF writer (bwa_amd/csrc/dev_bgzf_out.h and its host side in bwagpu_index.hip) under AddressSanitizer and
// UndefinedBehaviorSanitizer, on the CPU: a stand-alone program linked with the library sources compiled against the mock HIP runtime
// (tests/hostsim).  It reads the texts tests/bgzf_out_cases.py dumps, one file per case, and hands each to bwagpu_bgzf_deflate from a heap
// copy of exactly the text's size, at blocks of 0xff00, 333 and (short texts) 1 byte, with and without the end-of-file block; what comes
// back goes through bwagpu_bgzf_inflate into a buffer of exactly the text's size and is compared.  Device buffers are heap blocks under
// the mock, so a read or write outside a text, a token array, a slot or the packed blocks is reported.  tools/bgzf_out_asan.sh builds and
// runs it.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../include/bwagpu.h"

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: bgzf_out_asan <text file> ...\n"); return 2; }
	bwagpu_fastq_parser_t *p = nullptr;
	char eb[256];
	if (bwagpu_fastq_begin(&p, 0, eb, sizeof eb) != 0) { fprintf(stderr, "bwagpu_fastq_begin: %s\n", eb); return 2; }
	long n_calls = 0, failed = 0;
	for (int a = 1; a < argc; ++a) {
		FILE *f = fopen(argv[a], "rb");
		if (!f) { perror(argv[a]); return 2; }
		fseek(f, 0, SEEK_END);
		const long n = ftell(f);
		fseek(f, 0, SEEK_SET);
		unsigned char *text = (unsigned char*)malloc(n ? n : 1), *back = (unsigned char*)malloc(n ? n : 1);
		if (n && fread(text, 1, (size_t)n, f) != (size_t)n) { fprintf(stderr, "%s: short read\n", argv[a]); return 2; }
		fclose(f);
		const int sizes[4] = { 0, 0xff00, 333, 1 };
		for (int k = 0; k < 4; ++k) {
			if (sizes[k] == 1 && n > 600) continue;
			for (int eof = 0; eof < 2; ++eof) {
				void *comp = nullptr; bwagpu_bgzf_out_info_t info;
				int rc = bwagpu_bgzf_deflate(p, text, n, sizes[k], eof, &comp, &info);
				++n_calls;
				if (rc != 0 || info.text_len != n || (info.comp_len && !comp)) { fprintf(stderr, "%s, blocks of %d: rc %d\n", argv[a], sizes[k], rc); ++failed; continue; }
				unsigned char *c = (unsigned char*)malloc(info.comp_len ? info.comp_len : 1);      // (an exact-size copy for the reader)
				memcpy(c, comp, (size_t)info.comp_len);
				bwagpu_free(comp);
				bwagpu_bgzf_info_t in;
				rc = bwagpu_bgzf_inflate(p, c, info.comp_len, 1, back, n, &in);
				if (rc != 0 || in.damaged_at != -1 || in.inflated != n || in.used_comp != info.comp_len || memcmp(back, text, (size_t)n)) {
					fprintf(stderr, "%s, blocks of %d: the stream does not inflate to the text (rc %d, damaged_at %lld)\n", argv[a], sizes[k], rc, (long long)in.damaged_at); ++failed;
				}
				free(c);
			}
		}
		free(text); free(back);
	}
	void *comp = nullptr; bwagpu_bgzf_out_info_t info;
	if (bwagpu_bgzf_deflate(p, nullptr, 4, 0, 1, &comp, &info) != BWAGPU_EINVAL || bwagpu_bgzf_deflate(p, "text", 4, 0xff01, 1, &comp, &info) != BWAGPU_EINVAL) ++failed;
	bwagpu_fastq_end(p);
	printf("%d texts, %ld calls, %ld disagreements\n", argc - 1, n_calls, failed);
	return failed ? 1 : 0;
}
