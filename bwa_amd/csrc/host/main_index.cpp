// main_index.cpp -- `bwa-amd index`: the reference's `bwa index` (bwtindex.c:209-323) on the device.  The FASTA text (plain, gzip or
// BGZF, read by host_input.h's Reader one buffer ahead of the parser) is parsed by the bwagpu_fasta_* kernels, the suffix sort and the
// BWT / Occ / sampled-SA layout are bwagpu_index_build's; the five files are byte-identical to those `bwa index` writes.
#include <getopt.h>
#include <chrono>
#include "bwamem_host.h"
#include "host_input.h"

static double idx_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static int index_usage()
{
	fprintf(stderr, "\nUsage:   bwa-amd index [options] <in.fasta[.gz]>\n\n"
			"Options: -p STR    prefix of the index [same as fasta name]\n"
			"         -6        index files named as <in.fasta>.64.* instead of <in.fasta>.*\n"
			"         -a STR    accepted for compatibility (bwtsw, is or rb2); the device builder ignores it\n"
			"         -b INT    accepted for compatibility; ignored\n"
			"         -v INT    verbosity; 3 prints the stage times [3]\n\n");
	return 1;
}

// the five files of bns_dump / bwt_dump_bwt / bwt_dump_sa and the .pac tail of bns_fasta2bntseq (bntseq.c:65-95, 314-323; bwt.c:385-407)
static bool write_index(const std::string &prefix, const bwagpu_fasta_t &fa, const bwagpu_built_t &b)
{
	bool ok = true;
	FILE *fp = fopen((prefix + ".pac").c_str(), "wb");
	if (!fp) return false;
	const int64_t l_pac = fa.l_pac;
	ok &= fwrite(fa.pac, 1, (size_t)((l_pac >> 2) + ((l_pac & 3) ? 1 : 0)), fp) == (size_t)((l_pac >> 2) + ((l_pac & 3) ? 1 : 0));
	if (l_pac % 4 == 0) ok &= fputc(0, fp) != EOF;
	ok &= fputc((int)(l_pac % 4), fp) != EOF;
	ok &= fclose(fp) == 0;
	if (!ok || !(fp = fopen((prefix + ".ann").c_str(), "w"))) return false;
	fprintf(fp, "%lld %d %u\n", (long long)l_pac, fa.n_seqs, 11u);
	const char *nm = fa.names;
	for (int i = 0; i < fa.n_seqs; ++i) {
		const char *anno = nm + strlen(nm) + 1;
		fprintf(fp, "%d %s", 0, nm);
		if (anno[0]) fprintf(fp, " %s\n", anno); else fprintf(fp, "\n");
		fprintf(fp, "%lld %d %d\n", (long long)fa.seq_offset[i], fa.seq_len[i], fa.seq_n_ambs[i]);
		nm = anno + strlen(anno) + 1;
	}
	ok &= !ferror(fp); ok &= fclose(fp) == 0;
	if (!ok || !(fp = fopen((prefix + ".amb").c_str(), "w"))) return false;
	fprintf(fp, "%lld %d %u\n", (long long)l_pac, fa.n_seqs, (unsigned)fa.n_holes);
	for (int64_t i = 0; i < fa.n_holes; ++i) fprintf(fp, "%lld %d %c\n", (long long)fa.hole_offset[i], fa.hole_len[i], fa.hole_amb[i]);
	ok &= !ferror(fp); ok &= fclose(fp) == 0;
	const uint64_t hdr[5] = { b.primary, b.L2[1], b.L2[2], b.L2[3], b.L2[4] };
	if (!ok || !(fp = fopen((prefix + ".bwt").c_str(), "wb"))) return false;
	ok &= fwrite(hdr, 8, 5, fp) == 5;
	ok &= fwrite(b.bwt, 4, (size_t)b.bwt_size, fp) == (size_t)b.bwt_size;
	ok &= fclose(fp) == 0;
	if (!ok || !(fp = fopen((prefix + ".sa").c_str(), "wb"))) return false;
	const uint64_t sa_hdr[2] = { (uint64_t)b.sa_intv, b.seq_len };
	ok &= fwrite(hdr, 8, 5, fp) == 5;
	ok &= fwrite(sa_hdr, 8, 2, fp) == 2;
	ok &= fwrite(b.sa + 1, 8, (size_t)(b.n_sa - 1), fp) == (size_t)(b.n_sa - 1);    // sa[0] = -1 is not stored (bwt.c:404)
	ok &= fclose(fp) == 0;
	return ok;
}

int main_index(int argc, char *argv[])
{
	std::string prefix;
	int is_64 = 0, verbose = 3, c;
	optind = 1;
	while ((c = getopt(argc, argv, "6a:p:b:v:")) >= 0) {
		switch (c) {
		case 'a':
			if (strcmp(optarg, "rb2") && strcmp(optarg, "bwtsw") && strcmp(optarg, "is")) { fprintf(stderr, "[E::bwa_index] unknown algorithm: '%s'.\n", optarg); return 1; }
			break;
		case 'p': prefix = optarg; break;
		case '6': is_64 = 1; break;
		case 'b': break;
		case 'v': verbose = atoi(optarg); break;
		default: return 1;
		}
	}
	if (optind + 1 > argc) return index_usage();
	const char *fn = argv[optind];
	if (prefix.empty()) { prefix = fn; if (is_64) prefix += ".64"; }
	const int64_t chunk = getenv("BWAGPU_FASTA_CHUNK") ? atoll(getenv("BWAGPU_FASTA_CHUNK")) : 0;   // (tests: tiny device chunks)
	char err[512] = "";
	const double t0 = idx_now();
	double t_read = 0;
	bwagpu_fasta_parser_t *p = nullptr;
	int rc = bwagpu_fasta_begin(&p, 0, chunk, err, sizeof err);
	if (rc) { fprintf(stderr, "[E::bwa_index] %s %s\n", bwagpu_strerror(rc), err); return 1; }
	bwagpu_fasta_t fa; memset(&fa, 0, sizeof fa);
	{
		ParPool pool(4);
		Reader r;
		if (!r.open(fn, &pool)) { fprintf(stderr, "[E::bwa_index] fail to open file '%s' : %s\n", fn, strerror(errno)); (void)bwagpu_fasta_end(p, nullptr, nullptr, 0); return 1; }
		const size_t cap = getenv("BWAGPU_CLI_BUF") ? r.buf.size() : ((size_t)64 << 20);    // the reader's buffers: 64 MiB pieces unless a test sets them
		r.buf.resize(cap); r.nbuf.resize(cap);
		for (;;) {
			const double tr = idx_now();
			const bool more = r.fill();            // (the next buffer is read and inflated by the reader's thread meanwhile)
			t_read += idx_now() - tr;
			if (!more) break;
			if ((rc = bwagpu_fasta_feed(p, r.buf.data(), r.len, err, sizeof err)) != 0) break;
		}
	}
	rc = bwagpu_fasta_end(p, &fa, err, sizeof err);
	const double t1 = idx_now();
	if (rc) { fprintf(stderr, "[E::bwa_index] %s: %s\n", fn, err); return 1; }
	if (verbose >= 3) fprintf(stderr, "[bwa_index] read + inflate (waits) %.2f sec; FASTA parse %.2f sec (kernels %.1f ms): %lld bp, %d sequences, %lld holes\n",
							  t_read, t1 - t0 - t_read, fa.parse_ms, (long long)fa.l_pac, fa.n_seqs, (long long)fa.n_holes);
	bwagpu_built_t b; memset(&b, 0, sizeof b);
	rc = bwagpu_index_build(fa.pac, fa.l_pac, 32, 0, &b, err, sizeof err);
	const double t2 = idx_now();
	if (rc) { fprintf(stderr, "[E::bwa_index] bwagpu_index_build: %s %s\n", bwagpu_strerror(rc), err); bwagpu_fasta_free(&fa); return 1; }
	if (verbose >= 3) fprintf(stderr, "[bwa_index] suffix sort + BWT + SA %.2f sec (device %.1f ms)\n", t2 - t1, b.build_ms);
	const bool ok = write_index(prefix, fa, b);
	bwagpu_built_free(&b);
	bwagpu_fasta_free(&fa);
	if (!ok) {
		fprintf(stderr, "[E::bwa_index] failed to write the index files %s.*: %s\n", prefix.c_str(), strerror(errno));
		for (const char *ext : { ".pac", ".ann", ".amb", ".bwt", ".sa" }) unlink((prefix + ext).c_str());
		return 1;
	}
	if (verbose >= 3) fprintf(stderr, "[bwa_index] file writes %.2f sec; total %.2f sec\n", idx_now() - t2, idx_now() - t0);
	return 0;
}
