// host_input.h -- the input reader of the command line (`bwa-amd mem`, `bwa-amd index`): plain files by read(2), BGZF files inflated
// block-parallel, other gzip and stdin through zlib; the bytes delivered are those gzread would deliver (kseq.h over gzread).
#pragma once
#include <ctype.h>
#include <errno.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <sys/mman.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

// ---- FASTA/FASTQ input (what kseq_read + bseq_read deliver, kseq.h:175-220, bwa.c:79-112) ----------------------------
// One record = four NUL-terminated strings in its batch's text arena (no per-record allocation: the reader is a single
// thread and sets the pace of the whole pipeline).
struct Seq { size_t name = 0, comment = 0, seq = 0, qual = 0; int l_name = 0, l_seq = 0, l_qual = 0; bool has_comment = false, has_qual = false;
	char *base = nullptr;   /* the text the offsets refer to when it is not the batch's own arena (a parsed block, see ParFile) */ };
typedef std::vector<char> Arena;

// does any of the n bytes at p hold a blank or control character (<= ' ')?  Eight bytes per step.
static inline bool has_blank(const char *p, size_t n) {
	const uint64_t ones = ~0ull / 255;
	size_t i = 0;
	for (; i + 8 <= n; i += 8) { uint64_t w; memcpy(&w, p + i, 8); if ((w - ones * 0x21) & ~w & (ones * 0x80)) return true; }
	for (; i < n; ++i) if ((unsigned char)p[i] <= ' ') return true;
	return false;
}

// One plain four-line FASTQ record at b (the text ends at e): appended to A as name\0 comment\0 bases\0 qualities\0, its successor's
// address returned -- or null, nothing appended, when the record is not of that kind or not completely there (the general reader
// decides then).  Both the streaming reader and the block parsers below go through here, so they accept exactly the same records.
static inline const char *parse_fast_record(const char *b, const char *e, Seq &s, Arena &A)
{
	if (b >= e || *b != '@') return nullptr;
	const char *n1 = (const char*)memchr(b, '\n', (size_t)(e - b)); if (!n1 || n1 + 1 >= e) return nullptr;
	const char *n2 = (const char*)memchr(n1 + 1, '\n', (size_t)(e - n1 - 1)); if (!n2 || n2 + 1 >= e || n2[1] != '+') return nullptr;
	const char *n3 = (const char*)memchr(n2 + 1, '\n', (size_t)(e - n2 - 1)); if (!n3 || n3 + 1 >= e) return nullptr;
	const char *n4 = (const char*)memchr(n3 + 1, '\n', (size_t)(e - n3 - 1)); if (!n4) return nullptr;
	const char *sq = n1 + 1, *ql = n3 + 1;
	const size_t ls = (size_t)(n2 - sq), lq = (size_t)(n4 - ql);
	if (ls == 0 || ls != lq || n1[-1] == '\r' || n2[-1] == '\r' || n4[-1] == '\r') return nullptr;
	if (sq[0] == '>' || sq[0] == '+' || sq[0] == '@') return nullptr;              // the general reader treats these as record structure
	if (has_blank(sq, ls)) return nullptr;                                         // blanks / control characters: general path
	const char *h = b + 1, *he = n1, *ne = h;
	while (ne < he && !isspace((unsigned char)*ne)) ++ne;
	s = Seq();
	s.name = A.size(); s.l_name = (int)(ne - h);
	A.insert(A.end(), h, ne); A.push_back(0);
	s.comment = A.size();
	if (ne < he) { s.has_comment = true; A.insert(A.end(), ne + 1, he); }
	A.push_back(0);
	s.seq = A.size(); s.l_seq = (int)ls; A.insert(A.end(), sq, sq + ls); A.push_back(0);
	s.qual = A.size(); s.l_qual = (int)lq; s.has_qual = true; A.insert(A.end(), ql, ql + lq); A.push_back(0);
	return n4 + 1;
}

// A small pool of worker threads for the input stage: parsing blocks of plain FASTQ files (ParFile) and inflating the blocks of BGZF files (BgzfPipe).
// A task carries its owner, so that a file that is closed early can take its queued tasks back.
struct ParPool {
	struct Task { void *owner; std::function<void()> run; };
	std::mutex m; std::condition_variable cv; std::deque<Task> q; bool stop = false; std::vector<std::thread> th;
	explicit ParPool(int n) { for (int i = 0; i < n; ++i) th.emplace_back([this] { loop(); }); }
	~ParPool() { { std::lock_guard<std::mutex> l(m); stop = true; } cv.notify_all(); for (auto &t : th) t.join(); }
	void push(void *owner, std::function<void()> f) { { std::lock_guard<std::mutex> l(m); q.push_back(Task{owner, std::move(f)}); } cv.notify_one(); }
	int drop(void *owner) { std::lock_guard<std::mutex> l(m); int n = 0; for (auto it = q.begin(); it != q.end();) if (it->owner == owner) { it = q.erase(it); ++n; } else ++it; return n; }
	void loop() {
		for (;;) {
			Task t;
			{
				std::unique_lock<std::mutex> l(m);
				cv.wait(l, [&] { return stop || !q.empty(); });
				if (q.empty()) return;
				t = std::move(q.front()); q.pop_front();
			}
			t.run();
		}
	}
};

// ---- BGZF input (bgzip; the block-compressed gzip of htslib): independent blocks of at most 64 KiB, each a gzip member whose header says how long it is
// (extra field "BC", SAM spec 4.1), so the blocks of a file can be inflated side by side -- one zlib stream inflates ~210 MB/s of FASTQ on a host core,
// 0.7 M records/s per file, which is what `bwa-amd mem` delivered for ANY gzip input ("compressed input at the product's speed").  The file is
// mapped; one thread walks the block headers and queues groups of blocks (~0.5 MB compressed) to the pool; the reader takes the inflated groups in file
// order.  What comes out is the same byte stream gzread would deliver (bseq_read over kseq.h's gzread, bwa.c:79-112) and goes through the same parser.
// A plain gzip file (one stream, no block sizes) cannot be split and keeps its single inflating thread.
struct BgzfGroup { const unsigned char *src = nullptr; size_t src_len = 0; std::vector<char> out; size_t out_len = 0; bool done = false, bad = false; };
struct BgzfPipe {
	int fd = -1; const unsigned char *map = nullptr; size_t size = 0; ParPool *pool = nullptr; std::string path;
	std::mutex m; std::condition_variable cv;
	std::deque<std::shared_ptr<BgzfGroup>> inflight; bool io_done = false, stop = false, bad = false; int pending = 0;
	std::thread io; std::shared_ptr<BgzfGroup> cur; size_t cpos = 0;
	size_t start_off = 0, drop = 0;      // where the stream starts: the offset of a block in the file, and the leading bytes of the text from there that are not delivered (0, 0: the whole file)
	// total length of the BGZF block at p (header .. trailer), or 0 if p does not start one
	static size_t block_len(const unsigned char *p, size_t n) {
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
	static bool is_bgzf(const char *fn) {
		const int f = ::open(fn, O_RDONLY); if (f < 0) return false;
		unsigned char h[64]; const ssize_t n = pread(f, h, sizeof h, 0); struct stat st; const bool reg = fstat(f, &st) == 0 && S_ISREG(st.st_mode);
		::close(f);
		if (!reg || n < 18) return false;
		// (block_len wants the whole block in view: here only its header is, so the length is read without the bound)
		if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return false;
		const size_t xlen = h[10] | (size_t)h[11] << 8;
		for (size_t o = 12; o + 6 <= 12 + xlen && o + 6 <= (size_t)n;) { const size_t sl = h[o + 2] | (size_t)h[o + 3] << 8; if (h[o] == 'B' && h[o + 1] == 'C' && sl == 2) return true; o += 4 + sl; }
		return false;
	}
	~BgzfPipe() {
		{ std::lock_guard<std::mutex> l(m); stop = true; }
		cv.notify_all();
		if (io.joinable()) io.join();
		if (pool) { const int n = pool->drop(this); std::unique_lock<std::mutex> l(m); pending -= n; cv.wait(l, [&] { return pending == 0; }); }
		if (map) munmap((void*)map, size);
		if (fd >= 0) ::close(fd);
	}
	bool open(const char *fn, ParPool *pl, size_t block_off = 0, size_t drop_bytes = 0) {
		fd = ::open(fn, O_RDONLY); if (fd < 0) return false;
		struct stat st; if (fstat(fd, &st) != 0 || st.st_size <= 0) return false;
		size = (size_t)st.st_size;
		if (block_off > size) return false;
		start_off = block_off; drop = drop_bytes;
		void *mp = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
		if (mp == MAP_FAILED) return false;
		madvise(mp, size, MADV_SEQUENTIAL);
		map = (const unsigned char*)mp; pool = pl; path = fn;
		io = std::thread([this] { scan(); });
		return true;
	}
	static void inflate_group(BgzfGroup &G) {
		size_t want = 0;
		for (size_t o = 0; o < G.src_len;) { const size_t bl = block_len(G.src + o, G.src_len - o); if (!bl) { G.bad = true; return; } const unsigned char *t = G.src + o + bl - 4; want += t[0] | (size_t)t[1] << 8 | (size_t)t[2] << 16 | (size_t)t[3] << 24; o += bl; }
		if (G.out.size() < want) G.out.resize(want);
		z_stream z; memset(&z, 0, sizeof z);
		if (inflateInit2(&z, -15) != Z_OK) { G.bad = true; return; }
		size_t w = 0;
		for (size_t o = 0; o < G.src_len && !G.bad;) {
			const size_t bl = block_len(G.src + o, G.src_len - o);
			const unsigned char *b = G.src + o, *t = b + bl - 8;
			const size_t xlen = b[10] | (size_t)b[11] << 8, isize = t[4] | (size_t)t[5] << 8 | (size_t)t[6] << 16 | (size_t)t[7] << 24;
			const uint32_t crc = t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
			z.next_in = (Bytef*)(b + 12 + xlen); z.avail_in = (uInt)(bl - 12 - xlen - 8);
			Bytef spare[8];                                            // (an empty block -- bgzip's end-of-file marker -- still needs somewhere to "write")
			z.next_out = isize ? (Bytef*)G.out.data() + w : spare; z.avail_out = isize ? (uInt)isize : (uInt)sizeof spare;
			const int rc = inflate(&z, Z_FINISH);
			if (rc != Z_STREAM_END || z.total_out != isize || (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef*)G.out.data() + w, (uInt)isize) != crc) G.bad = true;
			w += isize; o += bl;
			inflateReset(&z);
		}
		inflateEnd(&z);
		G.out_len = w;
	}
	void scan() {
		size_t off = start_off;
		const size_t group_bytes = getenv("BWAGPU_CLI_BGZF_GROUP") ? (size_t)atoll(getenv("BWAGPU_CLI_BGZF_GROUP")) : (size_t)512 << 10;   // (tests: a block per group)
		while (off < size) {
			{ std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return stop || inflight.size() < 16; }); if (stop) break; }
			size_t end = off;
			while (end < size && end - off < group_bytes) { const size_t bl = block_len(map + end, size - end); if (!bl) break; end += bl; }
			if (end == off) { std::lock_guard<std::mutex> l(m); bad = true; break; }       // not a BGZF block where one must start: a corrupt or truncated file
			std::shared_ptr<BgzfGroup> G(new BgzfGroup());
			G->src = map + off; G->src_len = end - off;
			BgzfGroup *gp = G.get();
			{ std::lock_guard<std::mutex> l(m); inflight.push_back(G); ++pending; }
			auto work = [this, gp] { inflate_group(*gp); std::lock_guard<std::mutex> l(m); gp->done = true; --pending; cv.notify_all(); };
			if (pool) pool->push(this, work); else work();
			off = end;
		}
		{ std::lock_guard<std::mutex> l(m); io_done = true; }
		cv.notify_all();
	}
	// the next bytes of the inflated stream (blocking; in file order): > 0 bytes, 0 at the end, -1 for a damaged file
	int read(char *dst, size_t cap) {
		for (;;) {
			if (cur && drop) { const size_t d = drop < cur->out_len - cpos ? drop : cur->out_len - cpos; cpos += d; drop -= d; }
			if (cur && cpos < cur->out_len) { const size_t n = cur->out_len - cpos < cap ? cur->out_len - cpos : cap; memcpy(dst, cur->out.data() + cpos, n); cpos += n; return (int)n; }
			cur.reset();
			std::unique_lock<std::mutex> l(m);
			cv.wait(l, [&] { return (!inflight.empty() && inflight.front()->done) || (inflight.empty() && io_done); });
			if (inflight.empty()) return bad ? -1 : 0;
			cur = std::move(inflight.front()); inflight.pop_front(); cpos = 0;
			l.unlock(); cv.notify_all();
			if (cur->bad) return -1;
		}
	}
};

struct Reader {
	std::unique_ptr<BgzfPipe> bg;      // a BGZF file: blocks inflated by the pool (else fp / raw_fd)
	gzFile fp = nullptr; int raw_fd = -1; std::vector<char> buf; int pos = 0, len = 0; int last = 0; bool eof = false;
	// The file is read (and, for gzip input, inflated) by a thread of its own, one buffer ahead of the parser: inflating a FASTQ stream
	// costs several times what parsing it does, and for paired input the two files' streams then inflate side by side.
	std::thread ahead; std::mutex m; std::condition_variable cv;
	std::vector<char> nbuf; int nlen = 0; bool nfull = false, stop = false;
	~Reader() {
		if (ahead.joinable()) { { std::lock_guard<std::mutex> l(m); stop = true; } cv.notify_all(); ahead.join(); }      // (a read in flight completes: the pipe below is still alive)
		bg.reset();
		if (fp) gzclose(fp); else if (raw_fd >= 0) ::close(raw_fd);
	}
	// A regular file that does not start with the gzip magic is read with read(2) straight into the buffer: zlib's transparent mode
	// would copy every byte twice more.  Everything else (gzip files, stdin) goes through zlib as in the reference (kseq.h over gzread,
	// fastmap.c:357-372).
	bool open(const char *fn, ParPool *pool = nullptr) {
		size_t cap = 1 << 20;
		if (getenv("BWAGPU_CLI_BUF")) { cap = (size_t)atoll(getenv("BWAGPU_CLI_BUF")); if (cap < 8) cap = 8; }   // (tests: records that straddle buffer ends)
		buf.resize(cap); nbuf.resize(cap);
		if (strcmp(fn, "-")) {
			const int fd = ::open(fn, O_RDONLY);
			if (fd < 0) return false;
			unsigned char magic[2] = { 0, 0 };
			struct stat st;
			if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && pread(fd, magic, 2, 0) >= 0 && !(magic[0] == 0x1f && magic[1] == 0x8b)) { raw_fd = fd; return true; }
			if (pool && !getenv("BWAGPU_CLI_NO_BGZF") && BgzfPipe::is_bgzf(fn)) {
				bg.reset(new BgzfPipe());
				if (bg->open(fn, pool)) { ::close(fd); return true; }
				bg.reset();
			}
			fp = gzdopen(fd, "r");
			if (!fp) ::close(fd);
		} else fp = gzdopen(fileno(stdin), "r");
		if (fp) gzbuffer(fp, 1 << 20);
		return fp != nullptr;
	}
	// a BGZF file from a virtual offset on: the block at block_off, without the first drop_bytes of the text from there (pool may be null: the blocks are inflated by the pipe's own thread)
	bool open_bgzf_at(const char *fn, ParPool *pool, size_t block_off, size_t drop_bytes) {
		size_t cap = 1 << 20;
		if (getenv("BWAGPU_CLI_BUF")) { cap = (size_t)atoll(getenv("BWAGPU_CLI_BUF")); if (cap < 8) cap = 8; }
		buf.resize(cap); nbuf.resize(cap);
		bg.reset(new BgzfPipe());
		if (bg->open(fn, pool, block_off, drop_bytes)) return true;
		bg.reset();
		return false;
	}
	int read_some(char *dst, size_t cap) {
		int n;
		if (bg) n = bg->read(dst, cap);
		else if (raw_fd >= 0) { do n = (int)::read(raw_fd, dst, cap); while (n < 0 && errno == EINTR); }
		else n = gzread(fp, dst, (unsigned)cap);
		return n;
	}
	void read_ahead() {
		for (;;) {
			{ std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return !nfull || stop; }); if (stop) return; }
			const int n = read_some(nbuf.data(), nbuf.size());       // (nbuf belongs to this thread while !nfull)
			{ std::lock_guard<std::mutex> l(m); nlen = n; nfull = true; }
			cv.notify_all();
			if (n <= 0) return;
		}
	}
	bool fill() {
		if (eof) return false;
		if (!ahead.joinable()) ahead = std::thread([this] { read_ahead(); });
		{
			std::unique_lock<std::mutex> l(m);
			cv.wait(l, [&] { return nfull; });
			buf.swap(nbuf); len = nlen; nfull = false;
		}
		cv.notify_all();
		pos = 0;
		if (len < 0 && bg) { fprintf(stderr, "[E::%s] `%s' is a damaged or truncated BGZF file (a block does not inflate to its recorded size and checksum)\n", "main_mem", bg->path.c_str()); exit(EXIT_FAILURE); }
		if (len <= 0) { len = 0; eof = true; return false; }
		return true;
	}
	int getc_() { if (pos >= len && !fill()) return -1; return (unsigned char)buf[pos++]; }
	// append the bytes up to the next delimiter (newline, or any white space when `space`) to `out` and consume the delimiter;
	// returns the delimiter, or -1 at end of input.  Whole buffer spans are copied at once.
	int until(bool space, Arena *out) {
		for (;;) {
			if (pos >= len && !fill()) return -1;
			const char *b = buf.data() + pos; const int n = len - pos; int k;
			if (space) { for (k = 0; k < n && !isspace((unsigned char)b[k]); ++k) {} }
			else { const char *q = (const char*)memchr(b, '\n', (size_t)n); k = q ? (int)(q - b) : n; }
			if (out) out->insert(out->end(), b, b + k);
			pos += k;
			if (k < n) return (unsigned char)buf[pos++];
		}
	}
	// drop the characters of A[from..) for which `drop` holds
	template <class P> static void squeeze(Arena &A, size_t from, P drop) { size_t w = from; for (size_t i = from; i < A.size(); ++i) if (!drop((unsigned char)A[i])) A[w++] = A[i]; A.resize(w); }
	// The common case -- a four-line FASTQ record that lies completely in the buffer, without '\r' or blanks in the sequence --
	// located with four memchr calls and appended in bulk; anything else goes through the general reader below.
	bool read_fast(Seq &s, Arena &A) {
		if (last != 0 || pos >= len) return false;
		const char *next = parse_fast_record(buf.data() + pos, buf.data() + len, s, A);
		if (!next) return false;
		pos = (int)(next - buf.data());
		return true;
	}
	bool read(Seq &s, Arena &A) {
		if (read_fast(s, A)) return true;
		int c;
		if (last == 0) { while ((c = getc_()) != -1 && c != '>' && c != '@') {} if (c == -1) return false; last = c; }
		s = Seq();
		s.name = A.size();
		c = until(true, &A);
		size_t name_end = A.size();
		A.push_back(0);
		s.comment = A.size();
		if (c != '\n' && c != -1) { s.has_comment = true; until(false, &A); while (A.size() > s.comment && A.back() == '\r') A.pop_back(); }
		else while (name_end > s.name && A[name_end - 1] == '\r') A[--name_end] = 0;
		s.l_name = (int)(name_end - s.name);
		A.push_back(0);
		s.seq = A.size();
		while ((c = getc_()) != -1 && c != '>' && c != '+' && c != '@') {
			if (c == '\n') continue;
			A.push_back((char)c);
			until(false, &A);
		}
		bool ws = false;
		for (size_t i = s.seq; i < A.size(); ++i) if (isspace((unsigned char)A[i])) { ws = true; break; }
		if (ws) squeeze(A, s.seq, [](unsigned char ch) { return isspace(ch) != 0; });
		s.l_seq = (int)(A.size() - s.seq);
		A.push_back(0);
		s.qual = A.size();
		if (c == '>' || c == '@') last = c; else last = 0;
		if (c != '+') { A.push_back(0); return true; }
		if (until(false, nullptr) == -1) { A.push_back(0); last = 0; return false; } // '+' line, then end of input: kseq_read's "no quality string" error (-2), the record is dropped
		s.has_qual = true;
		while (A.size() - s.qual < (size_t)s.l_seq) {
			const size_t before = A.size();
			c = until(false, &A);
			const bool got = A.size() > before;
			if (memchr(A.data() + before, '\r', A.size() - before)) squeeze(A, before, [](unsigned char ch) { return ch == '\r'; });
			if (c == -1 && !got) break;
		}
		s.l_qual = (int)(A.size() - s.qual);
		A.push_back(0);
		last = 0;
		// kseq_read returns -2 when the quality string and the sequence differ in length (kseq.h:219): bseq_read's loop ends there
		// (bwa.c:88), the record is dropped and the batch closed; the next batch resumes scanning for a header after the text the
		// quality loop has consumed.  Passing such a record on would also let the SAM writer read qual[0..l_seq) out of bounds.
		if (s.l_qual != s.l_seq) return false;
		return true;
	}
};
