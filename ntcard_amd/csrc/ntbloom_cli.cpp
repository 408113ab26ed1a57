// ntbloom_cli.cpp — `ntbloom`: Bloom filters of every k-mer of the input, in the reference's layout (vendor/ntHash/lib/BloomFilter.hpp), sized from ntcard's F0
// (include/ntcard_hip.h: ntc_bloom_*; DESIGN.md §4 "Bloom filters"), and counting filters and the filter of the solid k-mers, sized from its f_i
// (ntc_cbloom_*; DESIGN.md §4 "Counting filters and solid k-mers").
//   ntbloom build -k K [-H N] [--blocked] [--strand=canonical|forward|reverse] (-m BITS | --distinct N --fpr P | --hist FILE --fpr P) -o OUT.bf FILE...
//                               inserts every k-mer of the files.  The filter has BITS bits, or what ntc_bloom_size gives for N distinct k-mers at false
//                               positive rate P; --hist takes N from the F0 line of a `.hist` file as ntcard writes it, so that
//                               `ntcard -k 32 -p s reads.fq && ntbloom build -k 32 --hist s_k32.hist --fpr 0.01 -o s.bf reads.fq` composes.  -H: hashes per
//                               k-mer (default 3).  OUT.bf is written whole or not at all (ntc_bloom_write).  --blocked: a BLOCKED filter (ntc_bbloom_*;
//                               DESIGN.md §4 "Blocked filters"), every bit of a k-mer in one 64-byte block: BITS is a multiple of 512, --distinct and --hist
//                               size by ntc_bbloom_size, the file has a magic of its own.  --blocked with `count` is refused: there is no blocked counting filter
//   ntbloom count -k K [-H N] [--strand=...] (-m COUNTERS | --distinct N --fpr P | --hist FILE --fpr P) -o OUT.cbf FILE...
//                               the same with 8-bit counters: every k-mer adds one to each of its N counters, saturating at 255 (ntc_cbloom_write)
//   ntbloom solid --min-count C [--fpr P --hist FILE [-H N] [--blocked]] -o OUT.bf IN.cbf [FILE...]
//                               the plain filter of the k-mers counted at least C times (k and strand come from IN.cbf).  Without input files IN.cbf is
//                               thresholded: OUT.bf has as many bits as IN.cbf counters and its hash count.  With input files, --hist and --fpr the
//                               files are walked again and every k-mer whose count in IN.cbf is >= C goes into a filter sized by ntc_bloom_size for
//                               n = F0 - sum_{i<C} f_i of the `.hist` file (its F0 line and its "i\tf_i" lines), N hashes (default 3); --blocked makes that
//                               filter a blocked one (ntc_bbloom_size, ntc_bbloom_insert_solid_device) and is refused without input files — a threshold has
//                               the counting filter's positions, which are not blocked:
//                               `ntcard -k 32 -p s reads.fq && ntbloom count -k 32 --hist s_k32.hist --fpr 0.01 -o s.cbf reads.fq &&
//                                ntbloom solid --min-count 2 --hist s_k32.hist --fpr 0.01 -o solid.bf s.cbf reads.fq && ntbloom query solid.bf other.fq`
//   ntbloom query [--min-count C] F.bf|F.cbf|F.bbf FILE...
//                               one TSV row per record: name, length, windows, hits, hits / windows (k, hashes and strand come from the file, whose
//                               magic says which of the three kinds it is).  On a .cbf a hit is a window whose count is >= C (default 1); --min-count with a .bf is refused
//   ntbloom info F.bf|F.cbf|F.bbf  the header (a blocked filter: its block size too), and with a GPU the popcount, the occupancy and the false positive
//                               rate it implies (a .cbf: the counters that are not 0, the saturated ones, the rate of a false "count >= 1"; a blocked
//                               filter: the rate from the histogram of its blocks' set bits); without one the header alone
// Input: FASTA (a record's lines are joined) and FASTQ, plain or through the decompressor its extension names (cli_common.hpp: LineReader).  One thread
// reads records into a pinned batch of at most 256 MiB, uploads it and calls ntc_bloom_insert_device / ntc_bloom_query_device.  SAM is not read here.
// Every malformed argument is refused with a message that names it, before a device is looked for.
#include <hip/hip_runtime_api.h>

#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "cli_common.hpp"

namespace cli {
const char* const kProgram = "ntbloom";
}

namespace {

const char* const kStrand[3] = {"canonical", "forward", "reverse"};
constexpr size_t kBatchBytes = 256u << 20;

int usage(const char* why, const char* what = nullptr)
{
	if (what)
		std::fprintf(stderr, "ntbloom: %s: %s\n", why, what);
	else
		std::fprintf(stderr, "ntbloom: %s\n", why);
	std::fprintf(stderr,
	             "usage: ntbloom build -k K [-H N] [--blocked] [--strand=canonical|forward|reverse] (-m BITS | --distinct N --fpr P | --hist FILE --fpr P) -o OUT.bf FILE...\n"
	             "       ntbloom count -k K [-H N] [--strand=canonical|forward|reverse] (-m COUNTERS | --distinct N --fpr P | --hist FILE --fpr P) -o OUT.cbf FILE...\n"
	             "       ntbloom solid --min-count C [--fpr P --hist FILE [-H N] [--blocked]] -o OUT.bf IN.cbf [FILE...]\n"
	             "       ntbloom query [--min-count C] F.bf|F.cbf|F.bbf FILE...\n"
	             "       ntbloom info F.bf|F.cbf|F.bbf\n");
	return EXIT_FAILURE;
}

int fail_lib()
{
	std::fprintf(stderr, "ntbloom: %s\n", ntc_last_error());
	return EXIT_FAILURE;
}

int fail_hip(const char* what, hipError_t rc)
{
	std::fprintf(stderr, "ntbloom: %s: %s\n", what, hipGetErrorString(rc));
	return EXIT_FAILURE;
}

bool parse_u64(const char* s, uint64_t& out)
{
	if (!s || !*s || *s == '-' || *s == '+') return false;
	char* end = nullptr;
	errno = 0;
	const unsigned long long v = std::strtoull(s, &end, 10);
	if (errno != 0 || *end != '\0') return false;
	out = v;
	return true;
}

bool parse_double(const char* s, double& out)
{
	if (!s || !*s) return false;
	char* end = nullptr;
	errno = 0;
	const double v = std::strtod(s, &end);
	if (errno != 0 || *end != '\0') return false;
	out = v;
	return true;
}

// the F0 line of a `.hist` file as ntc_write_hist writes it: "F0\t<integer>"
bool hist_f0(const char* path, uint64_t& f0)
{
	FILE* f = std::fopen(path, "rb");
	if (!f) return false;
	char line[256];
	bool found = false;
	while (!found && std::fgets(line, sizeof line, f)) {
		if (std::strncmp(line, "F0\t", 3) != 0) continue;
		std::string v(line + 3);
		while (!v.empty() && (v.back() == '\n' || v.back() == '\r'))
			v.pop_back();
		found = parse_u64(v.c_str(), f0);
		break;
	}
	std::fclose(f);
	return found;
}

// F0 - sum_{i < c} f_i of a `.hist` file: its F0 line and its "i\tf_i" lines, i = 1, 2, ... as ntc_write_hist writes them.  -1: no F0 line; -2: the f_i
// lines stop below c - 1; -3: the lines sum to more than F0; 0: n is set
int hist_solid_n(const char* path, uint64_t c, uint64_t& n)
{
	uint64_t f0 = 0;
	if (!hist_f0(path, f0)) return -1;
	FILE* f = std::fopen(path, "rb");
	if (!f) return -1;
	char line[256];
	uint64_t next = 1, below = 0;
	while (next < c && std::fgets(line, sizeof line, f)) {
		char* tab = std::strchr(line, '\t');
		if (!tab) continue;
		*tab = '\0';
		uint64_t i = 0, fi = 0;
		if (!parse_u64(line, i) || i != next) continue; // (the F1 and F0 lines, and whatever is no "i\tf_i" line of the next i)
		std::string v(tab + 1);
		while (!v.empty() && (v.back() == '\n' || v.back() == '\r'))
			v.pop_back();
		if (!parse_u64(v.c_str(), fi)) break;
		below += fi;
		++next;
	}
	std::fclose(f);
	if (next < c) return -2;
	if (below > f0) return -3;
	n = f0 - below;
	return 0;
}

// the kind of a filter file by its magic: a counting filter, a blocked filter, or plain — which is also anything else (ntc_bloom_read then says what is
// wrong with it)
enum Kind { kPlain = 0, kCounting = 1, kBlocked = 2 };
Kind file_kind(const char* path)
{
	FILE* f = std::fopen(path, "rb");
	if (!f) return kPlain;
	char magic[8] = {0};
	const bool whole = std::fread(magic, 1, 8, f) == 8;
	std::fclose(f);
	if (whole && std::memcmp(magic, "NTCCB1\0\0", 8) == 0) return kCounting;
	if (whole && std::memcmp(magic, "NTCBB1\0\0", 8) == 0) return kBlocked;
	return kPlain;
}

// device and pinned memory of one run, freed on every way out
struct Buffers {
	unsigned char* d_filter = nullptr;
	unsigned char* d_counters = nullptr; // solid: the counting filter beside the plain one
	unsigned char* d_bases = nullptr;
	unsigned char* h_bases = nullptr; // pinned
	uint32_t* d_counts = nullptr;     // query: [2][seq_cap]
	size_t seq_cap = 0;
	~Buffers()
	{
		if (d_filter) (void)hipFree(d_filter);
		if (d_counters) (void)hipFree(d_counters);
		if (d_bases) (void)hipFree(d_bases);
		if (h_bases) (void)hipHostFree(h_bases);
		if (d_counts) (void)hipFree(d_counts);
	}
};

// The record reader: one sequence per FASTA record (its lines joined, CR bytes and case kept) or FASTQ record (its second line), appended to the batch; a
// full batch goes to `flush`.  A sequence longer than the batch is cut with k - 1 bytes of overlap, so no window is lost or counted twice — only for build:
// a query needs every record whole.
struct Reader {
	Buffers& b;
	uint32_t k;
	bool whole; // query: records are never cut
	size_t fill = 0;
	std::vector<uint64_t> offsets{0};
	std::vector<std::string> names;
	bool keep_names; // query: the rows are printed by name
	int (*flush_fn)(Reader&, void*);
	void* ctx;
	Reader(Buffers& b_, uint32_t k_, bool whole_, int (*fn)(Reader&, void*), void* ctx_) : b(b_), k(k_), whole(whole_), keep_names(whole_), flush_fn(fn), ctx(ctx_) {}
	int flush()
	{
		if (offsets.size() == 1) return EXIT_SUCCESS;
		const int rc = flush_fn(*this, ctx);
		fill = 0;
		offsets.assign(1, 0);
		names.clear();
		return rc;
	}
	int add(const std::string& name, const std::string& seq)
	{
		size_t pos = 0;
		for (;;) {
			const size_t left = seq.size() - pos;
			if (left > kBatchBytes - fill && fill != 0) {
				if (int rc = flush()) return rc;
			}
			if (left <= kBatchBytes - fill) {
				std::memcpy(b.h_bases + fill, seq.data() + pos, left);
				fill += left;
				offsets.push_back(fill);
				if (keep_names) names.push_back(name);
				return EXIT_SUCCESS;
			}
			if (whole) {
				std::fprintf(stderr, "ntbloom: record %s has %zu bases: a query takes records of at most %zu\n", name.c_str(), seq.size(), kBatchBytes);
				return EXIT_FAILURE;
			}
			std::memcpy(b.h_bases, seq.data() + pos, kBatchBytes); // (fill == 0 here)
			fill = kBatchBytes;
			offsets.push_back(fill);
			if (int rc = flush()) return rc;
			pos += kBatchBytes - (k - 1);
		}
	}
	int read_file(const char* path)
	{
		cli::LineReader in(path);
		if (!in.ok()) {
			std::fprintf(stderr, "ntbloom: cannot read %s\n", path);
			return EXIT_FAILURE;
		}
		std::string line, name, seq;
		if (!in.getline(line)) return EXIT_SUCCESS; // an empty file
		auto name_of = [](const std::string& header) {
			size_t e = 1;
			while (e < header.size() && header[e] != ' ' && header[e] != '\t' && header[e] != '\r')
				++e;
			return header.substr(1, e - 1);
		};
		if (line[0] == '>') {
			name = name_of(line);
			bool more = true;
			while (more) {
				more = in.getline(line);
				if (!more || (!line.empty() && line[0] == '>')) {
					if (int rc = add(name, seq)) return rc;
					seq.clear();
					if (more) name = name_of(line);
				} else {
					seq += line;
				}
			}
		} else if (line[0] == '@') {
			for (;;) {
				name = name_of(line);
				std::string plus, qual;
				if (!in.getline(seq) || !in.getline(plus) || !in.getline(qual)) break; // (a record counts once its quality line could be read)
				if (int rc = add(name, seq)) return rc;
				if (!in.getline(line)) break;
			}
		} else {
			std::fprintf(stderr, "ntbloom: %s is neither FASTA nor FASTQ\n", path);
			return EXIT_FAILURE;
		}
		return EXIT_SUCCESS;
	}
};

bool alloc_batch(Buffers& b)
{
	hipError_t rc = hipHostMalloc((void**)&b.h_bases, kBatchBytes, hipHostMallocDefault);
	if (rc == hipSuccess) rc = hipMalloc((void**)&b.d_bases, kBatchBytes);
	if (rc == hipSuccess) return true;
	(void)fail_hip("cannot allocate the batch buffers", rc);
	return false;
}

struct BuildCtx {
	ntc_bloom_header h;
	bool counting = false;       // count: d_filter holds counters
	bool blocked = false;        // build --blocked, solid --blocked: d_filter is a blocked filter
	ntc_bloom_header c{};        // solid: the counting filter in d_counters ...
	uint32_t min_count = 0;      // ... and the count a k-mer needs (0: not solid)
};
int build_flush(Reader& r, void* ctx)
{
	BuildCtx& c = *static_cast<BuildCtx*>(ctx);
	const hipError_t rc = hipMemcpy(r.b.d_bases, r.b.h_bases, r.fill, hipMemcpyHostToDevice);
	if (rc != hipSuccess) return fail_hip("cannot upload a batch", rc);
	uint64_t n = 0;
	int rc2;
	if (c.min_count)
		rc2 = (c.blocked ? ntc_bbloom_insert_solid_device : ntc_bloom_insert_solid_device)(0, nullptr, r.b.d_filter, c.h.m_bits, c.h.n_hash, r.b.d_counters, c.c.m_bits, c.c.n_hash,
		                                                                                   c.min_count, c.h.k, c.h.strand, r.b.d_bases, r.offsets.data(), r.offsets.size() - 1, &n);
	else if (c.blocked)
		rc2 = ntc_bbloom_insert_device(0, nullptr, r.b.d_filter, c.h.m_bits, c.h.n_hash, c.h.k, c.h.strand, r.b.d_bases, r.offsets.data(), r.offsets.size() - 1, &n);
	else if (c.counting)
		rc2 = ntc_cbloom_insert_device(0, nullptr, r.b.d_filter, c.h.m_bits, c.h.n_hash, c.h.k, c.h.strand, r.b.d_bases, r.offsets.data(), r.offsets.size() - 1, &n);
	else
		rc2 = ntc_bloom_insert_device(0, nullptr, r.b.d_filter, c.h.m_bits, c.h.n_hash, c.h.k, c.h.strand, r.b.d_bases, r.offsets.data(), r.offsets.size() - 1, &n);
	if (rc2 != 0) return fail_lib();
	c.h.n_inserted += n;
	return EXIT_SUCCESS;
}

struct QueryCtx {
	ntc_bloom_header h;
	bool counting = false;
	bool blocked = false;
	uint32_t min_count = 1;
	std::vector<uint32_t> counts;
};
int query_flush(Reader& r, void* ctx)
{
	QueryCtx& c = *static_cast<QueryCtx*>(ctx);
	const size_t n_seqs = r.offsets.size() - 1;
	if (n_seqs > r.b.seq_cap) {
		if (r.b.d_counts) (void)hipFree(r.b.d_counts);
		r.b.d_counts = nullptr;
		r.b.seq_cap = std::max(n_seqs, 2 * r.b.seq_cap);
		const hipError_t rc = hipMalloc((void**)&r.b.d_counts, r.b.seq_cap * 8);
		if (rc != hipSuccess) return fail_hip("cannot allocate the result arrays", rc);
	}
	hipError_t rc = hipMemcpy(r.b.d_bases, r.b.h_bases, r.fill ? r.fill : 1, hipMemcpyHostToDevice);
	if (rc != hipSuccess) return fail_hip("cannot upload a batch", rc);
	uint32_t* d_w = r.b.d_counts;
	uint32_t* d_h = r.b.d_counts + r.b.seq_cap;
	const int rc2 = c.counting ? ntc_cbloom_query_device(0, nullptr, r.b.d_filter, c.h.m_bits, c.h.n_hash, c.h.k, c.h.strand, r.b.d_bases, r.offsets.data(), n_seqs, c.min_count, d_w, d_h)
	                : c.blocked ? ntc_bbloom_query_device(0, nullptr, r.b.d_filter, c.h.m_bits, c.h.n_hash, c.h.k, c.h.strand, r.b.d_bases, r.offsets.data(), n_seqs, d_w, d_h)
	                            : ntc_bloom_query_device(0, nullptr, r.b.d_filter, c.h.m_bits, c.h.n_hash, c.h.k, c.h.strand, r.b.d_bases, r.offsets.data(), n_seqs, d_w, d_h);
	if (rc2 != 0) return fail_lib();
	c.counts.resize(2 * n_seqs);
	rc = hipMemcpy(c.counts.data(), d_w, n_seqs * 4, hipMemcpyDeviceToHost);
	if (rc == hipSuccess) rc = hipMemcpy(c.counts.data() + n_seqs, d_h, n_seqs * 4, hipMemcpyDeviceToHost);
	if (rc != hipSuccess) return fail_hip("cannot fetch the results", rc);
	for (size_t i = 0; i < n_seqs; ++i) {
		const uint32_t w = c.counts[i], h = c.counts[n_seqs + i];
		std::printf("%s\t%llu\t%u\t%u\t%.6f\n", r.names[i].c_str(), (unsigned long long)(r.offsets[i + 1] - r.offsets[i]), w, h, w ? (double)h / (double)w : 0.0);
	}
	return EXIT_SUCCESS;
}

// the bytes of a filter's image: a plain filter's bits, a counting filter's counters
size_t image_bytes(const ntc_bloom_header& h, bool counting) { return counting ? h.m_bits : (h.m_bits + 7) / 8; }

bool upload_filter(Buffers& b, const ntc_bloom_header& h, const std::vector<unsigned char>* image, bool counting = false, unsigned char** where = nullptr)
{
	unsigned char*& d = where ? *where : b.d_filter;
	const size_t padded = (image_bytes(h, counting) + 3) & ~(size_t)3;
	hipError_t rc = hipMalloc((void**)&d, padded);
	if (rc == hipSuccess) rc = hipMemset(d, 0, padded);
	if (rc == hipSuccess && image) rc = hipMemcpy(d, image->data(), image->size(), hipMemcpyHostToDevice);
	if (rc == hipSuccess) return true;
	(void)fail_hip("cannot bring the filter to the device", rc);
	return false;
}

bool read_filter(const char* path, ntc_bloom_header& h, std::vector<unsigned char>* image, Kind kind = kPlain)
{
	const bool counting = kind == kCounting;
	const auto read = counting ? ntc_cbloom_read : kind == kBlocked ? ntc_bbloom_read : ntc_bloom_read;
	if (read(path, &h, nullptr, 0) != 0) {
		(void)fail_lib();
		return false;
	}
	if (!image) return true;
	image->resize(image_bytes(h, counting));
	if (read(path, &h, image->data(), image->size()) != 0) {
		(void)fail_lib();
		return false;
	}
	return true;
}

// build (a plain filter, OUT.bf) and count (a counting filter, OUT.cbf): the same arguments, -m in bits or in counters
int build(int argc, char** argv, bool counting)
{
	const char* const cmd = counting ? "count" : "build";
	auto needs = [&](const char* what) { return usage((std::string(cmd) + " needs " + what).c_str()); };
	uint64_t k = 0, n_hash = 3, m_bits = 0, distinct = 0;
	double fpr = 0.0;
	bool have_k = false, have_m = false, have_distinct = false, have_fpr = false, blocked = false;
	uint32_t strand = 0;
	const char* out = nullptr;
	const char* hist = nullptr;
	std::vector<const char*> files;
	for (int i = 0; i < argc; ++i) {
		const std::string a = argv[i];
		auto value = [&](const char* flag) -> const char* {
			if (i + 1 >= argc) {
				(void)usage("missing value behind", flag);
				return nullptr;
			}
			return argv[++i];
		};
		if (a == "-k") {
			const char* v = value("-k");
			if (!v) return EXIT_FAILURE;
			if (!parse_u64(v, k) || k < 1 || k > ntc_max_k()) return usage("-k is not a number of 1 .. ntc_max_k()", v);
			have_k = true;
		} else if (a == "-H") {
			const char* v = value("-H");
			if (!v) return EXIT_FAILURE;
			if (!parse_u64(v, n_hash) || n_hash < 1 || n_hash > 32) return usage("-H is not a number of 1 .. 32", v);
		} else if (a == "-m") {
			const char* v = value("-m");
			if (!v) return EXIT_FAILURE;
			if (!parse_u64(v, m_bits) || m_bits < 1 || m_bits >= (1ull << 40)) return usage("-m is not a number of 1 .. 2^40 - 1", v);
			have_m = true;
		} else if (a == "--distinct") {
			const char* v = value("--distinct");
			if (!v) return EXIT_FAILURE;
			if (!parse_u64(v, distinct) || distinct == 0) return usage("--distinct is not a positive number", v);
			have_distinct = true;
		} else if (a == "--fpr") {
			const char* v = value("--fpr");
			if (!v) return EXIT_FAILURE;
			if (!parse_double(v, fpr) || !(fpr > 0.0 && fpr < 1.0)) return usage("--fpr is not a number inside (0, 1)", v);
			have_fpr = true;
		} else if (a == "--hist") {
			hist = value("--hist");
			if (!hist) return EXIT_FAILURE;
		} else if (a == "-o") {
			out = value("-o");
			if (!out) return EXIT_FAILURE;
		} else if (a == "--blocked") {
			blocked = true;
		} else if (a.compare(0, 9, "--strand=") == 0) {
			const std::string s = a.substr(9);
			if (s == "canonical") strand = 0;
			else if (s == "forward") strand = 1;
			else if (s == "reverse") strand = 2;
			else return usage("--strand is none of canonical, forward, reverse", s.c_str());
		} else if (a.size() > 1 && a[0] == '-') {
			return usage("unknown option", a.c_str());
		} else {
			files.push_back(argv[i]);
		}
	}
	if (blocked && counting) return usage("--blocked goes with build and solid: there is no blocked counting filter");
	if (!have_k) return needs("-k");
	if (!out) return needs(counting ? "-o OUT.cbf" : "-o OUT.bf");
	const int ways = (have_m ? 1 : 0) + (have_distinct ? 1 : 0) + (hist ? 1 : 0);
	if (ways != 1) return needs(counting ? "exactly one of -m COUNTERS, --distinct N and --hist FILE" : "exactly one of -m BITS, --distinct N and --hist FILE");
	if (have_m && have_fpr) return usage("--fpr goes with --distinct or --hist, not with -m");
	if (!have_m && !have_fpr) return usage("--distinct and --hist need --fpr P");
	if (files.empty()) return needs("at least one input file");
	if (hist && !hist_f0(hist, distinct)) return usage("no F0 line of a .hist file in", hist);
	if (hist && distinct == 0) return usage("the F0 of the .hist file is 0", hist);
	if (blocked && have_m && m_bits % NTC_BBLOOM_BLOCK_BITS != 0) return usage("-m of a blocked filter is not a multiple of 512", std::to_string(m_bits).c_str());
	if (!have_m && (blocked ? ntc_bbloom_size : ntc_bloom_size)(distinct, (uint32_t)n_hash, fpr, &m_bits) != 0) return fail_lib();

	BuildCtx c;
	c.h = ntc_bloom_header{(uint32_t)k, (uint32_t)n_hash, strand, blocked ? NTC_BBLOOM_BLOCK_BITS : 0u, m_bits, 0};
	c.counting = counting;
	c.blocked = blocked;
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) {
		std::fprintf(stderr, "ntbloom: no HIP device\n");
		return EXIT_FAILURE;
	}
	Buffers b;
	if (!upload_filter(b, c.h, nullptr, counting) || !alloc_batch(b)) return EXIT_FAILURE;
	Reader r(b, (uint32_t)k, false, build_flush, &c);
	for (const char* f : files)
		if (int rc = r.read_file(f)) return rc;
	if (int rc = r.flush()) return rc;
	std::vector<unsigned char> image(image_bytes(c.h, counting));
	const hipError_t rc = hipMemcpy(image.data(), b.d_filter, image.size(), hipMemcpyDeviceToHost);
	if (rc != hipSuccess) return fail_hip("cannot fetch the filter", rc);
	if ((counting ? ntc_cbloom_write : blocked ? ntc_bbloom_write : ntc_bloom_write)(out, &c.h, image.data()) != 0) return fail_lib();
	std::fprintf(stderr, "ntbloom: %llu k-mers into %llu %s, %u hashes each\n", (unsigned long long)c.h.n_inserted, (unsigned long long)m_bits,
	             counting ? "counters" : blocked ? "bits in blocks of 512" : "bits", (uint32_t)n_hash);
	return EXIT_SUCCESS;
}

int solid(int argc, char** argv)
{
	uint64_t min_count = 0, n_hash = 3;
	double fpr = 0.0;
	bool have_c = false, have_fpr = false, have_h = false, blocked = false;
	const char* out = nullptr;
	const char* hist = nullptr;
	std::vector<const char*> files; // IN.cbf, then the input files
	for (int i = 0; i < argc; ++i) {
		const std::string a = argv[i];
		auto value = [&](const char* flag) -> const char* {
			if (i + 1 >= argc) {
				(void)usage("missing value behind", flag);
				return nullptr;
			}
			return argv[++i];
		};
		if (a == "--min-count") {
			const char* v = value("--min-count");
			if (!v) return EXIT_FAILURE;
			if (!parse_u64(v, min_count) || min_count < 1 || min_count > 255) return usage("--min-count is not a number of 1 .. 255", v);
			have_c = true;
		} else if (a == "-H") {
			const char* v = value("-H");
			if (!v) return EXIT_FAILURE;
			if (!parse_u64(v, n_hash) || n_hash < 1 || n_hash > 32) return usage("-H is not a number of 1 .. 32", v);
			have_h = true;
		} else if (a == "--fpr") {
			const char* v = value("--fpr");
			if (!v) return EXIT_FAILURE;
			if (!parse_double(v, fpr) || !(fpr > 0.0 && fpr < 1.0)) return usage("--fpr is not a number inside (0, 1)", v);
			have_fpr = true;
		} else if (a == "--hist") {
			hist = value("--hist");
			if (!hist) return EXIT_FAILURE;
		} else if (a == "-o") {
			out = value("-o");
			if (!out) return EXIT_FAILURE;
		} else if (a == "--blocked") {
			blocked = true;
		} else if (a.size() > 1 && a[0] == '-') {
			return usage("unknown option", a.c_str());
		} else {
			files.push_back(argv[i]);
		}
	}
	if (!have_c) return usage("solid needs --min-count C");
	if (!out) return usage("solid needs -o OUT.bf");
	if (files.empty()) return usage("solid needs IN.cbf");
	const bool walk = files.size() > 1;
	if (!walk && blocked) return usage("--blocked goes with input files: a threshold of IN.cbf has the counting filter's positions, which are not blocked");
	if (!walk && (hist || have_fpr || have_h)) return usage("--hist, --fpr and -H go with input files: without them IN.cbf is thresholded");
	if (walk && (!hist || !have_fpr)) return usage("solid with input files needs --hist FILE and --fpr P");
	BuildCtx c;
	std::vector<unsigned char> counters;
	if (!read_filter(files[0], c.c, nullptr, kCounting)) return EXIT_FAILURE; // (the header first: the refusals below need no counter)
	uint64_t m_bits = c.c.m_bits;
	if (walk) {
		uint64_t n = 0;
		const int rc = hist_solid_n(hist, min_count, n);
		if (rc == -1) return usage("no F0 line of a .hist file in", hist);
		if (rc == -2) return usage("the f_i lines of the .hist file stop below --min-count - 1", hist);
		if (rc == -3) return usage("the f_i lines of the .hist file sum to more than its F0", hist);
		if (n == 0) return usage("F0 minus the f_i below --min-count is 0 in", hist);
		if ((blocked ? ntc_bbloom_size : ntc_bloom_size)(n, (uint32_t)n_hash, fpr, &m_bits) != 0) return fail_lib();
	} else {
		n_hash = c.c.n_hash;
	}
	if (!read_filter(files[0], c.c, &counters, kCounting)) return EXIT_FAILURE;
	c.h = ntc_bloom_header{c.c.k, (uint32_t)n_hash, c.c.strand, blocked ? NTC_BBLOOM_BLOCK_BITS : 0u, m_bits, walk ? 0 : c.c.n_inserted};
	c.min_count = (uint32_t)min_count;
	c.blocked = blocked;
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) {
		std::fprintf(stderr, "ntbloom: no HIP device\n");
		return EXIT_FAILURE;
	}
	Buffers b;
	if (!upload_filter(b, c.c, &counters, true, &b.d_counters) || !upload_filter(b, c.h, nullptr)) return EXIT_FAILURE;
	if (walk) {
		if (!alloc_batch(b)) return EXIT_FAILURE;
		Reader r(b, c.h.k, false, build_flush, &c);
		for (size_t i = 1; i < files.size(); ++i)
			if (int rc = r.read_file(files[i])) return rc;
		if (int rc = r.flush()) return rc;
	} else if (ntc_cbloom_threshold_device(0, nullptr, b.d_counters, c.c.m_bits, c.min_count, b.d_filter) != 0) {
		return fail_lib();
	}
	std::vector<unsigned char> image(image_bytes(c.h, false));
	const hipError_t rc = hipMemcpy(image.data(), b.d_filter, image.size(), hipMemcpyDeviceToHost);
	if (rc != hipSuccess) return fail_hip("cannot fetch the filter", rc);
	if ((blocked ? ntc_bbloom_write : ntc_bloom_write)(out, &c.h, image.data()) != 0) return fail_lib();
	if (walk)
		std::fprintf(stderr, "ntbloom: %llu k-mers counted at least %u times into %llu %s, %u hashes each\n", (unsigned long long)c.h.n_inserted, c.min_count,
		             (unsigned long long)m_bits, blocked ? "bits in blocks of 512" : "bits", (uint32_t)n_hash);
	else
		std::fprintf(stderr, "ntbloom: the counters of at least %u into %llu bits\n", c.min_count, (unsigned long long)m_bits);
	return EXIT_SUCCESS;
}

int query(int argc, char** argv)
{
	QueryCtx c;
	bool have_c = false;
	if (argc >= 1 && std::strcmp(argv[0], "--min-count") == 0) {
		if (argc < 2) return usage("missing value behind", "--min-count");
		uint64_t v = 0;
		if (!parse_u64(argv[1], v) || v < 1 || v > 255) return usage("--min-count is not a number of 1 .. 255", argv[1]);
		c.min_count = (uint32_t)v;
		have_c = true;
		argc -= 2, argv += 2;
	}
	if (argc < 2) return usage("query needs F.bf and at least one input file");
	for (int i = 0; i < argc; ++i)
		if (argv[i][0] == '-' && argv[i][1] != '\0') return usage("unknown option", argv[i]);
	const Kind kind = file_kind(argv[0]);
	c.counting = kind == kCounting;
	c.blocked = kind == kBlocked;
	std::vector<unsigned char> image;
	if (!read_filter(argv[0], c.h, nullptr, kind)) return EXIT_FAILURE;
	if (have_c && !c.counting) return usage("--min-count goes with a counting filter (.cbf), not with", argv[0]);
	if (!read_filter(argv[0], c.h, &image, kind)) return EXIT_FAILURE;
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) {
		std::fprintf(stderr, "ntbloom: no HIP device\n");
		return EXIT_FAILURE;
	}
	Buffers b;
	if (!upload_filter(b, c.h, &image, c.counting) || !alloc_batch(b)) return EXIT_FAILURE;
	Reader r(b, c.h.k, true, query_flush, &c);
	std::printf("name\tlength\twindows\thits\tfraction\n");
	for (int i = 1; i < argc; ++i)
		if (int rc = r.read_file(argv[i])) return rc;
	return r.flush();
}

int info(int argc, char** argv)
{
	if (argc != 1) return usage("info takes one file");
	if (argv[0][0] == '-' && argv[0][1] != '\0') return usage("unknown option", argv[0]);
	ntc_bloom_header h;
	int n_dev = 0;
	const bool gpu = hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0;
	std::vector<unsigned char> image;
	const Kind kind = file_kind(argv[0]);
	const bool counting = kind == kCounting;
	if (!read_filter(argv[0], h, gpu ? &image : nullptr, kind)) return EXIT_FAILURE;
	std::printf("file\t%s\nk\t%u\nhashes\t%u\nstrand\t%s\n%s\t%llu\ninserted\t%llu\n", argv[0], h.k, h.n_hash, kStrand[h.strand], counting ? "counters" : "bits",
	            (unsigned long long)h.m_bits, (unsigned long long)h.n_inserted);
	if (kind == kBlocked) std::printf("block\t%u\nblocks\t%llu\n", h.reserved, (unsigned long long)(h.m_bits / h.reserved));
	if (!gpu) return EXIT_SUCCESS;
	Buffers b;
	if (!upload_filter(b, h, &image, counting)) return EXIT_FAILURE;
	if (counting) {
		uint64_t hist[256];
		if (ntc_cbloom_hist_device(0, nullptr, b.d_filter, h.m_bits, hist) != 0) return fail_lib();
		const uint64_t used = h.m_bits - hist[0];
		const double occ = (double)used / (double)h.m_bits;
		std::printf("nonzero\t%llu\nsaturated\t%llu\noccupancy\t%.6f\nfpr\t%.6g\n", (unsigned long long)used, (unsigned long long)hist[255], occ, std::pow(occ, (double)h.n_hash));
		return EXIT_SUCCESS;
	}
	uint64_t pop = 0;
	if (ntc_bloom_popcount_device(0, nullptr, b.d_filter, h.m_bits, &pop) != 0) return fail_lib();
	const double occ = (double)pop / (double)h.m_bits;
	double fpr = std::pow(occ, (double)h.n_hash);
	if (kind == kBlocked) { // per block: a block fuller than the average answers wrongly more often than the average says
		uint64_t hist[NTC_BBLOOM_BLOCK_BITS + 1];
		if (ntc_bbloom_hist_device(0, nullptr, b.d_filter, h.m_bits, hist) != 0) return fail_lib();
		fpr = 0.0;
		for (uint32_t v = 0; v <= NTC_BBLOOM_BLOCK_BITS; ++v)
			fpr += (double)hist[v] * std::pow((double)v / (double)NTC_BBLOOM_BLOCK_BITS, (double)h.n_hash);
		fpr /= (double)(h.m_bits / NTC_BBLOOM_BLOCK_BITS);
	}
	std::printf("popcount\t%llu\noccupancy\t%.6f\nfpr\t%.6g\n", (unsigned long long)pop, occ, fpr);
	return EXIT_SUCCESS;
}

} // namespace

int main(int argc, char** argv)
{
	if (argc < 2) return usage("no command");
	const std::string cmd = argv[1];
	if (cmd == "build") return build(argc - 2, argv + 2, false);
	if (cmd == "count") return build(argc - 2, argv + 2, true);
	if (cmd == "solid") return solid(argc - 2, argv + 2);
	if (cmd == "query") return query(argc - 2, argv + 2);
	if (cmd == "info") return info(argc - 2, argv + 2);
	return usage("unknown command", argv[1]);
}
