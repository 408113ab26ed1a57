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

// A `.hist` file as ntc_write_hist writes it, read in one pass: the value of its first "F0\t<integer>" line, and its "i\tf_i" lines, i = 1, 2, ... as far
// as they follow each other (whatever is no "i\tf_i" line of the next i is passed over: the F1 and F0 lines, say; an f_i that is no number ends the list)
struct Hist {
	bool have_f0 = false;
	uint64_t f0 = 0;
	std::vector<uint64_t> f; // f[i - 1] = f_i
};
Hist read_hist(const char* path)
{
	Hist h;
	FILE* f = std::fopen(path, "rb");
	if (!f) return h;
	char line[256];
	bool f0_line = false, list_ended = false;
	while (std::fgets(line, sizeof line, f)) {
		char* tab = std::strchr(line, '\t');
		if (!tab) continue;
		std::string v(tab + 1);
		while (!v.empty() && (v.back() == '\n' || v.back() == '\r'))
			v.pop_back();
		*tab = '\0';
		uint64_t i = 0, fi = 0;
		if (std::strcmp(line, "F0") == 0) {
			if (!f0_line) h.have_f0 = parse_u64(v.c_str(), h.f0);
			f0_line = true;
		} else if (!list_ended && parse_u64(line, i) && i == h.f.size() + 1) {
			if (parse_u64(v.c_str(), fi))
				h.f.push_back(fi);
			else
				list_ended = true;
		}
	}
	std::fclose(f);
	return h;
}

// A KIND of filter — plain, counting, blocked — is one row of this table: its file, its size, what its m counts and its entry points.  A command picks
// the row once, from `count` / --blocked or from a file's magic, and carries it; nothing below asks which kind it has.
struct Kind {
	const char* magic; // of its file; nullptr: the plain kind, which is also any file of no known magic (ntc_bloom_read then says what is wrong with it)
	int (*read)(const char*, ntc_bloom_header*, void*, uint64_t);
	int (*write)(const char*, const ntc_bloom_header*, const void*);
	int (*size)(uint64_t, uint32_t, double, uint64_t*);
	size_t (*image_bytes)(uint64_t m); // the bytes of its image
	uint32_t reserved;                 // of its header: the block size of a kind in blocks, else 0
	const char* what;                  // what m counts, in the reports ...
	const char* info_m;                // ... in `info` ...
	const char* need_out;              // ... and in the refusals of build and count
	const char* need_size;
	int (*insert)(int32_t, void*, void*, uint64_t, uint32_t, uint32_t, uint32_t, const void*, const uint64_t*, uint64_t, uint64_t*);
	// solid: the windows counted at least min_count times in a counting filter go into a filter of this kind (nullptr: no such destination)
	int (*insert_solid)(int32_t, void*, void*, uint64_t, uint32_t, const void*, uint64_t, uint32_t, uint32_t, uint32_t, uint32_t, const void*, const uint64_t*, uint64_t, uint64_t*);
	// the kind's query call; min_count is the counting kind's
	int (*query)(const ntc_bloom_header& h, const void* d_filter, const void* d_bases, const uint64_t* offsets, uint64_t n_seqs, uint32_t min_count, void* d_w, void* d_h);
	// info, with a device: the lines behind the header
	int (*report)(const ntc_bloom_header& h, const void* d_filter);
};

int report_bits(const ntc_bloom_header& h, const void* d_filter, const double* fpr_given)
{
	uint64_t pop = 0;
	if (ntc_bloom_popcount_device(0, nullptr, d_filter, h.m_bits, &pop) != 0) return fail_lib();
	const double occ = (double)pop / (double)h.m_bits;
	std::printf("popcount\t%llu\noccupancy\t%.6f\nfpr\t%.6g\n", (unsigned long long)pop, occ, fpr_given ? *fpr_given : std::pow(occ, (double)h.n_hash));
	return EXIT_SUCCESS;
}
int report_plain(const ntc_bloom_header& h, const void* d_filter) { return report_bits(h, d_filter, nullptr); }
int report_blocked(const ntc_bloom_header& h, const void* d_filter)
{
	uint64_t hist[NTC_BBLOOM_BLOCK_BITS + 1]; // per block: a block fuller than the average answers wrongly more often than the average says
	if (ntc_bbloom_hist_device(0, nullptr, d_filter, h.m_bits, hist) != 0) return fail_lib();
	double fpr = 0.0;
	for (uint32_t v = 0; v <= NTC_BBLOOM_BLOCK_BITS; ++v)
		fpr += (double)hist[v] * std::pow((double)v / (double)NTC_BBLOOM_BLOCK_BITS, (double)h.n_hash);
	fpr /= (double)(h.m_bits / NTC_BBLOOM_BLOCK_BITS);
	return report_bits(h, d_filter, &fpr);
}
int report_counting(const ntc_bloom_header& h, const void* d_filter)
{
	uint64_t hist[256];
	if (ntc_cbloom_hist_device(0, nullptr, d_filter, h.m_bits, hist) != 0) return fail_lib();
	const uint64_t used = h.m_bits - hist[0];
	const double occ = (double)used / (double)h.m_bits;
	std::printf("nonzero\t%llu\nsaturated\t%llu\noccupancy\t%.6f\nfpr\t%.6g\n", (unsigned long long)used, (unsigned long long)hist[255], occ, std::pow(occ, (double)h.n_hash));
	return EXIT_SUCCESS;
}

size_t bytes_of_bits(uint64_t m) { return (m + 7) / 8; }
size_t bytes_of_counters(uint64_t m) { return m; }

const Kind kPlain = {nullptr, ntc_bloom_read, ntc_bloom_write, ntc_bloom_size, bytes_of_bits, 0, "bits", "bits", "-o OUT.bf", "exactly one of -m BITS, --distinct N and --hist FILE",
                     ntc_bloom_insert_device, ntc_bloom_insert_solid_device,
                     [](const ntc_bloom_header& h, const void* f, const void* bases, const uint64_t* off, uint64_t n, uint32_t, void* w, void* hits) {
	                     return ntc_bloom_query_device(0, nullptr, f, h.m_bits, h.n_hash, h.k, h.strand, bases, off, n, w, hits);
                     },
                     report_plain};
const Kind kCounting = {"NTCCB1\0\0", ntc_cbloom_read, ntc_cbloom_write, ntc_bloom_size, bytes_of_counters, 0, "counters", "counters", "-o OUT.cbf",
                        "exactly one of -m COUNTERS, --distinct N and --hist FILE", ntc_cbloom_insert_device, nullptr,
                        [](const ntc_bloom_header& h, const void* f, const void* bases, const uint64_t* off, uint64_t n, uint32_t min_count, void* w, void* hits) {
	                        return ntc_cbloom_query_device(0, nullptr, f, h.m_bits, h.n_hash, h.k, h.strand, bases, off, n, min_count, w, hits);
                        },
                        report_counting};
const Kind kBlocked = {"NTCBB1\0\0", ntc_bbloom_read, ntc_bbloom_write, ntc_bbloom_size, bytes_of_bits, NTC_BBLOOM_BLOCK_BITS, "bits in blocks of 512", "bits", "-o OUT.bf",
                       "exactly one of -m BITS, --distinct N and --hist FILE", ntc_bbloom_insert_device, ntc_bbloom_insert_solid_device,
                       [](const ntc_bloom_header& h, const void* f, const void* bases, const uint64_t* off, uint64_t n, uint32_t, void* w, void* hits) {
	                       return ntc_bbloom_query_device(0, nullptr, f, h.m_bits, h.n_hash, h.k, h.strand, bases, off, n, w, hits);
                       },
                       report_blocked};

// the kind of a filter file by its magic
const Kind& file_kind(const char* path)
{
	char magic[8] = {0};
	FILE* f = std::fopen(path, "rb");
	const bool whole = f && std::fread(magic, 1, 8, f) == 8;
	if (f) std::fclose(f);
	for (const Kind* kind : {&kCounting, &kBlocked})
		if (whole && std::memcmp(magic, kind->magic, 8) == 0) return *kind;
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
	const Kind* kind;       // of the filter in d_filter
	ntc_bloom_header h;
	ntc_bloom_header c{};   // solid: the counting filter in d_counters ...
	uint32_t min_count = 0; // ... and the count a k-mer needs (0: not solid)
};
int build_flush(Reader& r, void* ctx)
{
	BuildCtx& c = *static_cast<BuildCtx*>(ctx);
	const hipError_t rc = hipMemcpy(r.b.d_bases, r.b.h_bases, r.fill, hipMemcpyHostToDevice);
	if (rc != hipSuccess) return fail_hip("cannot upload a batch", rc);
	uint64_t n = 0;
	const uint64_t n_seqs = r.offsets.size() - 1;
	const int rc2 = c.min_count ? c.kind->insert_solid(0, nullptr, r.b.d_filter, c.h.m_bits, c.h.n_hash, r.b.d_counters, c.c.m_bits, c.c.n_hash, c.min_count, c.h.k, c.h.strand,
	                                                   r.b.d_bases, r.offsets.data(), n_seqs, &n)
	                            : c.kind->insert(0, nullptr, r.b.d_filter, c.h.m_bits, c.h.n_hash, c.h.k, c.h.strand, r.b.d_bases, r.offsets.data(), n_seqs, &n);
	if (rc2 != 0) return fail_lib();
	c.h.n_inserted += n;
	return EXIT_SUCCESS;
}

struct QueryCtx {
	const Kind* kind;
	ntc_bloom_header h;
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
	if (c.kind->query(c.h, r.b.d_filter, r.b.d_bases, r.offsets.data(), n_seqs, c.min_count, d_w, d_h) != 0) return fail_lib();
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

// a filter of the kind on the device at `d`: zeros, or the image
bool upload_filter(unsigned char*& d, const Kind& kind, const ntc_bloom_header& h, const std::vector<unsigned char>* image)
{
	const size_t padded = (kind.image_bytes(h.m_bits) + 3) & ~(size_t)3;
	hipError_t rc = hipMalloc((void**)&d, padded);
	if (rc == hipSuccess) rc = hipMemset(d, 0, padded);
	if (rc == hipSuccess && image) rc = hipMemcpy(d, image->data(), image->size(), hipMemcpyHostToDevice);
	if (rc == hipSuccess) return true;
	(void)fail_hip("cannot bring the filter to the device", rc);
	return false;
}

// a file of the kind: its header, and its image where one is asked for
bool read_filter(const char* path, const Kind& kind, ntc_bloom_header& h, std::vector<unsigned char>* image)
{
	if (kind.read(path, &h, nullptr, 0) != 0) {
		(void)fail_lib();
		return false;
	}
	if (!image) return true;
	image->resize(kind.image_bytes(h.m_bits));
	if (kind.read(path, &h, image->data(), image->size()) != 0) {
		(void)fail_lib();
		return false;
	}
	return true;
}

// the end of build, count and solid: the image comes back and goes to OUT, whole or not at all
int write_filter(const Buffers& b, const Kind& kind, const ntc_bloom_header& h, const char* out)
{
	std::vector<unsigned char> image(kind.image_bytes(h.m_bits));
	const hipError_t rc = hipMemcpy(image.data(), b.d_filter, image.size(), hipMemcpyDeviceToHost);
	if (rc != hipSuccess) return fail_hip("cannot fetch the filter", rc);
	return kind.write(out, &h, image.data()) != 0 ? fail_lib() : EXIT_SUCCESS;
}

bool have_device()
{
	int n_dev = 0;
	return hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0;
}
int need_device()
{
	if (have_device()) return EXIT_SUCCESS;
	std::fprintf(stderr, "ntbloom: no HIP device\n");
	return EXIT_FAILURE;
}

// The options build, count and solid share, scanned in the order given; a command states which of them it `takes`, every other one is unknown to it.
// What is no option is a file.
enum : unsigned { kOptK = 1, kOptH = 2, kOptM = 4, kOptDistinct = 8, kOptFpr = 16, kOptHist = 32, kOptOut = 64, kOptBlocked = 128, kOptStrand = 256, kOptMinCount = 512 };
struct Options {
	uint64_t k = 0, n_hash = 3, m_bits = 0, distinct = 0, min_count = 0;
	double fpr = 0.0;
	uint32_t strand = 0;
	unsigned given = 0; // the options seen, as kOpt bits
	const char* out = nullptr;
	const char* hist = nullptr;
	std::vector<const char*> files;
	bool has(unsigned opt) const { return (given & opt) != 0; }
};
int scan_options(int argc, char** argv, unsigned takes, Options& o)
{
	const struct {
		const char* flag;
		unsigned opt;
		uint64_t Options::*to;
		uint64_t lo, hi;
		const char* why;
	} numbers[] = {{"-k", kOptK, &Options::k, 1, ntc_max_k(), "-k is not a number of 1 .. ntc_max_k()"},
	               {"-H", kOptH, &Options::n_hash, 1, 32, "-H is not a number of 1 .. 32"},
	               {"-m", kOptM, &Options::m_bits, 1, (1ull << 40) - 1, "-m is not a number of 1 .. 2^40 - 1"},
	               {"--distinct", kOptDistinct, &Options::distinct, 1, UINT64_MAX, "--distinct is not a positive number"},
	               {"--min-count", kOptMinCount, &Options::min_count, 1, 255, "--min-count is not a number of 1 .. 255"}};
	const struct {
		const char* flag;
		unsigned opt;
		const char* Options::*to;
	} names[] = {{"--hist", kOptHist, &Options::hist}, {"-o", kOptOut, &Options::out}};
	for (int i = 0; i < argc; ++i) {
		const std::string a = argv[i];
		unsigned opt = 0; // the option `a` is, if the command takes it
		const char* v = nullptr;
		auto value = [&](const char* flag, unsigned is) {
			if (a != flag || !(takes & is)) return false;
			opt = is;
			if (i + 1 >= argc)
				(void)usage("missing value behind", flag);
			else
				v = argv[++i];
			return true;
		};
		for (const auto& n : numbers)
			if (value(n.flag, n.opt)) {
				if (!v) return EXIT_FAILURE;
				if (!parse_u64(v, o.*n.to) || o.*n.to < n.lo || o.*n.to > n.hi) return usage(n.why, v);
			}
		for (const auto& n : names)
			if (value(n.flag, n.opt)) {
				if (!v) return EXIT_FAILURE;
				o.*n.to = v;
			}
		if (value("--fpr", kOptFpr)) {
			if (!v) return EXIT_FAILURE;
			if (!parse_double(v, o.fpr) || !(o.fpr > 0.0 && o.fpr < 1.0)) return usage("--fpr is not a number inside (0, 1)", v);
		} else if (a == "--blocked" && (takes & kOptBlocked)) {
			opt = kOptBlocked;
		} else if (a.compare(0, 9, "--strand=") == 0 && (takes & kOptStrand)) {
			opt = kOptStrand;
			const std::string s = a.substr(9);
			if (s == "canonical") o.strand = 0;
			else if (s == "forward") o.strand = 1;
			else if (s == "reverse") o.strand = 2;
			else return usage("--strand is none of canonical, forward, reverse", s.c_str());
		}
		if (opt)
			o.given |= opt;
		else if (a.size() > 1 && a[0] == '-')
			return usage("unknown option", a.c_str());
		else
			o.files.push_back(argv[i]);
	}
	return EXIT_SUCCESS;
}

// build (a plain or a blocked filter, OUT.bf) and count (a counting filter, OUT.cbf): the same arguments, -m in bits or in counters
int build(int argc, char** argv, bool counting)
{
	const char* const cmd = counting ? "count" : "build";
	auto needs = [&](const char* what) { return usage((std::string(cmd) + " needs " + what).c_str()); };
	Options o;
	if (int rc = scan_options(argc, argv, kOptK | kOptH | kOptM | kOptDistinct | kOptFpr | kOptHist | kOptOut | kOptBlocked | kOptStrand, o)) return rc;
	if (o.has(kOptBlocked) && counting) return usage("--blocked goes with build and solid: there is no blocked counting filter");
	const Kind& kind = counting ? kCounting : o.has(kOptBlocked) ? kBlocked : kPlain;
	if (!o.has(kOptK)) return needs("-k");
	if (!o.out) return needs(kind.need_out);
	const int ways = (o.has(kOptM) ? 1 : 0) + (o.has(kOptDistinct) ? 1 : 0) + (o.hist ? 1 : 0);
	if (ways != 1) return needs(kind.need_size);
	if (o.has(kOptM) && o.has(kOptFpr)) return usage("--fpr goes with --distinct or --hist, not with -m");
	if (!o.has(kOptM) && !o.has(kOptFpr)) return usage("--distinct and --hist need --fpr P");
	if (o.files.empty()) return needs("at least one input file");
	if (o.hist) {
		const Hist hist = read_hist(o.hist);
		if (!hist.have_f0) return usage("no F0 line of a .hist file in", o.hist);
		if (hist.f0 == 0) return usage("the F0 of the .hist file is 0", o.hist);
		o.distinct = hist.f0;
	}
	if (kind.reserved && o.has(kOptM) && o.m_bits % kind.reserved != 0) return usage("-m of a blocked filter is not a multiple of 512", std::to_string(o.m_bits).c_str());
	if (!o.has(kOptM) && kind.size(o.distinct, (uint32_t)o.n_hash, o.fpr, &o.m_bits) != 0) return fail_lib();

	BuildCtx c{&kind, ntc_bloom_header{(uint32_t)o.k, (uint32_t)o.n_hash, o.strand, kind.reserved, o.m_bits, 0}};
	if (int rc = need_device()) return rc;
	Buffers b;
	if (!upload_filter(b.d_filter, kind, c.h, nullptr) || !alloc_batch(b)) return EXIT_FAILURE;
	Reader r(b, (uint32_t)o.k, false, build_flush, &c);
	for (const char* f : o.files)
		if (int rc = r.read_file(f)) return rc;
	if (int rc = r.flush()) return rc;
	if (int rc = write_filter(b, kind, c.h, o.out)) return rc;
	std::fprintf(stderr, "ntbloom: %llu k-mers into %llu %s, %u hashes each\n", (unsigned long long)c.h.n_inserted, (unsigned long long)o.m_bits, kind.what, (uint32_t)o.n_hash);
	return EXIT_SUCCESS;
}

int solid(int argc, char** argv)
{
	Options o; // files: IN.cbf, then the input files
	if (int rc = scan_options(argc, argv, kOptMinCount | kOptH | kOptFpr | kOptHist | kOptOut | kOptBlocked, o)) return rc;
	if (!o.has(kOptMinCount)) return usage("solid needs --min-count C");
	if (!o.out) return usage("solid needs -o OUT.bf");
	if (o.files.empty()) return usage("solid needs IN.cbf");
	const bool walk = o.files.size() > 1;
	const Kind& kind = o.has(kOptBlocked) ? kBlocked : kPlain;
	if (!walk && o.has(kOptBlocked)) return usage("--blocked goes with input files: a threshold of IN.cbf has the counting filter's positions, which are not blocked");
	if (!walk && (o.hist || o.has(kOptFpr) || o.has(kOptH))) return usage("--hist, --fpr and -H go with input files: without them IN.cbf is thresholded");
	if (walk && (!o.hist || !o.has(kOptFpr))) return usage("solid with input files needs --hist FILE and --fpr P");
	BuildCtx c{&kind, ntc_bloom_header{}};
	std::vector<unsigned char> counters;
	if (!read_filter(o.files[0], kCounting, c.c, nullptr)) return EXIT_FAILURE; // (the header first: the refusals below need no counter)
	uint64_t m_bits = c.c.m_bits;
	if (walk) { // n = F0 - sum_{i < C} f_i of the `.hist` file
		const Hist hist = read_hist(o.hist);
		if (!hist.have_f0) return usage("no F0 line of a .hist file in", o.hist);
		if (hist.f.size() < o.min_count - 1) return usage("the f_i lines of the .hist file stop below --min-count - 1", o.hist);
		uint64_t n = hist.f0;
		for (uint64_t i = 1; i < o.min_count; ++i) {
			if (hist.f[i - 1] > n) return usage("the f_i lines of the .hist file sum to more than its F0", o.hist);
			n -= hist.f[i - 1];
		}
		if (n == 0) return usage("F0 minus the f_i below --min-count is 0 in", o.hist);
		if (kind.size(n, (uint32_t)o.n_hash, o.fpr, &m_bits) != 0) return fail_lib();
	} else {
		o.n_hash = c.c.n_hash;
	}
	if (!read_filter(o.files[0], kCounting, c.c, &counters)) return EXIT_FAILURE;
	c.h = ntc_bloom_header{c.c.k, (uint32_t)o.n_hash, c.c.strand, kind.reserved, m_bits, walk ? 0 : c.c.n_inserted};
	c.min_count = (uint32_t)o.min_count;
	if (int rc = need_device()) return rc;
	Buffers b;
	if (!upload_filter(b.d_counters, kCounting, c.c, &counters) || !upload_filter(b.d_filter, kind, c.h, nullptr)) return EXIT_FAILURE;
	if (walk) {
		if (!alloc_batch(b)) return EXIT_FAILURE;
		Reader r(b, c.h.k, false, build_flush, &c);
		for (size_t i = 1; i < o.files.size(); ++i)
			if (int rc = r.read_file(o.files[i])) return rc;
		if (int rc = r.flush()) return rc;
	} else if (ntc_cbloom_threshold_device(0, nullptr, b.d_counters, c.c.m_bits, c.min_count, b.d_filter) != 0) {
		return fail_lib();
	}
	if (int rc = write_filter(b, kind, c.h, o.out)) return rc;
	if (walk)
		std::fprintf(stderr, "ntbloom: %llu k-mers counted at least %u times into %llu %s, %u hashes each\n", (unsigned long long)c.h.n_inserted, c.min_count,
		             (unsigned long long)m_bits, kind.what, (uint32_t)o.n_hash);
	else
		std::fprintf(stderr, "ntbloom: the counters of at least %u into %llu bits\n", c.min_count, (unsigned long long)m_bits);
	return EXIT_SUCCESS;
}

int query(int argc, char** argv)
{
	uint64_t min_count = 1;
	bool have_c = false;
	if (argc >= 1 && std::strcmp(argv[0], "--min-count") == 0) {
		if (argc < 2) return usage("missing value behind", "--min-count");
		if (!parse_u64(argv[1], min_count) || min_count < 1 || min_count > 255) return usage("--min-count is not a number of 1 .. 255", argv[1]);
		have_c = true;
		argc -= 2, argv += 2;
	}
	if (argc < 2) return usage("query needs F.bf and at least one input file");
	for (int i = 0; i < argc; ++i)
		if (argv[i][0] == '-' && argv[i][1] != '\0') return usage("unknown option", argv[i]);
	QueryCtx c{&file_kind(argv[0]), ntc_bloom_header{}, (uint32_t)min_count, {}};
	std::vector<unsigned char> image;
	if (!read_filter(argv[0], *c.kind, c.h, nullptr)) return EXIT_FAILURE;
	if (have_c && c.kind != &kCounting) return usage("--min-count goes with a counting filter (.cbf), not with", argv[0]);
	if (!read_filter(argv[0], *c.kind, c.h, &image)) return EXIT_FAILURE;
	if (int rc = need_device()) return rc;
	Buffers b;
	if (!upload_filter(b.d_filter, *c.kind, c.h, &image) || !alloc_batch(b)) return EXIT_FAILURE;
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
	const bool gpu = have_device();
	std::vector<unsigned char> image;
	const Kind& kind = file_kind(argv[0]);
	if (!read_filter(argv[0], kind, h, gpu ? &image : nullptr)) return EXIT_FAILURE;
	std::printf("file\t%s\nk\t%u\nhashes\t%u\nstrand\t%s\n%s\t%llu\ninserted\t%llu\n", argv[0], h.k, h.n_hash, kStrand[h.strand], kind.info_m, (unsigned long long)h.m_bits,
	            (unsigned long long)h.n_inserted);
	if (kind.reserved) std::printf("block\t%u\nblocks\t%llu\n", h.reserved, (unsigned long long)(h.m_bits / h.reserved));
	if (!gpu) return EXIT_SUCCESS;
	Buffers b;
	if (!upload_filter(b.d_filter, kind, h, &image)) return EXIT_FAILURE;
	return kind.report(h, b.d_filter);
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
