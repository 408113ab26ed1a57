// ntbloom_cli.cpp — `ntbloom`: Bloom filters of every k-mer of the input, in the reference's layout (vendor/ntHash/lib/BloomFilter.hpp), sized from ntcard's F0
// (include/ntcard_hip.h: ntc_bloom_*; DESIGN.md §4 "Bloom filters").
//   ntbloom build -k K [-H N] [--strand=canonical|forward|reverse] (-m BITS | --distinct N --fpr P | --hist FILE --fpr P) -o OUT.bf FILE...
//                               inserts every k-mer of the files.  The filter has BITS bits, or what ntc_bloom_size gives for N distinct k-mers at false
//                               positive rate P; --hist takes N from the F0 line of a `.hist` file as ntcard writes it, so that
//                               `ntcard -k 32 -p s reads.fq && ntbloom build -k 32 --hist s_k32.hist --fpr 0.01 -o s.bf reads.fq` composes.  -H: hashes per
//                               k-mer (default 3).  OUT.bf is written whole or not at all (ntc_bloom_write).
//   ntbloom query F.bf FILE...  one TSV row per record: name, length, windows, hits, hits / windows (k, hashes and strand come from F.bf)
//   ntbloom info F.bf           the header, and with a GPU the popcount, the occupancy and the false positive rate it implies; without one the header alone
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
	             "usage: ntbloom build -k K [-H N] [--strand=canonical|forward|reverse] (-m BITS | --distinct N --fpr P | --hist FILE --fpr P) -o OUT.bf FILE...\n"
	             "       ntbloom query F.bf FILE...\n"
	             "       ntbloom info F.bf\n");
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

// device and pinned memory of one run, freed on every way out
struct Buffers {
	unsigned char* d_filter = nullptr;
	unsigned char* d_bases = nullptr;
	unsigned char* h_bases = nullptr; // pinned
	uint32_t* d_counts = nullptr;     // query: [2][seq_cap]
	size_t seq_cap = 0;
	~Buffers()
	{
		if (d_filter) (void)hipFree(d_filter);
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
};
int build_flush(Reader& r, void* ctx)
{
	BuildCtx& c = *static_cast<BuildCtx*>(ctx);
	const hipError_t rc = hipMemcpy(r.b.d_bases, r.b.h_bases, r.fill, hipMemcpyHostToDevice);
	if (rc != hipSuccess) return fail_hip("cannot upload a batch", rc);
	uint64_t n = 0;
	if (ntc_bloom_insert_device(0, nullptr, r.b.d_filter, c.h.m_bits, c.h.n_hash, c.h.k, c.h.strand, r.b.d_bases, r.offsets.data(), r.offsets.size() - 1, &n) != 0) return fail_lib();
	c.h.n_inserted += n;
	return EXIT_SUCCESS;
}

struct QueryCtx {
	ntc_bloom_header h;
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
	if (ntc_bloom_query_device(0, nullptr, r.b.d_filter, c.h.m_bits, c.h.n_hash, c.h.k, c.h.strand, r.b.d_bases, r.offsets.data(), n_seqs, d_w, d_h) != 0) return fail_lib();
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

bool upload_filter(Buffers& b, const ntc_bloom_header& h, const std::vector<unsigned char>* image)
{
	const size_t padded = (((h.m_bits + 7) / 8) + 3) & ~(size_t)3;
	hipError_t rc = hipMalloc((void**)&b.d_filter, padded);
	if (rc == hipSuccess) rc = hipMemset(b.d_filter, 0, padded);
	if (rc == hipSuccess && image) rc = hipMemcpy(b.d_filter, image->data(), image->size(), hipMemcpyHostToDevice);
	if (rc == hipSuccess) return true;
	(void)fail_hip("cannot bring the filter to the device", rc);
	return false;
}

bool read_filter(const char* path, ntc_bloom_header& h, std::vector<unsigned char>* image)
{
	if (ntc_bloom_read(path, &h, nullptr, 0) != 0) {
		(void)fail_lib();
		return false;
	}
	if (!image) return true;
	image->resize((h.m_bits + 7) / 8);
	if (ntc_bloom_read(path, &h, image->data(), image->size()) != 0) {
		(void)fail_lib();
		return false;
	}
	return true;
}

int build(int argc, char** argv)
{
	uint64_t k = 0, n_hash = 3, m_bits = 0, distinct = 0;
	double fpr = 0.0;
	bool have_k = false, have_m = false, have_distinct = false, have_fpr = false;
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
	if (!have_k) return usage("build needs -k");
	if (!out) return usage("build needs -o OUT.bf");
	const int ways = (have_m ? 1 : 0) + (have_distinct ? 1 : 0) + (hist ? 1 : 0);
	if (ways != 1) return usage("build needs exactly one of -m BITS, --distinct N and --hist FILE");
	if (have_m && have_fpr) return usage("--fpr goes with --distinct or --hist, not with -m");
	if (!have_m && !have_fpr) return usage("--distinct and --hist need --fpr P");
	if (files.empty()) return usage("build needs at least one input file");
	if (hist && !hist_f0(hist, distinct)) return usage("no F0 line of a .hist file in", hist);
	if (hist && distinct == 0) return usage("the F0 of the .hist file is 0", hist);
	if (!have_m && ntc_bloom_size(distinct, (uint32_t)n_hash, fpr, &m_bits) != 0) return fail_lib();

	BuildCtx c;
	c.h = ntc_bloom_header{(uint32_t)k, (uint32_t)n_hash, strand, 0, m_bits, 0};
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) {
		std::fprintf(stderr, "ntbloom: no HIP device\n");
		return EXIT_FAILURE;
	}
	Buffers b;
	if (!upload_filter(b, c.h, nullptr) || !alloc_batch(b)) return EXIT_FAILURE;
	Reader r(b, (uint32_t)k, false, build_flush, &c);
	for (const char* f : files)
		if (int rc = r.read_file(f)) return rc;
	if (int rc = r.flush()) return rc;
	std::vector<unsigned char> image((m_bits + 7) / 8);
	const hipError_t rc = hipMemcpy(image.data(), b.d_filter, image.size(), hipMemcpyDeviceToHost);
	if (rc != hipSuccess) return fail_hip("cannot fetch the filter", rc);
	if (ntc_bloom_write(out, &c.h, image.data()) != 0) return fail_lib();
	std::fprintf(stderr, "ntbloom: %llu k-mers into %llu bits, %u hashes each\n", (unsigned long long)c.h.n_inserted, (unsigned long long)m_bits, (uint32_t)n_hash);
	return EXIT_SUCCESS;
}

int query(int argc, char** argv)
{
	if (argc < 2) return usage("query needs F.bf and at least one input file");
	for (int i = 0; i < argc; ++i)
		if (argv[i][0] == '-' && argv[i][1] != '\0') return usage("unknown option", argv[i]);
	QueryCtx c;
	std::vector<unsigned char> image;
	if (!read_filter(argv[0], c.h, &image)) return EXIT_FAILURE;
	int n_dev = 0;
	if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) {
		std::fprintf(stderr, "ntbloom: no HIP device\n");
		return EXIT_FAILURE;
	}
	Buffers b;
	if (!upload_filter(b, c.h, &image) || !alloc_batch(b)) return EXIT_FAILURE;
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
	if (!read_filter(argv[0], h, gpu ? &image : nullptr)) return EXIT_FAILURE;
	std::printf("file\t%s\nk\t%u\nhashes\t%u\nstrand\t%s\nbits\t%llu\ninserted\t%llu\n", argv[0], h.k, h.n_hash, kStrand[h.strand], (unsigned long long)h.m_bits,
	            (unsigned long long)h.n_inserted);
	if (!gpu) return EXIT_SUCCESS;
	Buffers b;
	if (!upload_filter(b, h, &image)) return EXIT_FAILURE;
	uint64_t pop = 0;
	if (ntc_bloom_popcount_device(0, nullptr, b.d_filter, h.m_bits, &pop) != 0) return fail_lib();
	const double occ = (double)pop / (double)h.m_bits;
	std::printf("popcount\t%llu\noccupancy\t%.6f\nfpr\t%.6g\n", (unsigned long long)pop, occ, std::pow(occ, (double)h.n_hash));
	return EXIT_SUCCESS;
}

} // namespace

int main(int argc, char** argv)
{
	if (argc < 2) return usage("no command");
	const std::string cmd = argv[1];
	if (cmd == "build") return build(argc - 2, argv + 2);
	if (cmd == "query") return query(argc - 2, argv + 2);
	if (cmd == "info") return info(argc - 2, argv + 2);
	return usage("unknown command", argv[1]);
}
