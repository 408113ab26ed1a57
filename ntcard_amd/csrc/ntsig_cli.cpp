// ntsig_cli.cpp — `ntsig`: signature files (`ntcard --signature`, include/ntcard_hip.h: ntc_signature_write) from the command line.
//   ntsig info F.sig            the header: how the file was counted, and how many values it holds
//   ntsig compare A.sig B.sig   |A n B|, Jaccard and both containments — refused when the headers differ in anything but n
//   ntsig matrix [--containment] A.sig B.sig ...   all pairs at once, as a TSV: Jaccard, or the containment of the row's file in the column's
//   ntsig gather [--threshold N] QUERY.sig REF.sig ...   which references are in the query and what each explains on its own, as a TSV in pick order
//                               (ntc_signature_gather_device)
// info and compare are host code over the library's reader and ntc_signature_compare and need no GPU; matrix and gather read every header first (files counted
// differently are refused before a device is looked for: load_all), then upload the hash lists and call ntc_signature_matrix_device / _gather_device.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ntcard_hip.h"

namespace {

const char* const kStrand[3] = {"canonical", "forward", "reverse"};

struct Sig {
	ntc_sig_header h;
	std::vector<uint64_t> hashes;
	std::vector<uint32_t> counts;
};

bool load(const char* path, Sig& s, bool pairs)
{
	if (ntc_signature_read(path, &s.h, nullptr, nullptr, 0) != 0) {
		std::fprintf(stderr, "ntsig: %s\n", ntc_last_error());
		return false;
	}
	if (!pairs) return true;
	s.hashes.resize(s.h.n);
	s.counts.resize(s.h.n);
	uint64_t dummy_h = 0;
	uint32_t dummy_c = 0;
	if (ntc_signature_read(path, &s.h, s.h.n ? s.hashes.data() : &dummy_h, s.h.n ? s.counts.data() : &dummy_c, s.h.n) != 0) {
		std::fprintf(stderr, "ntsig: %s\n", ntc_last_error());
		return false;
	}
	return true;
}

void print_header(const char* path, const ntc_sig_header& h)
{
	std::printf("file\t%s\nk\t%u\nmask\t%s\ngap\t%u\nstrand\t%s\nhpc\t%u\nsBits\t%u\nn\t%llu\n", path, h.k, h.mask, h.gap, kStrand[h.strand], h.hpc, h.s_bits,
	            (unsigned long long)h.n);
}

// what two headers differ in beside n (nullptr: nothing — their values compare)
const char* differs_in(const ntc_sig_header& a, const ntc_sig_header& b)
{
	if (a.k != b.k) return "k";
	if (std::strcmp(a.mask, b.mask) != 0) return "mask";
	if (a.gap != b.gap) return "gap";
	if (a.strand != b.strand) return "strand";
	if (a.hpc != b.hpc) return "hpc";
	if (a.s_bits != b.s_bits) return "sBits";
	return nullptr;
}

int refuse(const char* a, const char* b, const char* differs)
{
	std::fprintf(stderr, "ntsig: %s and %s were counted differently (%s differs): their values cannot be compared\n", a, b, differs);
	return EXIT_FAILURE;
}

// device copies of the hash lists, freed on every way out
struct DeviceLists {
	std::vector<void*> p;
	~DeviceLists()
	{
		for (void* q : p)
			if (q) (void)hipFree(q);
	}
};

// hipMalloc + copy of n values of `bytes` bytes each from a file (n == 0: nothing, *out stays null)
bool to_device(void** out, const void* host, uint64_t n, size_t bytes, const char* file)
{
	if (n == 0) return true;
	hipError_t rc = hipMalloc(out, n * bytes);
	if (rc == hipSuccess) rc = hipMemcpy(*out, host, n * bytes, hipMemcpyHostToDevice);
	if (rc == hipSuccess) return true;
	std::fprintf(stderr, "ntsig: cannot bring the %llu values of %s to the device: %s\n", (unsigned long long)n, file, hipGetErrorString(rc));
	return false;
}

// what matrix and gather do with their files before anything goes to the device, in this order: every header is read, files[1 ..] counted differently from
// files[0] are refused, every file's pairs are read, and the library says whether a device can be used — the matrix of one empty list touches the device and
// nothing else.  EXIT_SUCCESS: sigs holds the files
int load_all(int n_files, char** files, std::vector<Sig>& sigs)
{
	sigs.resize(n_files);
	for (int i = 0; i < n_files; ++i)
		if (!load(files[i], sigs[i], false)) return EXIT_FAILURE;
	for (int i = 1; i < n_files; ++i)
		if (const char* d = differs_in(sigs[0].h, sigs[i].h)) return refuse(files[0], files[i], d);
	for (int i = 0; i < n_files; ++i)
		if (!load(files[i], sigs[i], true)) return EXIT_FAILURE;
	uint64_t none = 0, probe = 0;
	const void* null_list = nullptr;
	if (ntc_signature_matrix_device(0, nullptr, 1, &null_list, &none, &probe) != 0) {
		std::fprintf(stderr, "ntsig: %s\n", ntc_last_error());
		return EXIT_FAILURE;
	}
	return EXIT_SUCCESS;
}

int matrix(int n_files, char** files, bool containment)
{
	std::vector<Sig> sigs;
	if (int rc = load_all(n_files, files, sigs)) return rc;
	DeviceLists d;
	d.p.assign(n_files, nullptr);
	std::vector<uint64_t> n(n_files);
	for (int i = 0; i < n_files; ++i) {
		n[i] = sigs[i].h.n;
		if (!to_device(&d.p[i], sigs[i].hashes.data(), n[i], 8, files[i])) return EXIT_FAILURE;
	}
	std::vector<uint64_t> common((size_t)n_files * n_files);
	if (ntc_signature_matrix_device(0, nullptr, (uint32_t)n_files, d.p.data(), n.data(), common.data()) != 0) {
		std::fprintf(stderr, "ntsig: %s\n", ntc_last_error());
		return EXIT_FAILURE;
	}
	for (int j = 0; j < n_files; ++j)
		std::printf("\t%s", files[j]);
	std::printf("\n");
	for (int i = 0; i < n_files; ++i) {
		std::printf("%s", files[i]);
		for (int j = 0; j < n_files; ++j) {
			const uint64_t c = common[(size_t)i * n_files + j], den = containment ? n[i] : n[i] + n[j] - c;
			std::printf("\t%.6f", den ? (double)c / (double)den : 0.0);
		}
		std::printf("\n");
	}
	return EXIT_SUCCESS;
}

double ratio(uint64_t num, uint64_t den) { return den ? (double)num / (double)den : 0.0; }

// files[0] is the query, the references follow
int gather(int n_files, char** files, uint64_t threshold)
{
	std::vector<Sig> sigs;
	if (int rc = load_all(n_files, files, sigs)) return rc;
	const Sig& query = sigs[0];
	const int n_refs = n_files - 1;
	char** ref_files = files + 1;
	DeviceLists d; // [references][query hashes][query counts]
	d.p.assign(n_refs + 2, nullptr);
	std::vector<uint64_t> n(n_refs);
	const uint64_t nq = query.h.n;
	if (!to_device(&d.p[n_refs], query.hashes.data(), nq, 8, files[0]) || !to_device(&d.p[n_refs + 1], query.counts.data(), nq, 4, files[0])) return EXIT_FAILURE;
	for (int i = 0; i < n_refs; ++i) {
		n[i] = sigs[i + 1].h.n;
		if (!to_device(&d.p[i], sigs[i + 1].hashes.data(), n[i], 8, ref_files[i])) return EXIT_FAILURE;
	}
	std::vector<ntc_gather_row> rows(n_refs);
	uint32_t n_rows = 0;
	uint64_t rest = 0, rest_weight = 0, total_weight = 0;
	if (ntc_signature_gather_device(0, nullptr, d.p[n_refs], d.p[n_refs + 1], nq, (uint32_t)n_refs, d.p.data(), n.data(), threshold, rows.data(), (uint32_t)n_refs, &n_rows,
	                                &rest, &rest_weight) != 0) {
		std::fprintf(stderr, "ntsig: %s\n", ntc_last_error());
		return EXIT_FAILURE;
	}
	for (uint32_t c : query.counts)
		total_weight += c;
	std::printf("rank\treference\tcommon\tunique\tf_orig_query\tf_unique_query\tf_unique_weighted\tf_match\tavg_abund\n");
	for (uint32_t r = 0; r < n_rows; ++r) {
		const ntc_gather_row& g = rows[r];
		std::printf("%u\t%s\t%llu\t%llu\t%.6f\t%.6f\t%.6f\t%.6f\t%.6f\n", r + 1, ref_files[g.ref], (unsigned long long)g.common, (unsigned long long)g.unique, ratio(g.common, nq),
		            ratio(g.unique, nq), ratio(g.unique_weight, total_weight), ratio(g.unique, n[g.ref]), ratio(g.unique_weight, g.unique));
	}
	std::printf("unassigned\t-\t-\t%llu\t-\t%.6f\t%.6f\t-\t%.6f\n", (unsigned long long)rest, ratio(rest, nq), ratio(rest_weight, total_weight), ratio(rest_weight, rest));
	return EXIT_SUCCESS;
}

int usage()
{
	std::fprintf(stderr, "Usage: ntsig info F.sig\n       ntsig compare A.sig B.sig\n       ntsig matrix [--containment] A.sig B.sig ...\n"
	                     "       ntsig gather [--threshold N] QUERY.sig REF.sig ...\n");
	return EXIT_FAILURE;
}

} // namespace

int main(int argc, char** argv)
{
	if (argc < 2) return usage();
	const std::string cmd(argv[1]);
	if (cmd == "info" && argc == 3) {
		Sig s;
		if (!load(argv[2], s, false)) return EXIT_FAILURE;
		print_header(argv[2], s.h);
		return EXIT_SUCCESS;
	}
	if (cmd == "compare" && argc == 4) {
		Sig a, b;
		if (!load(argv[2], a, true) || !load(argv[3], b, true)) return EXIT_FAILURE;
		if (const char* differs = differs_in(a.h, b.h)) return refuse(argv[2], argv[3], differs);
		uint64_t common = 0;
		if (ntc_signature_compare(a.hashes.data(), a.h.n, b.hashes.data(), b.h.n, &common) != 0) {
			std::fprintf(stderr, "ntsig: %s\n", ntc_last_error());
			return EXIT_FAILURE;
		}
		const uint64_t uni = a.h.n + b.h.n - common;
		std::printf("n_a\t%llu\nn_b\t%llu\ncommon\t%llu\n", (unsigned long long)a.h.n, (unsigned long long)b.h.n, (unsigned long long)common);
		std::printf("jaccard\t%.6f\ncontainment_a_in_b\t%.6f\ncontainment_b_in_a\t%.6f\n", uni ? (double)common / (double)uni : 0.0,
		            a.h.n ? (double)common / (double)a.h.n : 0.0, b.h.n ? (double)common / (double)b.h.n : 0.0);
		return EXIT_SUCCESS;
	}
	if (cmd == "matrix") {
		const bool containment = argc > 2 && std::strcmp(argv[2], "--containment") == 0;
		const int first = containment ? 3 : 2;
		if (argc - first < 1 || argc - first > 1024) return usage();
		return matrix(argc - first, argv + first, containment);
	}
	if (cmd == "gather") {
		int first = 2;
		uint64_t threshold = 1;
		if (argc > 2 && std::strcmp(argv[2], "--threshold") == 0) {
			char* end = nullptr;
			if (argc < 4 || argv[3][0] < '0' || argv[3][0] > '9') return usage();
			threshold = std::strtoull(argv[3], &end, 10);
			if (*end) return usage();
			first = 4;
		}
		const int n_refs = argc - first - 1; // behind the query
		if (n_refs < 1 || n_refs > 1024) return usage();
		return gather(n_refs + 1, argv + first, threshold);
	}
	return usage();
}
