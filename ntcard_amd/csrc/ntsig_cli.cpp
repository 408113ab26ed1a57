// ntsig_cli.cpp — `ntsig`: signature files (`ntcard --signature`, include/ntcard_hip.h: ntc_signature_write) from the command line.
//   ntsig info F.sig            the header: how the file was counted, and how many values it holds
//   ntsig compare A.sig B.sig   |A n B|, Jaccard and both containments — refused when the headers differ in anything but n
//   ntsig matrix [--containment] A.sig B.sig ...   all pairs at once, as a TSV: Jaccard, or the containment of the row's file in the column's
//   ntsig gather [--threshold N] QUERY.sig REF.sig ...   which references are in the query and what each explains on its own, as a TSV in pick order
//                               (ntc_signature_gather_device)
//   ntsig merge     -o OUT.sig A.sig [B.sig ...]            the union, counts added and saturating at 2^32 - 1 (ntc_signature_union_device)
//   ntsig intersect -o OUT.sig A.sig REF.sig [REF.sig ...]  A's pairs whose hash every REF holds (ntc_signature_select_device, NTC_SIG_IN_ALL)
//   ntsig subtract  -o OUT.sig A.sig REF.sig [REF.sig ...]  A's pairs whose hash no REF holds (NTC_SIG_IN_NONE)
//   ntsig filter    [--min-count N] [--max-count N] -o OUT.sig A.sig   A's pairs whose count lies inside the bounds (no references)
//   ntsig hist      [-c COV] F.sig   the abundance spectrum of the file's counts as a TSV (ntc_signature_hist_device): the lines n, weight and sBits, then
//                               v, hist[v], hist[v] << (sBits - 1) for v = 1 .. COV (default 1000 like ntcard's -c, at most 65535) and a last row ">COV".  The
//                               third column scales by the NOMINAL sampling rate 2 * 2^-sBits; the rate of canonical k-mers is a little off it (DESIGN.md §4
//                               "What the rate means") and the column is not corrected for that.
// These five take at most 1024 files behind A (merge: 1024 in all, the lists of one union), go through load_all like matrix and gather, write OUT with ntc_signature_write under A's header with the new n
// — to OUT.part first, renamed when it is whole, so an OUT that cannot be written leaves nothing behind — and print a usage block of their own (usage_algebra)
// on their own argument errors.
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

enum class Algebra { merge, intersect, subtract, filter };

int fail_lib()
{
	std::fprintf(stderr, "ntsig: %s\n", ntc_last_error());
	return EXIT_FAILURE;
}

// the pairs under `header` with n = the number of pairs, to `path`: written to path.part and renamed when whole, so a failure leaves nothing behind
int write_sig(const char* path, ntc_sig_header header, const std::vector<uint64_t>& hashes, const std::vector<uint32_t>& counts)
{
	const std::string part = std::string(path) + ".part";
	header.n = hashes.size();
	if (ntc_signature_write(part.c_str(), &header, hashes.data(), counts.data()) != 0) {
		(void)std::remove(part.c_str());
		return fail_lib();
	}
	if (std::rename(part.c_str(), path) != 0) {
		(void)std::remove(part.c_str());
		std::fprintf(stderr, "ntsig: cannot write %s\n", path);
		return EXIT_FAILURE;
	}
	return EXIT_SUCCESS;
}

// files[0] is A; merge unions all files, intersect and subtract select A's pairs by the files behind it, filter by the count bounds alone
int algebra(Algebra op, int n_files, char** files, const char* out_path, uint32_t min_count, uint32_t max_count)
{
	std::vector<Sig> sigs;
	if (int rc = load_all(n_files, files, sigs)) return rc;
	const bool merge = op == Algebra::merge;
	DeviceLists d; // [hashes n_files][counts n_files (merge: all; else A's)][out hashes][out counts]
	d.p.assign(2 * (size_t)n_files + 2, nullptr);
	std::vector<uint64_t> n(n_files);
	uint64_t room = 0;
	for (int i = 0; i < n_files; ++i) {
		n[i] = sigs[i].h.n;
		if (!to_device(&d.p[i], sigs[i].hashes.data(), n[i], 8, files[i])) return EXIT_FAILURE;
		if ((merge || i == 0) && !to_device(&d.p[n_files + i], sigs[i].counts.data(), n[i], 4, files[i])) return EXIT_FAILURE;
		if (merge || i == 0) room += n[i];
	}
	void** out = &d.p[2 * (size_t)n_files];
	const uint32_t mode = op == Algebra::subtract ? NTC_SIG_IN_NONE : NTC_SIG_IN_ALL;
	auto call = [&](uint64_t cap, uint64_t* n_out) {
		if (merge) return ntc_signature_union_device(0, nullptr, (uint32_t)n_files, d.p.data(), d.p.data() + n_files, n.data(), out[0], out[1], cap, n_out);
		return ntc_signature_select_device(0, nullptr, d.p[0], d.p[n_files], n[0], (uint32_t)(n_files - 1), d.p.data() + 1, n.data() + 1, mode, min_count, max_count, out[0], out[1],
		                                   cap, n_out);
	};
	uint64_t n_out = 0;
	if (call(0, &n_out) != 0) return fail_lib(); // the size alone (room is always enough; the result is often far smaller)
	std::vector<uint64_t> hashes(n_out);
	std::vector<uint32_t> counts(n_out);
	if (n_out) {
		if (n_out > room || hipMalloc(&out[0], n_out * 8) != hipSuccess || hipMalloc(&out[1], n_out * 4) != hipSuccess) {
			std::fprintf(stderr, "ntsig: no device memory for the %llu pairs of %s\n", (unsigned long long)n_out, out_path);
			return EXIT_FAILURE;
		}
		uint64_t again = 0;
		if (call(n_out, &again) != 0) return fail_lib();
		if (again != n_out || hipMemcpy(hashes.data(), out[0], n_out * 8, hipMemcpyDeviceToHost) != hipSuccess ||
		    hipMemcpy(counts.data(), out[1], n_out * 4, hipMemcpyDeviceToHost) != hipSuccess) {
			std::fprintf(stderr, "ntsig: cannot bring the %llu pairs of %s back from the device\n", (unsigned long long)n_out, out_path);
			return EXIT_FAILURE;
		}
	}
	return write_sig(out_path, sigs[0].h, hashes, counts);
}

int hist(char* file, uint32_t cov)
{
	std::vector<Sig> sigs;
	if (int rc = load_all(1, &file, sigs)) return rc;
	const Sig& s = sigs[0];
	DeviceLists d;
	d.p.assign(1, nullptr);
	if (!to_device(&d.p[0], s.counts.data(), s.h.n, 4, file)) return EXIT_FAILURE;
	std::vector<uint64_t> h((size_t)cov + 2);
	uint64_t weight = 0;
	if (ntc_signature_hist_device(0, nullptr, d.p[0], s.h.n, cov, h.data(), &weight) != 0) return fail_lib();
	if (s.h.s_bits < 2 || s.h.s_bits > 24) {
		std::fprintf(stderr, "ntsig: %s: sBits %u (2 .. 24 are written)\n", file, s.h.s_bits);
		return EXIT_FAILURE;
	}
	const uint32_t shift = s.h.s_bits - 1; // 1 / (2 * 2^-sBits), the nominal sampling rate
	std::printf("n\t%llu\nweight\t%llu\nsBits\t%u\n", (unsigned long long)s.h.n, (unsigned long long)weight, s.h.s_bits);
	for (uint32_t v = 1; v <= cov; ++v)
		std::printf("%u\t%llu\t%llu\n", v, (unsigned long long)h[v], (unsigned long long)(h[v] << shift));
	std::printf(">%u\t%llu\t%llu\n", cov, (unsigned long long)h[cov + 1], (unsigned long long)(h[cov + 1] << shift));
	return EXIT_SUCCESS;
}

// the argument errors of merge, intersect, subtract, filter and hist (every other error path of ntsig ends in usage())
int usage_algebra()
{
	std::fprintf(stderr, "Usage: ntsig merge     -o OUT.sig A.sig [B.sig ...]\n       ntsig intersect -o OUT.sig A.sig REF.sig [REF.sig ...]\n"
	                     "       ntsig subtract  -o OUT.sig A.sig REF.sig [REF.sig ...]\n       ntsig filter    [--min-count N] [--max-count N] -o OUT.sig A.sig\n"
	                     "       ntsig hist      [-c COV] F.sig\n"
	                     "merge adds the counts of a hash (they saturate at 2^32 - 1); intersect keeps A's pairs whose hash every REF holds, subtract those no REF\n"
	                     "holds; at most 1024 files behind A (merge: 1024 in all), all counted alike.  hist prints v, the sampled distinct k-mers with count v, and that number scaled\n"
	                     "by the nominal sampling rate 2 * 2^-sBits (canonical k-mers are sampled at a slightly different rate; the column is not corrected),\n"
	                     "for v = 1 .. COV (default 1000, at most 65535), then a row >COV.\n");
	return EXIT_FAILURE;
}

// a decimal number of at most `most` -> true
bool number(const char* text, uint64_t most, uint64_t* out)
{
	if (text[0] < '0' || text[0] > '9' || std::strlen(text) > 10) return false;
	char* end = nullptr;
	*out = std::strtoull(text, &end, 10);
	return *end == 0 && *out <= most;
}

// merge, intersect, subtract, filter, hist: args are what stands behind the command
int algebra_main(const std::string& cmd, int n_args, char** args)
{
	const char* out_path = nullptr;
	uint64_t min_count = 0, max_count = 0, cov = 1000;
	bool have_cov = false, have_bounds = false;
	std::vector<char*> files;
	for (int i = 0; i < n_args; ++i) {
		const std::string a(args[i]);
		const bool value = i + 1 < n_args;
		if (a == "-o") {
			if (!value || out_path) return usage_algebra();
			out_path = args[++i];
		} else if (a == "--min-count" || a == "--max-count") {
			if (!value || !number(args[i + 1], 0xffffffffull, a == "--min-count" ? &min_count : &max_count)) return usage_algebra();
			have_bounds = true, ++i;
		} else if (a == "-c") {
			if (!value || !number(args[i + 1], 65535, &cov) || cov < 1) return usage_algebra();
			have_cov = true, ++i;
		} else if (a.size() > 1 && a[0] == '-') {
			return usage_algebra();
		} else {
			files.push_back(args[i]);
		}
	}
	const size_t nf = files.size();
	if (cmd == "hist") return (out_path || have_bounds || nf != 1) ? usage_algebra() : hist(files[0], (uint32_t)cov);
	if (!out_path || have_cov || (have_bounds && cmd != "filter") || (max_count != 0 && min_count > max_count)) return usage_algebra();
	if (cmd == "filter") return nf != 1 ? usage_algebra() : algebra(Algebra::filter, 1, files.data(), out_path, (uint32_t)min_count, (uint32_t)max_count);
	// (merge: A and what stands behind it are the union's lists, 1024 in all)
	if (cmd == "merge") return (nf < 1 || nf > 1024) ? usage_algebra() : algebra(Algebra::merge, (int)nf, files.data(), out_path, 0, 0);
	if (nf < 2 || nf > 1025) return usage_algebra();
	return algebra(cmd == "intersect" ? Algebra::intersect : Algebra::subtract, (int)nf, files.data(), out_path, 0, 0);
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
	if (cmd == "merge" || cmd == "intersect" || cmd == "subtract" || cmd == "filter" || cmd == "hist") return algebra_main(cmd, argc - 2, argv + 2);
	return usage();
}
