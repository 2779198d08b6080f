// tools/density_host_check.cpp -- the host half of `ska density` (skh_density_text, skh_density_mask_alignment and skh_density,
// ska.rust_amd/host/ska_density.cpp) on its own.  The device calls below skh_density -- loading the array, skx_array_snp_density and
// skx_array_map -- are replaced here by stand-ins that hand over a made-up result, every array in a heap block of exactly the size the ABI
// promises, so that a sanitizer sees a read past their end: from no sample, no chromosome, no region and no SNP to some hundred, chromosomes
// without a base, windows of 1 and of 2^31, regions at a chromosome's first and last position, names longer than a format buffer.  Every text
// and the masked alignment are formed a second time in plain loops here and compared byte for byte; the refusals (NULL arguments, another
// `which`, W or T out of range, a result that names what is not there, bins of another window, an alignment of another length, a prefix that
// cannot be written, the engine's own refusal) must come back as errors with a message.  No device and no libskx.so: the file is compiled
// together with ska_density.cpp.
//   g++ -std=c++17 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -o density_host_check tools/density_host_check.cpp ska.rust_amd/host/ska_density.cpp
//   ./density_host_check          prints the counts; exit code 0 when everything held
#include "../include/skx_host.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

static std::string g_error;
extern "C" void skx_set_last_error(const char *msg) { g_error = msg ? msg : ""; }
extern "C" void skx_free(void *p) { free(p); }
extern "C" void skx_phase_add(const char *, double) {}

// ---- the stand-ins for the device half: one made-up world at a time
struct World {
    std::vector<std::string> names, ids;
    std::vector<uint64_t> lens;
    uint64_t W = 1000;
    std::vector<skx_density_sample> samples;
    std::vector<skx_density_region> regions;
    std::vector<skx_density_bin> bins;
    std::vector<uint64_t> snps; std::vector<uint8_t> snp_ref;
    std::string aln;                                                // what the stand-in for skx_array_map hands over
    int fail_with = SKX_OK, map_fails_with = SKX_OK;
    uint64_t total() const { uint64_t t = 0; for (auto l : lens) t += l; return t; }
};
static World g_world;
struct skx_array { int unused; };
static skx_array g_array;
template <typename T> static T *exact_copy(const std::vector<T> &v)
{
    T *p = (T *)malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0));
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}
static skx_density_result result_of(const World &w, bool with_snps)
{
    skx_density_result r{};
    r.info.windows = 100; r.info.repeat_windows = 7; r.info.sites = 90; r.info.n_chrom = w.ids.size(); r.info.n_bins = w.bins.size();
    r.info.n_snps = w.snps.size(); r.info.n_regions = w.regions.size();
    r.samples = exact_copy(w.samples); r.regions = exact_copy(w.regions); r.bins = exact_copy(w.bins); r.chrom_lens = exact_copy(w.lens);
    std::vector<char> blob; for (auto &i : w.ids) { blob.insert(blob.end(), i.begin(), i.end()); blob.push_back(0); }
    r.chrom_ids = exact_copy(blob);
    if (with_snps) { r.snps = exact_copy(w.snps); r.snp_ref = exact_copy(w.snp_ref); }
    return r;
}
static void free_result(skx_density_result &r) { free(r.samples); free(r.regions); free(r.bins); free(r.chrom_ids); free(r.chrom_lens); free(r.snps); free(r.snp_ref); r = skx_density_result{}; }
extern "C" int skh_load_array(skx_ctx *, const char *const *, int, int, skx_array **out) { *out = &g_array; return SKX_OK; }
extern "C" void skx_array_free(skx_array *) {}
extern "C" int skx_array_info(const skx_array *, skx_array_info_t *info) { memset(info, 0, sizeof *info); info->n_samples = info->total_samples = g_world.names.size(); return SKX_OK; }
extern "C" const char *skx_array_name(const skx_array *, uint64_t i) { return g_world.names[i].c_str(); }
extern "C" int skx_array_snp_density(skx_array *, const char *, uint64_t, uint32_t, int flags, skx_density_result *out)
{
    memset(out, 0, sizeof *out);
    if (g_world.fail_with != SKX_OK) { skx_set_last_error("density: made-up refusal"); return g_world.fail_with; }
    *out = result_of(g_world, flags & SKX_DENSITY_WANT_SNPS);
    return SKX_OK;
}
extern "C" int skx_array_map(skx_array *, const char *, int ambig_mask, int repeat_mask, int format, int, char **buf, uint64_t *len)
{
    if (g_world.map_fails_with != SKX_OK || ambig_mask || !repeat_mask || format) { skx_set_last_error("map: made-up refusal"); return g_world.map_fails_with ? g_world.map_fails_with : SKX_EINVAL; }
    *buf = (char *)malloc(g_world.aln.size() + 1); memcpy(*buf, g_world.aln.data(), g_world.aln.size()); (*buf)[g_world.aln.size()] = 0; *len = g_world.aln.size();
    return SKX_OK;
}

static unsigned long long compared = 0, refused = 0, failures = 0;
static void fail(const char *what) { failures++; fprintf(stderr, "FAILED: %s (last error: %s)\n", what, g_error.c_str()); }

// ---- the texts and the masked alignment a second time, in plain loops
static std::string expected(int which, const World &w)
{
    std::vector<uint64_t> off(1, 0); for (auto l : w.lens) off.push_back(off.back() + l);
    std::ostringstream o;
    if (which == SKH_DENSITY_REGIONS) {
        o << "sample\tchromosome\tstart\tend\tlength\tsnps\n";
        for (auto &g : w.regions) o << w.names[g.sample] << '\t' << w.ids[g.chrom] << '\t' << (uint64_t)g.start + 1 << '\t' << (uint64_t)g.end + 1 << '\t' << (uint64_t)g.end - g.start + 1 << '\t' << g.snps << '\n';
    } else if (which == SKH_DENSITY_SUMMARY) {
        o << "sample\tsites\tcallable\tambiguous\tmissing\tsnps\tdense_snps\tregions\tregion_bases\tsnps_outside\n";
        for (size_t s = 0; s < w.names.size(); s++) {
            const skx_density_sample &q = w.samples[s];
            o << w.names[s] << '\t' << q.sites << '\t' << q.callable << '\t' << q.ambiguous << '\t' << q.missing << '\t' << q.snps << '\t' << q.dense_snps << '\t' << q.regions << '\t'
              << q.region_bases << '\t' << q.snps - q.dense_snps << '\n';
        }
    } else if (which == SKH_DENSITY_BINS) {
        o << "chromosome\tstart\tend\tsnps\tdense_snps\n";
        size_t b = 0;
        for (size_t c = 0; c < w.ids.size(); c++)
            for (uint64_t at = 0; at < w.lens[c]; at += w.W, b++) o << w.ids[c] << '\t' << at + 1 << '\t' << std::min(at + w.W, w.lens[c]) << '\t' << w.bins[b].snps << '\t' << w.bins[b].dense_snps << '\n';
    } else {
        o << "sample\tchromosome\tposition\tref\talt\tdense\n";
        for (size_t i = 0; i < w.snps.size(); i++) {
            const uint64_t v = w.snps[i], s = (v >> 34) & 0xFFFFFFFull, x = (v >> 2) & 0xFFFFFFFFull;
            size_t c = 0; while (!(off[c] <= x && x < off[c + 1])) c++;
            o << w.names[s] << '\t' << w.ids[c] << '\t' << x - off[c] + 1 << '\t' << (char)w.snp_ref[i] << '\t' << "ACTG"[v & 3] << '\t' << ((v >> 62) & 1) << '\n';
        }
    }
    return o.str();
}
static std::string expected_masked(const World &w)
{
    std::vector<uint64_t> off(1, 0); for (auto l : w.lens) off.push_back(off.back() + l);
    std::vector<std::string> line;
    { std::istringstream in(w.aln); std::string l; while (std::getline(in, l)) line.push_back(l); }
    for (auto &g : w.regions) { std::string &l = line[2 * g.sample + 1]; for (uint64_t x = off[g.chrom] + g.start; x <= off[g.chrom] + g.end; x++) if (l[x] != '-') l[x] = 'N'; }
    std::string o; for (auto &l : line) { o += l; o += '\n'; }
    return o;
}

static World make_world(std::mt19937_64 &g, size_t S, size_t C, uint64_t W, size_t n_regions, size_t n_snps)
{
    World w; w.W = W;
    for (size_t s = 0; s < S; s++) w.names.push_back(s % 5 == 3 ? std::string(s % 200 + 260, 'n') + std::to_string(s) : "sample_" + std::to_string(s));      // names longer than put()'s buffer
    for (size_t c = 0; c < C; c++) { w.ids.push_back(c % 4 == 2 ? std::string(300, 'c') + std::to_string(c) : "chr" + std::to_string(c)); w.lens.push_back(c % 3 == 1 ? 0 : 1 + g() % 700); }
    for (size_t s = 0; s < S; s++) { skx_density_sample q{}; uint64_t *f = &q.sites; for (int i = 0; i < 8; i++) f[i] = s % 2 ? g() : g() % 1000; if (q.dense_snps > q.snps) std::swap(q.dense_snps, q.snps); w.samples.push_back(q); }
    for (auto l : w.lens) for (uint64_t at = 0; at < l; at += W) w.bins.push_back({(uint32_t)g(), (uint32_t)g()});
    std::vector<size_t> full; for (size_t c = 0; c < C; c++) if (w.lens[c]) full.push_back(c);
    if (S && !full.empty()) {
        for (size_t i = 0; i < n_regions; i++) {
            const size_t c = full[g() % full.size()];
            uint32_t a = (uint32_t)(g() % w.lens[c]), b = (uint32_t)(g() % w.lens[c]); if (a > b) std::swap(a, b);
            if (i == 0) { a = 0; b = (uint32_t)w.lens[c] - 1; }    // a whole chromosome, first and last position
            w.regions.push_back({(uint32_t)(g() % S), (uint32_t)c, a, b, (uint32_t)g()});
        }
        std::vector<uint64_t> off(1, 0); for (auto l : w.lens) off.push_back(off.back() + l);
        for (size_t i = 0; i < n_snps; i++) {
            const uint64_t x = i == 0 ? w.total() - 1 : g() % w.total();
            w.snps.push_back(((uint64_t)(g() % S) << 34) | (x << 2) | (g() & 3) | ((g() & 1) << 62));
            w.snp_ref.push_back("ACGT"[g() & 3]);
        }
    }
    for (size_t s = 0; s < S; s++) { w.aln += ">" + w.names[s] + "\n"; for (uint64_t x = 0; x < w.total(); x++) w.aln += "ACGT-N"[g() % 6]; w.aln += "\n"; }
    return w;
}

static std::string slurp(const std::string &path) { std::ifstream in(path, std::ios::binary); std::ostringstream o; o << in.rdbuf(); return o.str(); }

int main()
{
    std::mt19937_64 g(20261021);
    const char *tmp = getenv("TMPDIR") ? getenv("TMPDIR") : "/tmp";
    const std::string prefix = std::string(tmp) + "/density_host_check_" + std::to_string((unsigned long long)g()), masked = prefix + ".masked.aln";
    const char *suffix[4] = {".density.regions.tsv", ".density.summary.tsv", ".density.bins.tsv", ".density.snps.tsv"};
    unsigned long long masked_bytes = 0;
    for (size_t S : {0, 1, 2, 17, 130})
        for (size_t C : {0, 1, 2, 3, 9})
            for (uint64_t W : {1ull, 7ull, 1000ull, 1ull << 31})
                for (size_t n : {0, 1, 5000}) {
                    g_world = make_world(g, S, C, W, n, n);
                    const World &w = g_world;
                    std::vector<const char *> names_v; for (auto &x : w.names) names_v.push_back(x.c_str());
                    const char **names = exact_copy(names_v);
                    skx_density_result r = result_of(w, true);
                    for (int which = SKH_DENSITY_REGIONS; which <= SKH_DENSITY_SNPS; which++) {
                        char *buf = nullptr; uint64_t len = 0;
                        if (skh_density_text(which, &r, S ? names : nullptr, S, W, &buf, &len) != SKX_OK) { fail("skh_density_text refused good arguments"); continue; }
                        if (std::string(buf, len) != expected(which, w) || buf[len] != 0) fail("a text differs from the plain-loop restatement");
                        skx_free(buf); compared++;
                    }
                    {
                        char *aln = (char *)malloc(w.aln.size() + 1); memcpy(aln, w.aln.data(), w.aln.size());
                        const std::string want = expected_masked(w);
                        if (skh_density_mask_alignment(aln, w.aln.size(), &r, S ? names : nullptr, S) != SKX_OK) fail("skh_density_mask_alignment refused good arguments");
                        else if (std::string(aln, w.aln.size()) != want) fail("the masked alignment differs from the plain-loop restatement");
                        for (size_t i = 0; i < want.size(); i++) masked_bytes += want[i] != w.aln[i];
                        free(aln); compared++;
                    }
                    free_result(r); free(names);
                    for (int with_snps = 0; with_snps < 2; with_snps++) {
                        for (auto s : suffix) remove((prefix + s).c_str());
                        remove(masked.c_str());
                        if (skh_density((skx_ctx *)&g_array, "ref.fa", "x.skf", prefix.c_str(), W, 5, with_snps, with_snps ? masked.c_str() : nullptr) != SKX_OK) { fail("skh_density refused good arguments"); continue; }
                        for (int which = 0; which < 4; which++) {
                            const bool there = std::ifstream(prefix + suffix[which]).good();
                            if (there != (which < 3 || with_snps)) fail("a file is missing, or one too many was written");
                            else if (there && slurp(prefix + suffix[which]) != expected(which, w)) fail("a file differs from the plain-loop restatement");
                            compared++;
                        }
                        if (with_snps && slurp(masked) != expected_masked(w)) fail("the masked alignment file differs");
                        if (!with_snps && std::ifstream(masked).good()) fail("a masked alignment nobody asked for");
                    }
                    for (auto s : suffix) remove((prefix + s).c_str());
                    remove(masked.c_str());
                }
    if (!masked_bytes) fail("no made-up world had a byte to mask");
    // refusals: each an error code and a message
    g_world = make_world(g, 4, 3, 50, 6, 6);
    {
        const World &w = g_world;
        std::vector<const char *> names_v; for (auto &x : w.names) names_v.push_back(x.c_str());
        const char **names = exact_copy(names_v);
        skx_density_result r = result_of(w, true);
        char *buf = nullptr; uint64_t len = 0;
        auto expect = [&](int rc, int code, const char *what) { if (rc != code || g_error.empty()) fail(what); else refused++; g_error.clear(); };
        expect(skh_density_text(4, &r, names, 4, 50, &buf, &len), SKX_EINVAL, "which = 4 taken");
        expect(skh_density_text(-1, &r, names, 4, 50, &buf, &len), SKX_EINVAL, "which = -1 taken");
        expect(skh_density_text(0, nullptr, names, 4, 50, &buf, &len), SKX_EINVAL, "NULL result taken");
        expect(skh_density_text(0, &r, nullptr, 4, 50, &buf, &len), SKX_EINVAL, "NULL names taken");
        expect(skh_density_text(0, &r, names, 4, 50, nullptr, &len), SKX_EINVAL, "NULL buf taken");
        expect(skh_density_text(0, &r, names, 4, 50, &buf, nullptr), SKX_EINVAL, "NULL len taken");
        expect(skh_density_text(2, &r, names, 4, 0, &buf, &len), SKX_EINVAL, "window 0 taken");
        expect(skh_density_text(2, &r, names, 4, 1, &buf, &len), SKX_EINVAL, "bins of another window taken");
        expect(skh_density_text(0, &r, names, 2, 50, &buf, &len), SKX_EINVAL, "a region of a sample that is not there taken");
        expect(skh_density_text(3, &r, names, 2, 50, &buf, &len), SKX_EINVAL, "a SNP of a sample that is not there taken");
        { skx_density_result q = r; q.snps = nullptr; expect(skh_density_text(3, &q, names, 4, 50, &buf, &len), SKX_EINVAL, "a result without the SNP list taken"); }
        { skx_density_result q = r; q.regions = nullptr; expect(skh_density_text(0, &q, names, 4, 50, &buf, &len), SKX_EINVAL, "a result without its regions taken"); }
        std::string aln = w.aln;
        expect(skh_density_mask_alignment(&aln[0], aln.size() - 1, &r, names, 4), SKX_EINVAL, "an alignment of another length taken");
        expect(skh_density_mask_alignment(&aln[0], aln.size(), nullptr, names, 4), SKX_EINVAL, "mask: NULL result taken");
        expect(skh_density_mask_alignment(&aln[0], aln.size(), &r, nullptr, 4), SKX_EINVAL, "mask: NULL names taken");
        { r.regions[2].end = (uint32_t)w.lens[r.regions[2].chrom]; expect(skh_density_mask_alignment(&aln[0], aln.size(), &r, names, 4), SKX_EINVAL, "a region past its chromosome taken"); }
        if (aln != w.aln) fail("a refusal wrote into the alignment");
        for (uint64_t bad : {0ull, (1ull << 31) + 1}) expect(skh_density((skx_ctx *)&g_array, "ref.fa", "x.skf", prefix.c_str(), bad, 5, 0, nullptr), SKX_EINVAL, "skh_density: a window out of range taken");
        for (uint32_t bad : {0u, 1u, 65536u}) expect(skh_density((skx_ctx *)&g_array, "ref.fa", "x.skf", prefix.c_str(), 1000, bad, 0, nullptr), SKX_EINVAL, "skh_density: min_snps out of range taken");
        expect(skh_density(nullptr, "ref.fa", "x.skf", prefix.c_str(), 1000, 5, 0, nullptr), SKX_EINVAL, "skh_density: NULL context taken");
        expect(skh_density((skx_ctx *)&g_array, nullptr, "x.skf", prefix.c_str(), 1000, 5, 0, nullptr), SKX_EINVAL, "skh_density: NULL reference taken");
        expect(skh_density((skx_ctx *)&g_array, "ref.fa", nullptr, prefix.c_str(), 1000, 5, 0, nullptr), SKX_EINVAL, "skh_density: NULL file taken");
        expect(skh_density((skx_ctx *)&g_array, "ref.fa", "x.skf", nullptr, 1000, 5, 0, nullptr), SKX_EINVAL, "skh_density: NULL prefix taken");
        expect(skh_density((skx_ctx *)&g_array, "ref.fa", "x.skf", "/nonexistent-directory/for/sure/out", 50, 5, 0, nullptr), SKX_EIO, "skh_density: an unwritable prefix taken");
        g_world.map_fails_with = SKX_EINVAL;
        expect(skh_density((skx_ctx *)&g_array, "ref.fa", "x.skf", prefix.c_str(), 50, 5, 0, masked.c_str()), SKX_EINVAL, "skh_density: skx_array_map's refusal not passed on");
        if (std::ifstream(masked).good()) fail("a refused alignment was written");
        for (auto s : suffix) remove((prefix + s).c_str());
        g_world.fail_with = SKX_EUNSUP;
        expect(skh_density((skx_ctx *)&g_array, "ref.fa", "x.skf", prefix.c_str(), 50, 5, 1, masked.c_str()), SKX_EUNSUP, "skh_density: the engine's refusal not passed on");
        for (auto s : suffix) if (std::ifstream(prefix + s).good()) fail("a refusal wrote a file");
        if (buf) fail("a refusal wrote through buf");
        free_result(r); free(names);
    }
    printf("density_host_check: %llu texts compared (%llu bytes masked among them), %llu refusals, %llu failures\n", compared, masked_bytes, refused, failures);
    return failures ? 1 : 0;
}
