// tools/qc_host_check.cpp -- the host half of `ska qc` (skh_qc_text and skh_qc, ska.rust_amd/host/ska_qc.cpp) on its own.  The device calls
// below skh_qc -- loading the array and skx_array_sample_qc -- are replaced here by stand-ins that hand over made-up counts, and skh_qc_text is
// given its records and names in heap blocks of exactly the size the ABI promises, so that a sanitizer sees a read past their end: from no sample
// to some hundred, counts at the rule's edges (all equal, one outlier exactly at and one above M x d, values above 2^32 and up to 2^64 - 1, a
// core_present above core_rows).  Every text is formed a second time in plain loops here and compared byte for byte; the refusals (NULL
// arguments, another `which`, a negative or NaN mad, min_freq outside [0, 1], an output prefix that cannot be written, the engine's own refusal)
// must come back as errors with a message.  No device and no libskx.so: the file is compiled together with ska_qc.cpp.
//   g++ -std=c++17 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -o qc_host_check tools/qc_host_check.cpp ska.rust_amd/host/ska_qc.cpp
//   ./qc_host_check          prints the counts; exit code 0 when everything held
#include "../include/skx_host.h"
#include <algorithm>
#include <cmath>
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
    std::vector<std::string> names;
    std::vector<skx_qc_sample> samples;
    skx_qc_info info{};
    int fail_with = SKX_OK;
};
static World g_world;
struct skx_array { int unused; };
static skx_array g_array;
extern "C" int skh_load_array(skx_ctx *, const char *const *, int, int, skx_array **out) { *out = &g_array; return SKX_OK; }
extern "C" void skx_array_free(skx_array *) {}
extern "C" int skx_array_info(const skx_array *, skx_array_info_t *info) { memset(info, 0, sizeof *info); info->n_samples = info->total_samples = g_world.names.size(); return SKX_OK; }
extern "C" const char *skx_array_name(const skx_array *, uint64_t i) { return g_world.names[i].c_str(); }
extern "C" int skx_array_sample_qc(skx_array *, double, skx_qc_sample *samples, skx_qc_info *info)
{
    if (g_world.fail_with != SKX_OK) { skx_set_last_error("qc: made-up refusal"); return g_world.fail_with; }
    for (size_t s = 0; s < g_world.samples.size(); s++) samples[s] = g_world.samples[s];
    if (info) *info = g_world.info;
    return SKX_OK;
}
template <typename T> static T *exact_copy(const std::vector<T> &v)
{
    T *p = (T *)malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0));
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

static unsigned long long compared = 0, refused = 0, failures = 0;
static void fail(const char *what) { failures++; fprintf(stderr, "FAILED: %s (last error: %s)\n", what, g_error.c_str()); }

// ---- the rule and the texts a second time, in plain loops
static const char *const METRICS[6] = {"kmers", "ambiguous", "singletons", "core_missing", "private_alleles", "minor_alleles"};
static uint64_t value_of(const World &w, size_t s, int m)
{
    const skx_qc_sample &q = w.samples[s];
    if (m == 0) return q.kmers;
    if (m == 1) return q.ambiguous;
    if (m == 2) return q.singletons;
    if (m == 3) return w.info.core_rows > q.core_present ? w.info.core_rows - q.core_present : 0;
    return m == 4 ? q.private_alleles : q.minor_alleles;
}
struct Stat { uint64_t min = 0, med = 0, max = 0, mad = 0, flagged = 0; std::vector<int> side; };      // side: -1 low, 1 high
static Stat stat_of(const World &w, int m, double M)
{
    const size_t S = w.samples.size();
    Stat st; st.side.assign(S, 0);
    if (!S) return st;
    std::vector<uint64_t> x(S), v, dev(S);
    for (size_t s = 0; s < S; s++) x[s] = value_of(w, s, m);
    v = x; std::sort(v.begin(), v.end());
    st.min = v[0]; st.max = v[S - 1]; st.med = v[(S - 1) / 2];
    for (size_t s = 0; s < S; s++) dev[s] = x[s] > st.med ? x[s] - st.med : st.med - x[s];
    v = dev; std::sort(v.begin(), v.end());
    st.mad = v[(S - 1) / 2];
    const double d = (double)(st.mad > 1 ? st.mad : 1);
    for (size_t s = 0; s < S; s++) {
        if ((double)dev[s] > M * d && x[s] != st.med) st.side[s] = x[s] > st.med ? 1 : (m == 0 ? -1 : 0);
        st.flagged += st.side[s] != 0;
    }
    return st;
}
static std::string expected(int which, const World &w, double M)
{
    const size_t S = w.samples.size();
    Stat st[6];
    for (int m = 0; m < 6; m++) st[m] = stat_of(w, m, M);
    std::vector<std::string> flags(S);
    for (size_t s = 0; s < S; s++)
        for (int m = 0; m < 6; m++)
            if (st[m].side[s]) { if (!flags[s].empty()) flags[s] += ","; flags[s] += m ? METRICS[m] : (st[m].side[s] < 0 ? "low_kmers" : "high_kmers"); }
    std::ostringstream o;
    if (which == SKH_QC_SAMPLES) {
        o << "sample\tkmers\tambiguous\tsingletons\tcore_present\tcore_missing\tprivate_alleles\tminor_alleles\tflags\n";
        for (size_t s = 0; s < S; s++) {
            const skx_qc_sample &q = w.samples[s];
            o << w.names[s] << '\t' << q.kmers << '\t' << q.ambiguous << '\t' << q.singletons << '\t' << q.core_present << '\t' << value_of(w, s, 3) << '\t'
              << q.private_alleles << '\t' << q.minor_alleles << '\t' << (flags[s].empty() ? "-" : flags[s]) << '\n';
        }
    } else if (which == SKH_QC_SUMMARY) {
        o << "samples\t" << S << "\nrows\t" << w.info.rows << "\nrows_present\t" << w.info.rows_present << "\ncore_rows\t" << w.info.core_rows << "\ncore_variant_rows\t"
          << w.info.core_variant_rows << "\nthreshold\t" << w.info.threshold << "\nmetric\tmin\tmedian\tmax\tmad\tflagged\n";
        for (int m = 0; m < 6; m++) o << METRICS[m] << '\t' << st[m].min << '\t' << st[m].med << '\t' << st[m].max << '\t' << st[m].mad << '\t' << st[m].flagged << '\n';
    } else {
        for (size_t s = 0; s < S; s++) if (!flags[s].empty()) o << w.names[s] << '\n';
    }
    return o.str();
}

static World make_world(std::mt19937_64 &g, size_t S, int kind)
{
    World w;
    const uint64_t top = kind == 0 ? 50 : kind == 1 ? (1ull << 40) : kind == 2 ? ~0ull : 7;
    for (size_t s = 0; s < S; s++) {
        w.names.push_back(s % 9 == 4 ? std::string(s % 300 + 260, 'n') + std::to_string(s) : "sample_" + std::to_string(s));      // names longer than put()'s buffer
        skx_qc_sample q{};
        uint64_t *f = &q.kmers;
        for (int c = 0; c < 6; c++) f[c] = kind == 3 ? 1000 + g() % 3 : g() % top;
        w.samples.push_back(q);
    }
    w.info.rows = top; w.info.rows_present = top / 2; w.info.core_rows = kind == 3 ? 1001 : top / 2 + 1; w.info.core_variant_rows = 3; w.info.threshold = S ? S : 1;
    if (kind == 3 && S > 4) {                                              // mad <= 1, d = 1: exactly M = 5 above the median is no flag, 6 above is one
        std::vector<uint64_t> v; for (auto &q : w.samples) v.push_back(q.kmers);
        std::sort(v.begin(), v.end());
        const uint64_t med = v[(S - 1) / 2];
        w.samples[1].kmers = med + 5; w.samples[2].kmers = med + 6; w.samples[3].kmers = med - 6; w.samples[4].ambiguous = 5000;
    }
    return w;
}

static std::string slurp(const std::string &path) { std::ifstream in(path, std::ios::binary); std::ostringstream o; o << in.rdbuf(); return o.str(); }

int main()
{
    std::mt19937_64 g(20261020);
    const char *tmp = getenv("TMPDIR") ? getenv("TMPDIR") : "/tmp";
    const std::string prefix = std::string(tmp) + "/qc_host_check_" + std::to_string((unsigned long long)g());
    const char *suffix[3] = {".qc.tsv", ".qc.summary.tsv", ".qc.flagged.txt"};
    const double mads[] = {5.0, 0.0, 1.0, 2.5, 1e18};
    const size_t sizes[] = {0, 1, 2, 3, 5, 17, 64, 130, 300};
    unsigned long long flagged_lines = 0;
    for (size_t S : sizes)
        for (int kind = 0; kind < 4; kind++) {
            g_world = make_world(g, S, kind);
            const World &w = g_world;
            std::vector<const char *> names_v; for (auto &n : w.names) names_v.push_back(n.c_str());
            const char **names = exact_copy(names_v);
            skx_qc_sample *rec = exact_copy(w.samples);
            for (double M : mads) {
                for (int which = SKH_QC_SAMPLES; which <= SKH_QC_FLAGGED; which++) {
                    char *buf = nullptr; uint64_t len = 0;
                    const int r = skh_qc_text(which, S ? rec : nullptr, S ? names : nullptr, S, &w.info, M, &buf, &len);
                    if (r != SKX_OK) { fail("skh_qc_text refused good arguments"); continue; }
                    const std::string want = expected(which, w, M);
                    if (std::string(buf, len) != want || buf[len] != 0) fail("a text differs from the plain-loop restatement");
                    if (which == SKH_QC_FLAGGED) flagged_lines += std::count(want.begin(), want.end(), '\n');
                    skx_free(buf); compared++;
                }
                for (auto s : suffix) remove((prefix + s).c_str());
                if (skh_qc((skx_ctx *)&g_array, "x.skf", prefix.c_str(), 0.9, M) != SKX_OK) { fail("skh_qc refused good arguments"); continue; }
                for (int which = 0; which < 3; which++) {
                    if (!std::ifstream(prefix + suffix[which]).good()) fail("a file is missing");
                    else if (slurp(prefix + suffix[which]) != expected(which, w, M)) fail("a file differs from the plain-loop restatement");
                    compared++;
                }
                for (auto s : suffix) remove((prefix + s).c_str());
            }
            free(names); free(rec);
        }
    if (!flagged_lines) fail("no made-up world had a flagged sample");
    // refusals: each an error code and a message, nothing written through the out pointers' targets
    g_world = make_world(g, 4, 0);
    {
        const World &w = g_world;
        std::vector<const char *> names_v; for (auto &n : w.names) names_v.push_back(n.c_str());
        const char **names = exact_copy(names_v);
        skx_qc_sample *rec = exact_copy(w.samples);
        char *buf = nullptr; uint64_t len = 0;
        auto expect = [&](int r, int code, const char *what) { if (r != code || g_error.empty()) fail(what); else refused++; g_error.clear(); };
        const double nan = std::nan("");
        expect(skh_qc_text(3, rec, names, 4, &w.info, 5.0, &buf, &len), SKX_EINVAL, "which = 3 taken");
        expect(skh_qc_text(-1, rec, names, 4, &w.info, 5.0, &buf, &len), SKX_EINVAL, "which = -1 taken");
        expect(skh_qc_text(0, nullptr, names, 4, &w.info, 5.0, &buf, &len), SKX_EINVAL, "NULL samples taken");
        expect(skh_qc_text(0, rec, nullptr, 4, &w.info, 5.0, &buf, &len), SKX_EINVAL, "NULL names taken");
        expect(skh_qc_text(0, rec, names, 4, nullptr, 5.0, &buf, &len), SKX_EINVAL, "NULL info taken");
        expect(skh_qc_text(0, rec, names, 4, &w.info, 5.0, nullptr, &len), SKX_EINVAL, "NULL buf taken");
        expect(skh_qc_text(0, rec, names, 4, &w.info, 5.0, &buf, nullptr), SKX_EINVAL, "NULL len taken");
        for (double bad : {nan, -0.001, -(double)INFINITY}) {
            expect(skh_qc_text(0, rec, names, 4, &w.info, bad, &buf, &len), SKX_EINVAL, "a negative or NaN mad taken");
            expect(skh_qc((skx_ctx *)&g_array, "x.skf", prefix.c_str(), 0.9, bad), SKX_EINVAL, "skh_qc: a negative or NaN mad taken");
        }
        for (double bad : {nan, -0.001, 1.001, (double)INFINITY})
            expect(skh_qc((skx_ctx *)&g_array, "x.skf", prefix.c_str(), bad, 5.0), SKX_EINVAL, "skh_qc: a min_freq outside [0, 1] taken");
        expect(skh_qc(nullptr, "x.skf", prefix.c_str(), 0.9, 5.0), SKX_EINVAL, "skh_qc: NULL context taken");
        expect(skh_qc((skx_ctx *)&g_array, nullptr, prefix.c_str(), 0.9, 5.0), SKX_EINVAL, "skh_qc: NULL file taken");
        expect(skh_qc((skx_ctx *)&g_array, "x.skf", nullptr, 0.9, 5.0), SKX_EINVAL, "skh_qc: NULL prefix taken");
        expect(skh_qc((skx_ctx *)&g_array, "x.skf", "/nonexistent-directory/for/sure/out", 0.9, 5.0), SKX_EIO, "skh_qc: an unwritable prefix taken");
        g_world.fail_with = SKX_EUNSUP;
        expect(skh_qc((skx_ctx *)&g_array, "x.skf", prefix.c_str(), 0.9, 5.0), SKX_EUNSUP, "skh_qc: the engine's refusal not passed on");
        for (auto s : suffix) if (std::ifstream(prefix + s).good()) fail("a refusal wrote a file");
        if (buf) fail("a refusal wrote through buf");
        free(names); free(rec);
    }
    printf("qc_host_check: %llu texts compared (%llu flagged lines among them), %llu refusals, %llu failures\n", compared, flagged_lines, refused, failures);
    return failures ? 1 : 0;
}
