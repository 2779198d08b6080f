// tools/screen_host_check.cpp -- the host half of `ska screen` (skh_screen_text and skh_screen, ska.rust_amd/host/ska_screen.cpp) on its own.
// The device calls below skh_screen -- loading the array and skx_array_screen -- are replaced here by stand-ins that hand over made-up counts in
// heap blocks of exactly the size the ABI promises, so that a sanitizer sees a read past their end: random shapes from no record and no sample to
// some hundred of each, ids of every length from empty on, records without windows, counts at the thresholds' edges.  Every text is formed a
// second time in plain loops here and compared byte for byte; the refusals (NULL arguments, NaN and out-of-range proportions, another `which`, an
// output prefix that cannot be written) must come back as errors with a message.  No device and no libskx.so: the file is compiled together with
// ska_screen.cpp.
//   g++ -std=c++17 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -o screen_host_check tools/screen_host_check.cpp ska.rust_amd/host/ska_screen.cpp
//   ./screen_host_check          prints the counts; exit code 0 when everything held
#include "../include/skx_host.h"
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
    std::vector<std::string> names, ids;
    std::vector<skx_screen_record> records;
    std::vector<skx_screen_cell> cells;
    int fail_with = SKX_OK;
};
static World g_world;
struct skx_array { int unused; };
static skx_array g_array;
extern "C" int skh_load_array(skx_ctx *, const char *const *, int, int, skx_array **out) { *out = &g_array; return SKX_OK; }
extern "C" void skx_array_free(skx_array *) {}
extern "C" int skx_array_info(const skx_array *, skx_array_info_t *info) { memset(info, 0, sizeof *info); info->n_samples = info->total_samples = g_world.names.size(); return SKX_OK; }
extern "C" const char *skx_array_name(const skx_array *, uint64_t i) { return g_world.names[i].c_str(); }
template <typename T> static T *exact_copy(const std::vector<T> &v)
{
    T *p = (T *)malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0));
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}
static char *exact_ids(const std::vector<std::string> &ids)
{
    size_t n = 0; for (auto &s : ids) n += s.size() + 1;
    char *p = (char *)malloc(n ? n : 1), *w = p;
    for (auto &s : ids) { memcpy(w, s.c_str(), s.size() + 1); w += s.size() + 1; }
    return p;
}
extern "C" int skx_array_screen(skx_array *, const char *, uint64_t *n_records, skx_screen_record **records, char **ids, skx_screen_cell **cells)
{
    if (g_world.fail_with != SKX_OK) { skx_set_last_error("screen: made-up refusal"); return g_world.fail_with; }
    *n_records = g_world.records.size(); *records = exact_copy(g_world.records); *ids = exact_ids(g_world.ids); *cells = exact_copy(g_world.cells);
    return SKX_OK;
}

static unsigned long long compared = 0, refused = 0, failures = 0;
static void fail(const char *what) { failures++; fprintf(stderr, "FAILED: %s (last error: %s)\n", what, g_error.c_str()); }

static bool passes(const skx_screen_record &r, const skx_screen_cell &c, double C, double I)
{
    if (!r.windows) return false;
    uint64_t need = (uint64_t)std::ceil(C * (double)r.windows); if (need < 1) need = 1;
    return c.found >= need && c.match >= (uint64_t)std::ceil(I * (double)c.found);
}
static std::string expected(int which, const World &w, double C, double I)
{
    const size_t S = w.names.size();
    std::ostringstream o;
    char num[64];
    if (which == SKH_SCREEN_PAIRS) {
        o << "record\tlength\twindows\tsample\tfound\tmatch\tambig\tsnp\tcover\tidentity\n";
        for (size_t r = 0; r < w.records.size(); r++)
            for (size_t s = 0; s < S; s++) {
                const skx_screen_cell &c = w.cells[r * S + s];
                if (!passes(w.records[r], c, C, I)) continue;
                o << w.ids[r] << '\t' << w.records[r].length << '\t' << w.records[r].windows << '\t' << w.names[s] << '\t' << c.found << '\t' << c.match << '\t' << c.ambig
                  << '\t' << c.found - c.match - c.ambig;
                snprintf(num, sizeof num, "\t%.4f\t%.4f\n", (double)c.found / (double)w.records[r].windows, (double)c.match / (double)c.found);
                o << num;
            }
    } else if (which == SKH_SCREEN_SUMMARY) {
        o << "record\tlength\twindows\trows_hit\tsamples_passing\n";
        for (size_t r = 0; r < w.records.size(); r++) {
            size_t n = 0; for (size_t s = 0; s < S; s++) n += passes(w.records[r], w.cells[r * S + s], C, I);
            o << w.ids[r] << '\t' << w.records[r].length << '\t' << w.records[r].windows << '\t' << w.records[r].rows_hit << '\t' << n << '\n';
        }
    } else {
        o << "record"; for (auto &n : w.names) o << '\t' << n; o << '\n';
        for (size_t r = 0; r < w.records.size(); r++) {
            o << w.ids[r];
            for (size_t s = 0; s < S; s++) o << '\t' << (passes(w.records[r], w.cells[r * S + s], C, I) ? '1' : '0');
            o << '\n';
        }
    }
    return o.str();
}

static World make_world(std::mt19937_64 &g, size_t R, size_t S)
{
    World w;
    for (size_t s = 0; s < S; s++) w.names.push_back("sample_" + std::string(s % 7, 'x') + std::to_string(s));
    for (size_t r = 0; r < R; r++) {
        w.ids.push_back(r % 11 == 3 ? std::string() : std::string(r % 300, 'g') + std::to_string(r));      // an empty id, and ids longer than put()'s buffer
        skx_screen_record rec{};
        rec.windows = r % 5 == 4 ? 0 : g() % 1000 + 1;
        rec.length = rec.windows ? rec.windows + 30 : g() % 31;
        rec.rows_hit = rec.windows ? g() % (rec.windows + 1) : 0;
        w.records.push_back(rec);
        for (size_t s = 0; s < S; s++) {
            skx_screen_cell c{};
            const uint64_t edge = (uint64_t)std::ceil(0.9 * (double)rec.windows);
            c.found = !rec.rows_hit ? 0 : (uint32_t)(s % 3 == 0 && edge <= rec.rows_hit ? edge - (g() % 2 && edge ? 1 : 0) : g() % (rec.rows_hit + 1));      // at the cover threshold and one below
            c.match = c.found ? (uint32_t)(g() % (c.found + 1)) : 0;
            c.ambig = (uint32_t)(g() % (c.found - c.match + 1));
            w.cells.push_back(c);
        }
    }
    return w;
}

static std::string slurp(const std::string &path) { std::ifstream in(path, std::ios::binary); std::ostringstream o; o << in.rdbuf(); return o.str(); }

int main()
{
    std::mt19937_64 g(20261020);
    const char *tmp = getenv("TMPDIR") ? getenv("TMPDIR") : "/tmp";
    const std::string prefix = std::string(tmp) + "/screen_host_check_" + std::to_string((unsigned long long)g());
    const double props[][2] = {{0.9, 0.0}, {0.0, 0.0}, {1.0, 1.0}, {0.5, 0.5}, {1e-9, 0.999999}};
    const size_t shapes[][2] = {{0, 0}, {0, 3}, {3, 0}, {1, 1}, {5, 2}, {17, 33}, {64, 16}, {130, 70}, {7, 300}};
    for (auto &sh : shapes) {
        g_world = make_world(g, sh[0], sh[1]);
        const World &w = g_world;
        std::vector<const char *> names; for (auto &n : w.names) names.push_back(n.c_str());
        skx_screen_record *rec = exact_copy(w.records); skx_screen_cell *cells = exact_copy(w.cells); char *ids = exact_ids(w.ids);
        for (auto &p : props) {
            for (int which = SKH_SCREEN_PAIRS; which <= SKH_SCREEN_MATRIX; which++) {
                char *buf = nullptr; uint64_t len = 0;
                const int r = skh_screen_text(which, w.records.size(), rec, ids, cells, names.data(), names.size(), p[0], p[1], &buf, &len);
                if (r != SKX_OK) { fail("skh_screen_text refused good arguments"); continue; }
                if (std::string(buf, len) != expected(which, w, p[0], p[1]) || buf[len] != 0) fail("a text differs from the plain-loop restatement");
                skx_free(buf); compared++;
            }
            for (int matrix = 0; matrix < 2; matrix++) {
                const char *suffix[3] = {".screen.tsv", ".screen.summary.tsv", ".screen.matrix.tsv"};
                for (auto s : suffix) remove((prefix + s).c_str());
                if (skh_screen((skx_ctx *)&g_array, "x.skf", "panel.fa", prefix.c_str(), p[0], p[1], matrix) != SKX_OK) { fail("skh_screen refused good arguments"); continue; }
                for (int which = 0; which < 3; which++) {
                    const bool there = std::ifstream(prefix + suffix[which]).good();
                    if (there != (which < 2 || matrix)) fail("the wrong set of files was written");
                    else if (there && slurp(prefix + suffix[which]) != expected(which, w, p[0], p[1])) fail("a file differs from the plain-loop restatement");
                    compared += there;
                }
                for (auto s : suffix) remove((prefix + s).c_str());
            }
        }
        free(rec); free(cells); free(ids);
    }
    // refusals: each an error code and a message, nothing written through the out pointers' targets
    g_world = make_world(g, 4, 3);
    {
        const World &w = g_world;
        std::vector<const char *> names; for (auto &n : w.names) names.push_back(n.c_str());
        skx_screen_record *rec = exact_copy(w.records); skx_screen_cell *cells = exact_copy(w.cells); char *ids = exact_ids(w.ids);
        char *buf = nullptr; uint64_t len = 0;
        auto expect = [&](int r, int code, const char *what) { if (r != code || g_error.empty()) fail(what); else refused++; g_error.clear(); };
        const double nan = std::nan("");
        expect(skh_screen_text(3, 4, rec, ids, cells, names.data(), 3, 0.9, 0.0, &buf, &len), SKX_EINVAL, "which = 3 taken");
        expect(skh_screen_text(-1, 4, rec, ids, cells, names.data(), 3, 0.9, 0.0, &buf, &len), SKX_EINVAL, "which = -1 taken");
        expect(skh_screen_text(0, 4, nullptr, ids, cells, names.data(), 3, 0.9, 0.0, &buf, &len), SKX_EINVAL, "NULL records taken");
        expect(skh_screen_text(0, 4, rec, nullptr, cells, names.data(), 3, 0.9, 0.0, &buf, &len), SKX_EINVAL, "NULL ids taken");
        expect(skh_screen_text(0, 4, rec, ids, nullptr, names.data(), 3, 0.9, 0.0, &buf, &len), SKX_EINVAL, "NULL cells taken");
        expect(skh_screen_text(0, 4, rec, ids, cells, nullptr, 3, 0.9, 0.0, &buf, &len), SKX_EINVAL, "NULL names taken");
        expect(skh_screen_text(0, 4, rec, ids, cells, names.data(), 3, 0.9, 0.0, nullptr, &len), SKX_EINVAL, "NULL buf taken");
        expect(skh_screen_text(0, 4, rec, ids, cells, names.data(), 3, 0.9, 0.0, &buf, nullptr), SKX_EINVAL, "NULL len taken");
        for (double bad : {nan, -0.001, 1.001, (double)INFINITY}) {
            expect(skh_screen_text(0, 4, rec, ids, cells, names.data(), 3, bad, 0.0, &buf, &len), SKX_EINVAL, "a cover outside [0, 1] taken");
            expect(skh_screen_text(0, 4, rec, ids, cells, names.data(), 3, 0.9, bad, &buf, &len), SKX_EINVAL, "an identity outside [0, 1] taken");
            expect(skh_screen((skx_ctx *)&g_array, "x.skf", "panel.fa", prefix.c_str(), bad, 0.0, 1), SKX_EINVAL, "skh_screen: a cover outside [0, 1] taken");
            expect(skh_screen((skx_ctx *)&g_array, "x.skf", "panel.fa", prefix.c_str(), 0.9, bad, 1), SKX_EINVAL, "skh_screen: an identity outside [0, 1] taken");
        }
        expect(skh_screen(nullptr, "x.skf", "panel.fa", prefix.c_str(), 0.9, 0.0, 0), SKX_EINVAL, "skh_screen: NULL context taken");
        expect(skh_screen((skx_ctx *)&g_array, "x.skf", "panel.fa", nullptr, 0.9, 0.0, 0), SKX_EINVAL, "skh_screen: NULL prefix taken");
        expect(skh_screen((skx_ctx *)&g_array, "x.skf", "panel.fa", "/nonexistent-directory/for/sure/out", 0.9, 0.0, 1), SKX_EIO, "skh_screen: an unwritable prefix taken");
        g_world.fail_with = SKX_EEMPTY;
        expect(skh_screen((skx_ctx *)&g_array, "x.skf", "panel.fa", prefix.c_str(), 0.9, 0.0, 1), SKX_EEMPTY, "skh_screen: the engine's refusal not passed on");
        if (buf) fail("a refusal wrote through buf");
        free(rec); free(cells); free(ids);
    }
    printf("screen_host_check: %llu texts compared, %llu refusals, %llu failures\n", compared, refused, failures);
    return failures ? 1 : 0;
}
