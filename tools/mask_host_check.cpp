// tools/mask_host_check.cpp -- the host half of `ska mask` (skh_mask_read_regions, skh_mask_read_bed, skh_mask_text and skh_mask,
// ska.rust_amd/host/ska_mask.cpp) on its own.  The device calls below skh_mask -- loading the array, skx_array_snp_density,
// skx_reference_records, skx_array_mask_regions and the save -- are replaced here by stand-ins that hand over a made-up world.  Every text a
// reader gets lies in a heap block of exactly its length (no terminator), so that a sanitizer sees a read past its end: good files, every
// truncation of them, and some ten thousand random edits (a byte changed, dropped, doubled; a tab, a line feed, a carriage return, a '#' or a
// digit put in).  Each text is read a second time by plain loops written here and the two answers compared: the same intervals, or a refusal
// that names the same line.  The summary text is formed a second time in plain loops and compared byte for byte.  skh_mask's own refusals (NULL
// arguments, no source, two sources, W or T out of range, an output that is the input, a file that cannot be opened, the engine's refusal)
// must come back as errors with a message.  No device and no libskx.so: the file is compiled together with ska_mask.cpp.
//   g++ -std=c++17 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -o mask_host_check tools/mask_host_check.cpp ska.rust_amd/host/ska_mask.cpp
//   ./mask_host_check          prints the counts; exit code 0 when everything held
#include "../include/skx_host.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

static std::string g_error;
extern "C" void skx_set_last_error(const char *msg) { g_error = msg ? msg : ""; }
extern "C" void skx_free(void *p) { free(p); }
extern "C" void skx_phase_add(const char *, double) {}

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, g_error.c_str()); g_failures++; } } while (0)

// ---- the stand-ins for the device half
struct World {
    std::vector<std::string> names, ids;
    std::vector<uint64_t> lens;
    std::vector<skx_density_region> regions;                         // what the stand-in for skx_array_snp_density finds
    int load_fails = SKX_OK, density_fails = SKX_OK, mask_fails = SKX_OK, save_fails = SKX_OK;
    std::vector<skx_mask_interval> seen;                             // what skx_array_mask_regions was given
    std::string saved; uint64_t window = 0; uint32_t min_snps = 0;
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
extern "C" int skh_load_array(skx_ctx *, const char *const *, int, int, skx_array **out)
{
    if (g_world.load_fails != SKX_OK) { skx_set_last_error("made-up load refusal"); return g_world.load_fails; }
    *out = &g_array; return SKX_OK;
}
extern "C" void skx_array_free(skx_array *) {}
extern "C" int skx_array_info(const skx_array *, skx_array_info_t *info) { memset(info, 0, sizeof *info); info->n_samples = info->total_samples = g_world.names.size(); return SKX_OK; }
extern "C" const char *skx_array_name(const skx_array *, uint64_t i) { return g_world.names[i].c_str(); }
extern "C" int skx_array_snp_density(skx_array *, const char *, uint64_t window, uint32_t min_snps, int, skx_density_result *out)
{
    memset(out, 0, sizeof *out);
    if (g_world.density_fails != SKX_OK) { skx_set_last_error("density: made-up refusal"); return g_world.density_fails; }
    g_world.window = window; g_world.min_snps = min_snps;
    out->info.n_regions = g_world.regions.size();
    out->regions = exact_copy(g_world.regions);
    return SKX_OK;
}
extern "C" int skx_reference_records(const char *, char **ids, uint64_t **lens, uint64_t *n)
{
    std::vector<char> blob; for (auto &i : g_world.ids) { blob.insert(blob.end(), i.begin(), i.end()); blob.push_back(0); }
    *ids = exact_copy(blob); *lens = exact_copy(g_world.lens); *n = g_world.ids.size();
    return SKX_OK;
}
extern "C" int skx_array_mask_regions(skx_array *, const char *, const skx_mask_interval *iv, uint64_t n, skx_mask_sample *samples, skx_mask_info *info)
{
    if (g_world.mask_fails != SKX_OK) { skx_set_last_error("mask: made-up refusal"); return g_world.mask_fails; }
    g_world.seen.assign(iv, iv + n);
    for (size_t s = 0; s < g_world.names.size(); s++) { samples[s].sites_in_regions = 100 + s; samples[s].cells_masked = 7 * s; }
    *info = skx_mask_info{1000, 2000, 30, 4, 1966, n};
    return SKX_OK;
}
extern "C" int skh_save_skf(skx_array *, const char *out_prefix)
{
    if (g_world.save_fails != SKX_OK) { skx_set_last_error("made-up save refusal"); return g_world.save_fails; }
    g_world.saved = out_prefix; return SKX_OK;
}

// ---- the readers a second time, in plain loops
struct Answer { bool ok = true; uint64_t line = 0; std::vector<skx_mask_interval> iv; };
static bool plain_number(const std::string &f, uint64_t &v)
{
    if (f.empty() || f.size() > 10) return false;
    v = 0;
    for (char ch : f) { if (ch < '0' || ch > '9') return false; v = v * 10 + (uint64_t)(ch - '0'); }
    return v <= 0xFFFFFFFFull;
}
static Answer plain_read(const std::string &text, bool bed, const World &w)
{
    Answer a;
    uint64_t no = 0;
    bool header = !bed;
    size_t at = 0;
    while (at < text.size()) {
        size_t nl = text.find('\n', at);
        std::string line = text.substr(at, nl == std::string::npos ? std::string::npos : nl - at);
        at = nl == std::string::npos ? text.size() : nl + 1;
        no++;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.find_first_not_of(" \t") == std::string::npos || line[0] == '#') continue;
        if (header) { header = false; continue; }
        std::vector<std::string> f;
        size_t p = 0;
        for (;;) { size_t t = line.find('\t', p); f.push_back(line.substr(p, t == std::string::npos ? std::string::npos : t - p)); if (t == std::string::npos) break; p = t + 1; }
        auto bad = [&]() { a.ok = false; a.line = no; a.iv.clear(); return a; };
        if (f.size() < (bed ? 3u : 4u)) return bad();
        int64_t s = -1, c = -1;
        if (!bed) { for (size_t i = 0; i < w.names.size() && s < 0; i++) if (w.names[i] == f[0]) s = (int64_t)i; if (s < 0) return bad(); }
        const std::string &chrom = f[bed ? 0 : 1];
        for (size_t i = 0; i < w.ids.size() && c < 0; i++) if (w.ids[i] == chrom) c = (int64_t)i;
        if (c < 0) return bad();
        uint64_t x = 0, y = 0;
        if (!plain_number(f[bed ? 1 : 2], x) || !plain_number(f[bed ? 2 : 3], y)) return bad();
        if (bed ? y <= x : (x < 1 || y < x)) return bad();
        if (y > w.lens[c]) return bad();
        a.iv.push_back(bed ? skx_mask_interval{SKX_MASK_ALL_SAMPLES, (uint32_t)c, (uint32_t)x, (uint32_t)(y - 1)} : skx_mask_interval{(uint32_t)s, (uint32_t)c, (uint32_t)(x - 1), (uint32_t)(y - 1)});
    }
    return a;
}
static uint64_t g_texts = 0, g_refused = 0, g_intervals = 0;
static void compare(const std::string &text, bool bed, const World &w)
{
    char *block = (char *)malloc(text.size() ? text.size() : 1);     // exactly the text: a read past its end is the sanitizer's to see
    if (!text.empty()) memcpy(block, text.data(), text.size());
    std::vector<const char *> names, ids;
    for (auto &n : w.names) names.push_back(n.c_str());
    for (auto &i : w.ids) ids.push_back(i.c_str());
    skx_mask_interval *out = nullptr; uint64_t n = 0;
    g_error.clear();
    const int rc = bed ? skh_mask_read_bed(text.empty() ? nullptr : block, text.size(), ids.data(), w.lens.data(), ids.size(), &out, &n)
                       : skh_mask_read_regions(text.empty() ? nullptr : block, text.size(), names.data(), names.size(), ids.data(), w.lens.data(), ids.size(), &out, &n);
    const Answer want = plain_read(text, bed, w);
    g_texts++;
    if (want.ok) {
        CHECK(rc == SKX_OK && n == want.iv.size());
        if (rc == SKX_OK && n == want.iv.size()) CHECK(n == 0 || memcmp(out, want.iv.data(), n * sizeof(skx_mask_interval)) == 0);
        g_intervals += n;
    } else {
        char expect[64];
        snprintf(expect, sizeof expect, "mask: %s line %llu: ", bed ? "bed" : "regions", (unsigned long long)want.line);
        CHECK(rc == SKX_EINVAL && out == nullptr && n == 0 && g_error.compare(0, strlen(expect), expect) == 0);
        g_refused++;
    }
    free(out);
    free(block);
}

// ---- the summary a second time
static std::string plain_summary(const std::vector<skx_mask_sample> &sm, const skx_mask_info &info, const std::vector<skx_mask_interval> &iv, const std::vector<std::string> &names)
{
    const size_t S = names.size();
    std::vector<uint64_t> count(S + 1, 0), bases(S + 1, 0);
    for (size_t s = 0; s <= S; s++) {
        const uint32_t who = s == S ? SKX_MASK_ALL_SAMPLES : (uint32_t)s;
        uint32_t n_chrom = 0;
        for (auto &q : iv) if (q.sample == who) n_chrom = std::max(n_chrom, q.chrom + 1);
        for (uint32_t c = 0; c < n_chrom; c++) {
            uint64_t top = 0;
            for (auto &q : iv) if (q.sample == who && q.chrom == c) top = std::max<uint64_t>(top, q.end);
            std::vector<char> covered(top + 2, 0);
            bool any = false;
            for (auto &q : iv) if (q.sample == who && q.chrom == c) { any = true; for (uint64_t x = q.start; x <= q.end; x++) covered[x] = 1; }
            if (!any) continue;
            for (uint64_t x = 0; x <= top; x++) { bases[s] += covered[x]; if (covered[x] && (x == 0 || !covered[x - 1])) count[s]++; }      // a run of covered positions is a merged interval
        }
    }
    std::string out = "sample\tintervals\tinterval_bases\tsites_in_regions\tcells_masked\n";
    for (size_t s = 0; s < S; s++)
        out += names[s] + "\t" + std::to_string(count[s]) + "\t" + std::to_string(bases[s]) + "\t" + std::to_string(sm[s].sites_in_regions) + "\t" + std::to_string(sm[s].cells_masked) + "\n";
    out += "all_samples_intervals\t" + std::to_string(count[S]) + "\nall_samples_bases\t" + std::to_string(bases[S]) + "\n";
    out += "sites\t" + std::to_string(info.sites) + "\nrows_in\t" + std::to_string(info.rows_in) + "\nrows_all_samples\t" + std::to_string(info.rows_all_samples) +
           "\nrows_emptied\t" + std::to_string(info.rows_emptied) + "\nrows_out\t" + std::to_string(info.rows_out) + "\n";
    return out;
}

int main()
{
    std::mt19937_64 rng(20261021);
    World &w = g_world;
    w.names = {"s0", "s1", "a sample", std::string(700, 'n'), "s0"};                   // a name longer than a format buffer; a name given twice
    w.ids = {"c1", "c2", "chromosome_three", "c1x"};
    w.lens = {85, 66, 4000000000ull, 1};
    const std::string good_regions = "sample\tchromosome\tstart\tend\tlength\tsnps\ns0\tc1\t21\t32\t12\t3\n# a comment\r\n\r\ns1\tc1\t21\t43\t23\t5\r\na sample\tc2\t66\t66\n \t \n"
                                     "s0\tc2\t1\t1\textra\tcolumns\n" + std::string(700, 'n') + "\tchromosome_three\t3999999999\t4000000000\ns1\tc1x\t1\t1\ns1\tc1\t85\t85";
    const std::string good_bed = "c1\t0\t85\n#track name=phage\nc2\t10\t11\tname\t0\t+\r\n\nc2\t65\t66\nchromosome_three\t0\t4000000000\nc1x\t0\t1\r\nc1\t20\t40";
    for (int bed = 0; bed < 2; bed++) {
        const std::string &good = bed ? good_bed : good_regions;
        const uint64_t before = g_intervals;
        compare(good, bed, w);
        CHECK(g_intervals - before == (bed ? 6u : 7u));
        for (size_t n = 0; n <= good.size(); n++) compare(good.substr(0, n), bed, w);             // every truncation
        static const char PUT[] = {'\t', '\n', '\r', '#', '0', '9', '-', ' ', 'c', 's', '1', 0};
        for (int round = 0; round < 6000; round++) {                                              // random edits, one to three a text
            std::string t = good;
            for (int e = 0, ne = 1 + (int)(rng() % 3); e < ne && !t.empty(); e++) {
                const size_t at = rng() % t.size();
                switch (rng() % 4) {
                case 0: t[at] = PUT[rng() % sizeof PUT]; break;
                case 1: t.erase(at, 1 + rng() % 3); break;
                case 2: t.insert(at, 1, t[at]); break;
                default: t.insert(at, 1, PUT[rng() % sizeof PUT]); break;
                }
            }
            compare(t, bed, w);
        }
    }
    // the refusals, each with its line
    struct Bad { const char *text; bool bed; uint64_t line; const char *what; };
    const Bad bad[] = {
        {"h\ns0\tc1\t5\n", false, 2, "fewer than four fields"}, {"h\n\ns9\tc1\t1\t2\n", false, 3, "unknown sample s9"}, {"h\ns0\tc3\t1\t2\n", false, 2, "unknown chromosome c3"},
        {"h\ns0\tc1\t1\t2\ns0\tc1\tx\t2\n", false, 3, "no number"}, {"h\ns0\tc1\t1\t99999999999\n", false, 2, "no number"}, {"h\ns0\tc1\t0\t2\n", false, 2, "start below 1"},
        {"h\n#x\ns0\tc1\t5\t4\n", false, 3, "end before start"}, {"h\ns0\tc1\t80\t86\n", false, 2, "end past chromosome c1 of 85 bases"},
        {"c1\t5\n", true, 1, "fewer than three fields"}, {"c1\t1\t2\nc9\t1\t2\n", true, 2, "unknown chromosome c9"}, {"c1\t-1\t2\n", true, 1, "no number"},
        {"\n\nc1\t5\t5\n", true, 3, "end not after start"}, {"c2\t0\t66\nc2\t0\t67\n", true, 2, "end past chromosome c2 of 66 bases"}};
    for (const Bad &b : bad) {
        compare(b.text, b.bed, w);
        char expect[128];
        snprintf(expect, sizeof expect, "mask: %s line %llu: ", b.bed ? "bed" : "regions", (unsigned long long)b.line);
        CHECK(g_error.compare(0, strlen(expect), expect) == 0 && g_error.find(b.what) != std::string::npos);
    }
    {   // NULL arguments
        skx_mask_interval *out = nullptr; uint64_t n = 0; const char *nm[1] = {"x"}; const uint64_t ln[1] = {5};
        CHECK(skh_mask_read_regions("x", 1, nm, 1, nm, ln, 1, nullptr, &n) == SKX_EINVAL && skh_mask_read_regions("x", 1, nm, 1, nm, ln, 1, &out, nullptr) == SKX_EINVAL);
        CHECK(skh_mask_read_regions(nullptr, 1, nm, 1, nm, ln, 1, &out, &n) == SKX_EINVAL && skh_mask_read_regions("x", 1, nullptr, 1, nm, ln, 1, &out, &n) == SKX_EINVAL);
        CHECK(skh_mask_read_bed("x", 1, nullptr, ln, 1, &out, &n) == SKX_EINVAL && skh_mask_read_bed("x", 1, nm, nullptr, 1, &out, &n) == SKX_EINVAL && out == nullptr);
    }

    // ---- the summary
    uint64_t summaries = 0;
    for (int round = 0; round < 300; round++) {
        const size_t S = round % 7;
        std::vector<std::string> names;
        for (size_t s = 0; s < S; s++) names.push_back(s == 3 ? std::string(600, 'x') : "sample_" + std::to_string(s));
        std::vector<skx_mask_interval> iv;
        for (int i = 0, ni = (int)(rng() % 40); i < ni; i++) {
            const uint32_t a = (uint32_t)(rng() % 300), len = (uint32_t)(rng() % 40);
            iv.push_back(skx_mask_interval{S && rng() % 4 ? (uint32_t)(rng() % S) : SKX_MASK_ALL_SAMPLES, (uint32_t)(rng() % 3), a, a + len});
        }
        std::vector<skx_mask_sample> sm(S);
        for (auto &q : sm) { q.sites_in_regions = rng() % 100000; q.cells_masked = rng(); }
        const skx_mask_info info{rng(), rng() % 1000, 5, 6, 7, iv.size()};
        std::vector<const char *> nm; for (auto &x : names) nm.push_back(x.c_str());
        skx_mask_sample *psm = exact_copy(sm); skx_mask_interval *piv = exact_copy(iv);
        char *buf = nullptr; uint64_t len = 0;
        const int rc = skh_mask_text(S ? psm : nullptr, &info, iv.empty() ? nullptr : piv, iv.size(), nm.data(), S, &buf, &len);
        CHECK(rc == SKX_OK);
        if (rc == SKX_OK) { CHECK(std::string(buf, len) == plain_summary(sm, info, iv, names) && buf[len] == 0); summaries++; }
        free(buf); free(psm); free(piv);
    }
    {
        const skx_mask_info info{}; skx_mask_sample sm[1] = {}; const char *nm[1] = {"x"}; char *buf = nullptr; uint64_t len = 0;
        const skx_mask_interval out_of_range[1] = {{1, 0, 1, 2}}, backwards[1] = {{0, 0, 3, 2}};
        CHECK(skh_mask_text(sm, &info, out_of_range, 1, nm, 1, &buf, &len) == SKX_EINVAL && skh_mask_text(sm, &info, backwards, 1, nm, 1, &buf, &len) == SKX_EINVAL);
        CHECK(skh_mask_text(sm, nullptr, nullptr, 0, nm, 1, &buf, &len) == SKX_EINVAL && skh_mask_text(nullptr, &info, nullptr, 0, nm, 1, &buf, &len) == SKX_EINVAL);
        CHECK(skh_mask_text(sm, &info, nullptr, 0, nm, 1, nullptr, &len) == SKX_EINVAL && buf == nullptr);
    }

    // ---- the command around the stand-ins
    skx_ctx *ctx = (skx_ctx *)&g_array;                              // (never looked into)
    char dir[] = "/tmp/mask_host_check_XXXXXX";
    CHECK(mkdtemp(dir) != nullptr);
    const std::string d = dir, regions = d + "/r.tsv", bedf = d + "/b.bed", in = d + "/in.skf";
    auto write = [](const std::string &p, const std::string &t) { FILE *f = fopen(p.c_str(), "wb"); fwrite(t.data(), 1, t.size(), f); fclose(f); };
    write(regions, good_regions); write(bedf, good_bed); write(in, "not looked into");
    w.regions = {{1, 0, 20, 42, 5}, {0, 1, 3, 9, 4}};
    CHECK(skh_mask(ctx, "ref.fa", in.c_str(), (d + "/out").c_str(), regions.c_str(), 0, 1000, 5, bedf.c_str(), (d + "/out").c_str()) == SKX_OK);
    CHECK(w.seen.size() == 13 && w.seen[0].start == 20 && w.seen[7].sample == SKX_MASK_ALL_SAMPLES && w.saved == d + "/out");
    {
        FILE *f = fopen((d + "/out.mask.summary.tsv").c_str(), "rb"); CHECK(f != nullptr);
        if (f) { char head[16] = {0}; CHECK(fread(head, 1, 7, f) == 7 && !strcmp(head, "sample\t")); fclose(f); }
    }
    CHECK(skh_mask(ctx, "ref.fa", in.c_str(), (d + "/dense.skf").c_str(), nullptr, 1, 200, 3, nullptr, nullptr) == SKX_OK);
    CHECK(w.seen.size() == 2 && w.seen[0].sample == 1 && w.seen[0].end == 42 && w.seen[1].chrom == 1 && w.window == 200 && w.min_snps == 3);
    CHECK(skh_mask(nullptr, "ref.fa", in.c_str(), "o", nullptr, 1, 1000, 5, nullptr, nullptr) == SKX_EINVAL && skh_mask(ctx, nullptr, in.c_str(), "o", nullptr, 1, 1000, 5, nullptr, nullptr) == SKX_EINVAL);
    CHECK(skh_mask(ctx, "ref.fa", nullptr, "o", nullptr, 1, 1000, 5, nullptr, nullptr) == SKX_EINVAL && skh_mask(ctx, "ref.fa", in.c_str(), nullptr, nullptr, 1, 1000, 5, nullptr, nullptr) == SKX_EINVAL);
    CHECK(skh_mask(ctx, "ref.fa", in.c_str(), "o", nullptr, 0, 1000, 5, nullptr, nullptr) == SKX_EINVAL && g_error.find("is required") != std::string::npos);
    CHECK(skh_mask(ctx, "ref.fa", in.c_str(), "o", regions.c_str(), 1, 1000, 5, nullptr, nullptr) == SKX_EINVAL && g_error.find("exclude each other") != std::string::npos);
    CHECK(skh_mask(ctx, "ref.fa", in.c_str(), "o", nullptr, 1, 0, 5, nullptr, nullptr) == SKX_EINVAL && skh_mask(ctx, "ref.fa", in.c_str(), "o", nullptr, 1, (1ull << 31) + 1, 5, nullptr, nullptr) == SKX_EINVAL);
    CHECK(skh_mask(ctx, "ref.fa", in.c_str(), "o", nullptr, 1, 1000, 1, nullptr, nullptr) == SKX_EINVAL && skh_mask(ctx, "ref.fa", in.c_str(), "o", nullptr, 1, 1000, 65536, nullptr, nullptr) == SKX_EINVAL);
    w.saved.clear();
    CHECK(skh_mask(ctx, "ref.fa", in.c_str(), in.c_str(), nullptr, 1, 1000, 5, nullptr, nullptr) == SKX_EINVAL && g_error.find("never overwritten") != std::string::npos);
    CHECK(skh_mask(ctx, "ref.fa", in.c_str(), (d + "/in").c_str(), nullptr, 1, 1000, 5, nullptr, nullptr) == SKX_EINVAL && skh_mask(ctx, "ref.fa", in.c_str(), (d + "/./in.skf").c_str(), nullptr, 1, 1000, 5, nullptr, nullptr) == SKX_EINVAL);
    CHECK(w.saved.empty());
    CHECK(skh_mask(ctx, "ref.fa", in.c_str(), (d + "/o").c_str(), (d + "/missing.tsv").c_str(), 0, 1000, 5, nullptr, nullptr) == SKX_EIO && g_error.find("cannot open") != std::string::npos);
    write(d + "/bad.bed", "c1\t0\t10\nc2\t0\t67\n");
    CHECK(skh_mask(ctx, "ref.fa", in.c_str(), (d + "/o").c_str(), nullptr, 0, 1000, 5, (d + "/bad.bed").c_str(), nullptr) == SKX_EINVAL && g_error.find("bed line 2") != std::string::npos && w.saved.empty());
    w.load_fails = SKX_EIO;     CHECK(skh_mask(ctx, "ref.fa", in.c_str(), (d + "/o").c_str(), nullptr, 1, 1000, 5, nullptr, nullptr) == SKX_EIO); w.load_fails = SKX_OK;
    w.density_fails = SKX_EINVAL; CHECK(skh_mask(ctx, "ref.fa", in.c_str(), (d + "/o").c_str(), nullptr, 1, 1000, 5, nullptr, nullptr) == SKX_EINVAL && g_error.find("density:") == 0); w.density_fails = SKX_OK;
    w.mask_fails = SKX_EUNSUP;  CHECK(skh_mask(ctx, "ref.fa", in.c_str(), (d + "/o").c_str(), nullptr, 1, 1000, 5, nullptr, nullptr) == SKX_EUNSUP && w.saved.empty()); w.mask_fails = SKX_OK;
    w.save_fails = SKX_EIO;     CHECK(skh_mask(ctx, "ref.fa", in.c_str(), (d + "/o").c_str(), nullptr, 1, 1000, 5, nullptr, (d + "/o").c_str()) == SKX_EIO); w.save_fails = SKX_OK;
    CHECK(skh_mask(ctx, "ref.fa", in.c_str(), (d + "/o").c_str(), nullptr, 1, 1000, 5, nullptr, (d + "/no/such/dir/p").c_str()) == SKX_EIO && g_error.find("cannot create") != std::string::npos);
    for (const char *f : {"/r.tsv", "/b.bed", "/in.skf", "/bad.bed", "/out.mask.summary.tsv"}) remove((d + f).c_str());
    remove(dir);

    printf("mask_host_check: %llu texts read twice (%llu refused with the same line, %llu intervals), %llu summaries formed twice, %d failures\n",
           (unsigned long long)g_texts, (unsigned long long)g_refused, (unsigned long long)g_intervals, (unsigned long long)summaries, g_failures);
    return g_failures ? 1 : 0;
}
