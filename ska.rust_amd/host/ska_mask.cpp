// ska_mask.cpp -- `ska mask`: regions of a reference taken out of a .skf, per sample or for every sample (host side above the C ABI): the two
// readers of interval files, the summary text and the command around one call of skx_array_mask_regions.  The reference has no such mode: its
// `ska weed` removes split k-mers by sequence.  The files and the text are stated in include/skx_host.h and, identically, in tests/mask_model.py.
#include "ska_host_util.h"
#include <string>
#include <vector>

using namespace skh;
namespace {

struct Field { const char *p; size_t n; };

// the next line that is neither blank nor a comment, split at tabs, without its '\r'; no: its number from 1.  false at the end of the text
bool next_line(const char *text, uint64_t len, uint64_t &at, uint64_t &no, std::vector<Field> &f)
{
    while (at < len) {
        const char *p = text + at;
        const char *nl = (const char *)memchr(p, '\n', len - at);
        size_t n = nl ? (size_t)(nl - p) : (size_t)(len - at);
        at += n + (nl ? 1 : 0);
        no++;
        if (n && p[n - 1] == '\r') n--;
        size_t blank = 0;
        while (blank < n && (p[blank] == ' ' || p[blank] == '\t')) blank++;
        if (blank == n || p[0] == '#') continue;
        f.clear();
        size_t a = 0;
        for (size_t i = 0; i <= n; i++)
            if (i == n || p[i] == '\t') { f.push_back(Field{p + a, i - a}); a = i + 1; }
        return true;
    }
    return false;
}

// an unsigned decimal number that fits 32 bits
bool number(const Field &f, uint64_t &v)
{
    if (!f.n || f.n > 10) return false;
    v = 0;
    for (size_t i = 0; i < f.n; i++) { if (f.p[i] < '0' || f.p[i] > '9') return false; v = v * 10 + (uint64_t)(f.p[i] - '0'); }
    return v <= 0xFFFFFFFFull;
}

// the index of the name that equals the field (the first of two equal names), or -1
int64_t find(const Field &f, const char *const *names, uint64_t n)
{
    for (uint64_t i = 0; i < n; i++) if (strlen(names[i]) == f.n && memcmp(names[i], f.p, f.n) == 0) return (int64_t)i;
    return -1;
}

int hand_over(const std::vector<skx_mask_interval> &v, skx_mask_interval **out, uint64_t *n)
{
    skx_mask_interval *p = (skx_mask_interval *)malloc(v.size() * sizeof(skx_mask_interval) + (v.empty() ? 1 : 0));
    if (!p) { skx_set_last_error("out of host memory"); return SKX_ENOMEM; }
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(skx_mask_interval));
    *out = p; *n = v.size();
    return SKX_OK;
}

struct Merged { uint32_t sample, chrom; uint64_t start, end; };
// skx_array_mask_regions' merge: per (sample, chromosome), overlapping or touching
std::vector<Merged> merge(const skx_mask_interval *iv, uint64_t n)
{
    std::vector<skx_mask_interval> v(iv, iv + n);
    std::sort(v.begin(), v.end(), [](const skx_mask_interval &x, const skx_mask_interval &y) {
        return x.sample != y.sample ? x.sample < y.sample : x.chrom != y.chrom ? x.chrom < y.chrom : x.start != y.start ? x.start < y.start : x.end < y.end; });
    std::vector<Merged> out;
    for (const skx_mask_interval &q : v) {
        if (!out.empty() && out.back().sample == q.sample && out.back().chrom == q.chrom && (uint64_t)q.start <= out.back().end + 1) out.back().end = std::max<uint64_t>(out.back().end, q.end);
        else out.push_back(Merged{q.sample, q.chrom, q.start, q.end});
    }
    return out;
}

int read_file(const char *path, std::string &text)
{
    FILE *f = fopen(path, "rb");
    if (!f) { set_error("mask: cannot open %s", path); return SKX_EIO; }
    char tmp[1 << 16];
    size_t n;
    while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) text.append(tmp, n);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) { set_error("mask: cannot read %s", path); return SKX_EIO; }
    return SKX_OK;
}

}  // namespace

extern "C" int skh_mask_read_regions(const char *text, uint64_t len, const char *const *names, uint64_t n_samples, const char *const *chrom_ids, const uint64_t *chrom_lens,
                                     uint64_t n_chrom, skx_mask_interval **out, uint64_t *n)
{
    return guarded([&]() -> int {
    if (out) *out = nullptr;
    if (n) *n = 0;
    if ((len && !text) || !out || !n || (n_samples && !names) || (n_chrom && (!chrom_ids || !chrom_lens))) { skx_set_last_error("skh_mask_read_regions: bad arguments"); return SKX_EINVAL; }
    std::vector<skx_mask_interval> v;
    std::vector<Field> f;
    uint64_t at = 0, no = 0;
    bool header = true;
    while (next_line(text, len, at, no, f)) {
        if (header) { header = false; continue; }
        if (f.size() < 4) { set_error("mask: regions line %llu: fewer than four fields", (unsigned long long)no); return SKX_EINVAL; }
        const int64_t s = find(f[0], names, n_samples), c = find(f[1], chrom_ids, n_chrom);
        if (s < 0) { set_error("mask: regions line %llu: unknown sample %.*s", (unsigned long long)no, (int)std::min<size_t>(f[0].n, 200), f[0].p); return SKX_EINVAL; }
        if (c < 0) { set_error("mask: regions line %llu: unknown chromosome %.*s", (unsigned long long)no, (int)std::min<size_t>(f[1].n, 200), f[1].p); return SKX_EINVAL; }
        uint64_t a = 0, b = 0;
        if (!number(f[2], a) || !number(f[3], b)) { set_error("mask: regions line %llu: start or end is no number", (unsigned long long)no); return SKX_EINVAL; }
        if (a < 1) { set_error("mask: regions line %llu: start below 1 (positions are 1-based)", (unsigned long long)no); return SKX_EINVAL; }
        if (b < a) { set_error("mask: regions line %llu: end before start", (unsigned long long)no); return SKX_EINVAL; }
        if (b > chrom_lens[c]) { set_error("mask: regions line %llu: end past chromosome %s of %llu bases", (unsigned long long)no, chrom_ids[c], (unsigned long long)chrom_lens[c]); return SKX_EINVAL; }
        v.push_back(skx_mask_interval{(uint32_t)s, (uint32_t)c, (uint32_t)(a - 1), (uint32_t)(b - 1)});
    }
    return hand_over(v, out, n);
    });
}

extern "C" int skh_mask_read_bed(const char *text, uint64_t len, const char *const *chrom_ids, const uint64_t *chrom_lens, uint64_t n_chrom, skx_mask_interval **out, uint64_t *n)
{
    return guarded([&]() -> int {
    if (out) *out = nullptr;
    if (n) *n = 0;
    if ((len && !text) || !out || !n || (n_chrom && (!chrom_ids || !chrom_lens))) { skx_set_last_error("skh_mask_read_bed: bad arguments"); return SKX_EINVAL; }
    std::vector<skx_mask_interval> v;
    std::vector<Field> f;
    uint64_t at = 0, no = 0;
    while (next_line(text, len, at, no, f)) {
        if (f.size() < 3) { set_error("mask: bed line %llu: fewer than three fields", (unsigned long long)no); return SKX_EINVAL; }
        const int64_t c = find(f[0], chrom_ids, n_chrom);
        if (c < 0) { set_error("mask: bed line %llu: unknown chromosome %.*s", (unsigned long long)no, (int)std::min<size_t>(f[0].n, 200), f[0].p); return SKX_EINVAL; }
        uint64_t a = 0, b = 0;
        if (!number(f[1], a) || !number(f[2], b)) { set_error("mask: bed line %llu: start or end is no number", (unsigned long long)no); return SKX_EINVAL; }
        if (b <= a) { set_error("mask: bed line %llu: end not after start (the end is exclusive)", (unsigned long long)no); return SKX_EINVAL; }
        if (b > chrom_lens[c]) { set_error("mask: bed line %llu: end past chromosome %s of %llu bases", (unsigned long long)no, chrom_ids[c], (unsigned long long)chrom_lens[c]); return SKX_EINVAL; }
        v.push_back(skx_mask_interval{SKX_MASK_ALL_SAMPLES, (uint32_t)c, (uint32_t)a, (uint32_t)(b - 1)});
    }
    return hand_over(v, out, n);
    });
}

extern "C" int skh_mask_text(const skx_mask_sample *samples, const skx_mask_info *info, const skx_mask_interval *iv, uint64_t n, const char *const *names, uint64_t n_samples,
                             char **buf, uint64_t *len)
{
    return guarded([&]() -> int {
    if (!buf || !len || !info || (n && !iv) || (n_samples && (!names || !samples))) { skx_set_last_error("skh_mask_text: bad arguments"); return SKX_EINVAL; }
    for (uint64_t i = 0; i < n; i++)
        if ((iv[i].sample != SKX_MASK_ALL_SAMPLES && iv[i].sample >= n_samples) || iv[i].start > iv[i].end) { skx_set_last_error("skh_mask_text: an interval names a sample that is not there, or ends before it starts"); return SKX_EINVAL; }
    const std::vector<Merged> mg = merge(iv, n);
    std::vector<uint64_t> count(n_samples + 1, 0), bases(n_samples + 1, 0);
    for (const Merged &m : mg) { const uint64_t s = m.sample == SKX_MASK_ALL_SAMPLES ? n_samples : m.sample; count[s]++; bases[s] += m.end - m.start + 1; }
    std::string out = "sample\tintervals\tinterval_bases\tsites_in_regions\tcells_masked\n";
    for (uint64_t s = 0; s < n_samples; s++) {
        out += names[s];
        put(out, "\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)count[s], (unsigned long long)bases[s], (unsigned long long)samples[s].sites_in_regions, (unsigned long long)samples[s].cells_masked);
    }
    put(out, "all_samples_intervals\t%llu\nall_samples_bases\t%llu\n", (unsigned long long)count[n_samples], (unsigned long long)bases[n_samples]);
    put(out, "sites\t%llu\nrows_in\t%llu\nrows_all_samples\t%llu\nrows_emptied\t%llu\nrows_out\t%llu\n", (unsigned long long)info->sites, (unsigned long long)info->rows_in,
        (unsigned long long)info->rows_all_samples, (unsigned long long)info->rows_emptied, (unsigned long long)info->rows_out);
    return to_buf(out, buf, len);
    });
}

extern "C" int skh_mask(skx_ctx *ctx, const char *reference_fasta, const char *skf_file, const char *out_file, const char *regions_file, int dense, uint64_t window,
                        uint32_t min_snps, const char *bed_file, const char *summary_prefix)
{
    return guarded([&]() -> int {
    if (!ctx || !reference_fasta || !skf_file || !out_file) { skx_set_last_error("skh_mask: bad arguments"); return SKX_EINVAL; }
    if (!regions_file && !dense && !bed_file) { skx_set_last_error("mask: one of a regions file, --dense and a BED file is required"); return SKX_EINVAL; }
    if (regions_file && dense) { skx_set_last_error("mask: a regions file and --dense exclude each other"); return SKX_EINVAL; }
    if (dense && (window < 1 || window > (1ull << 31))) { skx_set_last_error("mask: window must be between 1 and 2^31 (inclusive)"); return SKX_EINVAL; }
    if (dense && (min_snps < 2 || min_snps > 65535)) { skx_set_last_error("mask: min_snps must be between 2 and 65535 (inclusive)"); return SKX_EINVAL; }
    {   // the input is never overwritten: the name skh_save_skf will write must not be the input's
        std::string target = out_file;
        if (target.size() < 4 || target.compare(target.size() - 4, 4, ".skf") != 0) target += ".skf";
        char *ri = realpath(skf_file, nullptr), *ro = realpath(target.c_str(), nullptr);
        const bool same = target == skf_file || (ri && ro && strcmp(ri, ro) == 0);
        free(ri); free(ro);
        if (same) { set_error("mask: the output %s is the input file; the input is never overwritten", target.c_str()); return SKX_EINVAL; }
    }
    int rc;
    skx_array *a = nullptr;
    { Phase pl("mask.load"); const char *in[1] = {skf_file}; if ((rc = skh_load_array(ctx, in, 1, 1, &a)) != SKX_OK) return rc; }
    struct Free { skx_array *a; ~Free() { skx_array_free(a); } } free_a{a};
    skx_array_info_t ai; skx_array_info(a, &ai);
    const uint64_t S = ai.n_samples;
    std::vector<const char *> names(S);
    for (uint64_t s = 0; s < S; s++) names[s] = skx_array_name(a, s);
    std::vector<skx_mask_interval> iv;
    if (dense) {
        Phase pd("mask.density");
        skx_density_result r{};
        if ((rc = skx_array_snp_density(a, reference_fasta, window, min_snps, 0, &r)) != SKX_OK) return rc;
        for (uint64_t i = 0; i < r.info.n_regions; i++) iv.push_back(skx_mask_interval{r.regions[i].sample, r.regions[i].chrom, r.regions[i].start, r.regions[i].end});
        skx_free(r.samples); skx_free(r.regions); skx_free(r.bins); skx_free(r.chrom_ids); skx_free(r.chrom_lens); skx_free(r.snps); skx_free(r.snp_ref);
    }
    if (regions_file || bed_file) {
        Phase pr("mask.read_intervals");
        char *ids = nullptr; uint64_t *lens = nullptr, C = 0;
        if ((rc = skx_reference_records(reference_fasta, &ids, &lens, &C)) != SKX_OK) return rc;
        struct Mem { char *ids; uint64_t *lens; ~Mem() { skx_free(ids); skx_free(lens); } } mem{ids, lens};
        std::vector<const char *> id(C);
        { const char *p = ids; for (uint64_t c = 0; c < C; c++) { id[c] = p; p += strlen(p) + 1; } }
        for (int bed = 0; bed < 2; bed++) {
            const char *path = bed ? bed_file : regions_file;
            if (!path) continue;
            std::string text;
            if ((rc = read_file(path, text)) != SKX_OK) return rc;
            skx_mask_interval *got = nullptr; uint64_t n = 0;
            rc = bed ? skh_mask_read_bed(text.data(), text.size(), id.data(), lens, C, &got, &n)
                     : skh_mask_read_regions(text.data(), text.size(), names.data(), S, id.data(), lens, C, &got, &n);
            if (rc != SKX_OK) return rc;
            iv.insert(iv.end(), got, got + n);
            skx_free(got);
        }
    }
    std::vector<skx_mask_sample> samples(S ? S : 1);
    skx_mask_info info{};
    { Phase pk("mask.regions"); if ((rc = skx_array_mask_regions(a, reference_fasta, iv.data(), iv.size(), samples.data(), &info)) != SKX_OK) return rc; }
    { Phase ps("mask.save"); if ((rc = skh_save_skf(a, out_file)) != SKX_OK) return rc; }
    if (summary_prefix) {
        Phase pt("mask.text");
        char *buf = nullptr; uint64_t len = 0;
        if ((rc = skh_mask_text(samples.data(), &info, iv.data(), iv.size(), names.data(), S, &buf, &len)) != SKX_OK) return rc;
        rc = write_text_file(std::string(summary_prefix) + ".mask.summary.tsv", buf, len);
        skx_free(buf);
        if (rc != SKX_OK) return rc;
    }
    return SKX_OK;
    });
}
