// ska_screen.cpp -- `ska screen`: per-sample coverage and identity of the records of a sequence panel, from one load and one call of
// skx_array_screen (host side above the C ABI): which pairs pass, and the three texts.  The reference has no such mode: its users run
// `ska map` on the panel (generic_modes.rs:56-84) and count columns, or `ska weed --reverse` (lib.rs:760-806) and `ska nk` once per record.
#include "ska_host_util.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace skh;
namespace {

// windows > 0, found >= max(1, ceil(C * windows)), match >= ceil(I * found): the products in doubles
bool passes(const skx_screen_record &r, const skx_screen_cell &c, double min_cover, double min_identity)
{
    if (r.windows == 0) return false;
    const uint64_t need = std::max<uint64_t>(1, (uint64_t)std::ceil(min_cover * (double)r.windows));
    return c.found >= need && c.match >= (uint64_t)std::ceil(min_identity * (double)c.found);
}

}  // namespace

extern "C" int skh_screen_text(int which, uint64_t n_records, const skx_screen_record *records, const char *ids, const skx_screen_cell *cells,
                               const char *const *names, uint64_t n_samples, double min_cover, double min_identity, char **buf, uint64_t *len)
{
    return guarded([&]() -> int {
    if (!buf || !len || which < SKH_SCREEN_PAIRS || which > SKH_SCREEN_MATRIX || (n_records && (!records || !ids)) || (n_records && n_samples && !cells) || (n_samples && !names)) {
        skx_set_last_error("skh_screen_text: bad arguments"); return SKX_EINVAL;
    }
    if (!(min_cover >= 0.0 && min_cover <= 1.0) || !(min_identity >= 0.0 && min_identity <= 1.0)) { skx_set_last_error("skh_screen_text: cover and identity must be between 0 and 1 (inclusive)"); return SKX_EINVAL; }
    const uint64_t R = n_records, S = n_samples;
    std::vector<const char *> id(R);
    { const char *p = ids; for (uint64_t r = 0; r < R; r++) { id[r] = p; p += strlen(p) + 1; } }
    if (which == SKH_SCREEN_PAIRS)
        return format_rows("record\tlength\twindows\tsample\tfound\tmatch\tambig\tsnp\tcover\tidentity\n", R, [&](uint64_t r, std::string &out) {
            const skx_screen_record &rec = records[r];
            for (uint64_t s = 0; s < S; s++) {
                const skx_screen_cell &c = cells[r * S + s];
                if (!passes(rec, c, min_cover, min_identity)) continue;
                out += id[r];
                put(out, "\t%llu\t%llu\t", (unsigned long long)rec.length, (unsigned long long)rec.windows);
                out += names[s];
                put(out, "\t%u\t%u\t%u\t%u\t%.4f\t%.4f\n", c.found, c.match, c.ambig, c.found - c.match - c.ambig, (double)c.found / (double)rec.windows,
                    (double)c.match / (double)c.found);
            }
        }, buf, len);
    if (which == SKH_SCREEN_SUMMARY)
        return format_rows("record\tlength\twindows\trows_hit\tsamples_passing\n", R, [&](uint64_t r, std::string &out) {
            const skx_screen_record &rec = records[r];
            uint64_t n = 0;
            for (uint64_t s = 0; s < S; s++) n += passes(rec, cells[r * S + s], min_cover, min_identity);
            out += id[r];
            put(out, "\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)rec.length, (unsigned long long)rec.windows, (unsigned long long)rec.rows_hit, (unsigned long long)n);
        }, buf, len);
    std::string header = "record";
    for (uint64_t s = 0; s < S; s++) { header += '\t'; header += names[s]; }
    header += '\n';
    return format_rows(header.c_str(), R, [&](uint64_t r, std::string &out) {
        out += id[r];
        for (uint64_t s = 0; s < S; s++) { out += '\t'; out += passes(records[r], cells[r * S + s], min_cover, min_identity) ? '1' : '0'; }
        out += '\n';
    }, buf, len);
    });
}

extern "C" int skh_screen(skx_ctx *ctx, const char *skf_file, const char *panel_fasta, const char *out_prefix, double min_cover, double min_identity, int matrix)
{
    return guarded([&]() -> int {
    if (!ctx || !skf_file || !panel_fasta || !out_prefix) { skx_set_last_error("skh_screen: bad arguments"); return SKX_EINVAL; }
    if (!(min_cover >= 0.0 && min_cover <= 1.0) || !(min_identity >= 0.0 && min_identity <= 1.0)) { skx_set_last_error("skh_screen: cover and identity must be between 0 and 1 (inclusive)"); return SKX_EINVAL; }
    int r;
    skx_array *a = nullptr;
    { Phase pl("screen.load"); const char *in[1] = {skf_file}; if ((r = skh_load_array(ctx, in, 1, 1, &a)) != SKX_OK) return r; }
    struct Free { skx_array *a; ~Free() { skx_array_free(a); } } free_a{a};
    skx_array_info_t info; skx_array_info(a, &info);
    const uint64_t S = info.n_samples;
    uint64_t R = 0; skx_screen_record *records = nullptr; char *ids = nullptr; skx_screen_cell *cells = nullptr;
    { Phase pc("screen.counts"); if ((r = skx_array_screen(a, panel_fasta, &R, &records, &ids, &cells)) != SKX_OK) return r; }
    struct Mem { void *p[3]; ~Mem() { for (void *q : p) skx_free(q); } } mem{{records, ids, cells}};
    std::vector<const char *> names(S);
    for (uint64_t s = 0; s < S; s++) names[s] = skx_array_name(a, s);

    Phase pt("screen.text");
    static const char *const SUFFIX[3] = {".screen.tsv", ".screen.summary.tsv", ".screen.matrix.tsv"};
    for (int which = SKH_SCREEN_PAIRS; which <= (matrix ? SKH_SCREEN_MATRIX : SKH_SCREEN_SUMMARY); which++) {
        char *buf = nullptr; uint64_t len = 0;
        if ((r = skh_screen_text(which, R, records, ids, cells, names.data(), S, min_cover, min_identity, &buf, &len)) != SKX_OK) return r;
        r = write_text_file(std::string(out_prefix) + SUFFIX[which], buf, len);
        skx_free(buf);
        if (r != SKX_OK) return r;
    }
    return SKX_OK;
    });
}
