// ska_density.cpp -- `ska density`: dense-SNP regions per sample along a reference, from one load and one call of skx_array_snp_density (host
// side above the C ABI): the four texts and the masked alignment.  The reference has no such mode: its users write `ska map`'s alignment
// (generic_modes.rs:56-84) and run a separate tool over it.  The texts are stated in include/skx_host.h and, identically, in
// tests/density_model.py.
#include "ska_host_util.h"
#include <string>
#include <vector>

using namespace skh;
namespace {

std::vector<const char *> chrom_ids(const skx_density_result &r)
{
    std::vector<const char *> id(r.info.n_chrom);
    const char *p = r.chrom_ids;
    for (uint64_t c = 0; c < r.info.n_chrom; c++) { id[c] = p; p += strlen(p) + 1; }
    return id;
}

bool bad_result(const skx_density_result *r)
{
    const skx_density_info &i = r->info;
    return (i.n_chrom && (!r->chrom_ids || !r->chrom_lens)) || (i.n_regions && !r->regions) || (i.n_bins && !r->bins);
}

}  // namespace

extern "C" int skh_density_text(int which, const skx_density_result *r, const char *const *names, uint64_t n_samples, uint64_t window, char **buf, uint64_t *len)
{
    return guarded([&]() -> int {
    if (!buf || !len || !r || which < SKH_DENSITY_REGIONS || which > SKH_DENSITY_SNPS || (n_samples && (!names || !r->samples)) || bad_result(r)) {
        skx_set_last_error("skh_density_text: bad arguments"); return SKX_EINVAL;
    }
    if (window < 1) { skx_set_last_error("skh_density_text: window must be one or higher"); return SKX_EINVAL; }
    const uint64_t S = n_samples, C = r->info.n_chrom;
    const std::vector<const char *> id = chrom_ids(*r);
    if (which == SKH_DENSITY_REGIONS) {
        for (uint64_t i = 0; i < r->info.n_regions; i++)
            if (r->regions[i].sample >= S || r->regions[i].chrom >= C) { skx_set_last_error("skh_density_text: a region names a sample or a chromosome that is not there"); return SKX_EINVAL; }
        return format_slices("sample\tchromosome\tstart\tend\tlength\tsnps\n", r->info.n_regions, [&](uint64_t i, std::string &out) {
            const skx_density_region &g = r->regions[i];
            out += names[g.sample]; out += '\t'; out += id[g.chrom];
            put(out, "\t%llu\t%llu\t%llu\t%u\n", (unsigned long long)g.start + 1, (unsigned long long)g.end + 1, (unsigned long long)g.end - g.start + 1, g.snps);
        }, buf, len);
    }
    if (which == SKH_DENSITY_SUMMARY)
        return format_rows("sample\tsites\tcallable\tambiguous\tmissing\tsnps\tdense_snps\tregions\tregion_bases\tsnps_outside\n", S, [&](uint64_t s, std::string &out) {
            const skx_density_sample &q = r->samples[s];
            out += names[s];
            put(out, "\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)q.sites, (unsigned long long)q.callable, (unsigned long long)q.ambiguous,
                (unsigned long long)q.missing, (unsigned long long)q.snps, (unsigned long long)q.dense_snps, (unsigned long long)q.regions, (unsigned long long)q.region_bases,
                (unsigned long long)(q.snps - q.dense_snps));
        }, buf, len);
    if (which == SKH_DENSITY_BINS) {
        // bin -> its chromosome: the bins lie chromosome after chromosome, ceil(len / W) each
        std::vector<uint64_t> first(C + 1, 0);
        for (uint64_t c = 0; c < C; c++) first[c + 1] = first[c] + (r->chrom_lens[c] + window - 1) / window;
        if (first[C] != r->info.n_bins) { skx_set_last_error("skh_density_text: the bins are not those of this window"); return SKX_EINVAL; }
        return format_slices("chromosome\tstart\tend\tsnps\tdense_snps\n", r->info.n_bins, [&](uint64_t b, std::string &out) {
            const uint64_t c = (uint64_t)(std::upper_bound(first.begin(), first.end(), b) - first.begin()) - 1, at = (b - first[c]) * window;
            out += id[c];
            put(out, "\t%llu\t%llu\t%u\t%u\n", (unsigned long long)at + 1, (unsigned long long)std::min(at + window, r->chrom_lens[c]), r->bins[b].snps, r->bins[b].dense_snps);
        }, buf, len);
    }
    if (r->info.n_snps && (!r->snps || !r->snp_ref)) { skx_set_last_error("skh_density_text: the SNP list was not asked for"); return SKX_EINVAL; }
    std::vector<uint64_t> off(C + 1, 0);
    for (uint64_t c = 0; c < C; c++) off[c + 1] = off[c] + r->chrom_lens[c];
    for (uint64_t i = 0; i < r->info.n_snps; i++)
        if (((r->snps[i] >> 34) & 0xFFFFFFFull) >= S || ((r->snps[i] >> 2) & 0xFFFFFFFFull) >= off[C]) { skx_set_last_error("skh_density_text: a SNP names a sample or a position that is not there"); return SKX_EINVAL; }
    return format_slices("sample\tchromosome\tposition\tref\talt\tdense\n", r->info.n_snps, [&](uint64_t i, std::string &out) {
        const uint64_t v = r->snps[i], s = (v >> 34) & 0xFFFFFFFull, x = (v >> 2) & 0xFFFFFFFFull;
        const uint64_t c = (uint64_t)(std::upper_bound(off.begin(), off.begin() + (ptrdiff_t)C, x) - off.begin()) - 1;
        out += names[s]; out += '\t'; out += id[c];
        put(out, "\t%llu\t%c\t%c\t%d\n", (unsigned long long)(x - off[c]) + 1, (char)r->snp_ref[i], "ACTG"[v & 3], (int)((v >> SKX_DENSITY_DENSE_BIT) & 1));
    }, buf, len);
    });
}

extern "C" int skh_density_mask_alignment(char *aln, uint64_t len, const skx_density_result *r, const char *const *names, uint64_t n_samples)
{
    return guarded([&]() -> int {
    if (!r || (len && !aln) || (n_samples && !names) || bad_result(r)) { skx_set_last_error("skh_density_mask_alignment: bad arguments"); return SKX_EINVAL; }
    const uint64_t S = n_samples, C = r->info.n_chrom;
    std::vector<uint64_t> off(C + 1, 0);
    for (uint64_t c = 0; c < C; c++) off[c + 1] = off[c] + r->chrom_lens[c];
    // sample s: '>' name '\n', then off[C] letters and '\n'
    std::vector<uint64_t> line(S);
    uint64_t at = 0;
    for (uint64_t s = 0; s < S; s++) { at += 1 + strlen(names[s]) + 1; line[s] = at; at += off[C] + 1; }
    if (at != len) { skx_set_last_error("skh_density_mask_alignment: the text is not the alignment of these samples on this reference"); return SKX_EINVAL; }
    for (uint64_t i = 0; i < r->info.n_regions; i++) {               // (nothing is written before every region is known to fit)
        const skx_density_region &g = r->regions[i];
        if (g.sample >= S || g.chrom >= C || g.start > g.end || g.end >= r->chrom_lens[g.chrom]) { skx_set_last_error("skh_density_mask_alignment: a region lies outside the alignment"); return SKX_EINVAL; }
    }
    for (uint64_t i = 0; i < r->info.n_regions; i++) {
        const skx_density_region &g = r->regions[i];
        char *p = aln + line[g.sample] + off[g.chrom];
        for (uint64_t x = g.start; x <= g.end; x++) if (p[x] != '-') p[x] = 'N';
    }
    return SKX_OK;
    });
}

extern "C" int skh_density(skx_ctx *ctx, const char *reference_fasta, const char *skf_file, const char *out_prefix, uint64_t window, uint32_t min_snps, int snps, const char *masked_aln)
{
    return guarded([&]() -> int {
    if (!ctx || !reference_fasta || !skf_file || !out_prefix) { skx_set_last_error("skh_density: bad arguments"); return SKX_EINVAL; }
    if (window < 1 || window > (1ull << 31)) { skx_set_last_error("density: window must be between 1 and 2^31 (inclusive)"); return SKX_EINVAL; }
    if (min_snps < 2 || min_snps > 65535) { skx_set_last_error("density: min_snps must be between 2 and 65535 (inclusive)"); return SKX_EINVAL; }
    int rc;
    skx_array *a = nullptr;
    { Phase pl("density.load"); const char *in[1] = {skf_file}; if ((rc = skh_load_array(ctx, in, 1, 1, &a)) != SKX_OK) return rc; }
    struct Free { skx_array *a; ~Free() { skx_array_free(a); } } free_a{a};
    skx_array_info_t ai; skx_array_info(a, &ai);
    const uint64_t S = ai.n_samples;
    skx_density_result r{};
    { Phase pk("density.kernels"); if ((rc = skx_array_snp_density(a, reference_fasta, window, min_snps, snps ? SKX_DENSITY_WANT_SNPS : 0, &r)) != SKX_OK) return rc; }
    struct Mem { skx_density_result *r; ~Mem() { skx_free(r->samples); skx_free(r->regions); skx_free(r->bins); skx_free(r->chrom_ids); skx_free(r->chrom_lens); skx_free(r->snps); skx_free(r->snp_ref); } } mem{&r};
    std::vector<const char *> names(S);
    for (uint64_t s = 0; s < S; s++) names[s] = skx_array_name(a, s);
    {
        Phase pt("density.text");
        static const char *const SUFFIX[4] = {".density.regions.tsv", ".density.summary.tsv", ".density.bins.tsv", ".density.snps.tsv"};
        for (int which = SKH_DENSITY_REGIONS; which <= (snps ? SKH_DENSITY_SNPS : SKH_DENSITY_BINS); which++) {
            char *buf = nullptr; uint64_t len = 0;
            if ((rc = skh_density_text(which, &r, names.data(), S, window, &buf, &len)) != SKX_OK) return rc;
            rc = write_text_file(std::string(out_prefix) + SUFFIX[which], buf, len);
            skx_free(buf);
            if (rc != SKX_OK) return rc;
        }
    }
    if (masked_aln) {
        Phase pm("density.masked_aln");
        char *buf = nullptr; uint64_t len = 0;
        if ((rc = skx_array_map(a, reference_fasta, 0, 1, 0, 1, &buf, &len)) != SKX_OK) return rc;
        rc = skh_density_mask_alignment(buf, len, &r, names.data(), S);
        if (rc == SKX_OK) rc = write_text_file(masked_aln, buf, len);
        skx_free(buf);
        if (rc != SKX_OK) return rc;
    }
    return SKX_OK;
    });
}
