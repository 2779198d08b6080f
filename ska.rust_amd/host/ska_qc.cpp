// ska_qc.cpp -- `ska qc`: per-sample quality counts and outlier flags from one load and one call of skx_array_sample_qc (host side above the C
// ABI).  The reference has no such mode: `ska nk` (lib.rs:808-827) prints one k-mer count per sample, and its users run `ska delete`
// (generic_modes.rs:192-210) and `ska nk` once per sample.  The flag rule and the three texts are stated in include/skx_host.h and, identically,
// in tests/qc_model.py.
#include "ska_host_util.h"
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

using namespace skh;
namespace {

constexpr int N_METRICS = 6;
const char *const METRIC_NAMES[N_METRICS] = {"kmers", "ambiguous", "singletons", "core_missing", "private_alleles", "minor_alleles"};
enum { LOW = 1, HIGH = 2 };

uint64_t metric(const skx_qc_sample &s, const skx_qc_info &info, int m)
{
    switch (m) {
    case 0: return s.kmers;
    case 1: return s.ambiguous;
    case 2: return s.singletons;
    case 3: return info.core_rows > s.core_present ? info.core_rows - s.core_present : 0;
    case 4: return s.private_alleles;
    default: return s.minor_alleles;
    }
}

struct Metric {
    std::vector<uint64_t> x; std::vector<uint8_t> side;            // per sample: its value, LOW / HIGH / 0
    uint64_t min = 0, med = 0, max = 0, mad = 0, flagged = 0;
};

// integers and one double product: med and mad are place (S - 1) / 2 of the sorted values and of the sorted |x - med|, d = max(mad, 1)
Metric measure(const skx_qc_sample *samples, uint64_t S, const skx_qc_info &info, int m, double M)
{
    Metric r;
    r.x.resize(S); r.side.assign(S, 0);
    for (uint64_t s = 0; s < S; s++) r.x[s] = metric(samples[s], info, m);
    if (!S) return r;
    std::vector<uint64_t> v(r.x);
    std::sort(v.begin(), v.end());
    r.min = v.front(); r.max = v.back(); r.med = v[(S - 1) / 2];
    for (uint64_t s = 0; s < S; s++) v[s] = r.x[s] > r.med ? r.x[s] - r.med : r.med - r.x[s];
    std::sort(v.begin(), v.end());
    r.mad = v[(S - 1) / 2];
    const double bound = M * (double)std::max<uint64_t>(r.mad, 1);
    for (uint64_t s = 0; s < S; s++) {
        if (r.x[s] > r.med && (double)(r.x[s] - r.med) > bound) r.side[s] = HIGH;
        else if (m == 0 && r.x[s] < r.med && (double)(r.med - r.x[s]) > bound) r.side[s] = LOW;      // kmers alone is flagged on both sides
        r.flagged += r.side[s] != 0;
    }
    return r;
}

std::string flags_of(const Metric *ms, uint64_t s)
{
    std::string f;
    auto add = [&](const char *w) { if (!f.empty()) f += ','; f += w; };
    if (ms[0].side[s] == LOW) add("low_kmers");
    if (ms[0].side[s] == HIGH) add("high_kmers");
    for (int m = 1; m < N_METRICS; m++) if (ms[m].side[s]) add(METRIC_NAMES[m]);
    return f;
}

}  // namespace

extern "C" int skh_qc_text(int which, const skx_qc_sample *samples, const char *const *names, uint64_t n_samples, const skx_qc_info *info, double mad,
                           char **buf, uint64_t *len)
{
    return guarded([&]() -> int {
    if (!buf || !len || !info || (n_samples && (!samples || !names)) || which < SKH_QC_SAMPLES || which > SKH_QC_FLAGGED) { skx_set_last_error("skh_qc_text: bad arguments"); return SKX_EINVAL; }
    if (!(mad >= 0.0)) { skx_set_last_error("skh_qc_text: mad must be zero or higher"); return SKX_EINVAL; }
    const uint64_t S = n_samples;
    Metric ms[N_METRICS];
    for (int m = 0; m < N_METRICS; m++) ms[m] = measure(samples, S, *info, m, mad);
    std::string out;
    if (which == SKH_QC_SAMPLES) {
        out = "sample\tkmers\tambiguous\tsingletons\tcore_present\tcore_missing\tprivate_alleles\tminor_alleles\tflags\n";
        for (uint64_t s = 0; s < S; s++) {
            const skx_qc_sample &q = samples[s];
            const std::string f = flags_of(ms, s);
            out += names[s];
            put(out, "\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t", (unsigned long long)q.kmers, (unsigned long long)q.ambiguous, (unsigned long long)q.singletons,
                (unsigned long long)q.core_present, (unsigned long long)ms[3].x[s], (unsigned long long)q.private_alleles, (unsigned long long)q.minor_alleles);
            out += f.empty() ? "-" : f;
            out += '\n';
        }
    } else if (which == SKH_QC_SUMMARY) {
        put(out, "samples\t%llu\nrows\t%llu\nrows_present\t%llu\ncore_rows\t%llu\ncore_variant_rows\t%llu\nthreshold\t%llu\n", (unsigned long long)S,
            (unsigned long long)info->rows, (unsigned long long)info->rows_present, (unsigned long long)info->core_rows, (unsigned long long)info->core_variant_rows,
            (unsigned long long)info->threshold);
        out += "metric\tmin\tmedian\tmax\tmad\tflagged\n";
        for (int m = 0; m < N_METRICS; m++) {
            out += METRIC_NAMES[m];
            put(out, "\t%llu\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)ms[m].min, (unsigned long long)ms[m].med, (unsigned long long)ms[m].max,
                (unsigned long long)ms[m].mad, (unsigned long long)ms[m].flagged);
        }
    } else {
        for (uint64_t s = 0; s < S; s++) if (!flags_of(ms, s).empty()) { out += names[s]; out += '\n'; }
    }
    return to_buf(out, buf, len);
    });
}

extern "C" int skh_qc(skx_ctx *ctx, const char *skf_file, const char *out_prefix, double min_freq, double mad)
{
    return guarded([&]() -> int {
    if (!ctx || !skf_file || !out_prefix) { skx_set_last_error("skh_qc: bad arguments"); return SKX_EINVAL; }
    if (!(min_freq >= 0.0 && min_freq <= 1.0)) { skx_set_last_error("qc: min_freq must be between 0 and 1 (inclusive)"); return SKX_EINVAL; }
    if (!(mad >= 0.0)) { skx_set_last_error("qc: mad must be zero or higher"); return SKX_EINVAL; }
    int r;
    skx_array *a = nullptr;
    { Phase pl("qc.load"); const char *in[1] = {skf_file}; if ((r = skh_load_array(ctx, in, 1, 1, &a)) != SKX_OK) return r; }
    struct Free { skx_array *a; ~Free() { skx_array_free(a); } } free_a{a};
    skx_array_info_t ai; skx_array_info(a, &ai);
    const uint64_t S = ai.n_samples;
    std::vector<skx_qc_sample> samples(S ? S : 1);
    skx_qc_info info{};
    { Phase pk("qc.kernels"); if ((r = skx_array_sample_qc(a, min_freq, samples.data(), &info)) != SKX_OK) return r; }
    Phase pt("qc.text");
    std::vector<const char *> names(S);
    for (uint64_t s = 0; s < S; s++) names[s] = skx_array_name(a, s);
    const char *const suffix[3] = {".qc.tsv", ".qc.summary.tsv", ".qc.flagged.txt"};
    for (int which = SKH_QC_SAMPLES; which <= SKH_QC_FLAGGED; which++) {
        char *buf = nullptr; uint64_t len = 0;
        if ((r = skh_qc_text(which, samples.data(), names.data(), S, &info, mad, &buf, &len)) != SKX_OK) return r;
        r = write_text_file(std::string(out_prefix) + suffix[which], buf, len);
        skx_free(buf);
        if (r != SKX_OK) return r;
    }
    return SKX_OK;
    });
}
