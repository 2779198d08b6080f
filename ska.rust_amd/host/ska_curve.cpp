// ska_curve.cpp -- `ska curve`: pan, core, variant and core-variant counts after each sample of an order has been added, over seeded shuffles or
// one order from a file, from one load and one call of skx_array_curve (host side above the C ABI).  The reference has no such mode: `ska nk`
// (lib.rs:808-827) prints one number for the whole file, and its users run `ska delete` (generic_modes.rs:192-210) and `ska align` per prefix.
#include "ska_host_util.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <numeric>
#include <string>
#include <vector>

using namespace skh;
namespace {

struct SplitMix64 {
    uint64_t state;
    uint64_t next()
    {
        uint64_t z = (state += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    // j from [0, n) without modulo bias: draws at or above the largest multiple of n that 2^64 holds are thrown away
    uint64_t below(uint64_t n)
    {
        const uint64_t excess = (0 - n) % n;                      // 2^64 mod n
        for (;;) { const uint64_t x = next(); if (excess == 0 || x < 0 - excess) return x % n; }
    }
};

const char *const COUNT_NAMES[4] = {"pan", "core", "variant", "core_variant"};

}  // namespace

extern "C" int skh_curve_orders(uint64_t seed, uint32_t n_samples, uint32_t n_orders, int32_t *orders)
{
    if (!orders && n_samples && n_orders) { skx_set_last_error("skh_curve_orders: bad arguments"); return SKX_EINVAL; }
    SplitMix64 g{seed};
    for (uint32_t p = 0; p < n_orders; p++) {
        int32_t *o = orders + (uint64_t)p * n_samples;
        std::iota(o, o + n_samples, 0);
        for (uint64_t i = n_samples; i-- > 1;) std::swap(o[i], o[g.below(i + 1)]);
    }
    return SKX_OK;
}

extern "C" int skh_curve_tsv(const uint64_t *counts, uint32_t n_orders, uint32_t n_samples, char **buf, uint64_t *len)
{
    return guarded([&]() -> int {
    if (!counts || !buf || !len || n_orders == 0) { skx_set_last_error("skh_curve_tsv: bad arguments"); return SKX_EINVAL; }
    const uint64_t P = n_orders, S = n_samples;
    std::string out = "t";
    for (const char *c : COUNT_NAMES) for (const char *w : {"min", "median", "max", "mean"}) { out += '\t'; out += c; out += '_'; out += w; }
    out += '\n';
    std::vector<uint64_t> v(P);
    for (uint64_t t = 0; t < S; t++) {
        put(out, "%llu", (unsigned long long)(t + 1));
        for (int c = 0; c < 4; c++) {
            unsigned __int128 sum = 0;
            for (uint64_t p = 0; p < P; p++) { v[p] = counts[(p * S + t) * 4 + c]; sum += v[p]; }
            std::sort(v.begin(), v.end());
            const unsigned __int128 q = (sum * 1000 + P / 2) / P;                         // the mean in thousandths, rounded half up
            put(out, "\t%llu\t%llu\t%llu\t%llu.%03u", (unsigned long long)v[0], (unsigned long long)v[(P - 1) / 2], (unsigned long long)v[P - 1],
                (unsigned long long)(q / 1000), (unsigned)(q % 1000));
        }
        out += '\n';
    }
    return to_buf(out, buf, len);
    });
}

extern "C" int skh_curve(skx_ctx *ctx, const char *skf_file, const char *out_prefix, uint32_t n_permutations, uint64_t seed, double min_freq,
                         const char *order_file, int all_permutations)
{
    return guarded([&]() -> int {
    if (!ctx || !skf_file || !out_prefix || (!order_file && (n_permutations < 1 || n_permutations > 10000))) { skx_set_last_error("skh_curve: bad arguments"); return SKX_EINVAL; }
    std::vector<std::string> wanted;
    if (order_file) {
        std::ifstream in(order_file);
        if (!in) { set_error("order file %s: cannot be read", order_file); return SKX_EIO; }
        std::string line;
        while (std::getline(in, line)) {
            if (!line.empty() && line.back() == '\r') line.pop_back();
            if (!line.empty()) wanted.push_back(line);
        }
    }
    int r;
    skx_array *a = nullptr;
    { Phase pl("curve.load"); const char *in[1] = {skf_file}; if ((r = skh_load_array(ctx, in, 1, 1, &a)) != SKX_OK) return r; }
    struct Free { skx_array *a; ~Free() { skx_array_free(a); } } free_a{a};
    skx_array_info_t info; skx_array_info(a, &info);
    const uint64_t S = info.n_samples;
    const uint32_t P = order_file ? 1 : n_permutations;
    std::vector<int32_t> orders((size_t)P * S);
    {
        Phase po("curve.orders");
        if (order_file) {
            // names -> samples as skx_array_delete_samples finds them: the first sample of that name not taken yet (merge_ska_array.rs:243-249)
            std::vector<char> taken(S, 0);
            for (size_t i = 0; i < wanted.size(); i++) {
                bool found = false, known = false;
                for (uint64_t s = 0; s < S && !found; s++)
                    if (wanted[i] == skx_array_name(a, s)) { known = true; if (!taken[s]) { taken[s] = 1; found = true; if (i < S) orders[i] = (int32_t)s; } }
                if (!found && known) { set_error("order file %s: sample %s is listed twice", order_file, wanted[i].c_str()); return SKX_EINVAL; }
                if (!found) { set_error("order file %s: sample %s is not in %s", order_file, wanted[i].c_str(), skf_file); return SKX_EINVAL; }
            }
            for (uint64_t s = 0; s < S; s++) if (!taken[s]) { set_error("order file %s: sample %s is missing", order_file, skx_array_name(a, s)); return SKX_EINVAL; }
        } else if ((r = skh_curve_orders(seed, (uint32_t)S, P, orders.data())) != SKX_OK) return r;
    }
    std::vector<uint64_t> counts((size_t)P * S * 4);
    { Phase pk("curve.kernel"); if ((r = skx_array_curve(a, orders.data(), P, min_freq, counts.data())) != SKX_OK) return r; }

    Phase pt("curve.text");
    char *buf = nullptr; uint64_t len = 0;
    if ((r = skh_curve_tsv(counts.data(), P, (uint32_t)S, &buf, &len)) != SKX_OK) return r;
    r = write_text_file(std::string(out_prefix) + ".curve.tsv", buf, len);
    skx_free(buf);
    if (r != SKX_OK || !(all_permutations || order_file)) return r;
    std::string text = "permutation\tt\tsample\tpan\tcore\tvariant\tcore_variant\tnew\n";
    for (uint64_t p = 0; p < P; p++) {
        uint64_t before = 0;
        for (uint64_t t = 0; t < S; t++) {
            const uint64_t *c = &counts[(p * S + t) * 4];
            put(text, "%llu\t%llu\t", (unsigned long long)p, (unsigned long long)(t + 1));
            text += skx_array_name(a, orders[p * S + t]);
            put(text, "\t%llu\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2], (unsigned long long)c[3],
                (unsigned long long)(c[0] - before));
            before = c[0];
        }
    }
    return write_text_file(std::string(out_prefix) + ".curve.permutations.tsv", text.data(), text.size());
    });
}
