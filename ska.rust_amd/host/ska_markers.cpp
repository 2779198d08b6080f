// ska_markers.cpp -- `ska markers`: the split k-mers and middle-base alleles that tell each group of a groups file from everybody else, from one
// load and one call of skx_array_group_markers (host side above the C ABI).  The reference has no such mode: its users run `ska delete` of a
// group's samples (generic_modes.rs:192-210) and `ska nk --full-info` (lib.rs:808-827) per group and compare the text.
#include "ska_host_util.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

using namespace skh;
namespace {

int write_file(const std::string &path, const std::string &text)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) { set_error("cannot create output file %s", path.c_str()); return SKX_EIO; }
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    if (fclose(f) != 0 || !ok) { set_error("write failed: %s", path.c_str()); return SKX_EIO; }
    return SKX_OK;
}

const char IUPAC[] = "-ACMTWYHGRSVKDBN";       // the letter of a 4-bit base set (A 1, C 2, T 4, G 8)

}  // namespace

extern "C" void skh_key_arms(const skx_key *key, int k, char *upper, char *lower)
{
    static const char L[] = "ACTG";
    const int half = (k - 1) / 2;
    unsigned __int128 w = ((unsigned __int128)key->hi << 64) | key->lo;
    for (int b = 0; b < half; b++) { lower[half - 1 - b] = L[(int)(w & 3)]; w >>= 2; }
    for (int b = 0; b < half; b++) { upper[half - 1 - b] = L[(int)(w & 3)]; w >>= 2; }
    upper[half] = lower[half] = 0;
}

extern "C" int skh_markers(skx_ctx *ctx, const char *skf_file, const char *groups_file, const char *out_prefix, double min_in, double max_out,
                           int min_group_size, int kinds, int fasta)
{
    return guarded([&]() -> int {
    if (!ctx || !skf_file || !groups_file || !out_prefix || min_group_size < 1) { skx_set_last_error("skh_markers: bad arguments"); return SKX_EINVAL; }
    struct Group { std::string label; std::vector<std::string> names; };
    std::vector<Group> groups;
    int r;
    {
        char *buf = nullptr; uint64_t len = 0, n_pairs = 0;
        if ((r = skh_read_groups(groups_file, &buf, &len, &n_pairs)) != SKX_OK) return r;
        const char *p = buf;
        for (uint64_t i = 0; i < n_pairs; i++) {                                                      // "name\0label\0", group by group
            const std::string name(p); p += name.size() + 1;
            const std::string label(p); p += label.size() + 1;
            if (groups.empty() || groups.back().label != label) { groups.emplace_back(); groups.back().label = label; }
            groups.back().names.push_back(name);
        }
        skx_free(buf);
    }
    skx_array *a = nullptr;
    { Phase pl("markers.load"); const char *in[1] = {skf_file}; if ((r = skh_load_array(ctx, in, 1, 1, &a)) != SKX_OK) return r; }
    struct Free { skx_array *a; ~Free() { skx_array_free(a); } } free_a{a};
    skx_array_info_t info; skx_array_info(a, &info);
    const uint64_t S = info.n_samples;
    const int G = (int)groups.size();
    // names -> samples as skx_array_delete_samples finds them: first match wins (merge_ska_array.rs:243-249)
    std::vector<int32_t> segment_of(S, G);
    std::vector<char> taken(S, 0);
    std::vector<uint64_t> size(G, 0);
    for (int g = 0; g < G; g++)
        for (auto &w : groups[g].names) {
            bool found = false;
            for (uint64_t s = 0; s < S && !found; s++)
                if (!taken[s] && w == skx_array_name(a, s)) { taken[s] = 1; segment_of[s] = g; size[g]++; found = true; }
            if (!found) { set_error("Could not find sample(s): {\"%s\"}", w.c_str()); return SKX_EINVAL; }        // :252-254
        }
    std::vector<uint8_t> reported(std::max(G, 1), 0);
    for (int g = 0; g < G; g++) reported[g] = size[g] >= (uint64_t)min_group_size;
    std::vector<skx_marker_info> counts(std::max(G, 1));
    skx_marker *rec = nullptr; skx_key *keys = nullptr; uint64_t n = 0;
    { Phase pp("markers.pass"); if ((r = skx_array_group_markers(a, segment_of.data(), G, reported.data(), min_in, max_out, kinds, &rec, &keys, &n, counts.data())) != SKX_OK) return r; }
    struct FreeRec { skx_marker *r; skx_key *k; ~FreeRec() { skx_free(r); skx_free(k); } } free_rec{rec, keys};

    Phase pt("markers.text");
    static const char L[] = "ACTG";
    std::string tsv = "Group\tUpper\tLower\tKind\tIn\tOut\tBases\tOther bases\n", summary = "Group\tSamples\tPresence\tAllele\n";
    char line[256];
    uint64_t at = 0;
    for (int g = 0; g < G; g++) {
        const std::string &label = groups[g].label;
        if (!reported[g]) { snprintf(line, sizeof line, "\t%llu\t-\t-\n", (unsigned long long)size[g]); summary += label; summary += line; continue; }
        snprintf(line, sizeof line, "\t%llu\t%llu\t%llu\n", (unsigned long long)size[g], (unsigned long long)counts[g].presence, (unsigned long long)counts[g].allele);
        summary += label; summary += line;
        uint64_t end = at;
        while (end < n && rec[end].group == (uint32_t)g) end++;
        // within a group: the order `ska nk --full-info` prints the rows in, i.e. ascending split k-mer
        std::vector<uint64_t> idx(end - at); std::iota(idx.begin(), idx.end(), at);
        std::sort(idx.begin(), idx.end(), [&](uint64_t x, uint64_t y) { return keys[x].hi != keys[y].hi ? keys[x].hi < keys[y].hi : keys[x].lo < keys[y].lo; });
        std::string fa;
        uint64_t i = 0;
        for (uint64_t j : idx) {
            char up[32], lo[32];
            skh_key_arms(&keys[j], info.k, up, lo);
            const char *kind = rec[j].kind == SKX_MARKER_PRESENCE ? "presence" : "allele";
            const char bases = IUPAC[rec[j].bases_in & 15], other = IUPAC[rec[j].bases_out & 15];
            snprintf(line, sizeof line, "\t%s\t%u/%llu\t%u/%llu\t%c\t%c\n", kind, rec[j].n_in, (unsigned long long)size[g], rec[j].n_out,
                     (unsigned long long)(S - size[g]), bases, other);
            tsv += label; tsv += '\t'; tsv += up; tsv += '\t'; tsv += lo; tsv += line;
            if (fasta) {
                // one N behind the k bases: a record of exactly k bases gives the reference's reader no split k-mer, and an N adds none
                char mid = 'N';
                for (const char *c = "ACGT"; *c; c++) if ((rec[j].bases_in >> (strchr(L, *c) - L)) & 1) { mid = *c; break; }
                snprintf(line, sizeof line, "_%llu kind=%s in=%u/%llu out=%u/%llu bases=%c\n", (unsigned long long)++i, kind, rec[j].n_in, (unsigned long long)size[g],
                         rec[j].n_out, (unsigned long long)(S - size[g]), bases);
                fa += '>'; fa += label; fa += line; fa += up; fa += mid; fa += lo; fa += "N\n";
            }
        }
        at = end;
        if (fasta && !idx.empty() && (r = write_file(std::string(out_prefix) + "." + label + ".markers.fa", fa)) != SKX_OK) return r;
    }
    if ((r = write_file(std::string(out_prefix) + ".markers.tsv", tsv)) != SKX_OK) return r;
    return write_file(std::string(out_prefix) + ".markers.summary.tsv", summary);
    });
}
