// ska_groups.cpp -- `ska align --groups / --samples`: one alignment per group of samples from a single load (host side above the C ABI).
// The reference has no such mode: its users run `ska delete` + `ska align` per group (generic_modes.rs:192-210, 22-50); the files written here
// are those, byte for byte.  skh_read_groups touches no device.
#include "ska_host_util.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <fcntl.h>
#include <unistd.h>
#include <vector>

using namespace skh;
namespace {

struct Group { std::string label; std::vector<std::string> names; };

// The two-column file: records end at a line break outside quotes; a record with a tab outside quotes is split at those tabs, any other at
// its commas outside quotes.  A field that begins with " runs to the closing quote, "" inside it being one quote (RFC 4180, what
// skh_clusters_csv writes for names holding , " or a line break).
int read_groups(const char *path, std::vector<Group> &groups)
{
    FILE *fp = fopen(path, "rb");
    if (!fp) { set_error("Unable to open groups file: %s", path); return SKX_EIO; }
    std::string text;
    char chunk[1 << 16];
    for (size_t n; (n = fread(chunk, 1, sizeof chunk, fp)) > 0;) text.append(chunk, n);
    const bool read_failed = ferror(fp) != 0;
    fclose(fp);
    if (read_failed) { set_error("Unable to read groups file: %s", path); return SKX_EIO; }
    auto refuse = [&](uint64_t at, const std::string &why) {
        set_error("groups file %s: line %llu: %s", path, (unsigned long long)at, why.c_str());
        return SKX_EINVAL;
    };
    std::vector<std::pair<std::string, uint64_t>> seen;                      // sample name, line: sorted before the duplicates are looked for
    struct Pair { std::string name, label; uint64_t line; };
    std::vector<Pair> pairs;
    uint64_t line = 1; bool first_record = true;
    for (size_t i = 0; i < text.size();) {
        // one record: its raw extent first (quotes decide where it ends), then its fields
        const uint64_t line0 = line;
        size_t e = i; bool inq = false, field_start = true, has_tab = false;
        for (; e < text.size(); e++) {
            const char c = text[e];
            if (inq) { if (c == '"') { if (e + 1 < text.size() && text[e + 1] == '"') e++; else inq = false; } else if (c == '\n') line++; field_start = false; continue; }
            if (c == '\n') break;
            if (c == '"' && field_start) { inq = true; field_start = false; continue; }
            if (c == '\t') has_tab = true;
            field_start = c == ',' || c == '\t';
        }
        if (inq) return refuse(line0, "a quoted field is not closed");
        size_t end = e;                                                       // the record is text[i, end)
        const size_t next = e < text.size() ? e + 1 : e;
        if (e < text.size()) line++;
        if (end > i && text[end - 1] == '\r') end--;
        if (end == i) { i = next; continue; }                                 // blank line
        const char sep = has_tab ? '\t' : ',';
        std::vector<std::string> fields(1);
        bool quoted_done = false, bad_quote = false;
        for (size_t p = i; p < end; p++) {
            const char c = text[p];
            std::string &fl = fields.back();
            if (c == '"' && fl.empty() && !quoted_done) {
                for (p++; p < end; p++) {
                    if (text[p] == '"') { if (p + 1 < end && text[p + 1] == '"') { fl += '"'; p++; } else break; }
                    else fl += text[p];
                }
                quoted_done = true;
                continue;
            }
            if (c == sep) { fields.emplace_back(); quoted_done = false; continue; }
            if (quoted_done) { bad_quote = true; break; }                     // text behind a closing quote
            fl += c;
        }
        if (bad_quote) return refuse(line0, "text follows a closing quote");
        if (fields.size() != 2) return refuse(line0, "two fields are required (sample name, group label), found " + std::to_string(fields.size()));
        if (first_record) { first_record = false; if (fields[0] == "id" && fields[1] == "Cluster__autocolour") { i = next; continue; } }
        const std::string &name = fields[0], &label = fields[1];
        if (name.empty()) return refuse(line0, "the sample name is empty");
        if (label.empty()) return refuse(line0, "the group label is empty");
        if (name.find('\0') != std::string::npos) return refuse(line0, "the sample name holds a NUL");
        if (label.find('/') != std::string::npos || label.find('\0') != std::string::npos || label == "." || label == "..")
            return refuse(line0, "the group label cannot be part of a file name ('/', NUL, \".\" or \"..\")");
        pairs.push_back(Pair{name, label, line0});
        i = next;
    }
    for (auto &p : pairs) seen.emplace_back(p.name, p.line);
    std::sort(seen.begin(), seen.end());
    uint64_t dup_line = 0, dup_first = 0; const std::string *dup = nullptr;
    for (size_t j = 1; j < seen.size(); j++)
        if (seen[j].first == seen[j - 1].first && (!dup || seen[j].second < dup_line)) { dup = &seen[j].first; dup_line = seen[j].second; dup_first = seen[j - 1].second; }
    if (dup) return refuse(dup_line, "sample \"" + *dup + "\" is listed twice (first on line " + std::to_string(dup_first) + ")");
    for (auto &p : pairs) {
        size_t g = 0;
        while (g < groups.size() && groups[g].label != p.label) g++;
        if (g == groups.size()) { groups.emplace_back(); groups.back().label = p.label; }
        groups[g].names.push_back(p.name);
    }
    return SKX_OK;
}

// names -> column indices as skx_array_delete_samples finds them: first match wins (merge_ska_array.rs:243-249)
int resolve_names(skx_array *a, const std::vector<std::string> &want, std::vector<char> &taken, std::vector<int> &idx)
{
    skx_array_info_t info; skx_array_info(a, &info);
    for (auto &w : want) {
        bool found = false;
        for (uint64_t s = 0; s < info.n_samples && !found; s++)
            if (!taken[s] && w == skx_array_name(a, s)) { taken[s] = 1; idx.push_back((int)s); found = true; }
        if (!found) { set_error("Could not find sample(s): {\"%s\"}", w.c_str()); return SKX_EINVAL; }                   // :252-254
    }
    return SKX_OK;
}

void log_filters(uint64_t n, int filter_type, int mask_ambig, int ignore_const_gaps, double min_freq, int filter_ambig_as_missing)
{
    static const char *const FN[] = {"No filtering", "No constant sites", "No ambiguous sites", "No constant sites or ambiguous bases"};
    char msg[320];
    snprintf(msg, sizeof msg, "Applying filters: threshold=%llu constant_site_filter=%s filter_ambig_as_missing=%s ambig_mask=%s no_gap_only_sites=%s",
             (unsigned long long)std::ceil((double)n * min_freq), FN[filter_type & 3], filter_ambig_as_missing ? "true" : "false", mask_ambig ? "true" : "false",
             ignore_const_gaps ? "true" : "false");
    skh_log(2, "ska::generic_modes", msg);                                                                                // generic_modes.rs:121-122
}

}  // namespace

extern "C" int skh_read_groups(const char *path, char **buf, uint64_t *len, uint64_t *n_pairs)
{
    return guarded([&]() -> int {
    if (!path || !buf || !len) { skx_set_last_error("skh_read_groups: bad arguments"); return SKX_EINVAL; }
    std::vector<Group> groups;
    const int r = read_groups(path, groups);
    if (r != SKX_OK) return r;
    std::string o; uint64_t n = 0;
    for (auto &g : groups) for (auto &nm : g.names) { o += nm; o += '\0'; o += g.label; o += '\0'; n++; }
    char *p = (char *)malloc(o.size() + 1);
    if (!p) { skx_set_last_error("out of host memory"); return SKX_ENOMEM; }
    memcpy(p, o.data(), o.size()); p[o.size()] = 0;
    *buf = p; *len = o.size();
    if (n_pairs) *n_pairs = n;
    return SKX_OK;
    });
}

extern "C" int skh_align_groups(skx_ctx *ctx, const char *const *inputs, int n_inputs, int threads, int filter_type, int mask_ambig, int ignore_const_gaps,
                                double min_freq, int filter_ambig_as_missing, const char *groups_file, int min_group_size, const char *out_prefix)
{
    return guarded([&]() -> int {
    if (!ctx || !inputs || n_inputs < 1 || !groups_file || !out_prefix || min_group_size < 1) { skx_set_last_error("skh_align_groups: bad arguments"); return SKX_EINVAL; }
    std::vector<Group> groups;
    int r = read_groups(groups_file, groups);
    if (r != SKX_OK) return r;
    skx_array *a = nullptr;
    { Phase pl("align.groups_load"); if ((r = skh_load_array(ctx, inputs, n_inputs, threads, &a)) != SKX_OK) return r; }
    struct Free { skx_array *a; ~Free() { skx_array_free(a); } } free_a{a};
    skx_array_info_t info; skx_array_info(a, &info);
    std::vector<char> taken(info.n_samples, 0);
    std::vector<std::vector<int>> idx(groups.size());
    for (size_t g = 0; g < groups.size(); g++) if ((r = resolve_names(a, groups[g].names, taken, idx[g])) != SKX_OK) return r;
    const skx_filter_spec fs{min_freq, filter_ambig_as_missing, filter_type, mask_ambig, ignore_const_gaps, 0};
    std::string table = "Group\tSamples\tSplit k-mers\tRemoved\tSites\tFile\n";
    char msg[600];
    for (size_t g = 0; g < groups.size(); g++) {
        const int n = (int)idx[g].size();
        const bool skip = n < min_group_size;
        skx_array *sub = nullptr; skx_subset_info si{0, 0, 0, 0};
        // (the phases align.groups_verdicts and align.groups_rows are recorded by the call itself: both happen inside it)
        if (!skip) log_filters((uint64_t)n, filter_type, mask_ambig, ignore_const_gaps, min_freq, filter_ambig_as_missing);
        if ((r = skx_array_subset_filtered(a, idx[g].data(), n, &fs, skip ? nullptr : &sub, &si)) != SKX_OK) return r;
        char line[200];
        if (skip) {
            snprintf(msg, sizeof msg, "Group %s: %d samples, fewer than --min-group-size %d: no alignment", groups[g].label.c_str(), n, min_group_size);
            skh_log(2, "ska::generic_modes", msg);
            snprintf(line, sizeof line, "\t%d\t%llu\t-\t-\t-\n", n, (unsigned long long)si.rows_present);
            table += groups[g].label; table += line;
            continue;
        }
        struct FreeSub { skx_array *a; ~FreeSub() { skx_array_free(a); } } free_sub{sub};
        const std::string file = std::string(out_prefix) + "." + groups[g].label + ".aln";
        snprintf(msg, sizeof msg, "Group %s: %d samples, %llu split k-mers, filtering removed %llu, writing %llu sites to %s", groups[g].label.c_str(), n,
                 (unsigned long long)si.rows_present, (unsigned long long)si.removed, (unsigned long long)si.sites, file.c_str());
        skh_log(2, "ska::generic_modes", msg);
        {
            Phase pw("align.groups_write");
            const int fd = open(file.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0644);                                          // read-write: the writer maps the file
            if (fd < 0) { set_error("cannot create output file %s", file.c_str()); return SKX_EIO; }
            r = skx_array_write_fasta(sub, fd);
            if (close(fd) != 0 && r == SKX_OK) { set_error("write failed: %s", file.c_str()); r = SKX_EIO; }
            if (r != SKX_OK) return r;
        }
        snprintf(line, sizeof line, "\t%d\t%llu\t%llu\t%llu\t", n, (unsigned long long)si.rows_present, (unsigned long long)si.removed, (unsigned long long)si.sites);
        table += groups[g].label; table += line; table += file; table += '\n';
    }
    const std::string tsv = std::string(out_prefix) + ".groups.tsv";
    FILE *f = fopen(tsv.c_str(), "wb");
    if (!f) { set_error("cannot create output file %s", tsv.c_str()); return SKX_EIO; }
    const bool ok = fwrite(table.data(), 1, table.size(), f) == table.size();
    if (fclose(f) != 0 || !ok) { set_error("write failed: %s", tsv.c_str()); return SKX_EIO; }
    return SKX_OK;
    });
}

extern "C" int skh_align_samples_fd(skx_ctx *ctx, const char *const *inputs, int n_inputs, int threads, int filter_type, int mask_ambig, int ignore_const_gaps,
                                    double min_freq, int filter_ambig_as_missing, const char *const *names, int n_names, int fd)
{
    return guarded([&]() -> int {
    if (!ctx || !inputs || n_inputs < 1 || !names || n_names < 1) { skx_set_last_error("skh_align_samples_fd: bad arguments"); return SKX_EINVAL; }
    std::vector<std::string> want;                                            // a set of names, as `ska delete` takes its own
    for (int i = 0; i < n_names; i++) if (std::find(want.begin(), want.end(), names[i]) == want.end()) want.emplace_back(names[i]);
    skx_array *a = nullptr; int r;
    { Phase pl("align.groups_load"); if ((r = skh_load_array(ctx, inputs, n_inputs, threads, &a)) != SKX_OK) return r; }
    struct Free { skx_array *a; ~Free() { skx_array_free(a); } } free_a{a};
    skx_array_info_t info; skx_array_info(a, &info);
    std::vector<char> taken(info.n_samples, 0); std::vector<int> idx;
    if ((r = resolve_names(a, want, taken, idx)) != SKX_OK) return r;
    const skx_filter_spec fs{min_freq, filter_ambig_as_missing, filter_type, mask_ambig, ignore_const_gaps, 0};
    log_filters(idx.size(), filter_type, mask_ambig, ignore_const_gaps, min_freq, filter_ambig_as_missing);
    skx_array *sub = nullptr; skx_subset_info si{0, 0, 0, 0};
    if ((r = skx_array_subset_filtered(a, idx.data(), (int)idx.size(), &fs, &sub, &si)) != SKX_OK) return r;
    struct FreeSub { skx_array *a; ~FreeSub() { skx_array_free(a); } } free_sub{sub};
    char msg[200];
    snprintf(msg, sizeof msg, "Filtering removed %llu split k-mers", (unsigned long long)si.removed);                     // merge_ska_array.rs:385
    skh_log(2, "ska::merge_ska_array", msg);
    skh_log(2, "ska::generic_modes", "Writing alignment");                                                                // generic_modes.rs:45
    Phase pw("align.groups_write");
    return skx_array_write_fasta(sub, fd);
    });
}
