// ska_distance.cpp -- `ska distance` on the host, above the C ABI (generic_modes.rs:139-190, lib.rs:710-727): one load, one line writer,
// the entries of include/skx_host.h (table, --query*, the selecting options, --mst, --sites, --no-table), then the command line's half
// (what clap would refuse, and the dispatch).  The several-GPU table is skh_distance_sharded in ska_host.cpp.
#include "ska_host_util.h"
#include <climits>
#include <cmath>
#include <fstream>
#include <sstream>

namespace skh {
namespace {

// ---------------------------------------------------------------------------------------------- one load
void log_calculating() { skh_log(2, "ska::generic_modes", "Calculating distances"); }                   // generic_modes.rs:170
std::vector<const char *> names_of(skx_array *a, uint64_t S)
{
    std::vector<const char *> names(S);
    for (uint64_t i = 0; i < S; i++) names[i] = skx_array_name(a, i);
    return names;
}
// the array a mode sweeps, freed when the mode is done
struct Loaded {
    skx_array *a = nullptr; int64_t constant = 0; uint64_t S = 0; int k = 0; std::vector<const char *> names;
    Loaded() = default;
    Loaded(const Loaded &) = delete;
    ~Loaded() { if (a) skx_array_free(a); }
    // an array already loaded (skh_load_array, merge_files)
    void take(skx_array *arr)
    {
        a = arr;
        skx_array_info_t info; skx_array_info(a, &info);
        S = info.n_samples; k = info.k; names = names_of(a, S);
    }
    // the file with the two filters of generic_modes.rs:149-168 applied while its rows are read; `constant`: the rows the second took
    int load(skx_ctx *ctx, const char *skf_file, double min_freq)
    {
        log_calculating();
        skx_filter_spec fs{min_freq, 0, SKX_FILTER_NO_CONST, 0, 0, 1};
        skx_array *arr = nullptr; int64_t removed = 0;
        const int r = skx_array_load_filtered(ctx, skf_file, &fs, &arr, &removed, &constant);
        if (r == SKX_OK) take(arr);
        return r;
    }
};
struct Freed { void *p; ~Freed() { skx_free(p); } };                    // a buffer the engine handed out

// ---------------------------------------------------------------------------------------------- one line writer
const char DIST_HEADER[] = "Sample1\tSample2\tDistance\tMismatches (proportion)\tMatch count\tMismatch count\n";
void put_dist_line(std::string &o, const char *n1, const char *n2, const skx_dist &d)
{
    put(o, "%s\t%s\t%.2f\t%.5f\t%llu\t%llu\n", n1, n2, d.distance, d.mismatch_prop, (unsigned long long)d.match_count, (unsigned long long)d.mismatch_count);
}
// the lines of distance_text_names' table that name a query, in its order (ascending first sample, then ascending second); d as
// skx_array_distance_query lays it out: d[q * S + j] = the pair (query[q], j)
int distance_query_text(const std::vector<const char *> &names, const std::vector<int> &query, const skx_dist *d, char **buf, uint64_t *len)
{
    const uint64_t S = names.size();
    Phase pt("distance.table_text");
    std::vector<int> row_of(S, -1), sorted(query);
    for (size_t q = 0; q < query.size(); q++) row_of[query[q]] = (int)q;
    std::sort(sorted.begin(), sorted.end());
    return format_rows(DIST_HEADER, S, [&](uint64_t i, std::string &o) {
        if (row_of[i] >= 0) for (uint64_t j = i + 1; j < S; j++) put_dist_line(o, names[i], names[j], d[(uint64_t)row_of[i] * S + j]);
        else for (auto it = std::upper_bound(sorted.begin(), sorted.end(), (int)i); it != sorted.end(); ++it)
            put_dist_line(o, names[i], names[*it], d[(uint64_t)row_of[*it] * S + i]);
    }, buf, len);
}
// the header and one line per selected pair (ascending (i, j): the table's order)
int distance_select_text(const std::vector<const char *> &names, const skx_dist_pair *p, uint64_t n, char **buf, uint64_t *len)
{
    Phase pt("distance.table_text");
    return format_slices(DIST_HEADER, n, [&](uint64_t x, std::string &o) { put_dist_line(o, names[p[x].i], names[p[x].j], p[x].d); }, buf, len);
}

// ---------------------------------------------------------------------------------------------- the tree's file
int write_newick(const std::vector<const char *> &names, const skx_nj_join *joins, int S, const char *path)
{
    Phase pt("distance.tree_text");
    char *buf = nullptr; uint64_t len = 0;
    int r = skh_nj_newick(names.data(), joins, S, &buf, &len);
    if (r != SKX_OK) return r;
    r = write_text_file(path, buf, len);
    skx_free(buf);
    return r;
}
}  // namespace

// the whole table: the rows of one first sample are one part
int distance_text_names(const std::vector<const char *> &names, const skx_dist *d, char **buf, uint64_t *len)
{
    const uint64_t S = names.size();
    Phase pt("distance.table_text");
    return format_rows(DIST_HEADER, S, [&](uint64_t i, std::string &o) {
        size_t n = (size_t)(i * (2 * S - i - 1) / 2);               // pairs before row i
        for (uint64_t j = i + 1; j < S; j++, n++) put_dist_line(o, names[i], names[j], d[n]);
    }, buf, len);
}
// `ska distance --tree / --clusters`: the tree and the clusters of the table the command has just computed (x may be NULL)
int distance_extras(skx_ctx *ctx, const std::vector<const char *> &names, const skx_dist *d, const skh_dist_extras *x)
{
    if (!x) return SKX_OK;
    const int S = (int)names.size();
    int r = SKX_OK;
    if (x->tree) {
        std::vector<skx_nj_join> joins((size_t)std::max(S - 1, 1));
        { Phase pn("distance.nj"); if ((r = skx_dist_nj(ctx, d, S, joins.data())) != SKX_OK) return r; }
        if ((r = write_newick(names, joins.data(), S, x->tree)) != SKX_OK) return r;
    }
    if (x->clusters) {
        Phase pc("distance.clusters");
        char *csv = nullptr, *dot = nullptr; uint64_t nc = 0, nd = 0;
        if ((r = skh_distance_clusters(names.data(), d, S, x->cluster_snps, x->cluster_mismatches, &csv, &nc, &dot, &nd)) != SKX_OK) return r;
        r = write_text_file(std::string(x->clusters) + ".clusters.csv", csv, nc);
        if (r == SKX_OK) r = write_text_file(std::string(x->clusters) + ".graph.dot", dot, nd);
        skx_free(csv); skx_free(dot);
    }
    return r;
}
}  // namespace skh
using namespace skh;

// ---------------------------------------------------------------------------------------------- the entries
extern "C" int skh_distance_tsv(skx_array *a, double min_freq, int filt_ambig, char **buf, uint64_t *len)
{
    return guarded([&]() -> int {
    skx_array_info_t info; skx_array_info(a, &info);
    const uint64_t S = info.n_samples;
    std::vector<skx_dist> d(S * (S - 1) / 2 + 1);
    int64_t constant = 0; uint64_t rows = 0; int r;
    // the two filters of generic_modes.rs:149-168 are applied while the bit planes are built; the array itself stays as it is
    { Phase pd("distance.pair_sweep"); if ((r = skx_array_distance_filtered(a, min_freq, filt_ambig, d.data(), &constant, &rows)) != SKX_OK) return r; }
    return distance_text_names(names_of(a, S), d.data(), buf, len);
    });
}

extern "C" int skh_distance_skf_tsv(skx_ctx *ctx, const char *skf_file, double min_freq, int filt_ambig, char **buf, uint64_t *len)
{
    return skh_distance_skf_tsv_extras(ctx, skf_file, min_freq, filt_ambig, nullptr, buf, len);
}
extern "C" int skh_distance_skf_tsv_extras(skx_ctx *ctx, const char *skf_file, double min_freq, int filt_ambig, const skh_dist_extras *extras, char **buf,
                                           uint64_t *len)
{
    return guarded([&]() -> int {
    Loaded in; int r;
    if ((r = in.load(ctx, skf_file, min_freq)) != SKX_OK) return r;
    std::vector<skx_dist> d(in.S * (in.S - 1) / 2 + 1);
    { Phase pd("distance.pair_sweep"); if ((r = skx_array_distance(in.a, (double)in.constant, filt_ambig, d.data())) != SKX_OK) return r; }
    if ((r = distance_extras(skx_array_ctx(in.a), in.names, d.data(), extras)) != SKX_OK) return r;
    return distance_text_names(in.names, d.data(), buf, len);
    });
}

extern "C" int skh_distance_query_tsv(skx_ctx *ctx, const char *skf_file, const char *query_skf, const char *const *names, int n_names, double min_freq,
                                      int filt_ambig, char **buf, uint64_t *len)
{
    return guarded([&]() -> int {
    if (!ctx || !skf_file || !buf || !len || n_names < 0 || (n_names && !names)) { set_error("skh_distance_query_tsv: bad arguments"); return SKX_EINVAL; }
    Loaded in; int r;
    std::vector<uint64_t> n_each;
    if (query_skf) {                                                                   // `ska merge skf_file query_skf`, kept in memory
        const char *files[2] = {skf_file, query_skf};
        skx_array *m = nullptr;
        log_calculating();
        if ((r = merge_files(ctx, files, 2, &m, &n_each)) != SKX_OK) return r;
        in.take(m);
    } else if ((r = in.load(ctx, skf_file, min_freq)) != SKX_OK) return r;
    const uint64_t S = in.S;
    // the query set: the names (each its first match, as skx_array_delete_samples looks them up) and every sample the second file brought
    std::vector<char> is_q(S, 0);
    for (int n = 0; n < n_names; n++) {
        uint64_t i = 0;
        while (i < S && strcmp(in.names[i], names[n]) != 0) i++;
        if (i == S) { set_error("Could not find sample(s): {\"%s\"}", names[n]); return SKX_EINVAL; }                         // merge_ska_array.rs:252-254
        is_q[i] = 1;
    }
    if (query_skf) for (uint64_t i = std::min<uint64_t>(n_each[0], S); i < S; i++) is_q[i] = 1;               // (the first file's samples come first)
    std::vector<int> query;
    for (uint64_t i = 0; i < S; i++) if (is_q[i]) query.push_back((int)i);
    if (query.empty()) { set_error("No query samples given"); return SKX_EINVAL; }
    std::vector<skx_dist> d(query.size() * S);
    {
        Phase pd("distance.pair_sweep");
        if (query_skf) { uint64_t rows = 0; r = skx_array_distance_query_filtered(in.a, min_freq, filt_ambig, query.data(), (int)query.size(), d.data(), &in.constant, &rows); }
        else r = skx_array_distance_query(in.a, (double)in.constant, filt_ambig, query.data(), (int)query.size(), d.data());
        if (r != SKX_OK) return r;
    }
    return distance_query_text(in.names, query, d.data(), buf, len);
    });
}

// --max-snps / --max-mismatches / --closest: the lines of the table picked on the device
extern "C" int skh_distance_select_tsv(skx_ctx *ctx, const char *skf_file, double min_freq, int filt_ambig, const skx_select_spec *spec, char **buf, uint64_t *len)
{
    return guarded([&]() -> int {
    if (!ctx || !skf_file || !spec || !buf || !len) { set_error("skh_distance_select_tsv: bad arguments"); return SKX_EINVAL; }
    Loaded in; int r;
    if ((r = in.load(ctx, skf_file, min_freq)) != SKX_OK) return r;
    skx_dist_pair *pairs = nullptr; uint64_t n = 0;
    skx_select_info si{0, 0, 0, 0};
    { Phase pd("distance.pair_sweep"); if ((r = skx_array_distance_select_prefiltered(in.a, in.constant, filt_ambig, spec, &pairs, &n, &si)) != SKX_OK) return r; }
    Freed free_pairs{pairs};
    char msg[200];
    snprintf(msg, sizeof msg, "Selected %llu lines of %llu candidate pairs: %llu bands of %llu samples, count buffer of %llu bytes", (unsigned long long)n,
             (unsigned long long)si.candidates, (unsigned long long)si.bands, (unsigned long long)si.band_rows, (unsigned long long)si.count_buffer_bytes);
    skh_log(2, "ska::generic_modes", msg);
    return distance_select_text(in.names, pairs, n, buf, len);
    });
}

// `ska distance --mst`: the forest's lines as text, and with levels (n_levels > 0) the ladder's CSV from the same forest
static int distance_mst_run(skx_ctx *ctx, const char *skf_file, double min_freq, int filt_ambig, const skx_mst_spec *spec, const double *levels, int n_levels, char **buf,
                            uint64_t *len, char **csv, uint64_t *csv_len)
{
    return guarded([&]() -> int {
    Loaded in; int r;
    if ((r = in.load(ctx, skf_file, min_freq)) != SKX_OK) return r;
    skx_dist_pair *pairs = nullptr; uint64_t n = 0;
    skx_mst_info mi{0, 0, 0, 0, 0, 0, 0};
    { Phase pd("distance.pair_sweep"); if ((r = skx_array_distance_mst_prefiltered(in.a, in.constant, filt_ambig, spec, &pairs, &n, &mi)) != SKX_OK) return r; }
    Freed free_pairs{pairs};
    char msg[260];
    snprintf(msg, sizeof msg, "Spanning forest of %llu lines in %llu trees from %llu candidate pairs: %llu bands of %llu samples, count buffer of %llu bytes, at most %llu rounds a band",
             (unsigned long long)mi.edges, (unsigned long long)mi.components, (unsigned long long)mi.candidates, (unsigned long long)mi.bands, (unsigned long long)mi.band_rows,
             (unsigned long long)mi.count_buffer_bytes, (unsigned long long)mi.rounds);
    skh_log(2, "ska::generic_modes", msg);
    r = distance_select_text(in.names, pairs, n, buf, len);
    if (r == SKX_OK && n_levels > 0 && in.S) {
        r = skh_mst_levels_csv(in.names.data(), pairs, n, (int)in.S, levels, n_levels, csv, csv_len);
        if (r != SKX_OK) { skx_free(*buf); *buf = nullptr; }
    }
    return r;
    });
}
extern "C" int skh_distance_mst_tsv(skx_ctx *ctx, const char *skf_file, double min_freq, int filt_ambig, const skx_mst_spec *spec, char **buf, uint64_t *len)
{
    if (!ctx || !skf_file || !spec || !buf || !len) { set_error("skh_distance_mst_tsv: bad arguments"); return SKX_EINVAL; }
    return distance_mst_run(ctx, skf_file, min_freq, filt_ambig, spec, nullptr, 0, buf, len, nullptr, nullptr);
}

// `ska distance ... --sites PREFIX`: the selected lines from the array loaded with its split k-mers, then the rows behind each line's Distance
extern "C" int skh_distance_sites(skx_ctx *ctx, const char *skf_file, double min_freq, const skx_select_spec *spec, const skx_mst_spec *mst, const char *prefix,
                                  uint64_t max_records, char **buf, uint64_t *len)
{
    return guarded([&]() -> int {
    if (!ctx || !skf_file || !prefix || !buf || !len || !spec == !mst) { set_error("skh_distance_sites: bad arguments"); return SKX_EINVAL; }
    *buf = nullptr; *len = 0;
    log_calculating();
    Loaded in; int r;
    { const char *files[1] = {skf_file}; skx_array *a = nullptr; if ((r = skh_load_array(ctx, files, 1, 1, &a)) != SKX_OK) return r; in.take(a); }
    skx_dist_pair *pairs = nullptr; uint64_t n_pairs = 0;
    {
        Phase pd("distance.pair_sweep");
        uint64_t rows = 0;
        r = spec ? skx_array_distance_select(in.a, min_freq, 1, spec, &pairs, &n_pairs, &in.constant, &rows, nullptr)
                 : skx_array_distance_mst(in.a, min_freq, 1, mst, &pairs, &n_pairs, &in.constant, &rows, nullptr);
        if (r != SKX_OK) return r;
    }
    Freed free_pairs{pairs};
    if ((r = distance_select_text(in.names, pairs, n_pairs, buf, len)) != SKX_OK) return r;
    std::vector<uint32_t> ij(2 * n_pairs);
    for (uint64_t p = 0; p < n_pairs; p++) { ij[2 * p] = pairs[p].i; ij[2 * p + 1] = pairs[p].j; }
    skx_pair_site *rec = nullptr; skx_key *keys = nullptr; uint64_t n = 0;
    // (the phases distance.sites_count and distance.sites_write are recorded by the call itself: both happen inside it)
    if ((r = skx_array_pair_sites(in.a, min_freq, ij.data(), n_pairs, max_records, &rec, &keys, nullptr, &n)) != SKX_OK) return r;
    Freed free_rec{rec}, free_keys{keys};
    char msg[160];
    snprintf(msg, sizeof msg, "Sites: %llu records of %llu lines", (unsigned long long)n, (unsigned long long)n_pairs);
    skh_log(2, "ska::generic_modes", msg);
    Phase pt("distance.sites_text");
    const std::vector<std::string> part = slice_parts(n, [&](uint64_t x, std::string &o) {
        const skx_dist_pair &p = pairs[rec[x].pair];
        char up[32], lo[32];
        skh_key_arms(&keys[x], in.k, up, lo);
        o += in.names[p.i]; o += '\t'; o += in.names[p.j]; o += '\t'; o += up; o += '\t'; o += lo; o += '\t';
        o += (char)rec[x].base_i; o += '\t'; o += (char)rec[x].base_j; o += '\n';
    });
    // (the slices go to the file one after the other: the text, gigabytes for a large selection, is never held twice)
    const std::string path = std::string(prefix) + ".sites.tsv";
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) { set_error("cannot create %s", path.c_str()); return SKX_EIO; }
    bool ok = fputs("Sample1\tSample2\tUpper\tLower\tBase1\tBase2\n", f) >= 0;
    for (auto &x : part) ok = ok && fwrite(x.data(), 1, x.size(), f) == x.size();
    if (fclose(f) != 0 || !ok) { set_error("cannot write %s", path.c_str()); return SKX_EIO; }
    return SKX_OK;
    });
}

// `ska distance --no-table`: the extras' files from the banded sweep (x names at least one).  What reaches the host is S labels and S - 1 joins
extern "C" int skh_distance_banded_files(skx_ctx *ctx, const char *skf_file, double min_freq, int filt_ambig, const skh_dist_extras *x)
{
    return guarded([&]() -> int {
    if (!ctx || !skf_file || !x || (!x->tree && !x->clusters)) { set_error("skh_distance_banded_files: bad arguments"); return SKX_EINVAL; }
    Loaded in; int r;
    if ((r = in.load(ctx, skf_file, min_freq)) != SKX_OK) return r;
    const int S = (int)in.S;
    std::vector<uint32_t> labels((size_t)std::max(S, 1)); std::vector<skx_nj_join> joins((size_t)std::max(S - 1, 1));
    const skx_banded_spec spec{x->cluster_snps, x->cluster_mismatches, 0};
    skx_banded_info bi{0, 0, 0, 0, 0};
    // (the phases distance.pair_sweep and distance.nj are recorded by the call itself: both happen inside it)
    if ((r = skx_array_distance_banded_prefiltered(in.a, in.constant, filt_ambig, &spec, x->clusters ? labels.data() : nullptr, x->tree ? joins.data() : nullptr, &bi)) != SKX_OK) return r;
    char msg[200];
    snprintf(msg, sizeof msg, "No table: %llu bands of %llu samples, count buffer of %llu bytes; %llu pairs within the cluster thresholds, %llu clusters",
             (unsigned long long)bi.bands, (unsigned long long)bi.band_rows, (unsigned long long)bi.count_buffer_bytes, (unsigned long long)bi.edges, (unsigned long long)bi.clusters);
    skh_log(2, "ska::generic_modes", msg);
    if (x->tree && (r = write_newick(in.names, joins.data(), S, x->tree)) != SKX_OK) return r;
    if (x->clusters) {
        Phase pc("distance.clusters");
        char *csv = nullptr; uint64_t nc = 0;
        if ((r = skh_clusters_csv(in.names.data(), labels.data(), S, &csv, &nc)) != SKX_OK) return r;
        r = write_text_file(std::string(x->clusters) + ".clusters.csv", csv, nc);
        skx_free(csv);
    }
    return r;
    });
}

// ---------------------------------------------------------------------------------------------- the command line
namespace skh {
namespace {
// --query / --query-file / --query-skf: named samples against the rest of the array (skh_distance_query_tsv)
const char *const QUERY_OPTS[] = {"--query", "--query-file", "--query-skf"};
// --max-snps / --max-mismatches / --closest: the lines of the table picked on the device (skh_distance_select_tsv)
const char *const SELECT_OPTS[] = {"--max-snps", "--max-mismatches", "--closest"};
template <size_t N> bool has_any(const Args &a, const char *const (&flags)[N]) { for (auto f : flags) if (a.has(f)) return true; return false; }
skx_select_spec select_spec(const Args &a)
{
    skx_select_spec sp{-1.0, -1.0, 0, 0};
    if (a.has("--max-snps")) sp.max_snps = strtod(a.get("--max-snps").c_str(), nullptr);
    if (a.has("--max-mismatches")) sp.max_mismatches = strtod(a.get("--max-mismatches").c_str(), nullptr);
    if (a.has("--closest")) sp.closest = (int32_t)std::min<unsigned long long>(strtoull(a.get("--closest").c_str(), nullptr, 10), INT32_MAX);
    return sp;
}
// --mst / --mst-clusters / --levels: the table's minimum spanning forest (skx_array_distance_mst) and its clusters at a ladder of levels
const char *const MST_DEFAULT_LEVELS = "250,100,50,25,10,5,0";
constexpr size_t MST_MAX_LEVELS = 16;
// the comma-separated levels -> out; nullptr, or why the list does not stand (the values are checked by validate_distance before they are used)
const char *parse_levels(const std::string &v, std::vector<double> &out)
{
    out.clear();
    size_t at = 0;
    for (;;) {
        const size_t end = std::min(v.find(',', at), v.size());
        const std::string t = v.substr(at, end - at);
        if (t.empty()) return "cannot parse float from empty string";
        if (!lo_float(t)) return "invalid float literal";
        const double x = strtod(t.c_str(), nullptr);
        if (!(x >= 0.0)) return "a level must be zero or more";
        if (std::find(out.begin(), out.end(), x) != out.end()) return "a level is given twice";
        out.push_back(x);
        if (out.size() > MST_MAX_LEVELS) return "at most 16 levels";
        if (end == v.size()) return nullptr;
        at = end + 1;
    }
}
// --query / --query-file: the names of both, repeats collapsed.  0, or the exit code after the refusal was printed
int read_query_names(const Args &a, std::vector<std::string> &names)
{
    auto add = [&](const std::string &n) { if (!n.empty() && std::find(names.begin(), names.end(), n) == names.end()) names.push_back(n); };
    for (auto &o : a.opt) {
        if (o.first == "--query") { std::istringstream ls(o.second); std::string t; while (std::getline(ls, t, ',')) add(t); }
        else if (o.first == "--query-file") {                                          // io_utils::get_input_list as `ska delete -f` reads it: first column
            std::ifstream in(o.second);
            if (!in) return fail("Unable to open file_list");
            std::string line;
            while (std::getline(in, line)) { std::istringstream ls(line); std::string t; if (ls >> t) add(t); }
        }
    }
    return 0;
}
int required_value(const Args &a, const char *flag) { return a.has(flag) && a.get(flag).empty() ? clap_invalid("", clap_arg(flag), "a value is required") : 0; }
}  // namespace

// What clap would refuse of `ska distance` (the engine's own options are refused the way clap refuses the reference's): arguments that
// conflict, a missing requirement, a value that does not parse -- in that order within each block, the blocks in the order below.
int validate_distance(const Args &a, bool multi)
{
    if (a.has("--sites") || a.has("--sites-max")) {
        // the sites are those of the selected lines of one device's filter-ambiguous table (the ladder is cut from the prefiltered load's forest)
        if (int e = conflicts("distance", a, multi, {"--sites"}, {"--allow-ambiguous", "--no-table", "--query", "--query-file", "--query-skf", "--gpus", "--mst-clusters"})) return e;
        if (!a.has("--sites")) return clap_missing("distance", "--sites <PREFIX>");
        if (!has_any(a, SELECT_OPTS) && !a.has("--mst")) return clap_missing("distance", "<--max-snps <N>|--max-mismatches <P>|--closest <K>|--mst>");
        if (int e = required_value(a, "--sites")) return e;
        if (a.has("--sites-max")) if (int e = clap_uint(a.get("--sites-max"), "--sites-max <N>", 1, "must be one or higher", /*check_erange=*/true)) return e;
    }
    if (a.has("--no-table")) {
        // the tree and the clusters from the banded sweep, on one device, and nothing else
        if (int e = conflicts("distance", a, multi, {"--no-table"}, {"-o", "--max-snps", "--max-mismatches", "--closest", "--query", "--query-file", "--query-skf", "--gpus"})) return e;
        if (a.has("--mst")) return clap_conflict("distance", "--mst", "--no-table");
        if (!a.has("--tree") && !a.has("--clusters")) return clap_missing("distance", "<--tree <FILE>|--clusters <PREFIX>>");
    }
    if (has_any(a, SELECT_OPTS)) {
        // the selection runs on one device and never forms the table the tree, the clusters and the query cut are taken from; the earliest
        // selection option is named first
        if (int e = conflicts("distance", a, multi, {"--max-snps", "--max-mismatches", "--closest"}, {"--tree", "--clusters", "--gpus", "--query", "--query-file", "--query-skf"})) return e;
        if (a.has("--closest") && a.has("--mst")) return clap_conflict("distance", "--closest", "--mst");      // (the forest takes the two thresholds only)
        if (a.has("--max-snps")) if (int e = clap_float(a.get("--max-snps"), "--max-snps <N>", 0.0, INFINITY, "must be zero or more")) return e;
        if (a.has("--max-mismatches")) if (int e = clap_float(a.get("--max-mismatches"), "--max-mismatches <P>", 0.0, 1.0, "Proportion must be between 0 and 1 (inclusive)")) return e;
        if (a.has("--closest")) if (int e = clap_uint(a.get("--closest"), "--closest <K>", 1, "must be one or higher")) return e;
    }
    if (a.has("--mst") || a.has("--mst-clusters") || a.has("--levels")) {
        // the forest comes from one device's banded sweep, which forms neither the table nor what is cut from it (--mst is named when no
        // other selection option is: those were refused above)
        if (int e = conflicts("distance", a, multi, {"--mst"}, {"--tree", "--clusters", "--cluster-snps", "--cluster-mismatches", "--gpus", "--query", "--query-file", "--query-skf"})) return e;
        if (!a.has("--mst")) return clap_missing("distance", a.has("--levels") && !a.has("--mst-clusters") ? "--mst\n  --mst-clusters <PREFIX>" : "--mst");
        if (a.has("--levels") && !a.has("--mst-clusters")) return clap_missing("distance", "--mst-clusters <PREFIX>");
        if (int e = required_value(a, "--mst-clusters")) return e;
        std::vector<double> lv;
        if (a.has("--levels")) if (const char *why = parse_levels(a.get("--levels"), lv)) return clap_invalid(a.get("--levels"), "--levels <L1,L2,...>", why);
    }
    if (has_any(a, QUERY_OPTS)) {
        // the query is cut from one device's table, and the tree and the clusters need all of it
        if (int e = conflicts("distance", a, multi, {"--query", "--query-file", "--query-skf"}, {"--tree", "--clusters", "--cluster-snps", "--cluster-mismatches", "--gpus"})) return e;
        for (auto q : QUERY_OPTS) if (int e = required_value(a, q)) return e;
        std::vector<std::string> names;
        if (int e = read_query_names(a, names)) return e;
        if (names.empty() && !a.has("--query-skf")) return clap_invalid(a.get("--query", a.get("--query-file")), a.has("--query") ? "--query <NAMES>" : "--query-file <FILE>", "no sample names given");
    }
    if (multi) { if (int e = validate_build_inputs("distance", a)) return e; }      // (--gpus N: sequence files or -f, and the build options)
    else if (a.pos.size() != 1) return a.pos.empty() ? clap_missing("distance", "<SKF_FILE>") : fail("one .skf file required");
    if (int e = validate_min_freq(a)) return e;
    // the engine's own options (the reference's scripts/cluster_dists.py: --snps, --mismatches)
    for (const char *o : {"--cluster-snps", "--cluster-mismatches"}) {
        if (!a.has(o)) continue;
        if (!a.has("--clusters")) return clap_missing("distance", "--clusters <PREFIX>");
        if (int e = clap_float(a.get(o), clap_arg(o), 0.0, INFINITY, "Threshold must be zero or higher")) return e;
    }
    for (const char *o : {"--tree", "--clusters"}) if (int e = required_value(a, o)) return e;
    return 0;
}

// one device, one .skf (validate_distance: exactly one positional, and of the selecting options what each mode below needs)
int run_distance(skx_ctx *ctx, const Args &a)
{
    const char *skf = a.pos[0].c_str();
    const double mf = atof(a.get("--min-freq", a.get("-m", "0")).c_str());
    const int filt_ambig = !a.has("--allow-ambiguous");
    char *buf = nullptr; uint64_t len = 0;
    int r, rcode = 0;
    const DistExtras dx(a);
    if (has_any(a, QUERY_OPTS)) {
        std::vector<std::string> names; std::vector<const char *> cn;
        if (int e = read_query_names(a, names)) return e;
        for (auto &n : names) cn.push_back(n.c_str());
        const std::string qskf = a.get("--query-skf");
        r = skh_distance_query_tsv(ctx, skf, a.has("--query-skf") ? qskf.c_str() : nullptr, cn.data(), (int)cn.size(), mf, filt_ambig, &buf, &len);
    }
    else if (a.has("--no-table")) return skh_distance_banded_files(ctx, skf, mf, filt_ambig, dx.get()) != SKX_OK ? engine_fail() : 0;
    else if (a.has("--sites")) {
        const skx_select_spec sp = select_spec(a);
        const skx_mst_spec ms{sp.max_snps, sp.max_mismatches, 0};
        const unsigned long long cap = a.has("--sites-max") ? strtoull(a.get("--sites-max").c_str(), nullptr, 10) : 1ull << 27;
        r = skh_distance_sites(ctx, skf, mf, a.has("--mst") ? nullptr : &sp, a.has("--mst") ? &ms : nullptr, a.get("--sites").c_str(), cap, &buf, &len);
        if (buf) { rcode = emit(a.get("-o"), buf, len); skx_free(buf); }                        // the table's lines stand even when the sites are refused
        return r != SKX_OK ? engine_fail() : rcode;
    }
    else if (a.has("--mst")) {
        const skx_select_spec ss = select_spec(a);
        const skx_mst_spec sp{ss.max_snps, ss.max_mismatches, 0};
        std::vector<double> lv;
        if (a.has("--mst-clusters")) (void)parse_levels(a.get("--levels", MST_DEFAULT_LEVELS), lv);      // (validate_distance took the list)
        char *csv = nullptr; uint64_t csv_len = 0;
        if (distance_mst_run(ctx, skf, mf, filt_ambig, &sp, lv.data(), (int)lv.size(), &buf, &len, &csv, &csv_len) != SKX_OK) return engine_fail();
        rcode = emit(a.get("-o"), buf, len); skx_free(buf);
        if (csv && !rcode && write_text_file(a.get("--mst-clusters") + ".levels.csv", csv, csv_len) != SKX_OK) rcode = engine_fail();
        skx_free(csv);
        return rcode;
    }
    else if (has_any(a, SELECT_OPTS)) { const skx_select_spec sp = select_spec(a); r = skh_distance_select_tsv(ctx, skf, mf, filt_ambig, &sp, &buf, &len); }
    else r = skh_distance_skf_tsv_extras(ctx, skf, mf, filt_ambig, dx.get(), &buf, &len);
    if (r != SKX_OK) return engine_fail();
    rcode = emit(a.get("-o"), buf, len); skx_free(buf);
    return rcode;
}
}  // namespace skh
