// ska_tree.cpp -- what `ska distance --tree / --clusters` writes from the engine's results, on the host: the Newick text of the joins of
// skx_dist_nj (negative-length rule, midpoint root, fixed child order) and the single-linkage clusters of the distance table (a union-find
// over a table the CLI already holds is cheaper than formatting that table, so there is no kernel here).  The reference leaves both to
// scripts/cluster_dists.py (networkx + rapidnj + biopython); its thresholds, CSV header and rooting are kept, the orders are fixed here.
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
std::string newick_name(const char *name)
{
    const std::string s = name;
    if (s.find_first_of("()[]':;, \t\n\r\v\f") == std::string::npos) return s;
    std::string o = "'";
    for (char c : s) { if (c == '\'') o += '\''; o += c; }
    return o + "'";
}
struct Edge { uint32_t to; double len; };
}  // namespace

extern "C" int skh_nj_newick(const char *const *names, const skx_nj_join *joins, int n_, char **buf, uint64_t *len)
{
    if (!names || !joins || !buf || !len || n_ < 2) { set_error("skh_nj_newick: bad arguments (at least 2 leaves)"); return SKX_EINVAL; }
    const uint32_t n = (uint32_t)n_, N = 2 * n - 2;                // nodes of the unrooted tree: n leaves, n - 2 inner
    std::vector<std::vector<Edge>> adj(N + 1);                     // (+ 1: the root, placed below)
    auto link = [&](uint32_t x, uint32_t y, double l) { adj[x].push_back({y, l}); adj[y].push_back({x, l}); };
    for (uint32_t t = 0; t + 1 < n; t++) {
        const skx_nj_join &j = joins[t];
        const uint32_t u = n + t;
        if (j.a >= u || j.b >= u || j.a == j.b) { set_error("skh_nj_newick: join %u names a node that does not exist yet", t); return SKX_EINVAL; }
        // Kuhner-Felsenstein: a negative branch becomes 0 and its sibling takes the difference
        double la = j.len_a, lb = j.len_b;
        if (la < 0) { lb += la; la = 0; }
        if (lb < 0) { la += lb; lb = 0; }
        if (la < 0) la = 0;
        if (t + 2 < n) { link(u, j.a, la); link(u, j.b, lb); }
        else link(j.a, j.b, la + lb);                              // the last record: one edge between the two nodes left
    }
    // the two leaves furthest apart, ties to the lowest (id, id): distances accumulated outwards from the lower leaf
    std::vector<double> dist(N); std::vector<uint32_t> par(N), stack; stack.reserve(N);
    double best = -1; uint32_t bx = 0, by = 1;
    for (uint32_t x = 0; x + 1 < n; x++) {
        stack.assign(1, x); dist[x] = 0; par[x] = x;
        while (!stack.empty()) {
            const uint32_t v = stack.back(); stack.pop_back();
            if (v < n && v > x && dist[v] > best) { best = dist[v]; bx = x; by = v; }
            else if (v < n && v > x && dist[v] == best && bx == x && v < by) by = v;
            for (const Edge &e : adj[v]) if (e.to != par[v]) { par[e.to] = v; dist[e.to] = dist[v] + e.len; stack.push_back(e.to); }
        }
    }
    // the path bx -> by, and the first edge on it that reaches half the distance
    {
        stack.assign(1, bx); par[bx] = bx; dist[bx] = 0;
        while (!stack.empty()) {
            const uint32_t v = stack.back(); stack.pop_back();
            for (const Edge &e : adj[v]) if (e.to != par[v]) { par[e.to] = v; dist[e.to] = dist[v] + e.len; stack.push_back(e.to); }
        }
    }
    std::vector<uint32_t> path;
    for (uint32_t v = by; ; v = par[v]) { path.push_back(v); if (v == bx) break; }
    std::reverse(path.begin(), path.end());
    const double half = dist[by] / 2;
    uint32_t p = path[0], q = path[1]; double lp = 0, lq = 0;
    for (size_t i = 0; i + 1 < path.size(); i++) {
        p = path[i]; q = path[i + 1];
        if (dist[q] >= half || i + 2 == path.size()) { lp = half - dist[p]; lq = dist[q] - half; break; }
    }
    if (lp < 0) lp = 0;
    if (lq < 0) lq = 0;
    const uint32_t root = N;
    for (Edge &e : adj[p]) if (e.to == q) { e.to = root; e.len = lp; break; }
    for (Edge &e : adj[q]) if (e.to == p) { e.to = root; e.len = lq; break; }
    adj[root].push_back({p, lp}); adj[root].push_back({q, lq});
    // rooted: parents first, then the lowest leaf below every node, bottom-up
    std::vector<uint32_t> order, parent(N + 1), low(N + 1); std::vector<double> blen(N + 1, 0.0);
    order.reserve(N + 1); order.push_back(root); parent[root] = root;
    for (size_t i = 0; i < order.size(); i++) {
        const uint32_t v = order[i];
        for (const Edge &e : adj[v]) if (e.to != parent[v]) { parent[e.to] = v; blen[e.to] = e.len; order.push_back(e.to); }
    }
    for (uint32_t v = 0; v <= N; v++) low[v] = v < n ? v : 0xFFFFFFFFu;
    for (size_t i = order.size(); i-- > 1;) { const uint32_t v = order[i]; low[parent[v]] = std::min(low[parent[v]], low[v]); }
    std::vector<std::vector<uint32_t>> kids(N + 1);
    for (size_t i = 1; i < order.size(); i++) kids[parent[order[i]]].push_back(order[i]);
    for (auto &k : kids) std::sort(k.begin(), k.end(), [&](uint32_t x, uint32_t y) { return low[x] < low[y]; });
    // the text, with an explicit stack (a caterpillar tree is as deep as it has leaves)
    std::string o; char tmp[64];
    struct Frame { uint32_t v; size_t next; };
    std::vector<Frame> fs; fs.push_back({root, 0});
    while (!fs.empty()) {
        Frame &f = fs.back();
        const uint32_t v = f.v;
        if (kids[v].empty() || f.next == kids[v].size()) {
            if (kids[v].empty()) o += newick_name(names[v]); else o += ')';
            if (v != root) { snprintf(tmp, sizeof tmp, ":%.5f", blen[v]); o += tmp; }
            fs.pop_back();
            continue;
        }
        o += f.next == 0 ? '(' : ',';
        const uint32_t c = kids[v][f.next++];
        fs.push_back({c, 0});
    }
    o += ";\n";
    return to_buf(o, buf, len);
}

extern "C" int skh_clusters_csv(const char *const *names, const uint32_t *labels, int n_, char **csv, uint64_t *csv_len)
{
    if (!names || !labels || n_ < 1 || !csv || !csv_len) { set_error("skh_clusters_csv: bad arguments"); return SKX_EINVAL; }
    const uint32_t n = (uint32_t)n_;
    for (uint32_t i = 0; i < n; i++)
        if (labels[i] > i || labels[labels[i]] != labels[i]) { set_error("skh_clusters_csv: label %u of sample %u is not the lowest sample of a cluster", labels[i], i); return SKX_EINVAL; }
    // clusters by size descending, ties by their lowest sample
    std::vector<uint32_t> size(n, 0), roots;
    for (uint32_t i = 0; i < n; i++) size[labels[i]]++;
    for (uint32_t i = 0; i < n; i++) if (labels[i] == i) roots.push_back(i);
    std::stable_sort(roots.begin(), roots.end(), [&](uint32_t x, uint32_t y) { return size[x] > size[y]; });
    std::vector<std::vector<uint32_t>> members(n);
    for (uint32_t i = 0; i < n; i++) members[labels[i]].push_back(i);
    std::string c = "id,Cluster__autocolour\n";
    for (size_t k = 0; k < roots.size(); k++)
        for (uint32_t i : members[roots[k]]) {
            const std::string s = names[i];
            if (s.find_first_of(",\"\n\r") != std::string::npos) { c += '"'; for (char ch : s) { if (ch == '"') c += '"'; c += ch; } c += '"'; }
            else c += s;
            c += "," + std::to_string(k + 1) + "\n";
        }
    return to_buf(c, csv, csv_len);
}

extern "C" int skh_mst_levels_csv(const char *const *names, const skx_dist_pair *pairs, uint64_t n_pairs, int n_, const double *levels, int n_levels, char **buf, uint64_t *len)
{
    if (!names || (!pairs && n_pairs) || n_ < 1 || !levels || n_levels < 1 || !buf || !len) { set_error("skh_mst_levels_csv: bad arguments"); return SKX_EINVAL; }
    const uint32_t n = (uint32_t)n_;
    for (uint64_t p = 0; p < n_pairs; p++)
        if (pairs[p].i >= pairs[p].j || pairs[p].j >= n) { set_error("skh_mst_levels_csv: line %llu does not join two of the %u samples", (unsigned long long)p, n); return SKX_EINVAL; }
    // the values the table shows, as skh_distance_clusters reads them
    std::vector<double> printed(n_pairs);
    char tmp[512];
    for (uint64_t p = 0; p < n_pairs; p++) { snprintf(tmp, sizeof tmp, "%.2f", pairs[p].d.distance); printed[p] = strtod(tmp, nullptr); }
    std::vector<std::vector<uint32_t>> column((size_t)n_levels, std::vector<uint32_t>(n));
    std::string c = "id";
    for (int l = 0; l < n_levels; l++) {
        snprintf(tmp, sizeof tmp, ",snps_%g", levels[l]); c += tmp;
        std::vector<uint32_t> up(n), number(n, 0);
        std::iota(up.begin(), up.end(), 0u);
        auto find = [&](uint32_t x) { while (up[x] != x) { up[x] = up[up[x]]; x = up[x]; } return x; };
        for (uint64_t p = 0; p < n_pairs; p++) {
            if (!(printed[p] <= levels[l])) continue;
            const uint32_t a = find(pairs[p].i), b = find(pairs[p].j);
            if (a != b) up[std::max(a, b)] = std::min(a, b);       // the root of a cluster is its lowest sample
        }
        uint32_t next = 0;
        for (uint32_t i = 0; i < n; i++) { const uint32_t r = find(i); if (r == i) number[i] = ++next; column[l][i] = number[r]; }      // (r <= i: numbered already)
    }
    c += ",address\n";
    for (uint32_t i = 0; i < n; i++) {
        const std::string s = names[i];
        if (s.find_first_of(",\"\n\r") != std::string::npos) { c += '"'; for (char ch : s) { if (ch == '"') c += '"'; c += ch; } c += '"'; }
        else c += s;
        std::string address;
        for (int l = 0; l < n_levels; l++) { const std::string v = std::to_string(column[l][i]); c += "," + v; address += (l ? "." : "") + v; }
        c += "," + address + "\n";
    }
    return to_buf(c, buf, len);
}

extern "C" int skh_distance_clusters(const char *const *names, const skx_dist *d, int n_, double max_snps, double max_mismatches,
                                     char **csv, uint64_t *csv_len, char **dot, uint64_t *dot_len)
{
    if (!names || (!d && n_ > 1) || n_ < 1 || (csv && !csv_len) || (dot && !dot_len)) { set_error("skh_distance_clusters: bad arguments"); return SKX_EINVAL; }
    const uint32_t n = (uint32_t)n_;
    std::vector<uint32_t> up(n);
    std::iota(up.begin(), up.end(), 0u);
    auto find = [&](uint32_t x) { while (up[x] != x) { up[x] = up[up[x]]; x = up[x]; } return x; };
    auto dot_name = [](const char *s) { std::string o = "\""; for (; *s; s++) { if (*s == '"' || *s == '\\') o += '\\'; o += *s; } return o + "\""; };
    std::string g = "strict graph {\n";
    std::vector<std::string> dn(n);
    for (uint32_t i = 0; i < n; i++) { dn[i] = dot_name(names[i]); g += "\t" + dn[i] + ";\n"; }
    size_t p = 0; char tmp[64];
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t j = i + 1; j < n; j++, p++) {
            // the values the table shows, not the ones behind them: the partition is then the one the script makes of that table
            snprintf(tmp, sizeof tmp, "%.2f", d[p].distance); const double snps = strtod(tmp, nullptr);
            snprintf(tmp, sizeof tmp, "%.5f", d[p].mismatch_prop); const double mism = strtod(tmp, nullptr);
            if (!(snps <= max_snps && mism <= max_mismatches)) continue;
            g += "\t" + dn[i] + " -- " + dn[j] + ";\n";
            const uint32_t a = find(i), b = find(j);
            if (a != b) up[std::max(a, b)] = std::min(a, b);       // the root of a cluster is its lowest sample
        }
    g += "}\n";
    for (uint32_t i = 0; i < n; i++) up[i] = find(i);
    int r = SKX_OK;
    if (csv) r = skh_clusters_csv(names, up.data(), n_, csv, csv_len);
    if (r == SKX_OK && dot) r = to_buf(g, dot, dot_len);
    return r;
}
