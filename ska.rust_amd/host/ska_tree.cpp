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

// ---- a user's tree: Newick in (skh_newick_joins), and the tree out again with a count per branch as branch lengths
namespace {
// what the two writers need of a join table: parents, the hidden node Y of a trifurcating root, leaves below, lowest leaf
struct JoinTree {
    uint32_t S, root, hidden;                                      // hidden: 2S-3 when the text's root had three children, else no node
    const skx_tree_join *j;
    std::vector<uint32_t> parent, leaves, low;
    std::vector<uint64_t> len;                                     // the changes a branch is reported with
    JoinTree(const skx_tree_join *joins, uint32_t n, bool three, const uint64_t *changes)
        : S(n), root(2 * n - 2), hidden(three ? 2 * n - 3 : 0xFFFFFFFFu), j(joins), parent(2 * n - 1, 2 * n - 2), leaves(2 * n - 1, 1), low(2 * n - 1), len(2 * n - 2, 0)
    {
        for (uint32_t v = 0; v < S; v++) low[v] = v;
        for (uint32_t t = 0; t + 1 < S; t++) {
            parent[j[t].a] = parent[j[t].b] = S + t;
            leaves[S + t] = leaves[j[t].a] + leaves[j[t].b]; low[S + t] = std::min(low[j[t].a], low[j[t].b]);
        }
        for (uint32_t c = 0; c < root; c++) len[owner(c)] += changes[c];
    }
    uint32_t owner(uint32_t c) const { return c == hidden ? j[S - 2].a : c; }      // the hidden node's changes go to the root's first child
    uint32_t shown_parent(uint32_t c) const { return parent[c] == hidden ? root : parent[c]; }
    std::vector<uint32_t> kids(uint32_t v) const
    {
        const skx_tree_join &x = j[v - S];
        if (v == root && hidden != 0xFFFFFFFFu) return {x.a, j[x.b - S].a, j[x.b - S].b};
        return {x.a, x.b};
    }
    std::string label(const char *const *names, uint32_t c) const { return c < S ? names[c] : c == root ? "root" : "n" + std::to_string(c - S + 1); }
};
int bad(size_t at, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int bad(size_t at, const char *fmt, ...)                           // what skh_newick_joins refuses, with the place in the text
{
    char m[600];
    va_list ap; va_start(ap, fmt); vsnprintf(m, sizeof m, fmt, ap); va_end(ap);
    set_error("newick: position %zu: %s", at, m);
    return SKX_EINVAL;
}
int check_join_table(const char *who, const skx_tree_join *joins, int n_, int root_three)
{
    const uint32_t n = (uint32_t)n_;
    std::vector<char> used(2 * n - 1, 0);
    for (uint32_t t = 0; t + 1 < n; t++)
        for (const uint32_t c : {joins[t].a, joins[t].b}) {
            if (c >= n + t || used[c]) { set_error("%s: join %u names a node that does not exist yet, or a child for the second time", who, t); return SKX_EINVAL; }
            used[c] = 1;
        }
    if (root_three && (n < 3 || joins[n - 2].b != 2 * n - 3)) { set_error("%s: a trifurcating root is the join (a, 2S-3)", who); return SKX_EINVAL; }
    return SKX_OK;
}
}  // namespace

extern "C" int skh_newick_joins(const char *text, const char *const *names, int n_, skx_tree_join *joins, int *root_three)
{
    return guarded([&]() -> int {
    if (root_three) *root_three = 0;
    if (!text || !names || !joins || n_ < 2) { set_error("newick: bad arguments (at least 2 samples)"); return SKX_EINVAL; }
    const uint32_t S = (uint32_t)n_;
    const size_t n = strlen(text);
    // names -> samples: the first of two equal names wins, as everywhere
    std::vector<uint32_t> by_name(S);
    std::iota(by_name.begin(), by_name.end(), 0u);
    std::stable_sort(by_name.begin(), by_name.end(), [&](uint32_t x, uint32_t y) { return strcmp(names[x], names[y]) < 0; });
    auto find = [&](const std::string &s) -> int64_t {
        auto it = std::lower_bound(by_name.begin(), by_name.end(), s, [&](uint32_t x, const std::string &v) { return v.compare(names[x]) > 0; });
        return it != by_name.end() && s == names[*it] ? (int64_t)*it : -1;
    };
    static const char SPECIAL[] = "()[]':;, \t\n\r\v\f";
    auto special = [&](char c) { return c == 0 || strchr(SPECIAL, c) != nullptr; };
    std::vector<char> seen(S, 0);
    // an explicit stack (a caterpillar tree is as deep as it has leaves): the children of every open node, one run of `kids` each
    std::vector<uint32_t> kids; std::vector<size_t> open;          // open[d] = where the children of the d-th open node begin in kids
    size_t pos = 0; uint32_t made = 0; bool have_root = false, after = false, three = false;
    auto skip = [&]() -> bool {                                    // white space and [comments]; false: a comment without its end
        while (pos < n) {
            if (strchr(" \t\n\r\v\f", text[pos])) pos++;
            else if (text[pos] == '[') { const char *e = strchr(text + pos, ']'); if (!e) return false; pos = (size_t)(e - text) + 1; }
            else break;
        }
        return true;
    };
    // 0: a label (maybe empty) in `out`; else the error is set
    auto label = [&](std::string &out, bool &quoted) -> int {
        out.clear(); quoted = false;
        if (!skip()) return bad(pos, "a comment without its end");
        if (pos < n && text[pos] == '\'') {
            const size_t at = pos++; quoted = true;
            for (;;) {
                if (pos >= n) return bad(at, "a quoted label without its end");
                if (text[pos] == '\'') { if (pos + 1 < n && text[pos + 1] == '\'') { out += '\''; pos += 2; continue; } pos++; return 0; }
                out += text[pos++];
            }
        }
        const size_t s = pos;
        while (pos < n && !special(text[pos])) pos++;
        out.assign(text + s, pos - s);
        return 0;
    };
    // a node has closed: its branch length is read and dropped, and it becomes a child of the innermost open node, or the root
    auto closed = [&](uint32_t node) -> int {
        if (!skip()) return bad(pos, "a comment without its end");
        if (pos < n && text[pos] == ':') { pos++; if (!skip()) return bad(pos, "a comment without its end"); while (pos < n && !special(text[pos])) pos++; }
        after = true;
        if (!open.empty()) kids.push_back(node); else have_root = true;
        return 0;
    };
    std::string name; bool quoted;
    for (;;) {
        if (!skip()) return bad(pos, "a comment without its end");
        if (pos >= n) return bad(pos, "the text ends inside the tree");
        const char ch = text[pos];
        if (have_root) {
            if (ch != ';') return bad(pos, "text after the tree");
            pos++;
            if (!skip()) return bad(pos, "a comment without its end");
            if (pos < n) return bad(pos, "text after the tree");
            break;
        }
        if (after && ch != ',' && ch != ')' && ch != ';') return bad(pos, "unexpected character '%c'", ch);
        if (ch == '(') { open.push_back(kids.size()); pos++; }
        else if (ch == ',') {
            if (!after) return bad(pos, "a ',' without a node before it");
            after = false; pos++;
            if (!skip()) return bad(pos, "a comment without its end");
            if (pos < n && (text[pos] == ',' || text[pos] == ')')) return bad(pos, "a leaf without a name");
        }
        else if (ch == ')') {
            const size_t at = pos++;
            if (open.empty()) return bad(at, "a ')' without its '('");
            const size_t first = open.back(), k = kids.size() - first;
            open.pop_back();
            if (k == 1) return bad(at, "a node with one child");
            if (k == 0) return bad(at, "a leaf without a name");
            if (k != 2 && !(k == 3 && open.empty())) return bad(at, "a node with %zu children (only the root may have three)", k);
            if (made + (k - 1) > S - 1) return bad(at, "more nodes than %u samples can have", S);
            if (k == 3) { joins[made] = {kids[first + 1], kids[first + 2]}; joins[made + 1] = {kids[first], S + made}; made += 2; three = true; }
            else { joins[made] = {kids[first], kids[first + 1]}; made++; }
            kids.resize(first);
            if (int e = label(name, quoted)) return e;             // an inner label: read and dropped
            if (int e = closed(S + made - 1)) return e;
        }
        else if (ch == ';') return bad(pos, "%s", open.empty() ? "a tree without a node" : "the tree ends inside a node");
        else {
            const size_t at = pos;
            if (int e = label(name, quoted)) return e;
            if (name.empty() && !quoted) return bad(at, "unexpected character '%c'", ch);
            const int64_t s = find(name);
            if (s < 0) return bad(at, "leaf '%s' is not a sample of the array", name.c_str());
            if (seen[s]) return bad(at, "sample '%s' is named twice", name.c_str());
            seen[s] = 1;
            if (int e = closed((uint32_t)s)) return e;
        }
    }
    for (uint32_t s = 0; s < S; s++) if (!seen[s]) { set_error("newick: sample '%s' is missing from the tree", names[s]); return SKX_EINVAL; }
    if (made != S - 1) { set_error("newick: the tree does not join all samples"); return SKX_EINVAL; }
    if (root_three) *root_three = three;
    return SKX_OK;
    });
}

extern "C" int skh_parsimony_newick(const char *const *names, const skx_tree_join *joins, int n_, int root_three, const uint64_t *branch_changes, char **buf, uint64_t *len)
{
    return guarded([&]() -> int {
    if (!names || !joins || !branch_changes || !buf || !len || n_ < 2) { set_error("skh_parsimony_newick: bad arguments (at least 2 leaves)"); return SKX_EINVAL; }
    if (int e = check_join_table("skh_parsimony_newick", joins, n_, root_three)) return e;
    const JoinTree tr(joins, (uint32_t)n_, root_three != 0, branch_changes);
    // the text, with an explicit stack (a caterpillar tree is as deep as it has leaves)
    std::string o;
    struct Frame { uint32_t v; std::vector<uint32_t> kids; size_t next; };
    std::vector<Frame> fs; fs.push_back({tr.root, tr.kids(tr.root), 0});
    while (!fs.empty()) {
        Frame &f = fs.back();
        const uint32_t v = f.v;
        if (f.next == f.kids.size()) {
            if (v < tr.S) o += newick_name(names[v]); else { o += ')'; if (v != tr.root) o += tr.label(names, v); }
            if (v != tr.root) { o += ':'; o += std::to_string(tr.len[v]); }
            fs.pop_back();
            continue;
        }
        o += f.next == 0 ? '(' : ',';
        const uint32_t c = f.kids[f.next++];
        fs.push_back({c, c < tr.S ? std::vector<uint32_t>() : tr.kids(c), 0});
    }
    o += ";\n";
    return to_buf(o, buf, len);
    });
}

extern "C" int skh_parsimony_branches(const char *const *names, const skx_tree_join *joins, int n_, int root_three, const uint64_t *branch_changes, char **buf, uint64_t *len)
{
    return guarded([&]() -> int {
    if (!names || !joins || !branch_changes || !buf || !len || n_ < 2) { set_error("skh_parsimony_branches: bad arguments (at least 2 leaves)"); return SKX_EINVAL; }
    if (int e = check_join_table("skh_parsimony_branches", joins, n_, root_three)) return e;
    const JoinTree tr(joins, (uint32_t)n_, root_three != 0, branch_changes);
    std::string o = "Node\tParent\tLeaves\tLowest leaf\tChanges\n";
    for (uint32_t c = 0; c < tr.root; c++) {
        if (c == tr.hidden) continue;
        o += tr.label(names, c); o += '\t'; o += tr.label(names, tr.shown_parent(c)); o += '\t'; o += std::to_string(tr.leaves[c]); o += '\t';
        o += names[tr.low[c]]; o += '\t'; o += std::to_string(tr.len[c]); o += '\n';
    }
    return to_buf(o, buf, len);
    });
}
