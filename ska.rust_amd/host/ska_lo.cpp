// ska_lo.cpp -- `ska lo` (generic_modes.rs:286-306, src/skalo/*.rs) above the device graph of csrc/skx_lo.hip: compaction
// (compaction.rs), the depth-bounded DFS from every entry node (read_graph.rs:build_variant_groups), indels (process_indels.rs), SNPs
// (process_variants.rs, positioning.rs, output_snps.rs).  Where the reference's output order follows hash-map iteration the engine fixes
// one order; the DFS runs on `threads` host threads into per-entry slots merged in entry order, so the output does not
// depend on the thread count.
#include "../../include/skx_host.h"
#include "../csrc/skx_internal.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace {
typedef unsigned __int128 u128;
const char CODE[4] = {'A', 'C', 'T', 'G'};

u128 rc_n(u128 v, int n)
{
    u128 out = 0;
    for (int i = 0; i < n; i++) { out = (out << 2) | (u128)((uint32_t)(v & 3) ^ 2u); v >>= 2; }
    return out;
}
u128 encode(const char *s, size_t n)
{
    u128 v = 0;
    for (size_t i = 0; i < n; i++) v = (v << 2) | (u128)(((unsigned char)s[i] >> 1) & 3);
    return v;
}
std::string decode(u128 v, int n)
{
    std::string s(n, 'A');
    for (int i = n - 1; i >= 0; i--) { s[i] = CODE[(uint32_t)(v & 3)]; v >>= 2; }
    return s;
}
struct H128 { size_t operator()(u128 x) const { const uint64_t a = (uint64_t)x, b = (uint64_t)(x >> 64); return std::hash<uint64_t>()(a * 0x9E3779B97F4A7C15ull ^ b); } };

struct Variant { std::string seq; std::vector<size_t> snps; };
typedef std::vector<Variant> Group;
typedef std::pair<uint32_t, uint32_t> Ends;     // (entry, exit) node indices; index order == node value order

void info(const char *target, const std::string &m) { skh_log(2, target, m.c_str()); }

struct Lo {
    int k = 0, kg = 0; uint64_t S = 0, W = 0;
    std::vector<u128> val;                       // every node (sources and destinations), ascending
    std::vector<std::vector<uint32_t>> adj;      // neighbours (indices); empty for nodes without out-edges
    std::vector<uint8_t> is_entry, is_exit;
    std::vector<uint32_t> entries, exits;        // ascending
    std::unordered_map<uint32_t, std::vector<uint32_t>> compacted;
    size_t max_depth = 4;

    uint32_t idx(u128 v) const { return (uint32_t)(std::lower_bound(val.begin(), val.end(), v) - val.begin()); }

    void compact()
    {
        std::map<uint32_t, std::vector<uint32_t>> chains;
        for (const auto *list : {&entries, &exits})
            for (uint32_t node : *list)
                for (uint32_t s : adj[node]) {
                    uint32_t cur = s; std::unordered_set<uint32_t> seen; std::vector<uint32_t> chain;
                    for (;;) {
                        const auto &nx = adj[cur];
                        if (nx.size() == 1 && !seen.count(nx[0])) {
                            cur = nx[0]; chain.push_back(cur); seen.insert(cur);
                            if (is_exit[cur] || is_entry[cur]) break;
                        } else break;
                    }
                    if (chain.size() > 1) chains[s] = chain;
                }
        auto drop = [&](uint32_t from, uint32_t to) { auto &v = adj[from]; v.erase(std::remove(v.begin(), v.end(), to), v.end()); };
        for (auto &kv : chains) {                            // ascending first node
            auto &chain = kv.second;
            drop(kv.first, chain[0]);
            for (size_t i = 0; i + 2 < chain.size(); i++) drop(chain[i], chain[i + 1]);
            adj[kv.first].push_back(chain.back());
            chain.pop_back();
            compacted[kv.first] = chain;
        }
    }

    void extend(std::vector<uint32_t> &path, uint32_t n) const
    {
        auto it = compacted.find(n);
        if (it != compacted.end()) path.insert(path.end(), it->second.begin(), it->second.end());
    }

    // read_graph.rs:build_variant_groups for one entry node: the groups (entry, exit) it opens, by exit
    std::vector<std::pair<Ends, Group>> traverse(uint32_t e) const
    {
        struct State { uint32_t cur; std::unordered_set<uint32_t> seen; std::vector<uint32_t> path; size_t depth; };
        std::map<uint32_t, std::vector<std::vector<uint32_t>>> found;
        std::vector<uint32_t> good;
        for (uint32_t s : adj[e]) {
            std::vector<State> stack;
            State st{s, {e, s}, {e, s}, 0};
            extend(st.path, s);
            stack.push_back(std::move(st));
            while (!stack.empty()) {
                State cs = std::move(stack.back()); stack.pop_back();
                if (cs.depth > max_depth) continue;
                for (;;) {
                    good.clear();
                    for (uint32_t n : adj[cs.cur]) if (!cs.seen.count(n)) good.push_back(n);
                    if (good.size() == 1) {
                        const uint32_t nx = good[0];
                        cs.seen.insert(nx); cs.path.push_back(nx); cs.cur = nx;
                        extend(cs.path, nx);
                        if (is_exit[nx]) found[nx].push_back(cs.path);
                    } else if (good.size() > 1) {
                        const std::vector<uint32_t> g = good;
                        for (uint32_t nx : g) {
                            State ns{nx, cs.seen, cs.path, cs.depth + 1};
                            ns.seen.insert(nx); ns.path.push_back(nx);
                            extend(ns.path, nx);
                            if (is_exit[nx]) found[nx].push_back(ns.path);
                            stack.push_back(std::move(ns));
                        }
                        break;
                    } else break;
                }
            }
        }
        std::vector<std::pair<Ends, Group>> out;
        bool any = false;
        for (auto &kv : found) any |= kv.second.size() > 1;
        if (!any) return out;
        for (auto &kv : found) {
            const auto &paths = kv.second;
            std::set<uint32_t> second, stl;
            for (auto &p : paths) { second.insert(p[1]); stl.insert(p[p.size() - 2]); }
            if (second.size() < 2 || stl.size() < 2) continue;
            std::map<size_t, size_t> cnt;
            for (auto &p : paths) cnt[p.size()]++;
            size_t mcl = 0, best = 0;
            for (auto &c : cnt) if (c.second > best) { best = c.second; mcl = c.first; }     // ascending lengths: a tie keeps the shortest
            Group g;
            for (auto &p : paths) {
                if (paths.size() != 2 && p.size() != mcl) continue;
                Variant v;
                v.seq = decode(val[e], kg);
                for (size_t i = 1; i < p.size(); i++) v.seq.push_back(CODE[(uint32_t)(val[p[i]] & 3)]);
                for (size_t i = 0; i < p.size(); i++) {
                    if (is_entry[p[i]] && (p.size() < (size_t)kg || i <= p.size() - kg)) v.snps.push_back(i + kg);
                    else if (is_exit[p[i]]) v.snps.push_back(i - 1);
                }
                g.push_back(std::move(v));
            }
            out.emplace_back(Ends(e, kv.first), std::move(g));
        }
        return out;
    }
};

struct Colours {
    uint64_t W = 0;
    std::unordered_map<u128, std::vector<uint64_t>, H128> map;
    const std::vector<uint64_t> *get(u128 km) const { auto it = map.find(km); return it == map.end() ? nullptr : &it->second; }
};
bool bit(const std::vector<uint64_t> &c, uint64_t i) { return (c[i >> 6] >> (i & 63)) & 1; }
uint64_t popcount(const std::vector<uint64_t> &c) { uint64_t n = 0; for (uint64_t w : c) n += __builtin_popcountll(w); return n; }
float f32_ratio(uint64_t a, uint64_t b) { return (float)a / (float)b; }

int gather(skx_lo_graph *g, int wpn, const std::vector<u128> &want, Colours &out)
{
    std::vector<u128> q(want);
    std::sort(q.begin(), q.end());
    q.erase(std::unique(q.begin(), q.end()), q.end());
    std::vector<uint64_t> words(q.size() * wpn), cols(q.size() * out.W);
    for (size_t i = 0; i < q.size(); i++) { words[i * wpn] = (uint64_t)q[i]; if (wpn == 2) words[i * 2 + 1] = (uint64_t)(q[i] >> 64); }
    std::vector<uint8_t> found(q.size());
    if (!q.empty()) { int r = skx_lo_gather(g, words.data(), q.size(), cols.data(), found.data()); if (r != SKX_OK) return r; }
    for (size_t i = 0; i < q.size(); i++)
        if (found[i]) out.map.emplace(q[i], std::vector<uint64_t>(cols.begin() + i * out.W, cols.begin() + (i + 1) * out.W));
    return SKX_OK;
}

std::string join(const std::vector<std::string> &v, const char *sep)
{
    std::string s;
    for (size_t i = 0; i < v.size(); i++) { if (i) s += sep; s += v[i]; }
    return s;
}

int write_file(const std::string &path, const std::string &text)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(text.data(), 1, text.size(), f) != text.size()) { if (f) fclose(f); skx::set_error("Unable to create %s", path.c_str()); return SKX_EIO; }
    fclose(f);
    return SKX_OK;
}

// process_indels.rs:extract_middle_bases
std::pair<std::vector<std::string>, std::string> middle_bases(const Group &g, int kg)
{
    std::vector<std::string> red;
    for (auto &v : g) red.push_back(v.seq.substr(kg));
    size_t n = 0; bool identical = true;
    while (identical) {
        n++;
        std::set<std::string> ends;
        for (auto &s : red) { if (n > s.size()) identical = false; else ends.insert(s.substr(s.size() - n)); }
        if (ends.size() > 1) identical = false;
    }
    n--;
    std::string last = red[0].substr(red[0].size() - n);
    if (last.size() > (size_t)kg) last.resize(kg);
    std::vector<std::string> mid;
    for (auto &s : red) { std::string m = s.substr(0, s.size() - n); mid.push_back(m.empty() ? "-" : m); }
    return {mid, last};
}

// positioning.rs:most_frequent_position
std::pair<uint32_t, size_t> most_frequent(const std::vector<uint32_t> &v)
{
    std::map<uint32_t, size_t> c;
    for (uint32_t x : v) c[x]++;
    size_t best = 0, ties = 0; uint32_t pos = 0;
    for (auto &kv : c) { if (kv.second > best) { best = kv.second; pos = kv.first; ties = 1; } else if (kv.second == best) ties++; }
    if (ties > 1 || best < 10) return {0, 0};
    return {pos, best};
}

}  // namespace

extern "C" int skh_lo(skx_ctx *ctx, const char *skf_file, const char *reference, const char *out_prefix, float missing, size_t depth,
                      size_t indel_kmers, int threads)
{
    return skx_guarded([&]() -> int {
    if (!ctx || !skf_file || !out_prefix) { skx::set_error("bad arguments"); return SKX_EINVAL; }
    const char *RG = "ska::skalo::read_graph", *PV = "ska::skalo::process_variants";
    skx_array *a = nullptr;
    const char *in[1] = {skf_file};
    int r = skh_load_array(ctx, in, 1, 1, &a);
    if (r != SKX_OK) return r;
    std::unique_ptr<skx_array, void (*)(skx_array *)> own(a, skx_array_free);
    skx_array_info_t ai;
    SKX_TRY(skx_array_info(a, &ai));
    std::vector<std::string> names;
    for (uint64_t i = 0; i < ai.n_samples; i++) names.emplace_back(skx_array_name(a, i));
    Lo L; L.k = ai.k; L.kg = ai.k - 1; L.S = ai.n_samples; L.W = (L.S + 63) / 64; L.max_depth = depth;
    const int kg = L.kg, wpn = L.k <= 31 ? 1 : 2;
    info(RG, std::to_string(L.k) + "-mers");
    info(RG, std::to_string(L.S) + " samples");
    info(RG, "Building colored de Bruijn graph");
    skx_lo_graph *g = nullptr;
    SKX_TRY(skx_array_lo_graph(a, &g));
    std::unique_ptr<skx_lo_graph, void (*)(skx_lo_graph *)> gown(g, skx_lo_graph_free);
    skx_lo_info gi;
    SKX_TRY(skx_lo_graph_info(g, &gi));
    std::vector<uint64_t> nodes(gi.n_nodes * wpn), off(gi.n_nodes + 1), nb(gi.n_edges * wpn), ent(gi.n_entries * wpn), ex(gi.n_entries * wpn);
    SKX_TRY(skx_lo_graph_export(g, nodes.data(), off.data(), nb.data(), ent.data(), ex.data()));
    skx::PhaseTimer t_host("lo.host_graph");
    auto word = [&](const std::vector<uint64_t> &v, size_t i) -> u128 { return wpn == 1 ? (u128)v[i] : ((u128)v[2 * i + 1] << 64) | v[2 * i]; };
    for (size_t i = 0; i < gi.n_nodes; i++) L.val.push_back(word(nodes, i));
    for (size_t i = 0; i < gi.n_edges; i++) L.val.push_back(word(nb, i));
    std::sort(L.val.begin(), L.val.end());
    L.val.erase(std::unique(L.val.begin(), L.val.end()), L.val.end());
    L.adj.assign(L.val.size(), {});
    for (size_t i = 0; i < gi.n_nodes; i++) {
        auto &v = L.adj[L.idx(word(nodes, i))];
        for (uint64_t e = off[i]; e < off[i + 1]; e++) v.push_back(L.idx(word(nb, e)));
    }
    info(RG, std::to_string(gi.n_nodes) + " nodes");
    info("ska::skalo::extremities", "Identifying extremity nodes");
    if (gi.n_entries == 0) {
        skh_log(0, "ska::skalo::extremities", "Error: there is no entry node in this graph, hence no variant.\n");
        skx::set_error("there is no entry node in this graph, hence no variant");
        return SKX_EEMPTY;
    }
    info("ska::skalo::extremities", std::to_string(gi.n_entries) + " entry nodes");
    L.is_entry.assign(L.val.size(), 0); L.is_exit.assign(L.val.size(), 0);
    for (size_t i = 0; i < gi.n_entries; i++) { L.entries.push_back(L.idx(word(ent, i))); L.is_entry[L.entries.back()] = 1; }
    for (size_t i = 0; i < gi.n_entries; i++) { L.exits.push_back(L.idx(word(ex, i))); L.is_exit[L.exits.back()] = 1; }
    t_host.stop();

    info(RG, "Compacting graph");
    skx::PhaseTimer t_comp("lo.compact");
    L.compact();
    t_comp.stop();
    info(RG, "Traversing graph");
    skx::PhaseTimer t_dfs("lo.dfs");
    std::vector<std::vector<std::pair<Ends, Group>>> slots(L.entries.size());
    {
        std::atomic<size_t> next{0};
        auto work = [&]() { for (size_t i; (i = next.fetch_add(1)) < L.entries.size();) slots[i] = L.traverse(L.entries[i]); };
        std::vector<std::thread> th;
        for (int t = 1; t < std::max(1, threads); t++) th.emplace_back(work);
        work();
        for (auto &x : th) x.join();
    }
    std::map<Ends, Group> groups;
    for (auto &s : slots) for (auto &kv : s) groups.emplace(kv.first, std::move(kv.second));
    slots.clear();
    t_dfs.stop();
    info(RG, std::to_string(groups.size()) + " variant groups");
    info(RG, "Identifying indels");
    std::map<Ends, Group> finals, indels;
    for (auto &kv : groups) {
        const Group &vv = kv.second;
        if (vv.size() < 2) continue;
        if (vv.size() == 2 && vv[0].seq.size() != vv[1].seq.size()) {
            if (vv[0].seq.size() <= (size_t)(2 * kg) || vv[1].seq.size() <= (size_t)(2 * kg)) indels[kv.first] = vv;
        } else finals[kv.first] = vv;
    }
    groups.clear();

    // reference (positioning.rs:extract_genomic_kmers): one record, k-mers of k - 1 at up to 3 positions
    skx::PhaseTimer t_ref("lo.reference");
    std::string genome, gname;
    std::unordered_map<u128, std::vector<uint32_t>, H128> kmap;
    if (reference) {
        info(PV, "Reading reference genome");
        skx::HostStream hs;
        SKX_TRY(skx::read_sample_stream(reference, nullptr, 0.0, hs));
        if (hs.ids.size() > 1) { skx::set_error("\nError: more than one sequence detected in the reference genome file.\n"); return SKX_EINVAL; }
        gname = hs.ids.empty() ? "" : hs.ids[0];
        for (uint8_t c : hs.seq) if (!isspace(c)) genome.push_back((char)toupper(c));
        if (genome.size() >= (size_t)kg)
            for (size_t n = 0; n + kg <= genome.size(); n++) {
                bool ok = true;
                for (int j = 0; j < kg && ok; j++) ok = (genome[n + j] & 0xF) != 14;
                if (!ok) continue;
                auto &p = kmap[encode(genome.data() + n, kg)];
                if (p.size() < 3) p.push_back((uint32_t)(n + kg));
            }
    }
    t_ref.stop();

    // dereplicated indels and the paths the SNP pass keeps (they decide nothing from colours)
    // indels (process_indels.rs)
    std::vector<std::pair<size_t, Ends>> by_len;
    for (auto &kv : indels) { size_t t = 0; for (auto &v : kv.second) t += v.seq.size(); by_len.emplace_back(t, kv.first); }
    std::sort(by_len.begin(), by_len.end(), [&](const std::pair<size_t, Ends> &x, const std::pair<size_t, Ends> &y) {
        return x.first != y.first ? x.first < y.first : x.second < y.second; });
    std::unordered_set<u128, H128> taken;
    std::map<Ends, const Group *> final_indels;
    for (auto &t : by_len) {
        const u128 en = L.val[t.second.first], xn = L.val[t.second.second];
        if (taken.count(en)) continue;
        taken.insert(en); taken.insert(rc_n(en, kg)); taken.insert(xn); taken.insert(rc_n(xn, kg));
        final_indels[t.second] = &indels[t.second];
    }
    // paths with too many indel k-mers (process_variants.rs:find_internal_indels)
    for (auto &kv : finals) {
        Group kept;
        for (auto &v : kv.second) {
            size_t nb_in = 0;
            for (size_t i = 0; i + kg < v.seq.size(); i++) nb_in += taken.count(encode(v.seq.data() + i, kg));
            if (nb_in <= indel_kmers) kept.push_back(v);
        }
        kv.second.swap(kept);
    }
    // the colours any step below can ask for, in one batch: the indel alleles' first k bases, the SNP flanks
    skx::PhaseTimer t_gather("lo.colours");
    std::map<Ends, std::vector<size_t>> snp_pos;
    std::vector<u128> want;
    for (auto &kv : indels) for (auto &v : kv.second) if (v.seq.size() >= (size_t)L.k) want.push_back(encode(v.seq.data(), L.k));
    for (auto &kv : finals) {
        std::set<size_t> cand;
        for (auto &v : kv.second) cand.insert(v.snps.begin(), v.snps.end());
        std::vector<size_t> real;
        for (size_t pos : cand) {
            bool seen[4] = {false, false, false, false};
            for (auto &v : kv.second) if (pos < v.seq.size()) seen[((unsigned char)v.seq[pos] >> 1) & 3] = true;
            if (seen[0] + seen[1] + seen[2] + seen[3] > 1) real.push_back(pos);
        }
        for (size_t pos : real)
            for (auto &v : kv.second)
                if (pos >= (size_t)kg && pos + 1 <= v.seq.size()) want.push_back(encode(v.seq.data() + pos - kg, kg + 1));
        snp_pos[kv.first] = real;
    }
    Colours col; col.W = L.W;
    SKX_TRY(gather(g, wpn, want, col));
    t_gather.stop();

    skx::PhaseTimer t_out("lo.call");
    info("ska::skalo::process_indels", "Processing indels");
    std::string vcf = "##fileformat=VCFv4.2\n# REF corresponds to the most frequent variant among samples\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" +
                      join(names, "\t") + "\n";
    size_t n_indels = 0;
    for (auto &kv : final_indels) {
        const Group &vv = *kv.second;
        std::vector<const std::vector<uint64_t> *> bits;
        for (auto &v : vv) if (v.seq.size() >= (size_t)L.k) if (auto c = col.get(encode(v.seq.data(), L.k))) bits.push_back(c);
        if (bits.size() < 2) { skx::set_error("ska lo: an indel allele's k-mer is not in the graph"); return SKX_EINVAL; }
        uint64_t miss = 0; bool refp = false, altp = false;
        for (uint64_t i = 0; i < L.S; i++) {
            const bool x = bit(*bits[0], i), y = bit(*bits[1], i);
            if (x == y) miss++; else if (x) refp = true; else altp = true;
        }
        if (!(f32_ratio(miss, L.S) <= missing && refp && altp)) continue;
        n_indels++;
        auto mb = middle_bases(vv, kg);
        const std::string first = vv[0].seq.substr(0, kg);
        size_t ri = 0, ai = 1;
        if (popcount(*bits[1]) > popcount(*bits[0])) { ri = 1; ai = 0; }          // stable sort by count, descending
        std::vector<std::string> calls;
        for (uint64_t i = 0; i < L.S; i++) {
            const bool x = bit(*bits[ri], i), y = bit(*bits[ai], i);
            calls.push_back(x && y ? "0/1" : x ? "0" : y ? "1" : ".");
        }
        vcf += ".\t.\t.\t" + mb.first[ri] + "\t" + mb.first[ai] + "\t.\tbefore=" + first + ";after=" + mb.second + "\t.\tGT\t" + join(calls, "\t") + "\n";
    }
    SKX_TRY(write_file(std::string(out_prefix) + "_indels.vcf", vcf));
    info("ska::skalo::process_indels", std::to_string(n_indels) + " indels");
    info(PV, "Filtering paths");

    info(PV, "Sorting variant groups");
    std::vector<std::pair<double, Ends>> order;
    for (auto &kv : finals) if (!kv.second.empty()) order.emplace_back((double)kv.second.size() / (double)kv.second[0].seq.size(), kv.first);
    std::stable_sort(order.begin(), order.end(), [](const std::pair<double, Ends> &x, const std::pair<double, Ends> &y) { return x.first > y.first; });
    info(PV, "Processing SNPs");
    std::unordered_set<u128, H128> done;
    std::map<uint32_t, std::string> snps;
    size_t not_positioned = 0; uint32_t counter = 0;
    for (auto &o : order) {
        const Ends key = o.second;
        if (taken.count(L.val[key.first]) || taken.count(rc_n(L.val[key.second], kg))) continue;
        const Group &vv = finals[key];
        if (vv.size() < 2) continue;
        std::vector<std::pair<size_t, std::string>> found;
        std::vector<u128> to_save;
        for (size_t pos : snp_pos[key]) {
            std::string column(L.S, '-');
            std::vector<u128> tmp;
            bool fresh = true;
            for (auto &v : vv) {
                if (pos < (size_t)kg || pos + kg + 1 > v.seq.size()) { skx::set_error("ska lo: a SNP flank lies outside its path"); return SKX_EINVAL; }
                const u128 fb = encode(v.seq.data() + pos - kg, kg + 1), fa = encode(v.seq.data() + pos, kg + 1), ra = rc_n(fa, kg + 1);
                if (!done.count(fb) && !done.count(ra)) {
                    const char last = CODE[(uint32_t)(fb & 3)];
                    const auto *c = col.get(fb);
                    if (!c) { skx::set_error("ska lo: a SNP flank k-mer is not in the graph"); return SKX_EINVAL; }
                    for (uint64_t i = 0; i < L.S; i++)
                        if (bit(*c, i)) column[i] = (column[i] == '-' || column[i] == last) ? last : 'N';
                    tmp.push_back(fb); tmp.push_back(rc_n(fb, kg + 1)); tmp.push_back(fa); tmp.push_back(ra);
                } else fresh = false;
            }
            if (!fresh) continue;
            bool present[4] = {false, false, false, false}; uint64_t miss = 0;
            for (char c : column) {
                if (c == 'A') present[0] = true; else if (c == 'T') present[1] = true; else if (c == 'G') present[2] = true; else if (c == 'C') present[3] = true;
                else miss++;
            }
            if (present[0] + present[1] + present[2] + present[3] >= 2 && f32_ratio(miss, L.S) <= missing) {
                to_save.insert(to_save.end(), tmp.begin(), tmp.end());
                found.emplace_back(pos, column);
            }
        }
        done.insert(to_save.begin(), to_save.end());
        if (found.empty()) continue;
        if (reference) {
            std::vector<uint32_t> fwd, rev;
            for (auto &v : vv) {
                std::string rs(v.seq.rbegin(), v.seq.rend());
                for (char &c : rs) c = c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : 'C';
                for (int pass = 0; pass < 2; pass++) {
                    const std::string &s = pass ? rs : v.seq;
                    for (size_t p = 0; p + kg <= s.size(); p++) {
                        auto it = kmap.find(encode(s.data() + p, kg));
                        if (it != kmap.end()) for (uint32_t x : it->second) (pass ? rev : fwd).push_back(x - (uint32_t)p);
                    }
                }
            }
            auto F = fwd.empty() ? std::make_pair(0u, (size_t)0) : most_frequent(fwd);
            auto R = rev.empty() ? std::make_pair(0u, (size_t)0) : most_frequent(rev);
            bool positioned = true, forward = true; uint32_t position = 0;
            if (F.second && R.second) {
                if (F.second == R.second) positioned = false;
                else if (F.second > R.second) position = F.first;
                else { position = R.first; forward = false; }
            } else if (F.second) position = F.first;
            else if (R.second) { position = R.first; forward = false; }
            else positioned = false;
            if (!positioned) { not_positioned += found.size(); continue; }
            const size_t len = vv[0].seq.size();
            for (auto &f : found) {
                const uint32_t fp = position + (uint32_t)(forward ? f.first - kg : len - f.first - kg - 1);
                std::string c = f.second;
                if (!forward) for (char &x : c) x = x == 'A' ? 'T' : x == 'T' ? 'A' : x == 'C' ? 'G' : x == 'G' ? 'C' : x;
                if (snps.count(fp)) not_positioned++;
                else snps[fp] = c;
            }
        } else {
            for (auto &f : found) snps[++counter] = f.second;
        }
    }
    if (reference) info(PV, std::to_string(snps.size()) + " SNPs (+ " + std::to_string(not_positioned) + " w/o position)");
    else info(PV, std::to_string(snps.size()) + " SNPs");

    // output_snps.rs:create_fasta_and_vcf
    for (char &c : genome) if (c != 'A' && c != 'T' && c != 'G' && c != 'C' && c != 'N') c = 'N';
    const uint64_t glen = !genome.empty() ? genome.size() : snps.empty() ? 0 : (uint64_t)snps.rbegin()->first + 1;
    std::vector<std::string> seqs(L.S), aln(genome.empty() ? 0 : L.S);
    std::string svcf = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + join(names, "\t") + "\n";
    auto it = snps.begin();
    for (uint64_t pos = 0; pos < glen; pos++) {
        if (it != snps.end() && it->first == pos) {
            const std::string &c = it->second;
            if (!genome.empty()) {
                const char ref = genome[pos];
                std::string alts;
                for (char b : std::string("ACGT")) if (b != ref && c.find(b) != std::string::npos) alts.push_back(b);
                std::vector<std::string> gts, alt_s;
                for (char b : alts) alt_s.push_back(std::string(1, b));
                for (char x : c) {
                    if (x == ref) gts.push_back("0");
                    else if (x == '-' || x == 'N') gts.push_back(".");
                    else { const size_t j = alts.find(x); gts.push_back(j == std::string::npos ? "." : std::to_string(j + 1)); }
                }
                svcf += gname + "\t" + std::to_string(pos + 1) + "\t.\t" + std::string(1, ref) + "\t" + join(alt_s, ",") + "\t.\t.\t.\tGT\t" + join(gts, "\t") + "\n";
                for (uint64_t i = 0; i < L.S; i++) aln[i].push_back(c[i]);
            }
            for (uint64_t i = 0; i < L.S; i++) seqs[i].push_back(c[i]);
            ++it;
        } else if (!genome.empty()) {
            for (auto &s : aln) s.push_back(genome[pos]);
        }
    }
    std::string fas, pg;
    for (uint64_t i = 0; i < L.S; i++) fas += ">" + names[i] + "\n" + seqs[i] + "\n";
    SKX_TRY(write_file(std::string(out_prefix) + "_snps.fas", fas));
    if (!genome.empty()) {
        for (uint64_t i = 0; i < L.S; i++) pg += ">" + names[i] + "\n" + aln[i] + "\n";
        SKX_TRY(write_file(std::string(out_prefix) + "_pseudo_genomes.fas", pg));
        SKX_TRY(write_file(std::string(out_prefix) + "_snps.vcf", svcf));
    }
    return SKX_OK;
    });
}
