// ska_host_util.h -- what the host files above the C ABI share (private: not installed under include/): text buffers, the last
// error, the exception guard, wall-clock phases, the threaded text formatters, and the command line's helpers (defined in
// ska_host.cpp, used by ska_distance.cpp).
#pragma once
#include "../../include/skx_host.h"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace skh {

inline void put(std::string &s, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
inline void put(std::string &s, const char *fmt, ...)
{
    char tmp[256];
    va_list ap; va_start(ap, fmt); int n = vsnprintf(tmp, sizeof tmp, fmt, ap); va_end(ap);
    if (n < (int)sizeof tmp) { s.append(tmp, (size_t)n); return; }
    std::vector<char> big((size_t)n + 1);
    va_start(ap, fmt); vsnprintf(big.data(), big.size(), fmt, ap); va_end(ap);
    s.append(big.data(), (size_t)n);
}
inline int to_buf(const std::string &s, char **buf, uint64_t *len)
{
    char *p = (char *)malloc(s.size() + 1);
    if (!p) return SKX_ENOMEM;
    memcpy(p, s.data(), s.size()); p[s.size()] = 0;
    *buf = p; *len = s.size();
    return SKX_OK;
}
inline void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
inline void set_error(const char *fmt, ...)
{
    char tmp[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(tmp, sizeof tmp, fmt, ap); va_end(ap);
    skx_set_last_error(tmp);
}
template <typename F>
int guarded(F &&f) noexcept
{
    try { return f(); }
    catch (const std::bad_alloc &) { skx_set_last_error("out of host memory"); return SKX_ENOMEM; }
    catch (...) { skx_set_last_error("internal error"); return SKX_EINVAL; }
}
struct Phase {       // wall-clock phase recorded through the ABI (skx_phase_add)
    const char *name; std::chrono::steady_clock::time_point t0;
    explicit Phase(const char *n) : name(n), t0(std::chrono::steady_clock::now()) {}
    void stop() { if (name) { skx_phase_add(name, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()); name = nullptr; } }
    ~Phase() { stop(); }
};
inline int write_text_file(const std::string &path, const char *buf, uint64_t len)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) { set_error("cannot create %s", path.c_str()); return SKX_EIO; }
    const bool ok = fwrite(buf, 1, len, f) == len;
    if (fclose(f) != 0 || !ok) { set_error("cannot write %s", path.c_str()); return SKX_EIO; }
    return SKX_OK;
}

// ---- a text of many lines, formatted by a few threads: the parts in order, then the parts joined under a header line
inline unsigned format_threads_max() { return std::min(32u, std::max(1u, std::thread::hardware_concurrency())); }
// fn(i, part[i]) for every i < S, the rows handed out one at a time (a table of 1 000 samples is half a million printf calls, 20 MB)
template <typename F>
std::vector<std::string> row_parts(uint64_t S, F fn)
{
    const int T = (int)std::min<uint64_t>(std::max<uint64_t>(1, S / 16), format_threads_max());
    std::vector<std::string> part(S);
    std::atomic<uint64_t> next{0};
    auto work = [&]() { for (uint64_t i; (i = next.fetch_add(1)) < S;) fn(i, part[i]); };
    std::vector<std::thread> th;
    for (int t = 1; t < T; t++) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
    return part;
}
// fn(x, part) for every x < n, in T equal slices of at least 4 096 lines, a thread each
template <typename F>
std::vector<std::string> slice_parts(uint64_t n, F fn)
{
    const uint64_t T = std::max<uint64_t>(1, std::min<uint64_t>(n / 4096, format_threads_max()));
    std::vector<std::string> part(T);
    auto work = [&](uint64_t t) { for (uint64_t x = n * t / T; x < n * (t + 1) / T; x++) fn(x, part[t]); };
    std::vector<std::thread> th;
    for (uint64_t t = 1; t < T; t++) th.emplace_back(work, t);
    work(0);
    for (auto &t : th) t.join();
    return part;
}
inline int join_parts(const char *header, const std::vector<std::string> &part, char **buf, uint64_t *len)
{
    std::string out = header;
    size_t total = out.size();
    for (auto &x : part) total += x.size();
    out.reserve(total);
    for (auto &x : part) out += x;
    return to_buf(out, buf, len);
}
template <typename F> int format_rows(const char *header, uint64_t S, F fn, char **buf, uint64_t *len) { return join_parts(header, row_parts(S, fn), buf, len); }
template <typename F> int format_slices(const char *header, uint64_t n, F fn, char **buf, uint64_t *len) { return join_parts(header, slice_parts(n, fn), buf, len); }

// ---- the command line (ska_host.cpp)
struct Args {
    std::vector<std::string> pos;
    std::vector<std::pair<std::string, std::string>> opt;
    bool has(const std::string &k) const { for (auto &o : opt) if (o.first == k) return true; return false; }
    std::string get(const std::string &k, const std::string &d = "") const { for (auto &o : opt) if (o.first == k) return o.second; return d; }
};
int fail(const char *msg);                                                         // "error: <msg>", exit code 2
int engine_fail();                                                                 // "error: <the engine's last error>", exit code 101
int emit(const std::string &out_path, const char *buf, uint64_t len);              // io_utils::set_ostream: stdout or the file
bool lo_float(const std::string &v);                                               // what Rust's float parser takes
// clap's wording for what its derive macros refuse: exit code 2, the reason, the hint
const char *clap_arg(const char *flag);                                            // "--query-file" -> "--query-file <FILE>"; the flag itself where it takes no value
int clap_invalid(const std::string &value, const char *arg, const char *why);
int clap_possible(const std::string &value, const char *arg, const char *values);
int clap_missing(const char *cmd, const char *args);
int clap_conflict(const char *cmd, const char *x, const char *y);                  // x, y: flags (spelled by clap_arg) or a positional's spelling
// the first owner (owner-major) given together with one of the others is refused; --gpus counts as given when multi.  0: none
int conflicts(const char *cmd, const Args &a, bool multi, std::initializer_list<const char *> owners, std::initializer_list<const char *> others);
// usize::from_str / f32::from_str, then the range.  0: the value stands
int clap_uint(const std::string &v, const char *arg, unsigned long long min, const char *why_below, bool check_erange = false);
int clap_float(const std::string &v, const char *arg, double lo, double hi, const char *why_outside);
int validate_min_freq(const Args &a);                                              // --min-freq / -m
int validate_build_inputs(const char *cmd, const Args &a);                         // sequence files or -f, and the build options

// ---- ska distance (ska_distance.cpp)
// --tree / --clusters / --cluster-snps / --cluster-mismatches
struct DistExtras {
    std::string tree, clusters; skh_dist_extras x{};
    explicit DistExtras(const Args &a) : tree(a.get("--tree")), clusters(a.get("--clusters"))
    {
        x.tree = a.has("--tree") ? tree.c_str() : nullptr; x.clusters = a.has("--clusters") ? clusters.c_str() : nullptr;
        x.cluster_snps = atof(a.get("--cluster-snps", "10").c_str()); x.cluster_mismatches = atof(a.get("--cluster-mismatches", "1.0").c_str());
    }
    const skh_dist_extras *get() const { return x.tree || x.clusters ? &x : nullptr; }
};
int distance_text_names(const std::vector<const char *> &names, const skx_dist *d, char **buf, uint64_t *len);
int distance_extras(skx_ctx *ctx, const std::vector<const char *> &names, const skx_dist *d, const skh_dist_extras *x);
int validate_distance(const Args &a, bool multi);
int run_distance(skx_ctx *ctx, const Args &a);

// the files of `ska merge` loaded and merged in memory (ska_host.cpp)
int merge_files(skx_ctx *ctx, const char *const *skf_files, int n_files, skx_array **merged, std::vector<uint64_t> *n_each = nullptr);

}  // namespace skh
