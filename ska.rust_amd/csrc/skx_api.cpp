// skx_api.cpp -- the C ABI (include/skx.h): errors, phases, the device cache, the context, the batching of skx_build_and_merge, arrays from
// the host and back, filter and the .skf life-cycle operations (dictset construction: skx_dictset.cpp; rows, arrays over them, the append
// pass and skx_merge: skx_merge.cpp; cov / map / .skf files: skx_api_io.cpp; sequence files onto the device: skx_build_files.cpp; distance:
// skx_distance.cpp).
// No CPU fallback exists: without a usable HIP device every compute entry point fails with SKX_ENODEV.
#include "skx_internal.h"
#include "../../include/skx_host.h"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <optional>
#include <unordered_map>
#include <thread>
#include <cerrno>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

using namespace skx;

// ------------------------------------------------------------------------------------------ errors
static thread_local char g_err[1024];
void skx::set_error(const char *fmt, ...)
{
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
}
long skx::knob(const char *name, long absent)
{
    const char *e = getenv("SKX_KNOBS");
    if (!e) return absent;
    const size_t n = strlen(name);
    for (const char *p = e; *p;) {
        const char *q = strchr(p, ','); if (!q) q = p + strlen(p);
        if ((size_t)(q - p) >= n && !strncmp(p, name, n) && (p[n] == '=' || p + n == q)) return p[n] == '=' ? atol(p + n + 1) : 1;
        p = *q ? q + 1 : q;
    }
    return absent;
}
int skx::hip_fail(hipError_t e, const char *what)
{
    set_error("HIP error %d (%s) in %s", (int)e, hipGetErrorString(e), what);
    return e == hipErrorOutOfMemory ? SKX_ENOMEM : SKX_ENODEV;
}
extern "C" const char *skx_last_error(void) { return g_err; }

// ------------------------------------------------------------------------------------------ phases
namespace {
struct Phases { std::mutex mu; std::vector<std::pair<std::string, double>> v; } g_phases;
}
void skx::phase_add(const char *name, double secs)
{
    {
        std::lock_guard<std::mutex> lk(g_phases.mu);
        bool found = false;
        for (auto &p : g_phases.v) if (p.first == name) { p.second += secs; found = true; break; }
        if (!found) g_phases.v.emplace_back(name, secs);
    }
    if (getenv("SKX_DEBUG")) fprintf(stderr, "[skx] %-28s %.3f s\n", name, secs);
}
extern "C" void skx_phase_add(const char *name, double seconds) { if (name) skx::phase_add(name, seconds); }
extern "C" int skx_phases_json(char **buf, uint64_t *len, int reset)
{
    return skx_guarded([&]() -> int {
    std::string o = "{";
    {
        std::lock_guard<std::mutex> lk(g_phases.mu);
        for (size_t i = 0; i < g_phases.v.size(); i++) {
            char tmp[64]; snprintf(tmp, sizeof tmp, "%.6f", g_phases.v[i].second);
            o += (i ? ", \"" : "\"") + g_phases.v[i].first + "\": " + tmp;
        }
        if (reset) g_phases.v.clear();
    }
    o += "}";
    char *p = (char *)malloc(o.size() + 1);
    if (!p) { set_error("out of host memory"); return SKX_ENOMEM; }
    memcpy(p, o.c_str(), o.size() + 1);
    *buf = p; if (len) *len = o.size();
    return SKX_OK;
    });
}
extern "C" const char *skx_version(void) { return "0.5.2"; }      // Cargo.toml:3, written as ska_version
extern "C" void skx_free(void *p) { free(p); }

// ------------------------------------------------------------------------------------------ device memory cache
namespace {
// one pool per device: a block is only ever handed back to a request made while its own device is current
struct DevCache {
    std::mutex mu;
    std::map<int, std::multimap<size_t, void *>> free_blocks;      // device -> size -> block
    std::unordered_map<void *, std::pair<size_t, int>> live;       // block -> (size, device)
    size_t cached_bytes = 0;
} g_cache;
int current_device() { int d = 0; (void)hipGetDevice(&d); return d; }
}
void *skx::dev_alloc(size_t bytes, hipError_t *err)
{
    bytes = (bytes + 255) & ~(size_t)255;
    const int dev = current_device();
    {
        std::lock_guard<std::mutex> lk(g_cache.mu);
        auto &pool = g_cache.free_blocks[dev];
        auto it = pool.lower_bound(bytes);
        if (it != pool.end() && it->first <= bytes + bytes / 4 + (1u << 20)) {
            void *p = it->second; size_t sz = it->first;
            pool.erase(it); g_cache.cached_bytes -= sz; g_cache.live[p] = {sz, dev};
            return p;
        }
    }
    void *p = nullptr;
    const auto t_malloc = std::chrono::steady_clock::now();
    struct Took { std::chrono::steady_clock::time_point t0; ~Took() { skx::phase_add("alloc.hipMalloc_all_threads", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()); } } took{t_malloc};      // (what the driver took to hand out memory: the phase table's answer to "where did the seconds go" behind a process that has just released its own)
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {                                // out of memory: drop the cache and retry once
        (void)hipGetLastError();
        skx::dev_trim();
        e = hipMalloc(&p, bytes);
    }
    if (e != hipSuccess) { (void)hipGetLastError(); if (err) *err = e; return nullptr; }
    std::lock_guard<std::mutex> lk(g_cache.mu);
    g_cache.live[p] = {bytes, dev};
    return p;
}
void skx::dev_free(void *p)
{
    std::lock_guard<std::mutex> lk(g_cache.mu);
    auto it = g_cache.live.find(p);
    if (it == g_cache.live.end()) { (void)hipFree(p); return; }
    g_cache.free_blocks[it->second.second].emplace(it->second.first, p); g_cache.cached_bytes += it->second.first;
    g_cache.live.erase(it);
}
void skx::dev_trim()
{
    std::lock_guard<std::mutex> lk(g_cache.mu);
    for (auto &pool : g_cache.free_blocks) for (auto &kv : pool.second) (void)hipFree(kv.second);      // hipFree takes a block of any device
    g_cache.free_blocks.clear(); g_cache.cached_bytes = 0;
}

// CPUs this process may keep busy: the hardware's count or, where a control group caps the job (cgroup v2 cpu.max, v1 cfs quota), the cap --
// thread teams larger than that only take turns, and a team that overruns the quota has the whole process (the thread that feeds the GPU
// included) stopped for the rest of the scheduler's period
int skx::cpu_budget()
{
    static const int v = [] {
        int hc = (int)std::thread::hardware_concurrency(); if (hc < 1) hc = 1;
        double q = 0, per = 0; char w[64] = {0};
        if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) { if (fscanf(f, "%63s %lf", w, &per) == 2 && strcmp(w, "max") != 0) q = atof(w); fclose(f); }
        if (q <= 0) {
            long long qq = -1, pp = 0;
            if (FILE *f = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(f, "%lld", &qq) != 1) qq = -1; fclose(f); }
            if (FILE *f = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(f, "%lld", &pp) != 1) pp = 0; fclose(f); }
            if (qq > 0 && pp > 0) { q = (double)qq; per = (double)pp; }
        }
        if (q > 0 && per > 0) hc = std::min(hc, std::max(1, (int)std::ceil(q / per)));
        return hc;
    }();
    return v;
}

int skx::check_k(int k)
{
    if (k < 5 || k > 63 || (k & 1) == 0) { set_error("Invalid k-mer length"); return SKX_EINVAL; }   // ska_dict.rs:342-344
    return SKX_OK;
}

// ------------------------------------------------------------------------------------------ output page allocation
skx::Preallocator::Preallocator(int fd_, off_t base_) : fd(fd_), base(base_)
{
    th = std::thread([this]() {
        constexpr uint64_t STEP = 256ull << 20;
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv.wait(lk, [this] { return stop || done < target; });
            if (stop && done >= target) return;
            const uint64_t o = done, n = std::min(STEP, target - done);
            lk.unlock();
            // a failure (ENOSPC, quota) is recorded: a writer that stores through a mapping of pages that do not exist dies of SIGBUS
            if (posix_fallocate(fd, base + (off_t)o, (off_t)n) != 0) failed.store(true, std::memory_order_release);
            lk.lock();
            done = o + n;
            cv.notify_all();
        }
    });
}
skx::Preallocator::~Preallocator() { { std::lock_guard<std::mutex> lk(mu); stop = true; target = done; } cv.notify_all(); if (th.joinable()) th.join(); }
void skx::Preallocator::raise(uint64_t bytes) { { std::lock_guard<std::mutex> lk(mu); if (bytes > target) target = bytes; } cv.notify_all(); }
void skx::Preallocator::finish(uint64_t bytes)
{
    std::unique_lock<std::mutex> lk(mu);
    if (bytes > target) target = bytes;
    cv.notify_all();
    cv.wait(lk, [&] { return done >= bytes; });
}
// a regular file, opened read-write and not in append mode, can be written through a mapping
bool skx::mappable_output_fd(int fd, off_t *pos)
{
    struct stat sb;
    if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) return false;
    const int fl = fcntl(fd, F_GETFL);
    if (fl < 0 || (fl & O_APPEND) || (fl & O_ACCMODE) != O_RDWR) return false;
    *pos = lseek(fd, 0, SEEK_CUR);
    return *pos >= 0;
}
extern "C" int skx_ctx_expect_output(skx_ctx *ctx, int fd)
{
    if (!ctx) return SKX_EINVAL;
    off_t pos;
    ctx->expect_fd = (fd >= 0 && mappable_output_fd(fd, &pos)) ? fd : -1;
    return SKX_OK;
}

// ------------------------------------------------------------------------------------------ ctx
extern "C" int skx_ctx_create(int device, skx_ctx **out)
{
    return skx_guarded([&]() -> int {
    if (!out) { set_error("null out"); return SKX_EINVAL; }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { set_error("no HIP device available (%s); the engine has no CPU path", e == hipSuccess ? "count 0" : hipGetErrorString(e)); return SKX_ENODEV; }
    if (device < 0 || device >= ndev) { set_error("device %d out of range (%d devices)", device, ndev); return SKX_EINVAL; }
    SKX_HIP(hipSetDevice(device));
    skx_ctx *c = new skx_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev[0]) != hipSuccess || hipEventCreate(&c->ev[1]) != hipSuccess || hipEventCreate(&c->ev[2]) != hipSuccess ||
        hipEventCreate(&c->ev[3]) != hipSuccess) {
        delete c; set_error("cannot create HIP stream/events"); return SKX_ENODEV;
    }
    *out = c;
    return SKX_OK;
    });
}
extern "C" void skx_ctx_destroy(skx_ctx *c)
{
    if (!c) return;
    if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    for (auto &e : c->ev) if (e) (void)hipEventDestroy(e);
    skx::dev_trim();
    delete c;
}
extern "C" int skx_ctx_sync(skx_ctx *c) { SKX_HIP(hipSetDevice(c->device)); SKX_HIP(hipStreamSynchronize(c->stream)); return SKX_OK; }
extern "C" void *skx_ctx_stream(skx_ctx *c) { return (void *)c->stream; }
uint64_t skx::next_object_id() { static std::atomic<uint64_t> n{0}; return ++n; }
extern "C" const char *skx_ctx_merge_path(skx_ctx *c) { return c ? c->merge_path.c_str() : ""; }
extern "C" int skx_ctx_filter_cut(skx_ctx *c, uint64_t *ranks, uint64_t *blocks)
{
    if (!c) { set_error("bad arguments"); return SKX_EINVAL; }
    if (ranks) *ranks = c->cut_ranks;
    if (blocks) *blocks = c->cut_blocks;
    return SKX_OK;
}
// test hook (not declared in include/skx.h, like skx_debug_fastq_frame; tests bind it): pieces_cut_kernel alone (the filter takes the cut inside its statistics pass) -- out[j] = the
// min_count-th largest of plen[j * n_samples .. + n_samples) (host arrays; values <= cap), 0 when min_count > n_samples
extern "C" int skx_debug_pieces_cut(skx_ctx *ctx, const uint16_t *plen, int n_samples, int n_blocks, uint32_t cap, uint32_t min_count, uint32_t *out)
{
    return skx_guarded([&]() -> int {
    if (!ctx || !plen || !out || n_samples < 1 || n_samples > 65535 || n_blocks < 1 || cap < 32u || cap % 32u || cap > 12032u) { set_error("bad arguments"); return SKX_EINVAL; }
    SKX_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint64_t n = (uint64_t)n_blocks * (uint64_t)n_samples;
    DevBuf<uint16_t> d_pl; DevBuf<uint32_t> d_cut;
    SKX_TRY(d_pl.alloc(n)); SKX_TRY(d_cut.alloc((size_t)n_blocks));
    SKX_HIP(hipMemcpyAsync(d_pl.p, plen, n * 2, hipMemcpyHostToDevice, st));
    launch_pieces_cut(d_pl.p, n_samples, cap, min_count, nullptr, nullptr, 0, n_blocks, d_cut.p, nullptr, st);
    SKX_HIP(hipMemcpyAsync(out, d_cut.p, (size_t)n_blocks * 4, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    SKX_HIP(hipGetLastError());
    return SKX_OK;
    });
}
extern "C" int skx_ctx_timings(skx_ctx *c, skx_timings *t, int reset)
{
    return skx_guarded([&]() -> int {
    if (t) *t = c->tm;
    if (reset) c->tm = skx_timings{};
    return SKX_OK;
    });
}

// Test hook (not part of the drop-in boundary): FASTQ text through the device framing (skx_fastq.hip), the planes expanded to the two record
// streams the read-set kernels would see -- sequence A C T G N '\n', quality ' ' (passes) / '!' (fails) / '\n'.  seq / qual: room for len / 2 + 64.
extern "C" int skx_debug_fastq_frame(skx_ctx *ctx, const uint8_t *text, uint64_t len, uint64_t junction, int min_qual, uint8_t *seq, uint8_t *qual,
                                     uint64_t *positions, int *irregular)
{
    return skx_guarded([&]() -> int {
    if (!ctx || !text || !seq || !qual || !positions || !irregular) { set_error("bad arguments"); return SKX_EINVAL; }
    SKX_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf<uint8_t> d_text, d_seq, d_qual; DevBuf<uint64_t> planes;
    SKX_TRY(d_text.alloc(len + 64)); SKX_TRY(planes.alloc((len / 2 / 64 + 4) * 5));
    SKX_HIP(hipMemsetAsync(d_text.p, 0xAA, len + 64, st));                // (what lies behind the text is not zero in the pipeline either)
    SKX_HIP(hipMemcpyAsync(d_text.p, text, len, hipMemcpyHostToDevice, st));
    FastqScratch sc;
    SKX_TRY(fastq_frame_planes(ctx, d_text.p, len, junction, min_qual, planes.p, sc, positions, irregular));
    if (*irregular || *positions == 0) { SKX_HIP(hipStreamSynchronize(st)); return SKX_OK; }
    SKX_TRY(d_seq.alloc(*positions + 64)); SKX_TRY(d_qual.alloc(*positions + 64));
    launch_expand_planes(planes.p, *positions, d_seq.p, d_qual.p, st);
    SKX_HIP(hipMemcpyAsync(seq, d_seq.p, *positions, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipMemcpyAsync(qual, d_qual.p, *positions, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    SKX_HIP(hipGetLastError());
    return SKX_OK;
    });
}

// Test hook (not part of the drop-in boundary): a gzip file's bytes through the device inflater (skx_gzdev.hip).  status: gzd::Status -- 0: text[0..total)
// is the members' text, lengths and CRCs checked; otherwise nothing is vouched for (the engine would take the file through the reader threads'
// inflater).  ms[0..2): device time of the decode kernels and of the text + CRC kernels.
extern "C" int skx_debug_gz_inflate(skx_ctx *ctx, const uint8_t *gz, uint64_t len, uint64_t text_hint, uint8_t *text, uint64_t cap, uint64_t *total,
                                    uint32_t *status, uint32_t *n_members, double *ms)
{
    return skx_guarded([&]() -> int {
    if (!ctx || !gz || !text || !total || !status || !n_members) { set_error("bad arguments"); return SKX_EINVAL; }
    SKX_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf<uint8_t> d_gz, d_text;
    SKX_TRY(d_gz.alloc(len + 64));
    SKX_HIP(hipMemsetAsync(d_gz.p + (len & ~3ull), 0, 64 - (len & 3u), st));
    SKX_HIP(hipMemcpyAsync(d_gz.p, gz, len, hipMemcpyHostToDevice, st));
    GzDevWork wk;
    hipEvent_t e0, e1, e2;
    SKX_HIP(hipEventCreate(&e0)); SKX_HIP(hipEventCreate(&e1)); SKX_HIP(hipEventCreate(&e2));
    struct Ev { hipEvent_t a, b, c; ~Ev() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); (void)hipEventDestroy(c); } } ev{e0, e1, e2};
    int rc2 = SKX_OK;
    for (int rep = 0; rep < 2 && rc2 == SKX_OK; rep++) {                  // (the second pass is the timed one: buffers exist)
        SKX_HIP(hipEventRecord(e0, st));
        rc2 = gz_device_decode(ctx, st, d_gz.p, len, text_hint, wk);
        SKX_HIP(hipEventRecord(e1, st));
    }
    SKX_TRY(rc2);
    GzDevFileInfo fi;
    SKX_HIP(hipMemcpyAsync(&fi, wk.finfo.p, sizeof fi, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    float m0 = 0, m1 = 0;
    (void)hipEventElapsedTime(&m0, e0, e1);
    if (ms) { ms[0] = m0; ms[1] = 0; }
    *total = fi.total; *status = fi.status; *n_members = fi.n_members;
    if (fi.status == 0 && fi.total > cap) { *status = 2; return SKX_OK; }
    if (fi.status == 0 && fi.total) {
        SKX_TRY(d_text.alloc(fi.total + 64));
        SKX_HIP(hipEventRecord(e1, st));
        SKX_TRY(gz_device_text(ctx, st, wk, d_text.p, fi.total, fi.n_members));
        SKX_HIP(hipEventRecord(e2, st));
        SKX_HIP(hipMemcpyAsync(&fi, wk.finfo.p, sizeof fi, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipMemcpyAsync(text, d_text.p, fi.total, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipStreamSynchronize(st));
        (void)hipEventElapsedTime(&m1, e1, e2);
        *status = fi.status;
        if (fi.status == 0 && (fi.first != text[0] || fi.last != text[fi.total - 1])) { set_error("internal: first / last byte of the inflated text"); return SKX_EUNSUP; }
    }
    if (ms) { ms[0] = m0; ms[1] = m1; }
    SKX_HIP(hipGetLastError());
    return SKX_OK;
    });
}

extern "C" int skx_read_records(const char *file1, const char *file2, double proportion_reads, int streaming, uint8_t **seq, uint8_t **qual, uint64_t *len)
{
    return skx_guarded([&]() -> int {
    if (!file1 || !seq || !qual || !len) { set_error("bad arguments"); return SKX_EINVAL; }
    *seq = nullptr; *qual = nullptr; *len = 0;
    HostStream h;
    if (streaming) {
        const std::function<int(int, const uint8_t *, size_t)> emit = [&](int which, const uint8_t *p, size_t nb) -> int {
            std::vector<uint8_t> &v = which ? h.qual : h.seq;
            v.insert(v.end(), p, p + nb); v.push_back('\n');
            return SKX_OK;
        };
        for (const char *f : {file1, file2}) {
            if (!f) continue;
            const int r = stream_fastq_file(f, emit);
            if (r == SKF_NOT_TAKEN) { set_error("not a FASTQ file: %s", f); return SKX_EUNSUP; }
            if (r != SKX_OK) return r;
        }
        h.is_fastq = true;
    } else SKX_TRY(read_sample_stream(file1, file2, proportion_reads, h));
    if (h.is_fastq && h.qual.size() != h.seq.size()) { set_error("Invalid FASTA/Q record"); return SKX_EIO; }
    const size_t n = h.seq.size();
    uint8_t *s = (uint8_t *)malloc(n + 1), *q = h.is_fastq ? (uint8_t *)malloc(n + 1) : nullptr;
    if (!s || (h.is_fastq && !q)) { free(s); free(q); set_error("out of memory"); return SKX_ENOMEM; }
    memcpy(s, h.seq.data(), n);
    if (q) memcpy(q, h.qual.data(), n);
    *seq = s; *qual = q; *len = n;
    return SKX_OK;
    });
}

// ---- `ska build` on more samples than fit in HBM at once ---------------------------------------------------------------
// The per-sample dictionaries are the large transient (8-byte packed words, raw and deduplicated, per input base); the
// array that survives is 1 byte per (row, sample).  A batch of samples whose dictionaries fit is built and merged into
// an array, the batch arrays are then joined by the `ska merge` row-set path (skx_array_merge): the result has the same
// rows and columns as one big batch (merge_ska_dict.rs:354-417 builds the same union through its tree of appends).
// resident: what a sample holds on the device while its batch is built; transient: what building it needs for a moment (read sets are
// counted one sample at a time).  An assembly's dictionary is a packed word per base, raw and deduplicated, with slack.  A read set
// (first byte '@', or gzip: taken as reads) keeps its two record streams -- about the size of its files -- and a dictionary of at most
// one word per min_count windows; the windows of ONE sample with their partition copies are the transient.  (Pricing a 50x isolate as
// an assembly -- 22 GB instead of ~1.5 -- cut 12 isolates into three batches whose arrays were then joined on the host: 6 s instead of 2.5.)
struct SampleNeed { uint64_t resident = 0, transient = 0; };
static SampleNeed sample_device_bytes(const char *f1, const char *f2, bool wide, unsigned min_count)
{
    uint64_t bytes = 0; bool reads = false;
    for (const char *f : sample_files(f1, f2)) {
        const FileProbe p = probe_file(f);
        if (!p.found) continue;                                // the reader reports a missing file
        const bool gz = p.n_head >= 1 && p.head[0] == 0x1f;
        reads |= gz || (p.n_head >= 1 && p.head[0] == '@');
        bytes += p.size * (gz ? 5u : 1u);                      // upper estimate of the text
    }
    SampleNeed n;
    if (reads) {
        const uint64_t bases = bytes / 2;                      // sequence and quality lines
        n.resident = bytes + bases / std::max(1u, min_count) * (wide ? 20u : 12u) + (8u << 20);
        n.transient = bases * (wide ? 56u : 28u);
    } else
        n.resident = bytes * (wide ? 44u : 24u) + (8u << 20);  // sequence + raw regions (with slack) + deduplicated words
    return n;
}
static uint64_t cached_device_bytes()        // of the current device
{
    const int dev = current_device();
    std::lock_guard<std::mutex> lk(g_cache.mu);
    uint64_t n = 0;
    auto it = g_cache.free_blocks.find(dev);
    if (it != g_cache.free_blocks.end()) for (auto &kv : it->second) n += kv.first;
    return n;
}
static uint64_t build_budget_bytes(skx_ctx *ctx)
{
    if (const char *e = getenv("SKX_BUILD_BATCH_MB")) return (uint64_t)std::max(1.0, atof(e)) << 20;
    size_t fr = 0, tot = 0;
    if (hipSetDevice(ctx->device) != hipSuccess || hipMemGetInfo(&fr, &tot) != hipSuccess) return ~0ull;
    return (uint64_t)(fr + cached_device_bytes()) / 10 * 6;
}
static int build_range(skx_ctx *ctx, const char *const *names, const char *const *file1, const char *const *file2, int lo, int hi,
                       int k, int rc, const skx_qual *q, int threads, double proportion_reads, std::vector<skx_array *> &parts)
{
    skx_dictset *d = nullptr;
    skx_array *a = nullptr;
    int r = skx_dictset_build_files(ctx, file1 + lo, file2 ? file2 + lo : nullptr, hi - lo, k, rc, q, threads, proportion_reads, &d);
    if (r == SKX_OK) r = merge_batch(ctx, d, names + lo, &a);    // (the dictset is the merge's from here)
    if (r == SKX_ENOMEM && hi - lo > 1) {                      // the estimate was too low: halve the batch
        dev_trim();
        const int mid = lo + (hi - lo) / 2;
        SKX_TRY(build_range(ctx, names, file1, file2, lo, mid, k, rc, q, threads, proportion_reads, parts));
        return build_range(ctx, names, file1, file2, mid, hi, k, rc, q, threads, proportion_reads, parts);
    }
    if (r != SKX_OK) return r;
    parts.push_back(a);
    return SKX_OK;
}

extern "C" int skx_build_and_merge(skx_ctx *ctx, const char *const *names, const char *const *file1, const char *const *file2, int n,
                                   int k, int rc, const skx_qual *q, int threads, double proportion_reads, skx_array **out)
{
    return skx_guarded([&]() -> int {
    if (!ctx || !names || !file1 || n <= 0 || !out) { set_error("bad arguments"); return SKX_EINVAL; }
    SKX_TRY(check_k(k));
    const uint64_t budget = build_budget_bytes(ctx);
    std::vector<skx_array *> parts;
    struct Drop { std::vector<skx_array *> &v; ~Drop() { for (auto *a : v) skx_array_free(a); } } drop{parts};
    int r = SKX_OK, lo = 0;
    while (lo < n && r == SKX_OK) {
        uint64_t need = 0, transient = 0;
        int hi = lo;
        while (hi < n) {
            const SampleNeed s = sample_device_bytes(file1[hi], file2 ? file2[hi] : nullptr, k > 31, q ? q->min_count : 1);
            if (hi > lo && need + s.resident + std::max(transient, s.transient) > budget) break;
            need += s.resident; transient = std::max(transient, s.transient); hi++;
        }
        need += transient;
        if (getenv("SKX_DEBUG") && (lo || hi < n)) fprintf(stderr, "[skx] build: samples %d..%d as one batch (estimate %.1f MB of %.1f MB)\n", lo, hi - 1, need / 1048576.0, budget / 1048576.0);
        r = build_range(ctx, names, file1, file2, lo, hi, k, rc, q, threads, proportion_reads, parts);
        lo = hi;
    }
    if (r != SKX_OK) return r;
    if (parts.size() == 1) { *out = parts[0]; parts.clear(); return SKX_OK; }
    return skx_array_merge(ctx, parts.data(), (int)parts.size(), out);
    });
}

extern "C" int skx_array_device_matrix(skx_array *a, const uint8_t **dptr, uint64_t *pitch, uint64_t *n_rows)
{
    return skx_guarded([&]() -> int {
    SKX_TRY(array_materialize(a));
    *dptr = a->matrix.p; *pitch = a->pitch; *n_rows = a->n_rows;
    return SKX_OK;
    });
}

extern "C" int skx_array_device_stats(skx_array *a, uint32_t **present, uint32_t **unambig, uint32_t **mask, uint32_t **variant_count)
{
    { const int r = skx_guarded([&]() -> int { return a->lazy() ? array_lazy_stats(a) : SKX_OK; }); if (r != SKX_OK) return r; }      // a lazily held array stays one: statistics only
    if (present) *present = a->present.p;
    if (unambig) *unambig = a->unambig.p;
    if (mask) *mask = a->mask.p;
    if (variant_count) *variant_count = a->vcount.p;
    return SKX_OK;
}
extern "C" int skx_array_set_total_samples(skx_array *a, uint64_t total) { a->total_samples = total; return SKX_OK; }

extern "C" int skx_array_from_host(skx_ctx *ctx, int k, int rc, const char *const *names, int n_samples, const skx_key *keys,
                                   const uint8_t *variants, const uint64_t *variant_count, uint64_t n_rows, const char *version, skx_array **out)
{
    return skx_guarded([&]() -> int {
    if (!ctx || !out || n_samples <= 0) { set_error("bad arguments"); return SKX_EINVAL; }
    SKX_TRY(check_k(k));
    SKX_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::unique_ptr<skx_array> a(new skx_array());
    a->ctx = ctx; a->k = k; a->rc = rc; a->k_bits = k <= 31 ? 64 : 128; a->hp = make_hash_params(std::min(k, 31)); a->wh = make_wide_hash(k);
    a->version = version ? version : skx_version();
    for (int i = 0; i < n_samples; i++) a->names.emplace_back(names[i]);
    a->n_rows = a->n_kmers = n_rows; a->pitch = pitch_for(n_rows); a->engine_order = false;
    SKX_TRY(a->matrix.alloc((uint64_t)n_samples * a->pitch));
    SKX_TRY(a->present.alloc(n_rows)); SKX_TRY(a->unambig.alloc(n_rows)); SKX_TRY(a->mask.alloc(n_rows)); SKX_TRY(a->vcount.alloc(n_rows));
    if (k <= 31) {
        SKX_TRY(a->keys.alloc(n_rows));
        std::vector<uint64_t> lo(n_rows);
        for (uint64_t i = 0; i < n_rows; i++) lo[i] = keys[i].lo;
        DevBuf<uint64_t> tmp; SKX_TRY(tmp.alloc(n_rows));
        SKX_HIP(hipMemcpyAsync(tmp.p, lo.data(), n_rows * 8, hipMemcpyHostToDevice, st));
        launch_hash_keys(tmp.p, a->keys.p, n_rows, a->hp, st);
        SKX_HIP(hipStreamSynchronize(st));
    } else {
        a->host_keys.assign(keys, keys + n_rows);
    }
    DevBuf<int> d_bad; SKX_TRY(d_bad.alloc(1)); SKX_TRY(d_bad.zero(st));
    if (n_rows) {
        DevBuf<uint8_t> rm; SKX_TRY(rm.alloc(n_rows * (uint64_t)n_samples));
        SKX_HIP(hipMemcpyAsync(rm.p, variants, n_rows * (uint64_t)n_samples, hipMemcpyHostToDevice, st));
        SKX_HIP(hipMemsetAsync(a->matrix.p, '-', (uint64_t)n_samples * a->pitch, st));
        launch_transpose(rm.p, (uint64_t)n_samples, n_rows, (uint64_t)n_samples, a->matrix.p, a->pitch, st);
        launch_col_stats(a->matrix.p, a->pitch, n_samples, n_rows, a->present.p, a->unambig.p, a->mask.p, d_bad.p, st);
        if (variant_count) {
            std::vector<uint32_t> vc(n_rows);
            for (uint64_t i = 0; i < n_rows; i++) vc[i] = (uint32_t)variant_count[i];
            SKX_HIP(hipMemcpyAsync(a->vcount.p, vc.data(), n_rows * 4, hipMemcpyHostToDevice, st));
            SKX_HIP(hipStreamSynchronize(st));
        } else SKX_HIP(hipMemcpyAsync(a->vcount.p, a->present.p, n_rows * 4, hipMemcpyDeviceToDevice, st));
        SKX_HIP(hipStreamSynchronize(st));
    }
    int bad = 0;
    SKX_HIP(hipMemcpyAsync(&bad, d_bad.p, 4, hipMemcpyDeviceToHost, st));     // on the stream: without rows nothing above has waited for the flag's memset
    SKX_HIP(hipStreamSynchronize(st));
    SKX_HIP(hipGetLastError());
    if (bad) { set_error("variants contain a byte outside -ACGTMRWSYKVHDBN (not supported on the device path)"); return SKX_EUNSUP; }
    *out = a.release();
    return SKX_OK;
    });
}

// split k-mers of an array as the reference stores them (hash undone), in the array's row order
int skx::array_host_keys(skx_array *a, std::vector<skx_key> &hk)
{
    if (a->keys_absent) { set_error("this array was loaded without its split k-mers (skx_array_load_filtered)"); return SKX_EINVAL; }
    const uint64_t K = a->n_kmers;
    hk.assign(K, skx_key{0, 0});
    if (a->k <= 31) {
        std::vector<uint64_t> w(K);
        if (K) SKX_HIP(hipMemcpy(w.data(), a->keys.p, K * 8, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < K; i++) { hk[i].lo = hunmix(w[i] >> 4, a->hp); hk[i].hi = 0; }
    } else if (!a->host_keys.empty() || K == 0) hk = a->host_keys;
    else {
        std::vector<uint64_t> w(2 * K);
        SKX_HIP(hipMemcpy(w.data(), a->keys.p, K * 16, hipMemcpyDeviceToHost));
        // (the hash undone on the host: three rounds of 64-bit multiplies a key -- by a team, 0.16 s of `ska merge`'s save on one thread)
        const int team = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::min(16, cpu_budget()), K >> 16));
        std::vector<std::thread> th;
        auto part = [&](int t) {
            for (uint64_t i = K * (uint64_t)t / (uint64_t)team, e = K * (uint64_t)(t + 1) / (uint64_t)team; i < e; i++) {
                const u128 key = hunmix_w((((u128)w[2 * i + 1] << 64) | w[2 * i]) >> 4, a->wh);
                hk[i].lo = (uint64_t)key; hk[i].hi = (uint64_t)(key >> 64);
            }
        };
        for (int t = 1; t < team; t++) th.emplace_back(part, t);
        part(0);
        for (auto &x : th) x.join();
    }
    return SKX_OK;
}

int skx::array_wide_words(skx_array *a, DevBuf<uint64_t> &tmp, const u128 **words)
{
    if (a->keys_absent) { set_error("this array was loaded without its split k-mers (skx_array_load_filtered)"); return SKX_EINVAL; }
    const uint64_t K = a->n_kmers;
    if (a->host_keys.empty()) { *words = (const u128 *)a->keys.p; return SKX_OK; }           // built here: already packed words
    hipStream_t st = a->ctx->stream;
    DevBuf<uint64_t> raw; SKX_TRY(raw.alloc(2 * K)); SKX_TRY(tmp.alloc(2 * K));
    static_assert(sizeof(skx_key) == 16 && offsetof(skx_key, lo) == 0, "skx_key is a little-endian u128");
    SKX_HIP(hipMemcpyAsync(raw.p, a->host_keys.data(), K * 16, hipMemcpyHostToDevice, st));
    launch_hash_keys_wide((const u128 *)raw.p, (u128 *)tmp.p, K, a->wh, st);
    SKX_HIP(hipStreamSynchronize(st));
    *words = (const u128 *)tmp.p;
    return SKX_OK;
}

extern "C" int skx_array_export(skx_array *a, skx_key *keys, uint8_t *variants, uint64_t *counts)
{
    return skx_guarded([&]() -> int {
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    if (variants) SKX_TRY(array_materialize(a)); else SKX_TRY(array_lazy_stats(a));
    const uint64_t U = a->n_rows, S = a->names.size(), K = a->n_kmers;
    std::vector<skx_key> hk;
    SKX_TRY(array_host_keys(a, hk));
    std::vector<uint8_t> rm(variants ? U * S : 0);              // keys / counts alone (variants == NULL) never move the matrix
    std::vector<uint32_t> pres(U);
    if (U) {
        if (variants) {
            DevBuf<uint8_t> d_rm; SKX_TRY(d_rm.alloc(U * S));
            launch_transpose(a->matrix.p, a->pitch, S, U, d_rm.p, S, st);
            SKX_HIP(hipMemcpyAsync(rm.data(), d_rm.p, U * S, hipMemcpyDeviceToHost, st));
            SKX_HIP(hipStreamSynchronize(st));
        }
        SKX_HIP(hipMemcpyAsync(pres.data(), a->vcount.p, U * 4, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipStreamSynchronize(st));
    }
    // rows sorted by key when keys and rows are in step; otherwise stored order
    std::vector<uint64_t> idx(U); std::iota(idx.begin(), idx.end(), 0);
    const bool in_step = K == U;
    if (in_step) std::sort(idx.begin(), idx.end(), [&](uint64_t x, uint64_t y) { return hk[x].hi != hk[y].hi ? hk[x].hi < hk[y].hi : hk[x].lo < hk[y].lo; });
    if (keys) { if (in_step) for (uint64_t i = 0; i < K; i++) keys[i] = hk[idx[i]]; else std::copy(hk.begin(), hk.end(), keys); }
    if (variants) for (uint64_t i = 0; i < U; i++) memcpy(variants + i * S, rm.data() + idx[i] * S, S);
    if (counts) for (uint64_t i = 0; i < U; i++) counts[i] = pres[idx[i]];
    return SKX_OK;
    });
}

extern "C" int skx_array_sample_kmers(skx_array *a, int64_t *out)
{
    return skx_guarded([&]() -> int {
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    const size_t S = a->names.size();
    if (a->pieces) {                                                  // the cells of the sample's pieces that are not empty (counted when first asked for)
        skx_pieces *pc = a->pieces;
        if (pc->sample_cells.size() != S) {
            DevBuf<unsigned long long> d; SKX_TRY(d.alloc(S)); SKX_TRY(d.zero(st));
            launch_pieces_cells(pc->data.p, pc->plen.p, pc->cap, (int)S, 1 << pc->logQ, d.p, st);
            std::vector<unsigned long long> h(S);
            SKX_HIP(hipMemcpyAsync(h.data(), d.p, S * 8, hipMemcpyDeviceToHost, st));
            SKX_HIP(hipStreamSynchronize(st));
            pc->sample_cells.assign(h.begin(), h.end());
        }
        for (size_t i = 0; i < S; i++) out[i] = (int64_t)pc->sample_cells[i];
        return SKX_OK;
    }
    if (a->lazy()) { for (size_t i = 0; i < S; i++) out[i] = (int64_t)a->lazy_dict->sample_size[i]; return SKX_OK; }      // a sample's cells = its dictionary
    DevBuf<unsigned long long> d; SKX_TRY(d.alloc(S)); SKX_TRY(d.zero(st));
    launch_row_nonmissing(a->matrix.p, a->pitch, (int)S, a->n_rows, d.p, st);
    std::vector<unsigned long long> h(S);
    SKX_HIP(hipMemcpyAsync(h.data(), d.p, S * 8, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    for (size_t i = 0; i < S; i++) out[i] = (int64_t)h[i];
    return SKX_OK;
    });
}

extern "C" int skx_array_pieces_info(skx_array *a, uint64_t *piece_bytes, uint64_t *row_blocks, uint32_t *ranks_per_block)
{
    return skx_guarded([&]() -> int {
    if (!a) { set_error("bad arguments"); return SKX_EINVAL; }
    if (piece_bytes) *piece_bytes = 0;
    if (row_blocks) *row_blocks = 0;
    if (ranks_per_block) *ranks_per_block = 0;
    const skx_pieces *pc = a->pieces;
    if (!pc) return SKX_OK;
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    const uint64_t n = ((uint64_t)1 << pc->logQ) * a->names.size();
    std::vector<uint16_t> h(n);
    SKX_HIP(hipMemcpyAsync(h.data(), pc->plen.p, n * 2, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    uint64_t b = 0;
    for (uint16_t v : h) b += ((uint64_t)v + 31) / 32 * 16;           // append_kernel stores a piece 16 bytes (32 ranks) at a time
    if (piece_bytes) *piece_bytes = b;
    if (row_blocks) *row_blocks = (uint64_t)1 << pc->logQ;
    if (ranks_per_block) *ranks_per_block = pc->cap;
    return SKX_OK;
    });
}

// shared tail of filter / weed / delete_samples: rows with keep == 1 survive (pos = exclusive scan of keep)
static int array_compact(skx_array *a, DevBuf<uint8_t> &keep, DevBuf<uint64_t> &pos, uint64_t kept, int mask_ambig, bool vcount_from_unambig,
                         bool keys_follow)
{
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    const uint64_t U = a->n_rows; const size_t S = a->names.size();
    const bool filter_ambig_as_missing = vcount_from_unambig;
    if (kept == U && !mask_ambig) {                 // nothing goes: no 2 x U x S bytes of traffic, no second matrix
        a->stats_ready = true;                      // (every row kept: every row was counted, also by a filter's bounded pass)
        if (filter_ambig_as_missing && U) SKX_HIP(hipMemcpyAsync(a->vcount.p, a->unambig.p, U * 4, hipMemcpyDeviceToDevice, st));
        SKX_HIP(hipStreamSynchronize(st));
        return SKX_OK;
    }
    {
        StageTimer t(ctx, &ctx->tm.compact);
        const uint64_t np = pitch_for(kept);
        DevBuf<uint8_t> nm; DevBuf<uint32_t> p2, u2, m2, v2;
        SKX_TRY(nm.alloc((uint64_t)S * np)); SKX_TRY(p2.alloc(kept)); SKX_TRY(u2.alloc(kept)); SKX_TRY(m2.alloc(kept)); SKX_TRY(v2.alloc(kept));
        if (a->lazy())      // the kept rows straight from the pieces or the dictionaries: the unfiltered rows x samples matrix is never written
            SKX_TRY(array_lazy_rows(a, nm.p, np, 0, 0, 0, keep.p, pos.p, mask_ambig, knob("stats_eager") != 0));
        else
            launch_compact_matrix(a->matrix.p, a->pitch, nm.p, np, (int)S, U, keep.p, pos.p, mask_ambig, st);
        {   // the four statistics in one pass over keep / pos
            // update_counts(true) rewrites variant_count with the unambiguous counts (merge_ska_array.rs:139-163)
            const uint32_t *const in[4] = {a->present.p, a->unambig.p, a->mask.p, filter_ambig_as_missing ? a->unambig.p : a->vcount.p};
            uint32_t *const out[4] = {p2.p, u2.p, m2.p, v2.p};
            launch_compact_stats(in, out, U, keep.p, pos.p, st);
        }
        if (mask_ambig) launch_mask_ambig_stats(m2.p, kept, st);
        // update_counts(true) (merge_ska_array.rs:139-163) rewrites counts AND split_kmers whenever it ran
        if (a->n_kmers == U && keys_follow) {
            if (a->k <= 31) {
                DevBuf<uint64_t> k2; SKX_TRY(k2.alloc(kept));
                launch_compact_u64(a->keys.p, k2.p, U, keep.p, pos.p, st);
                a->keys = std::move(k2);
            } else if (a->host_keys.empty()) {
                DevBuf<uint64_t> k2; SKX_TRY(k2.alloc(kept * 2));
                launch_compact_u128(a->keys.p, k2.p, U, keep.p, pos.p, st);
                a->keys = std::move(k2);
            } else {
                std::vector<uint8_t> hkeep(U);
                SKX_HIP(hipMemcpyAsync(hkeep.data(), keep.p, U, hipMemcpyDeviceToHost, st));
                SKX_HIP(hipStreamSynchronize(st));
                std::vector<skx_key> nk; nk.reserve(kept);
                for (uint64_t i = 0; i < U; i++) if (hkeep[i] == 1) nk.push_back(a->host_keys[i]);
                a->host_keys.swap(nk);
            }
            a->n_kmers = kept;
        }
        SKX_HIP(hipStreamSynchronize(st));
        a->matrix = std::move(nm); a->present = std::move(p2); a->unambig = std::move(u2); a->mask = std::move(m2); a->vcount = std::move(v2);
        a->pitch = np; a->n_rows = kept;
        a->drop_lazy();
        a->stats_ready = true;                      // (kept rows: counted in full, also by a filter's bounded pass -- skx_array_filter)
    }
    return SKX_OK;
}

extern "C" int skx_array_filter(skx_array *a, uint64_t min_count, int filter_ambig_as_missing, int filter_type, int mask_ambig,
                                int ignore_const_gaps, int update_kmers, int32_t *removed)
{
    return skx_guarded([&]() -> int {
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    const uint64_t U = a->n_rows; const size_t S = a->names.size();
    // An array still over its pieces, not yet counted: the pass counts only the first-seen ranks that min_count samples reach.  The rows of
    // the others come out with count 0 < min_count and go; the rows that stay are counted in full, and the compaction below leaves only
    // them.  Not with filter_ambig_as_missing (the silent rows, keep == 2, are told by the unambiguous count of EVERY row, and `removed`
    // depends on them), not below min_count 2 (a zero count would pass), not for a sharded job's slab (its counts are the job's, not its own).
    ctx->cut_ranks = ctx->cut_blocks = 0;
    DevBuf<unsigned long long> tally;                                  // (the bounded pass's: read back with `kept` below)
    unsigned long long h_tally[2] = {0, 0};
    if (a->pieces && !a->stats_ready && !filter_ambig_as_missing && min_count >= 2 && a->total_samples == 0 && !knob("stats_eager"))
        SKX_TRY(pieces_stats_pass(a, min_count, &tally));              // (stats_ready stays false until the compaction has dropped the uncounted rows)
    else
        SKX_TRY(array_lazy_stats(a));
    DevBuf<uint8_t> keep; DevBuf<uint64_t> pos;
    SKX_TRY(keep.alloc(U)); SKX_TRY(pos.alloc(U + 1));
    uint64_t kept = 0, silent = 0;
    {
        StageTimer t(ctx, &ctx->tm.filter);
        FilterArgs fa{a->vcount.p, a->present.p, a->unambig.p, a->mask.p, U, (uint32_t)(a->total_samples ? a->total_samples : S), min_count, filter_ambig_as_missing, filter_type, ignore_const_gaps, keep.p};
        launch_filter_flags(fa, st);
        DevBuf<uint32_t> sc_sums; DevBuf<uint64_t> sc_offs;
        SKX_TRY(sc_sums.alloc(scan_u8_blocks(U))); SKX_TRY(sc_offs.alloc(scan_u8_blocks(U) + 1));
        launch_scan_u8(keep.p, pos.p, U, sc_sums.p, sc_offs.p, st);
        SKX_HIP(hipMemcpyAsync(&kept, pos.p + U, 8, hipMemcpyDeviceToHost, st));
        if (tally.p) SKX_HIP(hipMemcpyAsync(h_tally, tally.p, 16, hipMemcpyDeviceToHost, st));
        if (filter_ambig_as_missing) {
            DevBuf<unsigned long long> d_sil; SKX_TRY(d_sil.alloc(1)); SKX_TRY(d_sil.zero(st));
            launch_count_u8(keep.p, U, 2, d_sil.p, st);
            unsigned long long s2 = 0;
            SKX_HIP(hipMemcpyAsync(&s2, d_sil.p, 8, hipMemcpyDeviceToHost, st));
            SKX_HIP(hipStreamSynchronize(st));
            silent = s2;
        }
        SKX_HIP(hipStreamSynchronize(st));
    }
    ctx->cut_ranks = h_tally[0]; ctx->cut_blocks = h_tally[1];
    if (tally.p && getenv("SKX_DEBUG")) fprintf(stderr, "[skx] filter: min_count %llu, the rank bound left %llu ranks unread over %llu of %d row blocks\n", (unsigned long long)min_count, h_tally[0], h_tally[1], 1 << a->pieces->logQ);
    SKX_TRY(array_compact(a, keep, pos, kept, mask_ambig, filter_ambig_as_missing != 0, update_kmers || filter_ambig_as_missing));
    SKX_HIP(hipGetLastError());
    if (removed) *removed = (int32_t)(U - kept - silent);
    return SKX_OK;
    });
}

// ------------------------------------------------------------------------------------------ skf life-cycle (N1)

// flags -> scan -> compaction with the keys following the rows
int skx::array_keep_rows(skx_array *a, DevBuf<uint8_t> &keep, uint64_t *removed)
{
    hipStream_t st = a->ctx->stream;
    const uint64_t U = a->n_rows;
    DevBuf<uint64_t> pos; SKX_TRY(pos.alloc(U + 1));
    uint64_t kept = 0;
    DevBuf<uint32_t> sc_sums; DevBuf<uint64_t> sc_offs;
    SKX_TRY(sc_sums.alloc(scan_u8_blocks(U))); SKX_TRY(sc_offs.alloc(scan_u8_blocks(U) + 1));
    launch_scan_u8(keep.p, pos.p, U, sc_sums.p, sc_offs.p, st);
    SKX_HIP(hipMemcpyAsync(&kept, pos.p + U, 8, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    SKX_TRY(array_compact(a, keep, pos, kept, 0, false, true));
    SKX_HIP(hipGetLastError());
    if (removed) *removed = U - kept;
    return SKX_OK;
}

extern "C" skx_ctx *skx_array_ctx(const skx_array *a) { return a->ctx; }
extern "C" void skx_set_last_error(const char *msg) { set_error("%s", msg ? msg : ""); }

// RefSka::new(k, file, rc, ..) + kmer_iter (ska_ref.rs:189-262,541) as `ska weed` uses it: the canonical split k-mers of every
// record of a FASTA file, whatever their middle bases = the key set of the file's dictionary
extern "C" int skx_keyset_from_fasta(skx_ctx *ctx, const char *path, int k, int rc, skx_keyset **out)
{
    return skx_guarded([&]() -> int {
    if (!ctx || !path || !out) { set_error("bad arguments"); return SKX_EINVAL; }
    SKX_TRY(check_k(k));
    HostStream hs;
    SKX_TRY(read_sample_stream(path, nullptr, 0.0, hs));
    if (hs.is_fastq) { set_error("Cannot create reference from FASTQ files"); return SKX_EINVAL; }                                // ska_ref.rs:206-208
    skx_stream ss; ss.seq = hs.seq.data(); ss.qual = nullptr; ss.len = hs.seq.size();
    skx_dictset *d = nullptr;
    int r = skx_dictset_build(ctx, &ss, 1, 0, k, rc, nullptr, &d);
    if (r == SKX_EEMPTY) set_error("%s has no valid sequence", path);                                                             // ska_ref.rs:255-257
    if (r != SKX_OK) return r;
    r = skx_keyset_union(ctx, d, out);
    skx_dictset_free(d);
    return r;
    });
}

extern "C" int skx_array_merge(skx_ctx *ctx, skx_array *const *in, int n, skx_array **out)
{
    return skx_guarded([&]() -> int {
    if (!ctx || !in || n <= 0 || !out) { set_error("bad arguments"); return SKX_EINVAL; }
    SKX_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    uint64_t tot = 0; size_t S = 0;
    for (int i = 0; i < n; i++) SKX_TRY(array_materialize(in[i]));
    for (int i = 0; i < n; i++) {
        if (in[i]->k != in[0]->k) { set_error("K-mer lengths do not match: %d %d", in[i]->k, in[0]->k); return SKX_EINVAL; }     // merge_ska_dict.rs:169-171
        if (in[i]->rc != in[0]->rc) { set_error("Strand use inconsistent"); return SKX_EINVAL; }                                  // :172-174
        if (in[i]->n_kmers != in[i]->n_rows || in[i]->keys_absent) { set_error("split k-mers and variants are out of step (filtered without update_kmers)"); return SKX_EINVAL; }
        tot += in[i]->n_rows; S += in[i]->names.size();
    }
    if (S > 65535) { set_error("more than 65535 samples per device array"); return SKX_EUNSUP; }
    std::unique_ptr<skx_array> a(new skx_array());
    a->ctx = ctx; a->k = in[0]->k; a->rc = in[0]->rc; a->k_bits = in[0]->k_bits; a->hp = in[0]->hp; a->wh = in[0]->wh; a->version = skx_version();
    for (int i = 0; i < n; i++) for (auto &nm : in[i]->names) a->names.push_back(nm);                                             // :177
    // rows of the result = distinct split k-mers over all inputs; idx[i][r] = result row of row r of input i
    std::vector<DevBuf<uint32_t>> idx(n);
    uint64_t U = 0;
    if (a->k <= 31) {
        DevBuf<uint64_t> all, rows; SKX_TRY(all.alloc(tot));
        uint64_t o = 0;
        for (int i = 0; i < n; i++) { if (in[i]->n_rows) SKX_HIP(hipMemcpyAsync(all.p + o, in[i]->keys.p, in[i]->n_rows * 8, hipMemcpyDeviceToDevice, st)); o += in[i]->n_rows; }
        SKX_TRY(sort_unique_words(all.p, tot, rows, &U, st));
        for (int i = 0; i < n; i++) { SKX_TRY(idx[i].alloc(in[i]->n_rows)); launch_lookup_rows(in[i]->keys.p, in[i]->n_rows, rows.p, U, idx[i].p, st); }
        SKX_TRY(a->keys.alloc(U));
        if (U) SKX_HIP(hipMemcpyAsync(a->keys.p, rows.p, U * 8, hipMemcpyDeviceToDevice, st));
        SKX_HIP(hipStreamSynchronize(st));
        a->engine_order = true;
    } else {
        // 128-bit keys: the same on 2-word packed words (arrays from files keep the reference's keys on the host; they are
        // packed on the device for the occasion)
        std::vector<DevBuf<uint64_t>> tmp(n); std::vector<const u128 *> w(n, nullptr);
        DevBuf<uint64_t> all, rows; SKX_TRY(all.alloc(2 * tot));
        uint64_t o = 0;
        for (int i = 0; i < n; i++) {
            if (!in[i]->n_rows) continue;
            SKX_TRY(array_wide_words(in[i], tmp[i], &w[i]));
            SKX_HIP(hipMemcpyAsync(all.p + 2 * o, w[i], in[i]->n_rows * 16, hipMemcpyDeviceToDevice, st));
            o += in[i]->n_rows;
        }
        SKX_TRY(sort_unique_wide((const u128 *)all.p, tot, rows, &U, st));
        for (int i = 0; i < n; i++) { SKX_TRY(idx[i].alloc(in[i]->n_rows)); launch_lookup_rows_wide(w[i], in[i]->n_rows, (const u128 *)rows.p, U, idx[i].p, st); }
        SKX_TRY(a->keys.alloc(2 * U));
        if (U) SKX_HIP(hipMemcpyAsync(a->keys.p, rows.p, U * 16, hipMemcpyDeviceToDevice, st));
        SKX_HIP(hipStreamSynchronize(st));
        a->engine_order = true;
    }
    if (U > 0xFFFFFFF0ull) { set_error("too many rows"); return SKX_EUNSUP; }
    a->n_rows = a->n_kmers = U; a->pitch = pitch_for(U);
    SKX_TRY(a->matrix.alloc((uint64_t)S * a->pitch));
    SKX_TRY(a->present.alloc(U)); SKX_TRY(a->unambig.alloc(U)); SKX_TRY(a->mask.alloc(U)); SKX_TRY(a->vcount.alloc(U));
    SKX_HIP(hipMemsetAsync(a->matrix.p, '-', (uint64_t)S * a->pitch, st));                                                        // absent = 0 -> '-' (merge_ska_array.rs:175)
    size_t c0 = 0;
    for (int i = 0; i < n; i++) {
        launch_scatter_rows(in[i]->matrix.p, in[i]->pitch, (int)in[i]->names.size(), a->matrix.p + c0 * a->pitch, a->pitch, idx[i].p, in[i]->n_rows, st);
        c0 += in[i]->names.size();
    }
    DevBuf<int> d_bad; SKX_TRY(d_bad.alloc(1)); SKX_TRY(d_bad.zero(st));
    if (U) {
        launch_col_stats(a->matrix.p, a->pitch, (int)S, U, a->present.p, a->unambig.p, a->mask.p, d_bad.p, st);
        SKX_HIP(hipMemcpyAsync(a->vcount.p, a->present.p, U * 4, hipMemcpyDeviceToDevice, st));                                   // :172
    }
    SKX_HIP(hipStreamSynchronize(st));
    SKX_HIP(hipGetLastError());
    *out = a.release();
    return SKX_OK;
    });
}

extern "C" int skx_array_delete_samples(skx_array *a, const char *const *del_names, int n_del)
{
    return skx_guarded([&]() -> int {
    if (!a) { set_error("bad arguments"); return SKX_EINVAL; }
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    SKX_TRY(array_materialize(a));
    const size_t S = a->names.size();
    if (n_del <= 0 || (size_t)n_del == S) { set_error("Invalid number of samples to remove"); return SKX_EINVAL; }                // merge_ska_array.rs:232-234
    if (a->n_kmers != a->n_rows || a->keys_absent) { set_error("split k-mers and variants are out of step (filtered without update_kmers)"); return SKX_EINVAL; }
    // the request is a set of names; each must match a column (first match wins, :243-249)
    std::vector<std::string> want;
    for (int d = 0; d < n_del; d++) if (std::find(want.begin(), want.end(), del_names[d]) == want.end()) want.emplace_back(del_names[d]);
    std::vector<char> drop(S, 0);
    for (auto &w : want) {
        bool found = false;
        for (size_t s = 0; s < S && !found; s++) if (!drop[s] && a->names[s] == w) { drop[s] = 1; found = true; }
        if (!found) { set_error("Could not find sample(s): {\"%s\"}", w.c_str()); return SKX_EINVAL; }                           // :252-254
    }
    std::vector<std::string> names2;
    for (size_t s = 0; s < S; s++) if (!drop[s]) names2.push_back(a->names[s]);
    const size_t S2 = names2.size();
    if (S2 == 0) { set_error("Invalid number of samples to remove"); return SKX_EINVAL; }
    const uint64_t U = a->n_rows;
    DevBuf<uint8_t> nm; SKX_TRY(nm.alloc((uint64_t)S2 * a->pitch));
    size_t c = 0;
    for (size_t s = 0; s < S; s++) if (!drop[s]) { SKX_HIP(hipMemcpyAsync(nm.p + c * a->pitch, a->matrix.p + s * a->pitch, a->pitch, hipMemcpyDeviceToDevice, st)); c++; }
    SKX_HIP(hipStreamSynchronize(st));
    a->matrix = std::move(nm); a->names.swap(names2); a->total_samples = 0;
    // update_counts(false) (:139-163,270): recount, drop the rows no remaining sample has
    DevBuf<int> d_bad; SKX_TRY(d_bad.alloc(1)); SKX_TRY(d_bad.zero(st));
    DevBuf<uint8_t> keep; SKX_TRY(keep.alloc(U));
    if (U) {
        launch_col_stats(a->matrix.p, a->pitch, (int)S2, U, a->present.p, a->unambig.p, a->mask.p, d_bad.p, st);
        SKX_HIP(hipMemcpyAsync(a->vcount.p, a->present.p, U * 4, hipMemcpyDeviceToDevice, st));
        launch_nonzero_flags(a->present.p, U, keep.p, st);
    }
    return array_keep_rows(a, keep, nullptr);
    });
}

// delete_samples(everybody else) + apply_filters for a sample list, as a new array: one pass over the list's cells decides every row
// (launch_subset_verdicts), the scan places the kept ones and the compaction reads them through the list -- the n x pitch sub-matrix of
// the unfiltered rows is never made.  Device memory beside `a`: U bytes of keep, 8 (U + 1) of pos, the kept matrix.
extern "C" int skx_array_subset_filtered(skx_array *a, const int *samples, int n_samples, const skx_filter_spec *f, skx_array **out, skx_subset_info *info)
{
    return skx_guarded([&]() -> int {
    if (out) *out = nullptr;
    if (!a || !f || (n_samples > 0 && !samples)) { set_error("subset: bad arguments"); return SKX_EINVAL; }
    const size_t S = a->names.size();
    if (n_samples < 1) { set_error("subset: at least one sample is required"); return SKX_EINVAL; }
    if (f->two_stage != 0) { set_error("subset: the two-stage filter of `ska distance` does not apply to a subset"); return SKX_EINVAL; }
    if (!(f->min_freq >= 0.0 && f->min_freq <= 1.0)) { set_error("subset: min_freq must be between 0 and 1 (inclusive)"); return SKX_EINVAL; }
    std::vector<int> order(samples, samples + n_samples);
    for (int s : order) if (s < 0 || (size_t)s >= S) { set_error("subset: sample index %d out of range (the array has %zu samples)", s, S); return SKX_EINVAL; }
    std::sort(order.begin(), order.end());                                    // delete_samples leaves the columns in the array's order (:256-268)
    for (int i = 1; i < n_samples; i++) if (order[i] == order[i - 1]) { set_error("subset: sample index %d given twice", order[i]); return SKX_EINVAL; }
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    SKX_TRY(array_materialize(a));
    const uint64_t U = a->n_rows, n = (uint64_t)n_samples;
    const uint64_t thr = (uint64_t)std::ceil((double)n * f->min_freq);         // generic_modes.rs:118
    DevBuf<int> d_order, d_bad; DevBuf<uint8_t> keep; DevBuf<uint64_t> pos; DevBuf<unsigned long long> d_cnt;
    uint64_t kept = 0; unsigned long long cnt[3] = {0, 0, 0}; int bad = 0;
    {
        PhaseTimer pv("align.groups_verdicts");
        StageTimer t(ctx, &ctx->tm.filter);
        SKX_TRY(d_order.alloc(n)); SKX_TRY(d_bad.alloc(1)); SKX_TRY(d_bad.zero(st)); SKX_TRY(d_cnt.alloc(3)); SKX_TRY(d_cnt.zero(st));
        SKX_TRY(keep.alloc(U)); SKX_TRY(pos.alloc(U + 1));
        SKX_HIP(hipMemcpyAsync(d_order.p, order.data(), n * sizeof(int), hipMemcpyHostToDevice, st));
        launch_subset_verdicts(a->matrix.p, a->pitch, d_order.p, n_samples, U, thr, f->filter_ambig_as_missing != 0, f->filter_type, f->ignore_const_gaps != 0,
                               keep.p, d_cnt.p, d_bad.p, st);
        DevBuf<uint32_t> sc_sums; DevBuf<uint64_t> sc_offs;
        SKX_TRY(sc_sums.alloc(scan_u8_blocks(U))); SKX_TRY(sc_offs.alloc(scan_u8_blocks(U) + 1));
        if (out) {
            launch_scan_u8(keep.p, pos.p, U, sc_sums.p, sc_offs.p, st);
            SKX_HIP(hipMemcpyAsync(&kept, pos.p + U, 8, hipMemcpyDeviceToHost, st));
        }
        SKX_HIP(hipMemcpyAsync(cnt, d_cnt.p, sizeof cnt, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipMemcpyAsync(&bad, d_bad.p, 4, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipStreamSynchronize(st));                                     // (order[] is the host's again)
    }
    if (bad) { set_error("variants contain a byte outside -ACGTMRWSYKVHDBN (not supported on the device path)"); return SKX_EUNSUP; }
    const uint64_t rows_present = U - cnt[0];
    if (!out) kept = rows_present - cnt[1] - cnt[2];
    if (info) { info->rows_present = rows_present; info->removed = cnt[2]; info->silent = cnt[1]; info->sites = kept; }
    if (!out) { SKX_HIP(hipGetLastError()); return SKX_OK; }
    if (kept != rows_present - cnt[1] - cnt[2]) { set_error("subset: internal error: %llu rows placed, %llu counted", (unsigned long long)kept, (unsigned long long)(rows_present - cnt[1] - cnt[2])); return SKX_EINVAL; }
    PhaseTimer pr("align.groups_rows");
    std::unique_ptr<skx_array> b(new skx_array());
    b->ctx = ctx; b->k = a->k; b->rc = a->rc; b->k_bits = a->k_bits; b->hp = a->hp; b->wh = a->wh; b->version = a->version;
    for (int s : order) b->names.push_back(a->names[s]);
    // no split k-mers, as after skx_array_load_filtered; their number is what the chain's would be (update_kmers = false keeps the delete's,
    // update_counts(true) follows the rows)
    b->engine_order = false; b->keys_absent = true; b->n_kmers = f->filter_ambig_as_missing ? kept : rows_present;
    b->n_rows = kept; b->pitch = pitch_for(kept);
    {
        StageTimer t(ctx, &ctx->tm.compact);
        SKX_TRY(b->matrix.alloc(n * b->pitch));
        SKX_TRY(b->present.alloc(kept)); SKX_TRY(b->unambig.alloc(kept)); SKX_TRY(b->mask.alloc(kept)); SKX_TRY(b->vcount.alloc(kept));
        if (kept) {
            launch_compact_matrix(a->matrix.p, a->pitch, b->matrix.p, b->pitch, n_samples, U, keep.p, pos.p, f->mask_ambig != 0, st, d_order.p);
            // the statistics of the kept rows from the kept cells (after mask_ambig, like launch_mask_ambig_stats leaves them)
            launch_col_stats(b->matrix.p, b->pitch, n_samples, kept, b->present.p, b->unambig.p, b->mask.p, d_bad.p, st);
            SKX_HIP(hipMemcpyAsync(b->vcount.p, f->filter_ambig_as_missing ? b->unambig.p : b->present.p, kept * 4, hipMemcpyDeviceToDevice, st));
        }
        SKX_HIP(hipStreamSynchronize(st));
    }
    SKX_HIP(hipGetLastError());
    *out = b.release();
    return SKX_OK;
    });
}

// MergeSkaArray::weed (merge_ska_array.rs:452-487): rows whose split k-mer is (reverse: is not) in `weed` go.  variant_count is carried:
// a kept row keeps its stored count (array_keep_rows compacts vcount as it is) -- unlike merge and delete_samples above, which recount.
extern "C" int skx_array_weed(skx_array *a, skx_keyset *weed, int reverse, uint64_t *removed)
{
    return skx_guarded([&]() -> int {
    if (!a || !weed) { set_error("bad arguments"); return SKX_EINVAL; }
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    SKX_TRY(array_materialize(a));
    if (weed->k != a->k) { set_error("K-mer lengths do not match: %d %d", weed->k, a->k); return SKX_EINVAL; }
    if (weed->rc != a->rc) { set_error("Strand use inconsistent"); return SKX_EINVAL; }
    if (a->n_kmers != a->n_rows || a->keys_absent) { set_error("split k-mers and variants are out of step (filtered without update_kmers)"); return SKX_EINVAL; }
    const uint64_t U = a->n_rows;
    if (weed->logN >= 0) SKX_TRY(keyset_flatten(weed));
    DevBuf<uint8_t> keep; SKX_TRY(keep.alloc(U));
    if (a->k <= 31) {
        DevBuf<uint32_t> idx; SKX_TRY(idx.alloc(U));
        launch_lookup_rows(a->keys.p, U, weed->flat.p, weed->total, idx.p, st);
        launch_member_flags(idx.p, U, reverse, keep.p, st);                                                                       // merge_ska_array.rs:468
        SKX_HIP(hipStreamSynchronize(st));
    } else {
        DevBuf<uint64_t> tmp; const u128 *w = nullptr;
        if (U) SKX_TRY(array_wide_words(a, tmp, &w));
        DevBuf<uint32_t> idx; SKX_TRY(idx.alloc(U));
        launch_lookup_rows_wide(w, U, (const u128 *)weed->flat.p, weed->total, idx.p, st);
        launch_member_flags(idx.p, U, reverse, keep.p, st);
        SKX_HIP(hipStreamSynchronize(st));
    }
    return array_keep_rows(a, keep, removed);
    });
}

extern "C" int skx_array_fasta(skx_array *a, char **buf, uint64_t *len)
{
    return skx_guarded([&]() -> int {
    skx_ctx *ctx = a->ctx;
    SKX_HIP(hipSetDevice(ctx->device));
    SKX_TRY(array_materialize(a));
    const size_t S = a->names.size(); const uint64_t U = a->n_rows;
    uint64_t tot = 0;
    for (auto &nm : a->names) tot += nm.size() + U + 3;
    char *out = (char *)malloc(tot + 1), *p = out;
    if (!out) { set_error("out of host memory"); return SKX_ENOMEM; }
    for (size_t s = 0; s < S; s++) {
        *p++ = '>'; memcpy(p, a->names[s].data(), a->names[s].size()); p += a->names[s].size(); *p++ = '\n';
        if (U) { hipError_t e = hipMemcpy(p, a->matrix.p + s * a->pitch, U, hipMemcpyDeviceToHost); if (e != hipSuccess) { free(out); return hip_fail(e, "hipMemcpy"); } }
        p += U; *p++ = '\n';
    }
    *p = 0; *buf = out; *len = (uint64_t)(p - out);
    return SKX_OK;
    });
}
// write_fasta (merge_ska_array.rs:507-520) streamed to a file descriptor: batches of samples (header + row + newline) come off
// the device into pinned buffers; no copy of the alignment is held on the host.
//  * regular file opened read-write: the file is sized up front and mapped, and every batch is copied into the mapping by
//    several threads at once (page-cache pages of one file are filled in parallel; write()/pwrite() on one inode are serialised
//    by the kernel, which is what bounded the first version: 4.9 GB in 1.0 s);
//  * regular file, write-only: several batches in flight with pwrite at known offsets;
//  * pipe, or a descriptor opened with O_APPEND (`ska align x.skf >> out.aln`: Linux pwrite ignores the offset there and
//    appends): batches in order through write().
extern "C" int skx_array_write_fasta(skx_array *a, int fd)
{
    return skx_guarded([&]() -> int {
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    SKX_TRY(array_materialize(a));
    const size_t S = a->names.size(); const uint64_t U = a->n_rows;
    size_t max_rec = 0; uint64_t total = 0;
    for (auto &nm : a->names) { max_rec = std::max<size_t>(max_rec, nm.size() + U + 3); total += nm.size() + U + 3; }
    struct stat sb;
    const bool regular = fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode);
    const int fl = fcntl(fd, F_GETFL);
    const bool append = fl >= 0 && (fl & O_APPEND);
    off_t pos = regular ? lseek(fd, 0, SEEK_CUR) : 0;
    // ---- mapped output
    uint8_t *map = nullptr; size_t map_len = 0, map_skew = 0;
    if (regular && !append && pos >= 0 && fl >= 0 && (fl & O_ACCMODE) == O_RDWR && total) {
        const long pg = sysconf(_SC_PAGESIZE);
        map_skew = (size_t)(pos % pg);
        // the file is only ever grown: several writers (one per GPU) may each hold a window of the same file
        if ((off_t)sb.st_size >= pos + (off_t)total || ftruncate(fd, pos + (off_t)total) == 0) {
            map_len = total + map_skew;
            void *m = mmap(nullptr, map_len, PROT_READ | PROT_WRITE, MAP_SHARED, fd, pos - (off_t)map_skew);
            if (m != MAP_FAILED) map = (uint8_t *)m; else map_len = 0;
        }
    }
    struct Unmap { uint8_t *&p; size_t &n; ~Unmap() { if (p) munmap(p, n); } } unmap{map, map_len};
    // the file's pages are allocated by fallocate before the copies start (allocating a page-cache page inside a page fault
    // costs ~1 us and does not scale over the threads of one file; fallocate does ~12 GB/s on tmpfs, and copies that run beside
    // it contend with it: 4.9 GB in 0.8 s this way, 1.0 s with the copies chasing the allocation, 1.0-1.4 s through
    // write()/pwrite() -- tools/fasta_knobs.py); the first batches come off the device meanwhile
    std::shared_ptr<Preallocator> pre;
    std::atomic<bool> ok{true};                 // declared before the threads and slots that store to it
    std::atomic<bool> backed{false};
    struct Joiner { std::thread th; ~Joiner() { if (th.joinable()) th.join(); } } falloc;
    if (map) {
        if (a->prealloc && a->prealloc->fd == fd && a->prealloc->base == pos) pre = a->prealloc;      // started while the rows were being read
        else pre = std::make_shared<Preallocator>(fd, pos);
        a->prealloc.reset();
        // no copier touches the mapping before its pages exist; when they cannot be had the call fails with SKX_EIO as the write() path does
        falloc.th = std::thread([&backed, &ok, pre, total]() { pre->finish(total); if (pre->failed.load(std::memory_order_acquire)) ok = false; backed.store(true, std::memory_order_release); });
    }
    const size_t cap = std::max<size_t>(max_rec, map ? (32u << 20) : (64u << 20));
    const int NB = map ? 4 : (regular && !append && pos >= 0 ? 6 : 2);
    const int KT = map ? 4 : 1;                   // copier threads per batch (mapped output)

    struct Slot { char *p = nullptr; std::vector<std::thread> th; void join() { for (auto &t : th) if (t.joinable()) t.join(); th.clear(); }
                  ~Slot() { join(); if (p) (void)hipHostFree(p); } } slot[6];
    { PhaseTimer t_pin("fasta.pinned_buffers");
      for (int b = 0; b < NB; b++) if (hipHostMalloc((void **)&slot[b].p, cap, hipHostMallocDefault) != hipSuccess) { slot[b].p = nullptr; set_error("out of host memory"); return SKX_ENOMEM; } }
    int cur = 0, last = -1;
    double t_join = 0, t_d2h = 0;
    auto clk = [] { return std::chrono::steady_clock::now(); };
    auto sec = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    uint64_t done = 0;                          // bytes of the alignment handed to writers so far
    for (size_t s = 0; s < S && ok;) {
        Slot &sl = slot[cur];
        { const auto t0 = clk(); sl.join(); t_join += sec(t0, clk()); }
        char *buf = sl.p; size_t used = 0;
        const auto t1 = clk();
        while (s < S && used + a->names[s].size() + U + 3 <= cap) {
            const std::string &nm = a->names[s];
            buf[used++] = '>'; memcpy(buf + used, nm.data(), nm.size()); used += nm.size(); buf[used++] = '\n';
            if (U) SKX_HIP(hipMemcpyAsync(buf + used, a->matrix.p + s * a->pitch, U, hipMemcpyDeviceToHost, st));
            used += U; buf[used++] = '\n';
            s++;
        }
        SKX_HIP(hipStreamSynchronize(st));
        t_d2h += sec(t1, clk());
        if (map) {
            uint8_t *dst = map + map_skew + done;
            for (int t = 0; t < KT; t++) {
                const size_t lo = used * (size_t)t / KT, hi = used * (size_t)(t + 1) / KT;
                sl.th.emplace_back([dst, buf, lo, hi, &backed, &ok]() {
                    while (!backed.load(std::memory_order_acquire)) usleep(100);
                    if (!ok.load()) return;
                    memcpy(dst + lo, buf + lo, hi - lo);
                });
            }
        } else {
            if (NB == 2 && last >= 0) slot[last].join();                                     // keep the order on a pipe
            const off_t at = pos + (off_t)done;
            const bool positioned = NB > 2;
            sl.th.emplace_back([&ok, buf, used, fd, at, positioned]() {
                size_t w = 0;
                while (w < used) {
                    const ssize_t r = positioned ? pwrite(fd, buf + w, used - w, at + (off_t)w) : write(fd, buf + w, used - w);
                    if (r < 0 && errno == EINTR) continue;
                    if (r <= 0) { ok = false; return; }
                    w += (size_t)r;
                }
            });
        }
        done += used; last = cur; cur = (cur + 1) % NB;
    }
    { const auto t0 = clk(); for (int b = 0; b < NB; b++) slot[b].join(); t_join += sec(t0, clk()); }
    phase_add("fasta.device_to_pinned", t_d2h); phase_add("fasta.wait_for_writers", t_join);
    if (!ok) { set_error("write failed"); return SKX_EIO; }
    if (map || NB > 2) (void)lseek(fd, pos + (off_t)done, SEEK_SET);
    return SKX_OK;
    });
}
