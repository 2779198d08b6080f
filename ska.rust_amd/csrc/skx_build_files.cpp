// skx_build_files.cpp -- `ska build` from files: the two host pipelines that get sequence files onto the device (read sets through the
// pipelined form, everything else through the one-shot form) and the pinned upload ring both of them feed.  skx_dictset_build_files is the
// one ABI entry point here; the batch planner that calls it is in skx_api.cpp.
#include "skx_internal.h"
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstring>
#include <deque>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

using namespace skx;

namespace {
using Clock = std::chrono::steady_clock;
double secs_since(Clock::time_point t) { return std::chrono::duration<double>(Clock::now() - t).count(); }
long long us_since(Clock::time_point t) { return (long long)std::chrono::duration_cast<std::chrono::microseconds>(Clock::now() - t).count(); }
struct CloseFd { int fd; ~CloseFd() { if (fd >= 0) ::close(fd); } };
// a sequence file for one pass over it (-1: the error is set).  The pages are read once: without this hint every first access promotes its page on the
// kernel's LRU lists, under one lock for all reader threads (1 000 fresh 5 MB files on tmpfs: 0.47 s instead of 0.23 s for the same read() calls)
int open_for_one_pass(const char *f)
{
    const int fd = ::open(f, O_RDONLY);
    if (fd < 0) set_error("Invalid path/file: %s", f); else (void)posix_fadvise(fd, 0, 0, POSIX_FADV_NOREUSE);
    return fd;
}
}  // namespace

FileProbe skx::probe_file(const char *path, bool gz_trailer)
{
    FileProbe p;
    struct stat sb;
    const CloseFd cl{::open(path, O_RDONLY)};
    p.opened = cl.fd >= 0;
    if (!(p.opened ? fstat(cl.fd, &sb) == 0 : stat(path, &sb) == 0)) return p;
    p.found = true; p.regular = S_ISREG(sb.st_mode); p.size = (uint64_t)sb.st_size;
    if (p.opened && p.regular) p.n_head = (int)std::max<ssize_t>(0, ::read(cl.fd, p.head, 2));
    if (gz_trailer && p.gzip() && p.size > 18) p.has_tail = pread(cl.fd, p.tail, 4, (off_t)p.size - 4) == 4;
    return p;
}

namespace {

// ------------------------------------------------------------------------------------------ the pinned ring
// Slots of pinned host memory between the threads that read files and the device.  A reader takes a free slot, fills it and submits it with
// its destination; the uploader threads copy the queued pieces (each on a stream of its own, a batch at a time) and put the slots back.
// The uploaders end when the queue is empty and no reader is left; stop() makes every take() come back empty-handed at once.
class PinnedRing {
public:
    ~PinnedRing() { if (base_) (void)hipHostFree(base_); }
    bool allocate(int n_slots, size_t slot_bytes) {       // (on whichever thread: the one-shot form pins on a helper thread while it sizes its device buffers)
        if (hipHostMalloc((void **)&base_, (size_t)n_slots * slot_bytes, hipHostMallocDefault) != hipSuccess) { base_ = nullptr; return false; }
        for (int b = 0; b < n_slots; b++) free_slots.push_back(b);
        slot_bytes_ = slot_bytes; return true;
    }
    bool usable() const { return base_ != nullptr; }
    size_t slot_bytes() const { return slot_bytes_; }
    uint8_t *at(int slot) const { return base_ + (size_t)slot * slot_bytes_; }
    int take() {                                           // a free slot, waited for; -1: the ring was stopped
        const auto tw = Clock::now();
        std::unique_lock<std::mutex> lk(mu);
        cv_free.wait(lk, [&] { return !free_slots.empty() || stopped_; });
        us_waited += us_since(tw);
        if (stopped_) return -1;
        const int slot = free_slots.back(); free_slots.pop_back(); return slot;
    }
    void give_back(int slot) { { std::lock_guard<std::mutex> lk(mu); free_slots.push_back(slot); } cv_free.notify_one(); }
    void submit(int slot, uint8_t *dst, size_t bytes, int tag) { { std::lock_guard<std::mutex> lk(mu); work.push_back({slot, dst, bytes, tag}); in_flight_++; } cv_work.notify_one(); }
    // the only place the stop flag is set; on_stop wakes whoever waits on a condition of the caller's own under this ring's lock
    void stop(bool upload_failed) {
        { std::lock_guard<std::mutex> lk(mu); stopped_ = true; failed_ |= upload_failed; }
        cv_free.notify_all(); cv_work.notify_all(); if (on_stop) on_stop();
    }
    std::function<void()> on_stop;
    // state of the caller's own may live under the ring's lock (the read-set pipeline's device-slot pools do); the *_locked forms are for its holders
    std::mutex &mutex() { return mu; }
    bool stopped_locked() const { return stopped_; }
    int in_flight_locked() const { return in_flight_; }                 // pieces submitted and not yet on the device
    bool winding_down() { std::lock_guard<std::mutex> lk(mu); return stopped_ || readers_left == 0; }
    bool failed() { std::lock_guard<std::mutex> lk(mu); return failed_; }
    double waited_thread_s() const { return us_waited.load() * 1e-6; }   // what take() waited, summed over its callers
    // every reader thread holds one of these for as long as it may submit: the last to go wakes the uploaders, which then end
    void expect_readers(int n) { readers_left = n; }
    struct Reader { PinnedRing &r; explicit Reader(PinnedRing &r_) : r(r_) {} ~Reader() { { std::lock_guard<std::mutex> lk(r.mu); r.readers_left--; } r.cv_work.notify_all(); } };
    // on_landed(tag) is called under the ring's lock for every piece that has arrived
    void start_uploaders(int device, int n, std::function<void(int tag)> on_landed = nullptr) {
        for (int u = 0; u < n; u++) uploaders.emplace_back([this, device, on_landed]() {
            (void)hipSetDevice(device);
            hipStream_t up = nullptr;
            if (hipStreamCreateWithFlags(&up, hipStreamNonBlocking) != hipSuccess) up = nullptr;
            std::vector<Req> batch;
            for (;;) {
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv_work.wait(lk, [&] { return !work.empty() || readers_left == 0; });
                    if (work.empty() && readers_left == 0) break;
                    const size_t take = std::max<size_t>(1, work.size() / 2);          // leave work for the other uploader
                    batch.assign(work.begin(), work.begin() + (ptrdiff_t)take); work.erase(work.begin(), work.begin() + (ptrdiff_t)take);
                }
                bool bad = false;
                for (auto &r : batch) bad |= hipMemcpyAsync(r.dst, at(r.slot), r.bytes, hipMemcpyHostToDevice, up) != hipSuccess;
                bad |= hipStreamSynchronize(up) != hipSuccess;
                if (bad) stop(true);
                {
                    std::lock_guard<std::mutex> lk(mu);
                    for (auto &r : batch) { free_slots.push_back(r.slot); in_flight_--; if (on_landed) on_landed(r.tag); }
                }
                cv_free.notify_all();
            }
            if (up) (void)hipStreamDestroy(up);
        });
    }
    void join_uploaders() { for (auto &u : uploaders) u.join(); uploaders.clear(); }
private:
    struct Req { int slot; uint8_t *dst; size_t bytes; int tag; };
    uint8_t *base_ = nullptr; size_t slot_bytes_ = 0; std::mutex mu; std::condition_variable cv_free, cv_work;
    std::vector<int> free_slots; std::deque<Req> work; int readers_left = 0, in_flight_ = 0; bool stopped_ = false, failed_ = false;
    std::atomic<long long> us_waited{0}; std::vector<std::thread> uploaders;
};

// A cursor over a device destination: what is written through it fills pinned slots, and a slot leaves for its place behind the ones before it
// when `piece` bytes of it are filled (the slot's size unless the destination wants its pieces aligned otherwise).
class SlotCursor {
public:
    SlotCursor(PinnedRing &ring, uint8_t *dst, int tag = -1, size_t piece = 0) : ring_(ring), dst_(dst), tag_(tag), piece_(piece ? piece : ring.slot_bytes()) {}
    SlotCursor(const SlotCursor &) = delete; SlotCursor &operator=(const SlotCursor &) = delete;
    ~SlotCursor() { abandon(); }
    // where to write and how much fits, for a read() straight into the slot; nullptr: the ring was stopped
    uint8_t *room(size_t *n) {
        if (slot_ < 0) { if ((slot_ = ring_.take()) < 0) return nullptr; used_ = 0; }
        *n = piece_ - used_;
        return ring_.at(slot_) + used_;
    }
    void wrote(size_t n) { used_ += n; if (used_ >= piece_) flush(); }
    bool append(const uint8_t *p, size_t n) {               // false: the ring was stopped
        if (slot_ >= 0 && used_ + n < piece_) { memcpy(ring_.at(slot_) + used_, p, n); used_ += n; return true; }      // the common case: it fits the slot being filled
        while (n) {
            size_t fits; uint8_t *d = room(&fits);
            if (!d) return false;
            const size_t take = std::min(n, fits);
            memcpy(d, p, take); wrote(take);
            p += take; n -= take;
        }
        return true;
    }
    void flush() {                                                         // the partly filled slot leaves as it is
        if (slot_ < 0) return;
        if (used_) { ring_.submit(slot_, dst_ + off_, used_, tag_); pieces_++; } else ring_.give_back(slot_);
        off_ += used_; slot_ = -1; used_ = 0;
    }
    void abandon() { if (slot_ >= 0) ring_.give_back(slot_); slot_ = -1; used_ = 0; }      // what was not submitted is dropped
    uint64_t sent() const { return off_; }                               // bytes submitted
    uint64_t written() const { return off_ + used_; }
    int pieces() const { return pieces_; }
private:
    PinnedRing &ring_; uint8_t *dst_; int tag_; size_t piece_;
    int slot_ = -1, pieces_ = 0; size_t used_ = 0; uint64_t off_ = 0;
};

// A read set's records -> the five bit planes (groups of 64 positions x 5 words: two code bits, the bytes valid_base rejects, line ends,
// quality verdicts), fed line by line from stream_fastq_file; `push` takes a finished group.  Used by the reader threads that pack on the
// host and by the consumer when the device's framing calls a sample irregular (then it is this code that accepts or refuses the file).
struct PlanePacker {
    std::vector<uint64_t> pl;                                           // a record's four planes (sequence line, then its quality line)
    size_t line_n = 0;
    uint64_t cur[5] = {0, 0, 0, 0, 0}, pos = 0, cap = 0;                // the group being filled; positions so far; the most that may come
    int min_qual = 20; bool gz = false;
    std::function<int(const uint64_t *)> push;
    static constexpr int OVER_BOUND = -1002;                            // a gzip file longer than its trailer says: not an error of the input
    int emit(int which, const uint8_t *p, size_t nb)
    {
        const size_t words = (nb + 1 + 63) / 64;                        // the line and its end
        if (which == 0) {
            if (pos + nb + 1 > cap) { if (gz) return OVER_BOUND; skx::set_error("Invalid FASTA/Q record"); return SKX_EIO; }
            if (pl.size() < 4 * words) pl.resize(4 * words + 64);
            line_n = nb;
            for (int pln = 0; pln < 4; pln++) pl[pln * words + words - 1] = 0;
            skx::pack_bases_planes(p, nb, &pl[0], &pl[words], &pl[2 * words]);
            return SKX_OK;
        }
        if (nb != line_n) { skx::set_error("Invalid FASTA/Q record"); return SKX_EIO; }
        skx::pack_qual_plane(p, nb, min_qual, &pl[3 * words]);
        const uint64_t *lo = &pl[0], *hi = &pl[words], *bd = &pl[2 * words], *qb = &pl[3 * words];
        for (size_t w = 0; w < words; w++) {
            const unsigned take = (unsigned)std::min<size_t>(64, nb + 1 - 64 * w), off = (unsigned)(pos & 63);
            const uint64_t v[5] = {lo[w], hi[w], bd[w], nb / 64 == w ? 1ull << (nb & 63) : 0ull, qb[w]};
            for (int pln = 0; pln < 5; pln++) cur[pln] |= v[pln] << off;
            pos += take;
            if (off + take >= 64) {
                const int pr = push(cur); if (pr != SKX_OK) return pr;
                for (int pln = 0; pln < 5; pln++) cur[pln] = off ? v[pln] >> (64 - off) : 0ull;      // (what did not fit; bits beyond `take` are zero)
            }
        }
        return SKX_OK;
    }
    int finish() { return (pos & 63) ? push(cur) : SKX_OK; }           // the last, partly filled group
    // a sample's files through the plain-FASTQ line reader into this packer, the last group included
    int pack_files(const SampleFiles &files, bool any_gz, int not_fastq)
    {
        const std::function<int(int, const uint8_t *, size_t)> to_emit = [&](int which, const uint8_t *p, size_t nb) -> int { return emit(which, p, nb); };
        for (const char *f : files) {
            int r = stream_fastq_file(f, to_emit);
            if (r == SKF_NOT_TAKEN && !any_gz) { set_error("Invalid FASTA/Q record"); r = SKX_EIO; }      // (the first byte was '@' a moment ago)
            if (r == SKF_NOT_TAKEN || r == OVER_BOUND) r = not_fastq;                                 // (a gzip file that is not FASTQ: the one-shot form takes the batch)
            if (r != SKX_OK) return r;
        }
        return finish();
    }
};
constexpr int SKF_OVER_BOUND = PlanePacker::OVER_BOUND;

// ------------------------------------------------------------------------------------------ read sets, pipelined
// Read sets (every sample plain FASTQ, one or two files), pipelined.  The one-shot form below reads every sample, allocates stream buffers the
// size of all files together (24 GB for 96 isolates of BASELINE config 5's shape: a 1-3 s allocation when the memory has just been released
// by another process) and then filters one isolate after the other (11 ms each) on an idle PCIe link.  Here a small pool of stream slots
// (two device buffers per slot, sized for the largest sample) is filled by the reader threads through the pinned ring, and this thread runs a
// sample's window / count-filter kernels (reads_sample_words) as soon as its last piece has arrived, then hands the slot back: reading,
// upload and kernels overlap, and the device holds a few samples' text instead of all of it.  Results are those of the one-shot form
// (the per-sample kernels do not depend on the order samples arrive in).  SKF_NOT_TAKEN: not this kind of input, or a sample the
// partition kernels leave to the sort-based form -- the caller takes the one-shot path from the start.
struct ReadsPipeline {
    static constexpr size_t SLOT = ((8u << 20) / READ_GROUP_BYTES) * READ_GROUP_BYTES;          // whole groups
    static constexpr size_t RAW_CHUNK = (SLOT - 1) / 256 * 256;                                 // raw text leaves in pieces that keep their destinations aligned
    static constexpr int n_up = 2;
    skx_ctx *ctx; const char *const *file1, *const *file2; const int n, k, rc; const skx_qual *q; const int threads;
    const Clock::time_point t0 = Clock::now();
    // what probe() finds and size_pools() makes of it
    struct GzSizes { uint64_t comp[2] = {0, 0}, hint[2] = {0, 0}; int files = 0, gz_files = 0; bool all_gz() const { return gz_files == files; } };
    std::vector<uint64_t> bound, text_bytes;
    std::vector<GzSizes> gzs;                                                  // (a sample whose files are all gzip may be inflated on the device)
    uint64_t slot_bytes = 0, raw_cap = 0, comp_cap = 0, pslot_bytes = 0, rslot_bytes = 0, gslot_bytes = 0;
    int nt = 1, P = 0, R = 0, G = 0, gz_tail = 0, gz_feed = 0, n_gz_samples = 0, n_slots = 0, min_qual_host = 20;
    long raw_knob = 0; bool any_gz = false;
    // the device slots, and the thread that allocates all but the first of each kind INTO raw_slots / gz_slots: joined before they go (the destructor)
    DevBuf<uint8_t> packed_pool, raw_planes, gz_text;
    std::vector<DevBuf<uint8_t>> raw_slots, gz_slots;
    std::thread slot_alloc; PinnedRing ring;
    // under the ring's lock: the device-slot pools and the samples' progress
    struct Sample { int slot = -1, pieces = 0, landed = 0; bool read_done = false, raw = false, gzdev = false; uint64_t len = 0, junction = 0, coff[2] = {0, 0}; };
    std::condition_variable cv_stream, cv_ready;
    std::vector<int> free_stream, free_raw, free_gz; std::deque<int> ready;
    int raw_active = 0; bool prefer_packed = false;
    std::vector<Sample> smp;
    std::vector<int> rcodes; std::vector<std::string> errs;                  // the readers' verdicts
    std::atomic<long long> us_wait_stream{0}, us_files{0}, n_raw{0}, n_gzdev{0}, bytes_up{0};      // summed over the reader threads
    std::atomic<int> next{0};
    std::vector<DevBuf<uint64_t>> wl, wh2; std::vector<uint64_t> cnt;       // the consumer's: the samples' passing words
    int done = 0, krc = SKX_OK, n_irregular = 0, n_gz_host = 0, inflight = -1;      // inflight: the sample in the device's inflater
    double t_kernels = 0.0, t_frame = 0.0, t_inflate = 0.0; Clock::time_point t_sample;
    FastqScratch fsc;
    GzDevWork gzw[2];                                                          // the inflater's ONE set of buffers (a sample's two files)
    // a gzip sample's two files are decoded on streams of their own, beside each other AND beside the kernels of the samples the reader threads
    // inflated (this thread goes on with those while a decode is in flight, one at a time: the inflater's buffers are one set)
    struct Aux {
        hipStream_t s[2] = {nullptr, nullptr}; hipEvent_t ev[3] = {nullptr, nullptr, nullptr}; GzDevFileInfo *fi = nullptr;      // (events, verdicts: [file]; ev[2]: a sample's text is made)
        ~Aux() { for (auto x : s) if (x) (void)hipStreamDestroy(x); for (auto e : ev) if (e) (void)hipEventDestroy(e); if (fi) (void)hipHostFree(fi); }
    } aux;
    ReadsPipeline(skx_ctx *ctx_, const char *const *f1, const char *const *f2, int n_, int k_, int rc_, const skx_qual *q_, int threads_)
        : ctx(ctx_), file1(f1), file2(f2), n(n_), k(k_), rc(rc_), q(q_), threads(threads_), bound(n_, 0), text_bytes(n_, 0), gzs(n_), smp(n_), rcodes(n_, SKX_OK), errs(n_),
          wl(n_), wh2(n_), cnt(n_, 0) { ring.on_stop = [this] { cv_stream.notify_all(); cv_ready.notify_all(); }; }
    ~ReadsPipeline() { join_slot_alloc(); }                                    // (before any member goes)
    void join_slot_alloc() { if (slot_alloc.joinable()) slot_alloc.join(); }
    SampleFiles files(int i) const { return sample_files(file1, file2, i); }
    void stop() { ring.stop(false); }
    bool probe() {                                         // every file plain FASTQ or gzip: sizes and bounds.  false: not this kind of input
        for (int i = 0; i < n; i++) {
            uint64_t bytes = 0;
            for (const char *f : files(i)) {
                const FileProbe p = probe_file(f, true);
                bool ok = p.opened && p.regular && p.n_head == 2;
                uint64_t plain = ok ? p.size : 0;
                if (ok && p.gzip()) {
                    // gzip: the reader thread inflates as it goes; the stream's size from the trailer (ISIZE, the last member's length mod 2^32).  A
                    // batch in which a file turns out longer than that says is left to the one-shot form (SKF_OVER_BOUND below)
                    ok = p.has_tail;
                    plain = (uint64_t)p.tail[0] | ((uint64_t)p.tail[1] << 8) | ((uint64_t)p.tail[2] << 16) | ((uint64_t)p.tail[3] << 24);
                    // a trailer that cannot be the whole text (shorter than the file itself): several members -- bgzip's 64 KB blocks, files
                    // joined with cat -- or 4 GB and more.  Six times the file's size then stands for the text's length (reads deflate 3-5 x);
                    // a text that turns out longer sends the batch to the one-shot form like any file longer than its bound
                    if (ok && plain < p.size) plain = 6 * p.size;
                    any_gz = true;
                    gzs[i].gz_files++;
                } else ok = ok && p.head[0] == '@';
                if (!ok) return false;
                if (gzs[i].files < 2) { gzs[i].comp[gzs[i].files] = p.size; gzs[i].hint[gzs[i].files] = plain; }
                gzs[i].files++;
                bytes += plain;
            }
            if (gzs[i].all_gz()) comp_cap = std::max<uint64_t>(comp_cap, ((gzs[i].comp[0] + 64 + 255) & ~255ull) + (gzs[i].files > 1 ? ((gzs[i].comp[1] + 64 + 255) & ~255ull) : 0ull));
            bound[i] = (bytes / 2 + 64 + 255) & ~255ull;                             // plain FASTQ holds at most half its bytes in either stream
            text_bytes[i] = bytes;
            slot_bytes = std::max(slot_bytes, bound[i]);
            raw_cap = std::max(raw_cap, bytes);
        }
        return true;
    }
    void size_pools() {
        nt = std::max(1, std::min({threads, n, 64, cpu_budget()}));      // (parsing + packing: a reader keeps a CPU busy)
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        // a slot per reader thread and a few waiting for their kernels: more only costs allocation time (64 slots = 17 GB took 4.7 s right after
        // another process had released the memory, 32 slots 0.26 s: profiles/r03zr_reads_pipeline_512.log)
        // A sample crosses PCIe in one of two forms, chosen by its reader thread when it starts on it (round 6):
        //   * PACKED -- bit planes, groups of 64 positions, five words each: two code bits, the bases valid_base rejects, the line ends, the quality
        //     verdicts (fastx.cpp pack_*_planes) -- framed and packed by the reader thread: 5 bits per position instead of two bytes, 157 MB per 50x
        //     isolate, 0.1-0.3 s of a CPU;
        //   * RAW -- the file's bytes as read() delivers them (0.55 GB per 50x isolate), the reader thread does nothing else; the device frames the
        //     records and makes the same planes (skx_fastq.hip).
        // Raw text alone is bound by the link (~32 GB/s with the readers running = 60 isolates/s), packing alone by the CPUs (16 of them: 40-80
        // isolates/s); a reader takes RAW while the pinned ring has room -- the link is keeping up -- and PACKED when it is filling up, so
        // both are busy.  SKX_KNOBS=reads_raw=1: never raw; =2: always.  The window pass and the rebuild of the passing windows' words read the planes
        // as they are, whoever made them.
        //   * GZDEV (gzip files) -- the COMPRESSED bytes as read() delivers them, half to a fifth of the text: the reader thread does nothing else, and
        //     the device inflates (skx_gzdev.hip: block finder, symbolic decode per 64 KB chunk, window maps, text, member lengths and CRCs), frames and
        //     packs.  A file the device does not vouch for (damaged, unusual header, a stretch that deflates beyond the symbol area) goes through the
        //     reader threads' inflater on this thread, which accepts it or words the error.  SKX_KNOBS=reads_gz=1: inflate on the reader threads.
        raw_knob = knob("reads_raw");
        const bool raw_possible = raw_knob != 1 && raw_cap + 2 < 0xFFFFFF00ull;
        //     Both inflaters work at once: a few reader threads (gz_feed of them) only feed the device -- a 50x isolate is 0.1-0.3 s of read() for them
        //     and ~50 ms of the device's inflater -- and the others inflate and hand over text or planes as before (~1.1 s of a thread an isolate);
        //     all take their samples from the same counter, so the split follows the two rates.  reads_gz=2: the device only.
        const long gz_knob = knob("reads_gz");
        const bool gz_device = any_gz && raw_possible && comp_cap > 0 && gz_knob != 1;
        gz_tail = (int)(knob("reads_gz_tail") > 0 ? knob("reads_gz_tail") : 20);
        gz_feed = !gz_device ? 0 : gz_knob == 2 ? 1 << 30 : (int)std::max<long>(1, knob("reads_gz_feed") > 0 ? knob("reads_gz_feed") : 3);
        for (int i = 0; i < n; i++) if (gz_device && gzs[i].all_gz()) n_gz_samples++;
        pslot_bytes = ((slot_bytes / 64 + 2) * READ_GROUP_BYTES + 255) & ~255ull;
        rslot_bytes = raw_possible ? ((raw_cap + 2 + 64 + 255) & ~255ull) : 0;
        // Two pools of device slots: packed samples (157 MB each at 50x of 5 Mbp; a reader each and a few waiting for their kernels) and raw ones
        // (0.55 GB each: a few -- the link carries about one at a time -- plus ONE buffer for the planes the device makes of them, since the
        // kernels take a sample at a time).  Kept small on purpose: a pool of 24 slots that hold either form is 17 GB, and allocating that right
        // after another process has released its memory took 1.4-1.9 s of a 3 s build (profiles/r06b_reads_modes.log).
        P = (int)std::min<uint64_t>((uint64_t)n, std::max<uint64_t>(2, std::min<uint64_t>((uint64_t)nt + 8, (free_b / 8) / (pslot_bytes + 1))));
        // raw slots: up to one per reader and two waiting for their kernels (a reader holds its slot for as long as it reads -- 0.1 s of a file read
        // before, 0.25 s of one read for the first time, when sixteen read()s contend for the page cache's LRU lock -- so six slots carried 24 raw
        // samples a second at most and the link idled at 12 GB/s: profiles/r06d_reads_1000.log).  They are allocated one by one by a helper thread
        // while the pipeline already runs on the packed pool: 11 GB taken at once right after another process released its memory cost 1.4-1.9 s.
        R = raw_possible ? (int)std::min<uint64_t>((uint64_t)n, std::max<uint64_t>(2, std::min<uint64_t>(raw_knob == 2 || (any_gz && !gz_device) ? (uint64_t)nt + 2 : gz_device ? (uint64_t)std::max(1, (nt - std::min(gz_feed, nt)) / 2) + 2 : (uint64_t)std::max(1, nt / 8) + 3, (free_b / 8) / (rslot_bytes + 1)))) : 0;      // (beside the device's inflater: half the inflating readers send text, the others planes)
        // slots for compressed samples: one per reader and a few waiting for the inflater (0.27 GB each at 50x of 5 Mbp); the text the device makes of
        // a sample lives in ONE buffer (the kernels take a sample at a time)
        gslot_bytes = gz_device ? comp_cap : 0;
        G = gz_device ? (int)std::min<uint64_t>((uint64_t)n_gz_samples, std::max<uint64_t>(2, std::min<uint64_t>((uint64_t)std::min(gz_feed, nt) + 3, (free_b / 8) / (gslot_bytes + 1)))) : 0;
        if (raw_knob == 2) P = 1;
        min_qual_host = q ? (int)q->min_qual : 20;
        n_slots = 2 * nt + 8;
    }
    // the first slot of every kind and the pinned ring now, the other raw / compressed slots on a thread of their own while the pipeline runs
    int allocate() {
        raw_slots.resize((size_t)R); gz_slots.resize((size_t)G);
        SKX_TRY(packed_pool.alloc((uint64_t)P * pslot_bytes));
        if (R) { SKX_TRY(raw_planes.alloc(pslot_bytes)); SKX_TRY(raw_slots[0].alloc(rslot_bytes)); }
        if (G) { SKX_TRY(gz_text.alloc(rslot_bytes)); SKX_TRY(gz_slots[0].alloc(gslot_bytes)); }
        if (!ring.allocate(n_slots, SLOT)) return SKF_NOT_TAKEN;
        for (int p = 0; p < P; p++) free_stream.push_back(p);
        if (R) free_raw.push_back(0);
        if (G) free_gz.push_back(0);
        ring.expect_readers(nt);
        slot_alloc = std::thread([this]() {
            (void)hipSetDevice(ctx->device);
            auto grow = [this](std::vector<DevBuf<uint8_t>> &slots, std::vector<int> &free_list, uint64_t bytes) {
                for (size_t p = 1; p < slots.size(); p++) {
                    if (ring.winding_down() || slots[p].alloc(bytes) != SKX_OK) return;      // (no room: the pipeline goes on with what there is)
                    { std::lock_guard<std::mutex> lk(ring.mutex()); free_list.push_back((int)p); }
                    cv_stream.notify_all();
                }
            };
            grow(gz_slots, free_gz, gslot_bytes);
            grow(raw_slots, free_raw, rslot_bytes);
        });
        return SKX_OK;
    }
    void mark_ready_locked(int i) {      // (every sample is queued by whoever sees its last piece arrive)
        Sample &x = smp[i];
        if (x.read_done && x.landed == x.pieces) { ready.push_back(i); cv_ready.notify_all(); }      // (true once: at the last piece, or at read_done when all have landed)
    }
    bool choose_form(int i, bool feeder) {                 // which form sample i travels in, and a device slot for it; false: the pipeline was stopped
        const auto tw = Clock::now();
        std::unique_lock<std::mutex> lk(ring.mutex());
        // the link keeps up (few filled pieces of the pinned ring wait for their copy) and a raw slot is to be had: this sample goes as it
        // is; otherwise it is packed here.  (reads_raw=2: raw whatever the ring says -- then a raw slot is waited for.)
        // Measured (profiles/r06e_reads_modes.log, 16 readers): files read before -- packed 124 isolates/s through the pipeline, raw 91 (the link:
        // 46 GB/s), and a reader's time is the read() either way (0.10 s of its 0.11 s per isolate: packing is what fits beside it); files
        // read for the first time -- 35 isolates/s in every form (sixteen read()s of fresh tmpfs pages share 26 GB/s).  So raw text is
        // what relieves a processor that packs slowly or inflates (gzip: every sample raw), and beside fast packers only a sample or two
        // at a time travel raw, on bandwidth the link has left.
        const int raw_most = any_gz ? nt : std::max(1, nt / 8);
        auto want_raw = [&] { return R > 0 && !prefer_packed && (raw_knob == 2 || (!free_raw.empty() && raw_active < raw_most && ring.in_flight_locked() * 4 <= n_slots)); };
        // a sample of gzip files: its compressed bytes, the device inflates (unless a sample before it turned out irregular: then the
        // readers inflate and pack, as they do for plain files)
        auto want_gzdev = [&] { return G > 0 && feeder && gzs[i].all_gz() && !prefer_packed; };
        cv_stream.wait(lk, [&] { return ring.stopped_locked() || (want_gzdev() ? !free_gz.empty() : want_raw() ? !free_raw.empty() : !free_stream.empty()); });
        us_wait_stream += us_since(tw);
        if (ring.stopped_locked()) return false;
        Sample &s = smp[i];
        s.gzdev = want_gzdev();
        s.raw = !s.gzdev && want_raw();
        std::vector<int> &fl = s.gzdev ? free_gz : s.raw ? free_raw : free_stream;
        s.slot = fl.back(); fl.pop_back();
        if (s.raw) raw_active++;
        return true;
    }
    // COMPRESSED: the files as they are, each followed by zeros to the next multiple of 256 bytes (at least 64: the inflater's bit reader looks ahead)
    int read_compressed(int i, SlotCursor &cur) {
        n_gzdev++;
        int fno = 0;
        for (const char *f : files(i)) {
            const uint64_t want = gzs[i].comp[fno];
            smp[i].coff[fno++] = cur.written();
            const CloseFd cl{open_for_one_pass(f)}; const int fd = cl.fd;
            if (fd < 0) return SKX_EIO;
            for (uint64_t got_file = 0; got_file < want;) {
                size_t room; uint8_t *dstp = cur.room(&room);
                if (!dstp) return SKF_ABORTED;
                const ssize_t rd = ::read(fd, dstp, std::min<uint64_t>(room, want - got_file));
                if (rd < 0 && errno == EINTR) continue;
                if (rd < 0) { set_error("Invalid path/file: %s", f); return SKX_EIO; }
                if (rd == 0) return SKF_OVER_BOUND;                        // (the file shrank since it was measured: the one-shot form takes the batch)
                cur.wrote((size_t)rd); got_file += (uint64_t)rd;
            }
            static const uint8_t zeros[64 + 256] = {0};
            if (!cur.append(zeros, (size_t)(((want + 64 + 255) & ~255ull) - want))) return SKF_ABORTED;
        }
        return SKX_OK;
    }
    // RAW: the files' bytes into the pinned ring, nothing else: plain files by read() straight into a slot, gzip files inflated by this
    // thread's inflater and copied there.  A '\n' is put behind a file that lacks its last one (the device frames lines by their ends)
    int read_raw(int i, SlotCursor &cur, uint64_t &junction) {
        n_raw++;
        const uint64_t cap = text_bytes[i] + 2;
        int fno = 0;
        for (const char *f : files(i)) {
            if (fno++ == 1) junction = cur.written();
            const CloseFd cl{open_for_one_pass(f)}; const int fd = cl.fd;
            if (fd < 0) return SKX_EIO;
            unsigned char mg[2] = {0, 0};
            const bool gz = pread(fd, mg, 2, 0) == 2 && mg[0] == 0x1f && mg[1] == 0x8b;
            std::unique_ptr<GzReader> zr;
            if (gz) { zr.reset(new GzReader); zr->open(fd); }
            static const uint8_t nl = '\n';
            uint8_t last = nl; bool first = true;
            const uint64_t file_at = cur.written();
            for (;;) {
                size_t room; uint8_t *dstp = cur.room(&room);           // (room > 0: a full piece has left)
                if (!dstp) return SKF_ABORTED;
                if (zr) {
                    const uint8_t *np; size_t ng;
                    // (the inflater hands out what it has, up to its window: copied piecewise into the slots)
                    if (zr->next(&np, &ng, 0) != 0) { set_error("Invalid path/file: %s", f); return SKX_EIO; }
                    if (ng == 0) break;
                    if (cur.written() + ng > cap) return SKF_OVER_BOUND;
                    if (first && np[0] != '@') return SKF_OVER_BOUND;      // (a gzip file that is not FASTQ: the one-shot form takes the batch)
                    if (!cur.append(np, ng)) return SKF_ABORTED;
                    first = false; last = np[ng - 1];
                    continue;
                }
                const ssize_t rd = ::read(fd, dstp, std::min<uint64_t>(room, cap - cur.written()));
                if (rd < 0 && errno == EINTR) continue;
                if (rd < 0) { set_error("Invalid path/file: %s", f); return SKX_EIO; }
                if (rd == 0) {
                    // (the file grew since it was measured: what the bound was made from no longer holds)
                    if (cur.written() >= cap) { char c1; if (::read(fd, &c1, 1) > 0) { set_error("Invalid FASTA/Q record"); return SKX_EIO; } }
                    break;
                }
                if (first) { first = false; if (dstp[0] != '@') { set_error("Invalid FASTA/Q record"); return SKX_EIO; } }
                last = dstp[rd - 1];
                cur.wrote((size_t)rd);
            }
            if (cur.written() == file_at) { set_error("Invalid path/file: %s", f); return SKX_EIO; }
            if (last != nl && !cur.append(&nl, 1)) return SKF_ABORTED;
        }
        return SKX_OK;
    }
    int read_packed(int i, SlotCursor &cur, PlanePacker &pk) {      // PACKED: framed and packed here, the groups of planes into the ring
        pk.pos = 0; pk.cap = bound[i] - 32; for (auto &c : pk.cur) c = 0;
        pk.push = [&cur](const uint64_t *grp) -> int { return cur.append((const uint8_t *)grp, READ_GROUP_BYTES) ? SKX_OK : SKF_ABORTED; };
        return pk.pack_files(files(i), any_gz, SKF_OVER_BOUND);
    }
    void reader_thread(int t) {
        const bool feeder = t < gz_feed;                              // (this thread hands gzip samples to the device's inflater)
        PinnedRing::Reader leave(ring);
        PlanePacker pk; pk.min_qual = min_qual_host; pk.gz = any_gz;
        for (int i;;) {
            // the batch's last samples are left to the feeders: a thread that starts inflating one now (~1.1 s) would finish after the device has
            // been through all of them (~50 ms each)
            if (!feeder && gz_feed > 0 && n_gz_samples == n && n - next.load() < gz_tail) { std::lock_guard<std::mutex> lk(ring.mutex()); if (!prefer_packed) break; }
            if ((i = next.fetch_add(1)) >= n) break;
            if (!choose_form(i, feeder)) return;
            const auto t_files = Clock::now();
            Sample &s = smp[i];
            SlotCursor cur(ring, s.gzdev ? gz_slots[(size_t)s.slot].p : s.raw ? raw_slots[(size_t)s.slot].p : packed_pool.p + (uint64_t)s.slot * pslot_bytes, i, s.gzdev || s.raw ? RAW_CHUNK : SLOT);
            uint64_t junction = 0;
            int r = s.gzdev ? read_compressed(i, cur) : s.raw ? read_raw(i, cur, junction) : read_packed(i, cur, pk);
            if (r == SKX_OK) cur.flush();
            bytes_up += (long long)cur.sent();
            if (s.raw) { std::lock_guard<std::mutex> lk(ring.mutex()); raw_active--; }
            if (r != SKX_OK && r != SKF_ABORTED) { rcodes[i] = r; errs[i] = skx_last_error(); }      // (only the failure that started it is reported)
            if (r != SKX_OK) { stop(); return; }                          // (the cursor gives its slot back as it goes)
            us_files += us_since(t_files);
            std::lock_guard<std::mutex> lk(ring.mutex());
            s.len = s.gzdev || s.raw ? cur.sent() : pk.pos; s.junction = junction; s.pieces = cur.pieces(); s.read_done = true;
            mark_ready_locked(i);
        }
    }
    // the inflater's streams, events and verdict words, and its buffers at the size of the batch's largest file, before the first decode (see gz_device_reserve)
    int prepare_inflater() {
        for (int f = 0; f < 2; f++) SKX_HIP(hipStreamCreateWithFlags(&aux.s[f], hipStreamNonBlocking));
        for (auto &e : aux.ev) SKX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        SKX_HIP(hipHostMalloc((void **)&aux.fi, 2 * sizeof(GzDevFileInfo), hipHostMallocDefault));
        for (int i = 0; i < n; i++)
            for (int f = 0; gzs[i].all_gz() && f < gzs[i].files; f++) SKX_TRY(gz_device_reserve(gzw[f], gzs[i].comp[f], gzs[i].hint[f]));
        return SKX_OK;
    }
    int gz_start(int i) {
        const uint8_t *comp = gz_slots[(size_t)smp[i].slot].p;
        for (int f = 0; f < gzs[i].files; f++) {
            SKX_TRY(gz_device_decode(ctx, aux.s[f], comp + smp[i].coff[f], gzs[i].comp[f], gzs[i].hint[f], gzw[f]));
            SKX_HIP(hipMemcpyAsync(&aux.fi[f], gzw[f].finfo.p, sizeof(GzDevFileInfo), hipMemcpyDeviceToHost, aux.s[f]));
            SKX_HIP(hipEventRecord(aux.ev[f], aux.s[f]));
        }
        inflight = i; return SKX_OK;
    }
    bool gz_decoded(int i) const { for (int f = 0; f < gzs[i].files; f++) if (hipEventQuery(aux.ev[f]) != hipSuccess) return false; return true; }
    // the next gzip sample's decode starts as soon as this one's text is made (the inflater's buffers are free then: the streams wait for that
    // on the device), beside this one's framing and window kernels
    int start_next_gz(bool after_text) {
        int j = -1;
        { std::lock_guard<std::mutex> lk(ring.mutex()); if (!ready.empty() && smp[ready.front()].gzdev) { j = ready.front(); ready.pop_front(); } }
        if (j < 0) return SKX_OK;
        if (after_text) {
            SKX_HIP(hipEventRecord(aux.ev[2], ctx->stream));
            for (int f = 0; f < 2; f++) SKX_HIP(hipStreamWaitEvent(aux.s[f], aux.ev[2], 0));
        }
        return gz_start(j);
    }
    // a sample through the host reader on this thread: what the device's framing calls irregular, and gzip files the device's inflater does not
    // vouch for -- the reader accepts what is merely unusual and words the error for what is wrong
    int planes_by_host_reader(int i, uint8_t *slot_p, uint64_t &positions) {
        std::vector<uint64_t> hp;
        PlanePacker pk; pk.min_qual = min_qual_host; pk.gz = any_gz; pk.cap = bound[i] - 32;
        pk.push = [&](const uint64_t *grp) -> int { hp.insert(hp.end(), grp, grp + 5); return SKX_OK; };
        int hr = pk.pack_files(files(i), any_gz, SKF_NOT_TAKEN);                  // (not FASTQ after all, or longer than its bound: the one-shot form takes the batch)
        if (hr == SKX_OK && !hp.empty() && hipMemcpyAsync(slot_p, hp.data(), hp.size() * 8, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) hr = SKX_ENODEV;
        if (hr == SKX_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) hr = SKX_ENODEV;      // (hp goes)
        positions = pk.pos;
        return hr;
    }
    // the device called the sample's text irregular: it goes through the host reader here and now, and the readers pack the samples that follow
    int irregular_after_all(int i, uint8_t *slot_p, uint64_t &positions) {
        { std::lock_guard<std::mutex> lk(ring.mutex()); prefer_packed = true; n_irregular++; }
        return planes_by_host_reader(i, slot_p, positions);
    }
    // compressed bytes: both files decoded to symbols side by side, the verdicts and lengths read back, then the text of one behind the
    // other's (a '\n' behind a file that lacks its last one, as the raw form's readers put it), member CRCs checked, and the device's framing
    int planes_by_device_inflate(int i, uint8_t *slot_p, uint64_t &positions) {
        const int nf = gzs[i].files;
        GzDevFileInfo fi[2] = {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}};
        bool vouched = true;
        int r = SKX_OK;
        for (int f = 0; f < nf && r == SKX_OK; f++) {
            if (hipEventSynchronize(aux.ev[f]) != hipSuccess) r = SKX_ENODEV;
            fi[f] = aux.fi[f];
        }
        uint64_t junction = 0, len = 0;
        if (r == SKX_OK) {
            for (int f = 0; f < nf; f++) vouched = vouched && fi[f].status == 0 && fi[f].total > 0;
            if (vouched) {
                junction = nf > 1 ? fi[0].total + (fi[0].last != '\n') : 0;
                len = (nf > 1 ? junction + fi[1].total + (fi[1].last != '\n') : fi[0].total + (fi[0].last != '\n'));
                if (len > text_bytes[i] + 2 || len + 64 > gz_text.n || fi[0].first != '@' || (nf > 1 && fi[1].first != '@')) vouched = false;      // (the host reader decides what it is)
            }
        }
        if (r == SKX_OK && vouched) {
            hipStream_t st = ctx->stream;
            uint64_t at = 0;
            for (int f = 0; f < nf && r == SKX_OK; f++) {
                r = gz_device_text(ctx, st, gzw[f], gz_text.p + at, fi[f].total, fi[f].n_members);
                at += fi[f].total;
                if (r == SKX_OK && fi[f].last != '\n') { if (hipMemsetAsync(gz_text.p + at, '\n', 1, st) != hipSuccess) r = SKX_ENODEV; at++; }
            }
            for (int f = 0; f < nf && r == SKX_OK; f++)
                if (hipMemcpyAsync(&fi[f], gzw[f].finfo.p, sizeof(GzDevFileInfo), hipMemcpyDeviceToHost, st) != hipSuccess) r = SKX_ENODEV;
            if (r == SKX_OK) r = start_next_gz(true);
            t_inflate += secs_since(t_sample);
            int irregular = 0;
            if (r == SKX_OK) r = fastq_frame_planes(ctx, gz_text.p, len, junction, min_qual_host, (uint64_t *)slot_p, fsc, &positions, &irregular);      // (returns with the stream idle)
            for (int f = 0; f < nf; f++) vouched = vouched && fi[f].status == 0;                                                                   // (the members' CRCs)
            if (r == SKX_OK && vouched && irregular) r = irregular_after_all(i, slot_p, positions);
        }
        if (r == SKX_OK && !vouched) {
            if (inflight < 0) r = start_next_gz(false);
            if (knob("gz_debug"))
                fprintf(stderr, "gz on device: sample %d (%s) not vouched for: status %u / %u, text %llu / %llu bytes, first bytes %u / %u\n", i, file1[i], fi[0].status, fi[1].status,
                        (unsigned long long)fi[0].total, (unsigned long long)fi[1].total, fi[0].first, fi[1].first);
            n_gz_host++; r = planes_by_host_reader(i, slot_p, positions);
        }
        return r;
    }
    // raw text: the device frames the records and makes the planes; a text it calls irregular goes through the host reader here and now (which
    // accepts what is merely unusual -- blank lines between records -- and words the error for what is wrong), and the readers pack the
    // samples that follow: files of one run tend to share their quirks
    int planes_by_device_framing(int i, uint8_t *slot_p, uint64_t &positions) {
        int irregular = 0;
        const int r = fastq_frame_planes(ctx, raw_slots[(size_t)smp[i].slot].p, smp[i].len, smp[i].junction, min_qual_host, (uint64_t *)slot_p, fsc, &positions, &irregular);
        return r == SKX_OK && irregular ? irregular_after_all(i, slot_p, positions) : r;
    }
    void consume() {
        // (the reader threads are running: a failure here stops the pipeline the way a failed kernel does)
        if (G && (krc = prepare_inflater()) != SKX_OK) stop();
        const skx_qual qs = q ? *q : skx_qual{5, 20, SKX_QUAL_STRICT};
        while (done < n) {
            int i = -1; bool resume = false;
            {
                std::unique_lock<std::mutex> lk(ring.mutex());
                cv_ready.wait(lk, [&] { return !ready.empty() || ring.stopped_locked() || inflight >= 0; });
                if (ring.stopped_locked()) break;
                // the sample in the inflater is taken up again when its decode has ended, when nothing else waits, or when the next one needs the inflater
                if (inflight >= 0 && (ready.empty() || smp[ready.front()].gzdev || gz_decoded(inflight))) resume = true;
                else { i = ready.front(); ready.pop_front(); }
            }
            if (resume) { i = inflight; inflight = -1; }
            else if (smp[i].gzdev) {
                if ((krc = gz_start(i)) != SKX_OK) { stop(); break; }
                continue;
            }
            t_sample = Clock::now();
            const Sample &s = smp[i];
            uint8_t *slot_p = s.raw || s.gzdev ? raw_planes.p : packed_pool.p + (uint64_t)s.slot * pslot_bytes;      // where the sample's planes are
            uint64_t positions = s.len;
            if (s.gzdev) krc = planes_by_device_inflate(i, slot_p, positions);
            else if (s.raw) krc = planes_by_device_framing(i, slot_p, positions);
            if (s.gzdev || s.raw) t_frame += secs_since(t_sample);               // (a packed sample's planes are there: its reader made them)
            // (the kernels read the packed planes themselves: the two record streams never exist in memory)
            if (krc == SKX_OK) krc = reads_sample_words(ctx, nullptr, nullptr, positions, k, rc, qs, wl[i], wh2[i], &cnt[i], (const uint64_t *)slot_p);      // (returns with the stream idle: the slot is free)
            t_kernels += secs_since(t_sample);
            { std::lock_guard<std::mutex> lk(ring.mutex()); (s.gzdev ? free_gz : s.raw ? free_raw : free_stream).push_back(s.slot); }
            cv_stream.notify_all();
            if (krc != SKX_OK) break;
            done++;
        }
        if (done < n) stop();
    }
    // upload failure first, then the kernels' verdict (SKF_NOT_TAKEN included: the one-shot form takes the batch -- the readers it interrupted
    // recorded nothing), then the reader whose own failure stopped the pipeline
    int verdict(skx_dictset **out) {
        if (ring.failed()) { set_error("upload of the sequence files failed"); return SKX_ENODEV; }
        if (krc != SKX_OK) return krc;
        for (int i = 0; i < n; i++) if (rcodes[i] == SKF_OVER_BOUND) return SKF_NOT_TAKEN;
        for (int i = 0; i < n; i++) if (rcodes[i] != SKX_OK) { set_error("%s", errs[i].c_str()); return rcodes[i]; }
        if (done < n) { set_error("internal: read-set pipeline stopped early"); return SKX_EUNSUP; }
        join_slot_alloc();
        packed_pool.release(); raw_planes.release(); raw_slots.clear(); gz_slots.clear(); gz_text.release();
        for (auto &g : gzw) g = GzDevWork();
        const auto t1 = Clock::now();
        skx_dictset *d = nullptr;
        SKX_TRY(reads_words_to_dictset(ctx, wl, wh2, cnt, k, rc, &d));            // (SKF_NOT_TAKEN: regions beyond the LDS sort -- the sort-based form, from the files)
        phase_add("build.dictionaries", secs_since(t1));
        for (int s = 0; s < n; s++)
            if ((d->sorted ? d->sample_size[s] : d->raw_total[s]) == 0) { set_error("%s has no valid sequence", file1[s]); delete d; return SKX_EEMPTY; }
        *out = d;
        return SKX_OK;
    }
    int run(skx_dictset **out) {
        if (!probe()) return SKF_NOT_TAKEN;
        SKX_HIP(hipSetDevice(ctx->device));
        size_pools();
        SKX_TRY(allocate());
        phase_add("build.alloc_text_pin_ring", secs_since(t0));
        ring.start_uploaders(ctx->device, n_up, [this](int i) { smp[i].landed++; mark_ready_locked(i); });
        std::vector<std::thread> pool;
        for (int t = 0; t < nt; t++) pool.emplace_back([this, t]() { reader_thread(t); });
        consume();
        for (auto &th : pool) th.join();
        ring.join_uploaders();
        phase_add("build.read_upload", secs_since(t0));
        phase_add("build.reads_kernels_overlapped", t_kernels);
        phase_add("build.reads_device_framing_overlapped", t_frame);
        phase_add("build.readers_files_thread_s", us_files.load() * 1e-6);               // parse + pack, waits for pinned slots included
        phase_add("build.readers_wait_pinned_thread_s", ring.waited_thread_s());
        phase_add("build.readers_wait_device_slot_thread_s", us_wait_stream.load() * 1e-6);
        phase_add("build.reads_samples_sent_raw", (double)n_raw.load());
        phase_add("build.reads_samples_sent_compressed", (double)n_gzdev.load());
        phase_add("build.reads_samples_inflated_on_host_after_all", (double)n_gz_host);
        phase_add("build.reads_device_inflate_overlapped", t_inflate);
        phase_add("build.reads_samples_irregular", (double)n_irregular);
        phase_add("build.reads_uploaded_GB", (double)bytes_up.load() * 1e-9);
        return verdict(out);
    }
};

// ------------------------------------------------------------------------------------------ every other input, one shot
// Reader threads.  A plain (uncompressed, single-file) FASTA sample is not parsed on the host at all: its bytes are read
// into pinned memory and uploaded as they are, and the device strips headers and line breaks (skx_parse.hip) -- the host
// side of an assembly is one read() and one asynchronous copy.  FASTQ, .gz and two-file samples are parsed by the host
// reader (fastx.cpp) and uploaded as record streams.  Either way the uploads of some samples run beside the reading of
// others, each thread on its own stream.
struct FilesBuild {
    static constexpr size_t SLOT = 8u << 20;
    static constexpr int n_up = 2;                                               // two streams keep both copy engines busy
    skx_ctx *ctx; const char *const *file1, *const *file2; const int n, k, rc; const skx_qual *q; const int threads; const double proportion_reads;
    std::vector<int> rcodes; std::vector<std::string> errs;
    std::vector<DevBuf<uint8_t>> d_seq, d_qual;
    std::vector<uint64_t> raw_len, slot_off, slot_len;
    std::vector<char> is_raw;
    std::vector<skx_stream> ss;
    bool device_parse = false, any_pair = false, ring_ok = false, raw_ok = false;
    int nt = 1;
    Clock::time_point t_read0;
    // one device buffer for all raw texts and one for all record streams (a slot per single-file sample, sized from stat):
    // two allocations whatever the number of samples
    DevBuf<uint8_t> raw_all, out_all, hs_seq_all, hs_qual_all;
    std::vector<uint64_t> hs_off, hs_len;
    std::vector<uint8_t> hs_fq;
    PinnedRing ring;
    std::thread warm_thread, pin_thread;                                         // (joined on every exit: the destructor)
    std::atomic<int> next{0};
    FilesBuild(skx_ctx *ctx_, const char *const *f1, const char *const *f2, int n_, int k_, int rc_, const skx_qual *q_, int threads_, double proportion)
        : ctx(ctx_), file1(f1), file2(f2), n(n_), k(k_), rc(rc_), q(q_), threads(threads_), proportion_reads(proportion), rcodes(n_, SKX_OK), errs(n_), d_seq(n_), d_qual(n_),
          raw_len(n_, 0), slot_off(n_, 0), slot_len(n_, 0), is_raw(n_, 0), ss(n_), hs_off(n_, 0), hs_len(n_, 0), hs_fq(n_, 0)
    {
        size_t step = 1;
        if (proportion_reads > 0.0) { step = (size_t)std::llround(1.0 / proportion_reads); if (step == 0) step = 1; }
        device_parse = step == 1 && !knob("host_parse");
        t_read0 = Clock::now();
        for (int i = 0; file2 && i < n; i++) any_pair |= file2[i] != nullptr;
        nt = std::max(1, std::min({threads, n, any_pair ? 64 : 32, std::max(8, 2 * cpu_budget())}));      // (paired read sets are parsed on the host: CPU work, more threads pay)      // 5 GB of FASTA text: 0.43 / 0.24 / 0.24 / 0.32 s with 8 / 16 / 32 / 64 readers (tools/read_knobs.py)
    }
    ~FilesBuild() { for (std::thread *t : {&warm_thread, &pin_thread}) if (t->joinable()) t->join(); }
    SampleFiles files(int i) const { return sample_files(file1, file2, i); }
    static int upload_failed() { set_error("upload of the sequence files failed"); return SKX_ENODEV; }
    // The regions' word buffer -- the largest allocation of a build, ~10 bytes per base -- is asked for now, on a thread of its own, and put back
    // into the allocator's cache, where dictset_build_device finds it: as a box's first GPU process the allocation waits ~1 s for memory the
    // driver hands out for the first time (build.dictionaries 0.98 s of a 2.46 s `ska build`, profiles/r06f_bench_full.json), and that second
    // can pass beside the reading of the files.  The size is the one dictset_build_device computes (region_layout) if the longest sample is as long
    // as the largest plain file says (headers and line ends make it ~2 % more: the cache hands out a block up to a quarter larger than asked).
    void prewarm_word_buffer() {
        if (!device_parse || any_pair || n < 8 || knob("no_prewarm")) return;
        uint64_t maxlen = 0; bool plain = true;
        for (int i = 0; i < n && plain; i++) { struct stat sb; if (stat(file1[i], &sb) != 0 || !S_ISREG(sb.st_mode)) plain = false; else maxlen = std::max<uint64_t>(maxlen, (uint64_t)sb.st_size); }
        for (int i = 0; i < n && plain; i++) { const size_t L = strlen(file1[i]); if (L > 3 && (!strcmp(file1[i] + L - 3, ".gz") || !strcmp(file1[i] + L - 3, ".xz") || !strcmp(file1[i] + L - 4, ".bz2") || !strcmp(file1[i] + L - 4, ".zst"))) plain = false; }
        if (!plain || maxlen <= (1u << 20)) return;
        const RegionLayout lay = region_layout(maxlen, k);
        if (lay.logB < 0) return;
        const uint64_t bytes = (((uint64_t)n << lay.logB) * lay.cap * (k > 31 ? 2 : 1) + 2048) * 8;
        size_t free_b = 0, total_b = 0;
        (void)hipSetDevice(ctx->device);
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && bytes < free_b / 2) {
            const int dev = ctx->device;
            warm_thread = std::thread([bytes, dev]() { (void)hipSetDevice(dev); hipError_t e = hipSuccess; if (void *p = dev_alloc(bytes, &e)) dev_free(p); });
        }
    }
    // Raw path plumbing: reader threads make no HIP calls at all (creating a stream or a pinned buffer per thread serialises in
    // the runtime: 64 threads spent 0.28 s each waiting for theirs).  They read() file pieces into the slots of ONE pinned ring;
    // the uploaders issue the copies and recycle the slots.  The ring is pinned by a helper thread while
    // this one sizes and allocates the device buffers.
    int size_and_allocate() {
        if (!device_parse) return SKX_OK;
        // (a thread streaming a FASTQ sample fills a sequence and a quality slot at a time: two per thread and a few in flight)
        const int n_slots = any_pair ? 2 * nt + 8 : std::max(4, std::min(2 * nt, 32));
        pin_thread = std::thread([this, n_slots]() { (void)hipSetDevice(ctx->device); (void)ring.allocate(n_slots, SLOT); });
        // only plain FASTA text is parsed on the device (a slot in raw_all and out_all each); a FASTQ or gzip sample reserves nothing there (raw_upload
        // would refuse it and its two slots would stay allocated, uncounted by the batch planner).
        // The samples the host reader will parse (two files, FASTQ): one buffer for all their record streams and one for the quality
        // streams, a slot each bounded from the file sizes -- plain FASTQ holds at most half its bytes in either stream, plain FASTA
        // all of them; gzip (size unknown) keeps an allocation of its own.  No device allocation per sample from the reader threads
        // (64 of them for 32 isolates queued behind one another: most of 5 s).
        uint64_t tot = 0, htot = 0; bool any_q = false;
        for (int i = 0; i < n; i++) {
            uint64_t bytes = 0; bool fq = false, ok = true;
            for (const char *f : files(i)) {
                const FileProbe p = probe_file(f);
                if (!(p.opened && p.regular && p.n_head >= 1 && (p.head[0] == '@' || p.head[0] == '>'))) ok = false;
                else { bytes += p.size; fq |= p.head[0] == '@'; }
            }
            if (!ok || !bytes) continue;
            if (files(i).n == 1 && !fq) { slot_off[i] = tot; slot_len[i] = (bytes + 64 + 255) & ~255ull; tot += slot_len[i]; continue; }
            hs_off[i] = htot; hs_len[i] = ((fq ? bytes / 2 : bytes) + 64 + 255) & ~255ull; hs_fq[i] = fq ? 1 : 0;
            htot += hs_len[i]; any_q |= fq;
        }
        SKX_HIP(hipSetDevice(ctx->device));
        if (tot) { SKX_TRY(raw_all.alloc(tot)); SKX_TRY(out_all.alloc(tot)); }
        if (htot) { SKX_TRY(hs_seq_all.alloc(htot)); if (any_q) SKX_TRY(hs_qual_all.alloc(htot)); }
        pin_thread.join();
        phase_add("build.alloc_text_pin_ring", secs_since(t_read0));
        ring_ok = ring.usable();                                                 // the pinned ring + uploader threads carry raw files and host-parsed streams alike (no pinned memory: every sample takes the host reader)
        raw_ok = ring_ok && raw_all.p;
        return SKX_OK;
    }
    // raw upload of a plain FASTA file: SKX_OK (taken), SKF_NOT_TAKEN (use the host reader), or an error
    int raw_upload(int i) {
        if (!slot_len[i]) return SKF_NOT_TAKEN;
        const CloseFd cl{open_for_one_pass(file1[i])}; const int fd = cl.fd;
        if (fd < 0) return SKF_NOT_TAKEN;                                    // the host reader reports it
        const uint64_t cap = slot_len[i] - 64;                               // the size stat reported
        SlotCursor cur(ring, raw_all.p + slot_off[i]);
        while (cur.written() < cap) {
            size_t room; uint8_t *buf = cur.room(&room);
            if (!buf) return upload_failed();
            const size_t want = (size_t)std::min<uint64_t>(room, cap - cur.written());
            size_t got = 0;
            while (got < want) { const ssize_t r = read(fd, buf + got, want - got); if (r < 0 && errno == EINTR) continue; if (r <= 0) break; got += (size_t)r; }
            if (cur.written() == 0 && got && buf[0] != '>') return SKF_NOT_TAKEN;      // FASTQ ('@'), gzip (1f 8b), anything else: the host reader's
            if (got == 0) break;                                                 // the file shrank under us: what was read is the file
            cur.wrote(got);
        }
        cur.flush();
        if (cur.sent() == 0) return SKF_NOT_TAKEN;
        raw_len[i] = cur.sent(); is_raw[i] = 1;
        return SKX_OK;
    }
    // a plain FASTQ sample: its files' lines go straight from a small read buffer into pinned slots -- one filling with sequence
    // lines, one with quality lines -- which the uploaders copy to the sample's places in the two stream buffers
    int stream_fastq(int i) {
        SlotCursor seq(ring, hs_seq_all.p + hs_off[i]), qual(ring, hs_qual_all.p + hs_off[i]);
        const uint64_t cap = hs_len[i] - 32;
        static const uint8_t nl = '\n';
        const std::function<int(int, const uint8_t *, size_t)> emit = [&](int which, const uint8_t *p, size_t nb) -> int {
            SlotCursor &x = which ? qual : seq;
            if (x.written() + nb + 1 > cap) { set_error("Invalid FASTA/Q record"); return SKX_EIO; }      // (more sequence than half the file: not FASTQ)
            return x.append(p, nb) && x.append(&nl, 1) ? SKX_OK : upload_failed();
        };
        for (const char *f : files(i)) {
            int r = stream_fastq_file(f, emit);
            if (r == SKF_NOT_TAKEN && f != file1[i]) { set_error("Invalid FASTA/Q record"); r = SKX_EIO; }      // file 2 is parsed in file 1's mode (ska_dict.rs:356-366)
            if (r != SKX_OK) return r;                                   // (SKF_NOT_TAKEN: the first file, before anything was emitted)
        }
        seq.flush(); qual.flush();
        if (seq.sent() != qual.sent()) { set_error("Invalid FASTA/Q record"); return SKX_EIO; }
        ss[i].seq = hs_seq_all.p + hs_off[i]; ss[i].qual = hs_qual_all.p + hs_off[i]; ss[i].len = seq.sent();
        return SKX_OK;
    }
    // the parsed streams travel through the pinned ring like the raw files (a copy from pageable memory goes through the
    // runtime's one staging path: 32 reader threads shared ~3 GB/s, 5.6 s for 32 isolates); the uploads are complete when the
    // uploader threads have been joined, which is before anything reads them
    int upload_parsed(DevBuf<uint8_t> &own, uint8_t *dst, const std::vector<uint8_t> &src, size_t len, hipStream_t &up_st, uint8_t **where) {
        if (!dst) { (void)hipSetDevice(ctx->device); SKX_TRY(own.alloc(len + 16)); dst = own.p; }      // no slot (gzip, a stream longer than its bound)
        *where = dst;
        if (!ring_ok) {
            (void)hipSetDevice(ctx->device);
            if (!up_st && hipStreamCreateWithFlags(&up_st, hipStreamNonBlocking) != hipSuccess) up_st = nullptr;
            if (len) { SKX_HIP(hipMemcpyAsync(dst, src.data(), len, hipMemcpyHostToDevice, up_st)); SKX_HIP(hipStreamSynchronize(up_st)); }
            return SKX_OK;
        }
        SlotCursor cur(ring, dst);
        if (!cur.append(src.data(), len)) return upload_failed();
        cur.flush();
        return SKX_OK;
    }
    int host_reader(int i, HostStream &h, hipStream_t &up_st) {      // a sample through the host reader (fastx.cpp) and its record streams to the device
        SKX_TRY(read_sample_stream(files(i).f[0], files(i).f[1], proportion_reads, h));
        const size_t len = h.seq.size();
        const bool fits = hs_len[i] && len + 16 <= hs_len[i] && (!h.is_fastq || hs_qual_all.p);
        uint8_t *at_seq = nullptr, *at_qual = nullptr;
        SKX_TRY(upload_parsed(d_seq[i], fits ? hs_seq_all.p + hs_off[i] : nullptr, h.seq, len, up_st, &at_seq));
        if (h.is_fastq) SKX_TRY(upload_parsed(d_qual[i], fits ? hs_qual_all.p + hs_off[i] : nullptr, h.qual, len, up_st, &at_qual));
        ss[i].seq = at_seq; ss[i].qual = h.is_fastq ? at_qual : nullptr; ss[i].len = len;
        return SKX_OK;
    }
    void reader_thread() {
        PinnedRing::Reader leave(ring);
        hipStream_t up_st = nullptr;                                             // host-reader path only, created on first use
        struct Drop { hipStream_t &s; ~Drop() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } } } drop{up_st};
        HostStream h;                                                            // (its buffers live across this thread's samples: no fresh pages per sample)
        for (int i; (i = next.fetch_add(1)) < n;) {
            int r = raw_ok ? raw_upload(i) : SKF_NOT_TAKEN;
            if (r == SKF_NOT_TAKEN && ring_ok && hs_len[i] && hs_fq[i] && hs_qual_all.p) r = stream_fastq(i);
            if (r == SKF_NOT_TAKEN) r = host_reader(i, h, up_st);
            if (r != SKX_OK) { rcodes[i] = r; errs[i] = skx_last_error(); }
        }
    }
    int read_and_upload() {
        ring.expect_readers(nt);
        if (ring_ok) ring.start_uploaders(ctx->device, n_up);
        std::vector<std::thread> pool;
        for (int t = 0; t < nt; t++) pool.emplace_back([this]() { reader_thread(); });
        for (auto &th : pool) th.join();
        ring.join_uploaders();
        phase_add("build.read_upload", secs_since(t_read0));
        if (ring.failed()) return upload_failed();
        for (int i = 0; i < n; i++) if (rcodes[i] != SKX_OK) { set_error("%s", errs[i].c_str()); return rcodes[i]; }
        return SKX_OK;
    }
    int parse_on_device() {                                // the raw FASTA texts -> record streams, all files in one set of launches
        PhaseTimer t_parse("build.device_fasta_parse");
        SKX_HIP(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        std::vector<int> idx;
        for (int i = 0; i < n; i++) if (is_raw[i]) idx.push_back(i);
        const int m = (int)idx.size();
        if (m) {
            std::vector<const uint8_t *> h_raw(m); std::vector<uint8_t *> h_out(m); std::vector<uint64_t> h_len(m), h_base(m + 1, 0);
            for (int j = 0; j < m; j++) {
                const int i = idx[j];
                h_raw[j] = raw_all.p + slot_off[i]; h_out[j] = out_all.p + slot_off[i]; h_len[j] = raw_len[i];
                h_base[j + 1] = h_base[j] + fasta_parse_tiles(raw_len[i]);
            }
            const uint64_t tiles = h_base[m];
            std::vector<uint32_t> h_tf(tiles);
            for (int j = 0; j < m; j++) std::fill(h_tf.begin() + (ptrdiff_t)h_base[j], h_tf.begin() + (ptrdiff_t)h_base[j + 1], (uint32_t)j);
            DevBuf<const uint8_t *> g_raw; DevBuf<uint8_t *> g_out; DevBuf<uint64_t> g_len, g_outlen, g_base, g_off, g_sum; DevBuf<uint32_t> g_tf; DevBuf<uint8_t> g_kind;
            SKX_TRY(g_raw.alloc(m)); SKX_TRY(g_out.alloc(m)); SKX_TRY(g_len.alloc(m)); SKX_TRY(g_outlen.alloc(m)); SKX_TRY(g_base.alloc(m + 1));
            SKX_TRY(g_off.alloc(tiles)); SKX_TRY(g_sum.alloc(tiles)); SKX_TRY(g_tf.alloc(tiles)); SKX_TRY(g_kind.alloc(tiles));
            SKX_HIP(hipMemcpyAsync(g_raw.p, h_raw.data(), m * sizeof(void *), hipMemcpyHostToDevice, st));
            SKX_HIP(hipMemcpyAsync(g_out.p, h_out.data(), m * sizeof(void *), hipMemcpyHostToDevice, st));
            SKX_HIP(hipMemcpyAsync(g_len.p, h_len.data(), m * 8, hipMemcpyHostToDevice, st));
            SKX_HIP(hipMemcpyAsync(g_base.p, h_base.data(), (m + 1) * 8, hipMemcpyHostToDevice, st));
            if (tiles) SKX_HIP(hipMemcpyAsync(g_tf.p, h_tf.data(), tiles * 4, hipMemcpyHostToDevice, st));
            launch_fasta_parse(g_raw.p, g_len.p, g_out.p, g_outlen.p, g_tf.p, g_base.p, tiles, g_sum.p, g_off.p, g_kind.p, m, st);
            std::vector<uint64_t> h_outlen(m);
            SKX_HIP(hipMemcpyAsync(h_outlen.data(), g_outlen.p, m * 8, hipMemcpyDeviceToHost, st));
            SKX_HIP(hipStreamSynchronize(st));
            SKX_HIP(hipGetLastError());
            for (int j = 0; j < m; j++) { const int i = idx[j]; ss[i].seq = out_all.p + slot_off[i]; ss[i].qual = nullptr; ss[i].len = h_outlen[j]; }
        }
        raw_all.release();
        return SKX_OK;
    }
    int build_dictionaries(skx_dictset **out) {
        skx_dictset *d = nullptr;
        if (warm_thread.joinable()) { PhaseTimer t_w("build.wait_for_word_buffer"); warm_thread.join(); }
        const auto t_dev0 = Clock::now();
        int r = skx_dictset_build(ctx, ss.data(), n, 1, k, rc, q, &d);
        phase_add("build.dictionaries", secs_since(t_dev0));
        if (r == SKX_EEMPTY) {      // "{file} has no valid sequence" (ska_dict.rs:374-376)
            int bad = 0; sscanf(skx_last_error(), "sample %d", &bad);
            set_error("%s has no valid sequence", file1[bad]);
        }
        if (r != SKX_OK) return r;
        *out = d;
        return SKX_OK;
    }
};
}  // namespace

extern "C" int skx_dictset_build_files(skx_ctx *ctx, const char *const *file1, const char *const *file2, int n, int k, int rc,
                                       const skx_qual *q, int threads, double proportion_reads, skx_dictset **out)
{
    return skx_guarded([&]() -> int {
    if (!ctx || !file1 || n <= 0 || !out) { set_error("bad arguments"); return SKX_EINVAL; }
    SKX_TRY(check_k(k));
    if (!(proportion_reads > 0.0) && !knob("host_parse") && !knob("reads_sort") && !knob("no_reads_pipeline") && n >= 2) {
        ReadsPipeline reads(ctx, file1, file2, n, k, rc, q, threads);
        const int pr = reads.run(out);
        if (pr != SKF_NOT_TAKEN) return pr;
    }
    FilesBuild b(ctx, file1, file2, n, k, rc, q, threads, proportion_reads);
    b.prewarm_word_buffer();
    SKX_TRY(b.size_and_allocate());
    SKX_TRY(b.read_and_upload());
    SKX_TRY(b.parse_on_device());
    return b.build_dictionaries(out);
    });
}
