// skx_dictset.cpp -- construction of a skx_dictset (the host side of the build stage): record streams -> (sample, bucket) regions of packed
// words, as extracted (assemblies: what the append pass reads) or sorted and folded (a sample's SkaDict: per region in LDS, or as one flat
// list where the regions are beyond the LDS sort), and the dictset part of the C ABI (build / size / export / free).
#include "skx_internal.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <numeric>

using namespace skx;

extern "C" void skx_dictset_free(skx_dictset *d) { delete d; }
extern "C" int skx_dictset_nsamples(const skx_dictset *d) { return d->n; }
extern "C" int skx_dictset_key_bits(const skx_dictset *d) { return d->key_bits; }

static std::unique_ptr<skx_dictset> new_dictset(skx_ctx *ctx, int n, int k, int rc, int logB)
{
    std::unique_ptr<skx_dictset> d(new skx_dictset());
    d->ctx = ctx; d->n = n; d->k = k; d->rc = rc; d->logB = logB; d->hp = make_hash_params(std::min(k, 31)); d->wh = make_wide_hash(k);
    d->key_bits = k > 31 ? 128 : 64;                            // lib.rs:592: u64 for k <= 31, u128 above
    return d;
}

static void launch_dedupe_stage(skx_ctx *ctx, skx_dictset *d, uint32_t cap, int *flag, uint32_t typical, uint32_t *big_list, uint32_t big_from)
{
    const uint64_t nreg = (uint64_t)d->n << d->logB;
    StageTimer t(ctx, &ctx->tm.dedupe);
    if (d->wide()) launch_dedupe_wide((u128 *)d->words.p, d->off.p, d->raw.p, d->ucnt.p, nreg, cap, 2 * (d->k - 1) - d->logB, flag, d->sidx.p, d->sb, ctx->stream);
    else launch_dedupe_mb(d->words.p, d->off.p, d->raw.p, d->ucnt.p, nreg, cap, d->hp.bits - d->logB, flag, d->sidx.p, d->sb, ctx->stream, typical, big_list, big_from);
}

// The regions of a dictset sorted and folded in place (a sample's SkaDict per bucket: dedupe_mb_kernel / dedupe_wide_kernel), and the samples'
// sizes with them.  lds_cap bounds every raw[region] and is at most lds_sort_max: the launch shapes hold that many words, so a region the
// kernels report as not fitting is an internal error (`what` names the layout in its message).
// typical (0: unknown, one launch shape): a size all but ~5 in 10 000 regions stay below, which may need a smaller launch shape than the
// regions' capacity does (launch_dedupe_mb; 64-bit keys only)
// LDS capacity (words) of the per-region counting sort for regions of up to lds_cap words: 12 B per word, <= 160 KiB
static uint32_t dedupe_launch_cap(uint32_t lds_cap, bool wide)
{
    return std::max<uint32_t>(512, (uint32_t)std::min<uint64_t>(((uint64_t)lds_cap + 255) / 256 * 256, lds_sort_max(wide)));
}
static int dedupe_regions(skx_ctx *ctx, skx_dictset *d, uint32_t lds_cap, uint32_t typical, const char *what)
{
    hipStream_t st = ctx->stream;
    const bool wide = d->wide();
    const uint64_t nreg = (uint64_t)d->n << d->logB;
    const uint32_t cap = dedupe_launch_cap(lds_cap, wide);
    if (wide) typical = 0;
    DevBuf<int> d_flag; SKX_TRY(d_flag.alloc(1));
    DevBuf<uint32_t> d_big;
    if (typical) SKX_TRY(d_big.alloc(nreg + 1));
    SKX_TRY(d_flag.zero(st));
    SKX_HIP(hipMemsetAsync(d->sidx.p, 0xFF, nreg * skx::SUBIDX * sizeof(uint16_t), st));     // 0xFFFF = sub-range without words
    launch_dedupe_stage(ctx, d, cap, d_flag.p, typical, d_big.p, 0);
    int overflow = 0;
    SKX_HIP(hipMemcpyAsync(&overflow, d_flag.p, 4, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    for (uint32_t from = dedupe_spill_grid(); !wide && (overflow & 4); from += dedupe_spill_grid()) {     // more listed regions than one grid of the second stage
        int keep = overflow & ~4;
        SKX_HIP(hipMemcpyAsync(d_flag.p, &keep, 4, hipMemcpyHostToDevice, st));
        launch_dedupe_stage(ctx, d, cap, d_flag.p, typical, d_big.p, from);
        SKX_HIP(hipMemcpyAsync(&overflow, d_flag.p, 4, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipStreamSynchronize(st));
    }
    if (getenv("SKX_DEBUG") && typical) {
        uint32_t listed = 0;
        SKX_HIP(hipMemcpy(&listed, d_big.p, 4, hipMemcpyDeviceToHost));
        fprintf(stderr, "[skx] dedupe: typical region %u words, capacity %u; %u of %llu regions above the typical launch shape\n", typical, cap, listed, (unsigned long long)nreg);
    }
    std::vector<uint32_t> ucnt(nreg);
    SKX_HIP(hipMemcpyAsync(ucnt.data(), d->ucnt.p, nreg * 4, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    SKX_HIP(hipGetLastError());
    if (overflow) { set_error("internal: a %s region did not fit the counting sort (%d)", what, overflow); return SKX_EUNSUP; }
    d->sample_size.assign(d->n, 0);
    for (int s = 0; s < d->n; s++) for (uint64_t b = 0; b < (1ull << d->logB); b++) d->sample_size[s] += ucnt[((uint64_t)s << d->logB) + b];
    return SKX_OK;
}

// The passing windows' packed words of every sample (reads_sample_words) -> (sample, bucket) regions like an assembly's -> the same dedupe
// kernel: sorted, folded, sub-indexed regions, so union / assemble treat reads and assemblies alike.  SKF_NOT_TAKEN: regions the LDS
// sort cannot hold (the sort-based form takes the batch).
int skx::reads_words_to_dictset(skx_ctx *ctx, std::vector<DevBuf<uint64_t>> &wl, std::vector<DevBuf<uint64_t>> &wh2, const std::vector<uint64_t> &cnt,
                                int k, int rc, skx_dictset **out)
{
    const int n = (int)wl.size();
    hipStream_t st = ctx->stream;
    const bool wide_r = k > 31;
    const int wpk_r = wide_r ? 2 : 1, kbits = 2 * (k - 1);
    uint64_t maxn = 0;
    for (auto c : cnt) maxn = std::max(maxn, c);
    const uint64_t per = wide_r ? 2500 : 3500;
    int logB = std::min({ilog2_ceil((maxn + per - 1) / per), kbits, MAX_LOGB});
    if (logB < 0) logB = 0;
    std::unique_ptr<skx_dictset> d = new_dictset(ctx, n, k, rc, logB);
    const uint64_t nreg = (uint64_t)n << logB;
    SKX_TRY(d->raw.alloc(nreg)); SKX_TRY(d->ucnt.alloc(nreg)); SKX_TRY(d->off.alloc(nreg + 1)); SKX_TRY(d->sidx.alloc(nreg * skx::SUBIDX));
    d->sb = std::min(4, kbits - logB);
    SKX_TRY(d->raw.zero(st));
    for (int s = 0; s < n; s++) launch_words_regions(true, wl[s].p, wide_r ? wh2[s].p : nullptr, cnt[s], kbits, logB, (uint64_t)s << logB, d->raw.p, nullptr, nullptr, nullptr, st);
    DevBuf<uint32_t> d_max, cursor; SKX_TRY(d_max.alloc(1)); SKX_TRY(cursor.alloc(nreg)); SKX_TRY(cursor.zero(st));
    launch_scan_u32(d->raw.p, d->off.p, nreg, d_max.p, st);
    uint64_t total = 0; uint32_t max_raw = 0;
    SKX_HIP(hipMemcpyAsync(&total, d->off.p + nreg, 8, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipMemcpyAsync(&max_raw, d_max.p, 4, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    if (max_raw > lds_sort_max(wide_r)) { if (getenv("SKX_DEBUG")) fprintf(stderr, "[skx] reads: region of %u words, batch left to the sort-based form\n", max_raw); return SKF_NOT_TAKEN; }   // e.g. min_count 2 on deep reads: every repeat occurrence is a word
    SKX_TRY(d->words.alloc(std::max<uint64_t>(total, 1) * wpk_r));
    for (int s = 0; s < n; s++) {
        launch_words_regions(false, wl[s].p, wide_r ? wh2[s].p : nullptr, cnt[s], kbits, logB, (uint64_t)s << logB, nullptr, d->off.p, cursor.p, d->words.p, st);
        wl[s].release(); wh2[s].release();
    }
    SKX_TRY(dedupe_regions(ctx, d.get(), max_raw, 0, "read-set"));
    *out = d.release();
    return SKX_OK;
}

// Per-sample sorted, folded lists -> the flat sorted form of a dictset (logB = 0: one region a sample), which every consumer of sorted
// dictionaries takes: what the sort-based read-set path and the flat sort of an assembly both end in.
static int set_flat_sorted(skx_ctx *ctx, skx_dictset *d, const std::vector<DevBuf<uint64_t>> &lists, const std::vector<uint64_t> &sizes)
{
    hipStream_t st = ctx->stream;
    const int n = d->n, wpk = d->wide() ? 2 : 1;
    std::vector<uint64_t> offs(n + 1, 0);
    std::vector<uint32_t> uc(n);
    for (int s = 0; s < n; s++) {
        if (sizes[s] > 0xFFFFFFFFull) { set_error("sample too large"); return SKX_EUNSUP; }
        uc[s] = (uint32_t)sizes[s]; offs[s + 1] = offs[s] + sizes[s];
    }
    DevBuf<uint64_t> words, off; DevBuf<uint32_t> raw, ucnt;
    SKX_TRY(words.alloc(offs[n] * wpk)); SKX_TRY(off.alloc(n + 1)); SKX_TRY(raw.alloc(n)); SKX_TRY(ucnt.alloc(n));
    for (int s = 0; s < n; s++)
        if (sizes[s]) SKX_HIP(hipMemcpyAsync(words.p + offs[s] * wpk, lists[s].p, sizes[s] * 8 * wpk, hipMemcpyDeviceToDevice, st));
    SKX_HIP(hipMemcpyAsync(off.p, offs.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    SKX_HIP(hipMemcpyAsync(ucnt.p, uc.data(), n * 4, hipMemcpyHostToDevice, st));
    SKX_HIP(hipMemcpyAsync(raw.p, uc.data(), n * 4, hipMemcpyHostToDevice, st));
    SKX_HIP(hipStreamSynchronize(st));
    SKX_HIP(hipGetLastError());
    d->words = std::move(words); d->off = std::move(off); d->raw = std::move(raw); d->ucnt = std::move(ucnt);
    d->sidx.release(); d->sb = 0; d->logB = 0;
    d->sample_size = sizes;
    d->sorted = true; d->sketch.release();                      // (the sketch sizes the append pass, which reads unsorted regions only)
    return SKX_OK;
}

// Samples whose regions are beyond the per-region LDS sort (assemblies above ~5 Mbp keep 2^10 regions that grow with them, so that the
// extraction kernel's (tile, bucket) chunks stay whole lines: round 6; or a repeat that fills one region): every sample's words as ONE
// sorted, folded list.  Radix sort + fold (skx_prims, skx_reads.hip).
static int dictset_sort_flat(skx_ctx *ctx, skx_dictset *d)
{
    hipStream_t st = ctx->stream;
    const bool wide = d->wide();
    const int wpk = wide ? 2 : 1, n = d->n;
    const uint64_t B = 1ull << d->logB, nreg = (uint64_t)n << d->logB;
    std::vector<uint32_t> raw(nreg);
    SKX_HIP(hipMemcpyAsync(raw.data(), d->raw.p, nreg * 4, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    std::vector<DevBuf<uint64_t>> lists(n);
    std::vector<uint64_t> sizes(n, 0), dst(B);
    DevBuf<uint64_t> d_dst, lo, hi;
    SKX_TRY(d_dst.alloc(B));
    for (int s = 0; s < n; s++) {
        uint64_t m = 0;
        for (uint64_t b = 0; b < B; b++) { dst[b] = m; m += raw[(uint64_t)s * B + b]; }
        if (m == 0) continue;
        if (lo.n < m) { SKX_TRY(lo.alloc(m + m / 8)); if (wide) SKX_TRY(hi.alloc(m + m / 8)); }
        SKX_HIP(hipMemcpyAsync(d_dst.p, dst.data(), B * 8, hipMemcpyHostToDevice, st));
        launch_gather_regions(d->words.p, d->off.p, d->raw.p, d_dst.p, (uint64_t)s * B, B, wpk, lo.p, wide ? hi.p : nullptr, st);
        SKX_TRY(sort_fold_words(ctx, lo.p, wide ? hi.p : nullptr, m, lists[s], &sizes[s]));      // (returns with the stream idle: dst may be refilled)
    }
    lo.release(); hi.release();
    return set_flat_sorted(ctx, d, lists, sizes);
}

// windows per region are Poisson around len / B: all but ~5 in 10 000 regions stay below mean + 3.3 sigma
static uint32_t typical_region(uint64_t maxlen, int logB)
{
    const double mean_r = (double)(maxlen >> logB) + 1.0;
    return (uint32_t)(mean_r + 3.3 * std::sqrt(mean_r) + 1.0);
}
// raw regions -> the sorted form, whichever the regions' size asks for (`layout`: fixed-capacity or exact, for the error message)
static int sort_regions(skx_dictset *d, const char *layout, bool *flat = nullptr)
{
    skx_ctx *ctx = d->ctx;
    if (flat) *flat = d->region_cap > lds_sort_max(d->wide());
    if (d->region_cap > lds_sort_max(d->wide())) return dictset_sort_flat(ctx, d);
    SKX_TRY(dedupe_regions(ctx, d, d->region_cap, typical_region(d->maxlen, d->logB), layout));
    d->sorted = true; d->sketch.release();                      // sorted dictionaries: no sketch
    return SKX_OK;
}

int skx::dictset_sort(skx_dictset *d)
{
    if (d->sorted) return SKX_OK;
    SKX_HIP(hipSetDevice(d->ctx->device));
    return sort_regions(d, "fixed-capacity");                   // (only dictsets kept as the single-pass extraction left them are unsorted)
}

// The region layout of an assembly batch from its longest sample: how many buckets a sample's words are split into, and the fixed capacity of a region.
uint32_t skx::region_capacity(uint64_t maxlen, int logB)
{
    // hashed buckets are Poisson around len/B: 20 % + 256 words of head-room covers ordinary repeat content
    const uint64_t mean = (maxlen >> logB) + 1;
    return (uint32_t)std::min<uint64_t>(((mean + mean / 5 + 256) + 63) / 64 * 64, 0x7FFFFFFFull);
}
RegionLayout skx::region_layout(uint64_t maxlen, int k)
{
    const bool wide = k > 31;
    // windows per bucket (upper bound): the 64-bit dedupe sorts up to 6 144 words per region in LDS and the regions get 20 % + 256
    // words of head-room, so 4 900 is the largest mean that fits -- and the largest buckets give the scatter its widest chunks
    // (128-bit keys: 3 200, so that a region's fixed capacity -- 20 % + 256 above the mean -- stays within the 4 096 words of the wide counting sort
    // and the samples can stay as extracted for the append pass whatever their length)
    const uint64_t per_region = wide ? 3200 : 4900;
    // Longer samples (round 6): the bucket count stops growing at the 5 Mbp shape (2^10 regions; 2^11 for 128-bit keys) and the regions grow
    // instead -- the extraction kernel's (tile, bucket) chunks stay whole lines (with regions capped at 4 900 words a 20 Mbp sample took 13 ps per
    // base against 2.5, a 40 Mbp one 43, and beyond that the assembly kernels were left altogether), the append pass reads regions of any
    // size unsorted (2^(logQ - logB) row blocks per region: up to 32 readers a region), and who asks for sorted dictionaries of such samples
    // gets the flat sorted form (dictset_sort_flat).  Beyond 32 row blocks per region the buckets grow again (to 2^13: ~1.3 Gbp).
    const int need = std::max(0, ilog2_ceil((maxlen + per_region - 1) / per_region));
    const int base_logB = wide ? 11 : 10;
    if (need - 5 > MAX_LOGB) return {-1, 0};
    // SKX_KNOBS=region_logb=N (tests): a small sample in the layout of a long one -- the extraction kernels' 2^11 .. 2^13-region forms
    // are otherwise reached from 160 Mbp up
    if (const long forced = knob("region_logb", -1); forced >= 0) {
        const int logB = (int)std::min<long>(forced, std::min(2 * (k - 1), MAX_LOGB));
        return {logB, region_capacity(maxlen, logB)};
    }
    const int logB = std::max(0, std::min({need > base_logB ? std::max(base_logB, need - 5) : need, 2 * (k - 1), MAX_LOGB}));
    return {logB, region_capacity(maxlen, logB)};
}

// ------------------------------------------------------------------------------------------ a batch of record streams -> dictset
namespace {
struct Batch {                       // the record streams of skx_dictset_build, on the device
    const std::vector<const uint8_t *> &seqs, &quals;           // quals[s] == nullptr: a FASTA sample
    const std::vector<uint64_t> &lens;
    int k, rc; const skx_qual *q;
    int n() const { return (int)seqs.size(); }
    // a sample's gates: the batch's (ska's defaults without), none for a FASTA sample in a mixed batch
    skx_qual qual_of(int s) const
    {
        skx_qual qs = q ? *q : skx_qual{5, 20, SKX_QUAL_STRICT};
        if (!quals[s]) { qs.min_count = 0; qs.qual_filter = SKX_QUAL_NOFILTER; }
        return qs;
    }
};
}  // namespace

// reads: per-sample quality gates + KmerFilter (skx_reads.hip); the dictset is then one sorted region per sample.  The same
// sort-based path takes assemblies too large for the bucketed one (more than 2^MAX_LOGB regions' worth of windows: a 40 Mbp
// sample and up, to 4 Gbp), with the filters switched off.
static int build_sorted(skx_ctx *ctx, const Batch &b, skx_dictset **out)
{
    const int n = b.n();
    std::vector<DevBuf<uint64_t>> lists(n);
    std::vector<uint64_t> sizes(n, 0);
    for (int s = 0; s < n; s++) SKX_TRY(reads_sample_dict(ctx, b.seqs[s], b.quals[s], b.lens[s], b.k, b.rc, b.qual_of(s), lists[s], &sizes[s]));
    std::unique_ptr<skx_dictset> d = new_dictset(ctx, n, b.k, b.rc, 0);
    SKX_TRY(set_flat_sorted(ctx, d.get(), lists, sizes));
    *out = d.release();
    return SKX_OK;
}
// The same samples through the engine's own kernels (skx_reads2.hip): the windows that pass the gates and the count filter
// come back as packed words, which go into (sample, bucket) regions like an assembly's and through the same dedupe kernel
// -- sorted, folded, sub-indexed regions, so union / assemble treat reads and assemblies alike.  A sample the partition
// kernels do not take (or regions the LDS sort cannot hold) sends the batch to the sort-based form above.
static int build_bucketed_reads(skx_ctx *ctx, const Batch &b, skx_dictset **out)
{
    const int n = b.n();
    std::vector<DevBuf<uint64_t>> wl(n), wh2(n);
    std::vector<uint64_t> cnt(n, 0);
    for (int s = 0; s < n; s++) {
        const int r = reads_sample_words(ctx, b.seqs[s], b.quals[s], b.lens[s], b.k, b.rc, b.qual_of(s), wl[s], wh2[s], &cnt[s]);
        if (r != SKX_OK) return r;                                                       // SKF_NOT_TAKEN included
    }
    return reads_words_to_dictset(ctx, wl, wh2, cnt, b.k, b.rc, out);
}
static int build_reads(skx_ctx *ctx, const Batch &b, skx_dictset **out)
{
    if (!knob("reads_sort")) {
        const int r = build_bucketed_reads(ctx, b, out);
        if (r != SKF_NOT_TAKEN) return r;
    }
    return build_sorted(ctx, b, out);
}

// Single pass: every region has `region_cap` words of room; *over: a region got more (repeat content), its surplus was dropped
static int extract_fixed(skx_ctx *ctx, skx_dictset *d, ExtractArgs a, uint32_t region_cap, int *over)
{
    hipStream_t st = ctx->stream;
    const bool wide = d->wide();
    const uint64_t nreg = (uint64_t)d->n << d->logB;
    SKX_TRY(d->raw.zero(st)); SKX_HIP(hipMemsetAsync(a.overflow, 0, sizeof(int), st));
    launch_fill_offsets(d->off.p, nreg, region_cap, st);
    SKX_TRY(d->words.alloc(nreg * (uint64_t)region_cap * (wide ? 2 : 1) + 2048));      // (+ slack: the append pass reads whole chunks of up to 12 KB)
    // the split sketch, zeroed with the regions' fills: what append_pass sizes its row blocks from instead of a count-only launch
    if (sketch_ok(wide ? d->wh.bits : d->hp.bits, d->logB)) { SKX_TRY(d->sketch.alloc(sketch_words(d->logB))); SKX_TRY(d->sketch.zero(st)); a.sketch = d->sketch.p; }
    { StageTimer t(ctx, &ctx->tm.scatter); a.hist = d->raw.p; a.off = d->off.p; a.words = d->words.p; a.capacity = region_cap;
      if (wide) launch_scatter_wide(a, st); else launch_scatter(a, st); }
    SKX_HIP(hipMemcpyAsync(over, a.overflow, sizeof(int), hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    return SKX_OK;
}
// Two passes over the same dictset: count, scan to exact offsets, scatter; *max_raw: the largest region.  (No sketch: the result is sorted.)
static int extract_exact(skx_ctx *ctx, skx_dictset *d, ExtractArgs a, uint32_t *max_raw)
{
    hipStream_t st = ctx->stream;
    const bool wide = d->wide();
    const uint64_t nreg = (uint64_t)d->n << d->logB;
    d->words.release(); d->sketch.release();
    DevBuf<uint32_t> d_cursor, d_max;
    SKX_TRY(d_cursor.alloc(nreg)); SKX_TRY(d_max.alloc(1)); SKX_TRY(d_cursor.zero(st)); SKX_TRY(d->raw.zero(st));
    { StageTimer t(ctx, &ctx->tm.hist); a.hist = d->raw.p; if (wide) launch_hist_wide(a, st); else launch_hist(a, st); }
    launch_scan_u32(d->raw.p, d->off.p, nreg, d_max.p, st);
    uint64_t total = 0;
    SKX_HIP(hipMemcpyAsync(&total, d->off.p + nreg, 8, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipMemcpyAsync(max_raw, d_max.p, 4, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    SKX_TRY(d->words.alloc(total * (wide ? 2 : 1)));
    { StageTimer t(ctx, &ctx->tm.scatter); a.hist = d_cursor.p; a.off = d->off.p; a.words = d->words.p; a.capacity = 0xFFFFFFFFu;
      if (wide) launch_scatter_wide(a, st); else launch_scatter(a, st); }
    return SKX_OK;
}
// windows per sample of a dictset kept as extracted (0 = the sample has no valid sequence)
static int fetch_raw_totals(skx_ctx *ctx, skx_dictset *d)
{
    hipStream_t st = ctx->stream;
    DevBuf<unsigned long long> d_tot; SKX_TRY(d_tot.alloc(d->n));
    launch_region_totals(d->raw.p, d->n, d->logB, d_tot.p, st);
    d->raw_total.resize(d->n);
    SKX_HIP(hipMemcpyAsync(d->raw_total.data(), d_tot.p, (size_t)d->n * 8, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    SKX_HIP(hipGetLastError());
    return SKX_OK;
}

// What a build of n assemblies, the longest of maxlen bytes, is launched with: the regions, the extraction kernels' tiles and their
// dealing to XCDs, and what the per-region sort of regions of lds_cap words (the fixed capacity, or the largest region of the exact
// layout) would be launched with.  The 64-bit kernels' HI forms are 0 for 128-bit keys, which have one form.
namespace {
struct BuildPlan {
    RegionLayout lay; int tile_bases = 0, tiles_max = 0, parts = 0, tiles_part = 0; bool extract_hi = false;
    struct Sort { uint32_t cap = 0, shape = 0, typical = 0, shape_typ = 0; bool hi = false, hi_typ = false, flat = false; } sort;
};
}  // namespace
static BuildPlan::Sort sort_plan(uint64_t maxlen, int k, int logB, uint32_t lds_cap)
{
    const bool wide = k > 31;
    BuildPlan::Sort s;
    s.flat = lds_cap > lds_sort_max(wide);
    s.cap = dedupe_launch_cap(lds_cap, wide);
    s.typical = wide ? 0 : typical_region(maxlen, logB);
    if (wide) { s.shape = s.shape_typ = s.cap; return s; }
    const int rem_bits = make_hash_params(k).bits - logB, sb = std::min(4, rem_bits);      // (d->hp.bits - d->logB and d->sb of the launch)
    s.shape = dedupe_shape_words(s.cap); s.shape_typ = std::min(s.shape, dedupe_shape_words(s.typical));
    s.hi = dedupe_hi(s.cap, rem_bits, sb); s.hi_typ = dedupe_hi(s.shape_typ < s.shape ? s.shape_typ : s.cap, rem_bits, sb);
    return s;
}
static BuildPlan build_plan(uint64_t maxlen, int n, int k)
{
    BuildPlan p;
    p.lay = region_layout(maxlen, k);
    if (p.lay.logB < 0) return p;
    const bool wide = k > 31;
    p.tile_bases = wide ? extract_tile_bases_wide() : extract_tile_bases(p.lay.logB);
    p.tiles_max = (int)((maxlen + p.tile_bases - 1) / p.tile_bases);
    ExtractArgs a{}; a.n_samples = n; a.tiles_max = p.tiles_max;
    extract_parts(a);
    p.parts = a.parts; p.tiles_part = a.tiles_part;
    p.extract_hi = !wide && extract_hi(make_hash_params(k).bits, p.lay.logB);      // (a.hp.bits of the launch: new_dictset)
    p.sort = sort_plan(maxlen, k, p.lay.logB, p.lay.cap);
    return p;
}
// a test hook of the library (not in include/skx.h): the plan for a batch of n_samples assemblies, the longest of maxlen bytes -- out[0] logB
// (-1: left to the sort-based form, nothing else is set), [1] region capacity, [2] tile bases, [3] tiles_max, [4] parts, [5] tiles_part,
// [6] extraction takes its HI form, [7] capacity of the dedupe launch, [8] its shape (words), [9] the typical region, [10] the shape the
// typical region is sorted in, [11] / [12] the dedupe kernel's HI form in the capacity's / the typical shape's launch, [13] the fixed
// capacity is beyond the per-region sort (sorted dictionaries come from the flat sort)
extern "C" int skx_debug_build_plan(uint64_t maxlen, int n_samples, int k, int64_t *out)
{
    if (!out || n_samples <= 0 || check_k(k) != SKX_OK) { set_error("bad arguments"); return SKX_EINVAL; }
    const BuildPlan p = build_plan(maxlen, n_samples, k);
    for (int i = 0; i < 14; i++) out[i] = 0;
    out[0] = p.lay.logB;
    if (p.lay.logB < 0) return SKX_OK;
    out[1] = p.lay.cap; out[2] = p.tile_bases; out[3] = p.tiles_max; out[4] = p.parts; out[5] = p.tiles_part; out[6] = p.extract_hi;
    out[7] = p.sort.cap; out[8] = p.sort.shape; out[9] = p.sort.typical; out[10] = p.sort.shape_typ; out[11] = p.sort.hi; out[12] = p.sort.hi_typ;
    out[13] = p.sort.flat;
    return SKX_OK;
}

static int dictset_build_device(skx_ctx *ctx, const Batch &b, skx_dictset **out)
{
    const int n = b.n(), k = b.k;
    hipStream_t st = ctx->stream;
    for (auto p : b.quals) if (p) return build_reads(ctx, b, out);
    uint64_t maxlen = 0;
    for (auto l : b.lens) maxlen = std::max(maxlen, l);
    const BuildPlan plan = build_plan(maxlen, n, k);
    const RegionLayout lay = plan.lay;
    if (lay.logB < 0) return build_reads(ctx, b, out);

    std::unique_ptr<skx_dictset> d = new_dictset(ctx, n, k, b.rc, lay.logB);
    const bool wide = d->wide();
    const uint64_t nreg = (uint64_t)n << lay.logB;
    SKX_TRY(d->raw.alloc(nreg)); SKX_TRY(d->ucnt.alloc(nreg)); SKX_TRY(d->off.alloc(nreg + 1));
    SKX_TRY(d->sidx.alloc(nreg * skx::SUBIDX)); d->sb = std::min(4, (wide ? 2 * (k - 1) : d->hp.bits) - lay.logB);
    DevBuf<const uint8_t *> d_seqs; DevBuf<uint64_t> d_lens; DevBuf<int> d_flag;
    SKX_TRY(d_seqs.alloc(n)); SKX_TRY(d_lens.alloc(n)); SKX_TRY(d_flag.alloc(1));
    SKX_HIP(hipMemcpyAsync(d_seqs.p, b.seqs.data(), n * sizeof(void *), hipMemcpyHostToDevice, st));
    SKX_HIP(hipMemcpyAsync(d_lens.p, b.lens.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    ExtractArgs a{};                                            // (no quality streams here: quals, min_qual and qual_filter stay zero)
    a.seqs = d_seqs.p; a.lens = d_lens.p; a.n_samples = n; a.tiles_max = plan.tiles_max;
    a.k = k; a.rc = b.rc; a.logB = lay.logB; a.hp = d->hp; a.wh = d->wh; a.overflow = d_flag.p;

    // single pass with fixed-capacity regions first; the exact two-pass layout if a region overflows
    int over = 0;
    uint32_t lds_cap = lay.cap;
    SKX_TRY(extract_fixed(ctx, d.get(), a, lay.cap, &over));
    if (over) SKX_TRY(extract_exact(ctx, d.get(), a, &lds_cap));
    d->maxlen = maxlen; d->region_cap = lds_cap; d->sorted = false;
    // Assemblies whose regions kept their fixed capacity stay as the extraction kernel left them (both key widths): MergeSkaDict::append
    // (skx_append.hip) reads them unsorted, and the sorted, folded form (a sample's SkaDict) is made when something asks for it
    // (skx::dictset_sort: skx_dictset_size / _export, the key-set union of a sharded job) -- at once for SKX_KNOBS=sorted_dicts and for the
    // exact layout.  Regions beyond the per-region sort stay as extracted whatever the knob says -- that is what keeps the extraction's
    // chunks whole -- and get their sorted form from the flat sort.
    const bool sort_now = over || knob("sorted_dicts");
    if (!over && (!sort_now || lds_cap > lds_sort_max(wide))) SKX_TRY(fetch_raw_totals(ctx, d.get()));
    uint32_t largest = lds_cap;                                 // (the exact layout's scan left it; the fixed layout's is fetched for the debug line alone)
    if (getenv("SKX_DEBUG") && !over) {
        std::vector<uint32_t> raw(nreg);
        SKX_HIP(hipMemcpyAsync(raw.data(), d->raw.p, nreg * 4, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipStreamSynchronize(st));
        largest = *std::max_element(raw.begin(), raw.end());
    }
    bool went_flat = false;                                     // (what sort_regions did, for the debug line)
    if (sort_now) SKX_TRY(sort_regions(d.get(), over ? "exact-layout" : "fixed-capacity", &went_flat));
    if (getenv("SKX_DEBUG")) {
        const BuildPlan::Sort sp = sort_plan(maxlen, k, lay.logB, lds_cap);
        fprintf(stderr, "[skx] build: n=%d k=%d longest=%llu logB=%d cap=%u tile=%d tiles_max=%d parts=%d tiles_part=%d extract_hi=%d layout=%s largest=%u end=%s",
                n, k, (unsigned long long)maxlen, lay.logB, lay.cap, plan.tile_bases, plan.tiles_max, plan.parts, plan.tiles_part, (int)plan.extract_hi,
                over ? "exact" : "fixed", largest, !sort_now ? "extracted" : went_flat ? "flat" : "per-region");
        if (sort_now && !went_flat) fprintf(stderr, " sort_cap=%u shape=%u typical=%u shape_typ=%u dedupe_hi=%d/%d", sp.cap, sp.shape, sp.typical, sp.shape_typ, (int)sp.hi, (int)sp.hi_typ);
        fprintf(stderr, "\n");
    }
    *out = d.release();
    return SKX_OK;
}

extern "C" int skx_dictset_build(skx_ctx *ctx, const skx_stream *samples, int n, int on_device, int k, int rc, const skx_qual *q, skx_dictset **out)
{
    return skx_guarded([&]() -> int {
    if (!ctx || !samples || n <= 0 || !out) { set_error("bad arguments"); return SKX_EINVAL; }
    SKX_TRY(check_k(k));
    SKX_HIP(hipSetDevice(ctx->device));
    std::vector<const uint8_t *> seqs(n), quals(n, nullptr);
    std::vector<uint64_t> lens(n);
    std::vector<DevBuf<uint8_t>> own;
    if (on_device) {
        for (int i = 0; i < n; i++) {
            if (((uintptr_t)samples[i].seq & 15) || ((uintptr_t)samples[i].qual & 15)) { set_error("device record streams must be 16-byte aligned"); return SKX_EINVAL; }
            seqs[i] = samples[i].seq; quals[i] = samples[i].qual; lens[i] = samples[i].len;
        }
    } else {
        own.resize(2 * (size_t)n);
        for (int i = 0; i < n; i++) {
            lens[i] = samples[i].len;
            SKX_TRY(own[2 * i].alloc(samples[i].len + 16));
            SKX_HIP(hipMemcpyAsync(own[2 * i].p, samples[i].seq, samples[i].len, hipMemcpyHostToDevice, ctx->stream));
            seqs[i] = own[2 * i].p;
            if (samples[i].qual) {
                SKX_TRY(own[2 * i + 1].alloc(samples[i].len + 16));
                SKX_HIP(hipMemcpyAsync(own[2 * i + 1].p, samples[i].qual, samples[i].len, hipMemcpyHostToDevice, ctx->stream));
                quals[i] = own[2 * i + 1].p;
            }
        }
    }
    skx_dictset *d = nullptr;
    SKX_TRY(dictset_build_device(ctx, Batch{seqs, quals, lens, k, rc, q}, &d));
    for (int s = 0; s < n; s++)
        if ((d->sorted ? d->sample_size[s] : d->raw_total[s]) == 0) { set_error("sample %d has no valid sequence", s); delete d; return SKX_EEMPTY; }
    *out = d;
    return SKX_OK;
    });
}

extern "C" int skx_dictset_size(skx_dictset *d, int sample, uint64_t *n)
{
    return skx_guarded([&]() -> int {
    if (!d || sample < 0 || sample >= d->n) { set_error("bad sample index"); return SKX_EINVAL; }
    SKX_TRY(dictset_sort(d));
    *n = d->sample_size[sample];
    return SKX_OK;
    });
}

extern "C" int skx_dictset_export(skx_dictset *d, int sample, skx_key *keys, uint8_t *bases, uint64_t cap)
{
    return skx_guarded([&]() -> int {
    if (!d || sample < 0 || sample >= d->n) { set_error("bad sample index"); return SKX_EINVAL; }
    skx_ctx *ctx = d->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    SKX_TRY(dictset_sort(d));
    const uint64_t B = 1ull << d->logB, sz = d->sample_size[sample];
    if (cap < sz) { set_error("buffer too small"); return SKX_EINVAL; }
    std::vector<uint64_t> off(B + 1); std::vector<uint32_t> uc(B);
    SKX_HIP(hipMemcpyAsync(off.data(), d->off.p + ((uint64_t)sample << d->logB), (B + 1) * 8, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipMemcpyAsync(uc.data(), d->ucnt.p + ((uint64_t)sample << d->logB), B * 4, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    std::vector<skx_key> hk(sz); std::vector<uint8_t> hb(sz);
    static const char M2I[17] = "-ACMTWYHGRSVKDBN";
    const int wpk = d->wide() ? 2 : 1;
    {
        std::vector<uint64_t> raw((size_t)sz * wpk);
        uint64_t w = 0;
        for (uint64_t b = 0; b < B; b++) {
            if (uc[b]) SKX_HIP(hipMemcpyAsync(raw.data() + w * wpk, d->words.p + off[b] * wpk, (size_t)uc[b] * 8 * wpk, hipMemcpyDeviceToHost, st));
            w += uc[b];
        }
        SKX_HIP(hipStreamSynchronize(st));
        for (uint64_t i = 0; i < sz; i++) {
            if (d->wide()) {
                const u128 word = ((u128)raw[2 * i + 1] << 64) | raw[2 * i];
                const u128 key = hunmix_w(word >> 4, d->wh);
                hk[i].lo = (uint64_t)key; hk[i].hi = (uint64_t)(key >> 64); hb[i] = (uint8_t)M2I[(unsigned)word & 15u];
            } else {
                hk[i].lo = hunmix(raw[i] >> 4, d->hp); hk[i].hi = 0; hb[i] = (uint8_t)M2I[raw[i] & 15u];
            }
        }
    }
    std::vector<uint64_t> idx(sz); std::iota(idx.begin(), idx.end(), 0);
    std::sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b2) { return hk[a].hi != hk[b2].hi ? hk[a].hi < hk[b2].hi : hk[a].lo < hk[b2].lo; });
    for (uint64_t i = 0; i < sz; i++) { if (keys) keys[i] = hk[idx[i]]; if (bases) bases[i] = hb[idx[i]]; }
    return SKX_OK;
    });
}
