// skx_merge.cpp -- the merge stage's host side: dictionaries -> rows (skx_keyset_*), rows -> array (skx_array_assemble / _lazy), the lazily held
// array (statistics, all rows, a window, kept rows), MergeSkaDict::append from the raw regions (append_pass, the array over its pieces) and
// skx_merge.  In the order of use: no function is declared ahead of its definition.
#include "skx_internal.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>

using namespace skx;

// ------------------------------------------------------------------------------------------ keyset
extern "C" void skx_keyset_free(skx_keyset *ks) { delete ks; }
extern "C" int skx_keyset_size(const skx_keyset *ks, uint64_t *n) { *n = ks->total; return SKX_OK; }

static int keyset_finish(skx_keyset *ks)      // scan ncnt -> roff, total, max_rows
{
    hipStream_t st = ks->ctx->stream;
    const uint64_t nsub = 1ull << ks->logN;
    SKX_TRY(ks->roff.alloc(nsub + 1));
    DevBuf<uint32_t> d_max; SKX_TRY(d_max.alloc(1));
    launch_scan_u32(ks->ncnt.p, ks->roff.p, nsub, d_max.p, st);
    SKX_HIP(hipMemcpyAsync(&ks->total, ks->roff.p + nsub, 8, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipMemcpyAsync(&ks->max_rows, d_max.p, 4, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    if (getenv("SKX_DEBUG")) fprintf(stderr, "[skx] keyset: logN=%d sub-buckets=%llu rows=%llu mean=%.1f max=%u\n", ks->logN, (unsigned long long)nsub,
                                 (unsigned long long)ks->total, (double)ks->total / (double)nsub, ks->max_rows);
    return SKX_OK;
}

// the slabs of src (its stage, at its stride and key width) as one compact list in row order; ncnt / roff: the rows per slab and their scan
// (src's own, or the copy an array over pieces keeps)
static void gather_row_keys(const skx_keyset *src, const uint32_t *ncnt, const uint64_t *roff, uint64_t *out, hipStream_t st)
{
    if (src->wide) launch_gather_keys_wide((const u128 *)src->stage.p, src->stride, ncnt, roff, 1 << src->logN, (u128 *)out, st);
    else launch_gather_keys(src->stage.p, src->stride, ncnt, roff, 1 << src->logN, out, 0, src->hp, st);
}

// union over the samples of one dict view into one keyset
static int keyset_union_views(skx_ctx *ctx, const DictView &view, int k, int rc, HashParams hp, uint64_t est_hint, skx_keyset **out,
                              const skx_dictset *side_for = nullptr)
{
    const bool wide = k > 31;
    const WideHash wh = make_wide_hash(k);
    const int kbits = 2 * (k - 1);
    hipStream_t st = ctx->stream;
    DevBuf<int> d_flag; SKX_TRY(d_flag.alloc(1));
    const uint32_t table = wide ? 4096 : 8192, stride = wide ? 2048 : 4096, target = wide ? 1200 : 2500;
    int logN = std::max(std::max(0, view.logB), std::min(kbits, ilog2_ceil((est_hint + target - 1) / target)));
    DevBuf<uint16_t> side_buf;                     // kept across retries at a finer split
    for (;; logN++) {
        std::unique_ptr<skx_keyset> ks(new skx_keyset());
        ks->ctx = ctx; ks->k = k; ks->rc = rc; ks->logN = logN; ks->hp = hp; ks->wh = wh; ks->wide = wide; ks->stride = stride;
        const uint64_t nsub = 1ull << logN;
        SKX_TRY(ks->stage.alloc(nsub * stride * ks->wpk())); SKX_TRY(ks->ncnt.alloc(nsub));
        SKX_TRY(d_flag.zero(st));
        // side_for: the assemble over these dictionaries follows (skx_merge): the pass also notes where every word's key went, 2 bytes
        // per word, and the matrix is then filled from the notes instead of a second read of the dictionaries
        const bool with_side = side_for && (wide || union_side_ok(view, logN, stride));
        if (wide && with_side) {
            if (!side_buf.p) SKX_TRY(side_buf.alloc(side_for->words.n / 2 + 64));          // one note per 16-byte word
            SKX_TRY(ks->perm.alloc(nsub * stride));
            launch_union_side_wide(view, logN, (u128 *)ks->stage.p, stride, ks->ncnt.p, table, d_flag.p, side_buf.p, ks->perm.p, st);
            ks->side_of = side_for;
        } else if (wide) launch_union_wide(view, logN, (u128 *)ks->stage.p, stride, ks->ncnt.p, table, d_flag.p, st);
        else if (with_side) {
            if (!side_buf.p) SKX_TRY(side_buf.alloc(side_for->words.n));
            SKX_TRY(ks->perm.alloc(nsub * stride));
            launch_union_side(view, logN, ks->stage.p, stride, ks->ncnt.p, 7168u, d_flag.p, side_buf.p, ks->perm.p, st);
            ks->side_of = side_for;
        } else launch_union(view, logN, ks->stage.p, stride, ks->ncnt.p, table, d_flag.p, st);
        int overflow = 0;
        SKX_HIP(hipMemcpyAsync(&overflow, d_flag.p, 4, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipStreamSynchronize(st));
        SKX_HIP(hipGetLastError());
        if (overflow) {
            if (logN >= kbits) { set_error("key union overflow"); return SKX_EUNSUP; }
            continue;
        }
        SKX_TRY(keyset_finish(ks.get()));
        if (ks->side_of) ks->side = std::move(side_buf);
        *out = ks.release();
        return SKX_OK;
    }
}

// sorted key tables lying in one device buffer as the "samples" of a synthetic one-bucket dict: table i = h_cnt[i] keys at words + h_off[i] * wpk
// (h_off in keys, n + 1 of them; both host arrays outlive the union that reads the view)
struct TablesView { DevBuf<uint64_t> off; DevBuf<uint32_t> ucnt; DictView v; };
static int tables_view(TablesView &tv, const uint64_t *words, const uint64_t *h_off, const uint32_t *h_cnt, int n, int k, hipStream_t st)
{
    SKX_TRY(tv.off.alloc(n + 1)); SKX_TRY(tv.ucnt.alloc(n));
    SKX_HIP(hipMemcpyAsync(tv.off.p, h_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    SKX_HIP(hipMemcpyAsync(tv.ucnt.p, h_cnt, (size_t)n * 4, hipMemcpyHostToDevice, st));
    tv.v = DictView{words, tv.off.p, tv.ucnt.p, n, 0, 2 * (k - 1)};
    return SKX_OK;
}

// union of several sorted key tables lying in one device buffer (off in keys)
int skx::keyset_union_tables(skx_ctx *ctx, const uint64_t *words, const std::vector<uint64_t> &h_off, const std::vector<uint32_t> &h_cnt, int k, int rc,
                             skx_keyset **out)
{
    hipStream_t st = ctx->stream;
    const int n_sets = (int)h_cnt.size();
    StageTimer t(ctx, &ctx->tm.key_union);
    uint64_t total = 0, maxn = 0;
    for (int i = 0; i < n_sets; i++) { total += h_cnt[i]; maxn = std::max<uint64_t>(maxn, h_cnt[i]); }
    TablesView tv; SKX_TRY(tables_view(tv, words, h_off.data(), h_cnt.data(), n_sets, k, st));
    int r = keyset_union_views(ctx, tv.v, k, rc, make_hash_params(std::min(k, 31)), std::min(total, maxn * 2), out);
    SKX_HIP(hipStreamSynchronize(st));
    return r;
}

int skx::keyset_flatten(skx_keyset *ks)
{
    if (ks->flat.p) return SKX_OK;
    SKX_TRY(ks->flat.alloc(ks->total * ks->wpk()));
    gather_row_keys(ks, ks->ncnt.p, ks->roff.p, ks->flat.p, ks->ctx->stream);
    return SKX_OK;
}

extern "C" int skx_keyset_device(skx_keyset *ks, const void **dptr, uint64_t *n_keys, int *words_per_key)
{
    return skx_guarded([&]() -> int {
    SKX_HIP(hipSetDevice(ks->ctx->device));
    SKX_TRY(keyset_flatten(ks));
    SKX_HIP(hipStreamSynchronize(ks->ctx->stream));
    *dptr = ks->flat.p; *n_keys = ks->total; if (words_per_key) *words_per_key = ks->wpk();
    return SKX_OK;
    });
}

extern "C" int skx_keyset_from_device(skx_ctx *ctx, const void *dptr, uint64_t n_keys, int k, int rc, skx_keyset **out)
{
    return skx_guarded([&]() -> int {
    SKX_TRY(check_k(k));
    SKX_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<skx_keyset> ks(new skx_keyset());    // a flat sorted word list: no slabs (logN < 0)
    ks->ctx = ctx; ks->k = k; ks->rc = rc; ks->hp = make_hash_params(std::min(k, 31)); ks->wh = make_wide_hash(k); ks->wide = k > 31; ks->logN = -1; ks->total = n_keys;
    SKX_TRY(ks->flat.alloc(n_keys * ks->wpk()));
    SKX_HIP(hipMemcpyAsync(ks->flat.p, dptr, n_keys * 8 * ks->wpk(), hipMemcpyDeviceToDevice, ctx->stream));
    SKX_HIP(hipStreamSynchronize(ctx->stream));          // the caller may free or reuse dptr as soon as this returns
    *out = ks.release();
    return SKX_OK;
    });
}

extern "C" int skx_keyset_merge(skx_ctx *ctx, skx_keyset *const *sets, int n_sets, skx_keyset **out)
{
    return skx_guarded([&]() -> int {
    if (!ctx || !sets || n_sets <= 0 || !out) { set_error("bad arguments"); return SKX_EINVAL; }
    SKX_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    uint64_t total = 0;
    for (int i = 0; i < n_sets; i++) {
        if (sets[i]->k != sets[0]->k) { set_error("K-mer lengths do not match: %d %d", sets[i]->k, sets[0]->k); return SKX_EINVAL; }
        if (sets[i]->rc != sets[0]->rc) { set_error("Strand use inconsistent"); return SKX_EINVAL; }
        if (sets[i]->logN >= 0) SKX_TRY(keyset_flatten(sets[i]));
        total += sets[i]->total;
    }
    DevBuf<uint64_t> words;
    const int wpk = sets[0]->wpk();
    SKX_TRY(words.alloc(total * wpk));
    std::vector<uint64_t> h_off(n_sets + 1, 0); std::vector<uint32_t> h_cnt(n_sets);
    for (int i = 0; i < n_sets; i++) {
        if (sets[i]->total > 0xFFFFFFFFull) { set_error("keyset too large"); return SKX_EUNSUP; }
        h_cnt[i] = (uint32_t)sets[i]->total; h_off[i + 1] = h_off[i] + sets[i]->total;
        SKX_HIP(hipMemcpyAsync(words.p + h_off[i] * wpk, sets[i]->flat.p, sets[i]->total * 8 * wpk, hipMemcpyDeviceToDevice, st));
    }
    return keyset_union_tables(ctx, words.p, h_off, h_cnt, sets[0]->k, sets[0]->rc, out);
    });
}

// ------------------------------------------------------------------------------------------ array
extern "C" void skx_array_free(skx_array *a) { delete a; }
extern "C" const char *skx_array_name(const skx_array *a, uint64_t i) { return i < a->names.size() ? a->names[i].c_str() : ""; }
extern "C" const char *skx_array_version(const skx_array *a) { return a->version.c_str(); }
extern "C" int skx_array_info(const skx_array *a, skx_array_info_t *info)
{
    return skx_guarded([&]() -> int {
    info->k = a->k; info->rc = a->rc; info->k_bits = a->k_bits; info->n_kmers = a->n_kmers; info->n_rows = a->n_rows;
    info->n_samples = a->names.size();
    info->total_samples = a->total_samples ? a->total_samples : a->names.size();
    return SKX_OK;
    });
}

// an array over the samples of d with U rows in the order of H: the header, the five per-row buffers (statistics and keys) allocated, no matrix
static int new_array(skx_ctx *ctx, const skx_dictset *d, const char *const *names, uint64_t U, std::unique_ptr<skx_array> &a)
{
    a.reset(new skx_array());
    a->ctx = ctx; a->k = d->k; a->rc = d->rc; a->k_bits = d->key_bits; a->hp = d->hp; a->wh = d->wh; a->version = skx_version();
    for (int i = 0; i < d->n; i++) a->names.emplace_back(names && names[i] ? names[i] : "");
    a->n_rows = a->n_kmers = U; a->pitch = 0; a->engine_order = true;
    SKX_TRY(a->present.alloc(U)); SKX_TRY(a->unambig.alloc(U)); SKX_TRY(a->mask.alloc(U)); SKX_TRY(a->keys.alloc(U * (d->wide() ? 2 : 1))); SKX_TRY(a->vcount.alloc(U));
    return SKX_OK;
}

// dictionaries, rows and an array's statistics as the assemble kernels take them (no matrix: the caller names one)
static AssembleArgs assemble_args(const skx_dictset *d, const skx_keyset *rows, skx_array *a, int *d_flag)
{
    AssembleArgs aa{};
    aa.d = d->view(); aa.logN = rows->logN; aa.stage = rows->stage.p; aa.stride = rows->stride; aa.ncnt = rows->ncnt.p; aa.roff = rows->roff.p;
    aa.matrix = nullptr; aa.pitch = 0; aa.col_present = a->present.p; aa.col_unambig = a->unambig.p; aa.col_mask = a->mask.p;
    aa.max_rows = rows->max_rows; aa.missing = d_flag;
    return aa;
}
// what an assemble kernel left in its `missing` flag; returns with the stream idle
static int check_missing(skx_ctx *ctx, const int *d_flag)
{
    int missing = 0;
    SKX_HIP(hipMemcpyAsync(&missing, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    SKX_HIP(hipStreamSynchronize(ctx->stream));
    SKX_HIP(hipGetLastError());
    if (missing) { set_error("row keyset does not contain every split k-mer of the samples"); return SKX_EINVAL; }
    return SKX_OK;
}

// The statistics pass over an array's pieces.  min_count >= 2: the pass of a frequency filter at that count -- ranks that fewer samples reach
// are not read and their rows leave with zeros (pieces_stats_kernel), so the caller must NOT set stats_ready; it gives `tally` (two words,
// alive until its own synchronise), which receives what skx_ctx_filter_cut reports, and the pass does not wait.  0: every rank, finished on return.
int skx::pieces_stats_pass(skx_array *a, uint64_t min_count, DevBuf<unsigned long long> *tally)
{
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    const skx_pieces *pc = a->pieces; const skx_keyset *blk = a->lazy_rows;
    const int S = (int)a->names.size(), nb = 1 << pc->logQ;
    if (!a->n_rows) return SKX_OK;
    const bool bounded = min_count >= 2 && tally && pieces_stats_bound(pc->cap);
    if (bounded) { SKX_TRY(tally->alloc(2)); SKX_TRY(tally->zero(st)); }
    {
        StageTimer t(ctx, &ctx->tm.assemble);
        KernelTimer kt(ctx, &ctx->tm.pieces_stats);
        launch_pieces_stats(pc->data.p, pc->plen.p, pc->perm.p, pc->nrank.p, blk->ncnt.p, blk->roff.p, pc->cap, S, nb, a->present.p, a->unambig.p, a->mask.p, a->vcount.p, st,
                            bounded ? (uint32_t)std::min<uint64_t>(min_count, 0xFFFFFFFEull) : 0u, bounded ? tally->p : nullptr);
    }
    if (!bounded) SKX_HIP(hipStreamSynchronize(st));
    SKX_HIP(hipGetLastError());
    return SKX_OK;
}

// ---- MergeSkaDict::append from the raw regions (skx_append.hip) ----------------------------------------------------------------------
// rows, row statistics and the cells (as pieces) of all samples in one pass over the words the extraction kernel scattered; no sample is
// sorted.  Both key widths (append_kernel; append_wide_kernel for k > 31).  SKF_NOT_TAKEN: not this kind of dictset (sorted already, regions
// beyond the kernel's load rounds, a row-block split that would read every region too often), or blocks that kept overflowing -- the caller
// sorts the dictionaries and takes the union / assemble kernels.  ctx->merge_path says which way a merge went (skx_ctx_merge_path).
static int append_not_taken(skx_ctx *ctx, const char *why)
{
    ctx->merge_path = std::string("sorted: ") + why;
    if (getenv("SKX_DEBUG")) fprintf(stderr, "[skx] merge: %s\n", ctx->merge_path.c_str());
    return SKF_NOT_TAKEN;
}
static bool append_fits(bool wide, int bits, int logB, int lq, uint32_t region_cap, uint32_t nslots, uint32_t cap) { return wide ? append_wide_ok(bits, logB, lq, nslots, cap) : append_ok(bits, logB, lq, region_cap, nslots, cap); }
static uint32_t append_max_cap(bool wide) { return wide ? APPEND_WIDE_MAX_CAP : APPEND_MAX_CAP; }
static uint32_t append_max_slots(bool wide) { return wide ? APPEND_WIDE_MAX_SLOTS : APPEND_MAX_SLOTS; }
// ranks a block of `mean` expected rows needs: six sigma of its binomial size and of the estimate's own error together (independent: the
// variances add; est_relvar = the relative variance of |U| as the sketch gives it, 0 for a count), + 32
static double ranks_need(double mean, double est_relvar) { return mean + 6.0 * std::sqrt(mean + 1.0 + est_relvar * mean * mean) + 32.0; }
static uint32_t ranks_for(double mean, double est_relvar, uint32_t max_cap)
{
    return (uint32_t)std::min<double>(max_cap, std::ceil(ranks_need(mean, est_relvar) / 128.0) * 128.0);
}
static uint32_t slots_for(uint32_t cap, uint32_t max_slots)           // a power of two (the home slot is a shift), a third more than the ranks at least
{
    uint32_t n = 256u;
    while (n < cap + cap / 3 && n < max_slots) n <<= 1;
    return n;
}

// |U| from a slice of the hash space.  A dictset the single-pass scatter kernel filled brings a sketch of that slice (skx_device.h: a bitmap
// per sketch region, the zero bits of which give the region's distinct keys by linear counting), read out by one small kernel; the rows of a
// block are binomial around |U| / 2^logQ wherever they fall (H's top bits are uniform), so the estimate that sizes the split is the SUM over
// the sketch regions scaled to all regions -- what the count-only launch measures -- and the estimator's own error joins the block's binomial
// spread in the six sigma of ranks_need (two independent errors, so their variances add; added to |U| on top of the block's six sigma
// the same 0.2 % moved 1 000 x 5 Mbp to twice the row blocks and the step from 33.2 to 39.9 ms: its 5 521 rows a block are 0.3 % under the
// 5 537 at which the split doubles.  For the same reason not the LARGEST sketch region: the largest of four lies 0.7 % above their mean,
// which is the binomial spread counted a second time).  An underestimate ends where the launch's ended: the blocks overflow and append_pass
// comes back one step finer.  No sketch, a sketch more than SKETCH_MAX_FILL full or SKX_KNOBS=probe_launch: the first row blocks of a
// 2^logP split, rows counted only (aa: the pass's arguments as far as they describe the regions; its overflow flag is used).
// One sample: its windows, no device work.
struct RowEstimate { double u_est = 0, est_relvar = 0; char sized[160] = "one sample"; };
static int estimate_rows(skx_ctx *ctx, const skx_dictset *d, AppendArgs aa, int min_logQ, uint64_t raw_max, RowEstimate &e)
{
    hipStream_t st = ctx->stream;
    const bool wide = d->wide();
    const int logB = d->logB, bits = aa.bits;
    e.u_est = (double)raw_max;
    if (d->n <= 1) return SKX_OK;
    if (d->sketch.p && !knob("probe_launch")) {
        const int nsk = sketch_regions(logB);
        DevBuf<uint32_t> d_zeros; SKX_TRY(d_zeros.alloc(nsk));
        { KernelTimer kt(ctx, &ctx->tm.append_probe); launch_sketch_count(d->sketch.p, logB, d_zeros.p, st); }
        std::vector<uint32_t> zeros(nsk);
        SKX_HIP(hipMemcpyAsync(zeros.data(), d_zeros.p, (size_t)nsk * 4, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipStreamSynchronize(st));
        SKX_HIP(hipGetLastError());
        const double M = (double)(1u << SKETCH_M);
        double rows = 0, var = 0, fill = 0;
        for (uint32_t z : zeros) {
            fill = std::max(fill, 1.0 - (double)z / M);
            if (z == 0) continue;                                      // (a full bitmap: fill = 1, no estimate)
            const double t = -std::log((double)z / M);
            rows += M * t; var += M * (std::exp(t) - t - 1.0);
        }
        if (fill <= SKETCH_MAX_FILL) {
            const double scale = (double)(1u << sketch_step_log(logB));
            e.u_est = std::max((double)raw_max * 0.5, rows * scale);
            e.est_relvar = rows > 0 ? var / (rows * rows) : 0.0;
            snprintf(e.sized, sizeof e.sized, "the sketch: %.1f rows in %d sketch regions, fill %.3f", rows, nsk, fill);
            return SKX_OK;
        }
        snprintf(e.sized, sizeof e.sized, "the probe launch: the sketch is %.3f full", fill);
    } else snprintf(e.sized, sizeof e.sized, "the probe launch: %s", d->sketch.p ? "SKX_KNOBS=probe_launch" : "no sketch");
    const double target = wide ? 2600.0 : 5400.0;    // mean rows of a probe block (the final split: the coarsest whose blocks fit their ranks)
    DevBuf<unsigned long long> d_probe; SKX_TRY(d_probe.alloc(2));
    aa.probe = d_probe.p;
    int logP = std::min(bits, std::max(min_logQ, ilog2_ceil((uint64_t)((double)raw_max * 3.0 / target) + 1)));
    for (int attempt = 0;; attempt++) {
        const unsigned blocks = (unsigned)std::min<uint64_t>(64, 1ull << logP);
        aa.logQ = logP; aa.nslots = append_max_slots(wide); aa.cap = append_max_cap(wide); aa.rounds = 1; aa.bar = nullptr;
        if (!append_fits(wide, bits, logB, logP, d->region_cap, aa.nslots, aa.cap))
            return append_not_taken(ctx, "no probe split with room for a rank in a table entry (very short or very long hash)");
        SKX_HIP(hipMemsetAsync(aa.overflow, 0, sizeof(int), st)); SKX_TRY(d_probe.zero(st));
        { KernelTimer kt(ctx, &ctx->tm.append_probe); if (wide) launch_append_wide_probe(aa, blocks, st); else launch_append_probe(aa, d->region_cap, blocks, st); }
        unsigned long long pr[2] = {0, 0}; int ov = 0;
        SKX_HIP(hipMemcpyAsync(pr, d_probe.p, 16, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipMemcpyAsync(&ov, aa.overflow, 4, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipStreamSynchronize(st));
        SKX_HIP(hipGetLastError());
        if (!ov) { e.u_est = std::max((double)raw_max * 0.5, (double)pr[0] / blocks * (double)(1ull << logP)); return SKX_OK; }
        if (ov & 4) return append_not_taken(ctx, "the table's bytes are not at LDS address 0");
        if (attempt >= 4 || logP + 2 > bits) return append_not_taken(ctx, "the probe blocks kept overflowing");
        logP += 2;
    }
}

// How a 2^logQ split is launched -- host arithmetic only.  cap / nslots: ranks and table slots of a block for its expected rows.  amp: the
// workgroups that read every region, each keeping a share: 8 at most where the regions are the 5 Mbp shape's (beyond that the samples are
// unrelated and the sorted path reads less), 32 where the regions have grown with the samples (one XCD's workgroups: 256 / 8) -- unless
// the words read stay few (allowed).  grid: workgroups of the persistent launch -- one per CU, whole groups of a region's readers (8 XCDs x
// amp), `rounds` row blocks each -- when the blocks divide that way; 0: one workgroup per row block.
// two_tier: the block hands out up to APPEND_MAX_RANKS ranks and its LDS table holds what a row buffer covers (rb_ranks).
struct AppendSplit { uint32_t cap, nslots; uint64_t amp; bool allowed; uint32_t rounds; uint64_t grid; uint32_t rb_ranks; };
static AppendSplit append_split(double u_est, double est_relvar, int logQ, int logB, uint32_t region_cap, bool wide, int cus, uint64_t raw_sum, bool two_tier = false)
{
    AppendSplit s{};
    const uint64_t nsub = 1ull << logQ;
    s.cap = ranks_for(u_est / (double)nsub, est_relvar, two_tier ? APPEND_MAX_RANKS : append_max_cap(wide));
    s.rb_ranks = two_tier ? std::min(s.cap, APPEND_TT_LDS_RANKS) : s.cap;
    s.nslots = slots_for(s.rb_ranks, append_max_slots(wide));
    s.amp = 1ull << (logQ - logB);
    const uint64_t amp_max = region_cap > lds_sort_max(wide) ? 32 : 8;
    s.allowed = !(s.amp > amp_max && (double)raw_sum * (double)s.amp > 4e8);
    uint64_t g = nsub;
    while (g > (uint64_t)std::max(cus, 1) && g % 2 == 0) g /= 2;
    const bool persistent = g <= (uint64_t)std::max(cus, 1) && nsub % g == 0 && g % (8 * s.amp) == 0 && logB >= 3;
    s.grid = persistent ? g : 0; s.rounds = persistent ? (uint32_t)(nsub / g) : 1;
    return s;
}

// Two tiers: whether the split one step COARSER than the coarsest whose blocks fit the LDS ranks should run, and when its LDS tier closes --
// host arithmetic only, from the row estimate and the samples' window counts.  Half the readers per region, if
//   (a) a block's rows, with the same six sigma, fit APPEND_MAX_RANKS;
//   (b) the population is related: the longest sample's windows per block (the rows the block has after its first sample, and about what every
//       sample looks up) are at most TT_HOT of the LDS tier's ranks.  TT_HOT is not derivable; see profiles/append_two_tier_policy_*.log;
//       and a later sample brings at most TT_NEW of a sample's rows as new ones (per <= TT_NEW x first: 0.35 % at the flagship, 100 % for
//       unrelated samples, whose late rows are looked up as often as the early ones);
//   (c) the waves meet while the LDS tier still has room: rows arrive as the first sample's and then an even share of the rest per sample
//       (per), the waves meet every 16 x resync samples, and what a block has by the first meeting fits the tier with six sigma.
//   (d) the blocks of the finer split are nearly full (their mean is at least TT_FULL of APPEND_MAX_CAP).  Measured: 1 000 x 5 Mbp, 5 520 rows
//       of 6 016 (0.92), the coarser split wins 1.1 ms; 500 x 5 Mbp, 3 392 (0.56), it LOSES 0.8 ms -- the finer split's table is 41 % full
//       there and the coarser split's LDS tier 65 %, so more look-ups leave the eight-slot window
//       (profiles/append_two_tier_policy_2026-10-21.log).
// The tier closes at the first meeting that finds lds_close rows: the tier's ranks less what may arrive before the NEXT meeting (16 x resync x
// per, six sigma, + 32) -- closing later would risk the block (a full LDS table fails it), closing earlier sends rows to tier 2 that the LDS
// had room for.  The table's slots follow slots_for(): a third more than the ranks, where all but 2 % of the keys lie in the look-up's window
// of eight slots.  A wrong guess costs time only: a block that fills either tier fails, and the pass comes back at the finer split, one tier.
constexpr double TT_HOT = 0.5, TT_NEW = 0.02, TT_FULL = 0.8;
struct TwoTierPlan { bool on = false; uint32_t lds_close = 0, resync = 16; };
static TwoTierPlan two_tier_plan(double u_est, double est_relvar, uint64_t raw_max, int S, int logQ_fine, int min_logQ)
{
    TwoTierPlan p;
    p.resync = (uint32_t)std::min(16, std::max(1, S / 64));
    if (logQ_fine - 1 < min_logQ || S < 2) return p;
    if ((int)p.resync > (S - 16) / 16) return p;                          // (no meeting at which every wave has a sample: append_kernel)
    const double nsub = (double)(1ull << (logQ_fine - 1));
    const double first = (double)raw_max / nsub, per = std::max(0.0, u_est - (double)raw_max) / nsub / (double)(S - 1), between = 16.0 * p.resync * per;
    if (ranks_need(u_est / nsub, est_relvar) > (double)APPEND_MAX_RANKS) return p;                       // (a)
    if (first > TT_HOT * (double)APPEND_TT_LDS_RANKS) return p;                                            // (b)
    if (per > TT_NEW * first) return p;                                                                    // (b)
    if (ranks_need(first + between, est_relvar) > (double)APPEND_TT_LDS_RANKS) return p;                 // (c)
    if (u_est / (2.0 * nsub) < TT_FULL * (double)APPEND_MAX_CAP) return p;                                  // (d)
    p.lds_close = (uint32_t)std::max(1.0, (double)APPEND_TT_LDS_RANKS - ranks_need(between, 0.0));
    p.on = true;
    return p;
}

// a test hook of the library (not in include/skx.h): the plan for these numbers -- out[0] taken, out[1] lds_close, out[2] resync
extern "C" int skx_debug_two_tier_plan(double u_est, double est_relvar, uint64_t raw_max, int n_samples, int logQ_fine, int min_logQ, uint32_t *out)
{
    if (!out) { set_error("bad arguments"); return SKX_EINVAL; }
    const TwoTierPlan p = two_tier_plan(u_est, est_relvar, raw_max, n_samples, logQ_fine, min_logQ);
    out[0] = p.on ? 1u : 0u; out[1] = p.lds_close; out[2] = p.resync;
    return SKX_OK;
}

// the pass itself: the row blocks' keys (ks: stage / ncnt / roff, stride = cap) and the samples' pieces
static int append_pass(skx_ctx *ctx, skx_dictset *d, std::unique_ptr<skx_keyset> &ks_out, std::unique_ptr<skx_pieces> &pc_out)
{
    if (d->sorted) return append_not_taken(ctx, "the dictionaries are sorted (read sets, oversize or repeat-rich samples, SKX_KNOBS=sorted_dicts)");
    if (d->n > 65535 || d->n < 1) return append_not_taken(ctx, "more than 65535 samples");
    SKX_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const bool wide = d->wide();                                       // 16-byte words, 16-byte table entries: skx_append_wide.inc
    const int S = d->n, bits = wide ? d->wh.bits : d->hp.bits, logB = d->logB, wpk = wide ? 2 : 1;
    uint64_t raw_sum = 0, raw_max = 0;
    for (auto v : d->raw_total) { raw_sum += v; raw_max = std::max(raw_max, v); }
    const int min_logQ = std::max(logB, bits - (wide ? 113 : 50));
    if (min_logQ > bits) return append_not_taken(ctx, "no row-block split with room for a rank in a table entry");
    // (regions of any size: a wave streams a region in chunks of 1 024 words -- the samples above ~5 Mbp of round 6 keep their bucket count and
    // grow their regions)
    DevBuf<int> d_flag; SKX_TRY(d_flag.alloc(1));
    AppendArgs aa{};
    aa.words = d->words.p; aa.off = d->off.p; aa.raw = d->raw.p; aa.n_samples = S; aa.logB = logB; aa.bits = bits; aa.overflow = d_flag.p;
    StageTimer t(ctx, &ctx->tm.key_union);
    RowEstimate e;
    SKX_TRY(estimate_rows(ctx, d, aa, min_logQ, raw_max, e));
    // the coarsest split whose blocks hold their rows with six sigma to spare (a finer one reads every region more often)
    int logQ = min_logQ;
    while (logQ < bits && ranks_need(e.u_est / (double)(1ull << logQ), e.est_relvar) > (double)append_max_cap(wide)) logQ++;
    // (tests: SKX_KNOBS=append_coarse=N starts N steps coarser, so that row blocks overflow and the retries below run -- no input reaches them)
    // Two tiers (64-bit keys; SKX_KNOBS=append_two_tier=0: never): one step coarser where two_tier_plan() says so -- the first attempt only,
    // a block that fails comes back at the split above with one tier.  Tests: SKX_KNOBS=append_lds_ranks=N runs every attempt with two tiers
    // at whatever split it has, the waves meeting after every sample and the LDS tier closing at the first meeting that finds N rows (N = 1:
    // closed from the start, every row in tier 2).
    const long tt_knob = wide || knob("append_two_tier", 1) == 0 ? 0 : knob("append_lds_ranks");
    TwoTierPlan tt;
    if (!wide && knob("append_two_tier", 1) != 0 && tt_knob <= 0) tt = two_tier_plan(e.u_est, e.est_relvar, raw_max, S, logQ, min_logQ);
    if (tt.on) logQ--;
    if (tt_knob > 0) { tt.lds_close = tt_knob <= 1 ? 0u : (uint32_t)tt_knob; tt.resync = 1; }
    if (knob("append_coarse") > 0) logQ = std::max<long>(min_logQ, logQ - knob("append_coarse"));
    int cus = 0; (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
    for (int attempt = 0;; attempt++, logQ++) {
        const bool two = tt_knob > 0 || (tt.on && attempt == 0);
        if (logQ > bits || attempt > (tt.on ? 4 : 3)) return append_not_taken(ctx, "row blocks kept overflowing (a sample that is one repeat, or far more rows than the probe saw)");
        const uint64_t nsub = 1ull << logQ;
        const AppendSplit sp = append_split(e.u_est, e.est_relvar, logQ, logB, d->region_cap, wide, cus, raw_sum, two);
        if (!sp.allowed) return append_not_taken(ctx, "too many row blocks per region: every region would be read too often");
        if (!(two ? append_ok(bits, logB, logQ, d->region_cap, sp.nslots, sp.cap, sp.rb_ranks) : append_fits(wide, bits, logB, logQ, d->region_cap, sp.nslots, sp.cap)))
            return append_not_taken(ctx, "no row-block split that fits the LDS");
        std::unique_ptr<skx_keyset> ks(new skx_keyset());
        ks->ctx = ctx; ks->k = d->k; ks->rc = d->rc; ks->logN = logQ; ks->hp = d->hp; ks->wh = d->wh; ks->wide = wide; ks->stride = sp.cap;
        std::unique_ptr<skx_pieces> pc(new skx_pieces());
        pc->cap = sp.cap; pc->logQ = logQ;
        SKX_TRY(ks->stage.alloc(nsub * sp.cap * wpk)); SKX_TRY(ks->ncnt.alloc(nsub));
        if (pc->data.alloc(nsub * (uint64_t)S * (sp.cap / 2)) != SKX_OK) return append_not_taken(ctx, "no room for the pieces");      // (the sorted path holds rows + dictionaries instead)
        SKX_TRY(pc->plen.alloc(nsub * (uint64_t)S + 2)); SKX_TRY(pc->perm.alloc(nsub * sp.cap)); SKX_TRY(pc->nrank.alloc(nsub));
        SKX_TRY(d_flag.zero(st));
        DevBuf<int> d_bar;
        if (sp.grid) { SKX_TRY(d_bar.alloc(2ull << logB)); SKX_TRY(d_bar.zero(st)); }      // (second half: the readers' meetings inside a round)
        aa.logQ = logQ; aa.nslots = sp.nslots; aa.cap = sp.cap; aa.rounds = sp.rounds; aa.bar = d_bar.p;
        aa.pieces = pc->data.p; aa.plen = pc->plen.p; aa.perm = pc->perm.p; aa.nrank = pc->nrank.p;
        aa.stage = ks->stage.p; aa.stride = sp.cap; aa.ncnt = ks->ncnt.p;
        DevBuf<unsigned long long> d_t2, d_tts;
        aa.two_tier = two ? 1 : 0; aa.rb_ranks = sp.rb_ranks; aa.lds_close = tt.lds_close; aa.resync = tt.resync; aa.t2 = nullptr; aa.tt_stat = nullptr;
        if (two) {
            const uint64_t wgs = nsub / sp.rounds;                     // (the launch's workgroups: launch_append)
            if (d_t2.alloc(wgs * (uint64_t)(APPEND_T2_SLOTS + APPEND_T2_PAD)) != SKX_OK) return append_not_taken(ctx, "no room for the second tier");
            SKX_TRY(d_tts.alloc(APPEND_TT_STATS)); SKX_TRY(d_tts.zero(st));
            aa.t2 = d_t2.p; aa.tt_stat = d_tts.p;
        }
        { KernelTimer kt(ctx, &ctx->tm.append); if (wide) launch_append_wide(aa, st); else launch_append(aa, d->region_cap, st); }
        int ov = 0;
        unsigned long long tts[APPEND_TT_STATS] = {};
        SKX_HIP(hipMemcpyAsync(&ov, d_flag.p, 4, hipMemcpyDeviceToHost, st));
        if (two && getenv("SKX_DEBUG")) SKX_HIP(hipMemcpyAsync(tts, d_tts.p, sizeof tts, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipStreamSynchronize(st));
        SKX_HIP(hipGetLastError());
        if (getenv("SKX_DEBUG")) {
            fprintf(stderr, "[skx] append%s: logQ=%d (x%llu per region) cap=%u slots=%u rows~%.0f -> %s [sized by %s]\n", wide ? " (128-bit keys)" : "", logQ, (unsigned long long)sp.amp, sp.cap, sp.nslots, e.u_est, ov ? "overflow" : "ok", e.sized);
            // (blocks that failed are not counted: closed / tier-2 rows are those of the blocks that were emitted)
            if (two) fprintf(stderr, "[skx] append two tiers: %s split, lds_ranks=%u close_at=%u meet_every=%u closed_blocks=%llu of %llu lds_rows=%llu last_close_meeting=%llu tier2_rows=%llu list_flushes=%llu\n",
                             tt.on ? "coarser" : "same", sp.rb_ranks, tt.lds_close, tt.resync, tts[0], (unsigned long long)nsub, tts[1], tts[3], tts[2], tts[4]);
        }
        if (ov & 4) return append_not_taken(ctx, "the table's bytes are not at LDS address 0");
        if (ov) continue;
        SKX_TRY(keyset_finish(ks.get()));
        ctx->merge_path = wide ? "append128" : "append64";
        ks_out = std::move(ks); pc_out = std::move(pc);
        return SKX_OK;
    }
}

// An array over the pieces of an append pass.  own rows: the pass's own row blocks (ks: ncnt / roff / stage, the pieces' perm); global rows
// (a sharded job, `g` = the rows skx_keyset_allgather returned): the rank's columns over all ranks' rows -- block j covers rows
// [g_base[j], g_base[j] + g_n[j]) and g_perm maps its first-seen ranks to places in that range; rows the rank does not hold have no cell.
static int array_over_pieces(skx_ctx *ctx, const skx_dictset *d, skx_keyset *ks, skx_pieces *pc_, skx_keyset *g, const char *const *names, skx_array **out)
{
    std::unique_ptr<skx_pieces> pc(pc_);
    hipStream_t st = ctx->stream;
    const int logQ = pc->logQ;
    const uint64_t nsub = 1ull << logQ;
    std::unique_ptr<skx_keyset> blk(new skx_keyset());                 // what the array keeps of the row blocks: ncnt / roff
    blk->ctx = ctx; blk->k = d->k; blk->rc = d->rc; blk->logN = logQ; blk->hp = d->hp; blk->wh = d->wh; blk->wide = d->wide(); blk->stride = pc->cap;
    uint64_t U;
    if (g) {
        U = g->total;
        pc->perm = std::move(g->g_perm);
        blk->ncnt = std::move(g->g_n);
        SKX_TRY(blk->roff.alloc(nsub + 1));
        SKX_HIP(hipMemcpyAsync(blk->roff.p, g->g_base.p, nsub * 8, hipMemcpyDeviceToDevice, st));
        SKX_HIP(hipMemcpyAsync(blk->roff.p + nsub, &U, 8, hipMemcpyHostToDevice, st));
        SKX_HIP(hipStreamSynchronize(st));                             // (&U)
        g->g_base.release();
        blk->total = U; blk->max_rows = g->g_max;
    } else {
        // (copied, not taken: the caller's key set stays whole -- skx_keyset_allgather, keyset_flatten or a second assemble may follow)
        U = ks->total;
        SKX_TRY(blk->ncnt.alloc(nsub)); SKX_TRY(blk->roff.alloc(nsub + 1));
        SKX_HIP(hipMemcpyAsync(blk->ncnt.p, ks->ncnt.p, nsub * 4, hipMemcpyDeviceToDevice, st));
        SKX_HIP(hipMemcpyAsync(blk->roff.p, ks->roff.p, (nsub + 1) * 8, hipMemcpyDeviceToDevice, st));
        blk->total = U; blk->max_rows = ks->max_rows;
    }
    std::unique_ptr<skx_array> a;
    SKX_TRY(new_array(ctx, d, names, U, a));
    if (U) {
        if (g) gather_row_keys(g, g->ncnt.p, g->roff.p, a->keys.p, st);       // the rows' keys
        else gather_row_keys(ks, blk->ncnt.p, blk->roff.p, a->keys.p, st);
        if (g) { SKX_TRY(a->present.zero(st)); SKX_TRY(a->unambig.zero(st)); SKX_TRY(a->mask.zero(st)); SKX_TRY(a->vcount.zero(st)); }
    }
    a->pieces = pc.release(); a->lazy_rows = blk.release();
    // the rows' statistics, counted from the pieces: at once for a sharded job's rows (skx_array_reduce_stats reads every row next) and with
    // SKX_KNOBS=stats_eager (the A/B, the differential tests); a pass's own rows get them when first asked for -- `ska align` filters next, and
    // its pass reads only the ranks that can reach min_count (array_lazy_stats, skx_array_filter)
    a->stats_ready = g || knob("stats_eager");
    if (a->stats_ready) SKX_TRY(pieces_stats_pass(a.get(), 0));
    SKX_HIP(hipStreamSynchronize(st));
    SKX_HIP(hipGetLastError());
    *out = a.release();
    return SKX_OK;
}
static int merge_append(skx_ctx *ctx, skx_dictset *d, const char *const *names, skx_array **out)
{
    std::unique_ptr<skx_keyset> ks; std::unique_ptr<skx_pieces> pc;
    const int r = append_pass(ctx, d, ks, pc);
    if (r != SKX_OK) return r;
    return array_over_pieces(ctx, d, ks.get(), pc.release(), nullptr, names, out);
}

static int keyset_union_dict(skx_ctx *ctx, skx_dictset *d, skx_keyset **out, bool with_side)
{
    if (!ctx || !d || !out) { set_error("bad arguments"); return SKX_EINVAL; }
    SKX_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (with_side && !d->sorted && !d->wide()) {
        // assemblies as the extraction kernel left them: the append pass finds the rank's rows AND leaves the samples' cells as pieces, which
        // travel with the key set (to the global rows of a sharded job: skx_keyset_allgather) like the notes of the union pass
        // (128-bit keys: the exchange composes 64-bit rows only -- skx_comm.hip -- so a sharded job's ranks sort their dictionaries)
        std::unique_ptr<skx_keyset> ks; std::unique_ptr<skx_pieces> pc;
        const int r = append_pass(ctx, d, ks, pc);
        if (r == SKX_OK) { ks->pieces = pc.release(); ks->pieces_of = d; ks->pieces_of_id = d->id; *out = ks.release(); return SKX_OK; }
        if (r != SKF_NOT_TAKEN) return r;
    }
    if (!d->sorted && d->wide() && with_side) ctx->merge_path = "sorted: the key-table exchange of a sharded job composes 64-bit rows only";
    else if (!d->sorted && !with_side) ctx->merge_path = "sorted: a row set without cells was asked for (skx_keyset_union)";
    SKX_TRY(dictset_sort(d));                        // the union kernels read sorted slices
    StageTimer t(ctx, &ctx->tm.key_union);
    DictView v = d->view();
    // estimate |U| from a thin slice of the hash space (probe sub-buckets of a 2^logP split)
    uint64_t maxs = 0, sum = 0;
    for (auto s : d->sample_size) { maxs = std::max(maxs, s); sum += s; }
    uint64_t est = maxs;
    if (d->n > 1) {
        const int logP = std::min(2 * (d->k - 1), std::max(d->logB, ilog2_ceil((sum + 1023) / 1024)));
        const int probe = (int)std::min<uint64_t>(64, 1ull << logP);
        DevBuf<uint32_t> d_cnt; DevBuf<int> d_flag;
        SKX_TRY(d_cnt.alloc(1)); SKX_TRY(d_flag.alloc(1)); SKX_TRY(d_cnt.zero(st)); SKX_TRY(d_flag.zero(st));
        if (d->wide()) launch_union_probe_wide(v, logP, probe, d_cnt.p, 4096, d_flag.p, st);
        else launch_union_probe(v, logP, probe, d_cnt.p, 8192, d_flag.p, st);
        uint32_t cnt = 0; int ov = 0;
        SKX_HIP(hipMemcpyAsync(&cnt, d_cnt.p, 4, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipMemcpyAsync(&ov, d_flag.p, 4, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipStreamSynchronize(st));
        if (!ov) est = std::max<uint64_t>(maxs, (uint64_t)((double)cnt * (double)(1ull << logP) / probe * 1.1));
        else est = sum;
    }
    return keyset_union_views(ctx, v, d->k, d->rc, d->hp, est, out, with_side ? d : nullptr);
}
extern "C" int skx_keyset_union(skx_ctx *ctx, skx_dictset *d, skx_keyset **out)
{
    return skx_guarded([&]() -> int { return keyset_union_dict(ctx, d, out, false); });
}
extern "C" int skx_keyset_union_notes(skx_ctx *ctx, skx_dictset *d, skx_keyset **out)
{
    // (a sharded job hands this key set to skx_keyset_allgather, which carries the notes over to the global rows)
    return skx_guarded([&]() -> int { return keyset_union_dict(ctx, d, out, true); });
}

extern "C" int skx_array_assemble(skx_ctx *ctx, skx_dictset *d, skx_keyset *rows, const char *const *names, skx_array **out)
{
    return skx_guarded([&]() -> int {
    if (!ctx || !d || !rows || !out) { set_error("bad arguments"); return SKX_EINVAL; }
    if (rows->k != d->k) { set_error("K-mer lengths do not match: %d %d", d->k, rows->k); return SKX_EINVAL; }      // merge_ska_dict.rs:78-84
    if (rows->rc != d->rc) { set_error("Strand use inconsistent"); return SKX_EINVAL; }                              // :85-87
    if (d->n > 65535) { set_error("more than 65535 samples per device array"); return SKX_EUNSUP; }
    SKX_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (rows->holds_pieces_of(d)) {
        // the rows came from an append pass over these samples (skx_keyset_union_notes), directly (its own row blocks) or through the key-table
        // exchange of a sharded job (which hands the pieces on only together with g_perm): the cells are there already, as pieces
        skx_pieces *pc = rows->pieces; rows->pieces = nullptr; rows->pieces_of = nullptr;
        return array_over_pieces(ctx, d, rows, pc, rows->g_perm.p ? rows : nullptr, names, out);
    }
    SKX_TRY(dictset_sort(d));
    std::unique_ptr<skx_keyset> rebuilt;
    if (rows->logN < 0 || rows->logN < d->logB) {      // flat / too coarse: re-slab at a granularity the dictionaries' buckets divide
        if (rows->logN >= 0) SKX_TRY(keyset_flatten(rows));
        const uint64_t h_off[2] = {0, rows->total}; const uint32_t h_cnt = (uint32_t)rows->total;
        TablesView tv; SKX_TRY(tables_view(tv, rows->flat.p, h_off, &h_cnt, 1, rows->k, st));
        skx_keyset *tmp = nullptr;
        uint64_t hint = std::max<uint64_t>(rows->total, (uint64_t)2500 << d->logB);
        SKX_TRY(keyset_union_views(ctx, tv.v, rows->k, rows->rc, rows->hp, hint, &tmp));
        SKX_HIP(hipStreamSynchronize(st));
        rebuilt.reset(tmp);
        rows = tmp;
        if (rows->logN < d->logB) { set_error("internal: keyset granularity"); return SKX_EUNSUP; }
    }
    const uint64_t U = rows->total;
    std::unique_ptr<skx_array> a;
    SKX_TRY(new_array(ctx, d, names, U, a));
    a->pitch = pitch_for(U);
    SKX_TRY(a->matrix.alloc((uint64_t)d->n * a->pitch));
    DevBuf<int> d_flag; SKX_TRY(d_flag.alloc(1)); SKX_TRY(d_flag.zero(st));
    if (U) {
        AssembleArgs aa = assemble_args(d, rows, a.get(), d_flag.p);
        aa.matrix = a->matrix.p; aa.pitch = a->pitch;
        {
            StageTimer t(ctx, &ctx->tm.assemble);
            if (rows->g_perm.p && rows->side.p && rows->side_of == d && !rebuilt && !rows->wide) {
                // a sharded job: the notes were taken against this rank's own rows and composed with the global rows (skx_keyset_allgather):
                // workgroup j = own sub-bucket j, over the global rows of its hash range
                AssembleArgs ag = aa;
                ag.logN = rows->l_logN; ag.stride = rows->l_stride; ag.ncnt = rows->g_n.p; ag.roff = rows->g_base.p; ag.max_rows = rows->g_max;
                launch_assemble_side(ag, rows->side.p, rows->g_perm.p, st, false);
            }
            else if (rows->side.p && !rows->g_perm.p && rows->side_of == d && !rebuilt) launch_assemble_side(aa, rows->side.p, rows->perm.p, st, rows->wide);      // the union over d left its notes
            else if (rows->wide) launch_assemble_wide(aa, st);
            else launch_assemble(aa, st);
        }
        gather_row_keys(rows, rows->ncnt.p, rows->roff.p, a->keys.p, st);
        SKX_HIP(hipMemcpyAsync(a->vcount.p, a->present.p, U * 4, hipMemcpyDeviceToDevice, st));     // merge_ska_array.rs:172
    }
    SKX_TRY(check_missing(ctx, d_flag.p));
    *out = a.release();
    return SKX_OK;
    });
}

// ---- lazily held arrays -------------------------------------------------------------------------------------------------
// takes ownership of d and rows (also on failure)
static int array_make_lazy(skx_ctx *ctx, skx_dictset *d, skx_keyset *rows, const char *const *names, skx_array **out)
{
    std::unique_ptr<skx_dictset> own_d(d); std::unique_ptr<skx_keyset> own_rows(rows);
    // the union's notes serve the eager assemble only (skx_merge, skx_array_assemble): a lazily held array fills its windows from the
    // dictionaries, so the 2 bytes per word are not kept for its lifetime
    rows->side.release(); rows->perm.release(); rows->g_perm.release(); rows->g_n.release(); rows->g_base.release(); rows->side_of = nullptr;
    std::unique_ptr<skx_array> a;
    SKX_TRY(new_array(ctx, d, names, rows->total, a));
    a->lazy_dict = own_d.release(); a->lazy_rows = own_rows.release(); a->stats_ready = false;
    if (a->n_rows) gather_row_keys(rows, rows->ncnt.p, rows->roff.p, a->keys.p, ctx->stream);
    SKX_HIP(hipStreamSynchronize(ctx->stream));
    *out = a.release();
    return SKX_OK;
}
extern "C" int skx_array_assemble_lazy(skx_ctx *ctx, skx_dictset *d, skx_keyset *rows, const char *const *names, skx_array **out)
{
    return skx_guarded([&]() -> int {
    if (!ctx || !d || !rows || !out) { skx_dictset_free(d); skx_keyset_free(rows); set_error("bad arguments"); return SKX_EINVAL; }
    // an append pass's rows: the array over its pieces is the lazy form.  Otherwise the lazy form needs a row set slabbed at least as finely
    // as the dictionaries' buckets; anything else is assembled at once
    if (rows->holds_pieces_of(d) || rows->wide != d->wide() || rows->k != d->k || rows->rc != d->rc || rows->logN < 0 || rows->logN < d->logB || d->n > 65535 ||
        knob("eager_array")) {
        const int r = skx_array_assemble(ctx, d, rows, names, out);
        skx_dictset_free(d); skx_keyset_free(rows);
        return r;
    }
    SKX_HIP(hipSetDevice(ctx->device));
    { const int rs = dictset_sort(d); if (rs != SKX_OK) { skx_dictset_free(d); skx_keyset_free(rows); return rs; } }
    return array_make_lazy(ctx, d, rows, names, out);
    });
}

static void launch_assemble_lazy(skx_array *a, const AssembleArgs &aa, hipStream_t st, int mode, uint32_t n_blocks = 0)
{
    if (a->lazy_rows->wide) launch_assemble_wide(aa, st, mode, n_blocks); else launch_assemble(aa, st, mode, n_blocks);
}
int skx::array_lazy_stats(skx_array *a)
{
    if (!a->lazy() || a->stats_ready) return SKX_OK;
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    if (a->pieces) {                                                   // an append pass's own rows: counted from the pieces, every rank
        ctx->cut_ranks = ctx->cut_blocks = 0;
        SKX_TRY(pieces_stats_pass(a, 0));
        a->stats_ready = true;
        return SKX_OK;
    }
    DevBuf<int> d_flag; SKX_TRY(d_flag.alloc(1)); SKX_TRY(d_flag.zero(st));
    if (a->n_rows) {
        AssembleArgs aa = assemble_args(a->lazy_dict, a->lazy_rows, a, d_flag.p);
        { StageTimer t(ctx, &ctx->tm.assemble); launch_assemble_lazy(a, aa, st, 1); }
        SKX_HIP(hipMemcpyAsync(a->vcount.p, a->present.p, a->n_rows * 4, hipMemcpyDeviceToDevice, st));     // merge_ska_array.rs:172
    }
    SKX_TRY(check_missing(ctx, d_flag.p));
    a->stats_ready = true;
    return SKX_OK;
}

// Rows of a lazily held array into the caller's buffer, from the pieces or from the dictionaries, whichever the array holds: cell (s, r) at
// out + s * pitch + (r - col_base).  n_blocks = 0: every row block; else the blocks [j_base, j_base + n_blocks) of the rows' split (a window).
// keep / kpos (row flags and their exclusive scan): only the rows with keep == 1, row r at column kpos[r], ambiguous cells as 'N' with
// mask_ambig; full_pieces: see PiecesRowsArgs.  The dictionaries' kernel also reports a key the rows lack, and is waited for.
int skx::array_lazy_rows(skx_array *a, uint8_t *out, uint64_t pitch, uint32_t j_base, uint32_t n_blocks, uint64_t col_base, const uint8_t *keep, const uint64_t *kpos,
                         int mask_ambig, bool full_pieces)
{
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    if (a->pieces) {
        const skx_pieces *pc = a->pieces; const skx_keyset *rows = a->lazy_rows;
        PiecesRowsArgs pa{};
        pa.pieces = pc->data.p; pa.plen = pc->plen.p; pa.perm = pc->perm.p; pa.nrank = pc->nrank.p; pa.cap = pc->cap; pa.n_samples = (int)a->names.size();
        pa.ncnt = rows->ncnt.p; pa.roff = rows->roff.p;
        pa.out = out; pa.pitch = pitch; pa.j_base = j_base; pa.col_base = col_base;
        pa.keep = keep; pa.kpos = kpos; pa.mask_ambig = mask_ambig; pa.full_pieces = full_pieces ? 1 : 0;
        const uint32_t nb = n_blocks ? n_blocks : 1u << pc->logQ;
        // (the kept rows are the filter's: inside its compaction stage, with a slot of their own)
        if (keep) { KernelTimer kt(ctx, &ctx->tm.pieces_rows); launch_pieces_rows(pa, nb, st); }
        else { StageTimer t(ctx, &ctx->tm.assemble); launch_pieces_rows(pa, nb, st); }
        SKX_HIP(hipGetLastError());
        return SKX_OK;
    }
    DevBuf<int> d_flag; SKX_TRY(d_flag.alloc(1)); SKX_TRY(d_flag.zero(st));
    AssembleArgs aa = assemble_args(a->lazy_dict, a->lazy_rows, a, d_flag.p);
    aa.matrix = out; aa.pitch = pitch; aa.j_base = j_base; aa.col_base = col_base;
    aa.keep = keep; aa.kpos = kpos; aa.mask_ambig = mask_ambig;
    { StageTimer t(ctx, &ctx->tm.assemble); launch_assemble_lazy(a, aa, st, keep ? 2 : 0, n_blocks); }
    return check_missing(ctx, d_flag.p);
}
int skx::array_materialize(skx_array *a)
{
    if (!a->lazy()) return SKX_OK;
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    if (a->pieces) SKX_TRY(array_lazy_stats(a));                       // (the pieces are dropped below: the statistics are counted from them first)
    const uint64_t U = a->n_rows;
    a->pitch = pitch_for(U);
    SKX_TRY(a->matrix.alloc((uint64_t)a->names.size() * a->pitch));
    if (U) {
        SKX_TRY(array_lazy_rows(a, a->matrix.p, a->pitch));
        // (from the dictionaries without a statistics pass before: the kernel has just counted the rows)
        if (!a->stats_ready) SKX_HIP(hipMemcpyAsync(a->vcount.p, a->present.p, U * 4, hipMemcpyDeviceToDevice, st));
    }
    SKX_HIP(hipStreamSynchronize(st));
    SKX_HIP(hipGetLastError());
    a->stats_ready = true;
    a->drop_lazy();
    return SKX_OK;
}
int skx::array_lazy_window(skx_array *a, uint64_t r0, uint64_t nr, DevBuf<uint8_t> &buf, const uint8_t **win, uint64_t *wpitch)
{
    skx_keyset *rows = a->lazy_rows;
    if (rows->h_roff.empty()) {
        rows->h_roff.resize((1ull << rows->logN) + 1);
        SKX_HIP(hipMemcpy(rows->h_roff.data(), rows->roff.p, rows->h_roff.size() * 8, hipMemcpyDeviceToHost));
    }
    const auto &ro = rows->h_roff;
    const uint64_t j0 = (uint64_t)(std::upper_bound(ro.begin(), ro.end(), r0) - ro.begin()) - 1;                // sub-bucket holding row r0
    const uint64_t j1 = (uint64_t)(std::lower_bound(ro.begin(), ro.end(), r0 + nr) - ro.begin());                // first sub-bucket past the last row
    const uint64_t c0 = ro[j0] & ~15ull, span = ro[j1] - c0;                                                     // 16-B aligned window start
    const uint64_t wp = pitch_for(span);
    const size_t S = a->names.size();
    if (buf.n < S * wp) SKX_TRY(buf.alloc(S * wp));
    SKX_TRY(array_lazy_rows(a, buf.p, wp, (uint32_t)j0, (uint32_t)(j1 - j0), c0));
    *win = buf.p + (r0 - c0); *wpitch = wp;
    return SKX_OK;
}

// ---- merge ------------------------------------------------------------------------------------------------------------------------------
extern "C" int skx_merge(skx_ctx *ctx, skx_dictset *d, const char *const *names, skx_array **out)
{
    return skx_guarded([&]() -> int {
    if (!ctx || !d || !out) { set_error("bad arguments"); return SKX_EINVAL; }
    { const int ra = merge_append(ctx, d, names, out); if (ra != SKF_NOT_TAKEN) return ra; }
    // (sorted here: the union below would otherwise offer the dictset to the append pass once more -- probe and four launches again)
    SKX_TRY(dictset_sort(d));
    skx_keyset *ks = nullptr;
    SKX_TRY(keyset_union_dict(ctx, d, &ks, true));
    int r = skx_array_assemble(ctx, d, ks, names, out);
    skx_keyset_free(ks);
    return r;
    });
}

// One batch of skx_build_and_merge: the batch's dictset (owned from here on, also on failure) -> its array.  Assemblies: straight from the
// extraction kernel's regions, the array holds the pieces.  Else rows now, cells on demand: the array keeps the dictionaries (see
// skx_array::lazy_dict; the union without notes: a lazily held array does not use them) -- or, with SKX_KNOBS=eager_array, the matrix at once.
int skx::merge_batch(skx_ctx *ctx, skx_dictset *d, const char *const *names, skx_array **out)
{
    const auto t0 = std::chrono::steady_clock::now();
    int r = merge_append(ctx, d, names, out);
    if (r == SKF_NOT_TAKEN && !knob("eager_array")) {
        skx_keyset *ks = nullptr;
        r = skx_keyset_union(ctx, d, &ks);
        if (r == SKX_OK) r = array_make_lazy(ctx, d, ks, names, out); else skx_dictset_free(d);
        d = nullptr;
    } else if (r == SKF_NOT_TAKEN)
        r = skx_merge(ctx, d, names, out);
    const auto t1 = std::chrono::steady_clock::now();
    skx_dictset_free(d);
    phase_add("build.merge", std::chrono::duration<double>(t1 - t0).count());
    phase_add("build.release_dictionaries", std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count());
    return r;
}
