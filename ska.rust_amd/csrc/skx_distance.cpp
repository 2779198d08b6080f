// skx_distance.cpp -- the distance entry points of the C ABI (include/skx.h).  Each is its steps: check the arguments, materialise the array,
// the query plan if there is one, the bit planes (build_planes), the pair sweep (sweep_band: one band for a table, the band loop for the
// selection and the banded consumers), the finish (finish_counts: the table's arithmetic, whoever prints the pair).
#include "skx_internal.h"
#include "../../include/skx_host.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>

using namespace skx;

// pair-class counts -> VariantDist (merge_ska_array.rs:596-631), pairs (i in [i_lo, i_hi), j > i) row-major; h rows are relative to i_lo.
// In two steps, because the line selection (skx_select.hip) does the first on the device and hands the integers over: the counts -> mismatches,
// m (what joins the constant in the matches) and key (the exact numerator of the distance: over 1 with filt_ambig, over 36 without;
// pair_class_num in skx_internal.h); the integers -> the table's doubles
static void pair_integers(const unsigned long long *c, int filt_ambig, unsigned long long &mism, unsigned long long &m, unsigned long long &key)
{
    mism = c[0];
    if (filt_ambig) { m = c[2]; key = c[2] - c[3]; }
    else {
        unsigned long long num = 0;
        m = 0;
        for (int q = 0; q < 10; q++) { m += c[2 + q]; num += c[2 + q] * (unsigned long long)pair_class_num(q); }
        key = 36ull * c[1] - num;
    }
}
static void finish_counts(unsigned long long mism, unsigned long long m, unsigned long long key, double constant, int filt_ambig, skx_dist &o)
{
    double mismatches = (double)mism, matches = constant;
    matches += (double)m;
    o.distance = key_distance(key, filt_ambig);
    o.mismatch_prop = (matches + mismatches) == 0.0 ? 0.0 : mismatches / (matches + mismatches);
    o.match_count = (uint64_t)matches; o.mismatch_count = (uint64_t)mismatches;
}
static void finish_pair(const unsigned long long *c, double constant, int filt_ambig, skx_dist &o)
{
    unsigned long long mism, m, key;
    pair_integers(c, filt_ambig, mism, m, key);
    finish_counts(mism, m, key, constant, filt_ambig, o);
}
static void finish_pairs(const unsigned long long *h, int S, int i_lo, int i_hi, double constant, int filt_ambig, skx_dist *out)
{
    uint64_t n = 0;
    for (int i = i_lo; i < i_hi; i++)
        for (int j = i + 1; j < S; j++, n++) finish_pair(&h[((uint64_t)(i - i_lo) * S + j) * DIST_NCOUNT], constant, filt_ambig, out[n]);
}
// ---- the query form (skx_array_distance_query*): the planes are built in query-first order -- slot s holds sample order[s], the queries
// ascending in slots [0, Q), every other sample ascending behind them -- and the band [0, Q) of the pair sweep then holds every pair with a
// query in it exactly once, in a count buffer of Q x S pairs.  The counts of a pair do not depend on which of the two comes first.
struct skx::QueryPlan {
    std::vector<int> query, slot;         // query[q] = sample of the caller's q-th row; slot[sample] = where the planes hold it
    DevBuf<int> order;                    // [S] on the device
    int Q() const { return (int)query.size(); }
};
static int query_plan(skx_array *a, const int *query, int n_query, QueryPlan &qp)
{
    const int S = (int)a->names.size();
    if (!query || n_query < 1) { set_error("distance query: at least one query sample is needed"); return SKX_EINVAL; }
    std::vector<char> is_q((size_t)S, 0);
    for (int q = 0; q < n_query; q++) {
        if (query[q] < 0 || query[q] >= S) { set_error("distance query: sample index %d is outside the array's %d samples", query[q], S); return SKX_EINVAL; }
        if (is_q[query[q]]) { set_error("distance query: sample index %d is given twice", query[q]); return SKX_EINVAL; }
        is_q[query[q]] = 1;
    }
    qp.query.assign(query, query + n_query);
    std::vector<int> order; order.reserve((size_t)S);
    for (int pass = 1; pass >= 0; pass--) for (int s = 0; s < S; s++) if (is_q[s] == pass) order.push_back(s);
    qp.slot.resize((size_t)S);
    for (int s = 0; s < S; s++) qp.slot[order[s]] = s;
    SKX_TRY(qp.order.alloc((uint64_t)S));
    SKX_HIP(hipMemcpyAsync(qp.order.p, order.data(), (size_t)S * sizeof(int), hipMemcpyHostToDevice, a->ctx->stream));
    SKX_HIP(hipStreamSynchronize(a->ctx->stream));            // (order is a local)
    return SKX_OK;
}
// h = the counts of the band [0, Q) over slots; out[q * S + j] = the pair (query[q], j), zeroed where j is the query itself
static void finish_query(const unsigned long long *h, int S, const QueryPlan &qp, double constant, int filt_ambig, skx_dist *out)
{
    for (int q = 0; q < qp.Q(); q++)
        for (int j = 0; j < S; j++) {
            skx_dist &o = out[(uint64_t)q * S + j];
            const int x = qp.slot[qp.query[q]], y = qp.slot[j];
            if (x == y) { o = skx_dist{}; continue; }
            finish_pair(&h[((uint64_t)std::min(x, y) * S + std::max(x, y)) * DIST_NCOUNT], constant, filt_ambig, o);      // (min < Q: x is a query's slot)
        }
}
// bit planes of the rows flagged 1 in keep: scan, keep words, planes (every word written).  rows = how many
int skx::planes_of_kept_rows(skx_array *a, const uint8_t *keep, int filt, DevBuf<uint64_t> &planes, uint64_t &wpr, uint64_t &rows, const int *order)
{
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    const int S = (int)a->names.size(); const uint64_t U = a->n_rows;
    DevBuf<uint64_t> pos, sc_offs, kb, gp; DevBuf<uint32_t> sc_sums, fg;
    SKX_TRY(pos.alloc(U + 1)); SKX_TRY(sc_sums.alloc(scan_u8_blocks(U))); SKX_TRY(sc_offs.alloc(scan_u8_blocks(U) + 1));
    SKX_TRY(kb.alloc((U + 63) / 64)); SKX_TRY(gp.alloc((U + 63) / 64));
    launch_scan_u8(keep, pos.p, U, sc_sums.p, sc_offs.p, st);
    SKX_HIP(hipMemcpyAsync(&rows, pos.p + U, 8, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    wpr = std::max<uint64_t>((rows + 63) / 64, 1);
    SKX_TRY(planes.alloc((filt ? 4 : 8) * (uint64_t)S * wpr));
    if (!rows) { SKX_TRY(planes.zero(st)); return SKX_OK; }
    launch_keep_bits(keep, pos.p, U, kb.p, gp.p, st);
    SKX_TRY(fg.alloc(rows / 4096 + 2));
    launch_build_planes_keep(a->matrix.p, a->pitch, S, U, kb.p, gp.p, planes.p, wpr, filt, st, fg.p, rows, order);
    SKX_HIP(hipStreamSynchronize(st));            // pos / kb / gp / fg go out of scope
    return SKX_OK;
}
// the planes a sweep runs on, as build_planes leaves them: one set (p: 4 planes with filt_ambig, 8 without), or the clean / dirty split of
// --allow-ambiguous (pc: 4 planes, pd: 8)
struct SweepPlanes {
    DevBuf<uint64_t> p, pc, pd; uint64_t wpr = 1, wc = 1, wd = 1, n = 0, nc = 0, nd = 0; bool split = false;
    PlanesView view() const { return split ? PlanesView{{pc.p, wc, nc}, {pd.p, wd, nd}, true} : PlanesView{{p.p, wpr, n}, {}, false}; }
};
// --allow-ambiguous over the rows flagged in keep (nullptr: all): the twelve pair classes differ from the three of the default sweep only on rows
// that hold an ambiguous cell (the row statistics say which), so the rows without one go through the 4-plane sweep, their counts filed as classes
// 0-2, and only the others through the 8-plane, twelve-class one (merge_ska_array.rs:587-632 sums per row: any split of the rows gives the sums)
static int ambiguous_split_planes(skx_array *a, const uint8_t *keep, const int *order, SweepPlanes &sp)
{
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    const int S = (int)a->names.size(); const uint64_t U = a->n_rows;
    DevBuf<uint8_t> clean, dirty;
    SKX_TRY(clean.alloc(U)); SKX_TRY(dirty.alloc(U));
    launch_split_keep(keep, a->mask.p, U, clean.p, dirty.p, st, knob("stale_row_mask") ? 2 : 0);
    DevBuf<uint64_t> &pc = sp.pc, &pd = sp.pd; uint64_t &wc = sp.wc, &wd = sp.wd, &nc = sp.nc, &nd = sp.nd;
    sp.split = true;
    SKX_TRY(planes_of_kept_rows(a, clean.p, 1, pc, wc, nc, order));
    if (nc) {
        // the split rests on the row statistics: on a clean row every present cell is one base, i.e. plane 0 (present) == plane 1 (unambiguous).
        // Statistics that missed a code (none of the engine's operations leaves such, but the array is the caller's) show up here: all rows
        // go through the twelve-class sweep then
        DevBuf<int> d_flag; SKX_TRY(d_flag.alloc(1)); SKX_TRY(d_flag.zero(st));
        launch_differ_u32((const uint32_t *)pc.p, (const uint32_t *)(pc.p + (uint64_t)S * wc), (uint64_t)S * wc * 2, d_flag.p, st);
        int differ = 0;
        SKX_HIP(hipMemcpyAsync(&differ, d_flag.p, 4, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipStreamSynchronize(st));
        if (differ) { launch_split_keep(keep, a->mask.p, U, clean.p, dirty.p, st, 1); nc = 0; pc.release(); }
    }
    return planes_of_kept_rows(a, dirty.p, 0, pd, wd, nd, order);
}
// rows of the array -> the planes a sweep runs on; rows = how many went in.  keep (device flags, 1: the row goes in; nullptr: every row),
// order: launch_build_planes'.  With filt_ambig one set of 4 planes, without it the clean / dirty split.  No row: one zeroed word a sample,
// not split -- every count comes out zero
static int build_planes(skx_array *a, const uint8_t *keep, int filt_ambig, const int *order, SweepPlanes &sp, uint64_t &rows)
{
    hipStream_t st = a->ctx->stream;
    const int S = (int)a->names.size(); const uint64_t U = a->n_rows;
    sp = SweepPlanes();
    if (U && !filt_ambig) { SKX_TRY(ambiguous_split_planes(a, keep, order, sp)); sp.n = sp.nc + sp.nd; }
    else if (U && keep) SKX_TRY(planes_of_kept_rows(a, keep, 1, sp.p, sp.wpr, sp.n, order));
    else if (U) {                                                                     // (filt_ambig: the split took the other case)
        sp.wpr = (U + 63) / 64; sp.n = U;
        SKX_TRY(sp.p.alloc(4 * (uint64_t)S * sp.wpr));
        launch_build_planes(a->matrix.p, a->pitch, S, U, sp.p.p, sp.wpr, 1, st, order);      // (every word is written)
    }
    rows = sp.n;
    if (rows) return SKX_OK;
    sp = SweepPlanes();
    SKX_TRY(sp.p.alloc((filt_ambig ? 4 : 8) * (uint64_t)S));
    return sp.p.zero(st);
}
// the two filters of generic_modes::distance per row, in one pass over the row statistics (skx_internal.h): what entry_planes and skx_array_pair_sites read
void skx::distance_filter_flags(skx_array *a, double min_freq, uint8_t *keep, hipStream_t st)
{
    const uint64_t S_total = a->total_samples ? a->total_samples : (uint64_t)a->names.size();
    const uint64_t thr = min_freq * (double)S_total >= 1.0 ? (uint64_t)std::ceil((double)S_total * min_freq) : 0;       // generic_modes.rs:149-159
    FilterArgs fa{a->vcount.p, a->present.p, a->unambig.p, a->mask.p, a->n_rows, (uint32_t)S_total, thr, 0, SKX_FILTER_NO_CONST, 0, keep, 1};
    launch_filter_flags(fa, st);
}
// the planes of an entry point.  prefiltered: the array has been filtered already (skx_array_distance, the *_prefiltered entry points) -- every
// row is swept and *prefiltered is the constant; nullptr: the two filters of generic_modes::distance (generic_modes.rs:136-189) decide per row
// and the planes are built over the rows that stay, without touching the array; constant = rows the NoConst stage removes
static int entry_planes(skx_array *a, const double *prefiltered, double min_freq, int filt_ambig, const int *order, SweepPlanes &sp, double &constant, uint64_t &kept)
{
    hipStream_t st = a->ctx->stream;
    const uint64_t U = a->n_rows;
    if (prefiltered) { constant = *prefiltered; return build_planes(a, nullptr, filt_ambig, order, sp, kept); }
    DevBuf<uint8_t> keep; DevBuf<unsigned long long> d_c; unsigned long long n_const = 0;
    if (U) {
        SKX_TRY(keep.alloc(U)); SKX_TRY(d_c.alloc(1)); SKX_TRY(d_c.zero(st));
        distance_filter_flags(a, min_freq, keep.p, st);
        launch_count_u8(keep.p, U, 3, d_c.p, st);
        SKX_HIP(hipMemcpyAsync(&n_const, d_c.p, 8, hipMemcpyDeviceToHost, st));      // arrives with the builder's row count: it synchronises for that
    }
    const int r = build_planes(a, keep.p, filt_ambig, order, sp, kept);
    if (r != SKX_OK) (void)hipStreamSynchronize(st);                                  // (n_const is a local)
    constant = (double)n_const;
    return r;
}
// counts of the band [i_lo, i_hi) (i_lo < i_hi) over a plane set into cnt, zeroed by the caller: the filtered launch derives a count from what
// its slot held on entry (launch_pair_counts), so it comes first and there is one of it
static int sweep_band(skx_ctx *ctx, const PlanesView &v, int S, int filt_ambig, unsigned long long *cnt, int i_lo, int i_hi)
{
    const PlanesView::Set *set[2] = {&v.one, &v.dirty}; const int mode[2] = {v.split ? 2 : filt_ambig, 0};
    for (int k = 0; k < (v.split ? 2 : 1); k++)
        if (set[k]->p && set[k]->rows) SKX_HIP((hipError_t)launch_pair_counts(set[k]->p, S, set[k]->wpr, mode[k], cnt, ctx->stream, i_lo, i_hi));
    return SKX_OK;
}
int skx::planes_table(skx_ctx *ctx, const PlanesView &v, int S, int filt_ambig, double constant, int i_lo, int i_hi, skx_dist *out, const QueryPlan *qp)
{
    hipStream_t st = ctx->stream;
    if (S < 2 || i_lo >= i_hi) return SKX_OK;
    const uint64_t rows = (uint64_t)(i_hi - i_lo);
    DevBuf<unsigned long long> cnt;
    SKX_TRY(cnt.alloc(rows * S * DIST_NCOUNT)); SKX_TRY(cnt.zero(st));
    SKX_TRY(sweep_band(ctx, v, S, filt_ambig, cnt.p, i_lo, i_hi));
    std::vector<unsigned long long> h(rows * S * DIST_NCOUNT);
    SKX_HIP(hipMemcpyAsync(h.data(), cnt.p, h.size() * 8, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    SKX_HIP(hipGetLastError());
    if (qp) finish_query(h.data(), S, *qp, constant, filt_ambig, out);
    else finish_pairs(h.data(), S, i_lo, i_hi, constant, filt_ambig, out);
    return SKX_OK;
}

// the table (skx_array_distance*, skx_array_distance_query*).  prefiltered / min_freq: see entry_planes; is_query: the rows of the query form
static int array_distance(skx_array *a, const double *prefiltered, double min_freq, int filt_ambig, const int *query, int n_query, bool is_query, skx_dist *out,
                          int64_t *constant, uint64_t *rows_used)
{
    if (!a || !out) { set_error("bad arguments"); return SKX_EINVAL; }
    skx_ctx *ctx = a->ctx;
    SKX_HIP(hipSetDevice(ctx->device));
    SKX_TRY(array_materialize(a));
    const int S = (int)a->names.size();
    QueryPlan plan; const QueryPlan *qp = nullptr;
    if (is_query) { SKX_TRY(query_plan(a, query, n_query, plan)); qp = &plan; }
    if (constant) *constant = 0;
    if (rows_used) *rows_used = 0;
    if (S < 2) { if (qp) out[0] = skx_dist{}; return SKX_OK; }
    StageTimer t(ctx, &ctx->tm.distance);
    SweepPlanes sp; double c = 0; uint64_t kept = 0;
    SKX_TRY(entry_planes(a, prefiltered, min_freq, filt_ambig, qp ? qp->order.p : nullptr, sp, c, kept));
    if (constant) *constant = (int64_t)c;
    if (rows_used) *rows_used = kept;
    return planes_table(ctx, sp.view(), S, filt_ambig, c, 0, qp ? qp->Q() : S, out, qp);
}
extern "C" int skx_array_distance(skx_array *a, double constant, int filt_ambig, skx_dist *out)
{
    return skx_guarded([&]() -> int { return array_distance(a, &constant, 0.0, filt_ambig, nullptr, 0, false, out, nullptr, nullptr); });
}
extern "C" int skx_array_distance_query(skx_array *a, double constant, int filt_ambig, const int *query, int n_query, skx_dist *out)
{
    return skx_guarded([&]() -> int { return array_distance(a, &constant, 0.0, filt_ambig, query, n_query, true, out, nullptr, nullptr); });
}
extern "C" int skx_array_distance_filtered(skx_array *a, double min_freq, int filt_ambig, skx_dist *out, int64_t *constant, uint64_t *rows_used)
{
    return skx_guarded([&]() -> int { return array_distance(a, nullptr, min_freq, filt_ambig, nullptr, 0, false, out, constant, rows_used); });
}
extern "C" int skx_array_distance_query_filtered(skx_array *a, double min_freq, int filt_ambig, const int *query, int n_query, skx_dist *out, int64_t *constant,
                                                 uint64_t *rows_used)
{
    return skx_guarded([&]() -> int { return array_distance(a, nullptr, min_freq, filt_ambig, query, n_query, true, out, constant, rows_used); });
}

// ---- the line selection (skx_array_distance_select): the same planes as the table's, the pair sweep band by band over the pair matrix, and
// after every band the selection kernels of skx_select.hip on its count buffer -- only the candidates' integers come back to the host, which
// finishes them with finish_counts, i.e. with the table's own arithmetic.
// the largest key whose distance, by finish_counts' own expression, is <= max_snps (>= 0): a floor, then a step either way against that expression
static unsigned long long select_kmax(double max_snps, int filt_ambig)
{
    const double scaled = max_snps * (filt_ambig ? 1.0 : 36.0);
    if (!(scaled < 4e18)) return 1ull << 62;                               // (no key reaches it; also +inf)
    unsigned long long k = (unsigned long long)std::floor(scaled);
    while (key_distance(k + 1, filt_ambig) <= max_snps) k++;
    while (k > 0 && key_distance(k, filt_ambig) > max_snps) k--;
    return k;
}
// first samples of the pair matrix swept at a time: as asked, or the largest multiple of 64 whose count buffer stays within 1 GiB, at least 64
static uint64_t banded_rows(int32_t asked, int S)
{
    uint64_t band = (uint64_t)asked;
    if (!band) band = std::max<uint64_t>(64, ((1ull << 30) / ((uint64_t)S * DIST_NCOUNT * 8)) / 64 * 64);
    return std::min<uint64_t>(band, (uint64_t)S);
}
// the band loop: cnt (band x S pairs) zeroed and swept for every band [lo, hi) in turn, then handed to consume(lo, hi) on the context's stream
template <typename F>
static int for_each_band(skx_ctx *ctx, const PlanesView &v, int S, int filt_ambig, DevBuf<unsigned long long> &cnt, uint64_t band, F &&consume)
{
    for (uint64_t lo = 0; lo < (uint64_t)S; lo += band) {
        const int hi = (int)std::min<uint64_t>((uint64_t)S, lo + band);
        SKX_TRY(cnt.zero(ctx->stream));
        SKX_TRY(sweep_band(ctx, v, S, filt_ambig, cnt.p, (int)lo, hi));
        SKX_TRY(consume((int)lo, hi));
    }
    return SKX_OK;
}
// prefiltered / min_freq: see entry_planes
static int array_distance_select(skx_array *a, const double *prefiltered, double min_freq, int filt_ambig, const skx_select_spec *spec, skx_dist_pair **pairs,
                                 uint64_t *n_pairs, int64_t *constant, uint64_t *rows_used, skx_select_info *info)
{
    if (!a || !spec || !pairs || !n_pairs) { set_error("distance select: bad arguments"); return SKX_EINVAL; }
    *pairs = nullptr; *n_pairs = 0;
    if (constant) *constant = 0;
    if (rows_used) *rows_used = 0;
    if (info) *info = skx_select_info{0, 0, 0, 0};
    const int S = (int)a->names.size();
    if (std::isnan(spec->max_snps) || std::isnan(spec->max_mismatches)) { set_error("distance select: a threshold is not a number"); return SKX_EINVAL; }
    if (spec->max_mismatches > 1.0) { set_error("distance select: max_mismatches is a proportion, at most 1"); return SKX_EINVAL; }
    if (spec->closest < 0) { set_error("distance select: closest must be zero (none) or more"); return SKX_EINVAL; }
    if (spec->band_rows < 0) { set_error("distance select: band_rows must be zero (the engine's choice) or more"); return SKX_EINVAL; }
    if (spec->max_snps < 0.0 && spec->max_mismatches < 0.0 && spec->closest == 0) {
        set_error("distance select: none of max_snps, max_mismatches and closest is given"); return SKX_EINVAL;
    }
    const bool nearest = spec->closest > 0 && (int64_t)spec->closest < (int64_t)S - 1;        // K >= S - 1: every candidate is among the nearest
    if (nearest && (uint32_t)spec->closest > SEL_MAX_K) {
        set_error("distance select: closest %d is above the %u a sample's list holds (and below the %d that would keep every pair)", spec->closest, SEL_MAX_K, S - 1);
        return SKX_EINVAL;
    }
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    SKX_TRY(array_materialize(a));
    if (S < 2) return SKX_OK;
    StageTimer t(ctx, &ctx->tm.distance);
    SweepPlanes sp; uint64_t kept = 0; double n_const = 0;
    SKX_TRY(entry_planes(a, prefiltered, min_freq, filt_ambig, nullptr, sp, n_const, kept));
    if (constant) *constant = (int64_t)n_const;
    if (rows_used) *rows_used = kept;
    // a --closest list orders by (key, partner) in one 64-bit word: the key, at most 36 per swept row, must stay below 2^32
    if (nearest && kept >= (1ull << 32) / 36) { set_error("distance select: closest is not available above %llu rows", (1ull << 32) / 36); return SKX_EUNSUP; }
    const SelCriteria crit{filt_ambig, n_const, spec->max_snps < 0.0 ? ~0ull : select_kmax(spec->max_snps, filt_ambig), spec->max_mismatches < 0.0 ? -1.0 : spec->max_mismatches};
    const uint64_t band = banded_rows(spec->band_rows, S);
    const uint64_t bands = ((uint64_t)S + band - 1) / band;
    DevBuf<unsigned long long> cnt;
    SKX_TRY(cnt.alloc(band * S * DIST_NCOUNT));
    std::vector<SelRecord> rec;
    unsigned long long candidates = 0;
    if (!nearest) {
        DevBuf<uint32_t> d_n; DevBuf<uint64_t> d_off; DevBuf<SelRecord> d_rec;
        SKX_TRY(d_n.alloc(band)); SKX_TRY(d_off.alloc(band + 1));
        std::vector<uint32_t> h_n(band); std::vector<uint64_t> h_off(band + 1);
        SKX_TRY(for_each_band(ctx, sp.view(), S, filt_ambig, cnt, band, [&](int lo, int hi) -> int {
            const int rows = hi - lo;
            launch_select_count(cnt.p, S, lo, hi, crit, d_n.p, st);
            SKX_HIP(hipMemcpyAsync(h_n.data(), d_n.p, (size_t)rows * 4, hipMemcpyDeviceToHost, st));
            SKX_HIP(hipStreamSynchronize(st));
            h_off[0] = 0;
            for (int r = 0; r < rows; r++) h_off[r + 1] = h_off[r] + h_n[r];
            const uint64_t n = h_off[rows];
            if (!n) return SKX_OK;
            if (d_rec.n < n) SKX_TRY(d_rec.alloc(n));
            SKX_HIP(hipMemcpyAsync(d_off.p, h_off.data(), (size_t)(rows + 1) * 8, hipMemcpyHostToDevice, st));
            launch_select_write(cnt.p, S, lo, hi, crit, d_off.p, d_rec.p, st);
            const size_t at = rec.size();
            rec.resize(at + n);
            SKX_HIP(hipMemcpyAsync(rec.data() + at, d_rec.p, n * sizeof(SelRecord), hipMemcpyDeviceToHost, st));
            SKX_HIP(hipStreamSynchronize(st));                                  // (h_off is reused by the next band)
            return SKX_OK;
        }));
        SKX_HIP(hipGetLastError());
        candidates = rec.size();
    } else {
        const uint32_t K = (uint32_t)spec->closest;
        DevBuf<SelNear> lists; DevBuf<unsigned long long> d_cand;
        SKX_TRY(lists.alloc((uint64_t)S * K)); SKX_TRY(d_cand.alloc(1)); SKX_TRY(d_cand.zero(st));
        SKX_HIP(hipMemsetAsync(lists.p, 0xFF, (uint64_t)S * K * sizeof(SelNear), st));          // every place unused
        SKX_TRY(for_each_band(ctx, sp.view(), S, filt_ambig, cnt, band, [&](int lo, int hi) -> int {
            launch_select_nearest(cnt.p, S, lo, hi, crit, K, lists.p, d_cand.p, st);
            return SKX_OK;
        }));
        std::vector<SelNear> h_lists((uint64_t)S * K);
        SKX_HIP(hipMemcpyAsync(h_lists.data(), lists.p, h_lists.size() * sizeof(SelNear), hipMemcpyDeviceToHost, st));
        SKX_HIP(hipMemcpyAsync(&candidates, d_cand.p, 8, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipStreamSynchronize(st));
        SKX_HIP(hipGetLastError());
        // the union of the lists as (min, max) pairs, each once, in the table's order
        for (int s = 0; s < S; s++)
            for (uint32_t e = 0; e < K; e++) {
                const SelNear &x = h_lists[(uint64_t)s * K + e];
                if (x.sort_key == ~0ull) break;                                   // (the used places come first)
                const uint32_t partner = (uint32_t)x.sort_key;
                rec.push_back(SelRecord{std::min((uint32_t)s, partner), std::max((uint32_t)s, partner), x.mism, x.m, x.key});
            }
        std::sort(rec.begin(), rec.end(), [](const SelRecord &x, const SelRecord &y) { return x.i != y.i ? x.i < y.i : x.j < y.j; });
        rec.erase(std::unique(rec.begin(), rec.end(), [](const SelRecord &x, const SelRecord &y) { return x.i == y.i && x.j == y.j; }), rec.end());
    }
    skx_dist_pair *out = (skx_dist_pair *)malloc(std::max<size_t>(rec.size(), 1) * sizeof(skx_dist_pair));
    if (!out) { set_error("out of host memory"); return SKX_ENOMEM; }
    for (size_t n = 0; n < rec.size(); n++) {
        out[n].i = rec[n].i; out[n].j = rec[n].j;
        finish_counts(rec[n].mism, rec[n].m, rec[n].key, n_const, filt_ambig, out[n].d);
    }
    *pairs = out; *n_pairs = rec.size();
    if (info) *info = skx_select_info{bands, band, band * (uint64_t)S * DIST_NCOUNT * 8, candidates};
    return SKX_OK;
}
extern "C" int skx_array_distance_select(skx_array *a, double min_freq, int filt_ambig, const skx_select_spec *spec, skx_dist_pair **pairs, uint64_t *n_pairs,
                                         int64_t *constant, uint64_t *rows_used, skx_select_info *info)
{
    return skx_guarded([&]() -> int { return array_distance_select(a, nullptr, min_freq, filt_ambig, spec, pairs, n_pairs, constant, rows_used, info); });
}
extern "C" int skx_array_distance_select_prefiltered(skx_array *a, int64_t constant, int filt_ambig, const skx_select_spec *spec, skx_dist_pair **pairs,
                                                     uint64_t *n_pairs, skx_select_info *info)
{
    return skx_guarded([&]() -> int {
    if (constant < 0) { set_error("distance select: constant must be zero or more"); return SKX_EINVAL; }
    const double c = (double)constant;
    return array_distance_select(a, &c, 0.0, filt_ambig, spec, pairs, n_pairs, nullptr, nullptr, info);
    });
}

// ---- `ska distance --mst` (skx_array_distance_mst): the selection's planes and band loop, and after every band the kernels of skx_mst.hip on its
// count buffer -- the forest of the bands so far stays on the device (two buffers of S records, labels, a word per component), a band merges its
// candidates into it by Boruvka rounds, and after the last band at most S - 1 records come back, to be finished as the selection's are.
// Between rounds the host reads one word back, the new forest's length: a round that adds nothing ends the band (and S - 1 records end it at
// once), so a band costs one small copy and wait per round, at most ceil(log2 S) + 2 of them, against a sweep of band x S pairs.
// prefiltered / min_freq: see entry_planes
static int array_distance_mst(skx_array *a, const double *prefiltered, double min_freq, int filt_ambig, const skx_mst_spec *spec, skx_dist_pair **pairs, uint64_t *n_pairs,
                              int64_t *constant, uint64_t *rows_used, skx_mst_info *info)
{
    if (!a || !spec || !pairs || !n_pairs) { set_error("distance mst: bad arguments"); return SKX_EINVAL; }
    *pairs = nullptr; *n_pairs = 0;
    if (constant) *constant = 0;
    if (rows_used) *rows_used = 0;
    if (info) *info = skx_mst_info{0, 0, 0, 0, 0, 0, 0};
    const int S = (int)a->names.size();
    if (std::isnan(spec->max_snps) || std::isnan(spec->max_mismatches)) { set_error("distance mst: a threshold is not a number"); return SKX_EINVAL; }
    if (spec->max_mismatches > 1.0) { set_error("distance mst: max_mismatches is a proportion, at most 1"); return SKX_EINVAL; }
    if (spec->band_rows < 0) { set_error("distance mst: band_rows must be zero (the engine's choice) or more"); return SKX_EINVAL; }
    // an edge is ordered by (key, i, j) in one 64-bit word, 16 bits a sample
    if (S > MST_MAX_SAMPLES) { set_error("distance mst: not available above %d samples (the array has %d)", MST_MAX_SAMPLES, S); return SKX_EUNSUP; }
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    SKX_TRY(array_materialize(a));
    if (S < 2) { if (info) info->components = (uint64_t)S; return SKX_OK; }
    StageTimer t(ctx, &ctx->tm.distance);
    SweepPlanes sp; uint64_t kept = 0; double n_const = 0;
    SKX_TRY(entry_planes(a, prefiltered, min_freq, filt_ambig, nullptr, sp, n_const, kept));
    if (constant) *constant = (int64_t)n_const;
    if (rows_used) *rows_used = kept;
    // the key, at most 36 per swept row, must stay below 2^32 (the rule of --closest)
    if (kept >= (1ull << 32) / 36) { set_error("distance mst: not available above %llu rows", (1ull << 32) / 36); return SKX_EUNSUP; }
    const SelCriteria crit{filt_ambig, n_const, spec->max_snps < 0.0 ? ~0ull : select_kmax(spec->max_snps, filt_ambig), spec->max_mismatches < 0.0 ? -1.0 : spec->max_mismatches};
    const uint64_t band = banded_rows(spec->band_rows, S);
    const uint64_t bands = ((uint64_t)S + band - 1) / band;
    DevBuf<unsigned long long> cnt, words, best, d_cand; DevBuf<uint32_t> comp, parent, d_n; DevBuf<SelRecord> forest[2];
    SKX_TRY(cnt.alloc(band * S * DIST_NCOUNT)); SKX_TRY(words.alloc(band * S));
    SKX_TRY(best.alloc((uint64_t)S)); SKX_TRY(comp.alloc((uint64_t)S)); SKX_TRY(parent.alloc((uint64_t)S));
    SKX_TRY(forest[0].alloc((uint64_t)S)); SKX_TRY(forest[1].alloc((uint64_t)S));
    SKX_TRY(d_n.alloc(1)); SKX_TRY(d_cand.alloc(1)); SKX_TRY(d_cand.zero(st));
    int max_rounds = 1;                                                          // ceil(log2 S) + 1: every round that chooses at least halves the trees that still have an edge out
    while ((1ll << (max_rounds - 1)) < (long long)S) max_rounds++;
    uint32_t n_forest = 0; int cur = 0; uint64_t most_rounds = 0;
    SKX_TRY(for_each_band(ctx, sp.view(), S, filt_ambig, cnt, band, [&](int lo, int hi) -> int {
        SelRecord *old_f = forest[cur].p, *new_f = forest[cur ^ 1].p;
        launch_mst_begin(comp.p, parent.p, best.p, S, st);
        launch_mst_gather(cnt.p, S, lo, hi, crit, words.p, d_cand.p, st);
        SKX_TRY(d_n.zero(st));
        uint32_t n_new = 0; uint64_t rounds = 0;
        for (int r = 0; n_new < (uint32_t)S - 1; r++) {
            if (r > max_rounds) { set_error("distance mst: a band took more than %d rounds", max_rounds); return SKX_ENODEV; }
            launch_mst_round(words.p, S, lo, hi, old_f, n_forest, comp.p, best.p, parent.p, new_f, (uint32_t)S, d_n.p, st);
            uint32_t n_now = 0;
            SKX_HIP(hipMemcpyAsync(&n_now, d_n.p, 4, hipMemcpyDeviceToHost, st));
            SKX_HIP(hipStreamSynchronize(st));
            if (n_now > (uint32_t)S - 1) { set_error("distance mst: %u lines in a forest of %d samples", n_now, S); return SKX_ENODEV; }
            if (n_now == n_new) break;                                           // no component has an edge out
            n_new = n_now; rounds++;
            launch_mst_relabel(comp.p, parent.p, best.p, S, st);
        }
        launch_mst_finish(cnt.p, S, lo, hi, filt_ambig, new_f, n_new, st);
        n_forest = n_new; cur ^= 1;
        most_rounds = std::max(most_rounds, rounds);
        return SKX_OK;
    }));
    std::vector<SelRecord> rec(n_forest);
    unsigned long long candidates = 0;
    if (n_forest) SKX_HIP(hipMemcpyAsync(rec.data(), forest[cur].p, (size_t)n_forest * sizeof(SelRecord), hipMemcpyDeviceToHost, st));
    SKX_HIP(hipMemcpyAsync(&candidates, d_cand.p, 8, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    SKX_HIP(hipGetLastError());
    std::sort(rec.begin(), rec.end(), [](const SelRecord &x, const SelRecord &y) { return x.i != y.i ? x.i < y.i : x.j < y.j; });
    skx_dist_pair *out = (skx_dist_pair *)malloc(std::max<size_t>(rec.size(), 1) * sizeof(skx_dist_pair));
    if (!out) { set_error("out of host memory"); return SKX_ENOMEM; }
    for (size_t n = 0; n < rec.size(); n++) {
        out[n].i = rec[n].i; out[n].j = rec[n].j;
        finish_counts(rec[n].mism, rec[n].m, rec[n].key, n_const, filt_ambig, out[n].d);
    }
    *pairs = out; *n_pairs = rec.size();
    if (info) *info = skx_mst_info{bands, band, band * (uint64_t)S * DIST_NCOUNT * 8, candidates, (uint64_t)rec.size(), (uint64_t)S - rec.size(), most_rounds};
    return SKX_OK;
}
extern "C" int skx_array_distance_mst(skx_array *a, double min_freq, int filt_ambig, const skx_mst_spec *spec, skx_dist_pair **pairs, uint64_t *n_pairs,
                                      int64_t *constant, uint64_t *rows_used, skx_mst_info *info)
{
    return skx_guarded([&]() -> int { return array_distance_mst(a, nullptr, min_freq, filt_ambig, spec, pairs, n_pairs, constant, rows_used, info); });
}
extern "C" int skx_array_distance_mst_prefiltered(skx_array *a, int64_t constant, int filt_ambig, const skx_mst_spec *spec, skx_dist_pair **pairs, uint64_t *n_pairs,
                                                  skx_mst_info *info)
{
    return skx_guarded([&]() -> int {
    if (constant < 0) { set_error("distance mst: constant must be zero or more"); return SKX_EINVAL; }
    const double c = (double)constant;
    return array_distance_mst(a, &c, 0.0, filt_ambig, spec, pairs, n_pairs, nullptr, nullptr, info);
    });
}

// ---- `ska distance --no-table` (skx_array_distance_banded): the selection's planes and band loop, and after every band the consumers of
// skx_banded.hip on its count buffer -- the union-find of the clusters and the neighbour-joining matrix stay on the device from the first band
// to the last, S labels and S - 1 join records come back.
// The clusters' thresholds are on the table's PRINTED values (skh_distance_clusters: strtod of "%.2f" / "%.5f").  Rounding to a fixed number of
// decimals is monotone, so each rule is a down-set with a largest member: kmax among the integer keys, pmax among the doubles of [0, 1].  Both
// are found by bisection against the very expressions (key_distance, snprintf, strtod); the device then compares key <= kmax and p <= pmax.
static bool printed_passes(const char *fmt, double v, double threshold)
{
    char tmp[512];
    snprintf(tmp, sizeof tmp, fmt, v);
    return strtod(tmp, nullptr) <= threshold;
}
extern "C" int skh_cluster_cutoffs(double max_snps, double max_mismatches, int filt_ambig, uint64_t *kmax, double *pmax)
{
    if (!kmax || !pmax) { set_error("skh_cluster_cutoffs: bad arguments"); return SKX_EINVAL; }
    if (std::isnan(max_snps) || std::isnan(max_mismatches) || max_snps < 0.0 || max_mismatches < 0.0) {
        set_error("skh_cluster_cutoffs: a threshold is not a number or negative"); return SKX_EINVAL;
    }
    // key 0 prints 0.00 and p = 0 prints 0.00000: both pass every threshold >= 0, so the bisections start from a member
    unsigned long long k_in = 0, k_out = 1ull << 62;                         // (no key reaches 2^62: at most 36 per swept row)
    if (printed_passes("%.2f", key_distance(k_out, filt_ambig), max_snps)) k_in = k_out;
    else while (k_out - k_in > 1) {
        const unsigned long long mid = k_in + (k_out - k_in) / 2;
        (printed_passes("%.2f", key_distance(mid, filt_ambig), max_snps) ? k_in : k_out) = mid;
    }
    // non-negative doubles are ordered as their bit patterns
    auto of_bits = [](uint64_t b) { double d; memcpy(&d, &b, 8); return d; };
    uint64_t p_in = 0, p_out = 0x3FF0000000000000ull;                          // 0.0, 1.0
    if (printed_passes("%.5f", 1.0, max_mismatches)) p_in = p_out;
    else while (p_out - p_in > 1) {
        const uint64_t mid = p_in + (p_out - p_in) / 2;
        (printed_passes("%.5f", of_bits(mid), max_mismatches) ? p_in : p_out) = mid;
    }
    *kmax = k_in; *pmax = of_bits(p_in);
    return SKX_OK;
}
// prefiltered / min_freq: see entry_planes
static int array_distance_banded(skx_array *a, const double *prefiltered, double min_freq, int filt_ambig, const skx_banded_spec *spec, uint32_t *labels,
                                 skx_nj_join *joins, int64_t *constant, uint64_t *rows_used, skx_banded_info *info)
{
    if (!a || !spec) { set_error("distance banded: bad arguments"); return SKX_EINVAL; }
    if (constant) *constant = 0;
    if (rows_used) *rows_used = 0;
    if (info) *info = skx_banded_info{0, 0, 0, 0, 0};
    if (!labels && !joins) { set_error("distance banded: neither the labels nor the joins are asked for"); return SKX_EINVAL; }
    if (labels && (std::isnan(spec->cluster_snps) || std::isnan(spec->cluster_mismatches) || spec->cluster_snps < 0.0 || spec->cluster_mismatches < 0.0)) {
        set_error("distance banded: a cluster threshold is not a number or negative"); return SKX_EINVAL;
    }
    if (spec->band_rows < 0) { set_error("distance banded: band_rows must be zero (the engine's choice) or more"); return SKX_EINVAL; }
    const int S = (int)a->names.size();
    if (joins) SKX_TRY(nj_check_n(S));
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    SKX_TRY(array_materialize(a));
    if (S < 2) {                                                              // (labels only: the joins need two samples)
        for (int i = 0; i < S; i++) labels[i] = (uint32_t)i;
        if (info) info->clusters = (uint64_t)S;
        return SKX_OK;
    }
    std::optional<StageTimer> t(std::in_place, ctx, &ctx->tm.distance);
    PhaseTimer tp("distance.pair_sweep");                                     // what the table's phase of that name covers: planes, sweep, and here the consumers
    SweepPlanes sp; uint64_t kept = 0; double n_const = 0;
    SKX_TRY(entry_planes(a, prefiltered, min_freq, filt_ambig, nullptr, sp, n_const, kept));
    if (constant) *constant = (int64_t)n_const;
    if (rows_used) *rows_used = kept;
    SelCriteria crit{filt_ambig, n_const, 0, 0.0};
    if (labels) { uint64_t kmax = 0; SKX_TRY(skh_cluster_cutoffs(spec->cluster_snps, spec->cluster_mismatches, filt_ambig, &kmax, &crit.pmax)); crit.kmax = kmax; }
    const uint64_t band = banded_rows(spec->band_rows, S);
    const uint64_t bands = ((uint64_t)S + band - 1) / band, cnt_bytes = band * (uint64_t)S * DIST_NCOUNT * 8, pitch = nj_pitch((uint64_t)S);
    // everything is allocated before the first band: a matrix that does not fit is refused here, with its message
    if (joins) SKX_TRY(nj_fits(ctx, (uint64_t)S, cnt_bytes));
    DevBuf<unsigned long long> cnt, d_n; DevBuf<double> D; DevBuf<uint32_t> parent, d_label;
    SKX_TRY(cnt.alloc(band * S * DIST_NCOUNT));
    if (joins) { SKX_TRY(D.alloc(pitch * S)); SKX_TRY(D.zero(st)); }         // (the diagonal and the pad column of an odd S stay zero)
    unsigned long long h_n[2] = {0, 0};                                       // edges, roots
    const bool per_edge = knob("union_per_edge") != 0;                        // (the plain union, for the comparison)
    if (labels) {
        SKX_TRY(parent.alloc((uint64_t)S)); SKX_TRY(d_label.alloc((uint64_t)S)); SKX_TRY(d_n.alloc(2)); SKX_TRY(d_n.zero(st));
        launch_cluster_init(parent.p, S, st);
    }
    SKX_TRY(for_each_band(ctx, sp.view(), S, filt_ambig, cnt, band, [&](int lo, int hi) -> int {
        if (labels) launch_cluster_union(cnt.p, S, lo, hi, crit, parent.p, d_n.p, per_edge, st);
        if (joins) launch_dist_fill(cnt.p, S, lo, hi, filt_ambig, D.p, pitch, st);
        return SKX_OK;
    }));
    if (labels) {
        launch_cluster_labels(parent.p, S, d_label.p, d_n.p + 1, st);
        SKX_HIP(hipMemcpyAsync(labels, d_label.p, (size_t)S * 4, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipMemcpyAsync(h_n, d_n.p, sizeof h_n, hipMemcpyDeviceToHost, st));
    }
    SKX_HIP(hipGetLastError());
    SKX_HIP(hipStreamSynchronize(st));
    tp.stop(); t.reset();
    cnt.release(); sp = SweepPlanes();                                        // (the joins need the matrix only)
    if (joins) { PhaseTimer tn("distance.nj"); SKX_TRY(nj_run_device(ctx, D, pitch, (uint32_t)S, joins)); }
    if (info) *info = skx_banded_info{bands, band, cnt_bytes, h_n[0], h_n[1]};
    return SKX_OK;
}
extern "C" int skx_array_distance_banded(skx_array *a, double min_freq, int filt_ambig, const skx_banded_spec *spec, uint32_t *labels, skx_nj_join *joins,
                                         int64_t *constant, uint64_t *rows_used, skx_banded_info *info)
{
    return skx_guarded([&]() -> int { return array_distance_banded(a, nullptr, min_freq, filt_ambig, spec, labels, joins, constant, rows_used, info); });
}
extern "C" int skx_array_distance_banded_prefiltered(skx_array *a, int64_t constant, int filt_ambig, const skx_banded_spec *spec, uint32_t *labels,
                                                     skx_nj_join *joins, skx_banded_info *info)
{
    return skx_guarded([&]() -> int {
    if (constant < 0) { set_error("distance banded: constant must be zero or more"); return SKX_EINVAL; }
    const double c = (double)constant;
    return array_distance_banded(a, &c, 0.0, filt_ambig, spec, labels, joins, nullptr, nullptr, info);
    });
}

extern "C" int skx_array_distance_planes(skx_array *a, int filt_ambig, const void **planes, uint64_t *words_per_row, int *n_planes)
{
    return skx_guarded([&]() -> int {
    if (!a || !planes || !words_per_row) { set_error("bad arguments"); return SKX_EINVAL; }
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    SKX_TRY(array_materialize(a));
    const int S = (int)a->names.size(); const uint64_t U = a->n_rows;
    const uint64_t wpr = std::max<uint64_t>((U + 63) / 64, 1);
    const int np = filt_ambig ? 4 : 8;
    SKX_TRY(a->planes.alloc((uint64_t)np * S * wpr));
    if (U == 0) SKX_TRY(a->planes.zero(st));
    launch_build_planes(a->matrix.p, a->pitch, S, U, a->planes.p, wpr, filt_ambig, st);
    SKX_HIP(hipStreamSynchronize(st));
    SKX_HIP(hipGetLastError());
    *planes = a->planes.p; *words_per_row = wpr; if (n_planes) *n_planes = np;
    return SKX_OK;
    });
}
extern "C" int skx_planes_distance(skx_ctx *ctx, const void *planes, int n_samples, uint64_t words_per_row, int filt_ambig, double constant,
                                   int i_lo, int i_hi, skx_dist *out)
{
    return skx_guarded([&]() -> int {
    if (!ctx || !planes || !out || n_samples < 0 || i_lo < 0 || i_hi > n_samples) { set_error("bad arguments"); return SKX_EINVAL; }
    SKX_HIP(hipSetDevice(ctx->device));
    StageTimer t(ctx, &ctx->tm.distance);
    const PlanesView v{{(const uint64_t *)planes, words_per_row, words_per_row * 64}, {}, false};      // (rows: all the caller says is how many words)
    return planes_table(ctx, v, n_samples, filt_ambig, constant, i_lo, i_hi, out);
    });
}
