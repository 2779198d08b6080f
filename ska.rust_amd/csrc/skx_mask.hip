// skx_mask.hip -- `ska mask`: regions of a reference taken out of an array, per sample or for every sample (skx_array_mask_regions, include/skx.h;
// definition there and in tests/mask_model.py).  The reference has no counterpart: `ska weed` removes split k-mers by sequence, never by position
// and never per sample.
//
// The windows, their look-up and the repeat flags are `ska map`'s (RefLookup, skx_internal.h), the sites `ska density`'s: a repeated window is no
// site, so a row is the row of at most one site.  Masked cells are sparse (some hundred regions in a thousand samples x five million rows), so
// the matrix is not streamed to find them:
//   mask_sites_kernel    per hit window, in reference order: its position in the concatenated reference, its row, and whether it is a site;
//                        two order-keeping selections (prim_select_u32) leave the sites' positions xs[N] (ascending) and rows site_row[N]
//   mask_bounds_kernel   per merged interval [x0, x1] (the host merges per (sample, chromosome) and sorts): lo = the first site at or after x0,
//                        len = the sites up to x1, by two binary searches.  The host scans the lengths in 64 bits: the items
//   mask_items_kernel    a workgroup takes SKX_MASK_CHUNK consecutive items, a thread every 256th of them; an item finds its interval in the
//                        scan (a bounded binary search) and from it its sample and its row.
//                          <true>   ALL intervals: keep[row] = 0, no cell is read
//                          <false>  per-sample intervals, launched after the first: a row still kept counts for the sample; a present cell
//                                   becomes '-', vcount[row] drops by one (a 32-bit atomic), keep[row] = 2 notes that the row lost a cell.  The
//                                   sample's two counts are summed over the wave when all of its items are one sample's (consecutive items are
//                                   mostly of one interval), else added per lane
//                        The intervals are merged per sample and a row is the row of one site, so no (row, sample) is visited twice: no cell is
//                        stored by two threads and no count is lowered twice.  keep[row] = 2 may be stored by several threads: the same byte
//   launch_col_stats     only when a cell was masked: present / unambig / mask of every row again from the cells (one read of the matrix;
//                        the set of letters of a row cannot be lowered by an atomic)
//   mask_verdict_kernel  keep[r] = 0 where a row that lost a cell has no present cell left (rows_emptied), else 1 unless an ALL interval took it
// and skx_array_weed's path (array_keep_rows: scan, compaction of matrix, keys, counts and statistics) does the rest.
//
// Integer atomics only, no floats, no sort inside a kernel.  No workgroup waits for another, every loop is bounded (four items a thread, 32 steps
// of a binary search), no kernel holds a barrier, and every store is a plain vector store.
//
// Device memory beside the array: `ska map`'s window buffers and the repeat sort's (as `ska density`), 9 bytes a hit window, 8 bytes a site,
// 24 bytes a merged interval, 16 bytes a sample, one byte a row, and the compaction's second matrix when a row goes.
#include "skx_internal.h"
#include "skx_cells.h"
#include <algorithm>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

namespace skx {
namespace {

constexpr uint32_t MK_CHUNK = SKX_MASK_CHUNK;
static_assert(MK_CHUNK % 256 == 0 && MK_CHUNK >= 256, "a workgroup of 256 threads strides over a chunk");
static_assert(sizeof(skx_mask_sample) == 2 * sizeof(uint64_t) && sizeof(skx_mask_interval) == 16, "the device writes the first, the callers lay out the second");

// per hit window m (reference order): position in the concatenated reference (density_rows_kernel's xcat), row, and whether it is a site
__global__ __launch_bounds__(256) void mask_sites_kernel(const uint32_t *mapped, const uint32_t *row, const uint8_t *rep, uint32_t h, const uint64_t *cstart, uint32_t n_chrom,
                                                        uint64_t M, uint32_t *x_all, uint32_t *row_all, uint8_t *is_site)
{
    const uint64_t m = blockIdx.x * 256ull + threadIdx.x;
    if (m >= M) return;
    const uint32_t p = mapped[m];
    const uint64_t mid = (uint64_t)p - h;
    x_all[m] = (uint32_t)(mid - chrom_of(cstart, n_chrom, mid));
    row_all[m] = row[p];
    is_site[m] = rep[p] ? 0 : 1;
}

// interval i = positions [x0[i], x1[i]] of the concatenated reference: lo[i] = the first site at or after x0, len[i] = the sites up to x1
__global__ __launch_bounds__(256) void mask_bounds_kernel(const uint32_t *xs, uint64_t N, const uint32_t *x0, const uint32_t *x1, uint64_t n_iv, uint32_t *lo, uint32_t *len)
{
    const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= n_iv) return;
    uint64_t a = 0, b = N;
    const uint32_t v0 = x0[i], v1 = x1[i];
    while (a < b) { const uint64_t mid = (a + b) >> 1; if (xs[mid] < v0) a = mid + 1; else b = mid; }      // (N < 2^32: at most 32 steps)
    const uint64_t first = a;
    b = N;
    while (a < b) { const uint64_t mid = (a + b) >> 1; if (xs[mid] <= v1) a = mid + 1; else b = mid; }
    lo[i] = (uint32_t)first; len[i] = (uint32_t)(a - first);
}

struct MaskArgs {
    const uint32_t *iv_sample, *iv_lo; const uint64_t *iv_off; uint32_t n_iv;      // off[n_iv + 1]: the exclusive scan of the lengths
    uint64_t total;                                                                 // = off[n_iv]
    const uint32_t *site_row; uint64_t N;
    uint8_t *matrix; uint64_t pitch, U; uint32_t S;
    uint32_t *vcount; uint8_t *keep;
    unsigned long long *counts;                                                     // [S][2] in the order of skx_mask_sample
};

template <bool ALL>
__global__ __launch_bounds__(256) void mask_items_kernel(MaskArgs a)
{
    const uint64_t base = (uint64_t)blockIdx.x * MK_CHUNK;
    for (uint32_t j = threadIdx.x; j < MK_CHUNK; j += 256) {         // (the same trip count for every lane: the ballots below are whole waves')
        const uint64_t item = base + j;
        bool in = false, masked = false; uint32_t s = 0;
        if (item < a.total) {
            uint32_t lo = 0, hi = a.n_iv;                               // the last interval that starts at or before the item: never an empty one
            while (hi - lo > 1) { const uint32_t c = (lo + hi) >> 1; if (a.iv_off[c] <= item) lo = c; else hi = c; }
            const uint64_t at = (uint64_t)a.iv_lo[lo] + (item - a.iv_off[lo]);
            const uint32_t r = at < a.N ? a.site_row[at] : 0xFFFFFFFFu;                     // (the bounds were searched in this list: never false)
            if (r < a.U) {
                if (ALL) a.keep[r] = 0;
                else {
                    s = a.iv_sample[lo];
                    if (s < a.S && a.keep[r]) {                         // (the host checked the samples; the ALL launch has finished)
                        in = true;
                        uint8_t *cell = a.matrix + (uint64_t)s * a.pitch + r;
                        const uint8_t b = *cell;
                        if (b != 0 && b != '-') {
                            masked = true;
                            *cell = '-';
                            atomicSub(a.vcount + r, 1u);
                            a.keep[r] = 2;
                        }
                    }
                }
            }
        }
        if (ALL) continue;
        const unsigned long long im = __ballot(in), mm = __ballot(masked);
        if (!im) continue;                                              // (a whole wave's decision)
        const uint32_t lane = threadIdx.x & 63u;
        const uint32_t s_first = (uint32_t)__shfl((int)s, __ffsll((long long)im) - 1, 64);
        const bool one = __all(!in || s == s_first);
        if (one) {
            if (lane == 0) {
                atomicAdd(a.counts + (uint64_t)s_first * 2, (unsigned long long)__popcll(im));
                if (mm) atomicAdd(a.counts + (uint64_t)s_first * 2 + 1, (unsigned long long)__popcll(mm));
            }
        } else if (in) {
            atomicAdd(a.counts + (uint64_t)s * 2, 1ull);
            if (masked) atomicAdd(a.counts + (uint64_t)s * 2 + 1, 1ull);
        }
    }
}

// keep: 0 an ALL interval took the row, 1 untouched, 2 lost a cell -> 0 / 1 as the compaction reads them; a count is not lowered below 0 (a file
// may store counts smaller than its present cells: update_counts(true))
__global__ __launch_bounds__(256) void mask_verdict_kernel(uint8_t *keep, const uint32_t *present, uint32_t *vcount, uint64_t U, unsigned long long *emptied)
{
    const uint64_t r = blockIdx.x * 256ull + threadIdx.x;
    bool gone = false;
    if (r < U) {
        const uint8_t k = keep[r];
        gone = k == 2 && present[r] == 0;
        keep[r] = (k == 0 || gone) ? 0 : 1;
        if (k == 2 && (int32_t)vcount[r] < 0) vcount[r] = 0;
    }
    const unsigned long long gm = __ballot(gone);
    if ((threadIdx.x & 63u) == 0 && gm) atomicAdd(emptied, (unsigned long long)__popcll(gm));
}

struct Merged { uint32_t sample, x0, x1; };

}  // namespace
}  // namespace skx

using namespace skx;

extern "C" int skx_array_mask_regions(skx_array *a, const char *reference_fasta, const skx_mask_interval *iv, uint64_t n, skx_mask_sample *samples, skx_mask_info *info)
{
    return skx_guarded([&]() -> int {
    if (info) memset(info, 0, sizeof *info);
    if (!a || !reference_fasta || !info || (n && !iv)) { set_error("mask: bad arguments"); return SKX_EINVAL; }
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    const int k = a->k, h = (k - 1) / 2;
    const uint64_t S = a->names.size();
    if (samples) memset(samples, 0, (size_t)S * sizeof *samples);
    if (a->n_kmers != a->n_rows || a->keys_absent) { set_error("split k-mers and variants are out of step (filtered without update_kmers)"); return SKX_EINVAL; }
    if (a->total_samples && a->total_samples != S) { set_error("mask: needs every sample of the array on one device"); return SKX_EUNSUP; }
    for (uint64_t i = 0; i < n; i++) {
        if (iv[i].start > iv[i].end) { set_error("mask: interval %llu starts at %u and ends at %u", (unsigned long long)i, iv[i].start, iv[i].end); return SKX_EINVAL; }
        if (iv[i].sample != SKX_MASK_ALL_SAMPLES && iv[i].sample >= S) {
            set_error("mask: interval %llu names sample %u (the array has %llu samples)", (unsigned long long)i, iv[i].sample, (unsigned long long)S); return SKX_EINVAL;
        }
    }
    RefLookup ref;
    {
        PhaseTimer pr("mask.read_reference");
        SKX_TRY(ref.read(reference_fasta, "mask: reference longer than 4 G bases"));
    }
    const HostStream &hs = ref.hs;
    const std::vector<uint64_t> &cstart = ref.cstart, &clen = ref.clen, &coff = ref.coff;
    const uint64_t C = cstart.size();
    if (hs.ids.size() != C) { set_error("mask: %s: %llu record ids for %llu records", reference_fasta, (unsigned long long)hs.ids.size(), (unsigned long long)C); return SKX_EINVAL; }
    {
        std::unordered_set<std::string> seen;
        for (auto &id : hs.ids) if (!seen.insert(id).second) { set_error("mask: %s: chromosome id %s occurs more than once", reference_fasta, id.c_str()); return SKX_EINVAL; }
    }
    for (uint64_t i = 0; i < n; i++) {
        if (iv[i].chrom >= C) { set_error("mask: interval %llu names chromosome %u (the reference has %llu)", (unsigned long long)i, iv[i].chrom, (unsigned long long)C); return SKX_EINVAL; }
        if (iv[i].end >= clen[iv[i].chrom]) {
            set_error("mask: interval %llu ends at %u, past chromosome %s of %llu bases", (unsigned long long)i, iv[i].end, hs.ids[iv[i].chrom].c_str(), (unsigned long long)clen[iv[i].chrom]);
            return SKX_EINVAL;
        }
    }
    SKX_TRY(array_materialize(a));
    const uint64_t U = a->n_rows;
    if (U >= (1ull << 32)) { set_error("mask: %llu rows; at most 2^32 - 1 are taken", (unsigned long long)U); return SKX_EUNSUP; }

    // merged per (sample, chromosome): sorted by (sample, chromosome, start), ALL (the highest sample) last; overlapping or touching ones joined
    std::vector<Merged> mg;
    {
        std::vector<skx_mask_interval> v(iv, iv + n);
        std::sort(v.begin(), v.end(), [](const skx_mask_interval &x, const skx_mask_interval &y) {
            return x.sample != y.sample ? x.sample < y.sample : x.chrom != y.chrom ? x.chrom < y.chrom : x.start != y.start ? x.start < y.start : x.end < y.end; });
        uint32_t last_chrom = 0;
        for (const skx_mask_interval &q : v) {
            const uint32_t x0 = (uint32_t)(coff[q.chrom] + q.start), x1 = (uint32_t)(coff[q.chrom] + q.end);
            if (!mg.empty() && mg.back().sample == q.sample && last_chrom == q.chrom && (uint64_t)x0 <= (uint64_t)mg.back().x1 + 1) mg.back().x1 = std::max(mg.back().x1, x1);
            else { mg.push_back(Merged{q.sample, x0, x1}); last_chrom = q.chrom; }
        }
    }
    const uint64_t n_mg = mg.size();
    uint64_t n_own = 0;                                                 // the per-sample ones come first
    while (n_own < n_mg && mg[n_own].sample != SKX_MASK_ALL_SAMPLES) n_own++;

    {
        PhaseTimer pw("mask.windows");
        SKX_TRY(ref.windows(a, reference_fasta, true));
    }
    if (U) {
        PhaseTimer pl("mask.lookup");
        SKX_TRY(ref.lookup(a));
    }
    ref.wlo.release(); ref.whi.release(); ref.flag.release();
    const uint64_t M = ref.M;

    // ---- the sites in reference order
    PhaseTimer pk("mask.kernels");
    uint64_t N = 0;
    DevBuf<uint32_t> xs, site_row; DevBuf<uint64_t> d_cstart;
    if (M) {
        DevBuf<uint32_t> x_all, row_all; DevBuf<uint8_t> is_site;
        SKX_TRY(x_all.alloc(M)); SKX_TRY(row_all.alloc(M)); SKX_TRY(is_site.alloc(M)); SKX_TRY(xs.alloc(M)); SKX_TRY(site_row.alloc(M)); SKX_TRY(d_cstart.alloc(C));
        SKX_HIP(hipMemcpyAsync(d_cstart.p, cstart.data(), C * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(mask_sites_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, ref.mapped.p, ref.row.p, ref.rep.p, (uint32_t)h, d_cstart.p, (uint32_t)C, M,
                           x_all.p, row_all.p, is_site.p);
        SKX_HIP(hipGetLastError());
        uint64_t n2 = 0;
        SKX_TRY(prim_select_u32(x_all.p, is_site.p, xs.p, M, &N, st));
        SKX_TRY(prim_select_u32(row_all.p, is_site.p, site_row.p, M, &n2, st));
        if (n2 != N) { set_error("mask: internal error: %llu site positions and %llu site rows", (unsigned long long)N, (unsigned long long)n2); return SKX_EINVAL; }
    }
    ref.row.release(); ref.mapped.release(); ref.is_rc.release(); ref.rep.release(); ref.d_seq.release();

    // ---- the intervals' places in that list, and the items
    std::vector<uint32_t> h_lo(n_mg, 0), h_len(n_mg, 0);
    DevBuf<uint32_t> d_sample, d_lo;
    if (n_mg && N) {
        std::vector<uint32_t> hx0(n_mg), hx1(n_mg), hsm(n_mg);
        for (uint64_t i = 0; i < n_mg; i++) { hx0[i] = mg[i].x0; hx1[i] = mg[i].x1; hsm[i] = mg[i].sample; }
        DevBuf<uint32_t> d_x0, d_x1, d_len;
        SKX_TRY(d_x0.alloc(n_mg)); SKX_TRY(d_x1.alloc(n_mg)); SKX_TRY(d_len.alloc(n_mg)); SKX_TRY(d_lo.alloc(n_mg)); SKX_TRY(d_sample.alloc(n_mg));
        SKX_HIP(hipMemcpyAsync(d_x0.p, hx0.data(), n_mg * 4, hipMemcpyHostToDevice, st));
        SKX_HIP(hipMemcpyAsync(d_x1.p, hx1.data(), n_mg * 4, hipMemcpyHostToDevice, st));
        SKX_HIP(hipMemcpyAsync(d_sample.p, hsm.data(), n_mg * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(mask_bounds_kernel, dim3((unsigned)((n_mg + 255) / 256)), dim3(256), 0, st, xs.p, N, d_x0.p, d_x1.p, n_mg, d_lo.p, d_len.p);
        SKX_HIP(hipGetLastError());
        SKX_HIP(hipMemcpyAsync(h_lo.data(), d_lo.p, n_mg * 4, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipMemcpyAsync(h_len.data(), d_len.p, n_mg * 4, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipStreamSynchronize(st));                              // (the three host vectors are the host's again)
    }
    // the exclusive scans, in 64 bits: the per-sample intervals' items and the ALL intervals' items, each from 0
    std::vector<uint64_t> h_off(n_mg + 2, 0);                           // [0 .. n_own] and [n_own + 1 .. n_mg + 1]
    for (uint64_t i = 0; i < n_own; i++) h_off[i + 1] = h_off[i] + h_len[i];
    for (uint64_t i = n_own; i < n_mg; i++) h_off[i + 2] = h_off[i + 1] + h_len[i];
    const uint64_t items_own = h_off[n_own], items_all = h_off[n_mg + 1];
    if ((items_own + MK_CHUNK - 1) / MK_CHUNK >= (1ull << 31) || (items_all + MK_CHUNK - 1) / MK_CHUNK >= (1ull << 31)) {
        set_error("mask: %llu cells to visit; fewer than 2^31 chunks of %u are taken", (unsigned long long)std::max(items_own, items_all), MK_CHUNK); return SKX_EUNSUP;
    }

    info->sites = N; info->rows_in = U; info->rows_out = U; info->n_intervals_merged = n_mg; info->rows_all_samples = items_all;
    if (!items_own && !items_all) { SKX_HIP(hipGetLastError()); return SKX_OK; }       // nothing lies in an interval: the array stays as it is

    // ---- from here on the array changes
    DevBuf<uint8_t> keep; DevBuf<uint64_t> d_off; DevBuf<unsigned long long> d_counts; DevBuf<int> d_bad;
    SKX_TRY(keep.alloc(U)); SKX_TRY(d_off.alloc(n_mg + 2)); SKX_TRY(d_counts.alloc((size_t)S * 2 + 1)); SKX_TRY(d_bad.alloc(1));
    SKX_HIP(hipMemsetAsync(keep.p, 1, U, st));
    SKX_TRY(d_counts.zero(st)); SKX_TRY(d_bad.zero(st));
    SKX_HIP(hipMemcpyAsync(d_off.p, h_off.data(), (n_mg + 2) * 8, hipMemcpyHostToDevice, st));
    MaskArgs ka{};
    ka.site_row = site_row.p; ka.N = N; ka.matrix = a->matrix.p; ka.pitch = a->pitch; ka.U = U; ka.S = (uint32_t)S; ka.vcount = a->vcount.p; ka.keep = keep.p; ka.counts = d_counts.p;
    if (items_all) {
        ka.iv_sample = d_sample.p + n_own; ka.iv_lo = d_lo.p + n_own; ka.iv_off = d_off.p + n_own + 1; ka.n_iv = (uint32_t)(n_mg - n_own); ka.total = items_all;
        hipLaunchKernelGGL(mask_items_kernel<true>, dim3((unsigned)((items_all + MK_CHUNK - 1) / MK_CHUNK)), dim3(256), 0, st, ka);
        SKX_HIP(hipGetLastError());
    }
    std::vector<unsigned long long> h_counts((size_t)S * 2 + 1, 0);
    if (items_own) {
        ka.iv_sample = d_sample.p; ka.iv_lo = d_lo.p; ka.iv_off = d_off.p; ka.n_iv = (uint32_t)n_own; ka.total = items_own;
        hipLaunchKernelGGL(mask_items_kernel<false>, dim3((unsigned)((items_own + MK_CHUNK - 1) / MK_CHUNK)), dim3(256), 0, st, ka);
        SKX_HIP(hipGetLastError());
        SKX_HIP(hipMemcpyAsync(h_counts.data(), d_counts.p, (size_t)S * 2 * 8, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipStreamSynchronize(st));
    }
    uint64_t cells = 0;
    for (uint64_t s = 0; s < S; s++) cells += h_counts[s * 2 + 1];
    if (cells) launch_col_stats(a->matrix.p, a->pitch, (int)S, U, a->present.p, a->unambig.p, a->mask.p, d_bad.p, st);
    hipLaunchKernelGGL(mask_verdict_kernel, dim3((unsigned)((U + 255) / 256)), dim3(256), 0, st, keep.p, a->present.p, a->vcount.p, U, d_counts.p + S * 2);
    SKX_HIP(hipGetLastError());
    unsigned long long emptied = 0;
    SKX_HIP(hipMemcpyAsync(&emptied, d_counts.p + S * 2, 8, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    a->planes.release();                                                // (bit planes of a distance sweep were those of the cells before)
    pk.stop();
    uint64_t removed = 0;
    {
        PhaseTimer pc("mask.compact");
        SKX_TRY(array_keep_rows(a, keep, &removed));
    }
    if (removed != items_all + emptied) { set_error("mask: internal error: %llu rows removed, %llu + %llu counted", (unsigned long long)removed, (unsigned long long)items_all, emptied); return SKX_EINVAL; }
    info->rows_emptied = emptied; info->rows_out = U - removed;
    if (samples) for (uint64_t s = 0; s < S; s++) { samples[s].sites_in_regions = h_counts[s * 2]; samples[s].cells_masked = h_counts[s * 2 + 1]; }
    return SKX_OK;
    });
}

extern "C" int skx_reference_records(const char *reference_fasta, char **ids, uint64_t **lens, uint64_t *n)
{
    return skx_guarded([&]() -> int {
    if (ids) *ids = nullptr;
    if (lens) *lens = nullptr;
    if (n) *n = 0;
    if (!reference_fasta || !ids || !lens || !n) { set_error("reference records: bad arguments"); return SKX_EINVAL; }
    RefLookup ref;
    SKX_TRY(ref.read(reference_fasta, "reference longer than 4 G bases"));
    const uint64_t C = ref.cstart.size();
    if (ref.hs.ids.size() != C) { set_error("%s: %llu record ids for %llu records", reference_fasta, (unsigned long long)ref.hs.ids.size(), (unsigned long long)C); return SKX_EINVAL; }
    size_t id_bytes = 0; for (auto &id : ref.hs.ids) id_bytes += id.size() + 1;
    char *pi = (char *)malloc(id_bytes ? id_bytes : 1);
    uint64_t *pl = (uint64_t *)malloc((C ? C : 1) * sizeof(uint64_t));
    if (!pi || !pl) { free(pi); free(pl); set_error("out of host memory"); return SKX_ENOMEM; }
    { char *w = pi; for (auto &id : ref.hs.ids) { memcpy(w, id.c_str(), id.size() + 1); w += id.size() + 1; } }
    for (uint64_t c = 0; c < C; c++) pl[c] = ref.clen[c];
    *ids = pi; *lens = pl; *n = C;
    return SKX_OK;
    });
}
