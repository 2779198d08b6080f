// skx_density.hip -- `ska density`: dense-SNP regions per sample along a reference (skx_array_snp_density, include/skx.h; definition there and in
// tests/density_model.py).  The reference has no counterpart: its users write `ska map`'s S x L alignment and run a separate tool over it.
//
// The windows, their look-up, the repeat flags and the compaction of the hits are `ska map`'s (RefLookup, skx_internal.h).  A repeated window
// is no site, so a row is the row of at most one site, and what a cell has to be compared with can be written per ROW: density_rows_kernel
// leaves want[row] -- the byte a matching cell holds (want_byte, skx_cells.h), with bit 5 set where it was complemented so that a SNP's base
// can be reported on the reference's strand; 0: the row is no site -- and xcat[row], the site's position in the concatenated reference.
//
// density_kernel streams the matrix (sample-major, so a row of the reference is a column here) in units of (SKX_DENSITY_TILE_ROWS columns,
// SKX_DENSITY_SAMPLES samples), the sample blocks fastest along the grid so that the units in flight share their part of want
// (qc_samples_kernel's shape).  A lane holds 16 columns: their 16 want bytes are loaded once, then the unit's samples are walked with one
// 16-byte load each, four in flight (the walk of walk_columns, skx_cells.h, spelled out).  The cells of columns that are no site are masked to the 0 byte before they are
// classed, which counts them as missing; a lane takes its number of such columns off again.  One template, two launches (skx_sites.hip):
//   count   per sample and lane one word of three 10-bit fields (missing, ambiguous, one of ACGT) from an LDS table and the count of cells equal
//           to want; summed over each half of the wave by DPP adds (half_wave_sum), added to the unit's [samples][4] block in LDS, and from
//           there one 64-bit atomic per (sample, count) and unit; the unit's number of SNPs is stored.
//   write   after prim_scan_add_u32 over the units: units without a SNP return at once; a lane that finds SNPs takes their slots from a counter
//           in LDS and stores one record a SNP at the unit's offset: sample << 34 | xcat << 2 | base.  xcat is read only there.
// The records are unique per (sample, position), so their sorted list (prim_sort_keys_u64, 62 bits) does not depend on the order of arrival.
// Over the sorted list, in blocks of SKX_DENSITY_SCAN_BLOCK: q[i] = records i and i + T - 1 are of one sample and chromosome and less than W
// apart; the last qualifying index at or before i (prim_scan_max_u32) says whether i is dense; the first and the last record of every run
// of dense SNPs of one (sample, chromosome) are selected (prim_select_index_u8) and paired up as regions.
//
// Integer atomics only, no floats, no sort inside a kernel.  No workgroup waits for another, every loop is bounded by the unit or by log2 of the
// chromosomes, and every barrier is reached by all 256 threads (a write unit without SNPs returns as a whole before the first one).
//
// Device memory beside the array: `ska map`'s window buffers (25 bytes a reference byte at k <= 31, 33 above) and the repeat sort's (28 bytes a
// window), 5 bytes a row (rounded up to SKX_DENSITY_TILE_ROWS), 8 bytes a unit, 64 bytes a sample, 8 bytes a bin, and per SNP record 16 bytes
// and the radix sort's own buffers while the list is sorted, 27 bytes after it, 20 bytes a region.
#include "skx_internal.h"
#include "skx_cells.h"
#include <algorithm>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

namespace skx {
namespace {

constexpr uint32_t DN_THREADS = SKX_DENSITY_TILE_ROWS / 16;
constexpr uint32_t DN_B = SKX_DENSITY_SAMPLES;
constexpr uint32_t DN_SCAN = SKX_DENSITY_SCAN_BLOCK;
static_assert(DN_THREADS == 256, "a workgroup of 256 threads, 16 columns each");
static_assert(DN_B % 4 == 0 && DN_B <= 256, "the walk is unrolled by the four loads in flight; a thread a sample at the unit's end");
static_assert(SKX_DENSITY_TILE_ROWS / 4 / 2 <= 0x3FF, "half a wave's sum of a count fits a 10-bit field");
static_assert(DN_SCAN % 256 == 0, "a workgroup of 256 threads strides over a scan block");
static_assert(sizeof(skx_density_sample) == 8 * sizeof(uint64_t) && sizeof(skx_density_region) == 20 && sizeof(skx_density_bin) == 8, "the device writes these records");

// per hit window m (reference order) that is not repeated: want and xcat of its row.  The record stream holds one '\n' behind every chromosome, so
// a middle base at stream position mid of chromosome c sits at mid - c of the concatenated reference
__global__ __launch_bounds__(256) void density_rows_kernel(const uint32_t *mapped, const uint32_t *row, const uint8_t *is_rc, const uint8_t *rep, const uint8_t *seq, uint32_t h,
                                                          const uint64_t *cstart, uint32_t n_chrom, uint64_t M, uint8_t *want, uint32_t *xcat, unsigned long long *n_sites)
{
    const uint64_t m = blockIdx.x * 256ull + threadIdx.x;
    bool site = false;
    if (m < M) {
        const uint32_t p = mapped[m];
        if (!rep[p]) {
            site = true;
            const uint64_t mid = (uint64_t)p - h;
            const uint32_t c = chrom_of(cstart, n_chrom, mid);
            const uint32_t r = row[p];
            want[r] = want_byte(seq[mid], is_rc[p]) | (is_rc[p] ? 0x20u : 0u);
            xcat[r] = (uint32_t)(mid - c);
        }
    }
    const uint32_t n = (uint32_t)__popcll(__ballot(site));
    if ((threadIdx.x & 63u) == 0 && n) atomicAdd(n_sites, (unsigned long long)n);
}

struct DensityArgs {
    const uint8_t *matrix; uint64_t pitch, n_cols;
    const uint8_t *want;                                            // [n_tiles * SKX_DENSITY_TILE_ROWS]
    const uint32_t *xcat;                                           // [n_cols]
    uint32_t S, n_sblocks;
    unsigned long long *counts;                                     // [S][8] in the order of skx_density_sample
    uint32_t *unit_snps;                                            // [units] the count launch's
    const uint32_t *unit_incl;                                      // their inclusive scan
    unsigned long long *total;                                      // the count launch adds every unit's SNPs
    uint64_t *rec; uint64_t cap;
    int *bad_byte;
};

template <bool WRITE>
__global__ __launch_bounds__(256) void density_kernel(DensityArgs a)
{
    __shared__ uint32_t s_lut[256];                                 // 1: '-' or the 0 byte; 1 << 10: present and none of A, C, G, T; 1 << 20: one of them; 0: outside the alphabet
    __shared__ uint32_t s_cnt[DN_B * 4];                            // count: missing, ambiguous, one of ACGT, equal to want
    __shared__ uint32_t s_unit;                                     // count: the unit's SNPs; write: the slots handed out
    const uint32_t have = WRITE ? a.unit_snps[blockIdx.x] : 0u;
    if (WRITE && !have) return;                                     // (the same for the whole workgroup: no barrier is skipped by a part of it)
    const uint32_t sb = blockIdx.x % a.n_sblocks;
    const uint64_t tile = blockIdx.x / a.n_sblocks;
    const uint64_t c0 = (tile * 256 + threadIdx.x) * 16;
    const int lane = threadIdx.x & 63;
    const uint32_t s0 = sb * DN_B, s1 = min(a.S, s0 + DN_B);        // s0 < S: the grid holds no empty block
    {
        const uint32_t c = cell_code(threadIdx.x);
        s_lut[threadIdx.x] = c == CELL_OUTSIDE ? 0u : c == 0 ? 1u : cell_one_base(c) ? 1u << 20 : 1u << 10;
    }
    if (!WRITE) for (uint32_t j = threadIdx.x; j < DN_B * 4; j += 256) s_cnt[j] = 0;
    if (threadIdx.x == 0) s_unit = 0;
    // the lane's 16 columns: what a matching cell holds (0x100: no site, no byte equals it), which strand, and the byte mask of the sites.  want
    // covers whole tiles and is 0 past the last column, so the sites' mask stands in for ColumnLane's: only its column pointer is taken
    const uint8_t *col = ColumnLane(a.matrix, a.n_cols, c0).col;
    uint32_t w[16], rc2 = 0, n_off = 0;
    u32x4 sm;
    {
        const u32x4 wv = *reinterpret_cast<const u32x4 *>(a.want + c0);
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t x = (wv[i >> 2] >> (8 * (i & 3))) & 0xFFu;
            w[i] = x ? (x & 0xDFu) : 0x100u;
            rc2 |= ((x >> 5) & 1u) << i;
            n_off += x ? 0u : 1u;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t x = wv[q];
            sm[q] = (x & 0xFFu ? 0xFFu : 0u) | (x & 0xFF00u ? 0xFF00u : 0u) | (x & 0xFF0000u ? 0xFF0000u : 0u) | (x & 0xFF000000u ? 0xFF000000u : 0u);
        }
    }
    __syncthreads();
    auto load = [&](uint32_t t) -> u32x4 { return *reinterpret_cast<const u32x4 *>(col + (uint64_t)min(t, s1 - 1) * a.pitch); };
    const uint32_t shift = 10u * ((uint32_t)lane % 3u);
    uint32_t bad = 0;
    const uint64_t base = WRITE ? (uint64_t)a.unit_incl[blockIdx.x] - have : 0;     // (the scan is inclusive; the total is below 2^32)
    auto step = [&](uint32_t t, const u32x4 raw) {
        const u32x4 cur = raw & sm;
        if (!WRITE) {
            uint32_t all = 0, eq = 0;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const uint32_t b = (cur[i >> 2] >> (8 * (i & 3))) & 0xFFu;
                all += s_lut[b];
                eq += b == w[i] ? 1u : 0u;
            }
            // every cell is of one class: the three fields sum to 16 unless a site's cell lies outside the alphabet
            bad |= (all & 0x3FFu) + ((all >> 10) & 0x3FFu) + (all >> 20) != 16u ? 1u : 0u;
            all -= n_off;                                           // (the masked cells read as missing: at least n_off of the field)
            const uint32_t w1 = half_wave_sum(all), w2 = half_wave_sum(eq);
            const uint32_t x1 = (uint32_t)__builtin_amdgcn_readlane((int)w1, 31), y1 = (uint32_t)__builtin_amdgcn_readlane((int)w1, 63);
            const uint32_t x2 = (uint32_t)__builtin_amdgcn_readlane((int)w2, 31), y2 = (uint32_t)__builtin_amdgcn_readlane((int)w2, 63);
            const uint32_t v = lane < 3 ? ((x1 >> shift) & 0x3FFu) + ((y1 >> shift) & 0x3FFu) : x2 + y2;
            if (lane < 4 && v) atomicAdd(&s_cnt[(t - s0) * 4 + lane], v);
        } else {
            uint32_t m = 0;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const uint32_t b = (cur[i >> 2] >> (8 * (i & 3))) & 0xFFu;
                m |= ((s_lut[b] >> 20) & (b != w[i] ? 1u : 0u)) << i;
            }
            if (m) {
                uint32_t slot = atomicAdd(&s_unit, (uint32_t)__popc(m));
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    if (!((m >> i) & 1u)) continue;
                    const uint32_t b = (cur[i >> 2] >> (8 * (i & 3))) & 0xFFu;
                    const uint64_t pos = base + slot;
                    if (slot < have && pos < a.cap)                 // (the count launch sized the unit and the buffer: never false)
                        a.rec[pos] = ((uint64_t)t << 34) | ((uint64_t)a.xcat[c0 + i] << 2) | (((b >> 1) & 3u) ^ (((rc2 >> i) & 1u) << 1));
                    slot++;
                }
            }
        }
    };
    // walk_columns' walk (skx_cells.h) spelled out: the shared form adds 10 vector and 58 scalar instructions to the loop (NOTEBOOK 2026-10-21, one column walk)
    u32x4 b0 = load(s0);
    __builtin_amdgcn_sched_barrier(0);
    u32x4 b1 = load(s0 + 1);
    __builtin_amdgcn_sched_barrier(0);
    u32x4 b2 = load(s0 + 2);
    __builtin_amdgcn_sched_barrier(0);
    u32x4 b3 = load(s0 + 3);
    for (uint32_t t = s0; t < s1; t += 4) {                         // (b0 holds sample t; every bound is the same for the whole workgroup)
        step(t, b0); b0 = load(t + 4);
        if (t + 1 < s1) step(t + 1, b1);
        b1 = load(t + 5);
        if (t + 2 < s1) step(t + 2, b2);
        b2 = load(t + 6);
        if (t + 3 < s1) step(t + 3, b3);
        b3 = load(t + 7);
    }
    if (WRITE) return;
    __syncthreads();
    if (threadIdx.x < s1 - s0) {
        const uint32_t *c = s_cnt + threadIdx.x * 4;
        const uint32_t missing = c[0], ambiguous = c[1], callable = c[2], snps = c[2] - c[3];
        unsigned long long *o = a.counts + (uint64_t)(s0 + threadIdx.x) * 8;
        if (callable) atomicAdd(o + 1, (unsigned long long)callable);
        if (ambiguous) atomicAdd(o + 2, (unsigned long long)ambiguous);
        if (missing) atomicAdd(o + 3, (unsigned long long)missing);
        if (snps) { atomicAdd(o + 4, (unsigned long long)snps); atomicAdd(&s_unit, snps); }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.unit_snps[blockIdx.x] = s_unit;
        if (s_unit) atomicAdd(a.total, (unsigned long long)s_unit);
    }
    if (bad) *a.bad_byte = 1;
}

// ---- over the sorted records.  A workgroup takes DN_SCAN consecutive records, a thread every 256th of them
struct DenseArgs {
    const uint64_t *key; uint64_t n;
    const uint64_t *coff; uint32_t n_chrom;                         // [n_chrom + 1] where a chromosome starts in the concatenated reference
    const uint64_t *binoff;                                         // [n_chrom] its first bin
    uint64_t W; uint32_t T;
    uint32_t *last_in; const uint32_t *last;                        // i + 1 where q[i], else 0; its inclusive max-scan
    uint8_t *dense, *first, *final_;
    skx_density_bin *bins;
    unsigned long long *counts;
    const uint32_t *starts, *ends; uint64_t n_regions;
    skx_density_region *regions;
};
__device__ inline uint64_t rec_sample(uint64_t k) { return k >> 34; }
__device__ inline uint64_t rec_x(uint64_t k) { return (k >> 2) & 0xFFFFFFFFull; }

// q[i]: records i .. i + T - 1 are T consecutive SNPs of one (sample, chromosome) inside W consecutive positions
__global__ __launch_bounds__(256) void density_q_kernel(DenseArgs a)
{
    for (uint32_t j = threadIdx.x; j < DN_SCAN; j += 256) {
        const uint64_t i = (uint64_t)blockIdx.x * DN_SCAN + j;
        if (i >= a.n) break;
        bool q = false;
        if (i + a.T - 1 < a.n) {
            const uint64_t ka = a.key[i], kb = a.key[i + a.T - 1];
            if (rec_sample(ka) == rec_sample(kb) && rec_x(kb) - rec_x(ka) < a.W)
                q = chrom_of(a.coff, a.n_chrom, rec_x(ka)) == chrom_of(a.coff, a.n_chrom, rec_x(kb));
        }
        a.last_in[i] = q ? (uint32_t)(i + 1) : 0u;                  // (n < 2^32 - 1)
    }
}

// dense[i], the bins' counters and the samples' dense_snps.  The records of a wave's step are 64 consecutive ones of the sorted list: mostly of
// one sample, which then gets one atomic
__global__ __launch_bounds__(256) void density_mark_kernel(DenseArgs a)
{
    for (uint32_t j = threadIdx.x; j < DN_SCAN; j += 256) {         // (the same trip count for every lane: the ballots below are whole waves')
        const uint64_t i = (uint64_t)blockIdx.x * DN_SCAN + j;
        const bool valid = i < a.n;
        bool d = false; uint64_t s = 0;
        if (valid) {
            const uint64_t k = a.key[i], x = rec_x(k);
            const uint32_t l = a.last[i];
            d = l != 0 && (uint64_t)(l - 1) + a.T - 1 >= i;
            s = rec_sample(k);
            a.dense[i] = d ? 1 : 0;
            const uint32_t c = chrom_of(a.coff, a.n_chrom, x);
            skx_density_bin *b = a.bins + a.binoff[c] + (x - a.coff[c]) / a.W;
            atomicAdd(&b->snps, 1u);
            if (d) atomicAdd(&b->dense_snps, 1u);
        }
        const unsigned long long dm = __ballot(d);
        const uint64_t s_first = __shfl(s, 0, 64);
        const bool one = __all(!valid || s == s_first);
        if (one) { if ((threadIdx.x & 63u) == 0 && dm) atomicAdd(a.counts + s * 8 + 5, (unsigned long long)__popcll(dm)); }
        else if (d) atomicAdd(a.counts + s * 8 + 5, 1ull);
    }
}

// first[i] / final[i]: record i is the first / the last of a maximal run of dense SNPs of one (sample, chromosome)
__global__ __launch_bounds__(256) void density_edges_kernel(DenseArgs a)
{
    for (uint32_t j = threadIdx.x; j < DN_SCAN; j += 256) {
        const uint64_t i = (uint64_t)blockIdx.x * DN_SCAN + j;
        if (i >= a.n) break;
        uint8_t f = 0, l = 0;
        if (a.dense[i]) {
            const uint64_t k = a.key[i];
            const uint32_t c = chrom_of(a.coff, a.n_chrom, rec_x(k));
            auto joined = [&](uint64_t o) { const uint64_t ko = a.key[o]; return a.dense[o] && rec_sample(ko) == rec_sample(k) && chrom_of(a.coff, a.n_chrom, rec_x(ko)) == c; };
            f = !(i > 0 && joined(i - 1));
            l = !(i + 1 < a.n && joined(i + 1));
        }
        a.first[i] = f; a.final_[i] = l;
    }
}

// region r = the records starts[r] .. ends[r]: the runs are disjoint and in order, so the r-th first pairs with the r-th last
__global__ __launch_bounds__(256) void density_regions_kernel(DenseArgs a)
{
    const uint64_t r = blockIdx.x * 256ull + threadIdx.x;
    if (r >= a.n_regions) return;
    const uint32_t i0 = a.starts[r], i1 = a.ends[r];
    const uint64_t k0 = a.key[i0], k1 = a.key[i1];
    const uint32_t c = chrom_of(a.coff, a.n_chrom, rec_x(k0));
    skx_density_region o;
    o.sample = (uint32_t)rec_sample(k0); o.chrom = c;
    o.start = (uint32_t)(rec_x(k0) - a.coff[c]); o.end = (uint32_t)(rec_x(k1) - a.coff[c]); o.snps = i1 - i0 + 1;
    a.regions[r] = o;
    atomicAdd(a.counts + (uint64_t)o.sample * 8 + 6, 1ull);
    atomicAdd(a.counts + (uint64_t)o.sample * 8 + 7, (unsigned long long)(o.end - o.start) + 1ull);
}

}  // namespace
}  // namespace skx

using namespace skx;

extern "C" int skx_array_snp_density(skx_array *a, const char *reference_fasta, uint64_t window, uint32_t min_snps, int flags, skx_density_result *out)
{
    return skx_guarded([&]() -> int {
    if (out) memset(out, 0, sizeof *out);
    if (!a || !reference_fasta || !out) { set_error("density: bad arguments"); return SKX_EINVAL; }
    if (window < 1 || window > (1ull << 31)) { set_error("density: window must be between 1 and 2^31 (inclusive)"); return SKX_EINVAL; }
    if (min_snps < 2 || min_snps > 65535) { set_error("density: min_snps must be between 2 and 65535 (inclusive)"); return SKX_EINVAL; }
    if (flags & ~SKX_DENSITY_WANT_SNPS) { set_error("density: unknown flags"); return SKX_EINVAL; }
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    const int k = a->k, h = (k - 1) / 2;
    const uint64_t S = a->names.size(), W = window; const uint32_t T = min_snps;
    if (a->n_kmers != a->n_rows || a->keys_absent) { set_error("split k-mers and variants are out of step (filtered without update_kmers)"); return SKX_EINVAL; }
    if (a->total_samples && a->total_samples != S) { set_error("density: needs every sample of the array on one device"); return SKX_EUNSUP; }
    if (S >= (1ull << 28)) { set_error("density: %llu samples; fewer than 2^28 are taken (a record's sample holds 28 bits)", (unsigned long long)S); return SKX_EUNSUP; }
    SKX_TRY(array_materialize(a));
    const uint64_t U = a->n_rows;
    if (U >= (1ull << 32)) { set_error("density: %llu rows; at most 2^32 - 1 are taken", (unsigned long long)U); return SKX_EUNSUP; }
    RefLookup ref;
    {
        PhaseTimer pr("density.read_reference");
        SKX_TRY(ref.read(reference_fasta, "density: reference longer than 4 G bases"));
    }
    const HostStream &hs = ref.hs;
    const std::vector<uint64_t> &cstart = ref.cstart, &clen = ref.clen, &coff = ref.coff;      // chromosomes: start in the record stream, length, start in the concatenated reference
    const uint64_t C = cstart.size();
    if (hs.ids.size() != C) { set_error("density: %s: %llu record ids for %llu records", reference_fasta, (unsigned long long)hs.ids.size(), (unsigned long long)C); return SKX_EINVAL; }
    {
        std::unordered_set<std::string> seen;
        for (auto &id : hs.ids) if (!seen.insert(id).second) { set_error("density: %s: chromosome id %s occurs more than once", reference_fasta, id.c_str()); return SKX_EINVAL; }
    }
    PhaseTimer pw("density.windows");
    SKX_TRY(ref.windows(a, reference_fasta, true));
    const std::vector<uint8_t> &hrep = ref.hrep;
    const uint64_t n_windows = ref.n_windows;
    uint64_t n_repeat = 0;
    for (uint64_t p = 0; p < ref.L; p++) n_repeat += ref.hflag[p] && hrep[p];
    std::vector<uint64_t> binoff(C);
    uint64_t n_bins = 0;
    for (uint64_t c = 0; c < C; c++) { binoff[c] = n_bins; n_bins += (clen[c] + W - 1) / W; }
    pw.stop();

    // look-up and compaction (an array without rows has no hit)
    if (U) {
        PhaseTimer pl("density.lookup");
        SKX_TRY(ref.lookup(a));
    }
    ref.wlo.release(); ref.whi.release(); ref.flag.release();
    DevBuf<uint32_t> &row = ref.row, &mapped = ref.mapped; DevBuf<uint8_t> &is_rc = ref.is_rc, &rep = ref.rep, &d_seq = ref.d_seq;
    const uint64_t M = ref.M;

    // the results that do not depend on a kernel
    skx_density_result res{};
    struct Mem { skx_density_result *r; bool keep = false; ~Mem() { if (!keep) { free(r->samples); free(r->regions); free(r->bins); free(r->chrom_ids); free(r->chrom_lens); free(r->snps); free(r->snp_ref); } } } mem{&res};
    res.samples = (skx_density_sample *)calloc(S ? S : 1, sizeof(skx_density_sample));
    res.bins = (skx_density_bin *)calloc(n_bins ? n_bins : 1, sizeof(skx_density_bin));
    res.chrom_lens = (uint64_t *)malloc((C ? C : 1) * sizeof(uint64_t));
    size_t id_bytes = 0; for (auto &id : hs.ids) id_bytes += id.size() + 1;
    res.chrom_ids = (char *)malloc(id_bytes ? id_bytes : 1);
    if (!res.samples || !res.bins || !res.chrom_lens || !res.chrom_ids) { set_error("out of host memory"); return SKX_ENOMEM; }
    { char *w = res.chrom_ids; for (auto &id : hs.ids) { memcpy(w, id.c_str(), id.size() + 1); w += id.size() + 1; } }
    for (uint64_t c = 0; c < C; c++) res.chrom_lens[c] = clen[c];
    res.info.windows = n_windows; res.info.repeat_windows = n_repeat; res.info.n_chrom = C; res.info.n_bins = n_bins;

    uint64_t n_sites = 0, n_snps = 0, n_regions = 0;
    if (M && S) {
        const uint64_t n_tiles = (U + SKX_DENSITY_TILE_ROWS - 1) / SKX_DENSITY_TILE_ROWS, n_sblocks = (S + DN_B - 1) / DN_B, units = n_tiles * n_sblocks;
        if (units >= (1ull << 31)) { set_error("density: %llu tiles of rows x %llu blocks of samples; fewer than 2^31 units are taken", (unsigned long long)n_tiles, (unsigned long long)n_sblocks); return SKX_EUNSUP; }
        DevBuf<uint8_t> want; DevBuf<uint32_t> xcat, unit_snps, unit_incl; DevBuf<uint64_t> d_cstart, d_coff, d_binoff; DevBuf<unsigned long long> d_counts, d_tot; DevBuf<int> d_bad;
        DevBuf<skx_density_bin> d_bins;
        {
            PhaseTimer pk("density.rows");
            SKX_TRY(want.alloc((size_t)n_tiles * SKX_DENSITY_TILE_ROWS)); SKX_TRY(xcat.alloc(U)); SKX_TRY(d_cstart.alloc(C)); SKX_TRY(d_coff.alloc(C + 1)); SKX_TRY(d_binoff.alloc(C));
            SKX_TRY(d_counts.alloc((size_t)S * 8)); SKX_TRY(d_tot.alloc(2)); SKX_TRY(d_bad.alloc(1)); SKX_TRY(unit_snps.alloc(units)); SKX_TRY(unit_incl.alloc(units));
            if (d_bins.alloc(n_bins) != SKX_OK) { set_error("density: %llu bins do not fit in device memory", (unsigned long long)n_bins); return SKX_ENOMEM; }
            SKX_TRY(want.zero(st)); SKX_TRY(d_counts.zero(st)); SKX_TRY(d_tot.zero(st)); SKX_TRY(d_bad.zero(st)); SKX_TRY(d_bins.zero(st));
            SKX_HIP(hipMemcpyAsync(d_cstart.p, cstart.data(), C * 8, hipMemcpyHostToDevice, st));
            SKX_HIP(hipMemcpyAsync(d_coff.p, coff.data(), (C + 1) * 8, hipMemcpyHostToDevice, st));
            SKX_HIP(hipMemcpyAsync(d_binoff.p, binoff.data(), C * 8, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(density_rows_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, mapped.p, row.p, is_rc.p, rep.p, d_seq.p, (uint32_t)h, d_cstart.p, (uint32_t)C, M,
                               want.p, xcat.p, d_tot.p + 1);
            SKX_HIP(hipGetLastError());
            SKX_HIP(hipStreamSynchronize(st));
        }
        row.release(); mapped.release(); is_rc.release(); rep.release();
        DensityArgs ka{};
        ka.matrix = a->matrix.p; ka.pitch = a->pitch; ka.n_cols = U; ka.want = want.p; ka.xcat = xcat.p; ka.S = (uint32_t)S; ka.n_sblocks = (uint32_t)n_sblocks;
        ka.counts = d_counts.p; ka.unit_snps = unit_snps.p; ka.unit_incl = unit_incl.p; ka.total = d_tot.p; ka.bad_byte = d_bad.p;
        unsigned long long tot[2] = {0, 0}; int bad = 0;
        {
            PhaseTimer pk("density.count");
            hipLaunchKernelGGL(density_kernel<false>, dim3((unsigned)units), dim3(256), 0, st, ka);
            SKX_HIP(hipGetLastError());
            SKX_HIP(hipMemcpyAsync(tot, d_tot.p, sizeof tot, hipMemcpyDeviceToHost, st));
            SKX_HIP(hipMemcpyAsync(&bad, d_bad.p, 4, hipMemcpyDeviceToHost, st));
            SKX_HIP(hipStreamSynchronize(st));
        }
        if (bad) { set_error("density: variants contain a byte outside -ACGTMRWSYKVHDBN"); return SKX_EINVAL; }
        n_snps = tot[0]; n_sites = tot[1];
        if (n_snps >= 0xFFFFFFFEull) { set_error("density: %llu SNP records; fewer than 2^32 - 2 are taken", (unsigned long long)n_snps); return SKX_EUNSUP; }
        if (n_snps) {
            DevBuf<uint64_t> rec, key;
            if (rec.alloc(n_snps) != SKX_OK || key.alloc(n_snps) != SKX_OK) { set_error("density: %llu SNP records (%llu MB) do not fit in device memory", (unsigned long long)n_snps, (unsigned long long)(n_snps * 16 >> 20)); return SKX_ENOMEM; }
            {
                PhaseTimer pk("density.write");
                SKX_TRY(prim_scan_add_u32(unit_snps.p, unit_incl.p, units, st));
                ka.rec = rec.p; ka.cap = n_snps;
                hipLaunchKernelGGL(density_kernel<true>, dim3((unsigned)units), dim3(256), 0, st, ka);
                SKX_HIP(hipGetLastError());
                SKX_HIP(hipStreamSynchronize(st));
            }
            {
                PhaseTimer pk("density.sort");
                SKX_TRY(prim_sort_keys_u64(rec.p, key.p, n_snps, 62, st));
            }
            rec.release();
            PhaseTimer pk("density.dense");
            DevBuf<uint32_t> last_in, last, starts, ends; DevBuf<uint8_t> dense, first, final_;
            SKX_TRY(last_in.alloc(n_snps)); SKX_TRY(last.alloc(n_snps)); SKX_TRY(dense.alloc(n_snps)); SKX_TRY(first.alloc(n_snps)); SKX_TRY(final_.alloc(n_snps));
            DenseArgs da{};
            da.key = key.p; da.n = n_snps; da.coff = d_coff.p; da.n_chrom = (uint32_t)C; da.binoff = d_binoff.p; da.W = W; da.T = T;
            da.last_in = last_in.p; da.last = last.p; da.dense = dense.p; da.first = first.p; da.final_ = final_.p; da.bins = d_bins.p; da.counts = d_counts.p;
            const dim3 sgrid((unsigned)((n_snps + DN_SCAN - 1) / DN_SCAN));
            hipLaunchKernelGGL(density_q_kernel, sgrid, dim3(256), 0, st, da);
            SKX_HIP(hipGetLastError());
            SKX_TRY(prim_scan_max_u32(last_in.p, last.p, n_snps, st));
            hipLaunchKernelGGL(density_mark_kernel, sgrid, dim3(256), 0, st, da);
            hipLaunchKernelGGL(density_edges_kernel, sgrid, dim3(256), 0, st, da);
            SKX_HIP(hipGetLastError());
            uint64_t n_ends = 0;
            SKX_TRY(starts.alloc(n_snps)); SKX_TRY(ends.alloc(n_snps));
            SKX_TRY(prim_select_index_u8(first.p, starts.p, n_snps, &n_regions, st));
            SKX_TRY(prim_select_index_u8(final_.p, ends.p, n_snps, &n_ends, st));
            if (n_ends != n_regions) { set_error("density: internal error: %llu region starts and %llu region ends", (unsigned long long)n_regions, (unsigned long long)n_ends); return SKX_EINVAL; }
            DevBuf<skx_density_region> d_regions;
            if (n_regions) {
                SKX_TRY(d_regions.alloc(n_regions));
                res.regions = (skx_density_region *)malloc(n_regions * sizeof(skx_density_region));
                if (!res.regions) { set_error("out of host memory"); return SKX_ENOMEM; }
                da.starts = starts.p; da.ends = ends.p; da.n_regions = n_regions; da.regions = d_regions.p;
                hipLaunchKernelGGL(density_regions_kernel, dim3((unsigned)((n_regions + 255) / 256)), dim3(256), 0, st, da);
                SKX_HIP(hipGetLastError());
                SKX_HIP(hipMemcpyAsync(res.regions, d_regions.p, n_regions * sizeof(skx_density_region), hipMemcpyDeviceToHost, st));
            }
            if (flags & SKX_DENSITY_WANT_SNPS) {
                res.snps = (uint64_t *)malloc(n_snps * sizeof(uint64_t)); res.snp_ref = (uint8_t *)malloc(n_snps);
                std::vector<uint8_t> hd(n_snps);
                if (!res.snps || !res.snp_ref) { set_error("density: %llu SNP records do not fit in host memory", (unsigned long long)n_snps); return SKX_ENOMEM; }
                SKX_HIP(hipMemcpyAsync(res.snps, key.p, n_snps * 8, hipMemcpyDeviceToHost, st));
                SKX_HIP(hipMemcpyAsync(hd.data(), dense.p, n_snps, hipMemcpyDeviceToHost, st));
                SKX_HIP(hipStreamSynchronize(st));
                for (uint64_t i = 0; i < n_snps; i++) {
                    const uint64_t x = (res.snps[i] >> 2) & 0xFFFFFFFFull;
                    const uint64_t c = (uint64_t)(std::upper_bound(coff.begin(), coff.begin() + (ptrdiff_t)C, x) - coff.begin()) - 1;
                    res.snp_ref[i] = hs.seq[x + c] & 0xDFu;
                    res.snps[i] |= (uint64_t)hd[i] << SKX_DENSITY_DENSE_BIT;
                }
            }
            SKX_HIP(hipStreamSynchronize(st));
            SKX_HIP(hipGetLastError());
        }
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the device counters are a sample's record");
        SKX_HIP(hipMemcpyAsync(res.samples, d_counts.p, (size_t)S * sizeof(skx_density_sample), hipMemcpyDeviceToHost, st));
        SKX_HIP(hipMemcpyAsync(res.bins, d_bins.p, (size_t)n_bins * sizeof(skx_density_bin), hipMemcpyDeviceToHost, st));
        SKX_HIP(hipStreamSynchronize(st));
    }
    for (uint64_t s = 0; s < S; s++) res.samples[s].sites = n_sites;
    if (M && !S) {                                                  // (no sample to count for: the sites are still the reference's and the array's)
        uint64_t sites = 0;
        std::vector<uint32_t> hm(M);
        SKX_HIP(hipMemcpy(hm.data(), mapped.p, M * 4, hipMemcpyDeviceToHost));
        for (uint64_t m = 0; m < M; m++) sites += !hrep[hm[m]];
        n_sites = sites;
    }
    res.info.sites = n_sites; res.info.n_snps = n_snps; res.info.n_regions = n_regions;
    mem.keep = true;
    *out = res;
    return SKX_OK;
    });
}
