// skx_sites.hip -- `ska distance --sites`: the rows behind the distance of each selected pair (skx_array_pair_sites, include/skx.h; definition there
// and in tests/sites_model.py).  The reference has no counterpart: its users run `ska delete` down to the pair, `ska align` and `ska nk --full-info`
// and compare columns by eye.
//
//   sites(i, j) = { r swept : M[i][r] and M[j][r] unambiguous and M[i][r] != M[j][r] },  r ascending
//
// The matrix is sample-major, so a row of the reference is a column here.  A work unit is (chunk of 4 096 columns, pair): a workgroup of 256 lanes,
// each lane 16 consecutive columns -- one 16-byte load from either sample's row, one for the 16 keep flags of the two distance filters -- and from
// these a 16-bit mask of site columns.  The units are numbered with the pair index fastest: workgroups in flight together read the same chunk of at
// most S samples, which the caches then hold.
//
//   count launch   one uint32 per (pair, chunk), pair-major.  The engine's scan (skx_prims.hip) makes them offsets inside a pair (modulo 2^32: a
//                  pair holds fewer records than that before its last chunk), pair_totals_kernel the 64-bit total of every pair; the host adds the
//                  pairs up, knows the exact number of records before their buffer exists, and hands back where every pair starts.
//   write launch   units without a site return at once; the others recompute their masks, rank them inside the workgroup (popcount per lane,
//                  prefix across the wave, the waves' sums through LDS) and store 16-byte records at start[pair] + offset[pair][chunk] + rank.
//   keys launch    the split k-mer of every record from the array's key column, the hash undone.
//
// No atomics and no sort: the order (pair, row) is the layout.
#include "skx_internal.h"
#include "skx_cells.h"                                              // u32x4
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace skx {
namespace {

constexpr uint32_t SITES_CHUNK = 4096;                              // columns of a work unit: 256 lanes x 16
constexpr uint64_t SITES_MAX_GRID = 1u << 20;                       // workgroups of a launch; a workgroup strides over the units beyond

struct SitesArgs {
    const uint8_t *matrix; uint64_t pitch, n_cols;
    const uint8_t *keep;                                            // [n_cols rounded up to 16] 1: the column is swept
    const uint32_t *ij; uint64_t n_pairs, n_chunks;
    uint32_t *cnt;                                                  // [n_pairs][n_chunks] sites of the unit
    const uint32_t *incl;                                           // the inclusive scan of cnt, modulo 2^32
    const uint64_t *pair_start;                                     // [n_pairs] where a pair's records begin
    skx_pair_site *rec; uint64_t cap;
};

// A, C, G or T (65, 67, 71, 84: 64 + bit 1, 3, 7, 20)
__device__ inline uint32_t one_base(uint32_t b) { return (uint32_t)((b >> 5) == 2u) & (0x0010008Au >> (b & 31u)); }

// bit t of the result: column c0 + t is a site of the pair whose rows are x and y
__device__ inline uint32_t site_mask(const u32x4 x, const u32x4 y, const u32x4 k, uint32_t valid)
{
    uint32_t m = 0;
#pragma unroll
    for (int t = 0; t < 16; t++) {
        const uint32_t sh = 8 * (t & 3), a = (x[t >> 2] >> sh) & 0xFFu, b = (y[t >> 2] >> sh) & 0xFFu, f = (k[t >> 2] >> sh) & 0xFFu;
        m |= (one_base(a) & one_base(b) & (uint32_t)(a != b) & (uint32_t)(f == 1u)) << t;
    }
    return m & valid;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void sites_kernel(SitesArgs a)
{
    __shared__ uint32_t s_wave[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t units = a.n_pairs * a.n_chunks;
    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {      // (the same trip count for every lane of the workgroup)
        const uint64_t chunk = u / a.n_pairs, pair = u - chunk * a.n_pairs, slot = pair * a.n_chunks + chunk;
        uint32_t have = 0;
        if (WRITE) { have = a.cnt[slot]; if (!have) continue; }     // (uniform: no barrier is skipped by a part of the workgroup)
        const uint64_t c0 = chunk * SITES_CHUNK + (uint64_t)threadIdx.x * 16;
        // a lane past the last column loads nothing: its columns read as '-'.  Rows are padded to the pitch (>= 256 bytes past n_cols) and the
        // flags to 16, so the 16-byte loads of a lane with c0 < n_cols stay inside
        const bool live = c0 < a.n_cols;
        const uint32_t valid = !live ? 0u : (a.n_cols - c0 >= 16 ? 0xFFFFu : (1u << (uint32_t)(a.n_cols - c0)) - 1u);
        u32x4 x{0, 0, 0, 0}, y{0, 0, 0, 0}, k{0, 0, 0, 0};
        if (live) {
            const uint64_t i = a.ij[2 * pair], j = a.ij[2 * pair + 1];
            x = *reinterpret_cast<const u32x4 *>(a.matrix + i * a.pitch + c0);
            y = *reinterpret_cast<const u32x4 *>(a.matrix + j * a.pitch + c0);
            k = *reinterpret_cast<const u32x4 *>(a.keep + c0);
        }
        const uint32_t m = site_mask(x, y, k, valid), n = __popc(m);
        if (!WRITE) {
            uint32_t sum = n;
            for (int d = 32; d; d >>= 1) sum += __shfl_down(sum, d, 64);
            if (lane == 0) s_wave[wave] = sum;
            __syncthreads();
            if (threadIdx.x == 0) a.cnt[slot] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
            __syncthreads();                                        // (s_wave is the next unit's too)
        } else {
            uint32_t incl = n;
            for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
            if (lane == 63) s_wave[wave] = incl;
            __syncthreads();
            uint32_t before = incl - n;
            for (int w = 0; w < wave; w++) before += s_wave[w];
            __syncthreads();
            if (!m) continue;                                       // (after the barriers)
            const uint32_t in_pair = a.incl[slot] - have - (pair ? a.incl[pair * a.n_chunks - 1] : 0u);      // modulo 2^32
            uint64_t pos = a.pair_start[pair] + in_pair + before;
            const uint32_t p32 = (uint32_t)pair;
#pragma unroll
            for (int t = 0; t < 16; t++) {
                if (!((m >> t) & 1u)) continue;
                if (pos < a.cap) {                                  // (the count launch sized the buffer: never false)
                    const uint32_t sh = 8 * (t & 3), bi = (x[t >> 2] >> sh) & 0xFFu, bj = (y[t >> 2] >> sh) & 0xFFu;
                    const uint64_t row = c0 + t;
                    *reinterpret_cast<u32x4 *>(a.rec + pos) = u32x4{(uint32_t)row, (uint32_t)(row >> 32), p32, bi | (bj << 8)};
                }
                pos++;
            }
        }
    }
}

// tot[p] = the sites of pair p over all chunks; one wave a pair
__global__ __launch_bounds__(64) void pair_totals_kernel(const uint32_t *cnt, uint64_t n_pairs, uint64_t n_chunks, unsigned long long *tot)
{
    for (uint64_t p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        unsigned long long sum = 0;
        for (uint64_t c = threadIdx.x; c < n_chunks; c += 64) sum += cnt[p * n_chunks + c];
        for (int d = 32; d; d >>= 1) sum += __shfl_down(sum, d, 64);
        if (threadIdx.x == 0) tot[p] = sum;
    }
}

// out[n] = the split k-mer of record n's row: the packed word of the key column (H(key) << 4 | 1), the hash undone
template <bool WIDE>
__global__ __launch_bounds__(256) void sites_keys_kernel(const skx_pair_site *rec, uint64_t n, const uint64_t *words, HashParams hp, WideHash wh, skx_key *out)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t row = rec[i].row;
    skx_key k{0, 0};
    if (!WIDE) k.lo = hunmix(words[row] >> 4, hp);
    else {
        const u128 key = hunmix_w((((u128)words[2 * row + 1] << 64) | words[2 * row]) >> 4, wh);
        k.lo = (uint64_t)key; k.hi = (uint64_t)(key >> 64);
    }
    out[i] = k;
}

}  // namespace
}  // namespace skx

using namespace skx;

static_assert(sizeof(skx_pair_site) == 16 && offsetof(skx_pair_site, pair) == 8 && offsetof(skx_pair_site, base_i) == 12 && offsetof(skx_pair_site, base_j) == 13,
              "sites_kernel stores a record as four 32-bit words");

extern "C" int skx_array_pair_sites(skx_array *a, double min_freq, const uint32_t *ij, uint64_t n_pairs, uint64_t max_records,
                                    skx_pair_site **records, skx_key **keys, uint64_t *counts, uint64_t *n)
{
    return skx_guarded([&]() -> int {
    if (records) *records = nullptr;
    if (keys) *keys = nullptr;
    if (n) *n = 0;
    if (!a || !records || !n || (n_pairs && !ij)) { set_error("pair sites: bad arguments"); return SKX_EINVAL; }
    if (!(min_freq >= 0.0 && min_freq <= 1.0)) { set_error("pair sites: min_freq must be between 0 and 1 (inclusive)"); return SKX_EINVAL; }
    const uint64_t S = a->names.size();
    for (uint64_t p = 0; p < n_pairs; p++) {
        const uint32_t i = ij[2 * p], j = ij[2 * p + 1];
        if (i >= j) { set_error("pair sites: pair %llu is (%u, %u); the first sample must come before the second", (unsigned long long)p, i, j); return SKX_EINVAL; }
        if (j >= S) { set_error("pair sites: pair %llu is (%u, %u); the array has %llu samples", (unsigned long long)p, i, j, (unsigned long long)S); return SKX_EINVAL; }
    }
    if (keys && (a->keys_absent || a->n_kmers != a->n_rows)) {
        set_error("pair sites: this array holds no split k-mers for its rows (loaded or filtered without them)"); return SKX_EINVAL;
    }
    if (n_pairs > 0xFFFFFFFFull) { set_error("pair sites: %llu pairs; a record's pair index holds 32 bits", (unsigned long long)n_pairs); return SKX_EUNSUP; }
    if (a->total_samples && a->total_samples != S) { set_error("pair sites: needs every sample of the array on one device"); return SKX_EUNSUP; }
    if (counts) for (uint64_t p = 0; p < n_pairs; p++) counts[p] = 0;
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    SKX_TRY(array_materialize(a));
    const uint64_t U = a->n_rows;
    if (U > (1ull << 32)) { set_error("pair sites: %llu rows; at most 2^32 are taken", (unsigned long long)U); return SKX_EUNSUP; }
    if (!n_pairs || !U) return SKX_OK;

    const uint64_t n_chunks = (U + SITES_CHUNK - 1) / SITES_CHUNK, units = n_pairs * n_chunks;
    DevBuf<uint8_t> keep; DevBuf<uint32_t> d_ij, cnt, incl; DevBuf<unsigned long long> d_tot; DevBuf<uint64_t> d_start;
    std::vector<unsigned long long> tot(n_pairs);
    SitesArgs ka{};
    const unsigned grid = (unsigned)std::min<uint64_t>(units, SITES_MAX_GRID);
    {
        PhaseTimer tc("distance.sites_count");
        const uint64_t Upad = (U + 15) / 16 * 16;
        SKX_TRY(keep.alloc(Upad)); SKX_TRY(keep.zero(st));
        SKX_TRY(d_ij.alloc(2 * n_pairs)); SKX_TRY(d_tot.alloc(n_pairs)); SKX_TRY(d_start.alloc(n_pairs));
        if (cnt.alloc(units) != SKX_OK || incl.alloc(units) != SKX_OK) {
            set_error("pair sites: the counters of %llu pairs x %llu chunks of rows (%llu MB) do not fit in device memory", (unsigned long long)n_pairs,
                      (unsigned long long)n_chunks, (unsigned long long)(units * 8 >> 20));
            return SKX_ENOMEM;
        }
        distance_filter_flags(a, min_freq, keep.p, st);
        SKX_HIP(hipMemcpyAsync(d_ij.p, ij, 2 * n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        ka.matrix = a->matrix.p; ka.pitch = a->pitch; ka.n_cols = U; ka.keep = keep.p; ka.ij = d_ij.p; ka.n_pairs = n_pairs; ka.n_chunks = n_chunks;
        ka.cnt = cnt.p; ka.incl = incl.p; ka.pair_start = d_start.p;
        hipLaunchKernelGGL(sites_kernel<false>, dim3(grid), dim3(256), 0, st, ka);
        SKX_HIP(hipGetLastError());
        hipLaunchKernelGGL(pair_totals_kernel, dim3((unsigned)std::min<uint64_t>(n_pairs, SITES_MAX_GRID)), dim3(64), 0, st, cnt.p, n_pairs, n_chunks, d_tot.p);
        SKX_HIP(hipGetLastError());
        SKX_HIP(hipMemcpyAsync(tot.data(), d_tot.p, n_pairs * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        SKX_TRY(prim_scan_add_u32(cnt.p, incl.p, units, st));       // (returns with the stream idle: the totals are here)
    }
    std::vector<uint64_t> start(n_pairs);
    uint64_t total = 0;
    for (uint64_t p = 0; p < n_pairs; p++) { start[p] = total; total += tot[p]; if (counts) counts[p] = tot[p]; }
    if (!total) return SKX_OK;
    if (max_records && total > max_records) {
        set_error("pair sites: %llu records; the limit is %llu", (unsigned long long)total, (unsigned long long)max_records); return SKX_ENOMEM;
    }

    // the records: their number is known, so everything that holds them is sized (or refused) before the write launch runs
    PhaseTimer tw("distance.sites_write");
    skx_pair_site *h_rec = (skx_pair_site *)malloc(total * sizeof(skx_pair_site));
    skx_key *h_keys = keys ? (skx_key *)malloc(total * sizeof(skx_key)) : nullptr;
    struct Guard { skx_pair_site *r; skx_key *k; ~Guard() { free(r); free(k); } } guard{h_rec, h_keys};
    if (!h_rec || (keys && !h_keys)) { set_error("pair sites: %llu records do not fit in host memory", (unsigned long long)total); return SKX_ENOMEM; }
    const bool keys_on_host = keys && a->k > 31 && !a->host_keys.empty();      // (arrays loaded from k > 31 files keep their keys there)
    DevBuf<skx_pair_site> d_rec; DevBuf<skx_key> d_keys;
    if (d_rec.alloc(total) != SKX_OK || (keys && !keys_on_host && d_keys.alloc(total) != SKX_OK)) {
        set_error("pair sites: %llu records (%llu MB) do not fit in device memory", (unsigned long long)total, (unsigned long long)(total * (keys ? 32 : 16) >> 20));
        return SKX_ENOMEM;
    }
    SKX_HIP(hipMemcpyAsync(d_start.p, start.data(), n_pairs * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    ka.rec = d_rec.p; ka.cap = total;
    hipLaunchKernelGGL(sites_kernel<true>, dim3(grid), dim3(256), 0, st, ka);
    SKX_HIP(hipGetLastError());
    SKX_HIP(hipMemcpyAsync(h_rec, d_rec.p, total * sizeof(skx_pair_site), hipMemcpyDeviceToHost, st));
    if (keys && !keys_on_host) {
        const dim3 kgrid((unsigned)((total + 255) / 256));
        if (a->k <= 31) hipLaunchKernelGGL(sites_keys_kernel<false>, kgrid, dim3(256), 0, st, d_rec.p, total, a->keys.p, a->hp, a->wh, d_keys.p);
        else hipLaunchKernelGGL(sites_keys_kernel<true>, kgrid, dim3(256), 0, st, d_rec.p, total, a->keys.p, a->hp, a->wh, d_keys.p);
        SKX_HIP(hipGetLastError());
        SKX_HIP(hipMemcpyAsync(h_keys, d_keys.p, total * sizeof(skx_key), hipMemcpyDeviceToHost, st));
    }
    SKX_HIP(hipStreamSynchronize(st));                              // (start is a local)
    if (keys_on_host) for (uint64_t r = 0; r < total; r++) h_keys[r] = a->host_keys[h_rec[r].row];
    guard.r = nullptr; guard.k = nullptr;
    *records = h_rec; if (keys) *keys = h_keys;
    *n = total;
    return SKX_OK;
    });
}
