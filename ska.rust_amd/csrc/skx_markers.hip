// skx_markers.hip -- `ska markers`: the split k-mers (presence markers) and middle-base alleles (allele markers) that tell a group of samples from
// everybody else, for every group of a partition at once (skx_array_group_markers, include/skx.h; definition there and in tests/markers_model.py).
// The reference has no counterpart: its users chain `ska delete` of a group (merge_ska_array.rs:231-271) and `ska nk --full-info` (:649-698) once
// per group and compare the text.
//
// The matrix is sample-major, so a row of the reference is a column here.  A thread owns 16 consecutive columns (one 16-byte load per sample, inside
// the row's padding) and walks the samples segment by segment through a device order list -- the order[] of subset_verdict_kernel, sorted by segment.
//
//   walk 1   every sample.  Per column: cells present; per base the first segment that has it (16 bits) and whether a later segment has it too.
//            That answers "which bases do the samples outside segment g hold" for every g from 12 bytes a column:
//            base b is outside g  <=>  first[b] is a segment other than g, or a second segment has b.
//   walk 2   the samples of the reported groups again (the 4 096 columns x S cells a workgroup has just read).  At a segment's end `in` and `bases_in`
//            are in registers, out = present - in, and the verdicts of the 16 columns are decided.
//
// markers_kernel<false> runs both walks, keeps walk 1's state (12 bytes a column) and counts the markers per group and kind (wave sums, integer
// atomics) and per workgroup: the exact number of records is known before their buffer exists, and every workgroup has a range of its own in it.
// markers_kernel<true> reads the state back, repeats walk 2 and appends the records inside the workgroup's range (a cursor in LDS, one LDS atomic
// per wave and segment: no two workgroups share an address) with the word group << 32 | row; the engine's radix sort (skx_prims.hip) then orders
// them by that word, which is unique per record -- so the same input gives the same bytes whatever the arrival order.  The matrix is read three
// times (less what the caches keep), whatever the number of groups; device memory beside the array is 12 U bytes of state, 12 bytes a workgroup
// (4 096 columns), 16 bytes a group and 68 bytes a record while they are sorted.  No per-(group, row) table exists.
#include "skx_internal.h"
#include "skx_cells.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace skx {
namespace {

constexpr uint32_t NO_SEG = 0xFFFFu;

// a reported group's run of the second order list: it ends at `end`, was segment `seg` of walk 1, is group `group` of the caller
struct MarkerSeg { uint32_t end, seg, group, t_in, t_out; };

struct MarkerArgs {
    const uint8_t *matrix; uint64_t pitch, n_cols;
    const int *order1; const uint32_t *end1; uint32_t n1;           // walk 1: every sample, segment by segment; end1[k] = where segment k ends
    const int *order2; const MarkerSeg *seg2; uint32_t n2;          // walk 2: the samples of the reported groups
    int kinds;
    uint2 *first; uint32_t *tot;                                    // [n_cols rounded up to 16] walk 1's state
    unsigned long long *counts;                                     // [2 * n_groups] presence, allele
    uint32_t *blk_count; const uint64_t *blk_off;                   // [workgroups] records of the workgroup's columns; where they start
    skx_marker *rec; unsigned long long *keys; uint32_t *vals; uint64_t cap;
    int *bad_byte;
};

// acc[i] of a thread's 16 columns: cells present in the low 16 bits (at most 65 535 samples), the OR of their codes from bit 16
__device__ inline void absorb(const u32x4 cur, const uint8_t *lut, uint32_t (&acc)[16], uint32_t &bad)
{
#pragma unroll
    for (int i = 0; i < 16; i++) {
        uint32_t code = lut[(cur[i >> 2] >> (8 * (i & 3))) & 0xFFu];
        if (code == 0xFF) { bad |= 1u << i; code = 0; }
        acc[i] = (acc[i] + (code != 0 ? 1u : 0u)) | (code << 16);
    }
}

// the bases the samples outside segment k hold, from walk 1's state of one column
__device__ inline uint32_t bases_outside(uint32_t f01, uint32_t f23, uint32_t tot, uint32_t k)
{
    const uint32_t f[4] = {f01 & 0xFFFFu, f01 >> 16, f23 & 0xFFFFu, f23 >> 16};
    uint32_t o = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) o |= (uint32_t)((f[b] != NO_SEG && f[b] != k) || ((tot >> (16 + b)) & 1u)) << b;
    return o;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void markers_kernel(MarkerArgs a)
{
    __shared__ uint8_t s_lut[256];                                  // the IUPAC set code of cell_code; 0xFF: a byte outside the alphabet
    __shared__ uint32_t s_records;                                  // count pass: the workgroup's records; write pass: how many it has placed
    {
        const uint32_t c = cell_code(threadIdx.x);
        s_lut[threadIdx.x] = (uint8_t)(c == CELL_OUTSIDE ? 0xFFu : c);
    }
    if (threadIdx.x == 0) s_records = 0;
    __syncthreads();
    const uint64_t c0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    const int lane = threadIdx.x & 63;
    // a thread past the last column walks column 0 and decides nothing (ColumnLane, skx_cells.h); a bit of `valid` a column below n_cols
    const ColumnLane me(a.matrix, a.n_cols, c0);
    const bool live = me.live;
    const uint8_t *col = me.col;
    const uint32_t valid = !live ? 0u : (a.n_cols - c0 >= 16 ? 0xFFFFu : (1u << (uint32_t)(a.n_cols - c0)) - 1u);
    uint32_t acc[16], tot[16], f01[16], f23[16];
    uint32_t bad = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) { acc[i] = 0; tot[i] = 0; f01[i] = 0xFFFFFFFFu; f23[i] = 0xFFFFFFFFu; }
    auto load = [&](const int *order, uint32_t n, uint32_t p) -> u32x4 {
        return p < n ? *reinterpret_cast<const u32x4 *>(col + (uint64_t)order[p] * a.pitch) : u32x4{0, 0, 0, 0};
    };

    if (!WRITE) {
        // ---- walk 1: four samples' loads in flight across the segment ends
        u32x4 b0 = load(a.order1, a.n1, 0), b1 = load(a.order1, a.n1, 1), b2 = load(a.order1, a.n1, 2), b3 = load(a.order1, a.n1, 3);
        uint32_t k = 0, end = a.n1 ? a.end1[0] : 0;
        for (uint32_t p = 0; p < a.n1; p++) {
            const u32x4 cur = b0;
            b0 = b1; b1 = b2; b2 = b3; b3 = load(a.order1, a.n1, p + 4);
            absorb(cur, s_lut, acc, bad);
            if (p + 1 == end) {
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const uint32_t sb = acc[i] >> 16;
                    tot[i] += acc[i] & 0xFFFFu;
                    if (sb & 1u) { if ((f01[i] & 0xFFFFu) == NO_SEG) f01[i] = (f01[i] & 0xFFFF0000u) | k; else tot[i] |= 1u << 16; }
                    if (sb & 2u) { if ((f01[i] >> 16) == NO_SEG) f01[i] = (f01[i] & 0xFFFFu) | (k << 16); else tot[i] |= 2u << 16; }
                    if (sb & 4u) { if ((f23[i] & 0xFFFFu) == NO_SEG) f23[i] = (f23[i] & 0xFFFF0000u) | k; else tot[i] |= 4u << 16; }
                    if (sb & 8u) { if ((f23[i] >> 16) == NO_SEG) f23[i] = (f23[i] & 0xFFFFu) | (k << 16); else tot[i] |= 8u << 16; }
                    acc[i] = 0;
                }
                k++;
                end = p + 1 < a.n1 ? a.end1[k] : 0;
            }
        }
        if (live) {                                                 // (the state arrays are padded to 16 columns)
#pragma unroll
            for (int i = 0; i < 16; i += 2) *reinterpret_cast<uint4 *>(a.first + c0 + i) = uint4{f01[i], f23[i], f01[i + 1], f23[i + 1]};
#pragma unroll
            for (int i = 0; i < 16; i += 4) *reinterpret_cast<uint4 *>(a.tot + c0 + i) = uint4{tot[i], tot[i + 1], tot[i + 2], tot[i + 3]};
            if (bad & valid) *a.bad_byte = 1;
        }
    } else if (live) {
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
            const uint4 f = *reinterpret_cast<const uint4 *>(a.first + c0 + i);
            f01[i] = f.x; f23[i] = f.y; f01[i + 1] = f.z; f23[i + 1] = f.w;
        }
#pragma unroll
        for (int i = 0; i < 16; i += 4) {
            const uint4 t = *reinterpret_cast<const uint4 *>(a.tot + c0 + i);
            tot[i] = t.x; tot[i + 1] = t.y; tot[i + 2] = t.z; tot[i + 3] = t.w;
        }
    }

    // ---- walk 2: the reported groups
    u32x4 b0 = load(a.order2, a.n2, 0), b1 = load(a.order2, a.n2, 1), b2 = load(a.order2, a.n2, 2), b3 = load(a.order2, a.n2, 3);
    uint32_t q = 0;
    MarkerSeg sg = a.n2 ? a.seg2[0] : MarkerSeg{0, 0, 0, 0, 0};
    for (uint32_t p = 0; p < a.n2; p++) {
        const u32x4 cur = b0;
        b0 = b1; b1 = b2; b2 = b3; b3 = load(a.order2, a.n2, p + 4);
        absorb(cur, s_lut, acc, bad);
        if (p + 1 != sg.end) continue;
        uint32_t pm = 0, am = 0;                                    // bit i: column c0 + i is a presence / an allele marker of this group
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t in = acc[i] & 0xFFFFu, bin = acc[i] >> 16, out = (tot[i] & 0xFFFFu) - in;
            const bool ok = ((valid >> i) & 1u) && in >= sg.t_in, pres = ok && out <= sg.t_out;
            const bool alle = ok && !pres && (bin & bases_outside(f01[i], f23[i], tot[i], sg.seg)) == 0;
            pm |= (uint32_t)pres << i; am |= (uint32_t)alle << i;
        }
        if (!(a.kinds & 1)) pm = 0;
        if (!(a.kinds & 2)) am = 0;
        const uint32_t mm = pm | am;
        if (__ballot(mm != 0) != 0) {                               // (the same for the whole wave)
            if (!WRITE) {
                uint32_t np = __popc(pm), na = __popc(am);
                for (int d = 32; d; d >>= 1) { np += __shfl_down(np, d, 64); na += __shfl_down(na, d, 64); }
                if (lane == 0) {
                    if (np) atomicAdd(&a.counts[2 * (uint64_t)sg.group], (unsigned long long)np);
                    if (na) atomicAdd(&a.counts[2 * (uint64_t)sg.group + 1], (unsigned long long)na);
                    atomicAdd(&s_records, np + na);
                }
            } else {
                const uint32_t cnt = __popc(mm);
                uint32_t incl = cnt;
                for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
                const uint32_t total = __shfl(incl, 63, 64);
                uint32_t base = 0;
                if (lane == 63) base = atomicAdd(&s_records, total);
                base = __shfl(base, 63, 64);
                uint64_t pos = a.blk_off[blockIdx.x] + base + (incl - cnt);
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    if (!((mm >> i) & 1u)) continue;
                    if (pos < a.cap) {                              // (the count pass sized the buffer: never false)
                        const uint32_t in = acc[i] & 0xFFFFu;
                        skx_marker r;
                        r.row = c0 + i; r.group = sg.group; r.n_in = in; r.n_out = (tot[i] & 0xFFFFu) - in;
                        r.kind = (uint8_t)(((pm >> i) & 1u) ? 1 : 2); r.bases_in = (uint8_t)(acc[i] >> 16);
                        r.bases_out = (uint8_t)bases_outside(f01[i], f23[i], tot[i], sg.seg); r.reserved = 0;
                        a.rec[pos] = r;
                        a.keys[pos] = ((unsigned long long)sg.group << 32) | (unsigned long long)(c0 + i);
                        a.vals[pos] = (uint32_t)pos;
                    }
                    pos++;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 16; i++) acc[i] = 0;
        q++;
        if (p + 1 < a.n2) sg = a.seg2[q];
    }
    if (!WRITE) {
        __syncthreads();
        if (threadIdx.x == 0) a.blk_count[blockIdx.x] = s_records;
    }
}

__global__ void markers_gather_kernel(const skx_marker *in, const uint32_t *perm, skx_marker *out, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[perm[i]];
}

}  // namespace
}  // namespace skx

using namespace skx;

extern "C" int skx_array_group_markers(skx_array *a, const int32_t *segment_of, int n_groups, const uint8_t *reported, double min_in, double max_out, int kinds,
                                       skx_marker **records, skx_key **keys, uint64_t *n, skx_marker_info *info)
{
    return skx_guarded([&]() -> int {
    if (records) *records = nullptr;
    if (keys) *keys = nullptr;
    if (n) *n = 0;
    if (!a || !segment_of || n_groups < 0 || (n_groups > 0 && !reported) || !records || !keys || !n) { set_error("markers: bad arguments"); return SKX_EINVAL; }
    if (!(min_in >= 0.0 && min_in <= 1.0)) { set_error("markers: min_in must be between 0 and 1 (inclusive)"); return SKX_EINVAL; }
    if (!(max_out >= 0.0 && max_out <= 1.0)) { set_error("markers: max_out must be between 0 and 1 (inclusive)"); return SKX_EINVAL; }
    if (kinds == 0 || (kinds & ~(SKX_MARKER_PRESENCE | SKX_MARKER_ALLELE))) { set_error("markers: kinds must name presence (1), allele (2) or both (3)"); return SKX_EINVAL; }
    if (a->keys_absent || a->n_kmers != a->n_rows) { set_error("markers: this array holds no split k-mers for its rows (loaded or filtered without them)"); return SKX_EINVAL; }
    const uint64_t S = a->names.size();
    if (S > 65535) { set_error("markers: %llu samples; at most 65535 are taken (16-bit counts)", (unsigned long long)S); return SKX_EUNSUP; }
    if (n_groups > 65534) { set_error("markers: %d groups; at most 65535 segments are taken", n_groups); return SKX_EUNSUP; }
    if (a->total_samples && a->total_samples != S) { set_error("markers: needs every sample of the array on one device"); return SKX_EUNSUP; }
    // the partition: segment g < n_groups = group g, segment n_groups = the samples no group lists
    std::vector<std::vector<int>> members((size_t)n_groups + 1);
    for (uint64_t s = 0; s < S; s++) {
        if (segment_of[s] < 0 || segment_of[s] > n_groups) { set_error("markers: segment %d of sample %llu out of range (%d groups)", segment_of[s], (unsigned long long)s, n_groups); return SKX_EINVAL; }
        members[segment_of[s]].push_back((int)s);
    }
    for (int g = 0; g < n_groups; g++)
        if (reported[g] && members[g].empty()) { set_error("markers: reported group %d has no samples", g); return SKX_EINVAL; }
    std::vector<int> order1, order2; std::vector<uint32_t> end1; std::vector<MarkerSeg> seg2;
    for (int g = 0; g <= n_groups; g++) {
        if (members[g].empty()) continue;
        const uint32_t seg = (uint32_t)end1.size();
        order1.insert(order1.end(), members[g].begin(), members[g].end());
        end1.push_back((uint32_t)order1.size());
        if (g == n_groups || !reported[g]) continue;
        const double m = (double)members[g].size();
        const uint64_t t_in = std::max<uint64_t>(1, (uint64_t)std::ceil(m * min_in)), t_out = (uint64_t)std::floor(((double)S - m) * max_out);
        order2.insert(order2.end(), members[g].begin(), members[g].end());
        seg2.push_back(MarkerSeg{(uint32_t)order2.size(), seg, (uint32_t)g, (uint32_t)t_in, (uint32_t)t_out});
    }
    if (info) for (int g = 0; g < n_groups; g++) info[g] = skx_marker_info{0, 0};
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    SKX_TRY(array_materialize(a));
    const uint64_t U = a->n_rows;
    if (U >= (1ull << 32)) { set_error("markers: %llu rows; a record's sort word holds 32 bits of row", (unsigned long long)U); return SKX_EUNSUP; }
    if (!U || seg2.empty()) return SKX_OK;

    const uint64_t Upad = (U + 15) / 16 * 16;
    DevBuf<int> d_order1, d_order2, d_bad; DevBuf<uint32_t> d_end1, d_tot; DevBuf<MarkerSeg> d_seg2; DevBuf<uint2> d_first;
    DevBuf<unsigned long long> d_counts; DevBuf<uint32_t> d_blk_count; DevBuf<uint64_t> d_blk_off;
    const uint64_t n_blocks = (U + 4095) / 4096;
    SKX_TRY(d_order1.alloc(order1.size())); SKX_TRY(d_order2.alloc(order2.size())); SKX_TRY(d_end1.alloc(end1.size())); SKX_TRY(d_seg2.alloc(seg2.size()));
    SKX_TRY(d_first.alloc(Upad)); SKX_TRY(d_tot.alloc(Upad)); SKX_TRY(d_bad.alloc(1)); SKX_TRY(d_bad.zero(st));
    SKX_TRY(d_counts.alloc(2 * (size_t)n_groups)); SKX_TRY(d_counts.zero(st)); SKX_TRY(d_blk_count.alloc(n_blocks)); SKX_TRY(d_blk_off.alloc(n_blocks));
    SKX_HIP(hipMemcpyAsync(d_order1.p, order1.data(), order1.size() * sizeof(int), hipMemcpyHostToDevice, st));
    SKX_HIP(hipMemcpyAsync(d_order2.p, order2.data(), order2.size() * sizeof(int), hipMemcpyHostToDevice, st));
    SKX_HIP(hipMemcpyAsync(d_end1.p, end1.data(), end1.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    SKX_HIP(hipMemcpyAsync(d_seg2.p, seg2.data(), seg2.size() * sizeof(MarkerSeg), hipMemcpyHostToDevice, st));
    MarkerArgs ka{};
    ka.matrix = a->matrix.p; ka.pitch = a->pitch; ka.n_cols = U;
    ka.order1 = d_order1.p; ka.end1 = d_end1.p; ka.n1 = (uint32_t)order1.size();
    ka.order2 = d_order2.p; ka.seg2 = d_seg2.p; ka.n2 = (uint32_t)order2.size();
    ka.kinds = kinds; ka.first = d_first.p; ka.tot = d_tot.p; ka.counts = d_counts.p; ka.blk_count = d_blk_count.p; ka.blk_off = d_blk_off.p; ka.bad_byte = d_bad.p;
    const dim3 grid((unsigned)n_blocks);
    hipLaunchKernelGGL(markers_kernel<false>, grid, dim3(256), 0, st, ka);
    SKX_HIP(hipGetLastError());
    std::vector<unsigned long long> counts(2 * (size_t)n_groups, 0);
    std::vector<uint32_t> blk_count(n_blocks); std::vector<uint64_t> blk_off(n_blocks);
    int bad = 0;
    SKX_HIP(hipMemcpyAsync(blk_count.data(), d_blk_count.p, n_blocks * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SKX_HIP(hipMemcpyAsync(counts.data(), d_counts.p, counts.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    SKX_HIP(hipMemcpyAsync(&bad, d_bad.p, 4, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    if (bad) { set_error("variants contain a byte outside -ACGTMRWSYKVHDBN (not supported on the device path)"); return SKX_EUNSUP; }
    uint64_t total = 0;
    for (int g = 0; g < n_groups; g++) { total += counts[2 * g] + counts[2 * g + 1]; if (info) info[g] = skx_marker_info{counts[2 * g], counts[2 * g + 1]}; }
    if (!total) return SKX_OK;
    uint64_t placed = 0;
    for (uint64_t b = 0; b < n_blocks; b++) { blk_off[b] = placed; placed += blk_count[b]; }
    if (placed != total) { set_error("markers: internal error: %llu records counted per group, %llu per workgroup", (unsigned long long)total, (unsigned long long)placed); return SKX_EINVAL; }

    // the records: their number is known, so everything that holds them is sized (or refused) before the second pass runs
    if (total > 0xFFFFFFF0ull) { set_error("markers: %llu records; at most 2^32 - 16 are taken in one call", (unsigned long long)total); return SKX_EUNSUP; }
    skx_marker *h_rec = (skx_marker *)malloc(total * sizeof(skx_marker));
    skx_key *h_keys = (skx_key *)malloc(total * sizeof(skx_key));
    struct Guard { skx_marker *r; skx_key *k; ~Guard() { free(r); free(k); } } guard{h_rec, h_keys};
    if (!h_rec || !h_keys) { set_error("markers: %llu records do not fit in host memory", (unsigned long long)total); return SKX_ENOMEM; }
    DevBuf<skx_marker> d_rec, d_out; DevBuf<unsigned long long> d_keys, d_skeys; DevBuf<uint32_t> d_vals, d_svals;
    if (d_rec.alloc(total) != SKX_OK || d_out.alloc(total) != SKX_OK || d_keys.alloc(total) != SKX_OK || d_skeys.alloc(total) != SKX_OK ||
        d_vals.alloc(total) != SKX_OK || d_svals.alloc(total) != SKX_OK) {
        set_error("markers: %llu records (%llu MB with their sort) do not fit in device memory", (unsigned long long)total,
                  (unsigned long long)(total * (2 * sizeof(skx_marker) + 24) >> 20));
        return SKX_ENOMEM;
    }
    ka.rec = d_rec.p; ka.keys = d_keys.p; ka.vals = d_vals.p; ka.cap = total;
    SKX_HIP(hipMemcpyAsync(d_blk_off.p, blk_off.data(), n_blocks * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(markers_kernel<true>, grid, dim3(256), 0, st, ka);
    SKX_HIP(hipGetLastError());
    int gbits = 1; while (gbits < 16 && (1 << gbits) < n_groups) gbits++;
    SKX_TRY(prim_sort_pairs_u64((const uint64_t *)d_keys.p, (uint64_t *)d_skeys.p, d_vals.p, d_svals.p, total, 32 + gbits, st));
    hipLaunchKernelGGL(markers_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_rec.p, d_svals.p, d_out.p, total);
    SKX_HIP(hipGetLastError());
    SKX_HIP(hipMemcpyAsync(h_rec, d_out.p, total * sizeof(skx_marker), hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    std::vector<skx_key> hk;
    SKX_TRY(array_host_keys(a, hk));                                // the rows' split k-mers as skx_array_export gives them (H inverted)
    for (uint64_t i = 0; i < total; i++) h_keys[i] = hk[h_rec[i].row];
    guard.r = nullptr; guard.k = nullptr;
    *records = h_rec; *keys = h_keys; *n = total;
    return SKX_OK;
    });
}
