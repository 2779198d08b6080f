// skx_qc.hip -- `ska qc`: six counts per sample that each depend on a statistic of the row a cell sits in (skx_array_sample_qc, include/skx.h;
// definition there and in tests/qc_model.py).  The reference has no counterpart: `ska nk` (lib.rs:808-827) prints one k-mer count per sample.
//
// The matrix is sample-major, so a row of the reference is a column here.  Two launches, integer atomics only:
//
// qc_rows_kernel reads the matrix once.  A thread owns 16 consecutive columns (one 16-byte load per sample, inside the row's padding), a workgroup
// 4 096, and walks the samples with four loads in flight (ColumnLane and walk_columns, skx_cells.h).  Per column five 16-bit counters in three registers -- n | c[A] << 16, c[C] | c[T] << 16, c[G] | bad << 16 -- fed by three words of an
// LDS table per cell (one address, three adds, no comparison).  After the last sample a column's counters become its 16-bit descriptor (D_* below),
// stored 32 bytes a lane, and the three row totals are counted as lane masks in scalar registers and added through LDS to 64-bit counters.
//
// qc_samples_kernel runs over units of (SKX_QC_TILE_ROWS columns, SKX_QC_SAMPLES samples), the sample blocks fastest along the grid so that the
// units in flight share their descriptors.  A thread turns its 16 descriptors into two masks per column once; per sample and cell two words of an
// LDS table are added (kmers, ambiguous) or masked and added (the base one-hot in fields of five bits against the column's private and minor
// masks; the present bit against core and singleton): five vector instructions a cell behind the table read.  A lane's sums over its 16 columns
// (at most 16 a count) are packed into two words of three 10-bit fields, summed over each half of the wave by five DPP adds (at most 512 a
// field), and lanes 0-5 add the two halves' fields to the unit's [SKX_QC_SAMPLES][6] block in LDS, which the workgroup adds to the samples'
// 64-bit counters at its end: one atomic per (sample, count) and unit.  The other form of the wave sum -- a lane mask per predicate and cell,
// counted in scalar registers as curve_kernel does -- needs 96 comparisons and 96 mask counts a sample here, against 20 vector instructions.
//
// No workgroup waits for another, every loop is bounded by S or the unit, and every barrier is reached by all 256 threads: the ones past the last
// column walk column 0 behind a mask of zeros and count nothing.
//
// Device memory beside the array: 2 bytes a row (rounded up to SKX_QC_TILE_ROWS), 48 bytes a sample, 28 bytes of totals and the bad-byte flag.
#include "skx_internal.h"
#include "skx_cells.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace skx {
namespace {

constexpr uint32_t QC_THREADS = SKX_QC_TILE_ROWS / 16;
constexpr uint32_t QC_B = SKX_QC_SAMPLES;
static_assert(QC_THREADS == 256, "a workgroup of 256 threads, 16 columns each");
static_assert(QC_B % 4 == 0, "the walk is unrolled by the four loads in flight");
static_assert(SKX_QC_TILE_ROWS / 4 / 2 <= 0x3FF, "half a wave's sum of a count fits a 10-bit field");

// a row's descriptor
enum : uint32_t { D_PRESENT = 1u, D_SINGLE = 2u, D_CORE = 4u, D_VARIANT = 8u, D_PRIVATE_SHIFT = 4, D_MAJOR_SHIFT = 8 };

// a 4-bit set of bases in fields of five bits: A at bit 0, C at 5, T at 10, G at 15
__device__ inline uint32_t qc_spread(uint32_t m) { return (m & 1u) | ((m & 2u) << 4) | ((m & 4u) << 8) | ((m & 8u) << 12); }

struct QcRowsArgs {
    const uint8_t *matrix; uint64_t pitch, n_cols;
    uint32_t S, thr;
    uint16_t *desc;                                                 // [n_tiles * SKX_QC_TILE_ROWS]
    unsigned long long *totals;                                     // rows_present, core_rows, core_variant_rows
    int *bad_byte;
};

__global__ __launch_bounds__(256) void qc_rows_kernel(QcRowsArgs a)
{
    __shared__ uint32_t s_lut[3][256];                              // present | A << 16, C | T << 16, G | outside the alphabet << 16
    __shared__ uint32_t s_tot[3];
    const uint64_t c0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    const int lane = threadIdx.x & 63;
    const ColumnLane me(a.matrix, a.n_cols, c0);
    const uint32_t S = a.S;
    {
        const uint32_t c = cell_code(threadIdx.x);
        s_lut[0][threadIdx.x] = (cell_present(c) ? 1u : 0u) | (c == 1 ? 1u << 16 : 0u);
        s_lut[1][threadIdx.x] = (c == 2 ? 1u : 0u) | (c == 4 ? 1u << 16 : 0u);
        s_lut[2][threadIdx.x] = (c == 8 ? 1u : 0u) | (c == CELL_OUTSIDE ? 1u << 16 : 0u);
        if (threadIdx.x < 3) s_tot[threadIdx.x] = 0;
    }
    __syncthreads();
    uint32_t acc0[16], acc1[16], acc2[16];
#pragma unroll
    for (int i = 0; i < 16; i++) { acc0[i] = 0; acc1[i] = 0; acc2[i] = 0; }
    auto load = [&](uint32_t t) -> u32x4 { return *reinterpret_cast<const u32x4 *>(me.col + (uint64_t)min(t, S - 1) * a.pitch); };
    auto step = [&](uint32_t, const u32x4 raw) {
        const u32x4 cur = raw & me.vm;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t b = (cur[i >> 2] >> (8 * (i & 3))) & 0xFFu;
            acc0[i] += s_lut[0][b]; acc1[i] += s_lut[1][b]; acc2[i] += s_lut[2][b];      // at most 65 535 samples: no half overflows
        }
    };
    walk_columns(0, S, load, step);
    uint32_t bad = 0, n_present = 0, n_core = 0, n_core_variant = 0, d[16];
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t n = acc0[i] & 0xFFFFu, cA = acc0[i] >> 16, cC = acc1[i] & 0xFFFFu, cT = acc1[i] >> 16, cG = acc2[i] & 0xFFFFu;
        bad |= acc2[i] >> 16;
        const uint32_t unamb = cA + cC + cT + cG;
        const uint32_t once = (cA == 1 ? 1u : 0u) | (cC == 1 ? 2u : 0u) | (cT == 1 ? 4u : 0u) | (cG == 1 ? 8u : 0u);
        uint32_t best = cA, major = 1;                              // ties go to the lowest code
        if (cC > best) { best = cC; major = 2; }
        if (cT > best) { best = cT; major = 4; }
        if (cG > best) { best = cG; major = 8; }
        if (!unamb) major = 0;
        const bool present = n != 0, core = n >= a.thr, variant = (cA != 0) + (cC != 0) + (cT != 0) + (cG != 0) >= 2;      // thr >= 1: a core row is present
        d[i] = (present ? D_PRESENT : 0u) | (n == 1 ? D_SINGLE : 0u) | (core ? D_CORE : 0u) | (variant ? D_VARIANT : 0u)
             | ((unamb >= 2 ? once : 0u) << D_PRIVATE_SHIFT) | (major << D_MAJOR_SHIFT);
        n_present += (uint32_t)__popcll(__ballot(present));
        n_core += (uint32_t)__popcll(__ballot(core));
        n_core_variant += (uint32_t)__popcll(__ballot(core && variant));
    }
    // every thread stores its 16 descriptors (zeros past the last column): the buffer covers whole tiles
    u32x4 lo, hi;
#pragma unroll
    for (int w = 0; w < 4; w++) { lo[w] = d[2 * w] | (d[2 * w + 1] << 16); hi[w] = d[8 + 2 * w] | (d[9 + 2 * w] << 16); }
    u32x4 *dst = reinterpret_cast<u32x4 *>(a.desc + c0);
    dst[0] = lo; dst[1] = hi;
    if (lane == 0) {
        if (n_present) atomicAdd(&s_tot[0], n_present);
        if (n_core) atomicAdd(&s_tot[1], n_core);
        if (n_core_variant) atomicAdd(&s_tot[2], n_core_variant);
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_tot[threadIdx.x]) atomicAdd(a.totals + threadIdx.x, (unsigned long long)s_tot[threadIdx.x]);
    if (bad) *a.bad_byte = 1;
}

struct QcSamplesArgs {
    const uint8_t *matrix; uint64_t pitch, n_cols;
    const uint16_t *desc;
    uint32_t S, n_sblocks;
    unsigned long long *counts;                                     // [S][6] in the order of skx_qc_sample
};

__global__ __launch_bounds__(256) void qc_samples_kernel(QcSamplesArgs a)
{
    __shared__ uint32_t s_lut[2][256];                              // present | ambiguous << 5; the base in fields of five bits | present << 20
    __shared__ uint32_t s_cnt[QC_B * 6];
    const uint32_t sb = blockIdx.x % a.n_sblocks;
    const uint64_t tile = blockIdx.x / a.n_sblocks;
    const uint64_t c0 = (tile * 256 + threadIdx.x) * 16;
    const int lane = threadIdx.x & 63;
    const ColumnLane me(a.matrix, a.n_cols, c0);
    const uint32_t s0 = sb * QC_B, s1 = min(a.S, s0 + QC_B);       // s0 < S: the grid holds no empty block
    {
        const uint32_t c = cell_code(threadIdx.x);
        const bool present = cell_present(c), plain = cell_one_base(c);
        s_lut[0][threadIdx.x] = (present ? 1u : 0u) | (present && !plain ? 1u << 5 : 0u);
        s_lut[1][threadIdx.x] = (plain ? qc_spread(c) : 0u) | (present ? 1u << 20 : 0u);
        for (uint32_t j = threadIdx.x; j < QC_B * 6; j += 256) s_cnt[j] = 0;
    }
    // per column two masks: the bases private there | core << 20, and the bases that are minor there (none unless the row is core) | singleton << 20
    uint32_t m_private[16], m_minor[16];
    {
        const u32x4 *dp = reinterpret_cast<const u32x4 *>(a.desc + c0);
        const u32x4 lo = dp[0], hi = dp[1];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t w = i < 8 ? lo[i >> 1] : hi[(i - 8) >> 1], d = (w >> (16 * (i & 1))) & 0xFFFFu;
            const uint32_t core = d & D_CORE ? 1u : 0u;
            m_private[i] = qc_spread((d >> D_PRIVATE_SHIFT) & 0xFu) | (core << 20);
            m_minor[i] = (core ? qc_spread(~(d >> D_MAJOR_SHIFT) & 0xFu) : 0u) | (d & D_SINGLE ? 1u << 20 : 0u);
        }
    }
    __syncthreads();
    auto load = [&](uint32_t t) -> u32x4 { return *reinterpret_cast<const u32x4 *>(me.col + (uint64_t)min(t, s1 - 1) * a.pitch); };
    const uint32_t shift = 10u * ((uint32_t)lane % 3u);
    auto step = [&](uint32_t t, const u32x4 raw) {
        const u32x4 cur = raw & me.vm;
        uint32_t all = 0, pv = 0, mn = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t b = (cur[i >> 2] >> (8 * (i & 3))) & 0xFFu;
            const uint32_t wa = s_lut[0][b], wb = s_lut[1][b];
            all += wa; pv += wb & m_private[i]; mn += wb & m_minor[i];
        }
        // a cell adds to one base's field at most, so the four fields sum to 16 at most and no partial sum of the product carries
        const uint32_t n_private = (((pv & 0xFFFFFu) * 0x8421u) >> 15) & 0x1Fu, n_minor = (((mn & 0xFFFFFu) * 0x8421u) >> 15) & 0x1Fu;
        const uint32_t w1 = half_wave_sum((all & 0x1Fu) | ((all >> 5) << 10) | ((mn >> 20) << 20));      // kmers, ambiguous, singletons
        const uint32_t w2 = half_wave_sum((pv >> 20) | (n_private << 10) | (n_minor << 20));             // core_present, private_alleles, minor_alleles
        const uint32_t x1 = (uint32_t)__builtin_amdgcn_readlane((int)w1, 31), y1 = (uint32_t)__builtin_amdgcn_readlane((int)w1, 63);
        const uint32_t x2 = (uint32_t)__builtin_amdgcn_readlane((int)w2, 31), y2 = (uint32_t)__builtin_amdgcn_readlane((int)w2, 63);
        const uint32_t v = (((lane < 3 ? x1 : x2) >> shift) & 0x3FFu) + (((lane < 3 ? y1 : y2) >> shift) & 0x3FFu);
        if (lane < 6 && v) atomicAdd(&s_cnt[(t - s0) * 6 + lane], v);
    };
    // walk_columns' walk (skx_cells.h) spelled out: the shared form did not keep this kernel's time (NOTEBOOK 2026-10-21, one column walk)
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
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < (s1 - s0) * 6; j += 256)
        if (s_cnt[j]) atomicAdd(a.counts + (uint64_t)s0 * 6 + j, (unsigned long long)s_cnt[j]);
}

}  // namespace
}  // namespace skx

using namespace skx;

extern "C" int skx_array_sample_qc(skx_array *a, double min_freq, skx_qc_sample *samples, skx_qc_info *info)
{
    return skx_guarded([&]() -> int {
    if (!a || !samples) { set_error("qc: bad arguments"); return SKX_EINVAL; }
    if (!(min_freq >= 0.0 && min_freq <= 1.0)) { set_error("qc: min_freq must be between 0 and 1 (inclusive)"); return SKX_EINVAL; }
    const uint64_t S = a->names.size();
    if (S > 65535) { set_error("qc: %llu samples; at most 65535 are taken (16-bit counts)", (unsigned long long)S); return SKX_EUNSUP; }
    if (a->total_samples && a->total_samples != S) { set_error("qc: needs every sample of the array on one device"); return SKX_EUNSUP; }
    const uint64_t thr = std::max<uint64_t>(1, (uint64_t)std::ceil((double)S * min_freq));
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    SKX_TRY(array_materialize(a));
    const uint64_t U = a->n_rows;
    if (U >= (1ull << 32)) { set_error("qc: %llu rows; at most 2^32 - 1 are taken", (unsigned long long)U); return SKX_EUNSUP; }
    static_assert(sizeof(skx_qc_sample) == 6 * sizeof(uint64_t), "the device counters are a sample's record");
    if (S) memset(samples, 0, (size_t)S * sizeof(skx_qc_sample));
    skx_qc_info out{};
    out.rows = U; out.threshold = thr;
    if (info) *info = out;
    if (!U || !S) return SKX_OK;

    const uint64_t n_tiles = (U + SKX_QC_TILE_ROWS - 1) / SKX_QC_TILE_ROWS, n_sblocks = (S + QC_B - 1) / QC_B;      // <= 2^20 and <= 1 024
    DevBuf<uint16_t> d_desc; DevBuf<unsigned long long> d_counts, d_totals; DevBuf<int> d_bad;
    SKX_TRY(d_desc.alloc((size_t)n_tiles * SKX_QC_TILE_ROWS)); SKX_TRY(d_counts.alloc((size_t)S * 6)); SKX_TRY(d_totals.alloc(3)); SKX_TRY(d_bad.alloc(1));
    SKX_TRY(d_counts.zero(st)); SKX_TRY(d_totals.zero(st)); SKX_TRY(d_bad.zero(st));
    QcRowsArgs ra{};
    ra.matrix = a->matrix.p; ra.pitch = a->pitch; ra.n_cols = U; ra.S = (uint32_t)S; ra.thr = (uint32_t)thr;
    ra.desc = d_desc.p; ra.totals = d_totals.p; ra.bad_byte = d_bad.p;
    hipLaunchKernelGGL(qc_rows_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, ra);
    SKX_HIP(hipGetLastError());
    QcSamplesArgs sa{};
    sa.matrix = a->matrix.p; sa.pitch = a->pitch; sa.n_cols = U; sa.desc = d_desc.p; sa.S = (uint32_t)S; sa.n_sblocks = (uint32_t)n_sblocks; sa.counts = d_counts.p;
    hipLaunchKernelGGL(qc_samples_kernel, dim3((unsigned)(n_tiles * n_sblocks)), dim3(256), 0, st, sa);
    SKX_HIP(hipGetLastError());
    int bad = 0; unsigned long long totals[3] = {0, 0, 0};
    std::vector<skx_qc_sample> got(S);
    SKX_HIP(hipMemcpyAsync(got.data(), d_counts.p, (size_t)S * sizeof(skx_qc_sample), hipMemcpyDeviceToHost, st));
    SKX_HIP(hipMemcpyAsync(totals, d_totals.p, sizeof totals, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipMemcpyAsync(&bad, d_bad.p, 4, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    if (bad) { set_error("qc: variants contain a byte outside -ACGTMRWSYKVHDBN"); return SKX_EINVAL; }
    memcpy(samples, got.data(), (size_t)S * sizeof(skx_qc_sample));
    out.rows_present = totals[0]; out.core_rows = totals[1]; out.core_variant_rows = totals[2];
    if (info) *info = out;
    return SKX_OK;
    });
}
