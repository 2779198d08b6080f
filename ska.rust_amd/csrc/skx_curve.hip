// skx_curve.hip -- `ska curve`: how many rows are there (pan), pass --min-freq (core), hold two bases (variant) or both (core_variant) after each
// sample of an order has been added, for many orders from one load (skx_array_curve, include/skx.h; definition there and in tests/curve_model.py).
// The reference has no counterpart: `ska nk` prints one number for the whole file, and its users chain `ska delete` (merge_ska_array.rs:231-271)
// and `ska align` once per prefix and per shuffle and count columns.
//
// The matrix is sample-major, so a row of the reference is a column here.  A thread owns 16 consecutive columns (one 16-byte load per sample, inside
// the row's padding), a workgroup a tile of 4 096, and walks the samples of one order through order[p * S + t] with four loads in flight
// (ColumnLane and the walk of walk_columns, skx_cells.h, spelled out here across the LDS blocks), a decision after every sample.  Per column one register: cells present in the low 16 bits, the OR
// of the unambiguous cells' codes above them.  After sample t the four flags of a lane's 16 columns are summed (two packed words: pan | core << 16,
// variant | core_variant << 16; a tile holds 4 096 columns, so neither half overflows) over the wave -- each flag is a comparison whose lane mask is
// counted in scalar registers, no shuffles -- and added by one lane to the step's two words in LDS.  The LDS block covers SKX_CURVE_LDS_STEPS steps; at its end (and at S) the workgroup adds it to the order's [S][4] 64-bit
// counters in device memory and clears it.  Integer atomics only: the result does not depend on who arrives first.  No workgroup waits for
// another, every loop is bounded by S or the block, and every barrier is reached by all 256 threads: the ones past the last column walk
// column 0 behind a mask of zeros and count nothing.
//
// Device memory beside the array: 36 bytes per (order, step) of a batch -- its orders (4) and counters (32) -- for at most
// SKX_CURVE_BATCH_ORDERS orders and 2^22 (order, step) pairs a launch, and 4 S bytes of thresholds.
#include "skx_internal.h"
#include "skx_cells.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace skx {
namespace {

constexpr uint32_t CURVE_STEPS = SKX_CURVE_LDS_STEPS;
constexpr uint32_t CURVE_THREADS = SKX_CURVE_TILE_ROWS / 16;
static_assert(CURVE_THREADS == 256, "a workgroup of 256 threads, 16 columns each");
static_assert(CURVE_STEPS % 4 == 0, "the walk is unrolled by the four loads in flight");
static_assert(SKX_CURVE_TILE_ROWS <= 0xFFFF, "the packed halves of a step's LDS words hold a tile's columns");

struct CurveArgs {
    const uint8_t *matrix; uint64_t pitch, n_cols;
    const int *orders;                                              // [n_orders][S] of this launch
    const uint32_t *thr;                                            // [S]: thr[t] = the threshold of the prefix of t + 1 samples (>= 1)
    uint32_t S, n_orders, n_tiles; int orders_fastest;              // which of the two runs fastest along the grid
    unsigned long long *counts;                                     // [n_orders][S][4] pan, core, variant, core_variant
    int *bad_byte;
};

__global__ __launch_bounds__(256) void curve_kernel(CurveArgs a)
{
    __shared__ uint32_t s_lut[256];                                 // bit 0: present; bits 16-19: the set code of a single base (A 1, C 2, T 4, G 8); bit 8: outside the alphabet
    __shared__ uint32_t s_cnt[CURVE_STEPS][2];                      // per step of the block: pan | core << 16, variant | core_variant << 16
    __shared__ int s_ord[CURVE_STEPS + 4];                          // the block's samples and the four behind it (the loads in flight)
    __shared__ uint32_t s_thr[CURVE_STEPS];
    const uint32_t p = a.orders_fastest ? blockIdx.x % a.n_orders : blockIdx.x / a.n_tiles;
    const uint64_t tile = a.orders_fastest ? blockIdx.x / a.n_orders : blockIdx.x % a.n_tiles;
    const uint64_t c0 = (tile * 256 + threadIdx.x) * 16;
    const int lane = threadIdx.x & 63;
    const ColumnLane me(a.matrix, a.n_cols, c0);
    const uint32_t S = a.S;
    const int *order = a.orders + (uint64_t)p * S;
    unsigned long long *out = a.counts + (uint64_t)p * S * 4;
    // order[] and thr[] of a block of steps are staged in LDS: every lane reads the same word (a broadcast), and no wait for them stands between
    // the matrix loads in flight
    auto stage = [&](uint32_t t0) {
        for (uint32_t j = threadIdx.x; j < CURVE_STEPS + 4; j += 256) {
            if (t0 + j < S) s_ord[j] = order[t0 + j];
            if (j < CURVE_STEPS) { s_cnt[j][0] = 0; s_cnt[j][1] = 0; if (t0 + j < S) s_thr[j] = a.thr[t0 + j]; }
        }
    };
    uint32_t t0 = 0;                                                // the first step of the LDS block
    // (the loads run four samples ahead, past a block's end into the next block's first samples, which are staged with the block; past S the last sample again)
    auto load = [&](uint32_t t) -> u32x4 { return *reinterpret_cast<const u32x4 *>(me.col + (uint64_t)s_ord[min(t, S - 1) - t0] * a.pitch); };
    {
        const uint32_t c = cell_code(threadIdx.x);
        s_lut[threadIdx.x] = c == CELL_OUTSIDE ? 0x100u : c == 0 ? 0u : 1u | (cell_one_base(c) ? c << 16 : 0u);
    }
    stage(0);
    __syncthreads();
    uint32_t acc[16];
    uint32_t bad = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0;

    auto step = [&](uint32_t t, const u32x4 raw) {
        const u32x4 cur = raw & me.vm;
        const uint32_t thr = s_thr[t - t0];
        // the wave's sums are formed in scalar registers: a comparison leaves its lanes as a 64-bit mask, whose bits are counted there
        uint32_t pc = 0, vc = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t v = s_lut[(cur[i >> 2] >> (8 * (i & 3))) & 0xFFu];
            bad |= v;
            acc[i] = (acc[i] + (v & 1u)) | (v & 0xF0000u);
            const uint32_t n = acc[i] & 0xFFFFu, B = acc[i] >> 16;
            const unsigned long long pan = __ballot(n != 0), core = __ballot(n >= thr), var = __ballot((B & (B - 1u)) != 0);      // thr >= 1: a core row is a pan row
            pc += (uint32_t)__popcll(pan) + ((uint32_t)__popcll(core) << 16);
            vc += (uint32_t)__popcll(var) + ((uint32_t)__popcll(var & core) << 16);
        }
        if (lane == 0) {
            if (pc) atomicAdd(&s_cnt[t - t0][0], pc);
            if (vc) atomicAdd(&s_cnt[t - t0][1], vc);
        }
    };
    // walk_columns' walk (skx_cells.h) spelled out, its four buffers kept across the LDS blocks: with a walk of its own per block the kernel
    // runs out of scalar registers and a step grows by 6 % (NOTEBOOK 2026-10-21, one column walk)
    u32x4 b0 = load(0);
    __builtin_amdgcn_sched_barrier(0);
    u32x4 b1 = load(1);
    __builtin_amdgcn_sched_barrier(0);
    u32x4 b2 = load(2);
    __builtin_amdgcn_sched_barrier(0);
    u32x4 b3 = load(3);
    for (; t0 < S; t0 += CURVE_STEPS) {                             // (every bound below is the same for the whole workgroup)
        const uint32_t t1 = min(S, t0 + CURVE_STEPS);
        if (t0) { stage(t0); __syncthreads(); }
        for (uint32_t t = t0; t < t1; t += 4) {                     // (b0 holds sample t: CURVE_STEPS is a multiple of 4)
            step(t, b0); b0 = load(t + 4);
            if (t + 1 < t1) step(t + 1, b1);                        // (false only at the end of the last block)
            b1 = load(t + 5);
            if (t + 2 < t1) step(t + 2, b2);
            b2 = load(t + 6);
            if (t + 3 < t1) step(t + 3, b3);
            b3 = load(t + 7);
        }
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < t1 - t0; j += 256) {     // (the thread that reads a step's words here is the one that clears them in stage)
            const uint32_t w0 = s_cnt[j][0], w1 = s_cnt[j][1];
            unsigned long long *o = out + (uint64_t)(t0 + j) * 4;
            if (w0 & 0xFFFFu) atomicAdd(o + 0, (unsigned long long)(w0 & 0xFFFFu));
            if (w0 >> 16) atomicAdd(o + 1, (unsigned long long)(w0 >> 16));
            if (w1 & 0xFFFFu) atomicAdd(o + 2, (unsigned long long)(w1 & 0xFFFFu));
            if (w1 >> 16) atomicAdd(o + 3, (unsigned long long)(w1 >> 16));
        }
    }
    if (bad & 0x100u) *a.bad_byte = 1;
}

}  // namespace
}  // namespace skx

using namespace skx;

extern "C" int skx_array_curve(skx_array *a, const int32_t *orders, uint32_t n_orders, double min_freq, uint64_t *counts)
{
    return skx_guarded([&]() -> int {
    if (!a || !orders || !counts) { set_error("curve: bad arguments"); return SKX_EINVAL; }
    if (n_orders == 0) { set_error("curve: no orders given"); return SKX_EINVAL; }
    if (!(min_freq >= 0.0 && min_freq <= 1.0)) { set_error("curve: min_freq must be between 0 and 1 (inclusive)"); return SKX_EINVAL; }
    const uint64_t S = a->names.size();
    if (S > 65535) { set_error("curve: %llu samples; at most 65535 are taken (16-bit counts)", (unsigned long long)S); return SKX_EUNSUP; }
    if (a->total_samples && a->total_samples != S) { set_error("curve: needs every sample of the array on one device"); return SKX_EUNSUP; }
    if (S == 0) { set_error("curve: the array has no samples"); return SKX_EINVAL; }
    {
        std::vector<uint32_t> seen(S, 0);                                                   // seen[s] = the last order + 1 that named s
        for (uint32_t p = 0; p < n_orders; p++)
            for (uint64_t t = 0; t < S; t++) {
                const int32_t s = orders[(uint64_t)p * S + t];
                if (s < 0 || (uint64_t)s >= S) { set_error("curve: order %u: index %d at position %llu is outside the array's %llu samples", p, s, (unsigned long long)t, (unsigned long long)S); return SKX_EINVAL; }
                if (seen[s] == p + 1) { set_error("curve: order %u names sample %d twice: not a permutation", p, s); return SKX_EINVAL; }
                seen[s] = p + 1;
            }
    }
    std::vector<uint32_t> thr(S);
    for (uint64_t t = 1; t <= S; t++) thr[t - 1] = (uint32_t)std::max<uint64_t>(1, (uint64_t)std::ceil((double)t * min_freq));
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    SKX_TRY(array_materialize(a));
    const uint64_t U = a->n_rows;
    if (U >= (1ull << 32)) { set_error("curve: %llu rows; at most 2^32 - 1 are taken", (unsigned long long)U); return SKX_EUNSUP; }
    memset(counts, 0, (size_t)n_orders * S * 4 * sizeof(uint64_t));
    if (!U) return SKX_OK;

    const uint64_t n_tiles = (U + SKX_CURVE_TILE_ROWS - 1) / SKX_CURVE_TILE_ROWS;
    const uint32_t batch = (uint32_t)std::min<uint64_t>(n_orders, std::min<uint64_t>(SKX_CURVE_BATCH_ORDERS, std::max<uint64_t>(1, (1ull << 22) / S)));
    // which of tiles and orders runs fastest along the grid: SKX_KNOBS=curve_tiles_fastest is there to measure one against the other
    // (tools/curve_bench.py); the results are the same
    const int orders_fastest = knob("curve_tiles_fastest") ? 0 : 1;
    DevBuf<int> d_orders, d_bad; DevBuf<uint32_t> d_thr; DevBuf<unsigned long long> d_counts;
    SKX_TRY(d_orders.alloc((size_t)batch * S)); SKX_TRY(d_counts.alloc((size_t)batch * S * 4)); SKX_TRY(d_thr.alloc(S));
    SKX_TRY(d_bad.alloc(1)); SKX_TRY(d_bad.zero(st));
    SKX_HIP(hipMemcpyAsync(d_thr.p, thr.data(), S * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    int bad = 0;
    for (uint32_t p0 = 0; p0 < n_orders; p0 += batch) {
        const uint32_t np = std::min<uint32_t>(batch, n_orders - p0);
        SKX_HIP(hipMemcpyAsync(d_orders.p, orders + (uint64_t)p0 * S, (size_t)np * S * sizeof(int), hipMemcpyHostToDevice, st));
        SKX_HIP(hipMemsetAsync(d_counts.p, 0, (size_t)np * S * 4 * sizeof(unsigned long long), st));
        CurveArgs ka{};
        ka.matrix = a->matrix.p; ka.pitch = a->pitch; ka.n_cols = U;
        ka.orders = d_orders.p; ka.thr = d_thr.p; ka.S = (uint32_t)S; ka.n_orders = np; ka.n_tiles = (uint32_t)n_tiles; ka.orders_fastest = orders_fastest;
        ka.counts = d_counts.p; ka.bad_byte = d_bad.p;
        hipLaunchKernelGGL(curve_kernel, dim3((unsigned)(n_tiles * np)), dim3(256), 0, st, ka);      // n_tiles <= 2^20, np <= 2^10
        SKX_HIP(hipGetLastError());
        SKX_HIP(hipMemcpyAsync(counts + (uint64_t)p0 * S * 4, d_counts.p, (size_t)np * S * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        SKX_HIP(hipMemcpyAsync(&bad, d_bad.p, 4, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipStreamSynchronize(st));
        if (bad) { set_error("curve: variants contain a byte outside -ACGTMRWSYKVHDBN"); return SKX_EINVAL; }
    }
    return SKX_OK;
    });
}
