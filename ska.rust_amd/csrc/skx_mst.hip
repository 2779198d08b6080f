// skx_mst.hip -- the minimum spanning forest of `ska distance --mst` (skx_array_distance_mst of include/skx.h), kept on the device from the first
// band of the pair matrix to the last: after band b it is the forest F of every candidate line with a first sample below the band's end, and
// the next band makes F = MSF(F + its own candidates).  By the cycle property a line dropped once is in no later forest, so the last F is the
// forest of the whole table (tests/mst_model.py: mst_streamed).  O(S) state; a band's count buffer [band][S][DIST_NCOUNT] is read as
// launch_pair_counts leaves it, once, by the gather and at the band's end by the finish.
//
// The order is (key, i, j), key the exact numerator sel_pair gives, as one 64-bit word key << 32 | i << 16 | j (the host refuses more than 65 536
// samples and a row count that lets a key reach 2^32), so one 64-bit atomicMin orders by it.  All ones is no edge.  The order is strict: no two
// lines share a word.
//
// Per band (driver: array_distance_mst in skx_distance.cpp), every step its own launch, nothing loops on a device-wide condition:
//   mst_begin_kernel    comp[x] = parent[x] = x, best[x] = none
//   mst_gather_kernel   a workgroup per row i of the band, lanes over j > i (the walk of select_count_kernel): words[(i - i_lo) * S + j] = the
//                       pair's word if it passes the thresholds (sel_pair), else none -- 8 bytes a pair for the rounds instead of the counters' 128
//   rounds, until one chooses nothing (the host reads the forest's length back after each; at most ceil(log2 S) + 1 choose something):
//     mst_min_kernel    every edge -- the records of the forest so far, one a thread, and the band's words, the gather's walk -- whose ends lie in
//                       different components does atomicMin(best[comp], word) for both.  An atomic is skipped when the word is not below what
//                       best[] shows already (it only ever falls), and a wave's part of a row, which shares comp[i], reduces to one atomic
//     mst_claim_kernel  the same walk; an edge whose word EQUALS best[] of either end is chosen: appended to the new forest -- a record as it
//                       is, a band edge as (i, j, key) -- and its two trees joined in parent[] (uf_link of skx_unionfind.h).  Every edge has
//                       one thread, so it is appended once even where both ends chose it
//     mst_relabel_kernel comp[x] = root(x), best[x] = none
//   mst_finish_kernel   the new forest's band edges (i >= i_lo: every older record has a smaller i) take mism and m from the counters, before
//                       the next band zeroes them; the host then swaps the two forest buffers
// comp[] is what the round started with and is only read by min and claim; the links go to parent[], so a claim never sees a label move.
//
// Why the chosen edges of a round close no cycle: suppose they did, over the components C1 .. Cn, and let e be the cycle's largest edge under
// the strict order.  e was chosen by one of its two ends, say C1; but the cycle's other edge at C1 also leaves C1 and is smaller than e, so e
// was not C1's smallest outgoing edge.  Hence a band appends at most S - 1 records (the append is bounds-checked all the same), every chosen
// edge is the smallest across the cut around its component and so belongs to the unique forest, and which thread wins an atomic changes
// nothing: the forest's lines are the same from run to run; the host sorts them by (i, j).  No float atomics; the mismatch threshold is
// finish_pair's add and divide in float64, each rounded once: this file is compiled with -ffp-contract=off (Makefile).
#include "skx_internal.h"
#include "skx_unionfind.h"

namespace skx {
namespace {

constexpr int MST_NT = 256;                       // threads of every workgroup here
constexpr unsigned long long MST_NONE = ~0ull;    // no edge

__device__ inline unsigned long long edge_word(unsigned long long key, uint32_t i, uint32_t j) { return (key << 32) | ((unsigned long long)i << 16) | (unsigned long long)j; }
__device__ inline unsigned long long best_now(const unsigned long long *best, uint32_t c) { return __hip_atomic_load(best + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(MST_NT) void mst_begin_kernel(uint32_t *comp, uint32_t *parent, unsigned long long *best, int S)
{
    const int x = (int)(blockIdx.x * MST_NT + threadIdx.x);
    if (x < S) { comp[x] = (uint32_t)x; parent[x] = (uint32_t)x; best[x] = MST_NONE; }
}

__global__ __launch_bounds__(MST_NT) void mst_gather_kernel(const unsigned long long *cnt, int S, int i_lo, int i_hi, int filt_ambig, double constant,
                                                            unsigned long long kmax, double pmax, unsigned long long *words, unsigned long long *n_candidates)
{
    const int i = i_lo + (int)blockIdx.x;
    if (i >= i_hi) return;
    const unsigned long long *row = cnt + (uint64_t)(i - i_lo) * S * DIST_NCOUNT;
    unsigned long long *out = words + (uint64_t)(i - i_lo) * S;
    unsigned long long n = 0;
    for (int j = i + 1 + (int)threadIdx.x; j < S; j += MST_NT) {
        SelPair p;
        const bool take = sel_pair(row + (uint64_t)j * DIST_NCOUNT, filt_ambig, constant, kmax, pmax, p);
        out[j] = take ? edge_word(p.key, (uint32_t)i, (uint32_t)j) : MST_NONE;
        n += take ? 1u : 0u;
    }
    for (int off = 32; off; off >>= 1) n += __shfl_xor(n, off, 64);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(n_candidates, n);
}

// the blocks [0, rows) walk the band's rows, the blocks behind them the forest's records
__global__ __launch_bounds__(MST_NT) void mst_min_kernel(const unsigned long long *words, int S, int i_lo, int rows, const SelRecord *forest, uint32_t n_forest,
                                                         const uint32_t *comp, unsigned long long *best)
{
    if ((int)blockIdx.x >= rows) {
        const uint32_t e = (blockIdx.x - (uint32_t)rows) * MST_NT + threadIdx.x;
        if (e >= n_forest) return;
        const SelRecord r = forest[e];
        const uint32_t a = comp[r.i], b = comp[r.j];
        if (a == b) return;
        const unsigned long long w = edge_word(r.key, r.i, r.j);
        if (w < best_now(best, a)) atomicMin(best + a, w);
        if (w < best_now(best, b)) atomicMin(best + b, w);
        return;
    }
    const int i = i_lo + (int)blockIdx.x;
    const unsigned long long *in = words + (uint64_t)blockIdx.x * S;
    const uint32_t a = comp[i];
    unsigned long long low = MST_NONE;                  // the smallest word of this lane's edges that leave a
    for (int j = i + 1 + (int)threadIdx.x; j < S; j += MST_NT) {
        const unsigned long long w = in[j];
        if (w == MST_NONE) continue;
        const uint32_t b = comp[j];
        if (a == b) continue;
        low = w < low ? w : low;
        if (w < best_now(best, b)) atomicMin(best + b, w);
    }
    for (int off = 32; off; off >>= 1) { const unsigned long long o = __shfl_xor(low, off, 64); low = o < low ? o : low; }
    if ((threadIdx.x & 63) == 0 && low < best_now(best, a)) atomicMin(best + a, low);
}

// appends a chosen edge (cap: the records `out` holds) and joins its trees
__device__ inline void mst_choose(const SelRecord &r, SelRecord *out, uint32_t cap, uint32_t *n_out, uint32_t *parent)
{
    const uint32_t at = atomicAdd(n_out, 1u);
    if (at < cap) out[at] = r;
    uf_link(parent, r.i, r.j);
}
__global__ __launch_bounds__(MST_NT) void mst_claim_kernel(const unsigned long long *words, int S, int i_lo, int rows, const SelRecord *forest, uint32_t n_forest,
                                                           const uint32_t *comp, const unsigned long long *best, uint32_t *parent, SelRecord *out, uint32_t cap,
                                                           uint32_t *n_out)
{
    if ((int)blockIdx.x >= rows) {
        const uint32_t e = (blockIdx.x - (uint32_t)rows) * MST_NT + threadIdx.x;
        if (e >= n_forest) return;
        const SelRecord r = forest[e];
        const uint32_t a = comp[r.i], b = comp[r.j];
        if (a == b) return;
        const unsigned long long w = edge_word(r.key, r.i, r.j);
        if (w == best[a] || w == best[b]) mst_choose(r, out, cap, n_out, parent);
        return;
    }
    const int i = i_lo + (int)blockIdx.x;
    const unsigned long long *in = words + (uint64_t)blockIdx.x * S;
    const uint32_t a = comp[i];
    const unsigned long long best_a = best[a];
    for (int j = i + 1 + (int)threadIdx.x; j < S; j += MST_NT) {
        const unsigned long long w = in[j];
        if (w == MST_NONE) continue;
        const uint32_t b = comp[j];
        if (a == b) continue;
        if (w == best_a || w == best[b]) mst_choose(SelRecord{(uint32_t)i, (uint32_t)j, 0, 0, w >> 32}, out, cap, n_out, parent);      // (mism, m: mst_finish_kernel)
    }
}

__global__ __launch_bounds__(MST_NT) void mst_relabel_kernel(uint32_t *comp, const uint32_t *parent, unsigned long long *best, int S)
{
    const int x = (int)(blockIdx.x * MST_NT + threadIdx.x);
    if (x < S) { comp[x] = uf_root(parent, (uint32_t)x); best[x] = MST_NONE; }
}

__global__ __launch_bounds__(MST_NT) void mst_finish_kernel(const unsigned long long *cnt, int S, int i_lo, int i_hi, int filt_ambig, SelRecord *forest, uint32_t n_forest)
{
    const uint32_t e = blockIdx.x * MST_NT + threadIdx.x;
    if (e >= n_forest) return;
    const uint32_t i = forest[e].i, j = forest[e].j;
    if (i < (uint32_t)i_lo || i >= (uint32_t)i_hi || j >= (uint32_t)S) return;
    SelPair p;
    (void)sel_pair(cnt + ((uint64_t)(i - (uint32_t)i_lo) * S + j) * DIST_NCOUNT, filt_ambig, 0.0, ~0ull, -1.0, p);
    forest[e].mism = p.mism; forest[e].m = p.m; forest[e].key = p.key;
}

inline unsigned blocks_of(uint64_t n) { return (unsigned)((n + MST_NT - 1) / MST_NT); }

}  // namespace

void launch_mst_begin(uint32_t *comp, uint32_t *parent, unsigned long long *best, int S, hipStream_t st)
{
    if (S < 1) return;
    hipLaunchKernelGGL(mst_begin_kernel, dim3(blocks_of((uint64_t)S)), dim3(MST_NT), 0, st, comp, parent, best, S);
}
void launch_mst_gather(const unsigned long long *cnt, int S, int i_lo, int i_hi, const SelCriteria &c, unsigned long long *words, unsigned long long *n_candidates,
                       hipStream_t st)
{
    if (i_hi <= i_lo) return;
    hipLaunchKernelGGL(mst_gather_kernel, dim3((unsigned)(i_hi - i_lo)), dim3(MST_NT), 0, st, cnt, S, i_lo, i_hi, c.filt_ambig, c.constant, c.kmax, c.pmax, words, n_candidates);
}
void launch_mst_round(const unsigned long long *words, int S, int i_lo, int i_hi, const SelRecord *forest, uint32_t n_forest, const uint32_t *comp, unsigned long long *best,
                      uint32_t *parent, SelRecord *out, uint32_t cap, uint32_t *n_out, hipStream_t st)
{
    if (i_hi <= i_lo) return;
    const int rows = i_hi - i_lo;
    const dim3 grid((unsigned)rows + blocks_of(n_forest)), block(MST_NT);
    hipLaunchKernelGGL(mst_min_kernel, grid, block, 0, st, words, S, i_lo, rows, forest, n_forest, comp, best);
    hipLaunchKernelGGL(mst_claim_kernel, grid, block, 0, st, words, S, i_lo, rows, forest, n_forest, comp, (const unsigned long long *)best, parent, out, cap, n_out);
}
void launch_mst_relabel(uint32_t *comp, const uint32_t *parent, unsigned long long *best, int S, hipStream_t st)
{
    if (S < 1) return;
    hipLaunchKernelGGL(mst_relabel_kernel, dim3(blocks_of((uint64_t)S)), dim3(MST_NT), 0, st, comp, parent, best, S);
}
void launch_mst_finish(const unsigned long long *cnt, int S, int i_lo, int i_hi, int filt_ambig, SelRecord *forest, uint32_t n_forest, hipStream_t st)
{
    if (i_hi <= i_lo || !n_forest) return;
    hipLaunchKernelGGL(mst_finish_kernel, dim3(blocks_of(n_forest)), dim3(MST_NT), 0, st, cnt, S, i_lo, i_hi, filt_ambig, forest, n_forest);
}

}  // namespace skx
