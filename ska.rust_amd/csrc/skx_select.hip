// skx_select.hip -- line selection for `ska distance --max-snps / --max-mismatches / --closest` (skx_array_distance_select of include/skx.h):
// the pairs of one band of the pair matrix that pass the thresholds, or every sample's K nearest candidates, picked on the device from the
// band's count buffer [band][S][DIST_NCOUNT] as launch_pair_counts leaves it.  Only the picked pairs reach the host.
//
// A pair's integers restate the first half of finish_pair (skx_distance.cpp): mismatches, m (what is added to the constant for the matches) and
// key, the exact numerator of the distance (distance = key with filt_ambig, key / 36 without).  `key <= kmax` is the SNP threshold in
// integers (the host derives kmax from finish_pair's own expression); the mismatch threshold is finish_pair's expression in float64 --
// this file is compiled with -ffp-contract=off (Makefile) so that the add and the divide stay two correctly rounded operations.
//
// Threshold form, two launches a band, a workgroup per row i of the band:
//   select_count_kernel   candidates (j > i) of the row -> n_row[i - i_lo]                      (the host turns them into offsets)
//   select_write_kernel   the same walk, the candidates written at the row's offset in ascending j (ballot ranks inside a wave, the waves'
//                         totals through LDS): the records come out sorted by (i, j), nothing is sorted afterwards
// --closest form, two launches a band, a workgroup per owner; every list has one writer at a time, no atomics on the lists:
//   nearest_kernel<false> owner = row i of the band, candidates j > i along its buffer row
//   nearest_kernel<true>  owner = sample j > i_lo, candidates i < j down the band's column j (one 128-byte line each)
// The owner's list (K entries sorted by (key, partner), unused places all ones) sits in the lower half of an LDS array, a chunk of candidates
// in the upper half, one bitonic sort of the whole puts the smallest back in front.  (key, partner) is one 64-bit word: key < 2^32 is
// checked by the host from the row count.
#include "skx_internal.h"

namespace skx {
namespace {

constexpr int SEL_NT = 256;                       // threads of every workgroup here
constexpr unsigned long long SEL_NONE = ~0ull;    // an unused place of a list

// (a pair's integers and the threshold test: sel_pair of skx_internal.h, shared with skx_banded.hip)

__global__ __launch_bounds__(SEL_NT) void select_count_kernel(const unsigned long long *cnt, int S, int i_lo, int i_hi, int filt_ambig, double constant,
                                                              unsigned long long kmax, double pmax, uint32_t *n_row)
{
    const int i = i_lo + (int)blockIdx.x;
    if (i >= i_hi) return;
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const unsigned long long *row = cnt + (uint64_t)(i - i_lo) * S * DIST_NCOUNT;
    uint32_t n = 0;
    for (int j = i + 1 + (int)threadIdx.x; j < S; j += SEL_NT) { SelPair p; n += sel_pair(row + (uint64_t)j * DIST_NCOUNT, filt_ambig, constant, kmax, pmax, p) ? 1u : 0u; }
    for (int off = 32; off; off >>= 1) n += __shfl_xor(n, off, 64);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&s_n, n);
    __syncthreads();
    if (threadIdx.x == 0) n_row[i - i_lo] = s_n;
}

// row_off[r]: where row r's records start in out; row_off[r + 1] - row_off[r] = what select_count_kernel counted (the same predicate on the same counts)
__global__ __launch_bounds__(SEL_NT) void select_write_kernel(const unsigned long long *cnt, int S, int i_lo, int i_hi, int filt_ambig, double constant,
                                                              unsigned long long kmax, double pmax, const uint64_t *row_off, SelRecord *out)
{
    const int i = i_lo + (int)blockIdx.x;
    if (i >= i_hi) return;
    __shared__ uint32_t s_wave[SEL_NT / 64];
    const unsigned long long *row = cnt + (uint64_t)(i - i_lo) * S * DIST_NCOUNT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t end = row_off[blockIdx.x + 1];
    uint64_t at = row_off[blockIdx.x];
    for (int j0 = i + 1; j0 < S; j0 += SEL_NT) {                    // (uniform over the workgroup: the barriers are reached by all)
        const int j = j0 + (int)threadIdx.x;
        SelPair p{0, 0, 0};
        const bool take = j < S && sel_pair(row + (uint64_t)j * DIST_NCOUNT, filt_ambig, constant, kmax, pmax, p);
        const unsigned long long b = __ballot(take);
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < SEL_NT / 64; w++) { before += w < wave ? s_wave[w] : 0u; total += s_wave[w]; }
        const uint64_t slot = at + before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        if (take && slot < end) out[slot] = SelRecord{(uint32_t)i, (uint32_t)j, p.mism, p.m, p.key};
        at += total;
        __syncthreads();
    }
}

// ascending bitonic sort of n (a power of two) words with two payload words each, all in LDS
__device__ inline void sel_sort(unsigned long long *k, unsigned long long *a, unsigned long long *b, uint32_t n)
{
    for (uint32_t size = 2; size <= n; size <<= 1)
        for (uint32_t d = size >> 1; d; d >>= 1) {
            for (uint32_t x = threadIdx.x; x < n; x += SEL_NT) {
                const uint32_t y = x ^ d;
                if (y > x) {
                    const bool up = (x & size) == 0;
                    const unsigned long long kx = k[x], ky = k[y];
                    if ((kx > ky) == up && kx != ky) {
                        k[x] = ky; k[y] = kx;
                        const unsigned long long ax = a[x], bx = b[x];
                        a[x] = a[y]; a[y] = ax; b[x] = b[y]; b[y] = bx;
                    }
                }
            }
            __syncthreads();
        }
}

// L: places of the list in LDS, a power of two >= max(K, SEL_NT); the sort runs over 2 L
template <bool COLUMN>
__global__ __launch_bounds__(SEL_NT) void nearest_kernel(const unsigned long long *cnt, int S, int i_lo, int i_hi, int filt_ambig, double constant,
                                                         unsigned long long kmax, double pmax, uint32_t K, uint32_t L, SelNear *lists,
                                                         unsigned long long *n_candidates)
{
    extern __shared__ unsigned long long s_mem[];
    unsigned long long *s_k = s_mem, *s_a = s_mem + 2 * (size_t)L, *s_b = s_mem + 4 * (size_t)L;
    const int owner = COLUMN ? i_lo + 1 + (int)blockIdx.x : i_lo + (int)blockIdx.x;
    if (owner >= (COLUMN ? S : i_hi)) return;
    // the owner's candidates are the partners t in [t0, t1)
    const int t0 = COLUMN ? i_lo : owner + 1, t1 = COLUMN ? (owner < i_hi ? owner : i_hi) : S;
    if (t0 >= t1) return;
    SelNear *mine = lists + (uint64_t)owner * K;
    for (uint32_t e = threadIdx.x; e < L; e += SEL_NT) {
        const bool held = e < K;
        s_k[e] = held ? mine[e].sort_key : SEL_NONE; s_a[e] = held ? mine[e].mism : 0; s_b[e] = held ? mine[e].m : 0;
    }
    unsigned long long seen = 0;
    bool changed = false;
    for (int base = t0; base < t1; base += (int)L) {
        int any = 0;
        for (uint32_t e = threadIdx.x; e < L; e += SEL_NT) {
            const int t = base + (int)e;
            unsigned long long key = SEL_NONE; SelPair p{0, 0, 0};
            if (t < t1) {
                const uint64_t pair = COLUMN ? (uint64_t)(t - i_lo) * S + owner : (uint64_t)(owner - i_lo) * S + t;
                if (sel_pair(cnt + pair * DIST_NCOUNT, filt_ambig, constant, kmax, pmax, p)) { key = (p.key << 32) | (unsigned long long)(uint32_t)t; any = 1; seen++; }
            }
            s_k[L + e] = key; s_a[L + e] = p.mism; s_b[L + e] = p.m;
        }
        if (__syncthreads_or(any)) { sel_sort(s_k, s_a, s_b, 2 * L); changed = true; }       // (the barrier also covers the stores above)
    }
    if (changed)
        for (uint32_t e = threadIdx.x; e < K; e += SEL_NT) mine[e] = SelNear{s_k[e], s_a[e], s_b[e], s_k[e] == SEL_NONE ? 0ull : s_k[e] >> 32};
    if (!COLUMN) {                                  // every pair is some row owner's candidate exactly once
        for (int off = 32; off; off >>= 1) seen += __shfl_xor(seen, off, 64);
        if ((threadIdx.x & 63) == 0 && seen) atomicAdd(n_candidates, seen);
    }
}

}  // namespace

void launch_select_count(const unsigned long long *cnt, int S, int i_lo, int i_hi, const SelCriteria &c, uint32_t *n_row, hipStream_t st)
{
    if (i_hi <= i_lo) return;
    hipLaunchKernelGGL(select_count_kernel, dim3((unsigned)(i_hi - i_lo)), dim3(SEL_NT), 0, st, cnt, S, i_lo, i_hi, c.filt_ambig, c.constant, c.kmax, c.pmax, n_row);
}
void launch_select_write(const unsigned long long *cnt, int S, int i_lo, int i_hi, const SelCriteria &c, const uint64_t *row_off, SelRecord *out, hipStream_t st)
{
    if (i_hi <= i_lo) return;
    hipLaunchKernelGGL(select_write_kernel, dim3((unsigned)(i_hi - i_lo)), dim3(SEL_NT), 0, st, cnt, S, i_lo, i_hi, c.filt_ambig, c.constant, c.kmax, c.pmax, row_off, out);
}
uint32_t select_list_places(uint32_t K)
{
    uint32_t L = SEL_NT;
    while (L < K) L <<= 1;
    return L;
}
void launch_select_nearest(const unsigned long long *cnt, int S, int i_lo, int i_hi, const SelCriteria &c, uint32_t K, SelNear *lists, unsigned long long *n_candidates,
                           hipStream_t st)
{
    if (i_hi <= i_lo || K < 1 || K > SEL_MAX_K) return;
    const uint32_t L = select_list_places(K);
    const size_t lds = 6 * (size_t)L * sizeof(unsigned long long);           // 48 KB at K = 1 024
    hipLaunchKernelGGL(nearest_kernel<false>, dim3((unsigned)(i_hi - i_lo)), dim3(SEL_NT), lds, st, cnt, S, i_lo, i_hi, c.filt_ambig, c.constant, c.kmax, c.pmax, K, L, lists,
                       n_candidates);
    if (S - i_lo - 1 > 0)
        hipLaunchKernelGGL(nearest_kernel<true>, dim3((unsigned)(S - i_lo - 1)), dim3(SEL_NT), lds, st, cnt, S, i_lo, i_hi, c.filt_ambig, c.constant, c.kmax, c.pmax, K, L, lists,
                           n_candidates);
}

}  // namespace skx
