// skx_lo.hip -- the device half of `ska lo` (read_graph.rs:build_graph + extremities.rs:identify_good_kmers): the coloured de Bruijn graph of
// an array as loaded, in CSR form, and the colours of full k-mers on demand.  The irregular half (compaction, the bounded DFS, the indel / SNP
// passes) runs on the host (host/ska_host.cpp, skh_lo).
//
//   lo_colour_kernel  per-row sample bitsets: a wave owns 64 rows and walks the samples 64 at a time (lane = sample), reading 64 bytes of its
//                     sample per tile; one ballot per (row, base) gives the row's 64-sample word.  Only the (row, base) pairs some sample has
//                     are written (their number per row comes from the array's row statistics, so the matrix is read once).
//   lo_emit_kernel    per present (row, base): the edges K[0..kg] -> K[1..k] and rc(K[1..k]) -> rc(K[0..kg]), the k-mer records K and rc(K)
//   CSR               edges sorted by (source, destination) with two stable radix passes; sources' run starts = nodes and offsets
//   k-mer table       records sorted by K; a run of equal K keeps the colour of the lowest (split k-mer, base): "the first writer wins"
//   lo_entry_kernel   a node with two or more children whose full k-mers' colours differ is an entry node; exits = their reverse complements
//   lo_gather_kernel  colours of a batch of full k-mers by binary search in the table
//
// Nodes and k-mers are in the reference's 2-bit code (A=0, C=1, T=2, G=3, first base in the high bits): uint64_t for k <= 31, u128 above.
// Colours are stored word-major: colour c's word t at colours[t * n_colours + c].
#include "skx_internal.h"
#include <algorithm>
#include <cstring>
#include <vector>

struct skx_lo_graph {
    skx_ctx *ctx = nullptr;
    int k = 0, wpn = 1;                  // words per node / k-mer: 1 (k <= 31) or 2
    uint64_t S = 0, W = 0;               // samples, colour words per (row, base)
    uint64_t n_colours = 0, n_table = 0;
    std::vector<uint64_t> nodes, offsets, nbrs, entries, exits;   // host CSR (nodes / nbrs / entries / exits: wpn words each)
    skx::DevBuf<uint64_t> tab;           // [n_table] sorted full k-mers (wpn words each)
    skx::DevBuf<uint32_t> tab_c;         // [n_table] their colour index
    skx::DevBuf<uint64_t> colours;       // [W][n_colours]
};

namespace skx {
namespace {

template <typename T> __host__ __device__ inline T rc_n(T v, int n)
{
    T out = 0;
    for (int i = 0; i < n; i++) { out = (out << 2) | (T)((uint32_t)(v & 3) ^ 2u); v >>= 2; }
    return out;
}

// ASCII middle base -> bit set over the 2-bit codes (read_graph.rs degenerate_code); 0 for '-' and anything else
__host__ __device__ inline uint32_t lo_base_set(uint32_t b)
{
    switch (b) {
    case 'A': return 1; case 'C': return 2; case 'T': return 4; case 'G': return 8;
    case 'M': return 3; case 'S': return 10; case 'W': return 5; case 'R': return 9; case 'Y': return 6; case 'K': return 12;
    case 'B': return 14; case 'D': return 13; case 'H': return 7; case 'V': return 11; case 'N': return 15;
    default: return 0;
    }
}

__global__ void lo_unmix_kernel(const uint64_t *words, uint64_t n, HashParams hp, uint64_t *out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = hunmix(words[i] >> 4, hp);
}
__global__ void lo_unmix_wide_kernel(const u128 *words, uint64_t n, WideHash wh, u128 *out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = hunmix_w(words[i] >> 4, wh);
}

// pass 1: bases present per row, from the row statistics (mask bit c = IUPAC set c occurs in the row)
__global__ void lo_count_kernel(const uint32_t *mask, uint64_t n_rows, uint32_t *rowset, uint32_t *count)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    uint32_t m = mask[r], set = 0;
    for (uint32_t c = 1; c < 16; c++) if ((m >> c) & 1u) set |= c;
    rowset[r] = set;
    count[r] = __popc(set);
}

// pass 2 (see the file comment).  pitch >= n_rows rounded up to 64 (pitch_for), so the 64-byte reads of the last row block stay inside the
// sample's row of the matrix.  *bad: a sample has a base the row statistics did not announce
__global__ __launch_bounds__(256) void lo_colour_kernel(const uint8_t *matrix, uint64_t pitch, uint64_t S, uint64_t n_rows, const uint32_t *rowset,
                                                        const uint32_t *incl, uint64_t n_colours, uint64_t W, uint64_t *colours, int *bad)
{
    __shared__ uint8_t lut[256];
    lut[threadIdx.x] = (uint8_t)lo_base_set(threadIdx.x);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t r0 = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (r0 >= n_rows) return;
    const uint64_t row = r0 + lane;
    const uint32_t myset = row < n_rows ? rowset[row] : 0;
    const uint64_t base = row < n_rows && row ? incl[row - 1] : 0;
    int mybad = 0;
    for (uint64_t t = 0; t < W; t++) {
        const uint64_t s = t * 64 + lane;
        uint4 v[4];
        if (s < S) {
            const uint4 *p = reinterpret_cast<const uint4 *>(matrix + s * pitch + r0);
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = p[j];
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = make_uint4(0x2d2d2d2du, 0x2d2d2d2du, 0x2d2d2d2du, 0x2d2d2d2du);
        }
        uint64_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
        for (int r = 0; r < 64; r++) {
            const uint4 q = v[r >> 4];
            const uint32_t x = ((r >> 2) & 3) == 0 ? q.x : ((r >> 2) & 3) == 1 ? q.y : ((r >> 2) & 3) == 2 ? q.z : q.w;
            const uint32_t set = lut[(x >> (8 * (r & 3))) & 0xFFu];
            const uint64_t b0 = __ballot(set & 1u), b1 = __ballot(set & 2u), b2 = __ballot(set & 4u), b3 = __ballot(set & 8u);
            if (lane == (uint32_t)r) { w0 = b0; w1 = b1; w2 = b2; w3 = b3; }
        }
        if (row < n_rows) {
            uint64_t c = base;
            const uint64_t w[4] = {w0, w1, w2, w3};
#pragma unroll
            for (int b = 0; b < 4; b++) {
                if ((myset >> b) & 1u) colours[t * n_colours + c++] = w[b];
                else if (w[b]) mybad = 1;
            }
        }
    }
    if (mybad) *bad = 1;
}

// per present (row, b) = colour c: edges 2c, 2c + 1 and k-mer records 2c, 2c + 1 (both with colour c); crow / cb: the colour's row and base
template <typename T>
__global__ void lo_emit_kernel(const T *keys, uint64_t n_rows, const uint32_t *rowset, const uint32_t *incl, int k, T *src, T *dst, T *kmer,
                               uint32_t *kval, uint32_t *crow, uint8_t *cb)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const int half = (k - 1) / 2, kg = k - 1;
    const T key = keys[r];
    const T left = key >> (2 * half), right = key & (((T)1 << (2 * half)) - 1);
    const T gmask = ((T)1 << (2 * kg)) - 1;
    uint64_t c = r ? incl[r - 1] : 0;
    const uint32_t set = rowset[r];
    for (uint32_t b = 0; b < 4; b++) {
        if (!((set >> b) & 1u)) continue;
        const T K = (left << (2 * (half + 1))) | ((T)b << (2 * half)) | right;
        const T s = K >> 2, d = K & gmask;
        src[2 * c] = s; dst[2 * c] = d;
        src[2 * c + 1] = rc_n(d, kg); dst[2 * c + 1] = rc_n(s, kg);
        kmer[2 * c] = K; kmer[2 * c + 1] = rc_n(K, k);
        kval[2 * c] = (uint32_t)c; kval[2 * c + 1] = (uint32_t)c;
        crow[c] = (uint32_t)r; cb[c] = (uint8_t)b;
        c++;
    }
}

__global__ void lo_iota_kernel(uint32_t *out, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (uint32_t)i;
}
template <typename T> __global__ void lo_permute_kernel(const T *in, const uint32_t *perm, T *out, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[perm[i]];
}
template <typename T> __global__ void lo_run_start_kernel(const T *sorted, uint64_t n, uint8_t *flag)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = i == 0 || sorted[i] != sorted[i - 1];
}
// one thread per run of equal K: the colour of the lowest (split k-mer, base) among the run
template <typename T>
__global__ void lo_fold_kernel(const T *sorted, const uint32_t *val, uint64_t n, const uint32_t *starts, uint64_t runs, const T *keys,
                               const uint32_t *crow, const uint8_t *cb, T *tab, uint32_t *tab_c)
{
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= runs) return;
    const uint64_t i0 = starts[u], i1 = u + 1 < runs ? starts[u + 1] : n;
    uint32_t best = val[i0];
    for (uint64_t i = i0 + 1; i < i1; i++) {
        const uint32_t c = val[i];
        const T kc = keys[crow[c]], kb = keys[crow[best]];
        if (kc < kb || (kc == kb && cb[c] < cb[best])) best = c;
    }
    tab[u] = sorted[i0]; tab_c[u] = best;
}

template <typename T> __device__ inline int64_t lo_find(const T *tab, uint64_t n, T key)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t m = (lo + hi) >> 1; if (tab[m] < key) lo = m + 1; else hi = m; }
    return lo < n && tab[lo] == key ? (int64_t)lo : -1;
}

// one thread per node: flag = some child's full k-mer colour differs from the first child's (= some pair differs)
template <typename T>
__global__ void lo_entry_kernel(const T *nodes, const uint32_t *starts, uint64_t n_nodes, uint64_t n_edges, const T *nbrs, const T *tab,
                                const uint32_t *tab_c, uint64_t n_table, const uint64_t *colours, uint64_t n_colours, uint64_t W, uint8_t *flag, int *bad)
{
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_nodes) return;
    const uint64_t e0 = starts[u], e1 = u + 1 < n_nodes ? starts[u + 1] : n_edges;
    uint8_t f = 0;
    if (e1 - e0 > 1) {
        const T node = nodes[u];
        int64_t c0 = -1;
        for (uint64_t e = e0; e < e1 && !f; e++) {
            const int64_t i = lo_find(tab, n_table, (T)((node << 2) | (nbrs[e] & 3)));
            if (i < 0) { *bad = 1; break; }
            const uint32_t c = tab_c[i];
            if (c0 < 0) { c0 = c; continue; }
            for (uint64_t t = 0; t < W; t++)
                if (colours[t * n_colours + c] != colours[t * n_colours + (uint64_t)c0]) { f = 1; break; }
        }
    }
    flag[u] = f;
}
template <typename T> __global__ void lo_rc_kernel(const T *in, uint64_t n, int len, T *out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = rc_n(in[i], len);
}
template <typename T>
__global__ void lo_gather_kernel(const T *q, uint64_t n, const T *tab, const uint32_t *tab_c, uint64_t n_table, const uint64_t *colours,
                                 uint64_t n_colours, uint64_t W, uint64_t *out, uint8_t *found)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t j = lo_find(tab, n_table, q[i]);
    found[i] = j >= 0;
    for (uint64_t t = 0; t < W; t++) out[i * W + t] = j >= 0 ? colours[t * n_colours + tab_c[j]] : 0;
}

inline unsigned grid(uint64_t n, unsigned b = 256) { return (unsigned)((n + b - 1) / b); }

int sort_pairs(const uint64_t *kin, uint64_t *kout, const uint32_t *vin, uint32_t *vout, uint64_t n, int bits, hipStream_t st)
{ return prim_sort_pairs_u64(kin, kout, vin, vout, n, bits, st); }
int sort_pairs(const u128 *kin, u128 *kout, const uint32_t *vin, uint32_t *vout, uint64_t n, int bits, hipStream_t st)
{ return prim_sort_pairs_u128(kin, kout, vin, vout, n, bits, st); }

template <typename T> void to_words(const std::vector<T> &v, std::vector<uint64_t> &out)
{
    out.resize(v.size() * (sizeof(T) / 8));
    if (!v.empty()) memcpy(out.data(), v.data(), v.size() * sizeof(T));
}

// the whole device pass for node type T; keys: the rows' split k-mers (row order) on the device
template <typename T>
int lo_graph_t(skx_array *a, const T *keys, skx_lo_graph *g)
{
    hipStream_t st = a->ctx->stream;
    const uint64_t R = a->n_rows, S = g->S, W = g->W;
    const int k = a->k, kg = k - 1;
    DevBuf<uint32_t> rowset, cnt, incl;
    SKX_TRY(rowset.alloc(R)); SKX_TRY(cnt.alloc(R)); SKX_TRY(incl.alloc(R));
    PhaseTimer t_col("lo.colour");
    hipLaunchKernelGGL(lo_count_kernel, dim3(grid(R)), dim3(256), 0, st, a->mask.p, R, rowset.p, cnt.p);
    SKX_TRY(prim_scan_add_u32(cnt.p, incl.p, R, st));
    uint32_t P32 = 0;
    SKX_HIP(hipMemcpyAsync(&P32, incl.p + (R - 1), 4, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    const uint64_t P = P32;
    g->n_colours = P;
    if (P == 0) { g->offsets.assign(1, 0); return SKX_OK; }
    if (a->pitch % 16 || a->pitch < (R + 63) / 64 * 64 || ((uintptr_t)a->matrix.p & 15)) { set_error("ska lo: unexpected matrix layout"); return SKX_EINVAL; }
    if (2 * P >= (1ull << 32)) { set_error("ska lo: %llu (row, base) pairs exceed the 32-bit edge index", (unsigned long long)P); return SKX_EUNSUP; }
    SKX_TRY(g->colours.alloc(std::max<uint64_t>(1, W * P)));
    DevBuf<int> bad; SKX_TRY(bad.alloc(1)); SKX_TRY(bad.zero(st));
    hipLaunchKernelGGL(lo_colour_kernel, dim3(grid(R, 256)), dim3(256), 0, st, a->matrix.p, a->pitch, S, R, rowset.p, incl.p, P, W,
                       g->colours.p, bad.p);
    SKX_HIP(hipGetLastError());
    SKX_HIP(hipStreamSynchronize(st));
    t_col.stop();

    PhaseTimer t_emit("lo.emit");
    const uint64_t E = 2 * P;
    DevBuf<T> src, dst, kmer, s2, d2; DevBuf<uint32_t> kval, crow, v1, v2; DevBuf<uint8_t> cb;
    SKX_TRY(src.alloc(E)); SKX_TRY(dst.alloc(E)); SKX_TRY(kmer.alloc(E)); SKX_TRY(kval.alloc(E)); SKX_TRY(crow.alloc(P)); SKX_TRY(cb.alloc(P));
    hipLaunchKernelGGL(lo_emit_kernel<T>, dim3(grid(R)), dim3(256), 0, st, keys, R, rowset.p, incl.p, k, src.p, dst.p, kmer.p, kval.p, crow.p, cb.p);
    SKX_HIP(hipGetLastError());
    SKX_HIP(hipStreamSynchronize(st));
    rowset.release(); cnt.release(); incl.release();
    t_emit.stop();

    // CSR: by destination, then stably by source
    PhaseTimer t_sort("lo.sort_edges");
    SKX_TRY(s2.alloc(E)); SKX_TRY(d2.alloc(E)); SKX_TRY(v1.alloc(E)); SKX_TRY(v2.alloc(E));
    hipLaunchKernelGGL(lo_iota_kernel, dim3(grid(E)), dim3(256), 0, st, v1.p, E);
    SKX_TRY(sort_pairs(dst.p, d2.p, v1.p, v2.p, E, 2 * kg, st));
    hipLaunchKernelGGL(lo_permute_kernel<T>, dim3(grid(E)), dim3(256), 0, st, src.p, v2.p, s2.p, E);      // s2 = sources in destination order
    SKX_TRY(sort_pairs(s2.p, src.p, v1.p, v2.p, E, 2 * kg, st));                                           // src = sorted sources
    hipLaunchKernelGGL(lo_permute_kernel<T>, dim3(grid(E)), dim3(256), 0, st, d2.p, v2.p, dst.p, E);      // dst = their destinations
    DevBuf<uint8_t> flag; DevBuf<uint32_t> starts; SKX_TRY(flag.alloc(E)); SKX_TRY(starts.alloc(E));
    hipLaunchKernelGGL(lo_run_start_kernel<T>, dim3(grid(E)), dim3(256), 0, st, src.p, E, flag.p);
    uint64_t N = 0;
    SKX_TRY(prim_select_index_u8(flag.p, starts.p, E, &N, st));
    DevBuf<T> nodes; SKX_TRY(nodes.alloc(N));
    hipLaunchKernelGGL(lo_permute_kernel<T>, dim3(grid(N)), dim3(256), 0, st, src.p, starts.p, nodes.p, N);
    SKX_HIP(hipGetLastError());
    SKX_HIP(hipStreamSynchronize(st));
    s2.release(); d2.release(); src.release();
    t_sort.stop();

    // k-mer table: sorted by K, runs folded to the lowest (split k-mer, base)
    PhaseTimer t_tab("lo.sort_kmers");
    DevBuf<T> ksorted; SKX_TRY(ksorted.alloc(E));
    SKX_TRY(sort_pairs(kmer.p, ksorted.p, kval.p, v2.p, E, 2 * k, st));
    kmer.release();
    hipLaunchKernelGGL(lo_run_start_kernel<T>, dim3(grid(E)), dim3(256), 0, st, ksorted.p, E, flag.p);
    uint64_t U = 0;
    SKX_TRY(prim_select_index_u8(flag.p, v1.p, E, &U, st));
    DevBuf<T> tab; SKX_TRY(tab.alloc(U)); SKX_TRY(g->tab_c.alloc(U));
    hipLaunchKernelGGL(lo_fold_kernel<T>, dim3(grid(U)), dim3(256), 0, st, ksorted.p, v2.p, E, v1.p, U, keys, crow.p, cb.p, tab.p, g->tab_c.p);
    SKX_HIP(hipGetLastError());
    SKX_HIP(hipStreamSynchronize(st));
    g->n_table = U;
    ksorted.release();
    t_tab.stop();

    PhaseTimer t_entry("lo.entry");
    DevBuf<uint8_t> eflag; DevBuf<uint32_t> eidx; SKX_TRY(eflag.alloc(N)); SKX_TRY(eidx.alloc(N));
    hipLaunchKernelGGL(lo_entry_kernel<T>, dim3(grid(N)), dim3(256), 0, st, nodes.p, starts.p, N, E, dst.p, tab.p, g->tab_c.p, U, g->colours.p, P, W,
                       eflag.p, bad.p);
    uint64_t NE = 0;
    SKX_TRY(prim_select_index_u8(eflag.p, eidx.p, N, &NE, st));
    DevBuf<T> ent, ex, exs; SKX_TRY(ent.alloc(NE)); SKX_TRY(ex.alloc(NE)); SKX_TRY(exs.alloc(NE));
    if (NE) {
        hipLaunchKernelGGL(lo_permute_kernel<T>, dim3(grid(NE)), dim3(256), 0, st, nodes.p, eidx.p, ent.p, NE);
        hipLaunchKernelGGL(lo_rc_kernel<T>, dim3(grid(NE)), dim3(256), 0, st, ent.p, NE, kg, ex.p);
        SKX_TRY(sort_pairs(ex.p, exs.p, eidx.p, v1.p, NE, 2 * kg, st));
    }
    SKX_HIP(hipGetLastError());
    SKX_HIP(hipStreamSynchronize(st));
    int h_bad = 0;
    SKX_HIP(hipMemcpy(&h_bad, bad.p, 4, hipMemcpyDeviceToHost));
    if (h_bad) { set_error("ska lo: the colour table disagrees with the array's row statistics"); return SKX_EINVAL; }
    t_entry.stop();

    PhaseTimer t_copy("lo.copy_csr");
    std::vector<T> hn(N), hb(E), he(NE), hx(NE); std::vector<uint32_t> hs(N);
    if (N) {
        SKX_HIP(hipMemcpyAsync(hn.data(), nodes.p, N * sizeof(T), hipMemcpyDeviceToHost, st));
        SKX_HIP(hipMemcpyAsync(hs.data(), starts.p, N * 4, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipMemcpyAsync(hb.data(), dst.p, E * sizeof(T), hipMemcpyDeviceToHost, st));
    }
    if (NE) {
        SKX_HIP(hipMemcpyAsync(he.data(), ent.p, NE * sizeof(T), hipMemcpyDeviceToHost, st));
        SKX_HIP(hipMemcpyAsync(hx.data(), exs.p, NE * sizeof(T), hipMemcpyDeviceToHost, st));
    }
    SKX_HIP(hipStreamSynchronize(st));
    to_words(hn, g->nodes); to_words(hb, g->nbrs); to_words(he, g->entries); to_words(hx, g->exits);
    g->offsets.assign(hs.begin(), hs.end()); g->offsets.push_back(E);
    SKX_TRY(g->tab.alloc(U * g->wpn));
    if (U) SKX_HIP(hipMemcpyAsync(g->tab.p, tab.p, U * sizeof(T), hipMemcpyDeviceToDevice, st));
    SKX_HIP(hipStreamSynchronize(st));
    return SKX_OK;
}

template <typename T>
int lo_gather_t(skx_lo_graph *g, const uint64_t *kmers, uint64_t n, uint64_t *colours, uint8_t *found)
{
    hipStream_t st = g->ctx->stream;
    DevBuf<T> q; DevBuf<uint64_t> out; DevBuf<uint8_t> f;
    SKX_TRY(q.alloc(n)); SKX_TRY(out.alloc(n * g->W)); SKX_TRY(f.alloc(n));
    SKX_HIP(hipMemcpyAsync(q.p, kmers, n * sizeof(T), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(lo_gather_kernel<T>, dim3(grid(n)), dim3(256), 0, st, q.p, n, (const T *)g->tab.p, g->tab_c.p, g->n_table, g->colours.p,
                       g->n_colours, g->W, out.p, f.p);
    SKX_HIP(hipGetLastError());
    SKX_HIP(hipMemcpyAsync(colours, out.p, n * g->W * 8, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipMemcpyAsync(found, f.p, n, hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    return SKX_OK;
}

}  // namespace
}  // namespace skx

using namespace skx;

extern "C" int skx_array_lo_graph(skx_array *a, skx_lo_graph **out)
{
    return skx_guarded([&]() -> int {
    if (!a || !out) { set_error("bad arguments"); return SKX_EINVAL; }
    *out = nullptr;
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    const uint64_t S = a->names.size();
    // read_graph.rs: sample indexes are u16
    if (S > 65535) { set_error("ska lo: %llu samples; sample indexes are 16-bit (at most 65535 samples)", (unsigned long long)S); return SKX_EUNSUP; }
    if (a->total_samples && a->total_samples != S) { set_error("ska lo: needs every sample of the array on one device"); return SKX_EUNSUP; }
    if (a->keys_absent || a->n_kmers != a->n_rows) { set_error("ska lo: the array's split k-mers do not match its rows"); return SKX_EINVAL; }
    SKX_TRY(array_materialize(a));
    if (!a->stats_ready) SKX_TRY(array_lazy_stats(a));
    std::unique_ptr<skx_lo_graph> g(new skx_lo_graph());
    g->ctx = ctx; g->k = a->k; g->wpn = a->k <= 31 ? 1 : 2; g->S = S; g->W = (S + 63) / 64;
    const uint64_t R = a->n_rows;
    if (R == 0) { g->offsets.assign(1, 0); *out = g.release(); return SKX_OK; }
    PhaseTimer t_keys("lo.keys");
    if (a->k <= 31) {
        DevBuf<uint64_t> keys; SKX_TRY(keys.alloc(R));
        hipLaunchKernelGGL(lo_unmix_kernel, dim3(grid(R)), dim3(256), 0, st, a->keys.p, R, a->hp, keys.p);
        SKX_HIP(hipGetLastError());
        t_keys.stop();
        SKX_TRY(lo_graph_t<uint64_t>(a, keys.p, g.get()));
    } else {
        DevBuf<u128> keys; SKX_TRY(keys.alloc(R));
        if (!a->host_keys.empty()) {
            static_assert(sizeof(skx_key) == 16 && offsetof(skx_key, lo) == 0, "skx_key is a little-endian u128");
            SKX_HIP(hipMemcpyAsync(keys.p, a->host_keys.data(), R * 16, hipMemcpyHostToDevice, st));
        } else {
            hipLaunchKernelGGL(lo_unmix_wide_kernel, dim3(grid(R)), dim3(256), 0, st, (const u128 *)a->keys.p, R, a->wh, keys.p);
        }
        SKX_HIP(hipGetLastError());
        SKX_HIP(hipStreamSynchronize(st));
        t_keys.stop();
        SKX_TRY(lo_graph_t<u128>(a, keys.p, g.get()));
    }
    *out = g.release();
    return SKX_OK;
    });
}

extern "C" int skx_lo_graph_info(const skx_lo_graph *g, skx_lo_info *info)
{
    if (!g || !info) { set_error("bad arguments"); return SKX_EINVAL; }
    info->k = g->k; info->words_per_node = g->wpn; info->n_samples = g->S; info->colour_words = g->W;
    info->n_nodes = g->nodes.size() / g->wpn; info->n_edges = g->nbrs.size() / g->wpn; info->n_entries = g->entries.size() / g->wpn;
    info->n_colours = g->n_colours; info->n_kmers = g->n_table;
    return SKX_OK;
}

extern "C" int skx_lo_graph_export(const skx_lo_graph *g, uint64_t *nodes, uint64_t *offsets, uint64_t *neighbours, uint64_t *entries, uint64_t *exits)
{
    if (!g) { set_error("bad arguments"); return SKX_EINVAL; }
    auto put = [](uint64_t *dst, const std::vector<uint64_t> &v) { if (dst && !v.empty()) memcpy(dst, v.data(), v.size() * 8); };
    put(nodes, g->nodes); put(offsets, g->offsets); put(neighbours, g->nbrs); put(entries, g->entries); put(exits, g->exits);
    return SKX_OK;
}

extern "C" int skx_lo_gather(skx_lo_graph *g, const uint64_t *kmers, uint64_t n, uint64_t *colours, uint8_t *found)
{
    return skx_guarded([&]() -> int {
    if (!g || (n && (!kmers || !colours || !found))) { set_error("bad arguments"); return SKX_EINVAL; }
    if (!n) return SKX_OK;
    SKX_HIP(hipSetDevice(g->ctx->device));
    PhaseTimer t("lo.gather");
    return g->wpn == 1 ? lo_gather_t<uint64_t>(g, kmers, n, colours, found) : lo_gather_t<u128>(g, kmers, n, colours, found);
    });
}

extern "C" void skx_lo_graph_free(skx_lo_graph *g) { delete g; }
