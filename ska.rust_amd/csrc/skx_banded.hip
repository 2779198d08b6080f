// skx_banded.hip -- the consumers of `ska distance --no-table` (skx_array_distance_banded of include/skx.h): what the single-linkage clusters and
// the neighbour-joining tree need of one band of the pair matrix, taken from the band's count buffer [band][S][DIST_NCOUNT] as launch_pair_counts
// leaves it and kept on the device.  Nothing of a band reaches the host; after the last band S labels and S - 1 join records do.
//
// A workgroup per row i of the band, lanes over j > i, the walk of select_count_kernel (skx_select.hip), the same sel_pair (skx_internal.h):
//   cluster_union_kernel   every pair that passes (kmax, pmax) joins the trees of i and j in parent[S] (parent[x] <= x, a root has parent[x] == x);
//                          a wave first reduces its row's roots to the smallest met, then links each other root to that one
//   cluster_labels_kernel  after the last band: label[i] = the root of i, and the number of roots
//   dist_fill_kernel       D[i][j] = D[j][i] = the pair's distance in the pitched matrix nj_run takes (skx_nj.hip)
//
// The union: a link always points the HIGHER root at the LOWER one, by one 32-bit atomicMin on parent[higher].  Where the atomic finds that
// the higher node had been given a parent in the meantime it has still lowered that node's parent to min(old, lower), which keeps the node
// attached; what is left to join are the trees of `old` and `lower`, and the loop carries on with those two.  parent[] only ever decreases and
// parent[x] <= x, so no cycle can form, the root of a component is its lowest sample, and the final partition -- the connected components of
// the passing pairs -- and therefore every label is the same whatever the order of lanes, workgroups and bands.  No float atomics; the
// mismatch threshold is finish_pair's add and divide in float64, each rounded once: this file is compiled with -ffp-contract=off (Makefile).
#include "skx_internal.h"
#include "skx_unionfind.h"

namespace skx {
namespace {

constexpr int BND_NT = 256;                       // threads of the row workgroups

// (uf_root / uf_link: skx_unionfind.h, shared with skx_mst.hip)

__global__ void cluster_init_kernel(uint32_t *parent, int S)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < S) parent[i] = (uint32_t)i;
}

// ROW_WIDE: every edge of a row shares i, so a wave first reduces the roots of its passing j (and of i) to the smallest one met and then makes
// one link per lane whose root differs from it -- none at all once the row's samples hang under one root, which is what a dense band comes to
// after its first rows.  !ROW_WIDE: the plain form, one uf_link per edge (kept for the comparison: SKX_KNOBS=union_per_edge, NOTEBOOK).
template <bool ROW_WIDE>
__global__ __launch_bounds__(BND_NT) void cluster_union_kernel(const unsigned long long *cnt, int S, int i_lo, int i_hi, int filt_ambig, double constant,
                                                               unsigned long long kmax, double pmax, uint32_t *parent, unsigned long long *n_edges)
{
    const int i = i_lo + (int)blockIdx.x;
    if (i >= i_hi) return;
    const unsigned long long *row = cnt + (uint64_t)(i - i_lo) * S * DIST_NCOUNT;
    const int lane = threadIdx.x & 63;
    uint32_t n = 0;
    for (int j0 = i + 1 + (int)(threadIdx.x & ~63u); j0 < S; j0 += BND_NT) {       // (uniform over a wave: the shuffles below are reached by all of its lanes)
        const int j = j0 + lane;
        SelPair p;
        const bool edge = j < S && sel_pair(row + (uint64_t)j * DIST_NCOUNT, filt_ambig, constant, kmax, pmax, p);
        n += edge ? 1u : 0u;
        if (!ROW_WIDE) { if (edge) uf_link(parent, (uint32_t)i, (uint32_t)j); continue; }
        if (!__any(edge)) continue;
        const uint32_t rj = edge ? uf_root(parent, (uint32_t)j) : 0xFFFFFFFFu, ri = uf_root(parent, (uint32_t)i);
        uint32_t low = rj < ri ? rj : ri;
        for (int off = 32; off; off >>= 1) { const uint32_t o = __shfl_xor(low, off, 64); low = o < low ? o : low; }
        if (edge && rj != low) uf_link(parent, rj, low);
        if (lane == 0 && ri != low) uf_link(parent, ri, low);
    }
    for (int off = 32; off; off >>= 1) n += __shfl_xor(n, off, 64);
    if (lane == 0 && n) atomicAdd(n_edges, (unsigned long long)n);
}

__global__ __launch_bounds__(BND_NT) void cluster_labels_kernel(const uint32_t *parent, int S, uint32_t *label, unsigned long long *n_roots)
{
    const int i = (int)(blockIdx.x * BND_NT + threadIdx.x);
    uint32_t r = 0xFFFFFFFFu;
    if (i < S) { r = uf_root(parent, (uint32_t)i); label[i] = r; }
    const unsigned long long roots = __ballot(i < S && r == (uint32_t)i);
    if ((threadIdx.x & 63) == 0 && roots) atomicAdd(n_roots, (unsigned long long)__popcll(roots));
}

// the row writes are contiguous, the mirrored column writes 8-byte stores a pitch apart (the plain form)
__global__ __launch_bounds__(BND_NT) void dist_fill_kernel(const unsigned long long *cnt, int S, int i_lo, int i_hi, int filt_ambig, double *D, uint64_t pitch)
{
    const int i = i_lo + (int)blockIdx.x;
    if (i >= i_hi) return;
    const unsigned long long *row = cnt + (uint64_t)(i - i_lo) * S * DIST_NCOUNT;
    for (int j = i + 1 + (int)threadIdx.x; j < S; j += BND_NT) {
        SelPair p;
        (void)sel_pair(row + (uint64_t)j * DIST_NCOUNT, filt_ambig, 0.0, ~0ull, -1.0, p);
        const double d = key_distance(p.key, filt_ambig);
        D[(uint64_t)i * pitch + (uint64_t)j] = d;
        D[(uint64_t)j * pitch + (uint64_t)i] = d;
    }
}

}  // namespace

void launch_cluster_init(uint32_t *parent, int S, hipStream_t st)
{
    if (S < 1) return;
    hipLaunchKernelGGL(cluster_init_kernel, dim3((unsigned)((S + BND_NT - 1) / BND_NT)), dim3(BND_NT), 0, st, parent, S);
}
void launch_cluster_union(const unsigned long long *cnt, int S, int i_lo, int i_hi, const SelCriteria &c, uint32_t *parent, unsigned long long *n_edges, bool per_edge,
                          hipStream_t st)
{
    if (i_hi <= i_lo) return;
    const dim3 grid((unsigned)(i_hi - i_lo)), block(BND_NT);
    if (per_edge) hipLaunchKernelGGL(cluster_union_kernel<false>, grid, block, 0, st, cnt, S, i_lo, i_hi, c.filt_ambig, c.constant, c.kmax, c.pmax, parent, n_edges);
    else hipLaunchKernelGGL(cluster_union_kernel<true>, grid, block, 0, st, cnt, S, i_lo, i_hi, c.filt_ambig, c.constant, c.kmax, c.pmax, parent, n_edges);
}
void launch_cluster_labels(const uint32_t *parent, int S, uint32_t *label, unsigned long long *n_roots, hipStream_t st)
{
    if (S < 1) return;
    hipLaunchKernelGGL(cluster_labels_kernel, dim3((unsigned)((S + BND_NT - 1) / BND_NT)), dim3(BND_NT), 0, st, parent, S, label, n_roots);
}
void launch_dist_fill(const unsigned long long *cnt, int S, int i_lo, int i_hi, int filt_ambig, double *D, uint64_t pitch, hipStream_t st)
{
    if (i_hi <= i_lo) return;
    hipLaunchKernelGGL(dist_fill_kernel, dim3((unsigned)(i_hi - i_lo)), dim3(BND_NT), 0, st, cnt, S, i_lo, i_hi, filt_ambig, D, pitch);
}

}  // namespace skx
