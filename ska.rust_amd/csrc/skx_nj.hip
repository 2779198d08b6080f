// skx_nj.hip -- neighbour joining on the device (`ska distance --tree`; skx_dist_nj / skx_matrix_nj of include/skx.h): canonical NJ (Saitou-Nei
// with the Studier-Keppler Q criterion) in float64 on a dense symmetric matrix that stays on the device from the first join to the last.
//
// The live nodes occupy the leading n x n block of the matrix (compaction, not masking: a join puts the new node into the lower of the two
// slots and moves the last live slot into the other, so the row pass reads n^2 / 2 values per step instead of S^2, a sixth of the traffic
// over a whole run).  The tie rule is on node ids, which ids[slot] carries, so the slot shuffle does not show in the result.
//
// One step = four plain launches on the context's stream (a step is a grid-wide all-to-all seam; nothing comes back to the host between steps):
//   nj_row_kernel     a wave per live row x: Q(x, y) for the slots y > x (the matrix is symmetric; every pair is seen once), 16-byte loads
//                     along the row, the minimum with its (min id, max id) carried through a wave reduction, one (q, id, id, y) per row
//   nj_pick_kernel    one workgroup: the minimum over rows, the join record and its two lengths, the step's selection (slots, D[a][b], r[u])
//   nj_new_kernel     per live slot k: the new node's distance u[k], the updated r[k], and a copy of the last live row
//   nj_write_kernel   per live slot k: row and column of the new node, the last live slot moved into the retired one, r and ids
// Row sums r are kept incrementally (r[k] += u[k] - D[a][k] - D[b][k]; r[u] = (r[a] + r[b] - n D[a][b]) / 2).  No float atomics and no
// order-dependent reduction: the same input gives the same records bit for bit.  This file is compiled with -ffp-contract=off (Makefile),
// so a recorded length does not depend on where the compiler would have formed an FMA.
#include "skx_internal.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace skx {
namespace {

constexpr uint32_t NJ_NONE = 0xFFFFFFFFu;

// the step's selection, written by nj_pick_kernel and read by the two update kernels
struct NjSel { uint32_t lo, hi, id_new, pad; double dab, ru; };

struct NjBest { double q; uint32_t a, b, y; };     // a < b: node ids; y: the slot of the row's partner

// (q, min id, max id) in lexicographic order; NJ_NONE ids lose every tie
__device__ inline bool nj_less(double q1, uint32_t a1, uint32_t b1, double q2, uint32_t a2, uint32_t b2)
{
    if (q1 != q2) return q1 < q2;
    if (a1 != a2) return a1 < a2;
    return b1 < b2;
}
__device__ inline void nj_take(NjBest &m, double q, uint32_t a, uint32_t b, uint32_t y)
{
    if (nj_less(q, a, b, m.q, m.a, m.b)) { m.q = q; m.a = a; m.b = b; m.y = y; }
}
__device__ inline NjBest nj_wave_min(NjBest m)
{
    for (int off = 32; off; off >>= 1) {
        const double q = __shfl_xor(m.q, off, 64);
        const uint32_t a = __shfl_xor(m.a, off, 64), b = __shfl_xor(m.b, off, 64), y = __shfl_xor(m.y, off, 64);
        nj_take(m, q, a, b, y);
    }
    return m;
}

// packed upper triangle (pairs i < j row-major) -> the full symmetric matrix with a zero diagonal
__global__ void nj_expand_kernel(const double *tri, uint32_t S, uint64_t pitch, double *D)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= S || i >= S) return;
    double v = 0.0;
    if (i != j) {
        const uint64_t a = i < j ? i : j, b = i < j ? j : i;
        v = tri[a * (2 * (uint64_t)S - a - 1) / 2 + (b - a - 1)];
    }
    D[(uint64_t)i * pitch + j] = v;
}

// r[x] = sum of row x in slot order (one wave per row; the lanes' partial sums are combined in a fixed tree)
__global__ void nj_rowsum_kernel(const double *D, uint32_t S, uint64_t pitch, double *r, uint32_t *ids)
{
    const uint32_t x = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (x >= S) return;
    const double *row = D + (uint64_t)x * pitch;
    double s = 0.0;
    for (uint32_t y = lane; y < S; y += 64) s += row[y];
    for (int off = 32; off; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) { r[x] = s; ids[x] = x; }
}

__global__ void __launch_bounds__(256) nj_row_kernel(const double *D, uint64_t pitch, uint32_t n, const double *r, const uint32_t *ids,
                                                     double *row_q, uint32_t *row_a, uint32_t *row_b, uint32_t *row_y)
{
    const uint32_t x = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (x >= n) return;
    const double *row = D + (uint64_t)x * pitch;
    const double nm2 = (double)(n - 2), rx = r[x];
    const uint32_t idx = ids[x];
    NjBest m{INFINITY, NJ_NONE, NJ_NONE, NJ_NONE};
    // pairs of columns from the one that holds x + 1, 16 bytes of the row and of r per lane and load (rows are 16-byte aligned: pitch is even;
    // r and ids have a pad element).  A pair's second column exists in the allocation even where it is outside the live block; what is not
    // a partner of x (the diagonal, a column past the block) takes part with q = +inf and no ids, so the loads stay unconditional.
    for (uint32_t y0 = ((x + 1) & ~1u) + 2 * lane; y0 < n; y0 += 128) {
        const double2 d = *reinterpret_cast<const double2 *>(row + y0);
        const double2 ry = *reinterpret_cast<const double2 *>(r + y0);
        const uint2 iy = *reinterpret_cast<const uint2 *>(ids + y0);
        const bool ok0 = y0 > x, ok1 = y0 + 1 < n;            // (y0 + 1 > x always: y0 >= x + 1 or y0 == x)
        const double q0 = nm2 * d.x - (rx + ry.x), q1 = nm2 * d.y - (rx + ry.y);
        const uint32_t a0 = idx < iy.x ? idx : iy.x, b0 = idx < iy.x ? iy.x : idx, a1 = idx < iy.y ? idx : iy.y, b1 = idx < iy.y ? iy.y : idx;
        nj_take(m, ok0 ? q0 : INFINITY, ok0 ? a0 : NJ_NONE, ok0 ? b0 : NJ_NONE, y0);
        nj_take(m, ok1 ? q1 : INFINITY, ok1 ? a1 : NJ_NONE, ok1 ? b1 : NJ_NONE, y0 + 1);
    }
    m = nj_wave_min(m);
    if (lane == 0) { row_q[x] = m.q; row_a[x] = m.a; row_b[x] = m.b; row_y[x] = m.y; }
}

__global__ void __launch_bounds__(1024) nj_pick_kernel(const double *D, uint64_t pitch, uint32_t n, uint32_t id_new, const double *r, const uint32_t *ids,
                                                       const double *row_q, const uint32_t *row_a, const uint32_t *row_b, const uint32_t *row_y,
                                                       skx_nj_join *join, NjSel *sel)
{
    __shared__ double sq[16];
    __shared__ uint32_t sa[16], sb[16], sx[16];
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    // NjBest::y carries the ROW here: the partner's slot is looked up once the row is known
    NjBest m{INFINITY, NJ_NONE, NJ_NONE, NJ_NONE};
    for (uint32_t x = t; x < n; x += 1024) nj_take(m, row_q[x], row_a[x], row_b[x], x);
    m = nj_wave_min(m);
    if (lane == 0) { sq[w] = m.q; sa[w] = m.a; sb[w] = m.b; sx[w] = m.y; }
    __syncthreads();
    if (t != 0) return;
    for (uint32_t i = 1; i < 16; i++) nj_take(m, sq[i], sa[i], sb[i], sx[i]);
    uint32_t x = m.y, y = x < n ? row_y[x] : NJ_NONE;        // slots, x < y
    if (x >= n || y >= n) { x = 0; y = 1; }                  // (no finite Q: cannot happen on the finite input the entry points admit; stay inside the block)
    // a < b by id
    const uint32_t s_a = ids[x] < ids[y] ? x : y, s_b = s_a == x ? y : x;
    const double dab = D[(uint64_t)x * pitch + y], ra = r[s_a], rb = r[s_b];
    const double len_a = dab / 2.0 + (ra - rb) / (2.0 * (double)(n - 2));
    join->a = ids[s_a]; join->b = ids[s_b]; join->len_a = len_a; join->len_b = dab - len_a;
    sel->lo = x; sel->hi = y; sel->id_new = id_new; sel->pad = 0; sel->dab = dab;
    sel->ru = ((ra + rb) - (double)n * dab) / 2.0;
}

__global__ void nj_new_kernel(const double *D, uint64_t pitch, uint32_t n, const NjSel *sel, const double *r, double *u, double *rn, double *last)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t lo = sel->lo, hi = sel->hi;
    const double dl = D[(uint64_t)lo * pitch + k], dh = D[(uint64_t)hi * pitch + k];
    const double v = (k == lo || k == hi) ? 0.0 : ((dl + dh) - sel->dab) / 2.0;
    u[k] = v;
    rn[k] = ((r[k] - dl) - dh) + v;
    last[k] = D[(uint64_t)(n - 1) * pitch + k];
}

// n: the live slots before the join; afterwards the slots 0 .. n-2 are live
__global__ void nj_write_kernel(double *D, uint64_t pitch, uint32_t n, const NjSel *sel, double *r, uint32_t *ids, const double *u, const double *rn,
                                const double *last)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t L = n - 1;
    if (k >= L) return;
    const uint32_t lo = sel->lo, hi = sel->hi;
    const bool move = hi != L;                               // the last live slot takes the retired one
    if (k != hi) {
        const double v = u[k];                               // (u[lo] == 0: the diagonal)
        D[(uint64_t)lo * pitch + k] = v; D[(uint64_t)k * pitch + lo] = v;
        r[k] = k == lo ? sel->ru : rn[k];
        if (k == lo) ids[lo] = sel->id_new;
    }
    if (move) {
        // the moved node's distances: to the new node u[L], to itself 0, to the others as they were
        const double mv = k == lo ? u[L] : k == hi ? 0.0 : last[k];
        D[(uint64_t)hi * pitch + k] = mv; D[(uint64_t)k * pitch + hi] = mv;
        if (k == hi) { r[hi] = rn[L]; ids[hi] = ids[L]; }
    }
}

// the two nodes that are left
__global__ void nj_last_kernel(const double *D, uint64_t pitch, const uint32_t *ids, skx_nj_join *join)
{
    if (blockIdx.x || threadIdx.x) return;
    const uint32_t s_a = ids[0] < ids[1] ? 0 : 1;
    join->a = ids[s_a]; join->b = ids[1 - s_a]; join->len_a = D[1]; join->len_b = 0.0;
}

inline unsigned nj_grid(uint64_t n, unsigned b) { return (unsigned)((n + b - 1) / b); }

}  // namespace

// the matrix of S nodes on the device, pitch doubles per row (even, so that every row starts on 16 bytes)
uint64_t nj_pitch(uint64_t S) { return (S + 1) & ~(uint64_t)1; }

// refuses a matrix the device cannot hold (8 S^2 bytes plus `extra`) with a message instead of a failed allocation half way
int nj_fits(skx_ctx *ctx, uint64_t S, uint64_t extra)
{
    const uint64_t need = nj_pitch(S) * S * 8 + extra + S * 64 + (64ull << 20);
    size_t fr = 0, tot = 0;
    SKX_HIP(hipMemGetInfo(&fr, &tot));
    if (need > fr) { dev_trim(); SKX_HIP(hipMemGetInfo(&fr, &tot)); }
    if (need > fr) {
        set_error("neighbour joining: the %llu x %llu matrix needs %.1f GB on the device, %.1f GB are free", (unsigned long long)S, (unsigned long long)S,
                  (double)need / 1e9, (double)fr / 1e9);
        return SKX_ENOMEM;
    }
    return SKX_OK;
}

// D: the S x S matrix on the device (destroyed by the run); joins: S - 1 records on the host
static int nj_run(skx_ctx *ctx, DevBuf<double> &D, uint64_t pitch, uint32_t S, skx_nj_join *joins)
{
    hipStream_t st = ctx->stream;
    PhaseTimer ts("nj.steps");
    // workspace, all of it before the first step
    DevBuf<double> r, u, rn, last, row_q; DevBuf<uint32_t> ids, row_a, row_b, row_y; DevBuf<skx_nj_join> dj; DevBuf<NjSel> sel;
    SKX_TRY(r.alloc(S + 2)); SKX_TRY(u.alloc(S)); SKX_TRY(rn.alloc(S)); SKX_TRY(last.alloc(S)); SKX_TRY(row_q.alloc(S));
    SKX_TRY(ids.alloc(S + 2)); SKX_TRY(row_a.alloc(S)); SKX_TRY(row_b.alloc(S)); SKX_TRY(row_y.alloc(S));
    SKX_TRY(dj.alloc(S - 1)); SKX_TRY(sel.alloc(1));
    SKX_TRY(r.zero(st)); SKX_TRY(ids.zero(st));                              // (the pad elements are loaded, never used)
    hipLaunchKernelGGL(nj_rowsum_kernel, dim3(nj_grid(S, 4)), dim3(256), 0, st, D.p, S, pitch, r.p, ids.p);
    for (uint32_t n = S, t = 0; n > 2; n--, t++) {
        hipLaunchKernelGGL(nj_row_kernel, dim3(nj_grid(n, 4)), dim3(256), 0, st, D.p, pitch, n, r.p, ids.p, row_q.p, row_a.p, row_b.p, row_y.p);
        hipLaunchKernelGGL(nj_pick_kernel, dim3(1), dim3(1024), 0, st, D.p, pitch, n, S + t, r.p, ids.p, row_q.p, row_a.p, row_b.p, row_y.p, dj.p + t, sel.p);
        hipLaunchKernelGGL(nj_new_kernel, dim3(nj_grid(n, 256)), dim3(256), 0, st, D.p, pitch, n, sel.p, r.p, u.p, rn.p, last.p);
        hipLaunchKernelGGL(nj_write_kernel, dim3(nj_grid(n - 1, 256)), dim3(256), 0, st, D.p, pitch, n, sel.p, r.p, ids.p, u.p, rn.p, last.p);
    }
    hipLaunchKernelGGL(nj_last_kernel, dim3(1), dim3(64), 0, st, D.p, pitch, ids.p, dj.p + (S - 2));
    SKX_HIP(hipGetLastError());
    SKX_HIP(hipMemcpyAsync(joins, dj.p, (size_t)(S - 1) * sizeof(skx_nj_join), hipMemcpyDeviceToHost, st));
    SKX_HIP(hipStreamSynchronize(st));
    return SKX_OK;
}

int nj_check_n(int n)
{
    if (n < 2) { set_error("neighbour joining needs at least 2 samples (%d given)", n); return SKX_EINVAL; }
    if (n > 65535) { set_error("neighbour joining: %d samples; at most 65535", n); return SKX_EUNSUP; }
    return SKX_OK;
}
// the entry of the banded form (skx_distance.cpp), which fills the matrix on the device itself
int nj_run_device(skx_ctx *ctx, DevBuf<double> &D, uint64_t pitch, uint32_t S, skx_nj_join *joins) { return nj_run(ctx, D, pitch, S, joins); }

}  // namespace skx

using namespace skx;

static_assert(sizeof(skx_nj_join) == 24, "skx_nj_join is two ids and two doubles");

extern "C" int skx_dist_nj(skx_ctx *ctx, const skx_dist *d, int n_samples, skx_nj_join *joins)
{
    return skx_guarded([&]() -> int {
    if (!ctx || !d || !joins) { set_error("bad arguments"); return SKX_EINVAL; }
    SKX_TRY(nj_check_n(n_samples));
    SKX_HIP(hipSetDevice(ctx->device));
    const uint64_t S = (uint64_t)n_samples, P = S * (S - 1) / 2, pitch = nj_pitch(S);
    std::vector<double> tri(P);
    for (uint64_t i = 0; i < P; i++) {
        tri[i] = d[i].distance;
        if (!std::isfinite(tri[i])) { set_error("neighbour joining: pair %llu of the table has no finite distance", (unsigned long long)i); return SKX_EINVAL; }
    }
    SKX_TRY(nj_fits(ctx, S, P * 8));
    DevBuf<double> D, dtri;
    SKX_TRY(D.alloc(pitch * S)); SKX_TRY(dtri.alloc(P));
    hipStream_t st = ctx->stream;
    SKX_HIP(hipMemsetAsync(D.p, 0, pitch * S * 8, st));                     // (the pad column of an odd S is loaded, never used)
    PhaseTimer tu("nj.upload");
    SKX_HIP(hipMemcpyAsync(dtri.p, tri.data(), P * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(nj_expand_kernel, dim3(nj_grid(S, 256), (unsigned)S), dim3(256), 0, st, dtri.p, (uint32_t)S, pitch, D.p);
    SKX_HIP(hipGetLastError());
    SKX_HIP(hipStreamSynchronize(st));                                       // tri goes out of use
    dtri.release();
    tu.stop();
    return nj_run(ctx, D, pitch, (uint32_t)S, joins);
    });
}

extern "C" int skx_matrix_nj(skx_ctx *ctx, const double *m, int n, skx_nj_join *joins)
{
    return skx_guarded([&]() -> int {
    if (!ctx || !m || !joins) { set_error("bad arguments"); return SKX_EINVAL; }
    SKX_TRY(nj_check_n(n));
    const uint64_t S = (uint64_t)n, pitch = nj_pitch(S);
    {   // symmetric, zero diagonal, finite: in 64 x 64 tiles, so that the transposed reads stay in cache
        PhaseTimer tc("nj.check_matrix");
        for (uint64_t i0 = 0; i0 < S; i0 += 64)
            for (uint64_t j0 = i0; j0 < S; j0 += 64)
                for (uint64_t i = i0; i < std::min(i0 + 64, S); i++)
                    for (uint64_t j = std::max(j0, i); j < std::min(j0 + 64, S); j++) {
                        const double v = m[i * S + j];
                        if (i == j) { if (v != 0.0) { set_error("neighbour joining: the matrix has a non-zero diagonal (row %llu)", (unsigned long long)i); return SKX_EINVAL; } }
                        else if (!std::isfinite(v)) { set_error("neighbour joining: the matrix has no finite value at (%llu, %llu)", (unsigned long long)i, (unsigned long long)j); return SKX_EINVAL; }
                        else if (v != m[j * S + i]) { set_error("neighbour joining: the matrix is not symmetric at (%llu, %llu)", (unsigned long long)i, (unsigned long long)j); return SKX_EINVAL; }
                    }
    }
    SKX_HIP(hipSetDevice(ctx->device));
    SKX_TRY(nj_fits(ctx, S, 0));
    DevBuf<double> D;
    SKX_TRY(D.alloc(pitch * S));
    hipStream_t st = ctx->stream;
    SKX_HIP(hipMemsetAsync(D.p, 0, pitch * S * 8, st));
    {
        PhaseTimer tu("nj.upload");
        SKX_HIP(hipMemcpy2DAsync(D.p, pitch * 8, m, S * 8, S * 8, S, hipMemcpyHostToDevice, st));
        SKX_HIP(hipStreamSynchronize(st));
    }
    return nj_run(ctx, D, pitch, (uint32_t)S, joins);
    });
}
