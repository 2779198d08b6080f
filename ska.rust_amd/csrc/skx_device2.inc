// skx_device2.inc -- second half of skx_device.hip: MergeSkaArray kernels (statistics, filter, compaction,
// transpose, distance).  Included at the end of skx_device.hip.
namespace skx {

// ASCII middle base -> IUPAC set code (bit i == 2-bit base code i); 0 for '-', 0xFF for unsupported bytes
__device__ static inline uint32_t set_code(uint32_t b)
{
    switch (b) {
    case '-': return 0;
    case 'A': return 1;  case 'C': return 2;  case 'M': return 3;  case 'T': return 4;
    case 'W': return 5;  case 'Y': return 6;  case 'H': return 7;  case 'G': return 8;
    case 'R': return 9;  case 'S': return 10; case 'V': return 11; case 'K': return 12;
    case 'D': return 13; case 'B': return 14; case 'N': return 15;
    default: return 0xFF;
    }
}

// per-column statistics of a sample-major matrix; 4 columns per thread, coalesced rows
__global__ __launch_bounds__(256) void col_stats_kernel(const uint8_t *matrix, uint64_t pitch, int n_samples, uint64_t n_cols,
                                                        uint32_t *present, uint32_t *unambig, uint32_t *mask, int *bad_byte)
{
    const uint64_t c0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (c0 >= n_cols) return;
    uint32_t p[4] = {0, 0, 0, 0}, u[4] = {0, 0, 0, 0}, m[4] = {0, 0, 0, 0};
    int bad = 0;
    for (int s = 0; s < n_samples; s++) {
        const uint32_t x = *reinterpret_cast<const uint32_t *>(matrix + (uint64_t)s * pitch + c0);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t code = set_code((x >> (8 * i)) & 0xFFu);
            if (code == 0xFF) { if (c0 + i < n_cols) bad = 1; continue; }
            if (code) { p[i]++; u[i] += (code & (code - 1)) == 0; m[i] |= 1u << code; }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (c0 + i < n_cols) { present[c0 + i] = p[i]; unambig[c0 + i] = u[i]; mask[c0 + i] = m[i]; }
    if (bad) *bad_byte = 1;
}
void launch_col_stats(const uint8_t *matrix, uint64_t pitch, int n_samples, uint64_t n_cols, uint32_t *present, uint32_t *unambig,
                      uint32_t *mask, int *bad_byte, hipStream_t st)
{
    if (!n_cols) return;
    uint64_t threads = (n_cols + 3) / 4;
    hipLaunchKernelGGL(col_stats_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, matrix, pitch, n_samples, n_cols,
                       present, unambig, mask, bad_byte);
}

// MergeSkaArray::filter (merge_ska_array.rs:289-402) decided from the column statistics.
// keep: 1 kept, 0 removed (counts towards the return value), 2 dropped by update_counts(true) (:139-163, not counted)
// the filter_type cases of the rule for a row that passed the frequency test (m: the row's set of IUPAC codes, bit c = code c occurs):
// one function for filter_flags_kernel and subset_verdict_kernel
__device__ static inline uint8_t filter_type_keep(int filter_type, int ignore_const_gaps, uint32_t m, bool has_gap)
{
    const uint32_t acgt = (1u << 1) | (1u << 2) | (1u << 4) | (1u << 8);
    switch (filter_type) {
    case 0: return 1;
    case 1: return (__popc(m) + ((has_gap && !ignore_const_gaps) ? 1 : 0)) > 1;           // NoConst :322-334
    case 2: return (m & ~acgt) == 0;                                                        // NoAmbig :335-344
    default: return (__popc(m & acgt) + ((has_gap && !ignore_const_gaps) ? 1 : 0)) > 1;   // NoAmbigOrConst :345-367
    }
}
__global__ void filter_flags_kernel(FilterArgs a)
{
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.n_cols) return;
    const uint32_t present = a.present[c], unambig = a.unambig[c], m = a.mask[c];
    const uint32_t count = a.ambig_as_missing ? unambig : a.vcount[c];   // stored variant_count, or update_counts(true)
    uint8_t keep;
    if (a.two_stage) {          // generic_modes::distance: rows below min_count go first (NoFilter), then the constant ones (NoConst at 0)
        const bool has_gap = present < a.n_samples;
        if ((uint64_t)count < a.min_count) keep = 0;
        else keep = (__popc(m) + (has_gap ? 1 : 0)) > 1 ? 1 : 3;      // 3: constant (counted by the caller)
    }
    else if (a.ambig_as_missing && count == 0) keep = 2;
    else if ((uint64_t)count < a.min_count) keep = 0;
    else keep = filter_type_keep(a.filter_type, a.ignore_const_gaps, m, present < a.n_samples);
    a.keep[c] = keep;
}
void launch_filter_flags(const FilterArgs &a, hipStream_t st)
{
    if (!a.n_cols) return;
    hipLaunchKernelGGL(filter_flags_kernel, dim3((unsigned)((a.n_cols + 255) / 256)), dim3(256), 0, st, a);
}

// is_ambiguous (bit_encoding.rs:58-61) on the supported alphabet
__device__ static inline uint8_t mask_ambig_byte(uint8_t b)
{
    return (b == 'A' || b == 'C' || b == 'G' || b == 'T' || b == 'U' || b == '-') ? b : (uint8_t)'N';
}
// One workgroup = 4096 columns x 32 samples.  Threads read 16 columns at a time (16-B loads), drop the filtered ones and
// park the kept bytes of all 32 rows in LDS; the rows are then written with 16-B stores (the kept columns of a block are
// consecutive in the output because pos is a prefix sum), byte stores only at the unaligned ends.
// ORD (the subset alignments): output row s holds input row order[s]; the identity instantiation does not read `order`.
constexpr int CMP_ROWS = 4;
template <bool ORD = false>
__global__ __launch_bounds__(256) void compact_matrix_kernel(const uint8_t *in, uint64_t in_pitch, uint8_t *out, uint64_t out_pitch,
                                                             int n_samples, uint64_t n_cols, const uint8_t *keep, const uint64_t *pos, int mask_ambig,
                                                             const int *order)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_buf[];       // [CMP_ROWS][stride]
    __shared__ uint32_t s_tmp[17];
    const uint64_t c = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    uint32_t kf = 0;
    if (c + 16 <= n_cols) {
        const uint4 k4 = *reinterpret_cast<const uint4 *>(keep + c);        // keep[] is 256-B aligned, c % 16 == 0
        const uint32_t kw[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
        for (int i = 0; i < 16; i++) kf |= (uint32_t)(((kw[i >> 2] >> (8 * (i & 3))) & 0xFFu) == 1u) << i;
    } else if (c < n_cols)
        for (int i = 0; i < 16; i++) kf |= (uint32_t)(c + i < n_cols && keep[c + i] == 1) << i;
    uint32_t total;
    const uint32_t lofs = block_excl_scan(__popc(kf), s_tmp, &total);            // my first kept column, block-local
    if (total == 0) return;
    const uint64_t cblk = (uint64_t)blockIdx.x * blockDim.x * 16;
    const uint64_t p0 = pos[cblk < n_cols ? cblk : n_cols - 1];                   // output position of the block's first kept column
    const uint32_t shift = (uint32_t)(p0 & 15u);                                  // LDS image is aligned like the global destination
    const uint32_t stride = (4096 + 32 + 15) & ~15u;
    const int s0 = blockIdx.y * CMP_ROWS, s1 = s0 + CMP_ROWS < n_samples ? s0 + CMP_ROWS : n_samples;
    if (kf) {
        const uint8_t *src = in + (uint64_t)s0 * in_pitch + c;
#pragma unroll 2
        for (int s = s0; s < s1; s++, src += in_pitch) {
            const uint4 x4 = *reinterpret_cast<const uint4 *>(ORD ? in + (uint64_t)order[s] * in_pitch + c : src);
            const uint32_t xw[4] = {x4.x, x4.y, x4.z, x4.w};
            unsigned char *d = s_buf + (size_t)(s - s0) * stride + shift + lofs;
            uint32_t o = 0;
#pragma unroll
            for (int i = 0; i < 16; i++)
                if ((kf >> i) & 1u) { const uint8_t b = (uint8_t)(xw[i >> 2] >> (8 * (i & 3))); d[o++] = mask_ambig ? mask_ambig_byte(b) : b; }
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t head = (16u - shift) & 15u, h = head < total ? head : total, body = (total - h) / 16u, done = h + body * 16u;
    for (int s = s0 + wv; s < s1; s += 4) {
        const unsigned char *row = s_buf + (size_t)(s - s0) * stride + shift;
        uint8_t *dst = out + (uint64_t)s * out_pitch + p0;
        if ((uint32_t)lane < h) dst[lane] = row[lane];
        for (uint32_t v = lane; v < body; v += 64) *reinterpret_cast<uint4 *>(dst + h + 16u * v) = *reinterpret_cast<const uint4 *>(row + h + 16u * v);
        if (done + lane < total) dst[done + lane] = row[done + lane];
    }
}
void launch_compact_matrix(const uint8_t *in, uint64_t in_pitch, uint8_t *out, uint64_t out_pitch, int n_samples, uint64_t n_cols,
                           const uint8_t *keep, const uint64_t *pos, int mask_ambig, hipStream_t st, const int *order)
{
    if (!n_cols || !n_samples) return;
    const uint64_t groups = (n_cols + 15) / 16;
    const size_t lds = (size_t)CMP_ROWS * ((4096 + 32 + 15) & ~15u);
    const dim3 grid((unsigned)((groups + 255) / 256), (unsigned)((n_samples + CMP_ROWS - 1) / CMP_ROWS));
    if (order) {
        (void)hipFuncSetAttribute((const void *)compact_matrix_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(compact_matrix_kernel<true>, grid, dim3(256), lds, st, in, in_pitch, out, out_pitch, n_samples, n_cols, keep, pos, mask_ambig, order);
        return;
    }
    (void)hipFuncSetAttribute((const void *)compact_matrix_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(compact_matrix_kernel<false>, grid, dim3(256), lds, st, in, in_pitch, out, out_pitch, n_samples, n_cols, keep, pos, mask_ambig, order);
}

// ---- subset alignments (`ska align --groups / --samples`): delete_samples (merge_ska_array.rs:231-271, update_counts(false) :139-163) of
// everybody outside a sample list followed by the filter (:289-402), decided per column (= row of the reference) in one pass over the list's
// cells, without the sub-matrix and without per-column statistics in memory.  A thread takes 16 columns (one 16-byte load per sample), keeps
// present | unambig << 16 and the set of codes of each in registers, and writes keep[c] alone: 1 kept, 0 removed, 2 silent (update_counts(true))
// or absent (no sample of the list has the row: delete_samples drops it).  counts[0..2] += absent, silent, removed: wave sums by shuffles,
// the workgroup's through LDS, one atomic per workgroup and count.  The stored variant_count is not read: after the delete it is `present`.
__global__ __launch_bounds__(256) void subset_verdict_kernel(const uint8_t *matrix, uint64_t pitch, const int *order, int n, uint64_t n_cols, uint64_t min_count,
                                                             int ambig_as_missing, int filter_type, int ignore_const_gaps, uint8_t *keep,
                                                             unsigned long long *counts, int *bad_byte)
{
    __shared__ uint8_t s_lut[256];
    __shared__ uint32_t s_cnt[4][3];
    s_lut[threadIdx.x] = (uint8_t)set_code(threadIdx.x);
    __syncthreads();
    const uint64_t c0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    uint32_t n_absent = 0, n_silent = 0, n_removed = 0;
    if (c0 < n_cols) {
        uint32_t pu[16], m[16];
#pragma unroll
        for (int i = 0; i < 16; i++) { pu[i] = 0; m[i] = 0; }
        uint32_t bad = 0;                                                     // bit i: column c0 + i holds a byte outside the alphabet
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        const uint8_t *col = matrix + c0;                                     // rows are padded to the pitch (>= 256 bytes past n_cols): the load stays inside the row
        u32x4 nx = *reinterpret_cast<const u32x4 *>(col + (uint64_t)order[0] * pitch);
        for (int s = 0; s < n; s++) {
            const u32x4 cur = nx;
            if (s + 1 < n) nx = *reinterpret_cast<const u32x4 *>(col + (uint64_t)order[s + 1] * pitch);
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const uint32_t code = s_lut[(cur[i >> 2] >> (8 * (i & 3))) & 0xFFu];
                if (code == 0xFF) { bad |= 1u << i; continue; }
                if (code) { pu[i] += 1u + (((code & (code - 1)) == 0) ? 0x10000u : 0u); m[i] |= 1u << code; }
            }
        }
        uint32_t kw[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t present = pu[i] & 0xFFFFu, unambig = pu[i] >> 16, count = ambig_as_missing ? unambig : present;
            uint32_t k;
            if (present == 0) k = 2;
            else if (ambig_as_missing && count == 0) k = 2;
            else if ((uint64_t)count < min_count) k = 0;
            else k = filter_type_keep(filter_type, ignore_const_gaps, m[i], present < (uint32_t)n);
            if (c0 + i < n_cols) {
                n_absent += present == 0; n_silent += present != 0 && k == 2; n_removed += k == 0;
                kw[i >> 2] |= k << (8 * (i & 3));
            }
        }
        if (c0 + 16 <= n_cols) {
            *reinterpret_cast<u32x4 *>(keep + c0) = u32x4{kw[0], kw[1], kw[2], kw[3]};      // keep[] is 256-byte aligned, c0 % 16 == 0
            if (bad) *bad_byte = 1;
        } else {
            for (int i = 0; i < 16 && c0 + i < n_cols; i++) { keep[c0 + i] = (uint8_t)(kw[i >> 2] >> (8 * (i & 3))); if ((bad >> i) & 1u) *bad_byte = 1; }
        }
    }
    for (int d = 32; d; d >>= 1) { n_absent += __shfl_down(n_absent, d, 64); n_silent += __shfl_down(n_silent, d, 64); n_removed += __shfl_down(n_removed, d, 64); }
    if ((threadIdx.x & 63) == 0) { s_cnt[threadIdx.x >> 6][0] = n_absent; s_cnt[threadIdx.x >> 6][1] = n_silent; s_cnt[threadIdx.x >> 6][2] = n_removed; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const uint32_t t = s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
        if (t) atomicAdd(&counts[threadIdx.x], (unsigned long long)t);
    }
}
void launch_subset_verdicts(const uint8_t *matrix, uint64_t pitch, const int *order, int n, uint64_t n_cols, uint64_t min_count, int ambig_as_missing,
                            int filter_type, int ignore_const_gaps, uint8_t *keep, unsigned long long *counts, int *bad_byte, hipStream_t st)
{
    if (!n_cols || n <= 0) return;
    hipLaunchKernelGGL(subset_verdict_kernel, dim3((unsigned)((n_cols + 4095) / 4096)), dim3(256), 0, st, matrix, pitch, order, n, n_cols, min_count,
                       ambig_as_missing, filter_type, ignore_const_gaps, keep, counts, bad_byte);
}
template <typename T>
__global__ void compact_vec_kernel(const T *in, T *out, uint64_t n, const uint8_t *keep, const uint64_t *pos)
{
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (uint64_t)gridDim.x * blockDim.x)
        if (keep[c] == 1) out[pos[c]] = in[c];
}
void launch_compact_u32(const uint32_t *in, uint32_t *out, uint64_t n, const uint8_t *keep, const uint64_t *pos, hipStream_t st)
{
    if (!n) return;
    uint64_t g = (n + 255) / 256; if (g > 8192) g = 8192;
    hipLaunchKernelGGL(compact_vec_kernel<uint32_t>, dim3((unsigned)g), dim3(256), 0, st, in, out, n, keep, pos);
}
struct CompactStats { const uint32_t *in[4]; uint32_t *out[4]; };
__global__ void compact_stats_kernel(CompactStats a, uint64_t n, const uint8_t *keep, const uint64_t *pos)
{
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (uint64_t)gridDim.x * blockDim.x)
        if (keep[c] == 1) {
            const uint64_t o = pos[c];
#pragma unroll
            for (int i = 0; i < 4; i++) a.out[i][o] = a.in[i][c];
        }
}
void launch_compact_stats(const uint32_t *const in[4], uint32_t *const out[4], uint64_t n, const uint8_t *keep, const uint64_t *pos, hipStream_t st)
{
    if (!n) return;
    CompactStats a;
    for (int i = 0; i < 4; i++) { a.in[i] = in[i]; a.out[i] = out[i]; }
    uint64_t g = (n + 255) / 256; if (g > 8192) g = 8192;
    hipLaunchKernelGGL(compact_stats_kernel, dim3((unsigned)g), dim3(256), 0, st, a, n, keep, pos);
}
void launch_compact_u64(const uint64_t *in, uint64_t *out, uint64_t n, const uint8_t *keep, const uint64_t *pos, hipStream_t st)
{
    if (!n) return;
    uint64_t g = (n + 255) / 256; if (g > 8192) g = 8192;
    hipLaunchKernelGGL(compact_vec_kernel<uint64_t>, dim3((unsigned)g), dim3(256), 0, st, in, out, n, keep, pos);
}
struct alignas(16) pair64 { uint64_t a, b; };
void launch_compact_u128(const uint64_t *in, uint64_t *out, uint64_t n, const uint8_t *keep, const uint64_t *pos, hipStream_t st)
{
    if (!n) return;
    uint64_t g = (n + 255) / 256; if (g > 8192) g = 8192;
    hipLaunchKernelGGL(compact_vec_kernel<pair64>, dim3((unsigned)g), dim3(256), 0, st, (const pair64 *)in, (pair64 *)out, n, keep, pos);
}
// after ambig_mask: every ambiguous code in a column has become 'N'
__global__ void mask_ambig_stats_kernel(uint32_t *mask, uint64_t n)
{
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const uint32_t acgt = (1u << 1) | (1u << 2) | (1u << 4) | (1u << 8);
    uint32_t m = mask[c];
    if (m & ~acgt) m = (m & acgt) | (1u << 15);
    mask[c] = m;
}
void launch_mask_ambig_stats(uint32_t *mask, uint64_t n, hipStream_t st)
{
    if (!n) return;
    hipLaunchKernelGGL(mask_ambig_stats_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, mask, n);
}

// ---- streaming load (row-major row blocks straight from the .skf decoder): per-row statistics and kept rows -> sample-major ----
// One wave per row of `S` cells (bytes); rows start at arbitrary byte offsets, so lanes read aligned dwords covering the row and
// mask the bytes outside it.  bad_byte is set for a cell outside the alphabet.
__global__ __launch_bounds__(256) void row_stats_rm_kernel(const uint8_t *cells, uint64_t S, uint64_t nr, uint32_t *present, uint32_t *unambig,
                                                           uint32_t *mask, int *bad_byte)
{
    __shared__ uint8_t s_lut[256];
    s_lut[threadIdx.x] = (uint8_t)set_code(threadIdx.x);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * 4;
    for (uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < nr; r += waves) {
        const int64_t b = (int64_t)(r * S), e = b + (int64_t)S;                // byte range of the row (relative to cells)
        const int64_t skew = (int64_t)(((uintptr_t)cells + (uintptr_t)b) & 3u);
        uint32_t p = 0, u = 0, m = 0; bool bad = false;
        for (int64_t a = b - skew + 4 * lane; a < e; a += 256) {                // aligned dwords; a may start up to 3 bytes below b
            const uint32_t x = *reinterpret_cast<const uint32_t *>(cells + a);   // the buffers carry >= 8 bytes of slack on both sides
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int64_t q = a + i;
                if (q < b || q >= e) continue;
                const uint32_t code = s_lut[(x >> (8 * i)) & 0xFFu];
                if (code == 0xFF) { bad = true; continue; }
                if (code) { p++; u += (code & (code - 1)) == 0; m |= 1u << code; }
            }
        }
        for (int d = 32; d; d >>= 1) { p += __shfl_down(p, d, 64); u += __shfl_down(u, d, 64); m |= __shfl_down(m, d, 64); }
        if (lane == 0) { present[r] = p; unambig[r] = u; mask[r] = m; }
        if (bad) *bad_byte = 1;
    }
}
void launch_row_stats_rm(const uint8_t *cells, uint64_t S, uint64_t nr, uint32_t *present, uint32_t *unambig, uint32_t *mask, int *bad_byte, hipStream_t st)
{
    if (!nr || !S) return;
    const uint64_t g = (nr + 3) / 4 < 65536 ? (nr + 3) / 4 : 65536;
    hipLaunchKernelGGL(row_stats_rm_kernel, dim3((unsigned)g), dim3(256), 0, st, cells, S, nr, present, unambig, mask, bad_byte);
}
// kept rows of a row-major block -> columns [col0 + pos[r]] of the sample-major matrix.  One workgroup = RM_ROWS rows x 64 samples:
// the block's kept rows are listed in LDS, their bytes parked sample-major, and every sample's run written with adjacent lanes.
constexpr int RM_ROWS = 512;
__global__ __launch_bounds__(256) void compact_rm_kernel(const uint8_t *cells, uint64_t S, uint64_t nr, const uint8_t *keep, const uint64_t *pos,
                                                         uint8_t *out, uint64_t pitch, uint64_t col0, int mask_ambig)
{
    __shared__ uint16_t s_rows[RM_ROWS];
    __shared__ uint32_t s_n;
    __shared__ uint8_t s_tile[64][RM_ROWS + 4];
    const uint64_t r0 = (uint64_t)blockIdx.x * RM_ROWS, c0 = (uint64_t)blockIdx.y * 64;
    const uint32_t rows_here = (uint32_t)(nr - r0 < (uint64_t)RM_ROWS ? nr - r0 : (uint64_t)RM_ROWS);
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    // kept rows in order: pos is an exclusive scan of (keep == 1), so a kept row's slot is pos[r] - pos[r0]
    const uint64_t p0 = pos[r0];
    for (uint32_t i = threadIdx.x; i < rows_here; i += 256)
        if (keep[r0 + i] == 1) { s_rows[(uint32_t)(pos[r0 + i] - p0)] = (uint16_t)i; atomicAdd(&s_n, 1u); }
    __syncthreads();
    const uint32_t kn = s_n;
    if (!kn) return;
    const uint32_t cols_here = (uint32_t)(S - c0 < 64 ? S - c0 : 64);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (uint32_t j = wv; j < kn; j += 4) {                                    // a wave reads 64 consecutive cells of one kept row
        const uint64_t r = r0 + s_rows[j];
        if ((uint32_t)lane < cols_here) { const uint8_t b = cells[r * S + c0 + lane]; s_tile[lane][j] = mask_ambig ? mask_ambig_byte(b) : b; }
    }
    __syncthreads();
    for (uint32_t c = wv; c < cols_here; c += 4) {                              // a wave writes one sample's run
        uint8_t *dst = out + (c0 + c) * pitch + col0 + p0;
        for (uint32_t j = lane; j < kn; j += 64) dst[j] = s_tile[c][j];
    }
}
void launch_compact_rm(const uint8_t *cells, uint64_t S, uint64_t nr, const uint8_t *keep, const uint64_t *pos, uint8_t *out, uint64_t pitch,
                       uint64_t col0, int mask_ambig, hipStream_t st)
{
    if (!nr || !S) return;
    hipLaunchKernelGGL(compact_rm_kernel, dim3((unsigned)((nr + RM_ROWS - 1) / RM_ROWS), (unsigned)((S + 63) / 64)), dim3(256), 0, st, cells, S, nr, keep, pos,
                       out, pitch, col0, mask_ambig);
}

// 64x64 byte tiles through LDS (row pad 4 -> conflict-free b32 column reads)
__global__ __launch_bounds__(256) void transpose_kernel(const uint8_t *in, uint64_t in_pitch, uint64_t rows, uint64_t cols, uint8_t *out,
                                                        uint64_t out_pitch)
{
    __shared__ uint8_t tile[64][68];
    const uint64_t r0 = (uint64_t)blockIdx.y * 64, c0 = (uint64_t)blockIdx.x * 64;
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int r = i >> 6, c = i & 63;
        tile[r][c] = (r0 + r < rows && c0 + c < cols) ? in[(r0 + r) * in_pitch + c0 + c] : 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int c = i >> 6, r = i & 63;
        if (r0 + r < rows && c0 + c < cols) out[(c0 + c) * out_pitch + r0 + r] = tile[r][c];
    }
}
void launch_transpose(const uint8_t *in, uint64_t in_pitch, uint64_t rows, uint64_t cols, uint8_t *out, uint64_t out_pitch, hipStream_t st)
{
    if (!rows || !cols) return;
    hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((cols + 63) / 64), (unsigned)((rows + 63) / 64)), dim3(256), 0, st, in, in_pitch,
                       rows, cols, out, out_pitch);
}

__global__ __launch_bounds__(256) void row_nonmissing_kernel(const uint8_t *matrix, uint64_t pitch, uint64_t n_cols, unsigned long long *out)
{
    const uint64_t s = blockIdx.y;
    const uint8_t *row = matrix + s * pitch;
    unsigned long long cnt = 0;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_cols; c += (uint64_t)gridDim.x * blockDim.x) cnt += row[c] != '-';
    for (int d = 32; d; d >>= 1) cnt += __shfl_down(cnt, d, 64);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&out[s], cnt);
}
void launch_row_nonmissing(const uint8_t *matrix, uint64_t pitch, int n_samples, uint64_t n_cols, unsigned long long *out, hipStream_t st)
{
    if (!n_cols || !n_samples) return;
    uint64_t gx = (n_cols + 255) / 256; if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(row_nonmissing_kernel, dim3((unsigned)gx, (unsigned)n_samples), dim3(256), 0, st, matrix, pitch, n_cols, out);
}

__global__ void count_u8_kernel(const uint8_t *v, uint64_t n, uint8_t value, unsigned long long *out)
{
    unsigned long long cnt = 0;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (uint64_t)gridDim.x * blockDim.x) cnt += v[c] == value;
    for (int d = 32; d; d >>= 1) cnt += __shfl_down(cnt, d, 64);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(out, cnt);
}
void launch_count_u8(const uint8_t *v, uint64_t n, uint8_t value, unsigned long long *out, hipStream_t st)
{
    if (!n) return;
    uint64_t g = (n + 255) / 256; if (g > 2048) g = 2048;
    hipLaunchKernelGGL(count_u8_kernel, dim3((unsigned)g), dim3(256), 0, st, v, n, value, out);
}

__global__ void differ_u32_kernel(const uint32_t *a, const uint32_t *b, uint64_t n, int *flag)
{
    bool d = false;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (uint64_t)gridDim.x * blockDim.x) d |= a[c] != b[c];
    if (d) *flag = 1;
}
void launch_differ_u32(const uint32_t *a, const uint32_t *b, uint64_t n, int *flag, hipStream_t st)
{
    if (!n) return;
    uint64_t g = (n + 255) / 256; if (g > 2048) g = 2048;
    hipLaunchKernelGGL(differ_u32_kernel, dim3((unsigned)g), dim3(256), 0, st, a, b, n, flag);
}

// ------------------------------------------------------------------------------------------------
// distance (merge_ska_array.rs:587-632) as popcounts over bit planes.
// planes, 64 columns per word: 0 P (cell != '-'), 1..4 membership of A,C,T,G in the cell's base set,
// 5..7 set size == 1,2,3.   Pair counts (integers, combined on the host in a fixed order):
//   [0] exactly one '-'          [1] both present
//   filt_ambig:   [2] both unambiguous   [3] both unambiguous and equal
//   allow-ambig:  [2..11] cells with |S1 n S2| = t > 0, by (|S1||S2|, t) class, see PAIR_CLASS_NUM in skx_api
// ------------------------------------------------------------------------------------------------
// FILT (the default, filter-ambiguous distance) needs only: 0 P, 1 U (unambiguous: one base), 2..3 the 2-bit base code of
// unambiguous cells -> 4 planes.  A lane takes 16 consecutive rows of one sample (one 16-byte load), looks every cell up in a table of
// plane bits spread one per byte (plane p's bit at bit 8 p) and shifts the entry by the row's place into an accumulator: byte p of the
// accumulator is the lane's byte of plane p; two accumulators give the 16 bits it stores per plane -- the lanes' pieces are adjacent,
// a wave writes 128 contiguous bytes per plane.  No LDS traffic but the table, no ballots (a ballot per plane and 64 rows per wave
// instruction cost ~10 x the instructions: build_planes_out_kernel below has the numbers).  A workgroup serves PLS samples.
// ORD (the query sweep): slot s of the planes holds sample order[s] -- the queries in front, so that the band form of the pair sweep covers them.
// The identity instantiations are the code every other caller launches: `order` is not read there.
constexpr int PLS = 8;
template <bool FILT, bool ORD = false>
__global__ __launch_bounds__(256) void build_planes_kernel(const uint8_t *matrix, uint64_t pitch, int n_samples, uint64_t n_cols, uint64_t *planes,
                                                           uint64_t wpr, uint64_t plane_stride, const int *order)
{
    constexpr int NP = FILT ? 4 : 8, NA = NP / 4;
    __shared__ uint32_t s_lut[NA][256];
    {
        const uint32_t c0 = set_code(threadIdx.x), c = c0 == 0xFF ? 15u : c0, sz = __popc(c);
        if (FILT) s_lut[0][threadIdx.x] = (c != 0 ? 1u : 0u) | (sz == 1 ? 1u << 8 : 0u) | ((sz == 1 && (c & 10u)) ? 1u << 16 : 0u) | ((sz == 1 && (c & 12u)) ? 1u << 24 : 0u);
        else {
            s_lut[0][threadIdx.x] = (c != 0 ? 1u : 0u) | ((c & 1u) ? 1u << 8 : 0u) | ((c & 2u) ? 1u << 16 : 0u) | ((c & 4u) ? 1u << 24 : 0u);
            s_lut[NA - 1][threadIdx.x] = ((c & 8u) ? 1u : 0u) | (sz == 1 ? 1u << 8 : 0u) | (sz == 2 ? 1u << 16 : 0u) | (sz == 3 ? 1u << 24 : 0u);
        }
    }
    __syncthreads();
    const uint64_t c = (uint64_t)blockIdx.x * 4096 + 16ull * threadIdx.x;      // first of this lane's 16 rows
    if (c >= wpr * 64) return;                                                  // (past the last plane word)
    // rows at or past n_cols read as '-' (the last word's padding): byte masks of the rows that exist
    uint32_t km[4];
#pragma unroll
    for (int d = 0; d < 4; d++) { km[d] = 0; for (int i = 0; i < 4; i++) if (c + 4 * d + i < n_cols) km[d] |= 0xFFu << (8 * i); }
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const int s_lo = (int)blockIdx.y * PLS, s_hi = s_lo + PLS < n_samples ? s_lo + PLS : n_samples;
    auto fetch = [&](int s) {                                          // rows are padded to the pitch (>= 256 bytes past n_cols): the load stays inside the row's allocation
        u32x4 v = {0x2D2D2D2Du, 0x2D2D2D2Du, 0x2D2D2D2Du, 0x2D2D2D2Du};
        if (c < n_cols) v = *reinterpret_cast<const u32x4 *>(matrix + (uint64_t)(ORD ? order[s] : s) * pitch + c);
        return v;
    };
    u32x4 nx = fetch(s_lo);
    for (int s = s_lo; s < s_hi; s++) {
        const u32x4 cur = nx;
        if (s + 1 < s_hi) nx = fetch(s + 1);
        uint32_t acc[2][NA];
#pragma unroll
        for (int q = 0; q < NA; q++) { acc[0][q] = 0; acc[1][q] = 0; }
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const uint32_t x = (cur[d] & km[d]) | (0x2D2D2D2Du & ~km[d]);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t cell = (x >> (8 * i)) & 0xFFu;
#pragma unroll
                for (int q = 0; q < NA; q++) acc[d >> 1][q] |= s_lut[q][cell] << (4 * (d & 1) + i);
            }
        }
        uint16_t *dst = reinterpret_cast<uint16_t *>(planes + (uint64_t)s * wpr) + (c >> 4);
#pragma unroll
        for (int p = 0; p < NP; p++)
            dst[(uint64_t)p * plane_stride * 4] = (uint16_t)(((acc[0][p / 4] >> (8 * (p & 3))) & 0xFFu) | (((acc[1][p / 4] >> (8 * (p & 3))) & 0xFFu) << 8));
    }
}
void launch_build_planes(const uint8_t *matrix, uint64_t pitch, int n_samples, uint64_t n_cols, uint64_t *planes, uint64_t wpr, int filt,
                         hipStream_t st, const int *order)
{
    if (!wpr || !n_samples) return;
    const dim3 grid((unsigned)((wpr + 63) / 64), (unsigned)((n_samples + PLS - 1) / PLS));
    const uint64_t stride = (uint64_t)n_samples * wpr;
    if (order) {
        if (filt) hipLaunchKernelGGL((build_planes_kernel<true, true>), grid, dim3(256), 0, st, matrix, pitch, n_samples, n_cols, planes, wpr, stride, order);
        else hipLaunchKernelGGL((build_planes_kernel<false, true>), grid, dim3(256), 0, st, matrix, pitch, n_samples, n_cols, planes, wpr, stride, order);
    }
    else if (filt) hipLaunchKernelGGL(build_planes_kernel<true>, grid, dim3(256), 0, st, matrix, pitch, n_samples, n_cols, planes, wpr, stride, order);
    else hipLaunchKernelGGL(build_planes_kernel<false>, grid, dim3(256), 0, st, matrix, pitch, n_samples, n_cols, planes, wpr, stride, order);
}

// ---- planes of the kept rows only (`ska distance` on an array in memory: the filters of generic_modes::distance decide per row,
// and the planes are built over the rows that stay -- the byte matrix is neither compacted nor copied).
// keep_bits[g] = bit i set iff row 64 g + i stays; gpos[g] = rows that stay below 64 g.
__global__ __launch_bounds__(256) void keep_bits_kernel(const uint8_t *keep, const uint64_t *pos, uint64_t n, uint64_t *keep_bits, uint64_t *gpos)
{
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long b = __ballot(c < n && keep[c] == 1);
    if ((threadIdx.x & 63) == 0 && (c >> 6) <= (n - 1) / 64) { keep_bits[c >> 6] = b; gpos[c >> 6] = pos[c < n ? c : n]; }
}
constexpr int PS = 8;           // samples per workgroup of build_planes_out_kernel
// first_group[b] = the group of 64 rows that holds the kept row of rank 4096 b (the first row of output block b)
__global__ __launch_bounds__(256) void first_groups_kernel(const uint64_t *keep_bits, const uint64_t *gpos, uint64_t n_groups, uint32_t *first_group)
{
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_groups) return;
    const uint64_t a = gpos[g], e = a + (uint64_t)__popcll(keep_bits[g]);
    const uint64_t b = (a + 4095) / 4096;
    if (b * 4096 < e) first_group[b] = (uint32_t)g;                     // (a group holds at most 64 kept rows: at most one block starts in it)
}
// Bit planes of the rows that stay (keep_bits / gpos of keep_bits_kernel), for `ska distance`.  A lane takes eight rows: what depends on
// the rows only -- which of the eight stay, the rank of each kept row among them, where the lane's bits go -- is worked out once per
// stretch of 4 096 rows and serves PS samples.  Per sample the lane loads its 8 cells, blanks the rows that go ('-': no bit in any plane),
// looks every cell up in a table of plane bits spread one per byte (plane p's bit at bit 8 p) and shifts the entry by the row's rank into an
// accumulator: byte p of the accumulator is the lane's piece of plane p, OR-ed at its offset into the workgroup's output words in LDS.
// The work is cut by OUTPUT words: workgroup (b, y) owns words [64 b, 64 b + 64) of every plane of PS samples -- the kept rows of rank
// [4096 b, 4096 b + 4096) -- and walks the input groups from first_group[b] on, so its words leave with plain stores and the planes need
// not be zeroed; a lane's bits outside the block are dropped (below it) or land in spare words that are not stored (above it).
// 1 000 samples x 22.6 M rows, 22.54 M kept (the 72 339 constant rows go; 11.3 GB of planes): 35 ms (one row per lane, a ballot per plane, one sample per workgroup: ~640 wave instructions
// per 512 cells) -> 22 ms (this form cut by input rows, first / last word of a workgroup OR-ed into the planes atomically: 44 M global
// atomics) -> 9.3 ms (profiles/r03zzm_build_planes.log).
// ORD: as in build_planes_kernel -- slot s_lo + s holds sample order[s_lo + s]; the identity instantiations do not read `order`.
template <bool FILT, bool ORD = false>
__global__ __launch_bounds__(256) void build_planes_out_kernel(const uint8_t *matrix, uint64_t pitch, int n_samples, uint64_t n_cols, const uint64_t *keep_bits,
                                                               const uint64_t *gpos, const uint32_t *first_group, uint64_t kept,
                                                               uint64_t *planes, uint64_t wpr, uint64_t plane_stride, const int *order)
{
    constexpr int NP = FILT ? 4 : 8, NA = NP / 4;
    __shared__ uint32_t s_lut[NA][256];
    __shared__ unsigned long long s_out[PS][NP][66];
    __shared__ unsigned long long s_kb[64];
    __shared__ uint64_t s_gp[65];
    {
        const uint32_t c0 = set_code(threadIdx.x), c = c0 == 0xFF ? 15u : c0, sz = __popc(c);
        if (FILT) s_lut[0][threadIdx.x] = (c != 0 ? 1u : 0u) | (sz == 1 ? 1u << 8 : 0u) | ((sz == 1 && (c & 10u)) ? 1u << 16 : 0u) | ((sz == 1 && (c & 12u)) ? 1u << 24 : 0u);
        else {
            s_lut[0][threadIdx.x] = (c != 0 ? 1u : 0u) | ((c & 1u) ? 1u << 8 : 0u) | ((c & 2u) ? 1u << 16 : 0u) | ((c & 4u) ? 1u << 24 : 0u);
            s_lut[NA - 1][threadIdx.x] = ((c & 8u) ? 1u : 0u) | (sz == 1 ? 1u << 8 : 0u) | (sz == 2 ? 1u << 16 : 0u) | (sz == 3 ? 1u << 24 : 0u);
        }
    }
    for (uint32_t i = threadIdx.x; i < (uint32_t)PS * NP * 66; i += 256) (&s_out[0][0][0])[i] = 0ull;
    const uint64_t rank0 = (uint64_t)blockIdx.x * 4096, rank1 = rank0 + 4096 < kept ? rank0 + 4096 : kept;
    const uint64_t n_groups = (n_cols + 63) / 64;
    const int s_lo = (int)blockIdx.y * PS, ns = s_lo + PS < n_samples ? PS : n_samples - s_lo;
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    uint32_t *s_out32 = reinterpret_cast<uint32_t *>(&s_out[0][0][0]);
    for (uint64_t g0 = first_group[blockIdx.x]; g0 < n_groups; g0 += 64) {
        __syncthreads();                                                  // (the table / the zeroes the first time; s_kb, s_gp read by everybody after that)
        if (threadIdx.x < 64) s_kb[threadIdx.x] = g0 + threadIdx.x < n_groups ? keep_bits[g0 + threadIdx.x] : 0ull;
        else if (threadIdx.x < 129) {
            const uint64_t g = g0 + (threadIdx.x - 64);
            s_gp[threadIdx.x - 64] = g < n_groups ? gpos[g] : kept;
        }
        __syncthreads();
        const uint64_t c0 = g0 * 64;
        uint32_t kml[2], kmh[2], cpack[2], ob[2], drop[2];
        bool live[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t t = threadIdx.x + 256u * h, gl = t >> 3, j = t & 7u;
            const unsigned long long km = s_kb[gl];
            const uint32_t m8 = (uint32_t)(km >> (8u * j)) & 0xFFu;
            const uint64_t r = s_gp[gl] + (uint64_t)__popcll(km & ((1ull << (8u * j)) - 1ull));      // rank of the chunk's first kept row
            const uint32_t k8 = __popc(m8);
            live[h] = m8 != 0 && r + k8 > rank0 && r < rank1;
            drop[h] = r < rank0 ? (uint32_t)(rank0 - r) : 0u;               // its lowest bits belong to the block before
            ob[h] = r < rank0 ? 0u : (uint32_t)(r - rank0);
            uint32_t lo = 0, hi = 0, cp = 0;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                if ((m8 >> i) & 1u) { if (i < 4) lo |= 0xFFu << (8 * i); else hi |= 0xFFu << (8 * (i - 4)); }
                cp |= (uint32_t)__popc(m8 & ((1u << i) - 1u)) << (4 * i);
            }
            kml[h] = lo; kmh[h] = hi; cpack[h] = cp;
        }
        u32x2 nx[2];
        auto fetch = [&](int s) {
#pragma unroll
            for (int h = 0; h < 2; h++) { nx[h] = u32x2{0x2D2D2D2Du, 0x2D2D2D2Du}; if (live[h]) nx[h] = *reinterpret_cast<const u32x2 *>(matrix + (uint64_t)(ORD ? order[s_lo + s] : s_lo + s) * pitch + c0 + 8ull * (threadIdx.x + 256u * h)); }
        };
        fetch(0);
        for (int s = 0; s < ns; s++) {
            u32x2 cur[2] = {nx[0], nx[1]};
            if (s + 1 < ns) fetch(s + 1);
#pragma unroll
            for (int h = 0; h < 2; h++) {
                if (!live[h]) continue;
                const uint32_t xl = (cur[h].x & kml[h]) | (0x2D2D2D2Du & ~kml[h]), xh = (cur[h].y & kmh[h]) | (0x2D2D2D2Du & ~kmh[h]);      // rows that go read as '-'
                uint32_t acc[NA];
#pragma unroll
                for (int q = 0; q < NA; q++) acc[q] = 0;
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const uint32_t cell = ((i < 4 ? xl : xh) >> (8 * (i & 3))) & 0xFFu, r = (cpack[h] >> (4 * i)) & 15u;
#pragma unroll
                    for (int q = 0; q < NA; q++) acc[q] |= s_lut[q][cell] << r;
                }
                const uint32_t wi = ob[h] >> 5, sh = ob[h] & 31u;
#pragma unroll
                for (int p = 0; p < NP; p++) {
                    const uint32_t bits = ((acc[p / 4] >> (8 * (p & 3))) & 0xFFu) >> drop[h];
                    if (bits) {
                        uint32_t *o = s_out32 + ((uint32_t)s * NP + p) * 132u + wi;
                        atomicOr(o, bits << sh);
                        if (sh > 24u && (bits >> (32u - sh))) atomicOr(o + 1, bits >> (32u - sh));
                    }
                }
            }
        }
        if (s_gp[64] >= rank1) break;                                     // (uniform) the next stretch starts at or past the block's end
    }
    __syncthreads();
    const uint32_t nw = (uint32_t)((rank1 - rank0 + 63) >> 6);
    for (uint32_t i = threadIdx.x; i < (uint32_t)ns * NP * nw; i += 256) {
        const uint32_t w = i % nw, sp = i / nw, p = sp % NP, s = sp / NP;
        reinterpret_cast<unsigned long long *>(planes)[p * plane_stride + (uint64_t)(s_lo + s) * wpr + (uint64_t)blockIdx.x * 64 + w] = s_out[s][p][w];
    }
}
// rows that stay, by whether a cell of theirs is ambiguous (col_mask: bit c set iff set code c occurs in the row; codes 0 '-', 1 A, 2 C, 4 T, 8 G
// are the unambiguous ones): clean[r] / dirty[r] = 1.  keep == nullptr: every row stays.
// mode 1: every kept row counts as dirty, 2: as clean (the fallback of the caller, and the test of that fallback)
__global__ __launch_bounds__(256) void split_keep_kernel(const uint8_t *keep, const uint32_t *col_mask, uint64_t n, uint8_t *clean, uint8_t *dirty, int mode)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const bool k = !keep || keep[r] == 1, d = mode == 1 || (mode == 0 && (col_mask[r] & 0xFFFFu & ~0x117u) != 0);
    clean[r] = k && !d; dirty[r] = k && d;
}
void launch_split_keep(const uint8_t *keep, const uint32_t *col_mask, uint64_t n, uint8_t *clean, uint8_t *dirty, hipStream_t st, int mode)
{
    if (!n) return;
    hipLaunchKernelGGL(split_keep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, keep, col_mask, n, clean, dirty, mode);
}
// after the ranks' dirty bytes were summed: dirty[r] != 0 -> 1, clean[r] = the rest (every row is a kept row here)
__global__ __launch_bounds__(256) void split_from_dirty_kernel(uint8_t *dirty, uint64_t n, uint8_t *clean)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const bool d = dirty[r] != 0;
    dirty[r] = d; clean[r] = !d;
}
void launch_split_keep_from_dirty(uint8_t *dirty, uint64_t n, uint8_t *clean, hipStream_t st)
{
    if (!n) return;
    hipLaunchKernelGGL(split_from_dirty_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dirty, n, clean);
}
void launch_keep_bits(const uint8_t *keep, const uint64_t *pos, uint64_t n, uint64_t *keep_bits, uint64_t *gpos, hipStream_t st)
{
    if (!n) return;
    hipLaunchKernelGGL(keep_bits_kernel, dim3((unsigned)(((n + 63) / 64 * 64 + 255) / 256)), dim3(256), 0, st, keep, pos, n, keep_bits, gpos);
}
// planes must be zeroed; wpr = words per sample of the KEPT rows
void launch_build_planes_keep(const uint8_t *matrix, uint64_t pitch, int n_samples, uint64_t n_cols, const uint64_t *keep_bits, const uint64_t *gpos,
                              uint64_t *planes, uint64_t wpr, int filt, hipStream_t st, uint32_t *first_group, uint64_t kept, const int *order)
{
    if (!n_cols || !n_samples || !wpr || !kept) return;
    const uint64_t n_groups = (n_cols + 63) / 64;
    hipLaunchKernelGGL(first_groups_kernel, dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, st, keep_bits, gpos, n_groups, first_group);
    const dim3 grid((unsigned)((kept + 4095) / 4096), (unsigned)((n_samples + PS - 1) / PS));
    const uint64_t stride = (uint64_t)n_samples * wpr;
    if (order) {
        if (filt) hipLaunchKernelGGL((build_planes_out_kernel<true, true>), grid, dim3(256), 0, st, matrix, pitch, n_samples, n_cols, keep_bits, gpos, first_group, kept, planes, wpr, stride, order);
        else hipLaunchKernelGGL((build_planes_out_kernel<false, true>), grid, dim3(256), 0, st, matrix, pitch, n_samples, n_cols, keep_bits, gpos, first_group, kept, planes, wpr, stride, order);
    }
    else if (filt) hipLaunchKernelGGL(build_planes_out_kernel<true>, grid, dim3(256), 0, st, matrix, pitch, n_samples, n_cols, keep_bits, gpos, first_group, kept, planes, wpr, stride, order);
    else hipLaunchKernelGGL(build_planes_out_kernel<false>, grid, dim3(256), 0, st, matrix, pitch, n_samples, n_cols, keep_bits, gpos, first_group, kept, planes, wpr, stride, order);
}

// filter-ambiguous pair counts from the 4-plane layout: a 64 x 64 tile of sample pairs per workgroup, 4 x 2 pairs per thread
// (512 threads; every LDS word read feeds two or four pairs: 3 reads per pair and 64 rows instead of 8 with one pair per thread
// -- 14 VALU instructions per pair and 64 rows since round 3, the equality mask being two three-input operations), the next FW words of the 2 x 64 plane
// rows are on their way from HBM / the memory-side cache while the current ones are counted (two LDS buffers, one barrier
// per step).  1 000 samples x 22.5 M rows: 296 ms (32 x 32 tiles, 2 x 2 pairs) -> 175 (4 x 4, 256 threads) -> 160 -> 145 -> 134.6 ms (round 5: [0] derived,
// 10 instead of 14 instructions and 18 instead of 24 LDS reads: - 7 %; tile shapes, words per step, workgroups per CU, unrolling and leaving the
// present plane unfetched all within 3 % of one another, profiles/r05ac, r05ad) -> 74 ms: what held it was the launch -- as a 2-D grid of all
// tiles the upper triangle's tiles were dealt to the XCDs 10 : 24 (blockIdx % 8; PMC: 7.9 waves resident per CU of 16); now the list of tiles that hold a
// pair is launched, split by split (profiles/r05ag: two words of the loop unrolled, two workgroups per CU: another 3 %).  Round 3's account:
// the 121 VALU instructions of a word step issue at 1.0 per SIMD and 4 cycles on their own (a 75 ms floor), the 24 LDS reads beside them
// cost ~23 ms, the barrier per eight words and the issue of the next loads ~17 (profiles/r03zzk_pair_kernel_diagnostics.log).
// counts [0] exactly one '-', [2] both unambiguous, [3] both unambiguous and equal.  Rows (first samples) [i_lo, i_hi) only.
#ifndef SKX_PAIR_FW
#define SKX_PAIR_FW 8
#endif
constexpr int FT = 64, FW = SKX_PAIR_FW;
__device__ static inline uint32_t bcnt_acc(uint32_t x, uint32_t acc)
{
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
}
#ifndef SKX_PAIR_WPS
#define SKX_PAIR_WPS 2
#endif
#ifndef SKX_PAIR_EQ2
#define SKX_PAIR_EQ2 1
#endif
#ifndef SKX_PAIR_NB
#define SKX_PAIR_NB 2
#endif
#ifndef SKX_PAIR_UNROLL
#define SKX_PAIR_UNROLL 2
#endif
// NB = second samples per thread (4: 256 threads, 4 x 4 pairs each; 2: 512 threads, 4 x 2)
constexpr int FNB = SKX_PAIR_NB, FNT = 256 * 4 / FNB, FLJ = FT / FNB;
__global__ __launch_bounds__(FNT, SKX_PAIR_WPS) void pair_counts_filt_kernel(const uint64_t *planes, int n_samples, uint64_t wpr, uint64_t words_per_split,
                                                               unsigned long long *out, int i_lo, int i_hi, int slot_u, int slot_e, const uint32_t *tiles, uint32_t n_tiles, uint32_t split0)
{
    __shared__ uint64_t s_i[2][4][FT][FW + 1];                              // two buffers: one is counted while the next is filled (one barrier per step)
    __shared__ uint64_t s_j[2][4][FT][FW + 1];
    // Round 5: [0] is not counted pair by pair any more.  Where no cell of a word is ambiguous, present = unambiguous, and
    // |Pi ^ Pj| = |Ui| + |Uj| - 2 |Ui & Uj|: the per-sample totals are counted once (plane_totals_kernel), |Ui & Uj| is [slot_u] anyway, and
    // pair_fix_kernel puts the sum into [0] afterwards -- 10 instead of 14 instructions per pair and 64 rows, 18 instead of 24 LDS reads
    // a word.  A word in which some staged cell is present but ambiguous (the threads that stage it see that: s_amb[buffer][word] = the
    // step's number) is counted in full, as the difference |Pi ^ Pj| - |Ui ^ Uj| that the fix-up lacks.
    __shared__ uint32_t s_amb[2][FW];
    // the grid is the list of tiles that hold a pair (i, j > i), split by split: blockIdx -> XCD is b % 8, and as a 2-D grid of all tiles --
    // half of them empty -- XCD x got the tile columns x and x + 8, 10 tiles of the upper triangle of 16 x 16 for XCD 0 against 24 for XCD 7
    const uint32_t tile = tiles[blockIdx.x % n_tiles];
    const int row0 = i_lo + (int)(tile >> 16) * FT, tj = (int)(tile & 0xFFFFu);      // tile rows start at the band's first sample: no row outside the band is counted
    const uint64_t w_begin = ((uint64_t)split0 + blockIdx.x / n_tiles) * words_per_split;
    const uint64_t w_end = w_begin + words_per_split < wpr ? w_begin + words_per_split : wpr;
    if (w_begin >= w_end) return;
    const int li = threadIdx.x / FLJ, lj = threadIdx.x % FLJ;               // first samples li + 16 a (a < 4), second samples lj + FLJ b (b < NB)
    const uint64_t plane_stride = (uint64_t)n_samples * wpr;
    uint32_t cu[4][FNB], ce[4][FNB]; int32_t cx[4][FNB];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < FNB; b++) { cx[a][b] = 0; cu[a][b] = 0; ce[a][b] = 0; }
    if (threadIdx.x < 2 * FW) (&s_amb[0][0])[threadIdx.x] = 0u;           // (step numbers start at 1)
    // staging: thread t brings word t % FW of rows t / FW + RS h (h < NH) of each of the four planes, for both sides: loads whose
    // addresses are one 32-bit per-thread offset from a wave-uniform base each (plane, slab of RS rows)
    constexpr int RS = FNT / FW < FT ? FNT / FW : FT, NH = FT / RS, NQ = 4 * NH;
    uint64_t ri[NQ], rj[NQ];
    typedef const uint64_t __attribute__((address_space(1))) *gplane_t;
    const int sw = threadIdx.x % FW, sr = threadIdx.x / FW;
    const bool stager = sr < RS;                                          // (more threads than words when FNT / FW > FT)
    const uint32_t toff = (uint32_t)((uint64_t)sr * wpr + sw);            // < 64 rows x wpr words: fits (wpr < 2^25 per launch_pair_counts)
    bool oki[NH], okj[NH];
#pragma unroll
    for (int hh = 0; hh < NH; hh++) { oki[hh] = stager && row0 + sr + RS * hh < n_samples; okj[hh] = stager && tj * FT + sr + RS * hh < n_samples; }
    auto fetch = [&](uint64_t w0) {
        const bool inw = w0 + sw < w_end;
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const int pl = q / NH, hh = q % NH;
            gplane_t bi = (gplane_t)(uintptr_t)(planes + pl * plane_stride + ((uint64_t)row0 + RS * hh) * wpr + w0);
            gplane_t bj = (gplane_t)(uintptr_t)(planes + pl * plane_stride + ((uint64_t)tj * FT + RS * hh) * wpr + w0);
            ri[q] = (inw && oki[hh]) ? bi[toff] : 0ull;
            rj[q] = (inw && okj[hh]) ? bj[toff] : 0ull;
        }
    };
    auto park = [&](int buf, uint32_t step_no) {
        if (stager) {
            uint64_t amb = 0;                                               // present and not unambiguous, in any of this thread's rows of the word
#pragma unroll
            for (int q = 0; q < NQ; q++) { s_i[buf][q / NH][sr + RS * (q % NH)][sw] = ri[q]; s_j[buf][q / NH][sr + RS * (q % NH)][sw] = rj[q]; }
#pragma unroll
            for (int hh = 0; hh < NH; hh++) amb |= (ri[hh] & ~ri[NH + hh]) | (rj[hh] & ~rj[NH + hh]);
            if (amb) s_amb[buf][sw] = step_no;
        }
    };
    uint32_t step_no = 1;
    fetch(w_begin);
    __syncthreads();                                                         // (s_amb is zero)
    park(0, step_no);
    __syncthreads();
    int cur = 0;
    for (uint64_t w0 = w_begin; w0 < w_end; w0 += FW, cur ^= 1, step_no++) {
        const bool more = w0 + FW < w_end;
        if (more) fetch(w0 + FW);
#pragma unroll SKX_PAIR_UNROLL
        for (int w = 0; w < FW; w++) {
            uint64_t Ui[4], Ai[4], Bi[4];
#pragma unroll
            for (int a = 0; a < 4; a++) { Ui[a] = s_i[cur][1][li + 16 * a][w]; Ai[a] = s_i[cur][2][li + 16 * a][w]; Bi[a] = s_i[cur][3][li + 16 * a][w]; }
            if (__builtin_amdgcn_readfirstlane(s_amb[cur][w]) == step_no) {
                // a word with an ambiguous cell somewhere in the tile: what [0] gets there beyond the fix-up's formula
#pragma unroll
                for (int b = 0; b < FNB; b++) {
                    const uint64_t Pj = s_j[cur][0][lj + FLJ * b][w], Uj = s_j[cur][1][lj + FLJ * b][w];
#pragma unroll
                    for (int a = 0; a < 4; a++) {
                        const uint64_t Pi = s_i[cur][0][li + 16 * a][w];
                        cx[a][b] += (int32_t)__popcll(Pi ^ Pj) - (int32_t)__popcll(Ui[a] ^ Uj);
                    }
                }
            }
#pragma unroll
            for (int b = 0; b < FNB; b++) {
                const uint64_t Uj = s_j[cur][1][lj + FLJ * b][w], Aj = s_j[cur][2][lj + FLJ * b][w], Bj = s_j[cur][3][lj + FLJ * b][w];
#pragma unroll
                for (int a = 0; a < 4; a++) {
                    // 32-bit halves; every popcount adds into its counter (v_bcnt_u32_b32 dst = popcount(src0) + src1, written as asm:
                    // the compiler otherwise counts into zero and adds), the equality mask is one three-input bit operation:
                    // 10 instructions per pair and 64 rows -- 2 + 2 for [2], 3 + 3 for [3] ([0]: see s_amb)
#pragma unroll
                    for (int hf = 0; hf < 2; hf++) {
                        const uint32_t both = (uint32_t)(Ui[a] >> (32 * hf)) & (uint32_t)(Uj >> (32 * hf));
                        cu[a][b] = bcnt_acc(both, cu[a][b]);
#if SKX_PAIR_EQ2
                        // t & ~(x ^ y) is one three-input operation (table 0x90: t set and x == y): the code bits are compared plane by plane
                        const uint32_t ta = __builtin_amdgcn_bitop3_b32(both, (uint32_t)(Ai[a] >> (32 * hf)), (uint32_t)(Aj >> (32 * hf)), 0x90);
                        ce[a][b] = bcnt_acc(__builtin_amdgcn_bitop3_b32(ta, (uint32_t)(Bi[a] >> (32 * hf)), (uint32_t)(Bj >> (32 * hf)), 0x90), ce[a][b]);
#else
                        const uint32_t da = (uint32_t)(Ai[a] >> (32 * hf)) ^ (uint32_t)(Aj >> (32 * hf));
                        const uint32_t db = (uint32_t)(Bi[a] >> (32 * hf)) ^ (uint32_t)(Bj >> (32 * hf));
                        ce[a][b] = bcnt_acc(__builtin_amdgcn_bitop3_b32(both, da, db, 0x10), ce[a][b]);      // both & ~da & ~db
#endif
                    }
                }
            }
        }
        if (more) park(cur ^ 1, step_no + 1);                               // nobody reads that buffer: its last readers passed the barrier of the step before
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < FNB; b++) {
            const int si = row0 + li + 16 * a, sj = tj * FT + lj + FLJ * b;
            if (si < i_hi && sj < n_samples && si < sj) {
                unsigned long long *o = out + ((uint64_t)(si - i_lo) * n_samples + sj) * DIST_NCOUNT;
                if (cx[a][b]) atomicAdd(&o[0], (unsigned long long)(long long)cx[a][b]);      // (may be negative: the sum with the fix-up is not)
                if (cu[a][b]) atomicAdd(&o[slot_u], (unsigned long long)cu[a][b]);        // (2, 3; or 1, 2 when the rows are the clean rows of an --allow-ambiguous table)
                if (ce[a][b]) atomicAdd(&o[slot_e], (unsigned long long)ce[a][b]);
            }
        }
}

constexpr int PT = 32;        // PT x PT sample pairs per workgroup, 2 x 2 pairs per thread
constexpr int PW = 8;         // words staged per step
// --allow-ambiguous: all 8 planes, 12 pair classes.  32 x 32 sample pairs per workgroup, 2 x 2 pairs per thread (8 LDS reads per
// pair and 64 rows instead of 16).  Ambiguity codes are rare: when none of a wave's operand words has a cell with two or three
// bases (planes 6, 7), only classes [0], [1] and [2] can count, and [2] is "both unambiguous and equal" -- the wave takes the
// short form (26 instead of ~90 instructions per pair and 64 rows).  Counts accumulate through v_bcnt_u32_b32.
__global__ __launch_bounds__(256, 2) void pair_counts_kernel(const uint64_t *planes, int n_samples, uint64_t wpr, uint64_t words_per_split,
                                                          unsigned long long *out, int i_lo, int i_hi, const uint32_t *tiles, uint32_t n_tiles, uint32_t split0)
{
    constexpr int NP = 8;
    __shared__ uint64_t s_ib[2][NP][PT][PW + 1];                           // two buffers: one is counted while the next is filled (one barrier per step)
    __shared__ uint64_t s_jb[2][NP][PT][PW + 1];
    const uint32_t tile = tiles[blockIdx.x % n_tiles];                      // (the tiles that hold a pair, split by split: pair_counts_filt_kernel)
    const int row0 = i_lo + (int)(tile >> 16) * PT, tj = (int)(tile & 0xFFFFu);
    const uint64_t w_begin = ((uint64_t)split0 + blockIdx.x / n_tiles) * words_per_split;
    const uint64_t w_end = w_begin + words_per_split < wpr ? w_begin + words_per_split : wpr;
    if (w_begin >= w_end) return;
    const int li = threadIdx.x / 16, lj = threadIdx.x % 16;              // first samples li + 16 a, second samples lj + 16 b (a, b < 2)
    const uint64_t plane_stride = (uint64_t)n_samples * wpr;
    uint32_t cnt[2][2][12];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int i = 0; i < 12; i++) cnt[a][b][i] = 0;
    // staging as in pair_counts_filt_kernel: thread t brings word t % PW of row t / PW of each of the eight planes, for both sides
    static_assert(256 / PW == PT, "one row per thread");
    uint64_t ri[NP], rj[NP];
    typedef const uint64_t __attribute__((address_space(1))) *gplane_t;
    const int sw = threadIdx.x % PW, sr = threadIdx.x / PW;
    const uint32_t toff = (uint32_t)((uint64_t)sr * wpr + sw);
    const bool oki = row0 + sr < n_samples, okj = tj * PT + sr < n_samples;
    auto fetch = [&](uint64_t w0) {
        const bool inw = w0 + sw < w_end;
#pragma unroll
        for (int p = 0; p < NP; p++) {
            gplane_t bi = (gplane_t)(uintptr_t)(planes + p * plane_stride + (uint64_t)row0 * wpr + w0);
            gplane_t bj = (gplane_t)(uintptr_t)(planes + p * plane_stride + (uint64_t)tj * PT * wpr + w0);
            ri[p] = (inw && oki) ? bi[toff] : 0ull;
            rj[p] = (inw && okj) ? bj[toff] : 0ull;
        }
    };
    auto park = [&](int buf) {
#pragma unroll
        for (int p = 0; p < NP; p++) { s_ib[buf][p][sr][sw] = ri[p]; s_jb[buf][p][sr][sw] = rj[p]; }
    };
    fetch(w_begin);
    park(0);
    __syncthreads();
    int cur = 0;
    for (uint64_t w0 = w_begin; w0 < w_end; w0 += PW, cur ^= 1) {
        const bool more = w0 + PW < w_end;
        if (more) fetch(w0 + PW);
        const auto &s_i = s_ib[cur]; const auto &s_j = s_jb[cur];
#pragma unroll 1
        for (int w = 0; w < PW; w++) {
            uint64_t I[2][NP], J[2][NP];
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int p = 0; p < NP; p++) { I[a][p] = s_i[p][li + 16 * a][w]; J[a][p] = s_j[p][lj + 16 * a][w]; }
            const uint64_t amb = I[0][6] | I[0][7] | I[1][6] | I[1][7] | J[0][6] | J[0][7] | J[1][6] | J[1][7];
            const bool any_amb = __any(amb != 0ull);
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++) {
                    uint32_t *c = cnt[a][b];
#pragma unroll
                    for (int hf = 0; hf < 2; hf++) {
                        auto hi32 = [&](uint64_t x) { return (uint32_t)(x >> (32 * hf)); };
                        const uint32_t Pi = hi32(I[a][0]), Pj = hi32(J[b][0]);
                        const uint32_t iA = hi32(I[a][1]) & hi32(J[b][1]), iC = hi32(I[a][2]) & hi32(J[b][2]);
                        const uint32_t iT = hi32(I[a][3]) & hi32(J[b][3]), iG = hi32(I[a][4]) & hi32(J[b][4]);
                        const uint32_t z1 = hi32(I[a][5]) & hi32(J[b][5]);
                        c[0] = bcnt_acc(Pi ^ Pj, c[0]);
                        c[1] = bcnt_acc(Pi & Pj, c[1]);
                        if (!any_amb) {                                   // every present cell here is one base: equal <=> some base shared
                            c[2] = bcnt_acc(z1 & (__builtin_amdgcn_bitop3_b32(iA, iC, iT, 0xFE) | iG), c[2]);
                            continue;
                        }
                        // bit-sliced |S1 n S2| in {0..4}: s0 + 2 s1 (4 only when both are N, excluded by the size planes)
                        const uint32_t x3 = __builtin_amdgcn_bitop3_b32(iA, iC, iT, 0x96), m3 = __builtin_amdgcn_bitop3_b32(iA, iC, iT, 0xE8);   // a^b^c, majority
                        const uint32_t s0 = x3 ^ iG, s1 = m3 ^ (x3 & iG);
                        const uint32_t t1 = s0 & ~s1, t2 = ~s0 & s1, t3 = s0 & s1;
                        const uint32_t z1i = hi32(I[a][5]), z1j = hi32(J[b][5]), z2i = hi32(I[a][6]), z2j = hi32(J[b][6]), z3i = hi32(I[a][7]), z3j = hi32(J[b][7]);
                        const uint32_t m12 = (z1i & z2j) | (z2i & z1j), m13 = (z1i & z3j) | (z3i & z1j), m23 = (z2i & z3j) | (z3i & z2j);
                        const uint32_t z2 = z2i & z2j, z3 = z3i & z3j;
                        c[2] = bcnt_acc(z1 & t1, c[2]);                    // 1x1 t1 : 1
                        c[3] = bcnt_acc(m12 & t1, c[3]);                   // 1x2 t1 : 1/2
                        c[4] = bcnt_acc(m13 & t1, c[4]);                   // 1x3 t1 : 1/3
                        c[5] = bcnt_acc(z2 & t1, c[5]);                    // 2x2 t1 : 1/4
                        c[6] = bcnt_acc(z2 & t2, c[6]);                    // 2x2 t2 : 1/2
                        c[7] = bcnt_acc(m23 & t1, c[7]);                   // 2x3 t1 : 1/6
                        c[8] = bcnt_acc(m23 & t2, c[8]);                   // 2x3 t2 : 1/3
                        c[9] = bcnt_acc(z3 & t1, c[9]);                    // 3x3 t1 : 1/9
                        c[10] = bcnt_acc(z3 & t2, c[10]);                  // 3x3 t2 : 2/9
                        c[11] = bcnt_acc(z3 & t3, c[11]);                  // 3x3 t3 : 1/3
                    }
                }
        }
        if (more) park(cur ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const int si = row0 + li + 16 * a, sj = tj * PT + lj + 16 * b;
            if (si < i_hi && sj < n_samples && si < sj) {
                unsigned long long *o = out + ((uint64_t)(si - i_lo) * n_samples + sj) * DIST_NCOUNT;
#pragma unroll
                for (int i = 0; i < 12; i++) if (cnt[a][b][i]) atomicAdd(&o[i], (unsigned long long)cnt[a][b][i]);
            }
        }
}
// |U_s| of every sample over the planes' rows (plane 1 of the 4-plane layout): a wave per sample and slice of words
__global__ __launch_bounds__(256) void plane_totals_kernel(const uint64_t *planes, int n_samples, uint64_t wpr, unsigned long long *tot)
{
    const int s = blockIdx.x;
    const uint64_t *u = planes + (uint64_t)n_samples * wpr + (uint64_t)s * wpr;
    unsigned long long c = 0;
    for (uint64_t w = (uint64_t)blockIdx.y * 256 + threadIdx.x; w < wpr; w += (uint64_t)gridDim.y * 256) c += (unsigned long long)__popcll(u[w]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&tot[s], c);
}
// [0] of every pair of the band: |Ui| + |Uj| - 2 |Ui & Uj| on top of what the sweep left there (pair_counts_filt_kernel)
__global__ __launch_bounds__(256) void pair_fix_kernel(unsigned long long *out, const unsigned long long *tot, int n_samples, int i_lo, int i_hi, int slot_u)
{
    const int sj = blockIdx.x * 256 + threadIdx.x, si = i_lo + (int)blockIdx.y;
    if (si >= i_hi || sj >= n_samples || sj <= si) return;
    unsigned long long *o = out + ((uint64_t)(si - i_lo) * n_samples + sj) * DIST_NCOUNT;
    o[0] += tot[si] + tot[sj] - 2ull * o[slot_u];
}
// rows [i_lo, i_hi) of the pair matrix (out rows are relative to i_lo): one rank's band, or everything
// filt_ambig 2: the 4-plane sweep with its counts filed as the 12-class table's [0] exactly one '-', [1] both present, [2] both one base and
// equal -- what those classes are on rows where no cell is ambiguous (planes built with FILT over such rows: present = unambiguous there)
// Returns 0, or the hipError_t of the allocation / launch that failed (nothing is left running).  A filt_ambig launch derives count [0] from
// count [slot_u] (pair_fix_kernel: o[0] += |Ui| + |Uj| - 2 o[slot_u]): `out`'s slot_u must hold THIS launch's counts only, i.e. be zero on
// entry -- one filtered launch per out buffer (sweep_band in skx_distance.cpp runs its filtered launch first, into a zeroed buffer).
int launch_pair_counts(const uint64_t *planes, int n_samples, uint64_t wpr, int filt_ambig, unsigned long long *out, hipStream_t st, int i_lo, int i_hi)
{
    if (n_samples < 2 || !wpr) return 0;
    if (i_hi <= 0 || i_hi > n_samples) i_hi = n_samples;
    if (i_lo >= i_hi) return 0;
    const int side = filt_ambig ? FT : PT, step = filt_ambig ? FW : PW;
    const unsigned nt = (unsigned)((n_samples + side - 1) / side);
    const unsigned nty = (unsigned)((i_hi - i_lo + side - 1) / side);
    // the tiles with a pair (i, j > i) in them: (tile row of the band << 16 | tile column), row by row
    std::vector<uint32_t> h_tiles;
    for (unsigned by = 0; by < nty; by++) {
        const int row0 = i_lo + (int)by * side;
        for (unsigned tj = (unsigned)((row0 + 1) / side); tj < nt; tj++) h_tiles.push_back((by << 16) | tj);      // tj * side + side - 1 > row0
    }
    if (h_tiles.empty()) return 0;                                         // (nt, nty <= 1 024: at most 65 535 samples)
    // split the column range so that there are enough workgroups to fill 256 CUs; u32 counters hold < 2^32 columns per split
    uint64_t tiles = h_tiles.size();
    const uint64_t target = 2048;
    uint64_t splits = tiles >= target ? 1 : (target + tiles - 1) / tiles;
    uint64_t wps = (wpr + splits - 1) / splits;
    // workgroups run split by split (the split is the slow part of the block index) and every tile of a split re-reads that split's
    // slice of the planes: keep the slice (planes x samples x words) inside the 256 MB memory-side cache
    const uint64_t cache_words = (128ull << 20) / ((filt_ambig ? 4ull : 8ull) * (uint64_t)n_samples * 8ull);
    if (wps > cache_words) wps = cache_words ? cache_words : 1;
    wps = (wps + step - 1) / step * step;
    if (wps > (1ull << 25)) wps = 1ull << 25;
    splits = (wpr + wps - 1) / wps;
    uint32_t *d_tiles = nullptr; unsigned long long *tot = nullptr;
    hipError_t e = hipMalloc((void **)&d_tiles, tiles * 4);
    if (e != hipSuccess || !d_tiles) return (int)(e != hipSuccess ? e : hipErrorOutOfMemory);
    e = hipMemcpyAsync(d_tiles, h_tiles.data(), tiles * 4, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { (void)hipFree(d_tiles); return (int)e; }
    const uint64_t per_launch = std::max<uint64_t>(1, 0x3FFFFFFFull / tiles);            // splits per launch (the grid's x extent)
    if (filt_ambig) {
        const int slot_u = filt_ambig == 2 ? 1 : 2;
        e = hipMalloc((void **)&tot, (size_t)n_samples * 8);
        if (e != hipSuccess || !tot) { (void)hipFree(d_tiles); return (int)(e != hipSuccess ? e : hipErrorOutOfMemory); }
        (void)hipMemsetAsync(tot, 0, (size_t)n_samples * 8, st);
        const unsigned gy = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(64, wpr / 4096));
        hipLaunchKernelGGL(plane_totals_kernel, dim3((unsigned)n_samples, gy), dim3(256), 0, st, planes, n_samples, wpr, tot);
        for (uint64_t z0 = 0; z0 < splits; z0 += per_launch)
            hipLaunchKernelGGL(pair_counts_filt_kernel, dim3((unsigned)(tiles * std::min(per_launch, splits - z0))), dim3(FNT), 0, st, planes, n_samples, wpr, wps, out, i_lo, i_hi,
                               slot_u, filt_ambig == 2 ? 2 : 3, d_tiles, (uint32_t)tiles, (uint32_t)z0);
        hipLaunchKernelGGL(pair_fix_kernel, dim3((unsigned)((n_samples + 255) / 256), (unsigned)(i_hi - i_lo)), dim3(256), 0, st, out, tot, n_samples, i_lo, i_hi, slot_u);
    } else
        for (uint64_t z0 = 0; z0 < splits; z0 += per_launch)
            hipLaunchKernelGGL(pair_counts_kernel, dim3((unsigned)(tiles * std::min(per_launch, splits - z0))), dim3(256), 0, st, planes, n_samples, wpr, wps, out, i_lo, i_hi,
                               d_tiles, (uint32_t)tiles, (uint32_t)z0);
    e = hipGetLastError();                                                 // a launch that was refused
    const hipError_t es = hipStreamSynchronize(st);                        // (h_tiles, d_tiles and tot go)
    (void)hipFree(d_tiles);
    if (tot) (void)hipFree(tot);
    return (int)(e != hipSuccess ? e : es);
}

}  // namespace skx
