// skx_cells.h -- what the kernels of the matrix commands share (`ska markers`, `curve`, `screen`, `qc`, `density`): the cell alphabet, a lane's 16
// columns and the walk over their samples, the half-wave sum, and a reference window's record and matching byte.  Device code only.
//
// The matrix is sample-major, so a row of the reference is a column here.  A thread (ColumnLane) owns 16 consecutive columns -- one 16-byte load
// per sample -- and a workgroup of 256 threads a tile of 4 096.  walk_columns takes the samples [s0, s1) through four load buffers, each in
// registers of its own, so that a step waits for its own sample's load and leaves the three younger ones in flight (as compiled, three or four
// loads are in flight ahead of a step: the fourth of the first round is sunk into the loop, NOTEBOOK 2026-10-20, qc).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace skx {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ASCII middle base -> IUPAC set code (A 1, C 2, T 4, G 8; '-' and the 0 byte are 0); CELL_OUTSIDE: a byte outside -ACGTMRWSYKVHDBN.  Every
// kernel's LDS table is an expression of this code, written where the table is filled
constexpr uint32_t CELL_OUTSIDE = 0x100u;
constexpr uint32_t cell_code_of(uint32_t b)
{
    switch (b) {
    case 0: case '-': return 0;
    case 'A': return 1;  case 'C': return 2;  case 'M': return 3;  case 'T': return 4;  case 'W': return 5;  case 'Y': return 6;  case 'H': return 7;
    case 'G': return 8;  case 'R': return 9;  case 'S': return 10; case 'V': return 11; case 'K': return 12; case 'D': return 13; case 'B': return 14;
    case 'N': return 15;
    default: return CELL_OUTSIDE;
    }
}
// (the switch, taken per lane, compiles to a tree of compares under exec masks: some 200 instructions in front of every workgroup.  It is
// evaluated here for the 256 bytes when the file is compiled, and a lane reads its entry)
struct CellCodes {
    uint16_t v[256];
    constexpr CellCodes() : v{} { for (uint32_t b = 0; b < 256; b++) v[b] = (uint16_t)cell_code_of(b); }
};
__device__ inline uint32_t cell_code(uint32_t b)
{
    static constexpr CellCodes codes{};
    return codes.v[b & 0xFFu];
}
__device__ inline bool cell_present(uint32_t c) { return c != 0 && c != CELL_OUTSIDE; }
__device__ inline bool cell_one_base(uint32_t c) { return c == 1 || c == 2 || c == 4 || c == 8; }      // one of A, C, T, G

// what a thread owns: 16 columns from c0.  One past the last column walks column 0 behind a mask of zeros, so every barrier and wave operation
// stays whole.  Rows are padded to the pitch (>= 256 bytes past n_cols), so the 16-byte load of a thread with c0 < n_cols stays inside the row;
// what it holds past n_cols is masked away: vm holds 0xFF for the bytes of the columns below n_cols
struct ColumnLane {
    bool live; const uint8_t *col; u32x4 vm;
    __device__ ColumnLane(const uint8_t *matrix, uint64_t n_cols, uint64_t c0)
    {
        live = c0 < n_cols;
        col = matrix + (live ? c0 : 0);
        const uint32_t n_valid = !live ? 0u : (n_cols - c0 >= 16 ? 16u : (uint32_t)(n_cols - c0));
#pragma unroll
        for (int w = 0; w < 4; w++) { const uint32_t nb = n_valid > 4u * w ? min(n_valid - 4u * w, 4u) : 0u; vm[w] = nb >= 4 ? 0xFFFFFFFFu : (1u << (8 * nb)) - 1u; }
    }
};

// step(t, load(t)) for t = s0 .. s1 - 1 in order (s0 < s1; the bounds are the same for the whole workgroup), with the loads of t + 1 .. t + 3
// issued before step(t).  load is called up to s1 + 3 and clamps its argument itself: past the last sample the last one is loaded again and
// never used -- a load that is always issued keeps the count of loads in flight the same on every path, so a step waits for its own sample's
// load and not for the younger ones.  The first four are issued in the order the loop issues them: the wait at the loop's head then leaves the
// three younger loads in flight
template <typename Load, typename Step>
__device__ __forceinline__ void walk_columns(uint32_t s0, uint32_t s1, const Load &load, const Step &step)
{
    u32x4 b0 = load(s0);
    __builtin_amdgcn_sched_barrier(0);
    u32x4 b1 = load(s0 + 1);
    __builtin_amdgcn_sched_barrier(0);
    u32x4 b2 = load(s0 + 2);
    __builtin_amdgcn_sched_barrier(0);
    u32x4 b3 = load(s0 + 3);
    for (uint32_t t = s0; t < s1; t += 4) {                         // (b0 holds sample t)
        step(t, b0); b0 = load(t + 4);
        if (t + 1 < s1) step(t + 1, b1);
        b1 = load(t + 5);
        if (t + 2 < s1) step(t + 2, b2);
        b2 = load(t + 6);
        if (t + 3 < s1) step(t + 3, b3);
        b3 = load(t + 7);
    }
}

// the sum of v over lanes 0-31 in lane 31 and over lanes 32-63 in lane 63: four shifts inside each row of 16 lanes, then the last lane of rows 0
// and 2 added to rows 1 and 3
__device__ inline uint32_t half_wave_sum(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);      // row_shr:1 (a lane without a source adds the 0)
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);      // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);      // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);      // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);      // row_bcast:15 into rows 1 and 3
    return v;
}

// the record (chromosome) of position x: the last of starts[0 .. n) at or before x (starts ascending, starts[0] <= x)
__device__ inline uint32_t chrom_of(const uint64_t *starts, uint32_t n, uint64_t x)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint32_t c = (lo + hi) >> 1; if (starts[c] <= x) lo = c; else hi = c; }
    return lo;
}

// the byte a cell holds when it matches the reference at a window: the window's middle base upper-cased (a window's letters are ACGT in either
// case), complemented where the reference strand is not the canonical one.  RC_IUPAC is a bijection on the alphabet that keeps A, C, G, T among
// themselves, so cell == complement(base) says what RC_IUPAC(cell) == base says: no cell is translated
__device__ inline uint8_t want_byte(uint8_t mid, bool is_rc)
{
    const uint8_t b = mid & 0xDFu;
    const uint8_t comp = b == 'A' ? 'T' : b == 'C' ? 'G' : b == 'G' ? 'C' : 'A';
    return is_rc ? comp : b;
}

}  // namespace skx
