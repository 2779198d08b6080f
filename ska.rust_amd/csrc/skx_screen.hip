// skx_screen.hip -- `ska screen`: which samples carry which records of a multi-FASTA panel, and how well they match (skx_array_screen,
// include/skx.h; definition there and in tests/screen_model.py).  The reference has no counterpart: its users run `ska map` on the panel
// (generic_modes.rs:56-84) and count columns of an S x panel-length alignment, or `ska weed --reverse` and `ska nk` once per record.
//
// The windows, their look-up and the compaction of the hits are `ska map`'s (RefLookup, skx_internal.h).  What is
// new is the reduction from (hit window, sample) cells to three integers per (record, sample) without the cells ever being stored.
// screen_pack_kernel turns the hit list into what the walk needs per window: its row, its record and the byte a matching cell holds -- the
// record's middle base upper-cased, complemented where the reference strand is not the canonical one (want_byte, skx_cells.h; present and
// ambiguous are the same on either strand).  screen_kernel: a workgroup takes SKX_SCREEN_TILE consecutive hit windows and
// SKX_SCREEN_SAMPLES samples; a lane is a sample.  The tile's rows, records and bytes are staged in LDS and read as broadcasts into scalar
// registers; a lane's byte of window j is matrix[s * pitch + row[j]] -- the matrix is sample-major, so the 64 lanes of a wave read 64
// different lines: the gathers are inherent, what is left is to keep many in flight.  The walk is unrolled by SCREEN_UNROLL with the next
// group's loads issued before the current group's bytes are used, each in a register of its own, so a step waits for its own byte with the
// next group's loads left in flight (as in skx_curve.hip loads are issued on every path: past the tile's end the last window is loaded
// again and never counted).  The group's end copies the next bytes over the current ones, which waits for all of them: NOTEBOOK 2026-10-20, screen.
// A lane keeps the running record's three counts in registers and adds them to cells[record][s] when the record changes and at the tile's
// end.  Tiles share records, so these are integer atomics: the result does not depend on who arrives first.  No workgroup waits for
// another, every loop is bounded by the tile, and the one barrier is reached by all 256 threads: a wave whose samples are all past S
// leaves behind it, a lane past S in a live wave walks sample S - 1 and adds nothing.
//
// Device memory beside the array: `ska map`'s window buffers (25 bytes a panel byte at k <= 31, 33 above), 9 bytes a hit window and
// 12 bytes a (record, sample) pair.
#include "skx_internal.h"
#include "skx_cells.h"
#include <algorithm>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

namespace skx {
namespace {

constexpr uint32_t SCREEN_TILE = SKX_SCREEN_TILE;
constexpr uint32_t SCREEN_SAMPLES = SKX_SCREEN_SAMPLES;
constexpr uint32_t SCREEN_UNROLL = 8;
static_assert(SCREEN_SAMPLES == 256, "a workgroup of 256 threads, a sample each");
static_assert(SCREEN_TILE % SCREEN_UNROLL == 0, "the walk is unrolled by the loads of a group");

// per hit window m (panel order): the array's row, the record, the byte of a matching cell
__global__ __launch_bounds__(256) void screen_pack_kernel(const uint32_t *mapped, const uint32_t *row, const uint8_t *is_rc, const uint8_t *seq, uint32_t h,
                                                         const uint64_t *cstart, uint32_t n_records, uint64_t M, uint32_t *hrow, uint32_t *hrec, uint8_t *hwant)
{
    const uint64_t m = blockIdx.x * 256ull + threadIdx.x;
    if (m >= M) return;
    const uint32_t p = mapped[m];
    const uint64_t mid = (uint64_t)p - h;
    hrow[m] = row[p]; hrec[m] = chrom_of(cstart, n_records, mid); hwant[m] = want_byte(seq[mid], is_rc[p]);
}

struct ScreenArgs {
    const uint8_t *matrix; uint64_t pitch;
    const uint32_t *hrow, *hrec; const uint8_t *hwant; uint64_t M;
    uint32_t S;
    uint32_t *cells;                                                // [n_records][S][3] found, match, ambig
    int *bad_byte;
};

__global__ __launch_bounds__(256) void screen_kernel(ScreenArgs a)
{
    __shared__ uint32_t s_lut[256];                                 // bit 0: present; bit 1: present and none of A, C, G, T; bit 8: outside the alphabet
    __shared__ uint32_t s_row[SCREEN_TILE];
    __shared__ uint32_t s_rec[SCREEN_TILE];
    __shared__ uint32_t s_want[SCREEN_TILE];
    const uint64_t m0 = (uint64_t)blockIdx.x * SCREEN_TILE;
    const uint32_t n = (uint32_t)min((uint64_t)SCREEN_TILE, a.M - m0);          // >= 1: the grid has no empty tile
    {
        const uint32_t c = cell_code(threadIdx.x);
        s_lut[threadIdx.x] = c == CELL_OUTSIDE ? 0x100u : c == 0 ? 0u : cell_one_base(c) ? 1u : 3u;
    }
    // (past the tile's end the last window again: every index the walk forms names a staged window)
    for (uint32_t j = threadIdx.x; j < SCREEN_TILE; j += 256) {
        const uint64_t m = m0 + min(j, n - 1);
        s_row[j] = a.hrow[m]; s_rec[j] = a.hrec[m]; s_want[j] = a.hwant[m];
    }
    __syncthreads();
    const uint32_t s = blockIdx.y * SCREEN_SAMPLES + threadIdx.x;
    if (s - (threadIdx.x & 63u) >= a.S) return;                     // the whole wave is past the last sample (no barrier follows)
    const bool live = s < a.S;
    const uint8_t *col = a.matrix + (uint64_t)(live ? s : a.S - 1) * a.pitch;

    uint32_t found = 0, match = 0, ambig = 0, bad = 0;
    uint32_t cur = __builtin_amdgcn_readfirstlane(s_rec[0]);
    auto flush = [&]() {
        if (!live) return;
        uint32_t *o = a.cells + ((uint64_t)cur * a.S + s) * 3;
        if (found) atomicAdd(o + 0, found);
        if (match) atomicAdd(o + 1, match);
        if (ambig) atomicAdd(o + 2, ambig);
    };
    // a window's row is the same in every lane: read from LDS as a broadcast and kept in a scalar register
    auto load = [&](uint32_t j) -> uint32_t { return col[__builtin_amdgcn_readfirstlane(s_row[j])]; };
    auto step = [&](uint32_t j, uint32_t b) {
        const uint32_t rec = __builtin_amdgcn_readfirstlane(s_rec[j]);
        if (rec != cur) { flush(); cur = rec; found = match = ambig = 0; }
        const uint32_t v = s_lut[b];
        bad |= v;
        found += v & 1u; ambig += (v >> 1) & 1u;
        match += b == (uint32_t)__builtin_amdgcn_readfirstlane(s_want[j]) ? 1u : 0u;
    };
    uint32_t b[SCREEN_UNROLL], nx[SCREEN_UNROLL];
#pragma unroll
    for (uint32_t u = 0; u < SCREEN_UNROLL; u++) b[u] = load(u);
    for (uint32_t j0 = 0; j0 < n; j0 += SCREEN_UNROLL) {            // (n and every bound below are the same for the whole workgroup)
        const uint32_t jn = j0 + SCREEN_UNROLL < SCREEN_TILE ? j0 + SCREEN_UNROLL : j0;     // the next group, or this one again behind the last
#pragma unroll
        for (uint32_t u = 0; u < SCREEN_UNROLL; u++) nx[u] = load(jn + u);
#pragma unroll
        for (uint32_t u = 0; u < SCREEN_UNROLL; u++) if (j0 + u < n) step(j0 + u, b[u]);
#pragma unroll
        for (uint32_t u = 0; u < SCREEN_UNROLL; u++) b[u] = nx[u];
    }
    flush();
    if (live && (bad & 0x100u)) *a.bad_byte = 1;
}

}  // namespace
}  // namespace skx

using namespace skx;

extern "C" int skx_array_screen(skx_array *a, const char *panel_fasta, uint64_t *n_records, skx_screen_record **records, char **ids, skx_screen_cell **cells)
{
    return skx_guarded([&]() -> int {
    if (!a || !panel_fasta || !n_records || !records || !ids || !cells) { set_error("screen: bad arguments"); return SKX_EINVAL; }
    *n_records = 0; *records = nullptr; *ids = nullptr; *cells = nullptr;
    skx_ctx *ctx = a->ctx; hipStream_t st = ctx->stream;
    SKX_HIP(hipSetDevice(ctx->device));
    const int k = a->k, h = (k - 1) / 2;
    const uint64_t S = a->names.size();
    if (a->n_kmers != a->n_rows || a->keys_absent) { set_error("split k-mers and variants are out of step (filtered without update_kmers)"); return SKX_EINVAL; }
    if (a->total_samples && a->total_samples != S) { set_error("screen: needs every sample of the array on one device"); return SKX_EUNSUP; }
    if (S == 0) { set_error("screen: the array has no samples"); return SKX_EINVAL; }
    SKX_TRY(array_materialize(a));
    RefLookup ref;
    {
        PhaseTimer pr("screen.read_panel");
        SKX_TRY(ref.read(panel_fasta, "screen: panel longer than 4 G bases"));
    }
    const HostStream &hs = ref.hs;
    const std::vector<uint64_t> &cstart = ref.cstart, &clen = ref.clen;         // records: start in the record stream and length
    const uint64_t R = cstart.size();
    if (hs.ids.size() != R) { set_error("screen: %s: %llu record ids for %llu records", panel_fasta, (unsigned long long)hs.ids.size(), (unsigned long long)R); return SKX_EINVAL; }
    {
        std::unordered_set<std::string> seen;
        for (auto &id : hs.ids) if (!seen.insert(id).second) { set_error("screen: %s: record id %s occurs more than once", panel_fasta, id.c_str()); return SKX_EINVAL; }
    }
    PhaseTimer pw("screen.windows");
    SKX_TRY(ref.windows(a, panel_fasta, false));
    // a window is flagged at its last letter p; its middle base, p - h, says which record it belongs to
    std::vector<skx_screen_record> rec(R);
    for (uint64_t c = 0; c < R; c++) {
        uint64_t w = 0;
        for (uint64_t p = cstart[c]; p < cstart[c] + clen[c]; p++) w += ref.hflag[p] != 0;
        rec[c].length = clen[c]; rec[c].windows = w; rec[c].rows_hit = 0;
    }
    if (R * S > (1ull << 31)) { set_error("screen: %llu records x %llu samples; at most 2^31 (record, sample) pairs are taken", (unsigned long long)R, (unsigned long long)S); return SKX_EUNSUP; }
    pw.stop();

    // look-up and compaction (an array without rows has no hit)
    if (a->n_rows) {
        PhaseTimer pl("screen.lookup");
        SKX_TRY(ref.lookup(a));
    }
    ref.wlo.release(); ref.whi.release();
    const DevBuf<uint32_t> &row = ref.row, &mapped = ref.mapped; const DevBuf<uint8_t> &is_rc = ref.is_rc, &d_seq = ref.d_seq;
    const uint64_t M = ref.M;

    const size_t n_cells = (size_t)(R * S);
    skx_screen_cell *out_cells = (skx_screen_cell *)calloc(n_cells ? n_cells : 1, sizeof(skx_screen_cell));
    skx_screen_record *out_rec = (skx_screen_record *)malloc((R ? R : 1) * sizeof(skx_screen_record));
    size_t id_bytes = 0; for (auto &id : hs.ids) id_bytes += id.size() + 1;
    char *out_ids = (char *)malloc(id_bytes ? id_bytes : 1);
    struct Mem { void *p[3]; bool keep = false; ~Mem() { if (!keep) for (void *q : p) free(q); } } mem{{out_cells, out_rec, out_ids}};
    if (!out_cells || !out_rec || !out_ids) { set_error("out of host memory"); return SKX_ENOMEM; }
    { char *w = out_ids; for (auto &id : hs.ids) { memcpy(w, id.c_str(), id.size() + 1); w += id.size() + 1; } }

    if (M) {
        PhaseTimer pk("screen.kernel");
        // hits per record: the hit list is in panel order
        std::vector<uint32_t> hm(M);
        SKX_HIP(hipMemcpy(hm.data(), mapped.p, M * 4, hipMemcpyDeviceToHost));
        { uint64_t c = 0; for (uint64_t m = 0; m < M; m++) { const uint64_t mid = (uint64_t)hm[m] - h; while (c + 1 < R && cstart[c + 1] <= mid) c++; rec[c].rows_hit++; } }
        DevBuf<uint64_t> d_cstart; DevBuf<uint32_t> hrow, hrec, d_cells; DevBuf<uint8_t> hwant; DevBuf<int> d_bad;
        SKX_TRY(d_cstart.alloc(R)); SKX_TRY(hrow.alloc(M)); SKX_TRY(hrec.alloc(M)); SKX_TRY(hwant.alloc(M)); SKX_TRY(d_cells.alloc(n_cells * 3));
        SKX_TRY(d_bad.alloc(1)); SKX_TRY(d_bad.zero(st)); SKX_TRY(d_cells.zero(st));
        SKX_HIP(hipMemcpyAsync(d_cstart.p, cstart.data(), R * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(screen_pack_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, mapped.p, row.p, is_rc.p, d_seq.p, (uint32_t)h, d_cstart.p, (uint32_t)R, M,
                           hrow.p, hrec.p, hwant.p);
        SKX_HIP(hipGetLastError());
        ScreenArgs ka{};
        ka.matrix = a->matrix.p; ka.pitch = a->pitch; ka.hrow = hrow.p; ka.hrec = hrec.p; ka.hwant = hwant.p; ka.M = M; ka.S = (uint32_t)S;
        ka.cells = d_cells.p; ka.bad_byte = d_bad.p;
        const uint64_t n_tiles = (M + SCREEN_TILE - 1) / SCREEN_TILE, n_blocks = (S + SCREEN_SAMPLES - 1) / SCREEN_SAMPLES;      // M < 2^32: n_tiles < 2^22; S <= 2^31: n_blocks <= 2^23
        if (n_blocks > 65535) { set_error("screen: %llu samples; at most %u are taken", (unsigned long long)S, 65535u * SCREEN_SAMPLES); return SKX_EUNSUP; }
        hipLaunchKernelGGL(screen_kernel, dim3((unsigned)n_tiles, (unsigned)n_blocks), dim3(256), 0, st, ka);
        SKX_HIP(hipGetLastError());
        int bad = 0;
        SKX_HIP(hipMemcpyAsync(out_cells, d_cells.p, n_cells * sizeof(skx_screen_cell), hipMemcpyDeviceToHost, st));
        SKX_HIP(hipMemcpyAsync(&bad, d_bad.p, 4, hipMemcpyDeviceToHost, st));
        SKX_HIP(hipStreamSynchronize(st));
        if (bad) { set_error("screen: variants contain a byte outside -ACGTMRWSYKVHDBN"); return SKX_EINVAL; }
    }
    memcpy(out_rec, rec.data(), R * sizeof(skx_screen_record));
    mem.keep = true;
    *n_records = R; *records = out_rec; *ids = out_ids; *cells = out_cells;
    return SKX_OK;
    });
}
