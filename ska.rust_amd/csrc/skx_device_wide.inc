// skx_device_wide.inc -- the 128-bit path (k = 33..63, lib.rs:592-622 picks u128): same pipeline as the 64-bit
// kernels of skx_device.hip with arms of up to 62 bits and 16-byte packed words.  Included by skx_device.hip.
namespace skx {

WideHash make_wide_hash(int k)
{
    WideHash p;
    p.bits = 2 * (k - 1); p.hb = k - 1;
    p.hmask = p.hb >= 64 ? ~0ull : ((1ull << p.hb) - 1);
    p.c[0] = 0x9E3779B97F4A7C15ull; p.c[1] = 0xD6E8FEB86659FD93ull; p.c[2] = 0xC2B2AE3D27D4EB4Full;
    return p;
}

__device__ static inline uint64_t revcomp_arm64(uint64_t x, int n)
{
    x = __builtin_bitreverse64(x);
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
    x ^= 0xAAAAAAAAAAAAAAAAull;
    return n ? x >> (64 - 2 * n) : 0;
}
__device__ static inline uint32_t wide_bucket(u128 w, int bshift) { return (uint32_t)((w >> 4) >> bshift); }
// 128-bit words on 64-bit halves (the generic u128 shifts / compares the compiler emits cost 10-17 VALU instructions each, and
// the kernels below run at > 90 % of the VALU issue rate: profiles/r02q_pmc_wide.txt)
__device__ static inline uint32_t field_w(u128 w, int s, uint32_t mask)          // (w >> s) & mask, 4 <= s < 128, mask < 2^32
{
    const uint64_t lo = (uint64_t)w, hi = (uint64_t)(w >> 64);
    const uint64_t x = s >= 64 ? hi >> (s & 63) : (lo >> (s & 63)) | ((hi << 1) << (63 - (s & 63)));
    return (uint32_t)x & mask;
}
__device__ static inline bool same_key_w(u128 a, u128 b)                          // equal above the 4 base-mask bits
{
    return (uint64_t)(a >> 64) == (uint64_t)(b >> 64) && (((uint64_t)a ^ (uint64_t)b) < 16ull);
}
__device__ static inline bool differ_from_w(u128 x, int s)                        // (x >> s) != 0, 4 <= s < 128
{
    const uint64_t lo = (uint64_t)x, hi = (uint64_t)(x >> 64);
    return s >= 64 ? (hi >> (s & 63)) != 0ull : (hi | (lo >> (s & 63))) != 0ull;
}

#if defined(SKX_PHASE_PROF) && SKX_PHASE_PROF == 5
#define DW_PROF(i) PHASE_PROF_(i)
#else
#define DW_PROF(i) do { } while (0)
#endif
#ifndef SKX_WIDE_ROUNDS
#define SKX_WIDE_ROUNDS 4
#endif
#ifndef SKX_WIDE_WPS
#define SKX_WIDE_WPS 4
#endif
#ifndef SKX_WIDE_PPT
#define SKX_WIDE_PPT 16
#endif
#ifndef SKX_WIDE_PF
#define SKX_WIDE_PF 10
#endif
#if defined(SKX_PHASE_PROF) && SKX_PHASE_PROF == 3
#define WIDE_PROF(i) do { if (SCATTER) PHASE_PROF_(i); } while (0)
#else
#define WIDE_PROF(i) do { } while (0)
#endif
// WPPT window-end positions per thread (16, or 8: half a 16-base chunk each -- 40 instead of 80 registers of payload)
#ifndef SKX_WIDE_NT
#define SKX_WIDE_NT 512
#endif
constexpr int WPPT = SKX_WIDE_PPT, WNT = SKX_WIDE_NT, WTILE = WNT * WPPT, WROUNDS = SKX_WIDE_ROUNDS;
static_assert(WPPT == 8 || WPPT == 16, "8 or 16 positions per thread");
int extract_tile_bases_wide() { return WTILE; }

template <bool SCATTER>
__global__ __launch_bounds__(WNT, SKX_WIDE_WPS) void extract_wide_kernel(ExtractArgs a)
{
    constexpr int NCHUNK = WTILE / 16 + 5;
    constexpr uint32_t STAGE = (uint32_t)((WTILE + WROUNDS - 1) / WROUNDS);
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const int B = 1 << a.logB;
    uint32_t *s_hist = reinterpret_cast<uint32_t *>(s_raw);
    uint32_t *s_base = s_hist + B + 4;
    uint32_t *s_tmp = s_base + B;
    unsigned char *s_rest = reinterpret_cast<unsigned char *>(s_tmp + 20);
    uint32_t *s_code = reinterpret_cast<uint32_t *>(s_rest);
    uint16_t *s_bad = reinterpret_cast<uint16_t *>(s_code + NCHUNK + 3);
    uint16_t *s_nl = s_bad + NCHUNK + 3, *s_qbad = s_nl + NCHUNK + 3;
    u128 *s_stage = reinterpret_cast<u128 *>(s_rest);

    const int tid = threadIdx.x;
    PHASE_PROF_START;
    const uint64_t per_group = 8ull * (uint64_t)a.tiles_max;
    const uint64_t L = blockIdx.x;
    // workgroup L runs on XCD L % 8: a sample's tiles stay on one XCD, one after the other (its regions' lines are put together in ONE L2).  With
    // fewer than eight samples that would leave XCDs idle (one 100 Mbp sample: an eighth of the chip): then a sample's tiles are dealt to
    // `parts` XCDs in contiguous ranges
    int sample; uint64_t tile;
    if (a.parts > 1) {
        const int v = (int)(L & 7u);
        if (v >= a.n_samples * a.parts) return;
        sample = v / a.parts; tile = (uint64_t)(v % a.parts) * (uint64_t)a.tiles_part + (L >> 3);
        if (tile >= (uint64_t)a.tiles_max || (L >> 3) >= (uint64_t)a.tiles_part) return;
    } else { sample = (int)((L / per_group) * 8 + (L % per_group) % 8); tile = (L % per_group) / 8; }
    if (sample >= a.n_samples) return;
    const uint64_t len = a.lens[sample];
    const uint64_t T0 = tile * WTILE;
    if (T0 >= len) return;
    // record streams live in HBM: explicit global address space (a pointer fetched from memory is generic -> flat_load)
    typedef const uint8_t __attribute__((address_space(1))) *gbytes_t;
    gbytes_t seq = (gbytes_t)(uintptr_t)a.seqs[sample];
    gbytes_t qual = a.quals ? (gbytes_t)(uintptr_t)a.quals[sample] : (gbytes_t)0;

    for (int i = tid; i < B + 4; i += WNT) s_hist[i] = 0;
    for (int c = tid; c < NCHUNK; c += WNT) {
        const int64_t p = (int64_t)T0 - 64 + 16 * (int64_t)c;
        uint32_t w[4], q[4] = {0, 0, 0, 0};
        if (p >= 0 && (uint64_t)p + 16 <= len) {
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            typedef const u32x4 __attribute__((address_space(1))) *gvec_t;
            const u32x4 v = *(gvec_t)(seq + p);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
            if (qual) { const u32x4 u = *(gvec_t)(qual + p); q[0] = u.x; q[1] = u.y; q[2] = u.z; q[3] = u.w; }
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                uint32_t x = 0, y = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    int64_t pos = p + 4 * i + b;
                    bool in = pos >= 0 && (uint64_t)pos < len;
                    x |= (uint32_t)(in ? seq[pos] : (uint8_t)'\n') << (8 * b);
                    if (qual) y |= (uint32_t)(in ? qual[pos] : (uint8_t)'~') << (8 * b);
                }
                w[i] = x; q[i] = y;
            }
        }
        uint32_t code, bad, nl;
        pack16(w, code, bad, nl);
        uint32_t qb = 0;
        if (qual) { qb = qualbad16(q, a.min_qual) & ~nl; if (a.qual_filter == 2) bad |= qb; }
        s_code[c] = code; s_bad[c] = (uint16_t)bad; s_nl[c] = (uint16_t)nl; s_qbad[c] = (uint16_t)qb;
    }
    __syncthreads();
    WIDE_PROF(0);
    // as in extract_kernel: the text of a tile this XCD takes up shortly goes into its L2 now (one dword per 128-byte line)
    uint32_t pfw = 0;
    if (SCATTER && SKX_WIDE_PF && tid < WTILE / 128) {
        uint64_t pos = T0 + (uint64_t)SKX_WIDE_PF * WTILE + (uint64_t)tid * 128;
        gbytes_t ps = seq;
        uint64_t plen = len;
        if (T0 + (uint64_t)SKX_WIDE_PF * WTILE >= len && sample + 8 < a.n_samples) {
            pos = (tile + SKX_WIDE_PF - (len + WTILE - 1) / WTILE) * WTILE + (uint64_t)tid * 128;
            ps = (gbytes_t)(uintptr_t)a.seqs[sample + 8]; plen = a.lens[sample + 8];
        }
        if (pos + 4 <= plen) pfw = *(const uint32_t __attribute__((address_space(1))) *)(ps + pos);       // (never a byte beyond the stream)
    }

    const int k = a.k, h = (k - 1) / 2;
    const int c = (WPPT == 16 ? tid : tid >> 1) + 4;                      // my 16-base chunk; WPPT 8: its first or second half
    const int half8 = WPPT == 16 ? 0 : (tid & 1) * 8;
    // 80-bit fields: bit i <-> position p0 - 64 + i
    u128 bad80 = 0, qb80 = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) { bad80 |= (u128)s_bad[c - 4 + i] << (16 * i); qb80 |= (u128)s_qbad[c - 4 + i] << (16 * i); }
    const u128 G = ~bad80 & ((((u128)1) << 80) - 1);
    u128 Wk = ~(u128)0;
    {
        u128 A = G; int offset = 0, span = 1;
        for (int bit = 0; bit < 6; bit++) {
            if ((k >> bit) & 1) { Wk &= A << offset; offset += span; }
            A &= A << span; span <<= 1;
        }
    }
    const u128 NL = ((u128)s_nl[c] << 64) | ((u128)(s_nl[c + 1] & 1u) << 80);
    const u128 exact = Wk & ~(G << k);
    u128 V = Wk & ~(exact & (NL >> 1));
    if (qual && a.qual_filter != 0) V &= ~(qb80 << h);
    const uint32_t vm = ((uint32_t)(V >> 64) & 0xFFFFu) >> half8;
    const uint32_t cw = s_code[c] << (2 * half8);                              // my positions' bases, first one most significant

    const uint64_t am = (1ull << (2 * h)) - 1;                                 // arm mask (h <= 31)
    u128 prev = ((u128)s_code[c - 4] << 96) | ((u128)s_code[c - 3] << 64) | ((u128)s_code[c - 2] << 32) | s_code[c - 1];
    if (half8) prev = (prev << 16) | (s_code[c] >> 16);                        // the 64 bases before the chunk's second half
    uint64_t lower = (uint64_t)prev & am;
    uint32_t mid = (uint32_t)(prev >> (2 * h)) & 3u;
    uint64_t upper = (uint64_t)(prev >> (2 * h + 2)) & am;
    uint64_t rc_upper = revcomp_arm64(lower, h), rc_lower = revcomp_arm64(upper, h);
    uint32_t rc_mid = mid ^ 2u;
    const int hb = a.wh.hb;
    const int bshift = a.wh.bits - a.logB;
    const bool userc = a.rc != 0;
    // the packed word (H << 4) | mask on 64-bit halves, H = hl : hr with hb (32..62) bits each.  hl's place starts at bit sh = hb + 4
    // (36..66); one formula for both sides of 64, from wave-uniform shift counts: hl's part of the low half = (hl << a1) & m1, of the
    // high half = (hl >> a2) << a3.  (As u128 expressions the shifts by run-time counts were a third of the loop's instructions.)
    const int sh = hb + 4;
    const int a1 = sh < 64 ? sh : 0, a2 = sh < 64 ? 64 - sh : 0, a3 = sh < 64 ? 0 : sh - 64;
    const uint64_t m1 = sh < 64 ? ~0ull : 0ull;
    const int top_shift = hb - a.logB;                                         // bucket = the top logB bits of hl (hb >= 32 > logB)

    u128 wv[WPPT];
    uint32_t rk[WPPT];
#pragma unroll
    for (int j = 0; j < WPPT; j++) {
        const uint32_t code = (cw >> (30 - 2 * j)) & 3u;
        upper = ((upper << 2) | mid) & am;
        mid = (uint32_t)(lower >> (2 * h - 2));
        lower = ((lower << 2) | code) & am;
        rc_lower = (rc_lower >> 2) | ((uint64_t)rc_mid << (2 * h - 2));
        rc_mid = mid ^ 2u;
        rc_upper = (rc_upper >> 2) | ((uint64_t)(code ^ 2u) << (2 * h - 2));
        const bool ueq = upper == rc_upper;                                    // (no branches: the ?: form compiled into divergent control flow per window)
        const bool gt = userc & ((upper > rc_upper) | (ueq & (lower > rc_lower)));
        const bool eq = userc & ueq & (lower == rc_lower);
        uint64_t hl = gt ? rc_upper : upper, hr = gt ? rc_lower : lower;
        const uint32_t m4 = (1u << (gt ? rc_mid : mid)) | (eq ? (1u << rc_mid) : 0u);
        hmix_halves_w(hl, hr, a.wh);
        uint64_t wlo = (hr << 4) | m4 | ((hl << a1) & m1), whi = (hr >> 60) | ((hl >> a2) << a3);
        asm volatile("" : "+v"(wlo), "+v"(whi));                              // the word exists from here on (left alone, its last steps sink into the staging rounds and what they read stays live: 476 B of scratch)
        wv[j] = ((u128)whi << 64) | wlo;
        const bool valid = (vm >> j) & 1u;
        const uint32_t bk = valid ? (uint32_t)(hl >> top_shift) : (uint32_t)B;
        const uint32_t r = atomicAdd(&s_hist[bk], 1u);
        rk[j] = (bk << 16) | r;                                               // r <= WTILE < 65 536; no window = the dummy bucket B
    }
    __syncthreads();
    WIDE_PROF(1);
    uint32_t *ghist = a.hist + ((uint64_t)sample << a.logB);
    if (!SCATTER) {
        for (int i = tid; i < B; i += WNT) { uint32_t n = s_hist[i]; if (n) atomicAdd(&ghist[i], n); }
        return;
    }
    // one chunk per non-empty bucket reserved in the sample's region (global cursor).  Up to RW buckets per thread keep the returned
    // bases in registers, so the atomics stay in flight behind the block scan (parked in LDS each waits for its own round trip: the
    // cycle stamps had 14 % of a workgroup's time here)
    const int R = (B + WNT - 1) / WNT;
    const int b0 = tid * R < B ? tid * R : B, b1 = b0 + R < B ? b0 + R : B;
    constexpr int RW = 4;
    uint32_t gbw[RW], lsum = 0;
    if (R <= RW) {
#pragma unroll
        for (int r = 0; r < RW; r++) {
            gbw[r] = 0;
            if (b0 + r < b1) { const uint32_t n = s_hist[b0 + r]; if (n) gbw[r] = atomicAdd(&ghist[b0 + r], n); lsum += n; }
        }
    } else
        for (int b = b0; b < b1; b++) { const uint32_t n = s_hist[b]; s_base[b] = n ? atomicAdd(&ghist[b], n) : 0u; lsum += n; }
    uint32_t total;
    uint32_t lrun = block_excl_scan_row(lsum, s_tmp, &total, tid);
    // s_hist: counts -> local starts; s_base: where a staged word at index i goes, as a 32-bit word offset inside the sample's span of the
    // word buffer (region offset + chunk base - local start): the copy-out below adds i and stores -- no look-up in global memory between
    // two stores (a load behind a store waits for the store: loads, atomics and stores share one counter)
    const uint64_t *off = a.off + ((uint64_t)sample << a.logB);
    const bool fixed = a.capacity != 0xFFFFFFFFu;
    const uint64_t span0 = fixed ? ((uint64_t)sample << a.logB) * a.capacity : off[0];
    bool dropped = false;
    auto place = [&](int b, uint32_t gb) {
        const uint32_t n = s_hist[b];
        // a full region: the host falls back to exact offsets and builds every dictionary again, so the chunk only has to stay inside the
        // word buffer -- it goes to the head of the sample's span
        const bool over = n && gb + n > a.capacity;
        if (over) dropped = true;
        s_base[b] = over ? 0u - lrun : (fixed ? (uint32_t)b * a.capacity : (uint32_t)(off[b] - off[0])) + gb - lrun;
        s_hist[b] = lrun; lrun += n;
    };
    if (R <= RW) {
#pragma unroll
        for (int r = 0; r < RW; r++) if (b0 + r < b1) place(b0 + r, gbw[r]);
    } else
        for (int b = b0; b < b1; b++) place(b, s_base[b]);
    if (tid == 0) s_hist[B] = total;
    asm volatile("" :: "v"(pfw));
    __syncthreads();
    WIDE_PROF(2);
    typedef u128 __attribute__((address_space(1))) *gout_t;
    gout_t words = (gout_t)(uintptr_t)(reinterpret_cast<u128 *>(a.words) + span0);
    // where each of my words stands in the tile's bucket order (start of its bucket + its rank there); no window = beyond every round
#pragma unroll
    for (int j = 0; j < WPPT; j++) {
        const uint32_t b = rk[j] >> 16;
        rk[j] = b < (uint32_t)B ? s_hist[b] + (rk[j] & 0xFFFFu) : 0xFFFFFFFFu;
    }
    // the tile goes out in WROUNDS pieces of its bucket order, STAGE words each, through the staging buffer (a round is a range of staged
    // indices, not of buckets: every round is full, none can overflow, and a bucket's chunk is cut at most at a round's edge)
#pragma unroll 1
    for (uint32_t lo = 0; lo < total; lo += STAGE) {
#pragma unroll
        for (int j = 0; j < WPPT; j++) {
            uint32_t x = rk[j];
            asm volatile("" : "+v"(x));                     // taken apart here, every round (hoisted out of the round loop the pieces are spilled)
            x -= lo;
            if (x < STAGE) s_stage[x] = wv[j];
        }
        __syncthreads();
        const uint32_t n = total - lo < STAGE ? total - lo : STAGE;
        SketchRange skr = {0u, 0u};                          // the split sketch, as in extract_kernel
        if (a.sketch) skr = sketch_range(s_hist, lo, lo + n, a.logB, tid);
        for (uint32_t i = tid; i < n; i += WNT) {
            const u128 w = s_stage[i];
            const uint32_t b = wide_bucket(w, bshift);
            words[s_base[b] + lo + i] = w;
        }
        if (a.sketch) sketch_set(s_stage, skr, lo, a.logB, bshift + 4 - SKETCH_M, a.sketch, tid);      // (index bits: the hash bits below the bucket bits)
        if (lo + STAGE < total) __syncthreads();
        WIDE_PROF(3 + lo / STAGE);
    }
    if (dropped) *a.overflow = 1;
}
template <bool SCATTER>
static void launch_extract_wide(const ExtractArgs &a_, hipStream_t st)
{
    ExtractArgs a = a_;
    extract_parts(a);
    const uint64_t g = a.parts > 1 ? 8ull * (uint64_t)a.tiles_part : (((uint64_t)a.n_samples + 7) / 8) * 8ull * (uint64_t)a.tiles_max;
    if (!g) return;
    size_t codes = (size_t)(WTILE / 16 + 8) * 10 + 64;
    size_t stage = SCATTER ? (size_t)((WTILE + WROUNDS - 1) / WROUNDS) * 16 : 0;
    size_t lds = ((size_t)8 << a.logB) + 16 + 80 + (stage > codes ? stage : codes) + 16;
    (void)hipFuncSetAttribute((const void *)extract_wide_kernel<SCATTER>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(extract_wide_kernel<SCATTER>, dim3((unsigned)g), dim3(WNT), lds, st, a);
}
void launch_hist_wide(const ExtractArgs &a, hipStream_t st) { launch_extract_wide<false>(a, st); }
void launch_scatter_wide(const ExtractArgs &a, hipStream_t st) { launch_extract_wide<true>(a, st); }

// ---- dedupe (same algorithm as dedupe_mb_kernel) ----
template <int ITEMS, int NT>
__global__ __launch_bounds__(NT, NT == 1024 ? 8 : NT == 768 ? 6 : 4) void dedupe_wide_kernel(u128 *words, const uint64_t *off, const uint32_t *raw, uint32_t *ucnt, uint32_t cap,
                                                          int rem_bits, int *overflow, uint16_t *sidx, int sb)
{
    PHASE_PROF_START;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
    const uint64_t region = blockIdx.x;
    const uint32_t n = raw[region];
    if (n == 0) { if (threadIdx.x == 0) ucnt[region] = 0; return; }
    if (n > cap || n > (uint32_t)NT * ITEMS) { if (threadIdx.x == 0) { *overflow = 1; ucnt[region] = 0; } return; }
    u128 *s_elem = reinterpret_cast<u128 *>(s_mem);
    // one array for the micro-buckets, as in dedupe_mb_kernel: counts -> starts -> (after the scatter) ends, so that bucket m is
    // [s_cnt[m - 1], s_cnt[m]) with s_cnt[-1] = 0; ~1..2 words per micro-bucket
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_mem + (size_t)cap * 16) + 12;      // (two sentinel words behind the elements, then [-1])
    uint32_t *s_tmp = s_cnt + cap + 4;
    int logM = 31 - __clz(n);
    if (logM < 0) logM = 0;
    if (logM > rem_bits) logM = rem_bits;
    while ((1u << logM) > cap) logM--;
    const uint32_t M = 1u << logM;
    const int mshift = rem_bits - logM;
    auto mb_of = [&](u128 w) { return field_w(w, mshift + 4, M - 1); };      // the logM bits below the region's own (rem_bits + 4 and up are the region's)
    u128 *reg = words + off[region];
    u128 e[ITEMS];
#pragma unroll
    for (int t = 0; t < ITEMS; t++) { const uint32_t i = threadIdx.x + (uint32_t)NT * t; e[t] = i < n ? reg[i] : (u128)0; }
    for (uint32_t i = threadIdx.x; i < M; i += NT) s_cnt[i] = 0;
    if (threadIdx.x == 0) s_cnt[-1] = 0;
    if (threadIdx.x < 2) s_elem[n + threadIdx.x] = ~(u128)0;                 // what the ranking reads behind the last word
    __syncthreads();
    DW_PROF(0);
#pragma unroll
    for (int t = 0; t < ITEMS; t++) if (e[t]) atomicAdd(&s_cnt[mb_of(e[t])], 1u);
    __syncthreads();
    DW_PROF(1);
    const uint32_t R = (M + NT - 1) / NT;
    const uint32_t m0 = threadIdx.x * R < M ? threadIdx.x * R : M, m1 = m0 + R < M ? m0 + R : M;
    uint32_t sum = 0;
    for (uint32_t m = m0; m < m1; m++) sum += s_cnt[m];
    uint32_t run = block_excl_scan_row(sum, s_tmp, nullptr, (int)threadIdx.x);
    for (uint32_t m = m0; m < m1; m++) { uint32_t c = s_cnt[m]; s_cnt[m] = run; run += c; }
    __syncthreads();
    DW_PROF(2);
#pragma unroll
    for (int t = 0; t < ITEMS; t++) if (e[t]) s_elem[atomicAdd(&s_cnt[mb_of(e[t])], 1u)] = e[t];
    __syncthreads();
    DW_PROF(3);
    // rank inside the micro-bucket; the dependent LDS reads (word, bucket bounds) are issued for all of the
    // thread's words stage by stage
    uint32_t npos[ITEMS], bb[ITEMS], ee[ITEMS];
#pragma unroll
    for (int t = 0; t < ITEMS; t++) { const uint32_t p = threadIdx.x + (uint32_t)NT * t; e[t] = s_elem[p < n ? p : n - 1]; }
#pragma unroll
    for (int t = 0; t < ITEMS; t++) { const uint32_t m = mb_of(e[t]); bb[t] = s_cnt[(int)m - 1]; ee[t] = s_cnt[m]; }
#pragma unroll
    for (int t = 0; t < ITEMS; t++) {
        const uint32_t p = threadIdx.x + (uint32_t)NT * t;
        npos[t] = 0;
        if (p >= n) { e[t] = 0; continue; }
        // as dedupe_mb_kernel: the bucket's first NS slots are read and compared without a test of the bucket's end -- a slot behind
        // it holds a word of a later bucket (larger, never this key) or one of the sentinels behind the region's last word -- so the
        // common case (1-2 words per bucket) is straight-line code with its LDS reads in flight together; longer buckets finish in a
        // loop, and only a key that occurs again (rare in an assembly) orders its copies and folds their base masks
        const u128 w0 = e[t], w0lo = w0 & ~(u128)15;
        const uint32_t b = bb[t], eend = ee[t];
        constexpr uint32_t NS = 3;
        u128 wq[NS];
#pragma unroll
        for (uint32_t u = 0; u < NS; u++) wq[u] = s_elem[b + u];
        uint32_t less = 0, same = 0;
#pragma unroll
        for (uint32_t u = 0; u < NS; u++) { less += wq[u] < w0lo ? 1u : 0u; same += same_key_w(wq[u], w0) ? 1u : 0u; }
        bool dup = same > (p - b < NS ? 1u : 0u);
        for (uint32_t j = b + NS; j < eend; j++) {
            const u128 w = s_elem[j];
            less += w < w0lo ? 1u : 0u;
            dup |= j != p && same_key_w(w, w0);
        }
        uint32_t eqb = 0, mor = (uint32_t)w0 & 15u;
        if (dup)
            for (uint32_t j = b; j < eend; j++) {
                const u128 w = s_elem[j];
                const bool iseq = same_key_w(w, w0);
                eqb += iseq && j < p;
                mor |= iseq ? (uint32_t)w & 15u : 0u;
            }
        npos[t] = b + less + eqb;
        e[t] = w0lo | mor;
    }
    __syncthreads();
    DW_PROF(4);
#pragma unroll
    for (int t = 0; t < ITEMS; t++) if (e[t]) s_elem[npos[t]] = e[t];
    __syncthreads();
    DW_PROF(5);
    constexpr int NW = NT / 64;
    uint32_t *s_rows = s_cnt;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t flags = 0, sflags = 0, below[ITEMS];
    const int subshift = rem_bits - sb + 4;                 // sub-range of a word = its next sb hash bits (see dedupe_mb_kernel)
#pragma unroll
    for (int t = 0; t < ITEMS; t++) {
        const uint32_t p = threadIdx.x + (uint32_t)NT * t;
        bool lead = false;
        if (p < n) {
            e[t] = s_elem[p];
            const u128 x = p ? s_elem[p - 1] ^ e[t] : ~(u128)0;
            lead = differ_from_w(x, 4);
            if (differ_from_w(x, subshift)) sflags |= 1u << t;
        }
        const unsigned long long bal = __ballot(lead);
        below[t] = __popcll(bal & ((1ull << lane) - 1ull));
        if (lead) flags |= 1u << t;
        if (lane == 0) s_rows[t * NW + wv] = __popcll(bal);
    }
    __syncthreads();
    DW_PROF(6);
    uint32_t base = 0;
#pragma unroll
    for (int t = 0; t < ITEMS; t++) {
        uint32_t rowsum = 0, before = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) { const uint32_t c = s_rows[t * NW + w]; before += w < wv ? c : 0u; rowsum += c; }
        if ((flags >> t) & 1u) reg[base + before + below[t]] = e[t];
        if ((sflags >> t) & 1u) sidx[region * SUBIDX + field_w(e[t], subshift, (1u << sb) - 1)] = (uint16_t)(base + before + below[t]);
        base += rowsum;
    }
    if (threadIdx.x == 0) ucnt[region] = base;
    DW_PROF(7);
}
template <int ITEMS, int NT>
static void launch_dedupe_wide_items(u128 *words, const uint64_t *off, const uint32_t *raw, uint32_t *ucnt, uint64_t n_regions, uint32_t cap,
                                     int rem_bits, int *overflow, uint16_t *sidx, int sb, size_t lds, hipStream_t st)
{
    (void)hipFuncSetAttribute((const void *)dedupe_wide_kernel<ITEMS, NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((dedupe_wide_kernel<ITEMS, NT>), dim3((unsigned)n_regions), dim3(NT), lds, st, words, off, raw, ucnt, cap, rem_bits, overflow, sidx, sb);
}
void launch_dedupe_wide(u128 *words, const uint64_t *off, const uint32_t *raw, uint32_t *ucnt, uint64_t n_regions, uint32_t cap, int rem_bits,
                        int *overflow, uint16_t *sidx, int sb, hipStream_t st)
{
    if (!n_regions) return;
    size_t lds = (size_t)cap * 16 + (size_t)cap * 4 + 64 + 96;
    // latency-bound like the 64-bit kernel: 1 024 threads with <= 4 words each (the 20 B of LDS per word allow two regions per
    // CU, so this is what fills the wave slots); the host keeps wide regions <= 4 096 words
    // 5 Mbp samples have ~2 440-word regions (capacity 3 200): 768 threads x <= 5 words, 24 waves per CU, sort them 3 % faster than 1 024 x <= 4
    // (19.6 against 20.25 ms per 500 genomes; 512 x <= 7 is slower, 1 024 x <= 3 the same: profiles/r03zv_ab_wide_dedupe_shape.log)
    const int shape = 2;
    if (cap <= 2048) launch_dedupe_wide_items<4, 512>(words, off, raw, ucnt, n_regions, cap, rem_bits, overflow, sidx, sb, lds, st);
    else if (shape == 1 && cap <= 3584) launch_dedupe_wide_items<7, 512>(words, off, raw, ucnt, n_regions, cap, rem_bits, overflow, sidx, sb, lds, st);
    else if (shape == 2 && cap <= 3840) launch_dedupe_wide_items<5, 768>(words, off, raw, ucnt, n_regions, cap, rem_bits, overflow, sidx, sb, lds, st);
    else if (shape == 3 && cap <= 3072) launch_dedupe_wide_items<3, 1024>(words, off, raw, ucnt, n_regions, cap, rem_bits, overflow, sidx, sb, lds, st);
    else launch_dedupe_wide_items<4, 1024>(words, off, raw, ucnt, n_regions, cap, rem_bits, overflow, sidx, sb, lds, st);
}

// ---- union: order-preserving LDS table with 16-byte entries.  There is no 128-bit LDS CAS, so a slot is claimed by a
// 64-bit CAS of its low word to a LOCK value, the high word is written, then the low word is published; a lane that
// sees LOCK simply retries in its next loop iteration (every iteration is straight-line, so the owner always finishes).
__device__ static inline uint32_t home_slot_w(u128 w, int rem_bits, uint32_t nslots)
{
    uint32_t l32;                                          // the top 32 bits of the key's rem_bits local bits (left-aligned when there are fewer)
    if (rem_bits >= 32) l32 = field_w(w, rem_bits + 4 - 32, 0xFFFFFFFFu);
    else l32 = rem_bits == 0 ? 0u : (((uint32_t)((uint64_t)w >> 4)) & ((1u << rem_bits) - 1u)) << (32 - rem_bits);
    return (uint32_t)(((uint64_t)l32 * nslots) >> 32);
}
// A slot is two adjacent 64-bit words (low, high).  Every packed word carries a non-zero base mask in its low nibble, so a low
// word of 0 (empty) or WLOCK (claimed, high word on its way) can never be a key's: no separate state array, and one 128-bit
// LDS read shows a whole slot.
#define WLOCK 16ull
__device__ static inline bool table_insert_w(unsigned long long *tab, uint32_t total_slots, uint32_t home, u128 w)
{
    const unsigned long long wlo = (unsigned long long)w, whi = (unsigned long long)(w >> 64);
    uint32_t i = home;
    for (int guard = 0; guard < (1 << 22); guard++) {
        if (i >= total_slots) return false;
        unsigned long long old = reinterpret_cast<volatile unsigned long long *>(tab)[2 * i];
        if (old == 0ull) old = atomicCAS(&tab[2 * i], 0ull, WLOCK);
        if (old == 0ull) {                                  // claimed: high word first, the low word publishes the slot
            reinterpret_cast<volatile unsigned long long *>(tab)[2 * i + 1] = whi;
            __threadfence_block();
            atomicExch(&tab[2 * i], wlo);
            return true;
        }
        if (old == WLOCK) continue;                         // being written: look again (the owner's path is straight-line)
        if (((old ^ wlo) >> 4) == 0ull && reinterpret_cast<volatile unsigned long long *>(tab)[2 * i + 1] == whi) {
            if ((old | wlo) != old) atomicOr(&tab[2 * i], wlo & 15ull);
            return true;
        }
        i++;
    }
    return false;
}
// as table_insert_w, reporting where the key lives: 0 = table full, 1 = the key was there, 2 = this call put it there
__device__ static inline int table_insert_slot_w(unsigned long long *tab, uint32_t total_slots, uint32_t home, u128 w, uint32_t &slot)
{
    const unsigned long long wlo = (unsigned long long)w, whi = (unsigned long long)(w >> 64);
    uint32_t i = home;
    for (int guard = 0; guard < (1 << 22); guard++) {
        if (i >= total_slots) return 0;
        unsigned long long old = reinterpret_cast<volatile unsigned long long *>(tab)[2 * i];
        if (old == 0ull) old = atomicCAS(&tab[2 * i], 0ull, WLOCK);
        if (old == 0ull) {
            reinterpret_cast<volatile unsigned long long *>(tab)[2 * i + 1] = whi;
            __threadfence_block();
            atomicExch(&tab[2 * i], wlo);
            slot = i; return 2;
        }
        if (old == WLOCK) continue;
        if (((old ^ wlo) >> 4) == 0ull && reinterpret_cast<volatile unsigned long long *>(tab)[2 * i + 1] == whi) {
            if ((old | wlo) != old) atomicOr(&tab[2 * i], wlo & 15ull);
            slot = i; return 1;
        }
        i++;
    }
    return 0;
}
__device__ static inline uint32_t lower_bound_wide(const u128 *reg, uint32_t n, u128 x)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) { uint32_t mid = (lo + hi) >> 1; if ((reg[mid] >> 4) < x) lo = mid + 1; else hi = mid; }
    return lo;
}
__device__ static inline uint32_t lower_bound_wide_range(const u128 *reg, uint32_t lo, uint32_t hi, u128 x)
{
    while (lo < hi) { uint32_t mid = (lo + hi) >> 1; if ((reg[mid] >> 4) < x) lo = mid + 1; else hi = mid; }
    return lo;
}
__device__ static inline void sub_slice_w(const DictView &d, int sample, uint64_t j, int logN, const u128 *&reg, uint32_t &lo, uint32_t &hi)
{
    const int sh = logN - d.logB;
    const uint64_t b = j >> sh;
    const uint64_t region = ((uint64_t)sample << d.logB) + b;
    reg = reinterpret_cast<const u128 *>(d.words) + d.off[region];
    const uint32_t n = d.ucnt[region];
    if (sh == 0) { lo = 0; hi = n; return; }
    const uint32_t jj = (uint32_t)(j & ((1ull << sh) - 1)), last = (1u << sh) - 1;
    const int rb = d.bits - logN;
    const u128 xlo = (u128)j << rb, xhi = (u128)(j + 1) << rb;
    if (d.sidx) {                                             // the region's sub-index (see sub_slice in skx_device.hip)
        const uint16_t *ix = d.sidx + region * SUBIDX;
        auto start_of = [&](uint32_t a) -> uint32_t {
            for (; a < (1u << d.sb); a++) { const uint32_t v = ix[a]; if (v != 0xFFFFu) return v; }
            return n;
        };
        if (sh <= d.sb) {
            lo = start_of(jj << (d.sb - sh));
            hi = jj == last ? n : start_of((jj + 1) << (d.sb - sh));
            return;
        }
        if (d.sb > 0) {
            const uint32_t c = jj >> (sh - d.sb);
            const uint32_t a0 = start_of(c), a1 = start_of(c + 1);
            lo = lower_bound_wide_range(reg, a0, a1, xlo);
            hi = ((jj + 1) & ((1u << (sh - d.sb)) - 1)) == 0 ? a1 : lower_bound_wide_range(reg, lo, a1, xhi);
            return;
        }
    }
    lo = lower_bound_wide(reg, n, xlo);
    hi = jj == last ? n : lower_bound_wide(reg, n, xhi);
}

__device__ static inline uint64_t sub_slice_off_wide(const DictView &d, int sample, uint64_t j, int logN, uint32_t &lo, uint32_t &hi)
{
    const u128 *reg = nullptr;
    sub_slice_w(d, sample, j, logN, reg, lo, hi);
    return (uint64_t)(reg - reinterpret_cast<const u128 *>(d.words));
}

#ifndef SKX_UNIONW_U
#define SKX_UNIONW_U 4
#endif
// SIDE: as union_kernel<.., SIDE> -- the pass also leaves side[word index] = (first-seen rank of the key in its sub-bucket << 4) | base set for
// every word of every dictionary and perm[rank] = sorted row per sub-bucket; assemble_side_kernel<true> fills the matrix from those
template <bool COUNT_ONLY, bool SIDE>
__global__ __launch_bounds__(1024, 8) void union_wide_kernel(DictView d, int logN, u128 *stage, uint32_t stride, uint32_t *ncnt, uint32_t nslots,
                                                             int *overflow, uint16_t *side, uint16_t *perm)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
    __shared__ uint32_t s_tmp[17];
    __shared__ int s_fail;
    __shared__ uint32_t s_nrows;
    const uint64_t j = blockIdx.x;
    const uint32_t total_slots = nslots + TABLE_PAD;
    unsigned long long *tab = reinterpret_cast<unsigned long long *>(s_mem);          // [total_slots + 1][2]: one spare slot for the successor read
    uint16_t *s_rank = reinterpret_cast<uint16_t *>(tab + 2 * (total_slots + 1));     // SIDE: [total_slots + 1] first-seen rank of the key in each slot
    for (uint32_t i = threadIdx.x; i < 2 * (total_slots + 1); i += blockDim.x) tab[i] = 0ull;
    if (SIDE) for (uint32_t i = threadIdx.x; i < total_slots + 1; i += blockDim.x) s_rank[i] = 0xFFFFu;
    if (threadIdx.x == 0) { s_fail = 0; s_nrows = 0; }
    __syncthreads();
    typedef uint16_t __attribute__((address_space(1))) *gside_t;
    gside_t gside = (gside_t)(uintptr_t)side;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int rem_bits = d.bits - logN;
    const int per_wave = (d.n_samples + nw - 1) / nw;              // samples are dealt evenly to the waves
    const int wend = (wv + 1) * per_wave < d.n_samples ? (wv + 1) * per_wave : d.n_samples;
    constexpr int UU = SKX_UNIONW_U;
    for (int s0 = wv * per_wave; s0 < wend; s0 += 64) {
        const u128 *my_reg = nullptr; uint32_t my_lo = 0, my_hi = 0;
        const int cnt = wend - s0 < 64 ? wend - s0 : 64;
        if (lane < cnt) sub_slice_w(d, s0 + lane, j, logN, my_reg, my_lo, my_hi);
        // as union_kernel: a batch of UU words per lane is looked up with independent 128-bit LDS reads (home slot and its
        // successor); only first sightings, new bases and keys displaced further take the insert loop, re-read from global memory
        auto absorb = [&](const u128 (&q)[UU], const u128 *reg, uint32_t first) {
            uint32_t miss = 0;
            const uint64_t sbase = SIDE ? (uint64_t)(reg - reinterpret_cast<const u128 *>(d.words)) + first + lane : 0;   // this lane's first word in the side array
#pragma unroll
            for (int g = 0; g < UU; g += 2) {
                ulonglong2 a[2], b[2]; uint32_t hsl[2];
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    if (g + u >= UU) continue;
                    const uint32_t hs = home_slot_w(q[g + u], rem_bits, nslots);
                    a[u] = *reinterpret_cast<const ulonglong2 *>(tab + 2 * hs); b[u] = *reinterpret_cast<const ulonglong2 *>(tab + 2 * hs + 2); hsl[u] = hs;
                }
                uint32_t rkq[2];
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    if (g + u >= UU) continue;
                    const unsigned long long wlo = (unsigned long long)q[g + u], whi = (unsigned long long)(q[g + u] >> 64);
                    const bool at0 = ((a[u].x ^ wlo) >> 4) == 0ull && a[u].y == whi;
                    const unsigned long long at = at0 ? a[u].x
                                                : (a[u].x != 0ull && ((b[u].x ^ wlo) >> 4) == 0ull && b[u].y == whi) ? b[u].x : 0ull;
                    if (wlo && (wlo & 15ull & ~at) != 0ull) miss |= 1u << (g + u);
                    if (SIDE) rkq[u] = s_rank[hsl[u] + (at0 ? 0u : 1u)];
                }
                if (SIDE) {
#pragma unroll
                    for (int u = 0; u < 2; u++) {
                        if (g + u >= UU) continue;
                        const uint32_t wl = (uint32_t)q[g + u];
                        if (!((unsigned long long)q[g + u]) || ((miss >> (g + u)) & 1u)) continue;
                        if (rkq[u] == 0xFFFFu) { miss |= 1u << (g + u); continue; }       // the key is there, its rank is still being written
                        gside[sbase + 64u * (g + u)] = (uint16_t)((rkq[u] << 4) | (wl & 15u));
                    }
                }
            }
            while (miss) {
                const int u = __ffs(miss) - 1; miss &= miss - 1;
                const u128 w = reg[first + 64u * u + lane];
                if (!SIDE) { if (!table_insert_w(tab, total_slots, home_slot_w(w, rem_bits, nslots), w)) s_fail = 1; }
                else {
                    uint32_t sl = 0;
                    const int res = table_insert_slot_w(tab, total_slots, home_slot_w(w, rem_bits, nslots), w, sl);
                    if (res == 0) { s_fail = 1; continue; }
                    // (the writers of a wave first, then its waiters: see union_kernel)
                    uint32_t r = 0xFFFFu;
                    if (res == 2) { r = atomicAdd(&s_nrows, 1u); reinterpret_cast<volatile uint16_t *>(s_rank)[sl] = (uint16_t)r; }
                    __builtin_amdgcn_wave_barrier();
                    if (res == 1) {
                        for (int it = 0; it < (1 << 16) && r == 0xFFFFu; it++) r = reinterpret_cast<volatile uint16_t *>(s_rank)[sl];
                        if (r == 0xFFFFu) s_fail = 1;
                    }
                    gside[sbase + 64u * u] = (uint16_t)((r << 4) | ((uint32_t)w & 15u));
                }
            }
        };
        for (int t = 0; t < cnt; t++) {
            const u128 *reg = reinterpret_cast<const u128 *>(__shfl((unsigned long long)my_reg, t, 64));
            const uint32_t lo = __shfl(my_lo, t, 64), hi = __shfl(my_hi, t, 64);
            for (uint32_t o = lo; o < hi; o += 64u * UU) {
                u128 cur[UU];
#pragma unroll
                for (int u = 0; u < UU; u++) { const uint32_t i = o + 64u * u + lane; cur[u] = i < hi ? reg[i] : (u128)0; }
                absorb(cur, reg, o);
            }
        }
    }
    __syncthreads();
    if (s_fail) { if (threadIdx.x == 0) *overflow = 1; return; }
    // sorted emit: runs of occupied slots are sorted independently (same argument as table_emit_sorted)
    const uint32_t per = (total_slots + blockDim.x - 1) / blockDim.x;
    const uint32_t lo = threadIdx.x * per < total_slots ? threadIdx.x * per : total_slots;
    const uint32_t hi = lo + per < total_slots ? lo + per : total_slots;
    uint32_t cnt = 0;
    for (uint32_t i = lo; i < hi; i++) cnt += tab[2 * i] != 0ull;
    uint32_t total;
    uint32_t c = block_excl_scan(cnt, s_tmp, &total);
    if (COUNT_ONLY) { if (threadIdx.x == 0) atomicAdd(ncnt, total); return; }
    u128 *slab = stage + j * (uint64_t)stride;
    auto slot = [&](uint32_t q) { return ((u128)tab[2 * q + 1] << 64) | tab[2 * q]; };
    for (uint32_t i = lo; i < hi; i++) {
        if (!tab[2 * i]) continue;
        const u128 w = slot(i);
        uint32_t gl = 0, lr = 0;
        for (int64_t q = (int64_t)i - 1; q >= 0 && tab[2 * q]; q--) gl += (slot((uint32_t)q) >> 4) > (w >> 4);
        for (uint32_t q = i + 1; q < total_slots && tab[2 * q]; q++) lr += (slot(q) >> 4) < (w >> 4);
        const uint32_t idx = c - gl + lr;
        if (idx < stride) {
            slab[idx] = (w & ~(u128)15) | 1;
            if (SIDE) { const uint32_t r = s_rank[i]; if (r < stride) perm[j * (uint64_t)stride + r] = (uint16_t)idx; }
        }
        c++;
    }
    if (threadIdx.x == 0) { ncnt[j] = total; if (total > stride || (SIDE && total > 4095u)) *overflow = 1; }
}
void launch_union_wide(const DictView &d, int logN, u128 *stage, uint32_t stride, uint32_t *ncnt, uint32_t table_slots, int *overflow,
                       hipStream_t st)
{
    size_t lds = (size_t)(table_slots + TABLE_PAD + 1) * 16;
    (void)hipFuncSetAttribute((const void *)union_wide_kernel<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((union_wide_kernel<false, false>), dim3(1u << logN), dim3(1024), lds, st, d, logN, stage, stride, ncnt, table_slots, overflow, (uint16_t *)nullptr, (uint16_t *)nullptr);
}
void launch_union_side_wide(const DictView &d, int logN, u128 *stage, uint32_t stride, uint32_t *ncnt, uint32_t table_slots, int *overflow,
                            uint16_t *side, uint16_t *perm, hipStream_t st)
{
    size_t lds = (size_t)(table_slots + TABLE_PAD + 1) * 18;
    (void)hipFuncSetAttribute((const void *)union_wide_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((union_wide_kernel<false, true>), dim3(1u << logN), dim3(1024), lds, st, d, logN, stage, stride, ncnt, table_slots, overflow, side, perm);
}
void launch_union_probe_wide(const DictView &d, int logP, int probe, uint32_t *cnt, uint32_t table_slots, int *overflow, hipStream_t st)
{
    size_t lds = (size_t)(table_slots + TABLE_PAD + 1) * 16;
    (void)hipFuncSetAttribute((const void *)union_wide_kernel<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((union_wide_kernel<true, false>), dim3((unsigned)probe), dim3(1024), lds, st, d, logP, (u128 *)nullptr, 0u, cnt, table_slots, overflow, (uint16_t *)nullptr, (uint16_t *)nullptr);
}

// ---- assemble ----
// as assemble_kernel (mode 0): the slab's keys in LDS with a direct index on their next hash bits (~2 rows per index cell), words
// looked up a batch per lane at a time with independent LDS reads
#ifndef SKX_ASMW_U
#define SKX_ASMW_U 4
#endif
// MODE as in assemble_kernel: 0 matrix + statistics (columns at roff[j] - col_base: a window of sub-buckets into a small buffer), 1 statistics
// only, 2 kept rows only (keep[] / kpos[] select the rows and give their columns)
template <int MODE>
__global__ __launch_bounds__(512, 4) void assemble_wide_kernel(AssembleArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const uint64_t j = (uint64_t)blockIdx.x + a.j_base;
    const uint32_t n = a.ncnt[j];
    if (n == 0) return;
    const uint32_t maxr = (a.max_rows + 15u) & ~15u;
    u128 *s_keys = reinterpret_cast<u128 *>(s_raw);                       // [maxr + 1]
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_raw + ((size_t)maxr + 1) * 16);
    uint16_t *s_map = reinterpret_cast<uint16_t *>(s_cnt);                // MODE 2: row -> kept slot (0xFFFF: dropped); no counts in that mode
    uint32_t *s_msk = s_cnt + maxr;
    uint32_t *s_idx = s_msk + maxr;                                       // [maxr/2 + 4] first row at or above each index cell
    unsigned char *s_rows = reinterpret_cast<unsigned char *>(s_idx + maxr / 2 + 4);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const u128 *slab = reinterpret_cast<const u128 *>(a.stage) + j * (uint64_t)a.stride;
    const uint64_t r0 = a.roff[j];
    const uint64_t k0 = MODE == 2 ? a.kpos[r0] : 0;
    const uint32_t nout = MODE == 2 ? (uint32_t)(a.kpos[r0 + n] - k0) : n;      // cells every sample writes for this sub-bucket
    if (MODE == 2 && nout == 0) return;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        s_keys[i] = slab[i] >> 4;
        if (MODE == 2) s_map[i] = a.keep[r0 + i] == 1 ? (uint16_t)(a.kpos[r0 + i] - k0) : (uint16_t)0xFFFF;
        else { s_cnt[i] = 0; s_msk[i] = 0; }
    }
    if (threadIdx.x == 0) s_keys[n] = ~(u128)0;
    __syncthreads();
    const int rem = a.d.bits - a.logN;                                    // key bits below the slab number
    int logI = 31 - __clz(n | 1u);
    if (logI > rem) logI = rem;
    while ((1u << logI) > maxr / 2) logI--;
    const uint32_t nidx = 1u << logI;
    const u128 kbase = rem >= 124 ? (u128)0 : ((u128)j << rem);           // every key of the slab starts with the slab number
    for (uint32_t b = threadIdx.x; b <= nidx; b += blockDim.x) {
        uint32_t l = 0, r = n;
        if (b == nidx) l = n;
        else { const u128 x = kbase | ((u128)b << (rem - logI)); while (l < r) { const uint32_t m = (l + r) >> 1; if (s_keys[m] < x) l = m + 1; else r = m; } }
        s_idx[b] = l;
    }
    __syncthreads();
    const int ish = rem - logI + 4;                                       // index cell of a packed word = (w >> ish) & (nidx - 1)
    const uint64_t ocol = MODE == 2 ? k0 : r0 - a.col_base;               // first output column of this sub-bucket
    const uint32_t shift = (uint32_t)(ocol & 15u);
    unsigned char *row = s_rows + (size_t)wv * (maxr + 32u);
    const int per = (a.d.n_samples + nw - 1) / nw;                 // samples are dealt evenly to the waves
    const int wend = (wv + 1) * per < a.d.n_samples ? (wv + 1) * per : a.d.n_samples;
    constexpr int AU = SKX_ASMW_U;
    auto place = [&](const u128 (&q)[AU]) {
#pragma unroll
        for (int h = 0; h < AU; h += 2) {
            uint32_t l[2], le[2]; u128 kk[2];
#pragma unroll
            for (int u = 0; u < 2; u++) {
                if (h + u >= AU) continue;
                const uint32_t ib = field_w(q[h + u], ish, nidx - 1);
                l[u] = s_idx[ib]; le[u] = s_idx[ib + 1];
            }
#pragma unroll
            for (int u = 0; u < 2; u++) { if (h + u >= AU) continue; kk[u] = s_keys[l[u]]; }
#pragma unroll
            for (int u = 0; u < 2; u++) {
                if (h + u >= AU) continue;
                const u128 w = q[h + u];
                if (!w) continue;
                const u128 key = w >> 4;
                uint32_t ll = l[u]; u128 k = kk[u];
                while (ll < le[u] && k < key) { ll++; k = s_keys[ll]; }
                if (ll < le[u] && k == key) {
                    const uint32_t m4 = (uint32_t)w & 15u;
                    if (MODE == 0) row[shift + ll] = mask2iupac(m4);
                    if (MODE == 2) { const uint32_t o = s_map[ll]; if (o != 0xFFFFu) row[shift + o] = (a.mask_ambig && (m4 & (m4 - 1))) ? (unsigned char)'N' : mask2iupac(m4); }
                    if (MODE != 2) {
                        const uint32_t single = (m4 & (m4 - 1)) == 0;
                        atomicAdd(&s_cnt[ll], 1u | (single << 16));
                        atomicOr(&s_msk[ll], 1u << m4);
                    }
                } else {
                    *a.missing = 1;
                }
            }
        }
    };
    for (int sbase = wv * per; sbase < wend; sbase += 64) {
        const u128 *my_reg = nullptr; uint32_t my_lo = 0, my_hi = 0;
        const int cnt = wend - sbase < 64 ? wend - sbase : 64;
        if (lane < cnt) sub_slice_w(a.d, sbase + lane, j, a.logN, my_reg, my_lo, my_hi);
        for (int t = 0; t < cnt; t++) {
            const int s = sbase + t;
            const u128 *reg = reinterpret_cast<const u128 *>(__shfl((unsigned long long)my_reg, t, 64));
            const uint32_t lo = __shfl(my_lo, t, 64), hi = __shfl(my_hi, t, 64);
            u128 cur[AU];
#pragma unroll
            for (int u = 0; u < AU; u++) { const uint32_t i = lo + 64u * u + lane; cur[u] = i < hi ? reg[i] : (u128)0; }      // loads in flight during the fill
            if (MODE != 1) {
                for (uint32_t i = lane * 4; i < nout + shift + 3; i += 256) *reinterpret_cast<uint32_t *>(row + i) = 0x2D2D2D2Du;
                __builtin_amdgcn_wave_barrier();
            }
            place(cur);
            for (uint32_t o = lo + 64u * AU; o < hi; o += 64u * AU) {
#pragma unroll
                for (int u = 0; u < AU; u++) { const uint32_t i = o + 64u * u + lane; cur[u] = i < hi ? reg[i] : (u128)0; }
                place(cur);
            }
            if (MODE != 1) {
                __builtin_amdgcn_wave_barrier();
                unsigned char *dst = a.matrix + (uint64_t)s * a.pitch + ocol;
                const uint32_t head = (16u - shift) & 15u;
                const uint32_t h = head < nout ? head : nout;
                if ((uint32_t)lane < h) dst[lane] = row[shift + lane];
                const uint32_t body = (nout - h) / 16u;
                for (uint32_t v = lane; v < body; v += 64) {
                    const uint4 x = *reinterpret_cast<const uint4 *>(row + shift + h + 16u * v);
                    *reinterpret_cast<uint4 *>(dst + h + 16u * v) = x;
                }
                const uint32_t done = h + body * 16u;
                if (done + lane < nout) dst[done + lane] = row[shift + done + lane];
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    if (MODE == 2) return;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        a.col_present[r0 + i] = s_cnt[i] & 0xFFFFu;
        a.col_unambig[r0 + i] = s_cnt[i] >> 16;
        a.col_mask[r0 + i] = s_msk[i];
    }
}
template <int MODE>
static void launch_assemble_wide_t(const AssembleArgs &a, uint32_t n_blocks, hipStream_t st)
{
    const uint32_t maxr = (a.max_rows + 15u) & ~15u;
    const int nw = 8;
    size_t lds = ((size_t)maxr + 1) * 16 + (size_t)maxr * 8 + ((size_t)maxr / 2 + 4) * 4 + (MODE == 1 ? 0 : (size_t)nw * (maxr + 32u));
    (void)hipFuncSetAttribute((const void *)assemble_wide_kernel<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(assemble_wide_kernel<MODE>, dim3(n_blocks), dim3(64 * nw), lds, st, a);
}
// sub-buckets [a.j_base, a.j_base + n_blocks); n_blocks = 0: all of them
void launch_assemble_wide(const AssembleArgs &a, hipStream_t st, int mode, uint32_t n_blocks)
{
    if (!n_blocks) n_blocks = (1u << a.logN) - a.j_base;
    if (mode == 0) launch_assemble_wide_t<0>(a, n_blocks, st); else if (mode == 1) launch_assemble_wide_t<1>(a, n_blocks, st); else launch_assemble_wide_t<2>(a, n_blocks, st);
}

__global__ void gather_keys_wide_kernel(const u128 *stage, uint32_t stride, const uint32_t *ncnt, const uint64_t *roff, u128 *out)
{
    const uint64_t j = blockIdx.x;
    const uint32_t n = ncnt[j];
    const u128 *slab = stage + j * (uint64_t)stride;
    u128 *dst = out + roff[j];
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) dst[i] = slab[i];
}
void launch_gather_keys_wide(const u128 *stage, uint32_t stride, const uint32_t *ncnt, const uint64_t *roff, int n_sub, u128 *out, hipStream_t st)
{
    hipLaunchKernelGGL(gather_keys_wide_kernel, dim3((unsigned)n_sub), dim3(256), 0, st, stage, stride, ncnt, roff, out);
}

}  // namespace skx
