// Y pass of the tiled path on the matrix cores (16-bit tiles, gfx950): y6_kernel's results from MFMAs.
//
//   ym_kernel :  tiles of (P unorm16 | Q snorm16) dwords  ->  LoG = -s^2 ( G''(y) P + G(y) Q )  + NMS entries, sparse store
//
// Why.  y6_kernel (mmx_fused.hip) forms every output with 2R + 1 packed VALU taps per lane: at R = 16 that is 34
// instructions per wave and row, ~190 cycles -- as long as the memory system needs to deliver the row -- and the two
// overlap only partly: removing the taps takes the kernel from 2.1 to 1.5 ms per 64 blocks (R = 20: 2.5 to 1.4;
// profiles/r03_y6_experiments.txt).  A 1-D convolution along y is a product with a banded Toeplitz matrix, and the
// bytes of the 16-bit tiles are exact float16 numbers, so the taps can run on v_mfma_f32_16x16x32_f16 instead.
//
// Layout.  A workgroup owns one (column tile c, z tile U) as in y6_kernel, each wave 4 planes x 16 columns of it = 64
// columns.  The MFMA wants 8 consecutive y per lane (k) and 16 columns per instruction (n), so a lane does not keep
// "its" column: lane (kgroup = l >> 4, n = l & 15) loads 16 bytes = 4 consecutive x of (row k0 + 8 kgroup + i, plane
// n >> 2, x quad n & 3) -- per k-group 256 contiguous bytes, the wave's quarter of the tile row -- and the four dwords
// of a lane are the same (k, n) element of FOUR B operands (x mod 4 picks the MFMA).  Each dword holds P (low half)
// and Q (high half); the four bytes become four float16 pieces with ONE byte permute each: a byte in the low half of a
// float16 is the subnormal b x 2^-24, which the matrix cores take exactly (tools/exp/mfma_denorm.hip: measured); the
// high byte of Q, two's complement, is flipped to offset binary and its 128 leaves through the accumulators' start
// value.  So
//     acc = sum_k  W2[k] (256 Phi + Plo) + W0[k] (256 Qhi + Qlo),      W = weight x tile scale x 2^e  (float16 range)
// is six MFMAs per (output tile of 16 rows, k-block of 32 rows, column set): Phi x 256 wh, Plo x wh, Phi x wl
// (wl = 256 (W - wh); the Plo x (W - wh) term, <= 2^-12 of 255 / 65535 of the sum, is dropped and counted in
// mmx_tiled_q16_error_bound), the same for Q.  The A operands are Toeplitz fragments w[|k - m + delta|] for the NB
// block offsets delta = RB - 16 t, t = 0 .. NB - 1, of a k-block that starts RB = 8 (NB - 2) rows before the first tile
// it feeds: NB = 3 / 4 / 5 offsets reach every tap of radius <= 8 / 16 / 24 (the next offset at either end starts
// 8 (NB - 2) + 1 rows away).  Built once per workgroup in LDS.  SciPy's "reflect" boundary is taken by the loads (rows
// mirrored, rows beyond reach clamped: zero weights).
// Two output tiles are complete after every k-block; their accumulators (four consecutive y per lane) go through LDS
// (4 KiB per wave and tile) to come back as one row of 64 columns per step, lane = column as in y6_kernel, whose
// ballot / sparse store / entry code then runs unchanged -- except that a tile with nothing above the threshold (a
// ballot over the accumulators) skips all of it and writes its sixteen zero entries with one store.
//
// The k-block loop, as the listing has it (profiles/r19_y_kblock_loop.txt): the block's 32 registers of rows become 64
// of pieces, the next block's rows are loaded into the 32 just freed -- always, also behind the last block, so that no
// path merges loaded and kept registers --, then the rows of the two tiles the previous block finished (their stores a
// whole MFMA phase ahead of the wait for those loads: one counter counts both), the MFMAs, the hand-off.  Nothing is
// copied: not the rows, not the accumulators on their way to LDS (each leaves as it is, the reader takes four rows of
// its column with one read), not the window.  What a wave keeps per lane across the loop is counted in registers it
// does not have (166 of 168 at NB = 4), so lane-dependent offsets that only rare paths want are made where they are
// used.  The entry of a decided row is written into its lane from the scalar side (four v_writelane_b32), the tests
// behind it are compares whose results are the wave's words already.

#include <type_traits>

#include <cstdlib>

#include "mmx_device.h"

struct ym_cfg {
    float w2[MMX_MAX_RADIUS_FAST + 1];      // G''(y) x (-norm) x (bound(P) / 65535) x 2^e: what a P count weighs
    float w0[MMX_MAX_RADIUS_FAST + 1];      // G(y) x (-norm) x (bound(Q) / 32767) x 2^e: what a Q count weighs
    float unscale;                          // 2^-e x 2^24 (the pieces are b x 2^-24)
    float start;                            // accumulators start here: minus what the 128 of Q's high byte adds
    float lo, eps;                          // nms_lo, nms_eps in accumulator units (/ unscale: a power of two, exact)
    int radius;
    int reverse;                            // 1: blockIdx.y = n - 1 takes the first block (the launch walks the batch backwards)
};

namespace {

// v with lane LN replaced by the wave-uniform s (v_writelane_b32 has no builtin in this compiler; the lane is an immediate)
template <int LN>
__device__ __forceinline__ unsigned ym_writelane(unsigned v, unsigned s)
{
    asm("v_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(s), "n"(LN));
    return v;
}

// where lane (kq = lane >> 4, n16 = lane & 15) puts its accumulator 0 in a hand-off slot, in units of 16 bytes:
// 64 kq + 4 n16 + (n16 >> 2) (see trw in the kernel)
__device__ __forceinline__ int ym_hput(int lane) { return (lane << 2) | ((lane >> 2) & 3); }

// Workgroup = four waves = one tile column.  NB <= 4 (R <= 16): 154 / 166 registers and 44 / 48 KiB of LDS, three workgroups
// per CU; NB == 5 (R <= 24): 182 registers and 52 KiB, two (held to 168 registers it spilled 20 and was slower: 2.10
// against 1.72 ms per 64 blocks).  Measured with six offsets (RB = 32, what R <= 24 took before the five-offset
// alignment was found: 1.99 ms) and kept as the YM6_* switches: pieces built for two column sets at a time -- 32
// registers less, the fragments read twice -- with TWELVE waves = three tile columns sharing one fragment table, i.e.
// three waves per SIMD too: 2.42 ms -- the LDS then carries as many cycles of fragment reads as the matrix pipe has
// MFMAs.
#ifndef YM5_OCC
#define YM5_OCC 2
#endif
#ifndef YM6_WAVES
#define YM6_WAVES 4
#define YM6_JH 4
#define YM6_NF 4
#endif
template <int NB, bool MASK>
__global__ void __launch_bounds__(NB <= 4 ? 256 : YM6_WAVES * 64, NB <= 4 ? 3 : (YM6_WAVES == 4 ? YM5_OCC : 1))
ym_kernel(const mmx_block* __restrict__ blocks, int64_t slot_elems, int64_t tile_stride,
          const unsigned* __restrict__ gt, float* __restrict__ out, ym_cfg cfg,
          unsigned long long* __restrict__ mask)
{
    constexpr int RB = 8 * (NB - 2);            // rows a k-block starts before the first output tile it feeds
    constexpr int NF = NB <= 4 ? 4 : YM6_NF;    // fragments per tile: [kernel: G'' (P), G (Q)][piece: wh, wl(, 256 wh)]
    __shared__ v4u frag[NB * NF * 64];         // (NF == 4: 256 wh is made from wh -- 16 KiB instead of 24: the third workgroup)
    constexpr int WAVES = NB <= 4 ? 4 : YM6_WAVES;     // per workgroup: WAVES / 4 tile columns
    constexpr int JH = NB <= 4 ? 4 : YM6_JH;           // column sets whose pieces are held at a time
    __shared__ float tr[WAVES * 2 * 1024];      // per wave: two finished tiles of 16 rows x 64 columns

    // (reverse: the Z+X kernel has just written the batch's P / Q tiles block after block; walking the batch from its
    //  last block back starts with the tiles written last -- what the 256 MiB memory-side cache still holds)
    const mmx_block bd = blocks[cfg.reverse ? gridDim.y - 1 - blockIdx.y : blockIdx.y];
    const int ntx = (bd.nx + 15) >> 4, ntz = (bd.nz + 15) >> 4;
    if ((int)blockIdx.x * (WAVES / 4) >= ntx * ntz) return;     // (the whole workgroup)
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tile = (int)blockIdx.x * (WAVES / 4) + (wv >> 2);
    const int c = tile / ntz, U = tile - c * ntz;
    const int zq = wv & 3;
    const bool live = tile < ntx * ntz && 16 * U + 4 * zq < bd.nz;     // (whole waves; the others leave behind the barrier)
    const int lane = threadIdx.x & 63;
    const int n = bd.ny;
    // ---- as a loader / MFMA operand holder: k-group kq, column index n16 (plane n16 >> 2, x quad n16 & 3)
    const int kq = lane >> 4, n16 = lane & 15;
    const unsigned trow_b = (unsigned)(ntx * ntz) * 1024u;      // bytes from one y to the next
    const rsrc_t rs = make_rsrc(gt + (int64_t)bd.slot * tile_stride + (int64_t)tile * 256);
    const unsigned voff = (unsigned)(zq * 256 + n16 * 16);
    const unsigned voff_s = voff + (unsigned)(8 * kq) * trow_b;  // blocks wholly inside the column: rows by scalar offset
    // k-blocks of 32 input rows: block b holds rows -RB + 32 b + [0, 32), lane row 8 kq + i.  A block past the column's
    // last takes the second form too: rows clamped into the column, whatever they hold
    v4u raw[8];
    auto load_block = [&](int b) __attribute__((always_inline)) {
        const int r0 = -RB + 32 * b;
        if (r0 >= 0 && r0 + 32 <= n) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                raw[i] = __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(rs, voff_s, (unsigned)(r0 + i) * trow_b, 0));
        } else {
            // (the lane's first row, 8 kq, made from the lane number here: the blocks at the column's ends are the
            //  only ones to want it, and kept for them across the loop it is a register too many -- scratch)
            int ln;
            asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
            const int k8 = (ln >> 1) & 24;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                int v = r0 + k8 + i;
                v = v < 0 ? -1 - v : v;
                v = v >= n ? 2 * n - 1 - v : v;
                v = v < 0 ? 0 : (v > n - 1 ? n - 1 : v);       // beyond the taps' reach: any row, zero weights
                raw[i] = __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(rs, voff + (unsigned)v * trow_b, 0, 0));
            }
        }
    };
    // the first block's rows are on their way while the fragment table is built
    if (live) load_block(0);
    // ---- Toeplitz fragments: A[m][k] = w[|k - m + delta_t|], lane = (m = l & 15, k = 8 (l >> 4) + i)
    for (int e = threadIdx.x; e < NB * NF * 64; e += WAVES * 64) {
        const int ln = e & 63, f = e >> 6;
        const int piece = (f % NF) % (NF / 2), kern = (f % NF) / (NF / 2), t = f / NF;
        const int m = ln & 15, kq = ln >> 4;
        const int delta = RB - 16 * t;
        unsigned pk[4];
#pragma unroll
        for (int i = 0; i < 8; i += 2) {
            float v[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                int d = 8 * kq + i + u - m + delta;
                d = d < 0 ? -d : d;
                const float ws = d <= cfg.radius ? (kern ? cfg.w0[d] : cfg.w2[d]) : 0.f;
                const float h = (float)(_Float16)ws;
                v[u] = piece == 0 ? h : (piece == 1 ? (ws - h) * 256.f : h * 256.f);
            }
            pk[i >> 1] = pack_h2(v[0], v[1]);
        }
        frag[e] = (v4u){pk[0], pk[1], pk[2], pk[3]};
    }
    __syncthreads();

    if (!live) return;                                          // (no barriers below)
    const float nms_lo = cfg.lo, nms_eps = cfg.eps, us = cfg.unscale;
    // ---- as a row worker (y6_kernel's lane): plane lane >> 4 of the quarter, column lane & 15
    const int xi = lane & 15;
    const int z = 16 * U + 4 * zq + (lane >> 4), x = 16 * c + xi;
    const bool real = z < bd.nz && x < bd.nx;
    float* w1 = out + (int64_t)bd.slot * slot_elems;
    const rsrc_t rsw = make_rsrc(w1);
    const unsigned ooff = (unsigned)((real ? z : 0) * bd.ny * bd.px + (real ? x : 0)) * 4u;
    const unsigned row_b = (unsigned)bd.px * 4u;
    // the entries of this wave's footprint (mmx_entries.h, MMX_MASK_QUADS).  The pending row's state and the candidate
    // tests stay written out in this kernel: through mmx_pending_row / mmx_candidate it compiles to other code
    // (profiles/r11_kernel_isa.txt), and it is 30 % of the headline step.
    const mmx_entry_geom eg = mmx_entry_geom_make(MMX_MASK_QUADS, bd.nz, bd.nx, bd.px);
    const int nent = eg.per_row;
    ulonglong2* mrow = MASK ? reinterpret_cast<ulonglong2*>(mask) + mmx_entry_base(bd.slot, slot_elems) +
                              mmx_quads_entry(eg, 4 * U + zq, 0) + c      // (its plane quad's first entry, then the tile)
                            : nullptr;
    unsigned long long ab_prev = 0;
    const bool has_l = xi > 0, has_r = xi < 15 && x + 1 < bd.nx;
    // (the same three as words of the wave, for tests taken as ballots)
    const unsigned long long realw = __builtin_amdgcn_ballot_w64(real), has_lw = __builtin_amdgcn_ballot_w64(has_l),
                             has_rw = __builtin_amdgcn_ballot_w64(has_r);
    float prev1 = -INFINITY, prev2 = -INFINITY, nbx_prev = -INFINITY;
    int ydone = 0;
    // the wave's two hand-off slots, in units of 16 bytes: four consecutive rows of one column -- an accumulator as the
    // MFMA leaves it -- at unit 64 g + (col ^ (col >> 4)), col = the row worker's lane, g = row >> 2.  The swizzle spreads
    // the sixteen lanes of a k-group (columns 4 n16 + j) over all banks; a row worker's sixteen columns stay a permutation
    v4f* trw = reinterpret_cast<v4f*>(tr + wv * 2048);
    // (accumulator j of lane (kq, n16) goes to unit ym_hput(lane) ^ j)
    const int hget = lane ^ (lane >> 4);                        // rows 4 g .. 4 g + 3 of this lane's column: unit 64 g + hget

    // the pending row's entry when it has no successor (the block's last row), or one that cannot beat it
    auto close_pending = [&]() __attribute__((always_inline)) {
        unsigned long long m = 0;
        if (ab_prev) {
            const bool cand = real & (prev1 > nms_lo) & !(fmaxf(prev2, nbx_prev) > prev1 + nms_eps);
            m = __ballot(cand);
        }
        if (lane == 0) *mrow = make_ulonglong2(m, ab_prev);
    };
    // one output row (y6_kernel's step after its taps; values and thresholds in accumulator units)
    auto row = [&](float acc, int y) __attribute__((always_inline)) {
        const unsigned long long ab = MASK ? mmx_above_word(real, acc, nms_lo) : ~0ull;
#ifndef YM_NOSTORE
        if (ab && real) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc * us), rsw, ooff, (unsigned)y * row_b, 0);
#endif
        if constexpr (MASK) {
            float nbx = -INFINITY;
            if (ab) {
                nbx = mmx_x_neighbours<false>(acc, has_l, has_r);
            }
            if (ydone > 0) {      // decide row ydone - 1, now that its successor is known
                unsigned long long m = 0;
                if (ab_prev) {
                    const bool cand = real & (prev1 > nms_lo) & !(fmaxf(fmaxf(prev2, acc), nbx_prev) > prev1 + nms_eps);
                    m = __ballot(cand);
                }
                if (lane == 0) *mrow = make_ulonglong2(m, ab_prev);
                mrow += nent;
            }
            prev2 = prev1; prev1 = acc; nbx_prev = nbx;
            ab_prev = ab;
            ++ydone;
        }
    };
    // the rows of one finished tile, out of LDS slot s; `any`: something of it is above the threshold
    auto rows_of = [&](int T, int s, bool any) __attribute__((always_inline)) {
        if (T < 0 || 16 * T >= n) return;
        const int cnt = n - 16 * T < 16 ? n - 16 * T : 16;
        if (MASK && !any) {
            // nothing above the threshold in 16 rows x 64 columns: a value below it neither is a candidate nor beats
            // one, so the pending row is decided as if its successor were -inf and the rest are zero entries
            if (ydone > 0) {
                close_pending();
                mrow += nent;
            }
            int ln = lane;                  // (the lane's entry offset is made here: kept for this path it spills)
            asm volatile("" : "+v"(ln));
            if (ln < cnt - 1) mrow[(int64_t)ln * nent] = make_ulonglong2(0ull, 0ull);
            mrow += (int64_t)(cnt - 1) * nent;
            prev1 = prev2 = nbx_prev = -INFINITY;
            ab_prev = 0;
            ydone += cnt;
            return;
        }
        const v4f* src = trw + s * 256 + hget;
        if constexpr (!MASK) {                     // every row stored: four at a time
#pragma unroll 1
            for (int g = 0; 4 * g < cnt; ++g) {
                const v4f q = src[g * 64];
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (4 * g + r < cnt) row(q[r], 16 * T + 4 * g + r);
            }
            return;
        }
        if (cnt < 16) {                            // (the column's last, partial tile: row by row)
            const float* src1 = reinterpret_cast<const float*>(src);
#pragma unroll 1
            for (int r = 0; r < cnt; ++r) row(src1[(r >> 2) * 256 + (r & 3)], 16 * T + r);
            return;
        }
        // A whole tile at once: all sixteen rows in registers, one ballot each; only rows with something above the
        // threshold cost more than that (store, x neighbours, candidate test), and the sixteen entries decided here
        // -- the pending row and rows 0 .. 14 -- leave in one store, lane i holding the entry of row 16 T - 1 + i.
        float v[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const v4f q = src[g * 64];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[4 * g + r] = q[r];
        }
        // entry = (cand lo, cand hi, above lo, above hi), written into its lane from the scalar side.  A row's
        // candidates are its lanes above the threshold -- its word `a` -- that no neighbour beats
        unsigned e0 = 0, e1 = 0, e2 = 0, e3 = 0;
        auto put = [&](auto LN, unsigned long long beaten, unsigned long long a) __attribute__((always_inline)) {
            constexpr int ln = decltype(LN)::value;
            const unsigned long long m = a & ~beaten;
            e0 = ym_writelane<ln>(e0, (unsigned)m);
            e1 = ym_writelane<ln>(e1, (unsigned)(m >> 32));
            e2 = ym_writelane<ln>(e2, (unsigned)a);
            e3 = ym_writelane<ln>(e3, (unsigned)(a >> 32));
        };
        if (ab_prev)                                                // the pending row: its successor is v[0]
            put(std::integral_constant<int, 0>{},
                __builtin_amdgcn_ballot_w64(fmaxf(fmaxf(prev2, v[0]), nbx_prev) > prev1 + nms_eps), ab_prev);
        float nbx15 = -INFINITY;
        unsigned long long ab15 = 0;
        // (a row's word is taken when its turn comes: sixteen words taken first are thirty-two scalar registers held
        //  across the tile, which this kernel does not have)
        auto one = [&](auto R) __attribute__((always_inline)) {
            constexpr int r = decltype(R)::value;
            const unsigned long long ab_r = __builtin_amdgcn_ballot_w64(v[r] > nms_lo) & realw;
            if constexpr (r == 15) ab15 = ab_r;
            if (ab_r) {
#ifndef YM_NOSTORE
                if (real) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[r] * us), rsw, ooff, (unsigned)(16 * T + r) * row_b, 0);
#endif
                if constexpr (r < 15) {
                    // beaten by the row below or above, or by an x neighbour: the neighbours compared where they
                    // arrive (lanes without one get 0 and are masked out), not gathered into a maximum first
                    const float below = r > 0 ? v[r > 0 ? r - 1 : 0] : prev1;
                    const float t = v[r] + nms_eps;
                    const int b = (int)__float_as_uint(v[r]);
                    const float l = __uint_as_float((unsigned)__builtin_amdgcn_update_dpp(0, b, 0x111 /* row_shr:1 */, 0xf, 0xf, true));
                    const float rr = __uint_as_float((unsigned)__builtin_amdgcn_update_dpp(0, b, 0x101 /* row_shl:1 */, 0xf, 0xf, true));
                    put(std::integral_constant<int, r + 1>{},
                        __builtin_amdgcn_ballot_w64(below > t) | __builtin_amdgcn_ballot_w64(v[r < 15 ? r + 1 : 15] > t) |
                            (__builtin_amdgcn_ballot_w64(l > t) & has_lw) | (__builtin_amdgcn_ballot_w64(rr > t) & has_rw),
                        ab_r);
                } else {
                    nbx15 = mmx_x_neighbours<false>(v[r], has_l, has_r);      // (a value: the next tile, or row(), tests it)
                }
            }
        };
        auto each = [&](auto... R) __attribute__((always_inline)) { (one(R), ...); };
#define YM_R(i) std::integral_constant<int, i>{}
        each(YM_R(0), YM_R(1), YM_R(2), YM_R(3), YM_R(4), YM_R(5), YM_R(6), YM_R(7), YM_R(8), YM_R(9), YM_R(10), YM_R(11),
             YM_R(12), YM_R(13), YM_R(14), YM_R(15));
#undef YM_R
        if (lane < 16 && (lane > 0 || ydone > 0)) {
            ulonglong2* dst = mrow + (int64_t)(ydone > 0 ? lane : lane - 1) * nent;
            *dst = make_ulonglong2((unsigned long long)e0 | ((unsigned long long)e1 << 32),
                                   (unsigned long long)e2 | ((unsigned long long)e3 << 32));
        }
        mrow += (int64_t)(ydone > 0 ? 16 : 15) * nent;
        prev2 = v[14]; prev1 = v[15]; nbx_prev = nbx15;
        ab_prev = ab15;
        ydone += 16;
    };

    const int nT = (n + 15) >> 4;
    const int nKB = (nT + NB - 3) / 2 + 1;          // last block b with 2 b - NB + 2 <= nT - 1
    const v4f start = {cfg.start, cfg.start, cfg.start, cfg.start};
    v4f acc[NB][4];                                // output tiles t = 0 .. NB - 1 of the current block (the last two start in it)
#pragma unroll
    for (int t = 0; t < NB; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][j] = start;
    bool any0 = false, any1 = false;                // of the two tiles waiting in LDS

    const _Float16 k256 = (_Float16)256.f;
    // one k-block: rows of the tiles the previous block finished, then per group of JH column sets: this block's pieces,
    // (last group: the next block's loads,) the MFMAs, the hand-off of the two tiles that are complete
    auto iter = [&](int b) __attribute__((always_inline)) {
        // -- rows first (before this block's operands take their registers; their stores are older than the loads
        //    issued below, so waiting for those does not wait for these)
#ifndef YM_ROWS_LATE
#define YM_ROWS_LATE 1
#endif
        if (!YM_ROWS_LATE) {
#pragma unroll 1
            for (int h = 0; h < 2; ++h) rows_of(2 * (b - 1) - NB + 2 + h, h, h ? any1 : any0);
        }
        if constexpr (JH < 4) { any0 = !MASK; any1 = !MASK; }
#pragma unroll
        for (int j0 = 0; j0 < 4; j0 += JH) {
            __builtin_amdgcn_sched_barrier(0);
            // -- the four float16 pieces of every dword, one byte permute each: [j][Phi, Plo, Qhi, Qlo], k pairs (2p, 2p + 1)
            v4u pc[JH][4];
#pragma unroll
            for (int j = 0; j < JH; ++j)
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const unsigned d0 = raw[2 * p][j0 + j], d1 = raw[2 * p + 1][j0 + j];
                    // v_perm_b32 {S0 = d1, S1 = d0}: selector 0-3 = bytes of d0, 4-7 = bytes of d1, 0x0c = 0x00
                    pc[j][0][p] = __builtin_amdgcn_perm(d1, d0, 0x0c050c01u);
                    pc[j][1][p] = __builtin_amdgcn_perm(d1, d0, 0x0c040c00u);
                    pc[j][2][p] = __builtin_amdgcn_perm(d1, d0, 0x0c070c03u) ^ 0x00800080u;
                    pc[j][3][p] = __builtin_amdgcn_perm(d1, d0, 0x0c060c02u);
                }
            // (the pieces exist from here on: left to itself the compiler sinks the permutes below the row code, the
            //  block's rows stay alive across it, and the next block's rows go to a second set of registers and are
            //  copied back at the loop's end)
#pragma unroll
            for (int j = 0; j < JH; ++j)
#pragma unroll
                for (int k = 0; k < 4; ++k) asm volatile("" : "+v"(pc[j][k]));
            __builtin_amdgcn_sched_barrier(0);
            // -- the next block's rows, into the registers this block's rows have just left.  Always issued: a
            //    conditional load would merge loaded and old registers -- a copy of all of them per turn -- and the
            //    block past the last one is one more read of the column's last rows, which nobody uses
            if (j0 + JH == 4) load_block(b + 1);
            __builtin_amdgcn_sched_barrier(0);
            if (YM_ROWS_LATE && JH == 4) {
#pragma unroll 1
                for (int h = 0; h < 2; ++h) rows_of(2 * (b - 1) - NB + 2 + h, h, h ? any1 : any0);
                __builtin_amdgcn_sched_barrier(0);
            }
            // -- output tile T = 2 b - NB + 2 + t.  Tiles t = 0, 1 get their last block here and leave for LDS at once
            //    (their registers are free for the two tiles that start with this block: t = NB - 2, NB - 1)
            auto tile_mfmas = [&](int t, bool fresh) __attribute__((always_inline)) {
                v4f* a = &acc[t][j0];
                const v4u* fr = frag + (t * NF) * 64 + lane;
                const v4u ah = fr[0], al = fr[64], bh = fr[(NF / 2) * 64], bl = fr[(NF / 2 + 1) * 64];
                // (x 256: an exponent shift, exact)
                const v4u a256 = NF == 6 ? fr[128] : __builtin_bit_cast(v4u, __builtin_bit_cast(v8h, ah) * k256);
                const v4u b256 = NF == 6 ? fr[320] : __builtin_bit_cast(v4u, __builtin_bit_cast(v8h, bh) * k256);
#pragma unroll
                for (int j = 0; j < JH; ++j) a[j] = mfma16(a256, pc[j][0], fresh ? start : a[j]);
#pragma unroll
                for (int j = 0; j < JH; ++j) a[j] = mfma16(ah, pc[j][1], a[j]);
#pragma unroll
                for (int j = 0; j < JH; ++j) a[j] = mfma16(al, pc[j][0], a[j]);
#pragma unroll
                for (int j = 0; j < JH; ++j) a[j] = mfma16(b256, pc[j][2], a[j]);
#pragma unroll
                for (int j = 0; j < JH; ++j) a[j] = mfma16(bh, pc[j][3], a[j]);
#pragma unroll
                for (int j = 0; j < JH; ++j) a[j] = mfma16(bl, pc[j][2], a[j]);
            };
#pragma unroll
            for (int t = 0; t < 2; ++t) tile_mfmas(t, t >= NB - 2);      // (NB == 3: tile 1 starts and ends in this block)
            // (accumulator register r of lane (g, n16) is row 4 g + r, column 4 n16 + j of the wave's 64)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const v4f* a = &acc[t][j0];
                float mx = -INFINITY;
#pragma unroll
                for (int j = 0; j < JH; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) mx = fmaxf(mx, a[j][r]);
                const bool any = MASK ? __ballot(mx > nms_lo) != 0ull : true;
                // (each accumulator as it is: four rows of one column, one 16-byte store, nothing to assemble)
                if constexpr (JH == 4) {
                    if (t == 0) any0 = any; else any1 = any;
                    if (any) {
                        // (the units are made here from the lane number, a few instructions: kept across the loop
                        //  they are four registers this kernel does not have)
                        int ln = lane;
                        asm volatile("" : "+v"(ln));
                        const int hp = ym_hput(ln);
#pragma unroll
                        for (int j = 0; j < 4; ++j) trw[t * 256 + (hp ^ j)] = a[j];
                    }
                } else {        // (half a tile: the other half may be what is above the threshold)
                    if (t == 0) any0 |= any; else any1 |= any;
#pragma unroll
                    for (int j = 0; j < JH; ++j) trw[t * 256 + (ym_hput(lane) ^ (j0 + j))] = a[j];
                }
            }
            __builtin_amdgcn_sched_barrier(0);     // (the finished tiles' registers are free from here on)
#pragma unroll
            for (int t = 2; t < NB; ++t) {
                tile_mfmas(t, t >= NB - 2);
                if constexpr (NB > 4) __builtin_amdgcn_sched_barrier(0);       // one tile's fragments at a time
            }
        }
        // the window moves on by two tiles.  No instruction in the listing: the compiler shifts it through the C operand
        // of the tiles' first MFMAs, which read one set of registers and write the other
#pragma unroll
        for (int t = 0; t + 2 < NB; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[t][j] = acc[t + 2][j];
        __builtin_amdgcn_wave_barrier();
    };
#pragma unroll 1
    for (int b = 0; b < nKB; ++b) iter(b);
    // the rows of the last block's two tiles
#pragma unroll 1
    for (int h = 0; h < 2; ++h) rows_of(2 * (nKB - 1) - NB + 2 + h, h, h ? any1 : any0);
    if constexpr (MASK) close_pending();     // the last row has no successor
}

template <int NB>
int launch_ym(const mmx_block* d_blocks, int n_blocks, const mmx_zx6_plan& plan, int64_t slot_elems,
              const ym_cfg& cfg, const float* d_p, float* d_log, unsigned long long* d_mask, hipStream_t s)
{
    constexpr int TPW = NB <= 4 ? 1 : YM6_WAVES / 4;        // tile columns per workgroup
    dim3 grid((plan.max_tiles + TPW - 1) / TPW, n_blocks);
    if (d_mask)
        hipLaunchKernelGGL((ym_kernel<NB, true>), grid, dim3(256 * TPW), 0, s, d_blocks, slot_elems, plan.tile_stride,
                           reinterpret_cast<const unsigned*>(d_p), d_log, cfg, d_mask);
    else
        hipLaunchKernelGGL((ym_kernel<NB, false>), grid, dim3(256 * TPW), 0, s, d_blocks, slot_elems, plan.tile_stride,
                           reinterpret_cast<const unsigned*>(d_p), d_log, cfg, d_mask);
    return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
}

}  // namespace

// cp, cq: what one count of P (unorm16) and of Q (snorm16) is worth (mmx_launch_y6's); bias: the constant every output
// is owed (y6_kernel's BIAS: int16 voxels; else 0) -- it leaves through the accumulators' start value
int mmx_launch_ym(const mmx_block* d_blocks, int n_blocks, const mmx_zx6_plan& plan, int64_t slot_elems,
                  const mmx_taps_f32& taps, int radius, const float* d_p, float cp, float cq, float bias,
                  float* d_log, unsigned long long* d_mask, float nms_lo, float nms_eps, hipStream_t stream)
{
    if (!mmx_ym_accepts(taps.w0, taps.w2, radius, cp, cq)) return MMX_ERR_UNSUPPORTED;      // (radius, weights in float16's reach)
    ym_cfg cfg;
    float mx = 0.f;
    for (int k = 0; k <= radius; ++k) {
        cfg.w2[k] = taps.w2[k] * cp;
        cfg.w0[k] = taps.w0[k] * cq;
        mx = fmaxf(mx, fmaxf(fabsf(cfg.w2[k]), fabsf(cfg.w0[k])));
    }
    int e;
    frexpf(mx, &e);                             // mx = f x 2^e, f in [0.5, 1)
    const float up = ldexpf(1.f, -e - 1);       // largest weight into [0.25, 0.5)
    double q128 = 0.0;                          // sum over all taps of the two pieces Q's high byte meets
    for (int k = 0; k <= MMX_MAX_RADIUS_FAST; ++k) {
        cfg.w2[k] = k <= radius ? cfg.w2[k] * up : 0.f;
        cfg.w0[k] = k <= radius ? cfg.w0[k] * up : 0.f;
        const float h = (float)(_Float16)cfg.w0[k];
        const float l = (float)(_Float16)((cfg.w0[k] - h) * 256.f);
        q128 += (k ? 2.0 : 1.0) * ((double)h * 256.0 + (double)l);
    }
    // the pieces are bytes x 2^-24 (float16 subnormals); Q's high byte arrives as offset binary, 128 too large
    cfg.unscale = ldexpf(1.f, e + 1 + 24);
    cfg.start = (float)(-128.0 * 0x1p-24 * q128 + (double)bias / (double)cfg.unscale);
    cfg.lo = nms_lo / cfg.unscale;
    cfg.eps = nms_eps / cfg.unscale;
    cfg.radius = radius;
    cfg.reverse = 1;         // (a batch is walked from its last block backwards: the tiles Z+X wrote last)
    // NB block offsets cover every tap when the first offset beyond either end, RB + 16 - 15 and 16 NB - RB - 31 rows away,
    // is out of reach: R <= 8 (NB - 2) with RB = 8 (NB - 2)
    if (radius <= 8) return launch_ym<3>(d_blocks, n_blocks, plan, slot_elems, cfg, d_p, d_log, d_mask, stream);
    if (radius <= 16) return launch_ym<4>(d_blocks, n_blocks, plan, slot_elems, cfg, d_p, d_log, d_mask, stream);
    return launch_ym<5>(d_blocks, n_blocks, plan, slot_elems, cfg, d_p, d_log, d_mask, stream);
}
