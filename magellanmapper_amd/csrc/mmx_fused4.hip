// Fused X+Z pass on the matrix cores with split-float16 operands (gfx950), the default Z+X path for integer
// voxels.
//
//   zx4_kernel :  I (u8 / u16, read once, x contiguous)  ->  P = G(z) G(x) I
//                                                            Q = G(z) G''(x) I + G''(z) G(x) I
// in two forms that share the arithmetic below:
//   zx_mode 6                   voxels from the operand-ordered copy zx6_pack_kernel makes once per batch, P / Q out
//                               as 16 x 16 tiles of float32 -- every access one contiguous KiB -- feeding y6_kernel;
//   zx_mode 7  (Q16)            the same with the tiles as one dword per voxel (P unorm16, Q snorm16 of value /
//                               bound): the default, whenever the stated rounding bound is inside MMX_LOG_ABS_TOL and
//                               the caller's NMS band covers it.
// (The row-major form of round 4 -- zx_mode 4: the same arithmetic at 1.8 ms in a kernel of 5.3, because every access
// was "16 planes x 64 bytes" -- is what the tiling replaced; DESIGN.md section 4b has the measurements.)
//
// Why.  zx2_kernel needs 5R packed VALU instructions per voxel and a workgroup-wide LDS hand-off per 8 planes;
// measured, neither its arithmetic nor its skeleton (loads, LDS, barriers: 3.5 of its 5.4 ms per 64 blocks at
// R = 16) gets near the 1.8 ms its 10 B/voxel cost at HBM speed.  A 1-D convolution of
// 16 rows is a product with a banded Toeplitz matrix, and v_mfma_f32_16x16x32_f16 multiplies 16 x the flops
// per clock of the float32 pipes.  Float16 carries 11 significant bits, so every float32 factor is split into
// two float16 pieces, x = xh + xl / 2048 (xh = half(x), xl = half((x - xh) * 2048)), and a product is three
// MFMAs (xh wh -> acc0; xh wl + xl wh -> acc1; result acc0 + acc1 / 2048; the dropped xl wl term is 2^-22 of
// the product).  uint16 voxels split EXACTLY into two float16 pieces (high byte / 256 and low byte / 65536, the
// latter float16 subnormals), so the X pass, taken first and straight from global memory, has no data error at
// all.  Measured against the exact float64 values the result is as close as the float32 FMA chains were
// (bench.py: max_f32_error), far inside the eps / 4 the exactness machinery allows.
//
// Layout: no LDS, no barriers.  A WAVE owns one 16-column output tile of one block row (y) and marches along z
// in tiles of 16 planes:
//   X pass   D1[z][x_out] = sum_k In[z][x_in(k)] Wx[x_in(k)][x_out].  A operand = voxels: lane l loads 8
//            consecutive x of plane z0 + (l & 15) with ONE 16-byte load per k-step (k = 8 (l >> 4) + j) and
//            unpacks them into the two exact float16 pieces with byte permutes; B operand = the Toeplitz
//            fragments of this column (constant registers).  The accumulators come out with x_out on
//            lane & 15 and four consecutive z in the four registers --
//   Z pass   D2[x][z_out] = sum_k D1[z_in(k)][x] Wz[z_in(k)][z_out] -- which is exactly the A-operand layout
//            of the next product once two z tiles are put side by side (k = 8 (l >> 4) + j <-> tile j >> 2,
//            plane 4 (l >> 4) + (j & 3): the MFMA does not care in which order k runs as long as both
//            operands agree).  So the X results never leave the registers: they are split into float16 pieces
//            and kept in a sliding window of four z tiles, two k-steps; the Z Toeplitz fragments follow the same k
//            order.  Radius <= 16 needs z tiles U - 1 .. U + 1 of it; radius 17 .. 24 needs the 64 planes
//            [16 U - 24, 16 U + 40): z tiles U - 1 .. U + 1 and a split tile, per lane the half of z tile U + 2 or
//            of z tile U - 2 that the taps reach (cls4 has the map and why it always suffices).
//            The result has z_out on lane & 15 and four consecutive x in the registers: one 16-byte store per
//            lane for P and for Q.
// SciPy's "reflect" boundaries are folded into the Toeplitz fragments (the weight of a mirrored tap is added
// to the tap it mirrors), so no halo is ever materialised and no load leaves the block: chunks and planes that
// would are clamped into it and get zero weights.  The fragments are built on the device by a small setup
// kernel per launch (zx4_setup: one table per distinct block width / depth of the batch, in the part of the
// workspace the fused path does not use).  The X fragments live in registers in the main kernel; the Z fragments
// of the interior z tiles in registers or, for the classes with an LDS table (ZLDS), in LDS, shared by the workgroup.
// The Z fragments of the z tiles at a block's two faces -- the edge output tiles, whose taps leave the block --
// come from the global table when the march reaches them, except in the LDS form of the march (ELDS: 16-bit tiles
// of integer voxels, radius 9 .. 24, the kernels of the headline configuration), where they stand in LDS beside the
// interior table and no step of a wave waits for a load it has issued itself:
//   - head (straight-line): LA steps of the X pass alone, whose stores leave through the descriptor's range, then the
//     low edge tiles; steady loop as before, without the drain in front of it; tail: whole rings and an odd step, the
//     table a run-time LDS address, the X pass of the tiles past the block on the clamped last tile (zero weights);
//   - every step has the steady step's memory instructions, so every s_waitcnt vmcnt in the march is a counted one
//     that leaves the younger voxel tile and the stores in flight.  The global-table form had, per edge step, the
//     voxel tile waited for with vmcnt(0) and three drained fragment round trips in front of the MFMAs.
//   - the pair kernel (radius 9 .. 16) has a second entry point, zx4_rows_kernel, with ONE loop over the wave's linear tile
//     index instead of head / steady loop / tail, in which a wave marches through several rows of its column pair (the
//     row march: ROWS in the kernel's text).  launch_zx6 takes it when some block of the launch gets more than one row
//     per wave, and zx4_kernel, unchanged, when none does: at one row the single loop measured 1 .. 3 % behind.  The copy's
//     row tiles of row y + 1 follow those of row y, so step g loads tile min(g + PF, last), does the X pass of tile g and
//     the Z pass of tile g - 1 with the table of U = (g - 1) mod ntz, and stores into that tile's row -- the store
//     descriptors follow U on the scalar side.  The table fill and its barrier, the X fragments, the start values, the
//     X-only first step and the clamped last one are paid once per run of rows instead of once per row; at a row change
//     the window holds the neighbouring row's tile against the edge tables' zero weights.  Rows per wave: chosen on the
//     host per block of the launch (zx4_rows_rule -- two while enough work follows to keep the GPU full until such a
//     wave ends, one on the last blocks) or forced with MMX_ZX_ROWS(n); the grid is flat, block after block.  The
//     split-tile kernel (radius 17 .. 24) keeps one row per wave.  Measurements: profiles/r20_zx_row_march.txt.
// A batch with a depth whose edge tiles exceed the LDS budget (zx4_edges_fit), and any batch under
// MMX_ZX_EDGE_GLOBAL, runs the global-table form: the same arithmetic, bit for bit.  Measurements:
// profiles/r14_zx_edge_steps.txt, DESIGN.md section 4b.

#include <algorithm>
#include <atomic>
#include <type_traits>
#include <vector>

#include "mmx_device.h"

#define MMX_ZX4_MAXCLS 8
#define MMX_ZX4_MAXDEV 64          // devices whose wave slots are remembered (zx4_wave_slots)
// cache policy bits of the streaming accesses (gfx940+: 1 = sc0, 2 = nt, 16 = sc1)
#ifndef ZX4_ST_AUX
#define ZX4_ST_AUX 0
#endif
#ifndef ZX4_LD_AUX
#define ZX4_LD_AUX 0
#endif

// Row march (the pair kernel's LDS form): a wave keeps its column pair and walks down n rows of its block.  n is set
// per block of the launch (zx4_rows_rule) and never grows from one block to the next, so the blocks fall into at most
// MMX_ZX4_ROWCLS runs of equal n (two rows per wave, then one).  The grid is flat -- the workgroups of block 0, then
// those of block 1, ... in dispatch order -- and a workgroup finds its block from the first workgroup of each run.
#define MMX_ZX4_ROWCLS 2
struct zx4_rows_sched {
    int n[MMX_ZX4_ROWCLS];                 // rows per wave
    int blk[MMX_ZX4_ROWCLS];               // first block of the run
    int wg[MMX_ZX4_ROWCLS];                // workgroups per block (a multiple of 8: the XCD-aware order)
    int wg0[MMX_ZX4_ROWCLS];               // first workgroup of the run; an empty run starts where the next one does
    int total;                             // workgroups of the launch
};
struct zx4_rows_place { int block, wx, wgs, n; };     // of a workgroup: its block, its index and the count there, rows per wave
__host__ __device__ inline zx4_rows_place zx4_rows_decode(const zx4_rows_sched& r, int flat)
{
    int k_n = r.n[0], k_blk = r.blk[0], k_wg = r.wg[0], k_wg0 = r.wg0[0];
    for (int i = 1; i < MMX_ZX4_ROWCLS; ++i) {
        const bool in = flat >= r.wg0[i];
        k_n = in ? r.n[i] : k_n; k_blk = in ? r.blk[i] : k_blk; k_wg = in ? r.wg[i] : k_wg; k_wg0 = in ? r.wg0[i] : k_wg0;
    }
    const int rel = flat - k_wg0;
    return zx4_rows_place{k_blk + rel / k_wg, rel % k_wg, k_wg, k_n};
}

struct mmx_zx4_cfg {
    float w0[MMX_MAX_RADIUS_FAST + 1];     // order-0 half kernel (plain)
    float w2[MMX_MAX_RADIUS_FAST + 1];     // order-2 half kernel (plain)
    float xscale;                          // 65536 / 65535 (u16) or 256 / 255 (u8): the pieces carry v / 2^16
    int radius;
    int ncw, ncz;                          // distinct block widths / depths of the batch
    int wcls[MMX_ZX4_MAXCLS];              // widths (nx)
    int zcls[MMX_ZX4_MAXCLS];              // depths (nz)
    int maxcol, maxu;                      // table extents: columns per width class, z tiles per depth class
    float qp, qq;                          // Q16 tiles: P / bound(P) and Q / bound(Q) land in [0, 1] and [-1, 1]
    int staged;                            // 0: chunks clamped into the row (zx4); 1: at their natural position (zx5); 2: same, windows at 16 c - R8 (zx6)
    int ntw;                               // column tiles per wave (tiled form): 2 = tiles (2 p, 2 p + 1) share the window of tile 2 p
};
struct mmx_zx4_cfg_rows : mmx_zx4_cfg { zx4_rows_sched rows; };       // ... of the kernel with the row march
__device__ inline zx4_rows_sched zx4_sched_of(const mmx_zx4_cfg&) { return zx4_rows_sched{}; }
__device__ inline const zx4_rows_sched& zx4_sched_of(const mmx_zx4_cfg_rows& c) { return c.rows; }

namespace {

#ifndef ZX4_PF
#define ZX4_PF 3
#endif
constexpr int kPF4 = ZX4_PF;       // z tiles of voxels in flight per wave
#ifndef ZX6_PF
#define ZX6_PF 2
#endif
constexpr float kLoScale = 2048.f;
constexpr float kLoInv = 1.f / 2048.f;

// geometry classes actually compiled: (NKX, LA) = (1, 1) for R <= 8, (2, 1) for R <= 16, (2, 2) for R <= 24
template <int NKX, int LA> struct cls4 {
    static constexpr int R8 = NKX == 1 ? 8 : (LA == 1 ? 16 : 24);
    // first input column of output column tile c: 16 c - R8, moved down to a multiple of 32 voxels where the
    // k-steps still reach the last input (16 c + 15 + R8) -- whole 64-byte pieces per plane for uint16
    static __host__ __device__ constexpr int xstart(int c)
    {
        const int lo = 16 * c - R8;
        const int al = lo & ~31;
        return (al + 32 * NKX >= 16 * c + 16 + R8) ? al : lo;
    }
    // The Z pass of output tile U is two k-steps of two 16-plane operand slots each, in both depths of window.
    // LA = 1: [U - 1, U] [U + 1, zero weights].
    // LA = 2: [V, U - 1] [U, U + 1], where the SPLIT tile V holds, lane by lane, the two half tiles that the taps
    // still reach: planes 16 U + 32 .. 16 U + 39 (the lower half of tile U + 2) in the lanes with lane >> 4 in {0, 1}
    // and planes 16 U - 24 .. 16 U - 17 (the upper half of tile U - 2) in the lanes with lane >> 4 in {2, 3} -- under
    // the operand layout (plane 4 (lane >> 4) + (j & 3)) those are the lanes that hold these planes of either tile,
    // so V is a per-lane choice between two tiles' registers.  Together the 64 planes [16 U - 24, 16 U + 40).
    // They always suffice, for any block depth nz >= R (R <= 24):
    //   - the direct taps of a real output zo in [16 U, min(16 U + 15, nz - 1)] lie in [16 U - 24, 16 U + 39];
    //   - a left mirror image -1 - p of a tap exists only for U <= 1 and lands in [0, 23 - 16 U];
    //   - a right mirror image 2 nz - 1 - p lands in [nz - R, nz - 1], and nz - R >= 16 U - 24 because tile U has a
    //     real plane (nz > 16 U);
    // so every folded tap meets a plane the two k-steps hold, also in blocks of one or two z tiles.  (Five whole
    // tiles and an always-zero sixth, as this class had them, are three k-steps: 27 Z MFMAs per tile step for 18.)
    static constexpr bool SPLIT = LA == 2;
    static constexpr int NKZ = 2;
    static constexpr int NT = 4;
    // most edge output tiles whose tables a workgroup keeps in LDS beside the interior one (8 KiB each; three workgroups
    // of the LA = 2 class still share a CU's 160 KiB at four)
    static constexpr int kMaxEdge = LA == 1 ? 3 : 4;
};

// Edge output tiles of a block nz deep at radius R -- the z tiles whose taps leave the block: U < u_lo and U > u_hi --
// and whether the LDS form of zx4_kernel takes the block: they fit, its straight-line head (LA steps of X alone, tiles
// 0 .. LA - 1) is this block's head, and the block has that many steps.
struct zx4_edges { int u_lo, u_hi, hi0, n; };
__host__ __device__ inline zx4_edges zx4_edge_tiles(int nz, int R)
{
    zx4_edges e;
    const int ntz = (nz + 15) >> 4;
    e.u_lo = (R + 15) >> 4;                             // first U with 16 U - R >= 0
    e.u_hi = (nz - 16 - R) >> 4;                        // last U with 16 U + 15 + R <= nz - 1 (may be < u_lo)
    e.hi0 = e.u_hi + 1 > e.u_lo ? e.u_hi + 1 : e.u_lo;  // first high edge tile
    e.n = e.u_lo + (ntz > e.hi0 ? ntz - e.hi0 : 0);
    return e;
}
template <int NKX, int LA>
bool zx4_edges_fit(int nz, int R)
{
    const zx4_edges e = zx4_edge_tiles(nz, R);
    const int ntz = (nz + 15) >> 4;
    return e.n <= cls4<NKX, LA>::kMaxEdge && e.u_lo == LA && ntz + LA >= 2 * LA && ntz >= e.u_lo;
}

// Rows per wave of the row march, per block of a launch (blocks are dispatched in order).  A wave with two rows lives
// twice as long, and whatever is still running when the last workgroup has been dispatched drains on a GPU that is no
// longer full: a block gets two rows per wave only while the wave-rows of the blocks behind it fill every resident wave
// slot twice over, so that its waves end before the launch does.  The blocks at the end get one -- at least a slot
// count's worth of wave-rows -- and so does every block of a launch below kRowsFill slot counts, which then runs the
// one-row kernel as before.  More than two rows per wave measured slower (profiles/r20_zx_row_march.txt, section 4).
// Never growing from block to block.  forced > 0: that many rows per wave everywhere (cross-checks, sweeps).
constexpr int kRowsFill = 7;
inline void zx4_rows_rule(int n_blocks, const int32_t* rows, const int32_t* waves_per_row, int slots, int forced, int32_t* nr)
{
    int64_t total = 0;
    for (int b = 0; b < n_blocks; ++b) total += (int64_t)rows[b] * waves_per_row[b];
    int64_t behind = total;
    for (int b = 0; b < n_blocks; ++b) {
        behind -= (int64_t)rows[b] * waves_per_row[b];
        nr[b] = forced > 0 ? forced : (slots > 0 && total >= (int64_t)kRowsFill * slots && behind >= 2 * (int64_t)slots ? 2 : 1);
    }
}
// ... and the flat grid it makes: runs of equal n (zx4_rows_sched); false: more runs than the record holds
inline bool zx4_rows_make(int n_blocks, const int32_t* rows, const int32_t* waves_per_row, const int32_t* nr, zx4_rows_sched* s)
{
    int k = -1, total = 0;
    for (int b = 0; b < n_blocks; ++b) {
        if (k < 0 || nr[b] != s->n[k]) {
            if (++k == MMX_ZX4_ROWCLS) return false;
            s->n[k] = nr[b]; s->blk[k] = b; s->wg0[k] = total; s->wg[k] = 8;
            // workgroups per block: what the run's largest block needs
            for (int j = b; j < n_blocks && nr[j] == nr[b]; ++j) {
                const int waves = (rows[j] + nr[b] - 1) / nr[b] * waves_per_row[j];
                s->wg[k] = std::max(s->wg[k], (((waves + 3) / 4) + 7) & ~7);
            }
        }
        total += s->wg[k];
    }
    for (++k; k < MMX_ZX4_ROWCLS; ++k) { s->n[k] = 1; s->blk[k] = n_blocks; s->wg[k] = 8; s->wg0[k] = total; }
    s->total = total;
    return true;
}

// ------------------------------------------------------------------------------------ setup: Toeplitz fragments
// weight of input position p for output o on an axis of n voxels with SciPy "reflect" folded in
__device__ __forceinline__ float folded_tap(const float* w, int R, int p, int o, int n)
{
    float s = 0.f;
    int d = p - o; d = d < 0 ? -d : d;
    if (d <= R) s += w[d];
    d = (-1 - p) - o; d = d < 0 ? -d : d;            // left mirror image of p
    if (d <= R) s += w[d];
    d = (2 * n - 1 - p) - o; d = d < 0 ? -d : d;     // right mirror image of p
    if (d <= R) s += w[d];
    return s;
}

// One thread per (table entry, lane): 8 float16 weights (one MFMA operand register quad) as hi and lo pieces.
//   X table [class][column][m][kernel][piece][lane], Z table [class][U][ks][kernel][piece][lane]
template <int NKX, int LA>
__global__ void __launch_bounds__(256)
zx4_setup(mmx_zx4_cfg cfg, v4u* __restrict__ xtab, v4u* __restrict__ ztab)
{
    using cg = cls4<NKX, LA>;
    const int R = cfg.radius;
    const int lane = threadIdx.x & 63;
    const int kq = lane >> 4, col = lane & 15;
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);           // entry index over both tables: (.., kernel)
    const int nx_entries = cfg.ncw * cfg.maxcol * NKX * 2;
    const int nz_entries = cfg.ncz * cfg.maxu * cg::NKZ * 2;
    float wt[8];
    v4u* dst;
    if (e < nx_entries) {
        const int kern = e & 1;
        const int m = (e >> 1) % NKX;
        const int c = ((e >> 1) / NKX) % cfg.maxcol;
        const int cl = ((e >> 1) / NKX) / cfg.maxcol;
        const int W = cfg.wcls[cl];
        const float* w = kern ? cfg.w2 : cfg.w0;
        const int xo = 16 * c + col;
        // natural start of this lane's chunk (tiled form, staged == 2: windows start at 16 c - R8, any multiple of 8)
        // (two tiles per wave: the odd tile of a pair reads the even one's window, 16 columns further left)
        const int cwin = cfg.ntw == 2 ? (c & ~1) : c;
        const int xc = (cfg.staged == 2 ? 16 * cwin - cg::R8 : cg::xstart(c)) + 32 * m + 8 * kq;
        int xl = xc < 0 ? 0 : xc;
        xl = xl > W - 8 ? W - 8 : xl;                               // where the kernel loads it from
        if (cfg.staged) xl = xc;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int p = xl + j;
            const bool ok = p >= xc && p < xc + 8 && p >= 0 && p < W && xo < W;
            // (16-bit tiles: their scales ride in the weights -- G(x) carries 1 / bound(P), G''(x) 1 / bound(Q), and
            //  the order-2 Z fragments below the ratio -- so that the kernel's results come out ready to convert)
            wt[j] = ok ? folded_tap(w, R, p, xo, W) * cfg.xscale * (cfg.qp > 0.f ? (kern ? cfg.qq : cfg.qp) : 1.f) : 0.f;
        }
        dst = xtab + (size_t)e * 2 * 64;
    } else if (e < nx_entries + nz_entries) {
        const int ez = e - nx_entries;
        const int kern = ez & 1;
        const int ks = (ez >> 1) % cg::NKZ;
        const int U = ((ez >> 1) / cg::NKZ) % cfg.maxu;
        const int cl = ((ez >> 1) / cg::NKZ) / cfg.maxu;
        const int nz = cfg.zcls[cl];
        const float* w = kern ? cfg.w2 : cfg.w0;
        const int zo = 16 * U + col;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = 2 * ks + (j >> 2);                        // operand slot of this k
            // (LA = 2: slot 0 is the split tile -- this lane's planes of tile U + 2 or of tile U - 2: cls4)
            const int tile = cg::SPLIT ? (i == 0 ? (kq < 2 ? U + 2 : U - 2) : U - 2 + i) : U - LA + i;
            const int zi = 16 * tile + 4 * kq + (j & 3);
            const bool ok = (cg::SPLIT || i < cg::NT - 1) && zi >= 0 && zi < nz && zo < nz;
            wt[j] = ok ? folded_tap(w, R, zi, zo, nz) * (cfg.qp > 0.f && kern ? cfg.qq / cfg.qp : 1.f) : 0.f;
        }
        dst = ztab + (size_t)ez * 2 * 64;
    } else {
        return;
    }
    unsigned hi[4], lo[4];
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
        const v2f v = {wt[j], wt[j + 1]};
        const v2h h = __builtin_convertvector(v, v2h);
        const v2f r = {(wt[j] - (float)h.x) * kLoScale, (wt[j + 1] - (float)h.y) * kLoScale};
        hi[j >> 1] = __builtin_bit_cast(unsigned, h);
        lo[j >> 1] = __builtin_bit_cast(unsigned, __builtin_convertvector(r, v2h));
    }
    dst[lane] = (v4u){hi[0], hi[1], hi[2], hi[3]};
    dst[64 + lane] = (v4u){lo[0], lo[1], lo[2], lo[3]};
}

// ------------------------------------------------------------------------------------------------ main kernel
template <typename InT> struct pieces4;
// 8 consecutive uint16 voxels (4 dwords) -> high bytes / 256 and low bytes / 65536 as packed float16:
//   0x4400 | b  =  4 + b / 256      (float16, exponent 2^2, ulp 2^-8)
//   0x2400 | b  =  2^-6 + b / 65536 (exponent 2^-6, ulp 2^-16)
template <> struct pieces4<uint16_t> {
    using raw_t = v4u;
    static __device__ __forceinline__ raw_t load(rsrc_t r, unsigned off, unsigned soff = 0)
    {
        return __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(r, off, soff, ZX4_LD_AUX));
    }
    static __device__ __forceinline__ void split(const raw_t& d, v4u& hi, v4u& lo)
    {
        const v2h four = {(_Float16)4.0f, (_Float16)4.0f};
        const v2h sixty4th = {(_Float16)0.015625f, (_Float16)0.015625f};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            // v_perm_b32: bytes of {S0 = constant, S1 = data}; selector bytes 0-3 pick from S1, 4-7 from S0
            const unsigned th = __builtin_amdgcn_perm(0x44004400u, d[i], 0x07030501u);   // [44 b3 44 b1]
            const unsigned tl = __builtin_amdgcn_perm(0x24002400u, d[i], 0x07020500u);   // [24 b2 24 b0]
            hi[i] = __builtin_bit_cast(unsigned, __builtin_bit_cast(v2h, th) - four);
            lo[i] = __builtin_bit_cast(unsigned, __builtin_bit_cast(v2h, tl) - sixty4th);
        }
    }
    // The same pieces with their exponent offsets left in: hi = 4 + b / 256, lo = 2^-6 + b / 65536.  A constant added
    // to every element of an A operand adds (constant x column sum of B) to every row of the product: the kernel
    // starts its accumulators at minus that, computed once per wave -- half the split's instructions.
    static constexpr float kBiasHi = 4.0f, kBiasLo = 0.015625f;
    static __device__ __forceinline__ void split_biased(const raw_t& d, v4u& hi, v4u& lo)
    {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            hi[i] = __builtin_amdgcn_perm(0x44004400u, d[i], 0x07030501u);
            lo[i] = __builtin_amdgcn_perm(0x24002400u, d[i], 0x07020500u);
        }
    }
};
// (uint8 voxels: zx6_pack_kernel widens them to uint16, shifted into the high byte -- the uint16 pieces serve both)

// float voxels: zx6_pack_f32_kernel has split them already -- per unit of 8 columns x 16 planes the high
// float16 pieces (256 bytes) then the low ones, v = hi + lo / 2048 -- two 16-byte loads per k-step, no unpacking
struct presplit_t { v4u h, l; };
template <> struct pieces4<float> {
    using raw_t = presplit_t;
    static __device__ __forceinline__ raw_t load(rsrc_t r, unsigned off, unsigned soff = 0)
    {
        raw_t v;
        v.h = __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(r, off, soff, ZX4_LD_AUX));
        v.l = __builtin_bit_cast(v4u, __builtin_amdgcn_raw_buffer_load_b128(r, off + 256u, soff, ZX4_LD_AUX));
        return v;
    }
    static __device__ __forceinline__ void split(const raw_t& d, v4u& hi, v4u& lo) { hi = d.h; lo = d.l; }
    [[maybe_unused]] static constexpr float kBiasHi = 0.f, kBiasLo = 0.f;      // (never biased: read in discarded branches only)
    static __device__ __forceinline__ void split_biased(const raw_t& d, v4u& hi, v4u& lo) { hi = d.h; lo = d.l; }
};
template <typename InT> struct is_f32_4 { static constexpr bool value = false; };
template <> struct is_f32_4<float> { static constexpr bool value = true; };
template <typename InT> struct lo_scaled4 { static constexpr bool value = false; };     // low piece carries x 2048?
template <> struct lo_scaled4<float> { static constexpr bool value = true; };

// The voxels come from the operand-ordered copy zx6_pack_kernel leaves (`vol` = that copy,
// stride_z = its elements per block) and P / Q leave as 16 x 16 tiles of 1 KiB (slot_elems = tile elements per
// block) in (y, c, U) order, which y6_kernel (mmx_fused.hip) reads: every global access of a wave is then one
// contiguous KiB.
// Q16 (zx_mode 7): the tile holds one dword per voxel, P as unorm16 of P / bound(P) in the low half and Q as snorm16
// of Q / bound(Q) in the high half (the bounds follow from the weights alone: mmx_tiled_q16_error_bound) -- half
// the bytes for the Y pass to read and for this kernel to write, at a known error that the caller's band must cover.
// NTW = 2 (Q16, 8 < radius <= 16): a wave owns TWO adjacent column tiles (2 p, 2 p + 1).  Their windows -- 48
// of the 64 columns two k-steps load -- overlap by two thirds, and the 64 columns from 16 c - 16 on hold both: the
// same two loads per z step now feed two output tiles (half the L2 read requests per tile: the counters had shown
// 4.3 x as many bytes requested from L2 as read from HBM, neighbouring waves re-reading each other's windows), and
// the voxels are unpacked into float16 pieces once for both (-16 of ~92 VALU instructions per tile step).  The second
// tile's X fragments and window are another 64 registers: two waves per SIMD instead of three, each with twice the
// independent work per step.  An odd tile count leaves the last wave of a row one tile: it computes the second with
// zero weights and its stores are dropped by a zero-length buffer descriptor (no branch in the march).
// The kernel's text stands once, in mmx_zx4_march.inc, for two entry points: zx4_kernel, one row per wave, and
// zx4_rows_kernel, the pair kernel's LDS form with the row march (ROWS in the text), whose record carries the launch's
// row schedule.
template <int NKX, int LA, typename InT, bool Q16 = false, int NTW = 1, bool ELDS = false>
__global__ void __launch_bounds__(256, (NTW == 1 && (LA == 1 || Q16) && !is_f32_4<InT>::value) ? 3 : 2)   // (float32 tiles, LA == 2: 213 registers)
zx4_kernel(const InT* __restrict__ vol, int64_t stride_z, int64_t stride_y,
           const mmx_block* __restrict__ blocks, int64_t slot_elems,
           float* __restrict__ gp, float* __restrict__ gq,
           const v4u* __restrict__ xtab, const v4u* __restrict__ ztab, mmx_zx4_cfg cfg)
{
    constexpr bool ROWS = false;
#include "mmx_zx4_march.inc"
}
template <int NKX, int LA, typename InT, bool Q16, int NTW, bool ELDS>
__global__ void __launch_bounds__(256, 2)
zx4_rows_kernel(const InT* __restrict__ vol, int64_t stride_z, int64_t stride_y,
                const mmx_block* __restrict__ blocks, int64_t slot_elems,
                float* __restrict__ gp, float* __restrict__ gq,
                const v4u* __restrict__ xtab, const v4u* __restrict__ ztab, mmx_zx4_cfg_rows cfg)
{
    static_assert(ELDS && NTW == 2, "the row march: the pair kernel's LDS form");
    constexpr bool ROWS = true;
#include "mmx_zx4_march.inc"
}



// ------------------------------------------------------------------------------- tiled variant (zx_mode 6)
// Operand-ordered copy of the blocks' voxels, made once per batch: for every block row y and z tile t the row
// tile of 16 planes x nx voxels as units of 8 columns x 16 planes (256 bytes, plane-major inside), widened to
// uint16 (uint8 voxels shifted into the high byte): the four units a lane group of zx4_kernel needs for one
// k-step are one contiguous KiB
// wherever the window starts.  Planes past the block and columns past the row read as zero.  Any strides, any
// alignment: the copy is what lifts zx4's 16-byte alignment rules.
// WIDE: rows of more than 512 voxels, taken in x panels of 512 columns (64 units) through the same LDS tile -- panel p
// fills units 64 p .. 64 p + 63 of the row tile, the unit order of the copy is the same.  Rows up to 512 voxels run the
// one-panel form (WIDE = false): the same statements with x0 = 0 and the row's own unit count, no loop and no second
// barrier (C3's rows are 261 voxels: profiles/r10_c3_ab.txt has its zxpack times against the kernel without panels).
// (int16 voxels leave as u = x ^ 0x8000, the order-preserving uint16 -- the uint16 pieces and kernels serve them too:
//  zx4's weights carry 2 x 65536 / 65535 for them and the Y pass takes the constant off that the offset adds)
template <typename InT> struct pack_flip { static constexpr unsigned one = mmx_key<InT>::bias, two = one * 0x10001u; };
template <typename InT, bool WIDE>
__global__ void __launch_bounds__(256)
zx6_pack_kernel(const InT* __restrict__ vol, int64_t stride_z, int64_t stride_y, int64_t stride_x,
                const mmx_block* __restrict__ blocks, uint16_t* __restrict__ pack, int64_t pack_stride)
{
    constexpr int PITCH = 512 + 8;                       // uint16 per LDS row: one panel of 512 columns
    __shared__ __attribute__((aligned(16))) uint16_t tile[16][PITCH];
    const mmx_block bd = blocks[blockIdx.y];
    const int ntz = (bd.nz + 15) >> 4, nrow8 = (bd.nx + 7) >> 3;
    const int yt = blockIdx.x;
    if (yt >= bd.ny * ntz) return;
    const int y = yt / ntz, t = yt - y * ntz;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const InT* src0 = vol + bd.src_off + (int64_t)y * stride_y;
    // rows that start on 8-byte boundaries (the usual case: block origins on multiples of 4 voxels): 4 voxels per
    // lane and load; the last, partial group of a row and everything else one voxel at a time
    bool quads = false;
    if constexpr (sizeof(InT) == 2)
        quads = stride_x == 1 && ((bd.src_off | stride_y | stride_z) & 3) == 0 && (reinterpret_cast<uintptr_t>(vol) & 7) == 0;
    // panel p: its first column, its units, the voxels the row still holds from there (the zero fill starts at nx)
    auto panel = [&](int p) __attribute__((always_inline)) {
        const int x0 = WIDE ? 512 * p : 0;
        const int nch8 = WIDE ? (nrow8 - 64 * p < 64 ? nrow8 - 64 * p : 64) : nrow8;
        const int nx = bd.nx - x0;
        const InT* src = src0 + (int64_t)x0 * stride_x;
        if (quads) {
            // All of a wave's loads -- four planes x (up to) two 4-voxel groups per lane -- are issued before the first
            // LDS write: a workgroup moves 8 KiB in and 8 KiB out and nothing else hides its load latency (the loop form
            // had one or two loads in flight per wave: 2.8 TB/s).
            v2u v[4][2];
            bool have[4][2];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int z = 16 * t + 4 * wave + i;
                const InT* row = src + (int64_t)(z < bd.nz ? z : 0) * stride_z;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int x = lane * 4 + 256 * h;
                    have[i][h] = x < 8 * nch8;
                    v[i][h] = (v2u){0u, 0u};
                    if (have[i][h] && z < bd.nz) {
                        if (x + 3 < nx) {
                            v[i][h] = *reinterpret_cast<const v2u*>(row + x);
                            if constexpr (pack_flip<InT>::two != 0u) v[i][h] ^= (v2u){pack_flip<InT>::two, pack_flip<InT>::two};
                        } else {
                            unsigned e[4];
#pragma unroll
                            for (int j = 0; j < 4; ++j) e[j] = x + j < nx ? ((unsigned)row[x + j] & 0xffffu) ^ pack_flip<InT>::one : 0u;
                            v[i][h] = (v2u){e[0] | (e[1] << 16), e[2] | (e[3] << 16)};
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    if (have[i][h]) *reinterpret_cast<v2u*>(&tile[4 * wave + i][lane * 4 + 256 * h]) = v[i][h];
        } else
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 4 * wave + i, z = 16 * t + r;
            if (z >= bd.nz) {
                for (int x = lane * 4; x < 8 * nch8; x += 256) *reinterpret_cast<v2u*>(&tile[r][x]) = (v2u){0u, 0u};
            } else {
                for (int x = lane; x < 8 * nch8; x += 64)
                    tile[r][x] = x < nx ? (uint16_t)(((unsigned)src[(int64_t)z * stride_z + (int64_t)x * stride_x] << (sizeof(InT) == 1 ? 8 : 0)) ^
                                                     pack_flip<InT>::one)
                                           : (uint16_t)0;     // (uint8 voxels go to the HIGH byte: the exact high float16 piece carries them)
            }
        }
        __syncthreads();
        v4u* dst = reinterpret_cast<v4u*>(pack + (int64_t)bd.slot * pack_stride) + (int64_t)yt * nrow8 * 16 + (WIDE ? 1024 * p : 0);
        for (int u = threadIdx.x; u < nch8 * 16; u += 256) {
            const int j = u >> 4, r = u & 15;
            dst[u] = *reinterpret_cast<const v4u*>(&tile[r][8 * j]);
        }
    };
    if constexpr (WIDE) {
#pragma unroll 1
        for (int p = 0; p < (nrow8 + 63) >> 6; ++p) {
            if (p) __syncthreads();                      // (the panel before is out of the tile)
            panel(p);
        }
    } else {
        panel(0);
    }
}

// The same copy for float32 voxels, split into float16 pieces on the way (v = hi + lo / 2048: 22 significant bits, what
// the fragments carry too): per unit the 16 planes' high pieces (256 bytes), then their low pieces.  Valid for
// |v| < 65504 and loses nothing worth having above ~2^-10: the caller vouches for the range (MMX_ZX_FLOAT_RANGE_OK).
// (WIDE: x panels of 512 columns, as in zx6_pack_kernel)
template <bool WIDE>
__global__ void __launch_bounds__(256)
zx6_pack_f32_kernel(const float* __restrict__ vol, int64_t stride_z, int64_t stride_y, int64_t stride_x,
                    const mmx_block* __restrict__ blocks, uint16_t* __restrict__ pack, int64_t pack_stride)
{
    constexpr int PITCH = 512 + 4;                       // dwords (hi | lo << 16) per LDS row: one panel of 512 columns
    __shared__ __attribute__((aligned(16))) unsigned tile[16][PITCH];
    const mmx_block bd = blocks[blockIdx.y];
    const int ntz = (bd.nz + 15) >> 4, nrow8 = (bd.nx + 7) >> 3;
    const int yt = blockIdx.x;
    if (yt >= bd.ny * ntz) return;
    const int y = yt / ntz, t = yt - y * ntz;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* src0 = vol + bd.src_off + (int64_t)y * stride_y;
    auto pieces = [](float v) __attribute__((always_inline)) {
        const _Float16 h = (_Float16)v;
        const _Float16 l = (_Float16)((v - (float)h) * kLoScale);
        return (unsigned)__builtin_bit_cast(unsigned short, h) | ((unsigned)__builtin_bit_cast(unsigned short, l) << 16);
    };
    // rows that start on 16-byte boundaries (preprocessed slot buffers, most float images): 4 voxels per lane and load
    const bool quads = stride_x == 1 && ((bd.src_off | stride_y | stride_z) & 3) == 0 && (reinterpret_cast<uintptr_t>(vol) & 15) == 0;
    auto panel = [&](int p) __attribute__((always_inline)) {
        const int x0 = WIDE ? 512 * p : 0;
        const int nch8 = WIDE ? (nrow8 - 64 * p < 64 ? nrow8 - 64 * p : 64) : nrow8;
        const int nx = bd.nx - x0;
        const float* src = src0 + (int64_t)x0 * stride_x;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = 4 * wave + i, z = 16 * t + r;
            if (quads && z < bd.nz) {
                const float* row = src + (int64_t)z * stride_z;
                for (int x = lane * 4; x < 8 * nch8; x += 256) {
                    v4f v = {0.f, 0.f, 0.f, 0.f};
                    if (x + 3 < nx) v = *reinterpret_cast<const v4f*>(row + x);
                    else
                        for (int j = 0; j < 4; ++j) v[j] = x + j < nx ? row[x + j] : 0.f;
                    *reinterpret_cast<v4u*>(&tile[r][x]) = (v4u){pieces(v[0]), pieces(v[1]), pieces(v[2]), pieces(v[3])};
                }
            } else {
                for (int x = lane; x < 8 * nch8; x += 64) {
                    float v = 0.f;
                    if (z < bd.nz && x < nx) v = src[(int64_t)z * stride_z + (int64_t)x * stride_x];
                    tile[r][x] = pieces(v);
                }
            }
        }
        __syncthreads();
        v4u* dst = reinterpret_cast<v4u*>(pack + (int64_t)bd.slot * pack_stride) + (int64_t)yt * nrow8 * 32 + (WIDE ? 2048 * p : 0);
        for (int u = threadIdx.x; u < nch8 * 16; u += 256) {
            const int j = u >> 4, r = u & 15;
            const v4u a = *reinterpret_cast<const v4u*>(&tile[r][8 * j]);
            const v4u b = *reinterpret_cast<const v4u*>(&tile[r][8 * j + 4]);
            // dwords (hi | lo << 16) of 8 columns -> 4 dwords of packed high pieces, 4 of packed low pieces
            const v4u hi = {__builtin_amdgcn_perm(a[1], a[0], 0x05040100u), __builtin_amdgcn_perm(a[3], a[2], 0x05040100u),
                             __builtin_amdgcn_perm(b[1], b[0], 0x05040100u), __builtin_amdgcn_perm(b[3], b[2], 0x05040100u)};
            const v4u lo = {__builtin_amdgcn_perm(a[1], a[0], 0x07060302u), __builtin_amdgcn_perm(a[3], a[2], 0x07060302u),
                             __builtin_amdgcn_perm(b[1], b[0], 0x07060302u), __builtin_amdgcn_perm(b[3], b[2], 0x07060302u)};
            dst[j * 32 + r] = hi;
            dst[j * 32 + 16 + r] = lo;
        }
    };
    if constexpr (WIDE) {
#pragma unroll 1
        for (int p = 0; p < (nrow8 + 63) >> 6; ++p) {
            if (p) __syncthreads();                      // (the panel before is out of the tile)
            panel(p);
        }
    } else {
        panel(0);
    }
}

// The distinct block widths / depths of a batch (the Toeplitz tables hold one set of fragments per class) and its
// tile extents; false: more classes than MMX_ZX4_MAXCLS.
struct zx_classes {
    int ncw, ncz, wcls[MMX_ZX4_MAXCLS], zcls[MMX_ZX4_MAXCLS];
    int maxcol, maxu;       // column tiles / z tiles of the widest / deepest block
};
bool collect_classes(const mmx_block* h_blocks, int n_blocks, zx_classes* c)
{
    c->ncw = c->ncz = c->maxcol = c->maxu = 0;
    for (int i = 0; i < n_blocks; ++i) {
        const mmx_block& b = h_blocks[i];
        int j;
        for (j = 0; j < c->ncw && c->wcls[j] != b.nx; ++j) {}
        if (j == c->ncw) { if (j == MMX_ZX4_MAXCLS) return false; c->wcls[c->ncw++] = b.nx; }
        for (j = 0; j < c->ncz && c->zcls[j] != b.nz; ++j) {}
        if (j == c->ncz) { if (j == MMX_ZX4_MAXCLS) return false; c->zcls[c->ncz++] = b.nz; }
        c->maxcol = std::max(c->maxcol, (b.nx + 15) / 16);
        c->maxu = std::max(c->maxu, (b.nz + 15) / 16);
    }
    return true;
}

// Resident waves of a kernel of 256 threads on the current device: the runtime's workgroups per CU x 4 x the CUs; 0 when
// it cannot be had (the row march then keeps one row per wave).  Asked once per device.
int zx4_wave_slots(const void* kernel)
{
    static std::atomic<int> known[MMX_ZX4_MAXDEV];
    int dev = 0, cus = 0, wgs = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (dev >= 0 && dev < MMX_ZX4_MAXDEV && known[dev].load(std::memory_order_relaxed) > 0) return known[dev].load(std::memory_order_relaxed);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&wgs, kernel, 256, 0) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    const int slots = cus * wgs * 4;
    if (dev >= 0 && dev < MMX_ZX4_MAXDEV && slots > 0) known[dev].store(slots, std::memory_order_relaxed);
    return slots;
}

template <int NKX, int LA>
int launch_zx6(const mmx_volume* vol, const mmx_block* d_blocks, const mmx_block* h_blocks, int n_blocks,
               const mmx_zx6_plan& plan, const mmx_taps_f32& tx, int radius, void* d_work, float qp, float qq, bool edge_global,
               int rows_forced, hipStream_t s)
{
    using cg = cls4<NKX, LA>;
    mmx_zx4_cfg cfg{};          // (every field the setup kernel reads has a value: qp = qq = 0 means float32 tiles)
    for (int k = 0; k <= MMX_MAX_RADIUS_FAST; ++k) { cfg.w0[k] = tx.w0[k]; cfg.w2[k] = tx.w2[k]; }
    cfg.radius = radius;
    // the pieces carry v / 2^16 of the widened voxel: skimage's img_as_float scale on top
    cfg.xscale = (float)mmx_voxel_xscale(vol->dtype);
    cfg.staged = 2;
    cfg.qp = qp; cfg.qq = qq;
    // two column tiles per wave (zx4_kernel's NTW): 16-bit tiles of integer voxels, 8 < radius <= 16; tile rows past
    // the block are not stored (the A/B runs of both: profiles/r04_zx_experiments.txt)
    const bool pair = NKX == 2 && LA == 1 && qp > 0.f && vol->dtype != MMX_F32;
    cfg.ntw = pair ? 2 : 1;
    zx_classes cl;
    if (!collect_classes(h_blocks, n_blocks, &cl)) return MMX_ERR_UNSUPPORTED;
    cfg.ncw = cl.ncw; cfg.ncz = cl.ncz; cfg.maxcol = cl.maxcol; cfg.maxu = cl.maxu;
    for (int j = 0; j < MMX_ZX4_MAXCLS; ++j) {
        cfg.wcls[j] = j < cl.ncw ? cl.wcls[j] : -1;
        cfg.zcls[j] = j < cl.ncz ? cl.zcls[j] : -1;
    }
    int max_waves = 0;
    for (int i = 0; i < n_blocks; ++i) {
        const mmx_block& b = h_blocks[i];
        if (!mmx_zx6_launch_accepts(vol, b.nz, b.nx, radius)) return MMX_ERR_UNSUPPORTED;       // single reflection
        const int ntx = (b.nx + 15) / 16;
        max_waves = std::max(max_waves, b.ny * (pair ? (ntx + 1) / 2 : ntx));
    }
    // the LDS form of the edge steps (16-bit tiles of integer voxels, radius > 8: the class of radius <= 8 would pay for
    // it with its fourth wave per SIMD -- 131 registers for 124): every depth class of the batch has to fit
    bool elds = NKX == 2 && !edge_global && qp > 0.f && vol->dtype != MMX_F32;
    for (int j = 0; j < cl.ncz; ++j) elds = elds && zx4_edges_fit<NKX, LA>(cl.zcls[j], radius);
    const int nx_entries = cfg.ncw * cfg.maxcol * NKX * 2;
    const int nz_entries = cfg.ncz * cfg.maxu * cg::NKZ * 2;
    const size_t xbytes = (size_t)nx_entries * 2 * 64 * sizeof(v4u);
    const size_t zbytes = (size_t)nz_entries * 2 * 64 * sizeof(v4u);
    if ((int64_t)(xbytes + zbytes) > plan.tab_bytes) return MMX_ERR_UNSUPPORTED;
    char* w = reinterpret_cast<char*>(d_work);
    v4u* xtab = reinterpret_cast<v4u*>(w + plan.tab_off);
    v4u* ztab = reinterpret_cast<v4u*>(w + plan.tab_off + xbytes);
    hipLaunchKernelGGL((zx4_setup<NKX, LA>), dim3((nx_entries + nz_entries + 3) / 4), dim3(256), 0, s, cfg, xtab, ztab);
    dim3 grid((((max_waves + 3) / 4) + 7) & ~7, n_blocks);        // (a multiple of 8: the XCD-aware order in the kernel)
    if (vol->dtype == MMX_F32) {
        if (qp > 0.f)          // (16-bit tiles: the caller's bounds cover the voxels' range, mmx_volume.value_range)
            hipLaunchKernelGGL((zx4_kernel<NKX, LA, float, true>), grid, dim3(256), 0, s,
                               reinterpret_cast<const float*>(w + plan.pack_off), plan.pack_stride / 2, (int64_t)0, d_blocks,
                               plan.tile_stride, reinterpret_cast<float*>(w), reinterpret_cast<float*>(w + plan.q_off),
                               xtab, ztab, cfg);
        else
            hipLaunchKernelGGL((zx4_kernel<NKX, LA, float, false>), grid, dim3(256), 0, s,
                               reinterpret_cast<const float*>(w + plan.pack_off), plan.pack_stride / 2, (int64_t)0, d_blocks,
                               plan.tile_stride, reinterpret_cast<float*>(w), reinterpret_cast<float*>(w + plan.q_off),
                               xtab, ztab, cfg);
    } else if (pair) {
        if constexpr (NKX == 2 && LA == 1) {
            if (elds) {
                // the row march: rows per wave of every block from the launch's size and the wave slots of the device
                std::vector<int32_t> rows(n_blocks), wpr(n_blocks), nr(n_blocks);
                for (int i = 0; i < n_blocks; ++i) { rows[i] = h_blocks[i].ny; wpr[i] = ((h_blocks[i].nx + 15) / 16 + 1) / 2; }
                zx4_rows_rule(n_blocks, rows.data(), wpr.data(), zx4_wave_slots((const void*)zx4_rows_kernel<NKX, LA, uint16_t, true, 2, true>),
                              rows_forced, nr.data());
                mmx_zx4_cfg_rows cfr;
                static_cast<mmx_zx4_cfg&>(cfr) = cfg;
                if (!zx4_rows_make(n_blocks, rows.data(), wpr.data(), nr.data(), &cfr.rows)) return MMX_ERR_UNSUPPORTED;
                // one row per wave in every block: the one-row kernel with its head / steady loop / tail, which the row
                // march's single loop does not match at one row (profiles/r20_zx_row_march.txt, section 4)
                if (*std::max_element(nr.begin(), nr.end()) == 1)
                    hipLaunchKernelGGL((zx4_kernel<NKX, LA, uint16_t, true, 2, true>), grid, dim3(256), 0, s,
                                       reinterpret_cast<const uint16_t*>(w + plan.pack_off), plan.pack_stride, (int64_t)0, d_blocks,
                                       plan.tile_stride, reinterpret_cast<float*>(w), reinterpret_cast<float*>(w + plan.q_off),
                                       xtab, ztab, cfg);
                else
                    hipLaunchKernelGGL((zx4_rows_kernel<NKX, LA, uint16_t, true, 2, true>), dim3(cfr.rows.total), dim3(256), 0, s,
                                       reinterpret_cast<const uint16_t*>(w + plan.pack_off), plan.pack_stride, (int64_t)0, d_blocks,
                                       plan.tile_stride, reinterpret_cast<float*>(w), reinterpret_cast<float*>(w + plan.q_off),
                                       xtab, ztab, cfr);
            } else
                hipLaunchKernelGGL((zx4_kernel<NKX, LA, uint16_t, true, 2>), grid, dim3(256), 0, s,
                                   reinterpret_cast<const uint16_t*>(w + plan.pack_off), plan.pack_stride, (int64_t)0, d_blocks,
                                   plan.tile_stride, reinterpret_cast<float*>(w), reinterpret_cast<float*>(w + plan.q_off),
                                   xtab, ztab, cfg);
        }
    } else if (qp > 0.f) {
        if constexpr (!(NKX == 2 && LA == 1)) {      // (that class runs pairs)
            if constexpr (NKX == 2) if (elds)
                hipLaunchKernelGGL((zx4_kernel<NKX, LA, uint16_t, true, 1, true>), grid, dim3(256), 0, s,
                                   reinterpret_cast<const uint16_t*>(w + plan.pack_off), plan.pack_stride, (int64_t)0, d_blocks,
                                   plan.tile_stride, reinterpret_cast<float*>(w), reinterpret_cast<float*>(w + plan.q_off),
                                   xtab, ztab, cfg);
            if (!elds)
                hipLaunchKernelGGL((zx4_kernel<NKX, LA, uint16_t, true>), grid, dim3(256), 0, s,
                                   reinterpret_cast<const uint16_t*>(w + plan.pack_off), plan.pack_stride, (int64_t)0, d_blocks,
                                   plan.tile_stride, reinterpret_cast<float*>(w), reinterpret_cast<float*>(w + plan.q_off),
                                   xtab, ztab, cfg);
        }
    } else
        hipLaunchKernelGGL((zx4_kernel<NKX, LA, uint16_t, false>), grid, dim3(256), 0, s,
                           reinterpret_cast<const uint16_t*>(w + plan.pack_off), plan.pack_stride, (int64_t)0, d_blocks,
                           plan.tile_stride, reinterpret_cast<float*>(w), reinterpret_cast<float*>(w + plan.q_off),
                           xtab, ztab, cfg);
    return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
}

}  // namespace

int mmx_zx_rows_schedule(int n_blocks, const int32_t* rows, const int32_t* waves_per_row, int slots, int forced,
                         int32_t* nr, int32_t* cover)
{
    if (n_blocks < 1 || !rows || !waves_per_row || !nr || forced < 0 || forced > 15) return -MMX_ERR_ARG;
    if (slots < 0) slots = zx4_wave_slots((const void*)zx4_rows_kernel<2, 1, uint16_t, true, 2, true>);      // (the current device's)
    for (int b = 0; b < n_blocks; ++b) if (rows[b] < 1 || waves_per_row[b] < 1) return -MMX_ERR_ARG;
    zx4_rows_rule(n_blocks, rows, waves_per_row, slots, forced, nr);
    zx4_rows_sched s;
    if (!zx4_rows_make(n_blocks, rows, waves_per_row, nr, &s)) return -MMX_ERR_UNSUPPORTED;
    if (cover) {
        std::vector<int64_t> first(n_blocks + 1, 0);
        for (int b = 0; b < n_blocks; ++b) first[b + 1] = first[b] + (int64_t)rows[b] * waves_per_row[b];
        for (int64_t i = 0; i < first[n_blocks]; ++i) cover[i] = 0;
        // every wave of every workgroup, placed as zx4_kernel places itself
        for (int flat = 0; flat < s.total; ++flat) {
            const zx4_rows_place p = zx4_rows_decode(s, flat);
            if (p.block < 0 || p.block >= n_blocks) return -MMX_ERR_ARG;
            const int bx = (p.wx & 7) * (p.wgs >> 3) + (p.wx >> 3);
            for (int wv = 0; wv < 4; ++wv) {
                const int gw = bx * 4 + wv, ntp = waves_per_row[p.block];
                const int y = (gw / ntp) * p.n, col = gw % ntp;
                for (int r = y; r < y + p.n && r < rows[p.block]; ++r) cover[first[p.block] + (int64_t)r * ntp + col]++;
            }
        }
    }
    return s.total;
}

int mmx_zx6_plan_make(const mmx_block* h_blocks, int n_blocks, int64_t slot_elems, int voxel_dtype, mmx_zx6_plan* plan)
{
    if (!mmx_voxel(voxel_dtype)) return MMX_ERR_UNSUPPORTED;
    const int pieces = mmx_voxel(voxel_dtype)->pieces;        // float voxels: two float16 pieces per voxel in the copy
    int64_t tile = 0, pk = 0;
    int max_tiles = 0, max_rowtiles = 0;
    zx_classes cl;
    if (!collect_classes(h_blocks, n_blocks, &cl)) return MMX_ERR_UNSUPPORTED;
    for (int i = 0; i < n_blocks; ++i) {
        const mmx_block& b = h_blocks[i];
        const int ntx = (b.nx + 15) / 16, ntz = (b.nz + 15) / 16, nch8 = (b.nx + 7) / 8;
        const int64_t te = (int64_t)ntx * ntz * b.ny * 256, pe = (int64_t)b.ny * ntz * nch8 * 128 * pieces;
        if (te > tile) tile = te;
        if (pe > pk) pk = pe;
        if (ntx * ntz > max_tiles) max_tiles = ntx * ntz;
        if (b.ny * ntz > max_rowtiles) max_rowtiles = b.ny * ntz;
    }
    if (tile * 4 >= (int64_t(1) << 31) || pk * 2 >= (int64_t(1) << 31)) return MMX_ERR_UNSUPPORTED;   // 32-bit offsets in a block
    plan->tile_stride = tile;
    plan->pack_stride = pk;
    plan->q_off = (int64_t)n_blocks * tile * 4;
    plan->tab_off = 2 * plan->q_off;
    // room for the largest tables any radius class needs: widths x columns x 2 k-steps, depths x z tiles x 3 (every class
    // has two since radius 17 .. 24 took its split tile; the workspace layout stays as it was), two kernels each
    plan->tab_bytes = (int64_t)(cl.ncw * cl.maxcol * 2 * 2 + cl.ncz * cl.maxu * 3 * 2) * 2 * 64 * 16;
    plan->pack_off = (plan->tab_off + plan->tab_bytes + 255) & ~int64_t(255);
    plan->max_tiles = max_tiles;
    plan->max_rowtiles = max_rowtiles;
    const int64_t need = plan->pack_off + (int64_t)n_blocks * pk * 2;
    return need <= 4 * (int64_t)n_blocks * slot_elems * 4 ? MMX_OK : MMX_ERR_UNSUPPORTED;
}

int mmx_launch_zx6_pack(const mmx_volume* vol, const mmx_block* d_blocks, const mmx_block* h_blocks, int n_blocks,
                        const mmx_zx6_plan& plan, void* d_work, hipStream_t stream)
{
    uint16_t* pack = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(d_work) + plan.pack_off);
    dim3 grid(plan.max_rowtiles, n_blocks);
    // rows beyond one LDS panel of 512 columns anywhere in the batch: the panelled kernels for all of it
    bool wide = false;
    for (int i = 0; i < n_blocks; ++i) wide = wide || h_blocks[i].nx > 512;
    auto launch = [&](auto kernel, auto* data) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, data, vol->stride_z, vol->stride_y, vol->stride_x, d_blocks, pack,
                           plan.pack_stride);
        return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
    };
    return mmx_for_voxel<MMX_VOX_LOG>(vol->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
        using T = MMX_TAG_T(t);
        if constexpr (std::is_same<T, float>::value)       // (two float16 pieces per voxel: a kernel of its own)
            return wide ? launch(zx6_pack_f32_kernel<true>, (const T*)vol->d_data) : launch(zx6_pack_f32_kernel<false>, (const T*)vol->d_data);
        else
            return wide ? launch(zx6_pack_kernel<T, true>, (const T*)vol->d_data) : launch(zx6_pack_kernel<T, false>, (const T*)vol->d_data);
    });
}

// qp, qq > 0: Q16 tiles (P qp in [0, 1], Q qq in [-1, 1]); 0: float32 tiles
int mmx_launch_zx6(const mmx_volume* vol, const mmx_block* d_blocks, const mmx_block* h_blocks, int n_blocks,
                   const mmx_zx6_plan& plan, const mmx_taps_f32& tx, int radius, void* d_work, float qp, float qq,
                   bool edge_global, int rows, hipStream_t stream)
{
    if (!mmx_ring_radius(radius) || !mmx_voxels_ok(vol)) return MMX_ERR_UNSUPPORTED;
    if (radius <= 8) return launch_zx6<1, 1>(vol, d_blocks, h_blocks, n_blocks, plan, tx, radius, d_work, qp, qq, edge_global, rows, stream);
    if (radius <= 16) return launch_zx6<2, 1>(vol, d_blocks, h_blocks, n_blocks, plan, tx, radius, d_work, qp, qq, edge_global, rows, stream);
    return launch_zx6<2, 2>(vol, d_blocks, h_blocks, n_blocks, plan, tx, radius, d_work, qp, qq, edge_global, rows, stream);
}

