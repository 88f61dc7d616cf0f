// Wide-radius LoG passes: kernel radii 1 .. MMX_MAX_RADIUS_WIDE (64), i.e. the sigmas of fine-resolution images that the
// register-resident kernels (radius <= MMX_MAX_RADIUS_FAST) do not take.  Same separable LoG as every other path
// (scipy/ndimage/_filters.py:644-707 in float32 with fmaf), in the order Z, X, Y over the four slot arrays of d_work:
//
//   wide_z :  I (u8 / u16 / f32)  ->  Gz = G(z) I,  Gzz = G''(z) I                          (slots 2, 3)
//   wide_x :  (Gz, Gzz)           ->  P = G(x) Gz,  Q = G''(x) Gz + G(x) Gzz                (slots 0, 1)
//   wide_y :  (P, Q)              ->  LoG = -s^2 (G''(y) P + G(y) Q), NMS row entries       (d_log, d_nms_mask)
//
// One form for the three: a workgroup stages the T + 2 R inputs of its tile along the filter axis in LDS once (converted
// to float32, the single reflection applied while staging: every extent is >= R), and every thread then produces a run
// of J = 8 consecutive outputs along that axis from ONE LDS read per staged input.  Input i of a run feeds output j with
// the tap i - j of the full symmetric kernel, which is stored with J - 1 zeros either side: per step of J inputs the
// 2 J - 1 taps in reach are wave-uniform (scalar registers, read from the kernarg segment with a uniform index) and the
// inner J x J block is fully unrolled.  LDS reads per output: (J + 2 R) / J instead of the 2 R + 1 L1 loads of the
// generic passes; arithmetic per voxel and sigma: about 7 (J + 2 R) FMA (Z and Y one packed FMA per tap on the
// pairs (Gz, Gzz) / (P, Q), X one packed and one scalar).
//   Z, Y : lanes along x -- a column is one voxel of the flattened (y, x) / (z, x) plane, 64 columns per workgroup --
//          and the 8 waves of a workgroup own 8 consecutive runs: a tile is 64 outputs, staged as rows of 64 floats
//          (pairs for Y): lane-contiguous reads, no bank conflicts;
//   X    : the filter axis is the lane axis, so a thread's run is 8 consecutive x of one row: rows are staged as
//          (Gz, Gzz) pairs with one pad pair after every 32 (position p at p + (p >> 5)): the 8-byte reads of a half
//          wave at a lane stride of 8 pairs then fall on 32 distinct 8-byte bank slots.  A workgroup takes as many rows
//          as give its 256 threads one run each (a row of 261 voxels: 7 rows of 33 runs), and x tiles of 512 outputs,
//          so any row width goes;
//   Y    : runs last and writes the MMX_MASK_ROWS entries (mmx_entries.h) -- a
//          workgroup's 64 columns are one entry per row --, and leaves 64-voxel segments with nothing above the
//          threshold unwritten.  The y neighbours of a run's first and last output come from the neighbouring waves
//          through LDS; a tile's own first and last row are not tested against the next tile (word 0 stays a superset).

#include "mmx_device.h"

namespace {

constexpr int kJ = 8;                 // outputs per thread along the filter axis
constexpr int kOff = 8;               // zeros ahead of tap 0 in the padded kernel (>= kJ - 1)
constexpr int kRuns = 8;              // Z / Y: runs (waves) per workgroup
constexpr int kTile = kJ * kRuns;     // Z / Y: outputs per tile
constexpr int kColThreads = 64 * kRuns;
constexpr int kXThreads = 256;
constexpr int kXTile = 64 * kJ;       // X: outputs of one x tile
constexpr int kXMaxRows = 16;
// padded full kernel: taps 0 .. 2 R at kOff .., zeros elsewhere; the last step reads up to kOff + steps(R) * kJ + kJ - 2
constexpr int kTaps = kOff + 2 * MMX_MAX_RADIUS_WIDE + 3 * kJ;

struct wide_taps {
    v2f a[kTaps];       // Z: (w0, w2) x input scale;  X: (w0, w0);  Y: (w2, w0) x -norm
    float b[kTaps];     // X: w2
};

// inputs a run reads: J + 2 R rounded up to whole steps of J
__host__ __device__ constexpr int run_inputs(int R) { return (kJ + 2 * R + kJ - 1) / kJ * kJ; }

// ---------------------------------------------------------------- Z
template <typename InT>
__global__ void __launch_bounds__(kColThreads)
wide_z(const InT* __restrict__ vol, int64_t stride_z, int64_t stride_y, int64_t stride_x,
       const mmx_block* __restrict__ blocks, int64_t slot_elems, int R, int ntile_max,
       float* __restrict__ gz, float* __restrict__ gzz, wide_taps T)
{
    extern __shared__ float stage[];            // [kTile - kJ + run_inputs(R)][64]
    const mmx_block bd = blocks[blockIdx.y];
    const int cg = blockIdx.x / ntile_max, zt = blockIdx.x - cg * ntile_max;
    const int ncol = bd.ny * bd.px;
    const int z0 = zt * kTile;
    if (cg * 64 >= ncol || z0 >= bd.nz) return;             // whole workgroup
    const int lane = threadIdx.x & 63;
    const int run = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int col = cg * 64 + lane;
    const bool col_on = col < ncol;
    const int cc = col_on ? col : ncol - 1;
    const int y = cc / bd.px, x = cc - y * bd.px;
    const int xl = x < bd.nx ? x : bd.nx - 1;               // pitch columns re-read the last voxel of the row
    const InT* in = vol + bd.src_off + (int64_t)y * stride_y + (int64_t)xl * stride_x;
    const int NI = run_inputs(R);
    const int nstage = kTile - kJ + NI;
    for (int r = run; r < nstage; r += kRuns)
        stage[r * 64 + lane] = mmx_vox<InT>::of(in[(int64_t)reflect_clamped(z0 - R + r, bd.nz) * stride_z]);
    __syncthreads();
    const int zr = z0 + run * kJ;                           // first output of this wave's run
    if (zr >= bd.nz) return;                                // (no barrier below)
    v2f acc[kJ];
#pragma unroll
    for (int j = 0; j < kJ; ++j) acc[j] = (v2f){0.f, 0.f};
    const float* src = stage + run * kJ * 64 + lane;
#pragma unroll 1
    for (int c = 0; c < NI; c += kJ) {
        float v[kJ];
#pragma unroll
        for (int u = 0; u < kJ; ++u) v[u] = src[(c + u) * 64];
#pragma unroll
        for (int u = 0; u < kJ; ++u)
#pragma unroll
            for (int j = 0; j < kJ; ++j)
                acc[j] = __builtin_elementwise_fma((v2f){v[u], v[u]}, T.a[kOff + c + u - j], acc[j]);
    }
    if (!col_on) return;
    const int64_t o = (int64_t)bd.slot * slot_elems + (int64_t)zr * ncol + col;
#pragma unroll
    for (int j = 0; j < kJ; ++j)
        if (zr + j < bd.nz) {
            gz[o + (int64_t)j * ncol] = acc[j].x;
            gzz[o + (int64_t)j * ncol] = acc[j].y;
        }
}

// ---------------------------------------------------------------- X
__host__ __device__ __forceinline__ int x_pad(int p) { return p + (p >> 5); }
// runs per row of an x tile / rows per workgroup of a block nx wide
__host__ __device__ __forceinline__ int x_runs(int nx) { const int c = (nx + kJ - 1) / kJ; return c < 64 ? c : 64; }
__host__ __device__ __forceinline__ int x_rows(int nx)
{
    const int r = kXThreads / x_runs(nx);
    return r < kXMaxRows ? r : kXMaxRows;
}
// staged pairs of one row: the runs' inputs, padded
__host__ __device__ __forceinline__ int x_row_pitch(int nx, int R) { return x_pad(x_runs(nx) * kJ - kJ + run_inputs(R)) + 1; }

__global__ void __launch_bounds__(kXThreads)
wide_x(const mmx_block* __restrict__ blocks, int64_t slot_elems, int R,
       const float* __restrict__ gz, const float* __restrict__ gzz,
       float* __restrict__ gp, float* __restrict__ gq, wide_taps T)
{
    extern __shared__ v2f rows[];               // [x_rows][x_row_pitch]
    const mmx_block bd = blocks[blockIdx.y];
    const int nxt = (bd.nx + kXTile - 1) / kXTile;
    const int CH = x_runs(bd.nx), RW = x_rows(bd.nx);
    const int nrows = bd.nz * bd.ny;
    const int grp = blockIdx.x / nxt, xt = blockIdx.x - grp * nxt;
    const int row0 = grp * RW;
    if (row0 >= nrows) return;                  // whole workgroup
    const int x0 = xt * kXTile;
    const int NI = run_inputs(R);
    const int span = CH * kJ - kJ + NI;         // staged positions of a row: x0 - R ..
    const int pitch = x_row_pitch(bd.nx, R);
    const int64_t sbase = (int64_t)bd.slot * slot_elems;
    const int t = threadIdx.x;
    for (int r = 0; r < RW; ++r) {
        const int row = row0 + r < nrows ? row0 + r : nrows - 1;
        const int64_t rb = sbase + (int64_t)row * bd.px;
        for (int p = t; p < span; p += kXThreads) {
            const int xs = reflect_clamped(x0 - R + p, bd.nx);
            rows[r * pitch + x_pad(p)] = (v2f){gz[rb + xs], gzz[rb + xs]};
        }
    }
    __syncthreads();
    const int r = t / CH, c = t - r * CH;
    const int xo = x0 + c * kJ;                 // first output of this thread's run
    if (r >= RW || row0 + r >= nrows || xo >= bd.nx) return;
    v2f ps[kJ];                                 // (G(x) Gz, G(x) Gzz)
    float q[kJ];                                // G''(x) Gz
#pragma unroll
    for (int j = 0; j < kJ; ++j) { ps[j] = (v2f){0.f, 0.f}; q[j] = 0.f; }
    const v2f* src = rows + r * pitch;
    const int p0 = c * kJ;
#pragma unroll 1
    for (int s = 0; s < NI; s += kJ) {
        v2f v[kJ];
#pragma unroll
        for (int u = 0; u < kJ; ++u) v[u] = src[x_pad(p0 + s + u)];
#pragma unroll
        for (int u = 0; u < kJ; ++u)
#pragma unroll
            for (int j = 0; j < kJ; ++j) {
                ps[j] = __builtin_elementwise_fma(v[u], T.a[kOff + s + u - j], ps[j]);
                q[j] = fmaf(v[u].x, T.b[kOff + s + u - j], q[j]);
            }
    }
    // (a run of 8 from a multiple of 8 below nx lies inside the row pitch, a multiple of 32)
    const int64_t o = sbase + (int64_t)(row0 + r) * bd.px + xo;
    *reinterpret_cast<float4*>(gp + o) = make_float4(ps[0].x, ps[1].x, ps[2].x, ps[3].x);
    *reinterpret_cast<float4*>(gp + o + 4) = make_float4(ps[4].x, ps[5].x, ps[6].x, ps[7].x);
    *reinterpret_cast<float4*>(gq + o) = make_float4(ps[0].y + q[0], ps[1].y + q[1], ps[2].y + q[2], ps[3].y + q[3]);
    *reinterpret_cast<float4*>(gq + o + 4) = make_float4(ps[4].y + q[4], ps[5].y + q[5], ps[6].y + q[6], ps[7].y + q[7]);
}

// ---------------------------------------------------------------- Y
template <bool MASK>
__global__ void __launch_bounds__(kColThreads)
wide_y(const mmx_block* __restrict__ blocks, int64_t slot_elems, int R, int ntile_max,
       const float* __restrict__ gp, const float* __restrict__ gq, float* __restrict__ out, wide_taps T,
       unsigned long long* __restrict__ mask, float nms_lo, float nms_eps)
{
    extern __shared__ v2f stage2[];             // [kTile - kJ + run_inputs(R)][64] pairs, then the runs' edge values
    const mmx_block bd = blocks[blockIdx.y];
    const int cg = blockIdx.x / ntile_max, yt = blockIdx.x - cg * ntile_max;
    const int ncol = bd.nz * bd.px;
    const int y0 = yt * kTile;
    if (cg * 64 >= ncol || y0 >= bd.ny) return;             // whole workgroup
    const int lane = threadIdx.x & 63;
    const int run = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int col = cg * 64 + lane;
    const bool col_on = col < ncol;
    const int cc = col_on ? col : ncol - 1;
    const int z = cc / bd.px, x = cc - z * bd.px;
    const int64_t sbase = (int64_t)bd.slot * slot_elems;
    const int64_t cbase = sbase + (int64_t)z * bd.ny * bd.px + x;      // row 0 of this voxel's column
    const int NI = run_inputs(R);
    const int nstage = kTile - kJ + NI;
    for (int r = run; r < nstage; r += kRuns) {
        const int64_t i = cbase + (int64_t)reflect_clamped(y0 - R + r, bd.ny) * bd.px;
        stage2[r * 64 + lane] = (v2f){gp[i], gq[i]};
    }
    __syncthreads();
    const int yr = y0 + run * kJ;                           // first output of this wave's run
    const bool run_on = yr < bd.ny;                         // (wave-uniform; every wave stays for the barrier below)
    v2f acc[kJ];
#pragma unroll
    for (int j = 0; j < kJ; ++j) acc[j] = (v2f){0.f, 0.f};
    if (run_on) {
        const v2f* src = stage2 + run * kJ * 64 + lane;
#pragma unroll 1
        for (int c = 0; c < NI; c += kJ) {
            v2f v[kJ];
#pragma unroll
            for (int u = 0; u < kJ; ++u) v[u] = src[(c + u) * 64];
#pragma unroll
            for (int u = 0; u < kJ; ++u)
#pragma unroll
                for (int j = 0; j < kJ; ++j)
                    acc[j] = __builtin_elementwise_fma(v[u], T.a[kOff + c + u - j], acc[j]);
        }
    }
    const bool real = col_on && x < bd.nx;
    float val[kJ];           // (pitch columns: the X pass leaves those of P and Q unwritten; the cube holds 0 there)
#pragma unroll
    for (int j = 0; j < kJ; ++j) val[j] = real ? acc[j].x + acc[j].y : 0.f;
    if constexpr (!MASK) {
        if (!run_on || !col_on) return;
#pragma unroll
        for (int j = 0; j < kJ; ++j)
            if (yr + j < bd.ny) out[cbase + (int64_t)(yr + j) * bd.px] = val[j];
    } else {
        // the y neighbours across runs: every wave leaves its first and last output for the waves beside it
        float* edge = reinterpret_cast<float*>(stage2 + nstage * 64);      // [kRuns][2][64]
        edge[(run * 2 + 0) * 64 + lane] = val[0];
        edge[(run * 2 + 1) * 64 + lane] = val[kJ - 1];
        __syncthreads();
        if (!run_on) return;
        const bool has_below = run > 0, has_above = run + 1 < kRuns && yr + kJ < bd.ny;
        const float below = has_below ? edge[((run - 1) * 2 + 1) * 64 + lane] : -INFINITY;
        const float above = has_above ? edge[((run + 1) * 2 + 0) * 64 + lane] : -INFINITY;
        const bool has_l = lane > 0 && x > 0, has_r = lane < 63 && x + 1 < bd.nx && col + 1 < ncol;
        const mmx_entry_geom eg = mmx_entry_geom_make(MMX_MASK_ROWS, bd.nz, bd.nx, bd.px);
        const int nwords = eg.per_row;
        ulonglong2* mrow = reinterpret_cast<ulonglong2*>(mask) + mmx_entry_base(bd.slot, slot_elems) +
                           mmx_rows_entry(col) + (int64_t)yr * nwords;
#pragma unroll
        for (int j = 0; j < kJ; ++j) {
            if (yr + j >= bd.ny) break;                     // (wave-uniform)
            const float v = val[j];
            const unsigned long long ab = mmx_above_word(real, v, nms_lo);
            unsigned long long m = 0;
            if (ab) {
                if (col_on) out[cbase + (int64_t)(yr + j) * bd.px] = v;
                const float l = __shfl_up(v, 1), rr = __shfl_down(v, 1);
                float nb = fmaxf(has_l ? l : -INFINITY, has_r ? rr : -INFINITY);
                nb = fmaxf(nb, j > 0 ? val[j > 0 ? j - 1 : 0] : below);
                // (a neighbour past the block's last row is no neighbour: its value here is one of a row never stored)
                nb = fmaxf(nb, yr + j + 1 >= bd.ny ? -INFINITY : (j + 1 < kJ ? val[j + 1 < kJ ? j + 1 : 0] : above));
                m = __ballot(mmx_candidate(real, v, nms_lo, nms_eps, nb));
            }
            if (lane == 0) mrow[(int64_t)j * nwords] = make_ulonglong2(m, ab);
        }
    }
}

void fill_taps(wide_taps* T, int R, const float* a0, const float* a1, const float* b)
{
    for (int i = 0; i < kTaps; ++i) {
        const int t = i - kOff;
        const bool on = t >= 0 && t <= 2 * R;
        const int k = t < R ? R - t : t - R;
        T->a[i] = on ? (v2f){a0[k], a1[k]} : (v2f){0.f, 0.f};
        T->b[i] = on && b ? b[k] : 0.f;
    }
}

}  // namespace

// pass 0 = Z (in: the volume; out1, out2: Gz, Gzz), 1 = X (in1, in2 -> out1, out2: P, Q), 2 = Y (in1, in2: P, Q -> out1:
// the LoG array; d_mask: the row entries, or NULL).  w0 / w2: half kernels of that pass, already scaled.
int mmx_launch_wide_pass(int pass, const mmx_volume* vol, const mmx_block* d_blocks, const mmx_block* h_blocks, int n_blocks,
                         int64_t slot_elems, const float* w0, const float* w2, int radius,
                         const float* in1, const float* in2, float* out1, float* out2,
                         unsigned long long* d_mask, float nms_lo, float nms_eps, hipStream_t s)
{
    if (!mmx_wide_launch_accepts(vol, radius)) return MMX_ERR_UNSUPPORTED;
    const int R = radius;
    static_assert(kOff >= kJ - 1 && kTaps >= kOff + run_inputs(MMX_MAX_RADIUS_WIDE) + kJ - 1, "padded kernel too short");
    wide_taps T;
    const int nstage = kTile - kJ + run_inputs(R);
    if (pass == 1) {
        fill_taps(&T, R, w0, w0, w2);
        int64_t groups = 0;
        size_t lds = 0;
        for (int i = 0; i < n_blocks; ++i) {
            const mmx_block& b = h_blocks[i];
            const int rw = x_rows(b.nx);
            const int64_t n = ((int64_t)b.nz * b.ny + rw - 1) / rw * ((b.nx + kXTile - 1) / kXTile);
            if (n > groups) groups = n;
            const size_t bytes = (size_t)rw * x_row_pitch(b.nx, R) * sizeof(v2f);
            if (bytes > lds) lds = bytes;
        }
        if (groups > MMX_MAX_GRID_X || lds > 64 * 1024) return MMX_ERR_UNSUPPORTED;
        hipLaunchKernelGGL(wide_x, dim3((unsigned)groups, n_blocks), dim3(kXThreads), lds, s, d_blocks, slot_elems, R,
                           in1, in2, out1, out2, T);
        return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
    }
    // Z / Y: 64 columns of the plane across the filter axis x tiles of kTile outputs along it
    int64_t max_cols = 0;
    int max_n = 0;
    for (int i = 0; i < n_blocks; ++i) {
        const mmx_block& b = h_blocks[i];
        const int64_t cols = (int64_t)(pass == 0 ? b.ny : b.nz) * b.px;
        const int n = pass == 0 ? b.nz : b.ny;
        if (cols > max_cols) max_cols = cols;
        if (n > max_n) max_n = n;
    }
    const int ntile = (max_n + kTile - 1) / kTile;
    const int64_t gx = (max_cols + 63) / 64 * ntile;
    if (gx > MMX_MAX_GRID_X) return MMX_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)gx, n_blocks);
    if (pass == 0) {
        fill_taps(&T, R, w0, w2, nullptr);
        const size_t lds = (size_t)nstage * 64 * sizeof(float);
        return mmx_for_voxel<MMX_VOX_LOG>(vol->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
            using V = MMX_TAG_T(t);
            hipLaunchKernelGGL((wide_z<V>), grid, dim3(kColThreads), lds, s, (const V*)vol->d_data, vol->stride_z,
                               vol->stride_y, vol->stride_x, d_blocks, slot_elems, R, ntile, out1, out2, T);
            return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
        });
    } else {
        fill_taps(&T, R, w2, w0, nullptr);
        const size_t lds = (size_t)nstage * 64 * sizeof(v2f) + (size_t)kRuns * 2 * 64 * sizeof(float);
        if (d_mask)
            hipLaunchKernelGGL((wide_y<true>), grid, dim3(kColThreads), lds, s, d_blocks, slot_elems, R, ntile, in1, in2,
                               out1, T, d_mask, nms_lo, nms_eps);
        else
            hipLaunchKernelGGL((wide_y<false>), grid, dim3(kColThreads), lds, s, d_blocks, slot_elems, R, ntile, in1, in2,
                               out1, T, d_mask, nms_lo, nms_eps);
    }
    return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
}
