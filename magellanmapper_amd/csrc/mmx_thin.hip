// The folded-reflection passes of MMX_ZX_THIN: the separable LoG passes along an axis that is SHORTER than the kernel.
//
// The generic passes (mmx_generic.hip) read 2 R + 1 reflected taps per output and compute the reflection per tap, from an
// axis that holds only n distinct values -- for a 2-D image (n = 1) that is 2 R + 1 loads of one voxel.  SciPy's
// "reflect" folds those taps onto the n voxels of the axis, so the pass is a dense n x n matrix per order (M0 from the
// order-0 weights, M2 from the order-2 ones: mmx_fold.h) and an output is n multiply-adds per array instead of 2 R + 1:
//   Z: Gz = M0 v, Gzz = M2 v      Y: A = M0 Gz, BC = M2 Gz + M0 Gzz      X: LoG = M2 A + M0 BC
// (the arrays of the generic passes, float32 FMAs, no matrix cores).
//
// One kernel template over the axis.  A workgroup serves one block at a time: it builds the block's two matrices in LDS
// once (2 x 68^2 floats at the most, 37 KB), then takes units of L lines of the axis -- lines that are consecutive in
// memory (consecutive x for the Z and Y passes, consecutive rows for the X pass), so every global access runs along x; L
// is what the LDS tile holds of the block's n: 32 lines at n = 68, 1024 at n = 1 --, stages their n values in LDS and
// computes the L n outputs.  Matrix entries are stored [j][i]: the lanes of a wave that share an output index i
// broadcast, those with consecutive i read consecutive banks; the staged lines have an odd pitch.  A block whose extent
// along the axis exceeds MMX_FOLD_MAX_N runs the tap loop of the generic pass (mmx_taploop.h) and gets its bits: the
// call is total.

#include "mmx_taploop.h"
#include "mmx_fold.h"

// floats of LDS that hold the staged lines of a unit, per input array: 68 lines' worth of 47 values and more for shorter axes
#define MMX_FOLD_TILE 3200
// most lines of a unit
#define MMX_FOLD_MAX_LINES 1024
// outputs a workgroup is launched for (the grid; it strides over whatever its block holds)
#define MMX_FOLD_WG_OUTPUTS 2048

namespace {

constexpr int kMat = MMX_FOLD_MAX_N * MMX_FOLD_MAX_N, kTaps = MMX_MAX_RADIUS_GENERIC + 1;
static_assert((2 * kTaps + 2 * kMat + 2 * MMX_FOLD_TILE) * sizeof(float) <= MMX_LDS_BYTES, "the fold's LDS image");
static_assert(MMX_FOLD_MAX_N * (32 + 1) <= MMX_FOLD_TILE, "32 lines of the longest axis fit the tile");

template <int AX>
__global__ void __launch_bounds__(MMX_WG)
fold_kernel(mmx_volume vol, const mmx_block* __restrict__ blocks, int64_t slot_elems, int R,
            const float* __restrict__ in1, const float* __restrict__ in2, float* __restrict__ out1,
            float* __restrict__ out2, mmx_taps_generic t)
{
    const mmx_block bd = blocks[blockIdx.y];
    const int n = AX == 0 ? bd.nz : (AX == 1 ? bd.ny : bd.nx);
    const int tid = threadIdx.x;
    if (n > MMX_FOLD_MAX_N) {           // (uniform over the workgroup) too long to fold: the generic pass's tap loop
        const int first = blockIdx.x * MMX_WG + tid, step = gridDim.x * MMX_WG;
        if (AX == 0) mmx_taploop_z(vol, bd, slot_elems, R, out1, out2, t, first, step);
        else if (AX == 1) mmx_taploop_y(bd, slot_elems, R, in1, in2, out1, out2, t, first, step);
        else mmx_taploop_x(bd, slot_elems, R, in1, in2, out1, t, first, step);
        return;
    }
    // The lines of the axis, numbered so that consecutive lines are consecutive in memory: Z: (y, x) over the pitched
    // plane ny * px; Y: (z, x) over nz * px; X: the rows (z, y).  (Pitch columns x >= nx are lines that do nothing.)
    // A unit is L of them: as many as the tile holds of this block's n, a multiple of 32, with an odd pitch L + 1.
    const int lines = AX == 0 ? bd.ny * bd.px : (AX == 1 ? bd.nz * bd.px : bd.nz * bd.ny);
    int L = (MMX_FOLD_TILE / n - 1) & ~31;
    if (L > MMX_FOLD_MAX_LINES) L = MMX_FOLD_MAX_LINES;
    const int pitch = L + 1;
    const int units = (lines + L - 1) / L;
    if ((int)blockIdx.x >= units) return;

    __shared__ float lds[2 * kTaps + 2 * kMat + 2 * MMX_FOLD_TILE];
    float* wl0 = lds;
    float* wl2 = wl0 + kTaps;
    float* mt0 = wl2 + kTaps;           // [j][i]: mt0[j * n + i] = M0[i][j]
    float* mt2 = mt0 + kMat;
    float* tile0 = mt2 + kMat;          // [j][line of the unit], pitch L + 1
    float* tile1 = tile0 + MMX_FOLD_TILE;
    for (int k = tid; k <= R; k += MMX_WG) { wl0[k] = t.w0[k]; wl2[k] = t.w2[k]; }
    __syncthreads();
    for (int e = tid; e < n * n; e += MMX_WG) {
        const int j = e / n, i = e - j * n;
        mt0[e] = mmx_fold_entry(wl0, R, n, i, j);
        mt2[e] = mmx_fold_entry(wl2, R, n, i, j);
    }
    const int64_t base = (int64_t)bd.slot * slot_elems;
    const int total = L * n;
    const int64_t wstep = (int64_t)bd.ny * bd.px;           // (Z: from one plane to the next)
    for (int u = blockIdx.x; u < units; u += gridDim.x) {
        const int l0 = u * L;
        __syncthreads();                // (the matrices are built; the tiles of the unit before have been read)
        for (int e = tid; e < total; e += MMX_WG) {
            int c, j;
            if (AX == 2) { c = e / n; j = e - c * n; } else { j = e / L; c = e - j * L; }
            const int l = l0 + c;
            if (l >= lines) continue;
            if (AX == 2) {
                const int64_t at = base + (int64_t)l * bd.px + j;
                tile0[j * pitch + c] = in1[at];
                tile1[j * pitch + c] = in2[at];
            } else {
                const int f = l / bd.px, x = l - f * bd.px;       // (Z: y; Y: z)
                if (x >= bd.nx) continue;
                if (AX == 0) {
                    tile0[j * pitch + c] = mmx_load_any(vol.d_data, vol.dtype, bd.src_off + (int64_t)j * vol.stride_z +
                                                        (int64_t)f * vol.stride_y + (int64_t)x * vol.stride_x);
                } else {
                    const int64_t at = base + ((int64_t)f * bd.ny + j) * bd.px + x;
                    tile0[j * pitch + c] = in1[at];
                    tile1[j * pitch + c] = in2[at];
                }
            }
        }
        __syncthreads();
        for (int o = tid; o < total; o += MMX_WG) {
            int c, i;
            if (AX == 2) { c = o / n; i = o - c * n; } else { i = o / L; c = o - i * L; }
            const int l = l0 + c;
            if (l >= lines) continue;
            int64_t at;
            if (AX == 2) at = base + (int64_t)l * bd.px + i;
            else {
                const int f = l / bd.px, x = l - f * bd.px;
                if (x >= bd.nx) continue;
                at = AX == 0 ? base + (int64_t)i * wstep + l : base + ((int64_t)f * bd.ny + i) * bd.px + x;
            }
            const float* m0 = mt0 + i;
            const float* m2 = mt2 + i;
            const float* v1 = tile0 + c;
            const float* v2 = tile1 + c;
            float a = 0.f, b = 0.f;
            if (AX == 0) {
                for (int j = 0; j < n; ++j) {
                    const float v = v1[j * pitch];
                    a = fmaf(v, m0[j * n], a);
                    b = fmaf(v, m2[j * n], b);
                }
                out1[at] = a;
                out2[at] = b;
            } else if (AX == 1) {
                for (int j = 0; j < n; ++j) {
                    const float g = v1[j * pitch], gg = v2[j * pitch], k0 = m0[j * n];
                    a = fmaf(g, k0, a);
                    b = fmaf(g, m2[j * n], b);
                    b = fmaf(gg, k0, b);
                }
                out1[at] = a;
                out2[at] = b;
            } else {
                for (int j = 0; j < n; ++j) {
                    a = fmaf(v1[j * pitch], m2[j * n], a);
                    a = fmaf(v2[j * pitch], m0[j * n], a);
                }
                out1[at] = a;
            }
        }
    }
}

}  // namespace

// pass: 0 = z, 1 = y, 2 = x; the arrays and the (already scaled) weights of mmx_launch_generic_pass.
int mmx_launch_fold_pass(int pass, const mmx_volume* vol, const mmx_block* d_blocks, int n_blocks,
                         int max_vox, int64_t slot_elems, const float* w0, const float* w2, int radius,
                         const float* in1, const float* in2, float* out1, float* out2, hipStream_t s)
{
    if (radius < 0 || radius > MMX_MAX_RADIUS_GENERIC || pass < 0 || pass > 2) return MMX_ERR_UNSUPPORTED;
    mmx_taps_generic t;
    for (int k = 0; k <= MMX_MAX_RADIUS_GENERIC; ++k) {
        t.w0[k] = k <= radius ? w0[k] : 0.f;
        t.w2[k] = k <= radius ? w2[k] : 0.f;
    }
    int gx = (max_vox + MMX_FOLD_WG_OUTPUTS - 1) / MMX_FOLD_WG_OUTPUTS;
    if (gx > 8192) gx = 8192;
    if (gx < 1) gx = 1;
    dim3 grid(gx, n_blocks);
    if (pass == 0)
        hipLaunchKernelGGL(fold_kernel<0>, grid, dim3(MMX_WG), 0, s, *vol, d_blocks, slot_elems, radius, in1, in2, out1, out2, t);
    else if (pass == 1)
        hipLaunchKernelGGL(fold_kernel<1>, grid, dim3(MMX_WG), 0, s, *vol, d_blocks, slot_elems, radius, in1, in2, out1, out2, t);
    else
        hipLaunchKernelGGL(fold_kernel<2>, grid, dim3(MMX_WG), 0, s, *vol, d_blocks, slot_elems, radius, in1, in2, out1, out2, t);
    return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
}

extern "C" {

int mmx_fold_matrix(const float* w, int radius, int n, float* out)
{
    if (!w || !out || radius < 0 || radius > MMX_MAX_RADIUS_GENERIC || n < 1) return MMX_ERR_ARG;
    mmx_fold_matrix_host(w, radius, n, out);
    return MMX_OK;
}

int mmx_col_prefetch(void) { return MMX_COL_PREFETCH; }

}  // extern "C"
