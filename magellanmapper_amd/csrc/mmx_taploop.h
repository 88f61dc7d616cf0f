// The tap loops of the generic separable passes, one thread per output voxel of ONE block: SciPy's "reflect" per tap
// (it may wrap several times), taps read through L1/L2, weights from the kernarg segment (uniform index -> scalar
// loads).  Shared by the generic kernels (mmx_generic.hip) and by the folded passes (mmx_thin.hip), which run them on
// the blocks they do not fold: one statement of the arithmetic, so both give the same bits.
#pragma once

#include "mmx_common.h"

struct mmx_taps_generic {
    float w0[MMX_MAX_RADIUS_GENERIC + 1];
    float w2[MMX_MAX_RADIUS_GENERIC + 1];
};

__device__ __forceinline__ float mmx_load_any(const void* base, int dtype, int64_t idx)
{
    return mmx_for_voxel<MMX_VOX_ALL, float>(dtype, 0.f, [&](auto t) { return mmx_vox<MMX_TAG_T(t)>::of(((const MMX_TAG_T(t)*)base)[idx]); });
}

// idx runs over the pitched block [nz][ny][px]; returns 0 past the end, 1 for a voxel, 2 for a
// pitch column (skipped)
__device__ __forceinline__ int mmx_locate(const mmx_block& bd, int idx, int& z, int& y, int& x)
{
    const int plane = bd.ny * bd.px;
    if (idx >= bd.nz * plane) return 0;
    z = idx / plane;
    const int rem = idx - z * plane;
    y = rem / bd.px;
    x = rem - y * bd.px;
    return x < bd.nx ? 1 : 2;
}

// The voxels first, first + step, ... of block bd (a grid-stride loop: first = blockIdx.x * MMX_WG + threadIdx.x, step =
// gridDim.x * MMX_WG).
__device__ __forceinline__ void mmx_taploop_z(const mmx_volume& vol, const mmx_block& bd, int64_t slot_elems, int R,
                                              float* __restrict__ gz, float* __restrict__ gzz, const mmx_taps_generic& t,
                                              int first, int step)
{
    for (int idx = first;; idx += step) {
        int z, y, x;
        const int where = mmx_locate(bd, idx, z, y, x);
        if (where == 0) return;
        if (where == 2) continue;
        const int64_t col = bd.src_off + (int64_t)y * vol.stride_y + (int64_t)x * vol.stride_x;
        const float c = mmx_load_any(vol.d_data, vol.dtype, col + (int64_t)z * vol.stride_z);
        float a0 = c * t.w0[0], a2 = c * t.w2[0];
        for (int k = 1; k <= R; ++k) {
            const float p = mmx_load_any(vol.d_data, vol.dtype, col + (int64_t)mmx_reflect(z - k, bd.nz) * vol.stride_z) +
                            mmx_load_any(vol.d_data, vol.dtype, col + (int64_t)mmx_reflect(z + k, bd.nz) * vol.stride_z);
            a0 = fmaf(p, t.w0[k], a0);
            a2 = fmaf(p, t.w2[k], a2);
        }
        const int64_t o = (int64_t)bd.slot * slot_elems + idx;
        gz[o] = a0;
        gzz[o] = a2;
    }
}

__device__ __forceinline__ void mmx_taploop_y(const mmx_block& bd, int64_t slot_elems, int R,
                                              const float* __restrict__ gz, const float* __restrict__ gzz,
                                              float* __restrict__ oa, float* __restrict__ obc, const mmx_taps_generic& t,
                                              int first, int step)
{
    for (int idx = first;; idx += step) {
        int z, y, x;
        const int where = mmx_locate(bd, idx, z, y, x);
        if (where == 0) return;
        if (where == 2) continue;
        const int64_t col = (int64_t)bd.slot * slot_elems + (int64_t)z * bd.ny * bd.px + x;
        const float c1 = gz[col + (int64_t)y * bd.px], c2 = gzz[col + (int64_t)y * bd.px];
        float a = c1 * t.w0[0];
        float bc = fmaf(c2, t.w0[0], c1 * t.w2[0]);
        for (int k = 1; k <= R; ++k) {
            const int64_t lo = col + (int64_t)mmx_reflect(y - k, bd.ny) * bd.px;
            const int64_t hi = col + (int64_t)mmx_reflect(y + k, bd.ny) * bd.px;
            const float p1 = gz[lo] + gz[hi];
            const float p2 = gzz[lo] + gzz[hi];
            a = fmaf(p1, t.w0[k], a);
            bc = fmaf(p1, t.w2[k], bc);
            bc = fmaf(p2, t.w0[k], bc);
        }
        const int64_t o = (int64_t)bd.slot * slot_elems + idx;
        oa[o] = a;
        obc[o] = bc;
    }
}

__device__ __forceinline__ void mmx_taploop_x(const mmx_block& bd, int64_t slot_elems, int R,
                                              const float* __restrict__ ga, const float* __restrict__ gbc,
                                              float* __restrict__ out, const mmx_taps_generic& t, int first, int step)
{
    for (int idx = first;; idx += step) {
        int z, y, x;
        const int where = mmx_locate(bd, idx, z, y, x);
        if (where == 0) return;
        if (where == 2) continue;
        const int64_t row = (int64_t)bd.slot * slot_elems + ((int64_t)z * bd.ny + y) * bd.px;
        float acc = ga[row + x] * t.w2[0];
        for (int k = 1; k <= R; ++k)
            acc = fmaf(ga[row + mmx_reflect(x - k, bd.nx)] + ga[row + mmx_reflect(x + k, bd.nx)], t.w2[k], acc);
        acc = fmaf(gbc[row + x], t.w0[0], acc);
        for (int k = 1; k <= R; ++k)
            acc = fmaf(gbc[row + mmx_reflect(x - k, bd.nx)] + gbc[row + mmx_reflect(x + k, bd.nx)], t.w0[k], acc);
        out[row + x] = acc;
    }
}
