// One 2-D patch per blob, normalised to its own maximum: the input of the patch classifier.
// replaces: the per-blob loop of classifier.extract_patches (magmap/cv/classifier.py:16-55),
//     patch = roi[z, y - size // 2 : y + ceil(size / 2), x - size // 2 : x + size // 2];  patch / np.max(patch)
// with NumPy's arithmetic: integer and float64 voxels are divided in float64, float32 voxels in float32 (true divide
// keeps float32), np.max propagates NaN.  This file is compiled with -ffp-contract=off; the quotient is the plain IEEE
// division either way.
//
// One wave64 per patch, MMX_WG / 64 patches per workgroup.  Lanes stride over the size_y x size_x elements with
// element-sized loads (the patch origin x - size // 2 has no alignment to rely on; neighbouring lanes read neighbouring
// voxels of a row), the wave maximum comes from an xor butterfly of shuffles, and the elements are read a second time
// for the division -- a patch is at most a few cache lines that the first pass has just brought in, and no element has
// to be kept in a register array whose length would depend on `size`.  No LDS, no atomics, no scratch.
#include "mmx_common.h"

#define MMX_PATCH_WAVES (MMX_WG / 64)

// np.max's order: a NaN on either side wins (fmax would drop it)
template <typename T>
__device__ __forceinline__ T patch_nanmax(T a, T b)
{
    return (a >= b || a != a) ? a : b;
}

template <typename T>
__device__ __forceinline__ T patch_wave_max(T m)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = patch_nanmax(m, __shfl_xor(m, d, 64));
    return m;
}

// V: voxel type, T: the type NumPy divides in (and the type of `out`)
template <typename V, typename T>
__global__ void __launch_bounds__(MMX_WG)
patches_kernel(const V* __restrict__ data, int64_t sz, int64_t sy, int64_t sx, const int32_t* __restrict__ zyx, int64_t n,
               int back, int size_y, int size_x, T* __restrict__ out, float* __restrict__ out32)
{
    const int64_t p = (int64_t)blockIdx.x * MMX_PATCH_WAVES + (threadIdx.x >> 6);
    if (p >= n) return;                       // (whole waves leave: every shuffle below has its 64 lanes)
    const int lane = threadIdx.x & 63;
    const int64_t z = zyx[3 * p], y = zyx[3 * p + 1], x = zyx[3 * p + 2];
    const V* __restrict__ src = data + z * sz + (y - back) * sy + (x - back) * sx;
    const int elems = size_y * size_x;

    T m = -INFINITY;
    for (int i = lane; i < elems; i += 64) {
        const int r = i / size_x, c = i - r * size_x;
        m = patch_nanmax(m, (T)src[r * sy + c * sx]);
    }
    m = patch_wave_max(m);

    const int64_t o = p * elems;
    for (int i = lane; i < elems; i += 64) {
        const int r = i / size_x, c = i - r * size_x;
        const T q = (T)src[r * sy + c * sx] / m;
        if (out) out[o + i] = q;
        if (out32) out32[o + i] = (float)q;
    }
}

template <typename V, typename T>
static int patches_launch(const mmx_volume* vol, const int32_t* d_zyx, int64_t n, int size, void* d_out, float* d_out32,
                          hipStream_t s)
{
    const int64_t wgs = (n + MMX_PATCH_WAVES - 1) / MMX_PATCH_WAVES;
    if (wgs > MMX_MAX_GRID_X) return MMX_ERR_UNSUPPORTED;
    const int back = size / 2;
    hipLaunchKernelGGL((patches_kernel<V, T>), dim3((unsigned)wgs), dim3(MMX_WG), 0, s, (const V*)vol->d_data,
                       vol->stride_z, vol->stride_y, vol->stride_x, d_zyx, n, back, size, 2 * back, (T*)d_out, d_out32);
    return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
}

extern "C" int mmx_extract_patches(const mmx_volume* vol, const int32_t* d_zyx, int64_t n, int size, void* d_out,
                                   float* d_out32, void* stream)
{
    if (!vol || size < 2 || size > MMX_PATCH_MAX_SIZE || n < 0) return MMX_ERR_ARG;
    if (n == 0 || (!d_out && !d_out32)) return MMX_OK;
    if (!vol->d_data || !d_zyx) return MMX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    return mmx_for_voxel<MMX_VOX_ALL>(vol->dtype, MMX_ERR_ARG, [&](auto t) {
        using V = MMX_TAG_T(t);
        using T = typename std::conditional<std::is_same<V, float>::value, float, double>::type;    // (true divide keeps float32)
        return patches_launch<V, T>(vol, d_zyx, n, size, d_out, d_out32, s);
    });
}
