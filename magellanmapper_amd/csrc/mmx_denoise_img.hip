// Whole-image denoise (transformer.preprocess_img, task `denoise`): the device passes of plot_3d.denoise_roi over one
// channel of a resident volume -- np.clip, the sigma = 8 unsharp mask (scipy.ndimage.correlate1d along z, y, x with
// 'nearest' edges at the IMAGE border), the 7-point grey erosion -- in float64, bit for bit.
//
//   dn_sum_kernel      the sum that gates the erosion: int64 for the integer types (exact), sum x and sum |x| in float64
//                      for float64 voxels (any order: the host decides with a rounding bound, equalize.erosion_gate).
//   dn_march_kernel    one correlate pass along z or y.  A lane owns one column of the pass (lanes along x: loads and
//                      stores are coalesced) and marches along it with a window of 64 + DN_J float64 values in registers:
//                      DN_J outputs per step, then the window moves by DN_J registers and DN_J values (loaded a step
//                      ahead) enter.  No LDS: nothing is shared between lanes.  A long axis is cut into segments (each
//                      re-reads a 2 x 32 halo) only when the columns alone do not fill the chip.
//   dn_row_kernel      the pass along x: a wave stages 512 + 64 values of a row in LDS (coalesced, one padding word per 8
//                      so that lanes 8 values apart hit different banks), every lane takes the 72 values around its 8
//                      outputs into registers, and the outputs go back through LDS so that the store is coalesced too.
//   dn_clip_kernel     np.clip alone (unsharp_strength falsy: no blur at all).
//   dn_erode_kernel    min over a voxel and the face neighbours it has, planes [z0, z1) of the finished image.
// The first pass reads the source voxels (2 or 8 bytes) and clips in registers; the last one reads them again for
// den + (den - s * blur): the clipped image is never stored.  Per output and axis 97 float64 operations in
// NI_Correlate1D's order, acc = in[c] w[0]; for k = 32..1: acc += (in[c - k] + in[c + k]) w[k].
// Built with -ffp-contract=off: SciPy's and NumPy's arithmetic has no FMA.
#include <algorithm>

#include "mmx_pp_common.h"

#define DN_J 8                       // outputs per lane and step
#define DN_WIN (2 * PP_R + DN_J)     // the register window
#define DN_SEG (64 * DN_J)           // outputs of one wave's row segment (x pass)
#define DN_LDS_ROW (DN_SEG + 2 * PP_R + (DN_SEG + 2 * PP_R) / 8)     // padded: index p lives at p + p / 8

namespace {

struct dn_weights { double w[PP_R + 1]; };

enum { DN_FIRST = 0, DN_MIDDLE = 1, DN_LAST = 2 };

template <typename T>
__device__ __forceinline__ double dn_den(const T* __restrict__ src, int64_t at, double lo, double hi)
{
    return pp_clip((double)src[at], lo, hi);
}

__device__ __forceinline__ double dn_tap(const double (&r)[DN_WIN], int j, const dn_weights& W)
{
    double acc = r[PP_R + j] * W.w[0];
#pragma unroll
    for (int k = PP_R; k >= 1; --k) acc += (r[PP_R + j - k] + r[PP_R + j + k]) * W.w[k];
    return acc;
}

// MODE DN_FIRST: the pass reads clip(src); DN_MIDDLE: `in` -> `out`; DN_LAST: `in` -> the unsharp mask of clip(src).
// s_m / s_b / s_x: the source's strides along the marched axis, the other one and x; p_m / p_b: those of the packed
// float64 buffers (x pitch 1).  A lane's column is (b, x) = (col / nx, col % nx).
template <typename T, int MODE>
__global__ void __launch_bounds__(MMX_WG)
dn_march_kernel(const T* __restrict__ src, int64_t s_m, int64_t s_b, int64_t s_x, const double* __restrict__ in,
                double* __restrict__ out, int64_t p_m, int64_t p_b, int n_m, int64_t n_cols, int nx, int seg_len,
                double lo, double hi, double strength, dn_weights W)
{
    const int64_t col = (int64_t)blockIdx.x * MMX_WG + threadIdx.x;
    if (col >= n_cols) return;
    const int64_t b = col / nx;
    const int x = (int)(col - b * nx);
    const int64_t s_base = b * s_b + (int64_t)x * s_x;
    const int64_t p_base = b * p_b + x;
    const int m0 = (int)blockIdx.y * seg_len;
    const int m1 = m0 + seg_len < n_m ? m0 + seg_len : n_m;
    const int last = n_m - 1;
    auto value = [&](int m) -> double {
        m = m < 0 ? 0 : (m > last ? last : m);                  // 'nearest'
        if constexpr (MODE == DN_FIRST) return dn_den(src, s_base + (int64_t)m * s_m, lo, hi);
        else return in[p_base + (int64_t)m * p_m];
    };
    double r[DN_WIN], nxt[DN_J];
#pragma unroll
    for (int i = 0; i < 2 * PP_R; ++i) r[DN_J + i] = value(m0 - PP_R + i);
#pragma unroll
    for (int j = 0; j < DN_J; ++j) nxt[j] = value(m0 + PP_R + j);
    for (int m = m0; m < m1; m += DN_J) {
#pragma unroll
        for (int i = 0; i < 2 * PP_R; ++i) r[i] = r[i + DN_J];
#pragma unroll
        for (int j = 0; j < DN_J; ++j) r[2 * PP_R + j] = nxt[j];
#pragma unroll
        for (int j = 0; j < DN_J; ++j) nxt[j] = value(m + DN_J + PP_R + j);       // (clamped: always a voxel)
#pragma unroll
        for (int j = 0; j < DN_J; ++j) {
            if (m + j < m1) {
                double o = dn_tap(r, j, W);
                if constexpr (MODE == DN_LAST)
                    o = pp_unsharp(dn_den(src, s_base + (int64_t)(m + j) * s_m, lo, hi), o, strength);
                out[p_base + (int64_t)(m + j) * p_m] = o;
            }
        }
    }
}

// The pass along x, always the last one.  Wave w of a workgroup takes item blockIdx.x * 4 + w = (row, segment).
template <typename T>
__global__ void __launch_bounds__(MMX_WG)
dn_row_kernel(const T* __restrict__ src, int64_t sz, int64_t sy, int64_t sx, const double* __restrict__ in,
              double* __restrict__ out, int ny, int nx, int segs, int64_t n_items, double lo, double hi,
              double strength, dn_weights W)
{
    __shared__ double s_row[MMX_WG / 64][DN_LDS_ROW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t item = (int64_t)blockIdx.x * (MMX_WG / 64) + wave;
    const bool live = item < n_items;                            // (no early return: the barriers below are the group's)
    const int64_t row = live ? item / segs : 0;
    const int x0 = live ? (int)(item - row * segs) * DN_SEG : 0;
    const double* irow = in + row * nx;
    double* s = s_row[wave];
    if (live) {
#pragma unroll
        for (int t = 0; t < (DN_SEG + 2 * PP_R) / 64; ++t) {
            const int p = lane + 64 * t;
            int x = x0 - PP_R + p;
            x = x < 0 ? 0 : (x > nx - 1 ? nx - 1 : x);          // 'nearest'
            s[p + (p >> 3)] = irow[x];
        }
    }
    __syncthreads();
    double o[DN_J];
    {
        double r[DN_WIN];
#pragma unroll
        for (int i = 0; i < DN_WIN; ++i) r[i] = s[9 * lane + i + (i >> 3)];     // p = 8 lane + i
#pragma unroll
        for (int j = 0; j < DN_J; ++j) o[j] = dn_tap(r, j, W);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < DN_J; ++j) s[9 * lane + j] = o[j];       // output q = 8 lane + j at q + q / 8
    __syncthreads();
    if (live) {
        const int64_t z = row / ny, y = row - z * ny;
        const T* srow = src + z * sz + y * sy;
        double* orow = out + row * nx;
#pragma unroll
        for (int t = 0; t < DN_J; ++t) {
            const int q = lane + 64 * t;
            const int x = x0 + q;
            if (x < nx) orow[x] = pp_unsharp(dn_den(srow, (int64_t)x * sx, lo, hi), s[q + (q >> 3)], strength);
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(MMX_WG)
dn_clip_kernel(const T* __restrict__ src, int64_t sz, int64_t sy, int64_t sx, int64_t rows, int ny, int nx, double lo,
               double hi, double* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    constexpr int WPG = MMX_WG / 64;
    for (int64_t row = (int64_t)blockIdx.x * WPG + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * WPG) {
        const int64_t z = row / ny, y = row - z * ny;
        const T* p = src + z * sz + y * sy;
        double* drow = out + row * nx;
        for (int x = lane; x < nx; x += 64) drow[x] = dn_den(p, (int64_t)x * sx, lo, hi);
    }
}

// sums[0] += sum x (int64 for the integer types, float64 for float64 voxels); sums[1] += sum |x| (float64 voxels only)
template <typename T>
__global__ void __launch_bounds__(MMX_WG)
dn_sum_kernel(const T* __restrict__ src, int64_t sz, int64_t sy, int64_t sx, int64_t rows, int ny, int nx, void* sums)
{
    const int lane = threadIdx.x & 63;
    constexpr int WPG = MMX_WG / 64;
    using Acc = typename std::conditional<std::is_same<T, double>::value, double, long long>::type;
    Acc a = 0, aa = 0;
    for (int64_t row = (int64_t)blockIdx.x * WPG + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * WPG) {
        const int64_t z = row / ny, y = row - z * ny;
        const T* p = src + z * sz + y * sy;
        for (int x = lane; x < nx; x += 64) {
            const T v = p[(int64_t)x * sx];
            a += (Acc)v;
            if constexpr (std::is_same<T, double>::value) aa += fabs(v);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        a += __shfl_down(a, d);
        if constexpr (std::is_same<T, double>::value) aa += __shfl_down(aa, d);
    }
    if (lane == 0) {
        if constexpr (std::is_same<T, double>::value) {
            atomicAdd((double*)sums, a);
            atomicAdd((double*)sums + 1, aa);
        } else {
            atomicAdd((unsigned long long*)sums, (unsigned long long)a);
        }
    }
}

// planes [z0, z1) of the eroded image, packed from `out`; `in`: the whole (nz, ny, nx) image, packed
__global__ void __launch_bounds__(MMX_WG)
dn_erode_kernel(const double* __restrict__ in, int nz, int ny, int nx, int z0, int64_t rows, double* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    constexpr int WPG = MMX_WG / 64;
    const int64_t py = nx, pz = (int64_t)ny * nx;
    for (int64_t row = (int64_t)blockIdx.x * WPG + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * WPG) {
        const int64_t dz = row / ny;
        const int y = (int)(row - dz * ny), z = z0 + (int)dz;
        const int64_t base = z * pz + y * py;
        double* drow = out + row * nx;
        for (int x = lane; x < nx; x += 64)
            drow[x] = pp_erode7(in, base + x, py, pz, x > 0, x < nx - 1, y > 0, y < ny - 1, z > 0, z < nz - 1);
    }
}

inline unsigned dn_row_grid(int64_t rows)
{
    constexpr int WPG = MMX_WG / 64;
    return (unsigned)std::min<int64_t>((rows + 4 * WPG - 1) / (4 * WPG), 1 << 20);
}

inline bool dn_shape_ok(const mmx_ds_view* src, int nz, int ny, int nx)
{
    constexpr int DN_MAX_AXIS = 1 << 30;                         // (index arithmetic beyond an axis end stays in int)
    return src && src->d_data && nz >= 1 && ny >= 1 && nx >= 1 && nz <= DN_MAX_AXIS && ny <= DN_MAX_AXIS &&
           nx <= DN_MAX_AXIS;
}

constexpr unsigned DN_VOX = MMX_VOX_INTEGER | mmx_vox_bit(MMX_F64);

}  // namespace

extern "C" int mmx_dn_sum(const mmx_ds_view* src, int nz, int ny, int nx, void* d_sums, void* stream)
{
    if (!dn_shape_ok(src, nz, ny, nx) || !d_sums) return MMX_ERR_ARG;
    if (!mmx_voxel_in(src->dtype, DN_VOX)) return MMX_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(d_sums, 0, 16, s) != hipSuccess) return MMX_ERR_HIP;
    const int64_t rows = (int64_t)nz * ny;
    mmx_timed_scope ts(MMX_K_PREPROC, s);
    return mmx_for_voxel<DN_VOX>(src->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
        using T = MMX_TAG_T(t);
        hipLaunchKernelGGL(dn_sum_kernel<T>, dim3(std::min(dn_row_grid(rows), 4096u)), dim3(MMX_WG), 0, s,
                           (const T*)src->d_data, src->stride_z, src->stride_y, src->stride_x, rows, ny, nx, d_sums);
        return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
    });
}

extern "C" int mmx_dn_clip(const mmx_ds_view* src, int nz, int ny, int nx, double clip_min, double clip_max,
                           double* d_out, void* stream)
{
    if (!dn_shape_ok(src, nz, ny, nx) || !d_out) return MMX_ERR_ARG;
    if (!mmx_voxel_in(src->dtype, DN_VOX)) return MMX_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const int64_t rows = (int64_t)nz * ny;
    mmx_timed_scope ts(MMX_K_PREPROC, s);
    return mmx_for_voxel<DN_VOX>(src->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
        using T = MMX_TAG_T(t);
        hipLaunchKernelGGL(dn_clip_kernel<T>, dim3(dn_row_grid(rows)), dim3(MMX_WG), 0, s, (const T*)src->d_data,
                           src->stride_z, src->stride_y, src->stride_x, rows, ny, nx, clip_min, clip_max, d_out);
        return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
    });
}

extern "C" int mmx_dn_blur(const mmx_ds_view* src, int nz, int ny, int nx, int axis, const double* h_weights,
                           double clip_min, double clip_max, const double* d_in, double* d_out, int last,
                           double strength, void* stream)
{
    if (!dn_shape_ok(src, nz, ny, nx) || axis < 0 || axis > 2 || !h_weights || !d_out || d_in == d_out)
        return MMX_ERR_ARG;
    // the first pass reads the source, the last one the source again: the x pass is never first, the z pass never last
    if ((axis == 0) != (d_in == nullptr) || (axis == 0 && last) || (axis == 2 && !last)) return MMX_ERR_ARG;
    if (!mmx_voxel_in(src->dtype, DN_VOX)) return MMX_ERR_UNSUPPORTED;
    dn_weights W;
    for (int k = 0; k <= PP_R; ++k) W.w[k] = h_weights[k];
    hipStream_t s = (hipStream_t)stream;
    mmx_timed_scope ts(MMX_K_PREPROC, s);
    if (axis == 2) {
        const int segs = (nx + DN_SEG - 1) / DN_SEG;
        const int64_t n_items = (int64_t)nz * ny * segs;
        const int64_t groups = (n_items + MMX_WG / 64 - 1) / (MMX_WG / 64);
        if (groups > MMX_MAX_GRID_X) return MMX_ERR_UNSUPPORTED;
        return mmx_for_voxel<DN_VOX>(src->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
            using T = MMX_TAG_T(t);
            hipLaunchKernelGGL(dn_row_kernel<T>, dim3((unsigned)groups), dim3(MMX_WG), 0, s, (const T*)src->d_data,
                               src->stride_z, src->stride_y, src->stride_x, d_in, d_out, ny, nx, segs, n_items,
                               clip_min, clip_max, strength, W);
            return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
        });
    }
    const int n_m = axis == 0 ? nz : ny, n_b = axis == 0 ? ny : nz;
    const int64_t s_m = axis == 0 ? src->stride_z : src->stride_y, s_b = axis == 0 ? src->stride_y : src->stride_z;
    const int64_t p_z = (int64_t)ny * nx, p_y = nx;
    const int64_t p_m = axis == 0 ? p_z : p_y, p_b = axis == 0 ? p_y : p_z;
    const int64_t n_cols = (int64_t)n_b * nx;
    const int64_t groups = (n_cols + MMX_WG - 1) / MMX_WG;
    if (groups > MMX_MAX_GRID_X) return MMX_ERR_UNSUPPORTED;
    // segments of the marched axis: one while the columns fill the chip (no halo is read twice), more for a thin image
    const int64_t want = std::max<int64_t>(1, 1024 / groups);
    const int n_seg = (int)std::min<int64_t>(want, (n_m + 63) / 64);
    int seg_len = (n_m + n_seg - 1) / n_seg;
    seg_len = (seg_len + DN_J - 1) / DN_J * DN_J;
    dim3 grid((unsigned)groups, (unsigned)((n_m + seg_len - 1) / seg_len));
    if (axis == 0) {
        return mmx_for_voxel<DN_VOX>(src->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
            using T = MMX_TAG_T(t);
            hipLaunchKernelGGL((dn_march_kernel<T, DN_FIRST>), grid, dim3(MMX_WG), 0, s, (const T*)src->d_data, s_m, s_b,
                               src->stride_x, (const double*)nullptr, d_out, p_m, p_b, n_m, n_cols, nx, seg_len,
                               clip_min, clip_max, strength, W);
            return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
        });
    }
    if (!last) {
        hipLaunchKernelGGL((dn_march_kernel<double, DN_MIDDLE>), grid, dim3(MMX_WG), 0, s, (const double*)nullptr, s_m,
                           s_b, src->stride_x, d_in, d_out, p_m, p_b, n_m, n_cols, nx, seg_len, clip_min, clip_max,
                           strength, W);
        return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
    }
    return mmx_for_voxel<DN_VOX>(src->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
        using T = MMX_TAG_T(t);
        hipLaunchKernelGGL((dn_march_kernel<T, DN_LAST>), grid, dim3(MMX_WG), 0, s, (const T*)src->d_data, s_m, s_b,
                           src->stride_x, d_in, d_out, p_m, p_b, n_m, n_cols, nx, seg_len, clip_min, clip_max, strength,
                           W);
        return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
    });
}

extern "C" int mmx_dn_erode(const double* d_in, int nz, int ny, int nx, int z0, int z1, double* d_out, void* stream)
{
    if (!d_in || nz < 1 || ny < 1 || nx < 1 || z0 < 0 || z1 <= z0 || z1 > nz || !d_out || d_in == d_out)
        return MMX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int64_t rows = (int64_t)(z1 - z0) * ny;
    mmx_timed_scope ts(MMX_K_PREPROC, s);
    hipLaunchKernelGGL(dn_erode_kernel, dim3(dn_row_grid(rows)), dim3(MMX_WG), 0, s, d_in, nz, ny, nx, z0, rows, d_out);
    return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
}
