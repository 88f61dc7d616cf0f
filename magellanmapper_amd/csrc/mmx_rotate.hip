// Whole-image rotation (transformer.rotate_img -> cv_nd.rotate_nd): skimage.transform.rotate(plane, angle, order,
// mode="constant", preserve_range=True) of every plane along one axis of a resident volume, bit for bit.
//
//   rot_minmax_rows_kernel / rot_minmax_x_kernel
//                      every plane's minimum and maximum over all of its channels (the clip range of order 1), one pass.
//                      Planes along z or y are made of whole x rows: a wave folds a few rows of one plane.  Planes along
//                      x: a lane keeps the extremes of its own x through a run of rows.  Both end in 64-bit atomics on
//                      order-preserving keys of the float64 values, skipped where a plain read shows no improvement (the
//                      extremes only ever move one way); rot_keys_kernel turns the keys into float64.
//   rot_tile_kernel    planes along z or y (x lies in the plane): a workgroup takes a 32 x 128 tile of one plane, a wave
//                      eight rows of it, a lane consecutive columns -- the four corner reads of a wave fall into two
//                      slightly slanted source rows, and the footprints of a tile's rows overlap.  Tiles are dealt to the
//                      XCDs in contiguous runs (as mmx_preproc.hip), so that neighbouring tiles meet in one L2.
//   rot_lanes_kernel   planes along x: every plane has the same matrix, so a wave takes one (row, column) of the planes,
//                      works the coordinates out once and its lanes take consecutive x: all four corner reads and the
//                      store are contiguous.  The clip range differs per lane.
// The arithmetic is scikit-image 0.18's _warp_fast in its operand order: c = M00 tc + M01 tr + M02, r = M10 tc + M11 tr +
// M12; order 1 mixes the pixels at floor / ceil, (1 - dc) tl + dc tr and so on, a pixel outside the plane reading 0, clips
// to the plane's range and puts exact zeros back when 0 lies outside that range; order 0 reads the pixel at
// (Py_ssize_t)(v > 0 ? v + .5 : v - .5), the sum in float64 (scikit-image's own round), without a clip.  The float64
// result is cast to the voxel type as C does (truncation).  float32 volumes: order 0 only, coordinates in float32.
// Built with -ffp-contract=off: the reference's arithmetic has no FMA.
#include <algorithm>

#include "mmx_common.h"

namespace {

constexpr int ROT_TILE_R = 32, ROT_TILE_C = 128;
constexpr int ROT_MM_ROWS = 8;         // rows of one plane a wave folds (planes along z or y)
constexpr int ROT_MM_RUN = 2048;       // rows a lane follows its own x through (planes along x)

// One rotation as the kernels address it: planes, rows and columns of the planes with the element strides of each in
// the source and in the destination; the channels of a voxel lie at consecutive elements.
struct rot_geom {
    int64_t s_sp, s_sr, s_sc;
    int64_t d_sp, d_sr, d_sc;
    int32_t n_planes, rows, cols, n_chl;
    double m[6];
};

__device__ __forceinline__ unsigned long long rot_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ double rot_unkey(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

__device__ __forceinline__ void rot_fold(unsigned long long* keys, int plane, double lo, double hi)
{
    if (!(lo <= hi)) return;
    const unsigned long long klo = rot_key(lo), khi = rot_key(hi);
    unsigned long long* k = keys + 2 * (int64_t)plane;
    if (klo < k[0]) atomicMin(k, klo);
    if (khi > k[1]) atomicMax(k + 1, khi);
}

__global__ void __launch_bounds__(MMX_WG) rot_keys_init_kernel(unsigned long long* keys, int n_planes)
{
    const int i = blockIdx.x * MMX_WG + threadIdx.x;
    if (i < n_planes) {
        keys[2 * i] = ~0ull;
        keys[2 * i + 1] = 0ull;
    }
}

__global__ void __launch_bounds__(MMX_WG) rot_keys_kernel(unsigned long long* keys, int n_planes)
{
    const int i = blockIdx.x * MMX_WG + threadIdx.x;
    if (i < 2 * n_planes) reinterpret_cast<double*>(keys)[i] = rot_unkey(keys[i]);
}

// planes of whole x rows: unit = (plane, run of ROT_MM_ROWS rows of it); a row is one run of nx * channels elements
// when the channels are interleaved, and is stepped through by stride_x otherwise
template <typename T>
__global__ void __launch_bounds__(MMX_WG)
rot_minmax_rows_kernel(const T* __restrict__ vol, int64_t sp, int64_t sr, int64_t sx, int n_planes, int rows, int nx,
                       int n_chl, int64_t n_units, unsigned long long* __restrict__ keys)
{
    const int lane = threadIdx.x & 63;
    const int runs = (rows + ROT_MM_ROWS - 1) / ROT_MM_ROWS;
    const int64_t unit = (int64_t)blockIdx.x * (MMX_WG / 64) + (threadIdx.x >> 6);
    if (unit >= n_units) return;
    const int plane = (int)(unit / runs), r0 = (int)(unit % runs) * ROT_MM_ROWS;
    const int r1 = min(rows, r0 + ROT_MM_ROWS);
    double lo = INFINITY, hi = -INFINITY;
    for (int r = r0; r < r1; ++r) {
        const T* p = vol + plane * sp + r * sr;
        if (sx == n_chl) {
            for (int i = lane; i < nx * n_chl; i += 64) {
                const double v = (double)p[i];
                lo = fmin(lo, v);
                hi = fmax(hi, v);
            }
        } else {
            for (int x = lane; x < nx; x += 64)
                for (int c = 0; c < n_chl; ++c) {
                    const double v = (double)p[x * sx + c];
                    lo = fmin(lo, v);
                    hi = fmax(hi, v);
                }
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        lo = fmin(lo, __shfl_down(lo, d));
        hi = fmax(hi, __shfl_down(hi, d));
    }
    if (lane == 0) rot_fold(keys, plane, lo, hi);
}

// planes along x: unit = (64 consecutive x, run of ROT_MM_RUN (z, y) rows)
template <typename T>
__global__ void __launch_bounds__(MMX_WG)
rot_minmax_x_kernel(const T* __restrict__ vol, int64_t sz, int64_t sy, int64_t sx, int nz, int ny, int nx, int n_chl,
                    int64_t n_units, unsigned long long* __restrict__ keys)
{
    const int lane = threadIdx.x & 63;
    const int xchunks = (nx + 63) / 64;
    const int64_t unit = (int64_t)blockIdx.x * (MMX_WG / 64) + (threadIdx.x >> 6);
    if (unit >= n_units) return;
    const int x = (int)(unit % xchunks) * 64 + lane;
    const int64_t row0 = (unit / xchunks) * ROT_MM_RUN;
    const int64_t row1 = row0 + ROT_MM_RUN < (int64_t)nz * ny ? row0 + ROT_MM_RUN : (int64_t)nz * ny;
    if (x >= nx) return;
    double lo = INFINITY, hi = -INFINITY;
    for (int64_t row = row0; row < row1; ++row) {
        const int z = (int)(row / ny), y = (int)(row - (int64_t)z * ny);
        const T* p = vol + z * sz + y * sy + x * sx;
        for (int c = 0; c < n_chl; ++c) {
            const double v = (double)p[c];
            lo = fmin(lo, v);
            hi = fmax(hi, v);
        }
    }
    rot_fold(keys, x, lo, hi);
}

// The reads of one output pixel: element offsets of the four corners (order 0: of the one pixel) from the plane's
// origin, -1 for a pixel outside the plane, and the two fractions.
template <typename CT>
struct rot_taps {
    int64_t o[4];
    CT dr, dc;
};

__device__ __forceinline__ int64_t rot_offset(const rot_geom& g, double r, double c)
{
    if (r < 0.0 || r >= (double)g.rows || c < 0.0 || c >= (double)g.cols) return -1;
    return (int)r * g.s_sr + (int)c * g.s_sc;      // (inside the plane: both fit an int, one conversion each)
}

// scikit-image's round (_shared/interpolation.pxd): the literal is a double, the cast truncates
__device__ __forceinline__ double rot_round(double v) { return trunc(v > 0.0 ? v + 0.5 : v - 0.5); }

template <typename CT, int ORDER>
__device__ __forceinline__ rot_taps<CT> rot_make_taps(const rot_geom& g, int tr, int tc)
{
    const CT x = (CT)tc, y = (CT)tr;
    const CT c = (CT)g.m[0] * x + (CT)g.m[1] * y + (CT)g.m[2];
    const CT r = (CT)g.m[3] * x + (CT)g.m[4] * y + (CT)g.m[5];
    rot_taps<CT> t;
    if (ORDER == 0) {
        t.o[0] = rot_offset(g, rot_round((double)r), rot_round((double)c));
        t.o[1] = t.o[2] = t.o[3] = -1;
        t.dr = t.dc = 0;
    } else {
        const CT minr = floor(r), minc = floor(c), maxr = ceil(r), maxc = ceil(c);
        t.dr = r - minr;
        t.dc = c - minc;
        t.o[0] = rot_offset(g, (double)minr, (double)minc);
        t.o[1] = rot_offset(g, (double)minr, (double)maxc);
        t.o[2] = rot_offset(g, (double)maxr, (double)minc);
        t.o[3] = rot_offset(g, (double)maxr, (double)maxc);
    }
    return t;
}

// One voxel: `base` = the plane's origin plus the channel
template <typename T, typename CT, int ORDER>
__device__ __forceinline__ T rot_value(const T* __restrict__ base, const rot_taps<CT>& t, double lo, double hi)
{
    if (ORDER == 0) return t.o[0] < 0 ? (T)0 : base[t.o[0]];
    const CT tl = t.o[0] < 0 ? (CT)0 : (CT)base[t.o[0]];
    const CT tr = t.o[1] < 0 ? (CT)0 : (CT)base[t.o[1]];
    const CT bl = t.o[2] < 0 ? (CT)0 : (CT)base[t.o[2]];
    const CT br = t.o[3] < 0 ? (CT)0 : (CT)base[t.o[3]];
    const CT top = ((CT)1 - t.dc) * tl + t.dc * tr;
    const CT bottom = ((CT)1 - t.dc) * bl + t.dc * br;
    CT v = ((CT)1 - t.dr) * top + t.dr * bottom;
    // _clip_warp_output: np.clip to the plane's range; exact zeros (the fill) survive when 0 lies outside it
    const bool keep_zero = !(lo <= 0.0 && 0.0 <= hi) && v == (CT)0;
    v = fmin(fmax(v, (CT)lo), (CT)hi);
    if (keep_zero) v = (CT)0;
    return (T)v;
}

template <typename T, int ORDER>
__global__ void __launch_bounds__(MMX_WG)
rot_tile_kernel(const T* __restrict__ src, T* __restrict__ dst, rot_geom g, const double* __restrict__ bounds,
                int tiles_r, int tiles_c, int64_t n_tiles)
{
    using CT = typename std::conditional<std::is_same<T, float>::value, float, double>::type;
    // (workgroups go to the 8 XCDs round robin: each XCD gets a contiguous run of tiles)
    const int64_t per = (n_tiles + 7) >> 3;
    const int64_t id = (int64_t)(blockIdx.x & 7) * per + (int64_t)(blockIdx.x >> 3);
    if (id >= n_tiles) return;
    const int tile_c = (int)(id % tiles_c), tile_r = (int)((id / tiles_c) % tiles_r);
    const int plane = (int)(id / ((int64_t)tiles_c * tiles_r));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int ROWS_PER_WAVE = ROT_TILE_R / (MMX_WG / 64);
    double lo = 0.0, hi = 0.0;
    if (ORDER == 1) {
        lo = bounds[2 * plane];
        hi = bounds[2 * plane + 1];
    }
    const T* sp = src + plane * g.s_sp;
    T* dp = dst + plane * g.d_sp;
    for (int k = 0; k < ROWS_PER_WAVE; ++k) {
        const int tr = tile_r * ROT_TILE_R + wave * ROWS_PER_WAVE + k;
        if (tr >= g.rows) break;
        for (int tc = tile_c * ROT_TILE_C + lane; tc < min(g.cols, (tile_c + 1) * ROT_TILE_C); tc += 64) {
            const rot_taps<CT> t = rot_make_taps<CT, ORDER>(g, tr, tc);
            T* d = dp + tr * g.d_sr + tc * g.d_sc;
            for (int c = 0; c < g.n_chl; ++c) d[c] = rot_value<T, CT, ORDER>(sp + c, t, lo, hi);
        }
    }
}

template <typename T, int ORDER>
__global__ void __launch_bounds__(MMX_WG)
rot_lanes_kernel(const T* __restrict__ src, T* __restrict__ dst, rot_geom g, const double* __restrict__ bounds,
                 int64_t n_pos)
{
    using CT = typename std::conditional<std::is_same<T, float>::value, float, double>::type;
    const int64_t n_wg = (n_pos + MMX_WG / 64 - 1) / (MMX_WG / 64);
    const int64_t per = (n_wg + 7) >> 3;
    const int64_t wg = (int64_t)(blockIdx.x & 7) * per + (int64_t)(blockIdx.x >> 3);
    const int64_t pos = wg * (MMX_WG / 64) + (threadIdx.x >> 6);
    if (wg >= n_wg || pos >= n_pos) return;
    const int lane = threadIdx.x & 63;
    const int tr = __builtin_amdgcn_readfirstlane((int)(pos / g.cols));
    const int tc = __builtin_amdgcn_readfirstlane((int)(pos - (int64_t)tr * g.cols));
    const rot_taps<CT> t = rot_make_taps<CT, ORDER>(g, tr, tc);
    T* drow = dst + tr * g.d_sr + tc * g.d_sc;
    // (the planes' channels are one run of elements when the plane stride is the channel count)
    const bool packed = g.s_sp == g.n_chl && g.d_sp == g.n_chl;
    if (packed) {
        const int n = g.n_planes * g.n_chl;
        for (int i = lane; i < n; i += 64) {
            double lo = 0.0, hi = 0.0;
            if (ORDER == 1) {
                const int plane = i / g.n_chl;
                lo = bounds[2 * plane];
                hi = bounds[2 * plane + 1];
            }
            drow[i] = rot_value<T, CT, ORDER>(src + i, t, lo, hi);
        }
    } else {
        for (int plane = lane; plane < g.n_planes; plane += 64) {
            double lo = 0.0, hi = 0.0;
            if (ORDER == 1) {
                lo = bounds[2 * plane];
                hi = bounds[2 * plane + 1];
            }
            for (int c = 0; c < g.n_chl; ++c)
                drow[plane * g.d_sp + c] = rot_value<T, CT, ORDER>(src + plane * g.s_sp + c, t, lo, hi);
        }
    }
}

inline bool rot_view_ok(const mmx_ds_view* v)
{
    return v && v->d_data && v->stride_z > 0 && v->stride_y > 0 && v->stride_x > 0;
}

// the last element a (nz, ny, nx, n_chl) box of a view touches
inline int64_t rot_last(const mmx_ds_view* v, int nz, int ny, int nx, int n_chl)
{
    return (nz - 1) * v->stride_z + (ny - 1) * v->stride_y + (nx - 1) * v->stride_x + (n_chl - 1);
}

inline bool rot_shape_ok(int nz, int ny, int nx, int n_chl, int axis)
{
    return nz >= 1 && ny >= 1 && nx >= 1 && n_chl >= 1 && axis >= 0 && axis <= 2 &&
           (int64_t)nx * n_chl < (int64_t(1) << 31) && (int64_t)nz * ny < (int64_t(1) << 40);
}

}  // namespace

extern "C" int mmx_rotate_minmax(const mmx_ds_view* src, int64_t src_elems, int nz, int ny, int nx, int n_chl, int axis,
                                 double* d_bounds, void* stream)
{
    if (!rot_view_ok(src) || !d_bounds || !rot_shape_ok(nz, ny, nx, n_chl, axis)) return MMX_ERR_ARG;
    if (rot_last(src, nz, ny, nx, n_chl) >= src_elems) return MMX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int n[3] = {nz, ny, nx};
    const int n_planes = n[axis];
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(d_bounds);
    constexpr int WPG = MMX_WG / 64;
    mmx_timed_scope ts(MMX_K_PREPROC, s);
    hipLaunchKernelGGL(rot_keys_init_kernel, dim3((n_planes + MMX_WG - 1) / MMX_WG), dim3(MMX_WG), 0, s, keys, n_planes);
    int64_t n_units;
    if (axis == 2)
        n_units = (int64_t)((nx + 63) / 64) * (((int64_t)nz * ny + ROT_MM_RUN - 1) / ROT_MM_RUN);
    else
        n_units = (int64_t)n_planes * ((n[1 - axis] + ROT_MM_ROWS - 1) / ROT_MM_ROWS);
    const int64_t wgs = (n_units + WPG - 1) / WPG;
    if (wgs > MMX_MAX_GRID_X) return MMX_ERR_UNSUPPORTED;
    const int rc = mmx_for_voxel<MMX_VOX_ALL>(src->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
        using T = MMX_TAG_T(t);
        if (axis == 2)
            hipLaunchKernelGGL(rot_minmax_x_kernel<T>, dim3((unsigned)wgs), dim3(MMX_WG), 0, s, (const T*)src->d_data,
                               src->stride_z, src->stride_y, src->stride_x, nz, ny, nx, n_chl, n_units, keys);
        else
            hipLaunchKernelGGL(rot_minmax_rows_kernel<T>, dim3((unsigned)wgs), dim3(MMX_WG), 0, s,
                               (const T*)src->d_data, axis == 0 ? src->stride_z : src->stride_y,
                               axis == 0 ? src->stride_y : src->stride_z, src->stride_x, n_planes, n[1 - axis], nx,
                               n_chl, n_units, keys);
        return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
    });
    if (rc != MMX_OK) return rc;
    hipLaunchKernelGGL(rot_keys_kernel, dim3((2 * n_planes + MMX_WG - 1) / MMX_WG), dim3(MMX_WG), 0, s, keys, n_planes);
    return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
}

extern "C" int mmx_rotate_warp(const mmx_ds_view* src, int64_t src_elems, const mmx_ds_view* dst, int64_t dst_elems,
                               int nz, int ny, int nx, int n_chl, int axis, const double* matrix, int order,
                               const double* d_bounds, void* stream)
{
    if (!rot_view_ok(src) || !rot_view_ok(dst) || !matrix || !rot_shape_ok(nz, ny, nx, n_chl, axis)) return MMX_ERR_ARG;
    if (src->d_data == dst->d_data || src->dtype != dst->dtype) return MMX_ERR_ARG;
    if (order != 0 && order != 1) return MMX_ERR_UNSUPPORTED;
    if (order == 1 && (src->dtype == MMX_F32 || !d_bounds)) return src->dtype == MMX_F32 ? MMX_ERR_UNSUPPORTED : MMX_ERR_ARG;
    if (rot_last(src, nz, ny, nx, n_chl) >= src_elems || rot_last(dst, nz, ny, nx, n_chl) >= dst_elems)
        return MMX_ERR_ARG;
    // the channels of a voxel lie beside each other: no other stride may be shorter
    if (std::min({src->stride_z, src->stride_y, src->stride_x, dst->stride_z, dst->stride_y, dst->stride_x}) < n_chl)
        return MMX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int n[3] = {nz, ny, nx};
    const int64_t ss[3] = {src->stride_z, src->stride_y, src->stride_x};
    const int64_t ds[3] = {dst->stride_z, dst->stride_y, dst->stride_x};
    const int ra = axis == 0 ? 1 : 0, ca = axis == 2 ? 1 : 2;     // the planes' row and column axes
    rot_geom g;
    g.s_sp = ss[axis]; g.s_sr = ss[ra]; g.s_sc = ss[ca];
    g.d_sp = ds[axis]; g.d_sr = ds[ra]; g.d_sc = ds[ca];
    g.n_planes = n[axis]; g.rows = n[ra]; g.cols = n[ca]; g.n_chl = n_chl;
    for (int i = 0; i < 6; ++i) g.m[i] = matrix[i];
    mmx_timed_scope ts(MMX_K_PREPROC, s);
    if (axis == 2) {
        const int64_t n_pos = (int64_t)g.rows * g.cols;
        const int64_t wgs = (((n_pos + MMX_WG / 64 - 1) / (MMX_WG / 64)) + 7) / 8 * 8;
        if (wgs > MMX_MAX_GRID_X) return MMX_ERR_UNSUPPORTED;
        return mmx_for_voxel<MMX_VOX_ALL>(src->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
            using T = MMX_TAG_T(t);
            if (order == 0)
                hipLaunchKernelGGL((rot_lanes_kernel<T, 0>), dim3((unsigned)wgs), dim3(MMX_WG), 0, s,
                                   (const T*)src->d_data, (T*)dst->d_data, g, d_bounds, n_pos);
            else if constexpr (!std::is_same<T, float>::value)
                hipLaunchKernelGGL((rot_lanes_kernel<T, 1>), dim3((unsigned)wgs), dim3(MMX_WG), 0, s,
                                   (const T*)src->d_data, (T*)dst->d_data, g, d_bounds, n_pos);
            return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
        });
    }
    const int tiles_r = (g.rows + ROT_TILE_R - 1) / ROT_TILE_R, tiles_c = (g.cols + ROT_TILE_C - 1) / ROT_TILE_C;
    const int64_t n_tiles = (int64_t)g.n_planes * tiles_r * tiles_c;
    const int64_t wgs = (n_tiles + 7) / 8 * 8;
    if (wgs > MMX_MAX_GRID_X) return MMX_ERR_UNSUPPORTED;
    return mmx_for_voxel<MMX_VOX_ALL>(src->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
        using T = MMX_TAG_T(t);
        if (order == 0)
            hipLaunchKernelGGL((rot_tile_kernel<T, 0>), dim3((unsigned)wgs), dim3(MMX_WG), 0, s, (const T*)src->d_data,
                               (T*)dst->d_data, g, d_bounds, tiles_r, tiles_c, n_tiles);
        else if constexpr (!std::is_same<T, float>::value)
            hipLaunchKernelGGL((rot_tile_kernel<T, 1>), dim3((unsigned)wgs), dim3(MMX_WG), 0, s, (const T*)src->d_data,
                               (T*)dst->d_data, g, d_bounds, tiles_r, tiles_c, n_tiles);
        return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
    });
}
