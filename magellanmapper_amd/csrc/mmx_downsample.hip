// Whole-image down-sampling (transformer.transpose_img): the chunks of the reference's plan, resized on their own.
//
// Two streaming kernels, both one wave per output row (z, y) with the lanes along x, so that the z / y table entries
// are wave-uniform and a row's stores are contiguous:
//   ds_zoom_kernel   scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True) through per-axis (index, weight)
//                    tables, NI_ZoomShift's order of operations (t += ((v wz) wy) wx, z outermost, x fastest, every
//                    one of the eight terms), the clip to the converted chunk's range, the store at the chunk's place
//                    in the output volume.  It reads the raw image (img_as_float on load) or the compacted output of
//                    the pick passes.
//   ds_pick_kernel   one correlate1d pass of the anti-aliasing Gaussian evaluated only at the positions the zoom
//                    reads along that axis, written compacted: the same sum in the same order as the dense pass
//                    (mmx_gauss_axis_batch), for a fraction of its outputs.
// A down-sampling zoom reads two source positions per output index and axis; at a factor of 4 that is half of the
// planes, a quarter of the rows and an eighth of the columns -- the dense passes write a float64 copy of every voxel
// three times.  Built with -ffp-contract=off: SciPy's arithmetic has no FMA.
#include <algorithm>

#include "mmx_common.h"

namespace {

// img_as_float of a raw voxel (mmx_vox<T>::exact); the pick passes' float64 / float32 output goes through unchanged
template <typename T>
__device__ __forceinline__ double ds_load(const T* p) { return mmx_vox<T>::exact(*p); }

template <typename InT, typename OutT>
__global__ void __launch_bounds__(MMX_WG)
ds_zoom_kernel(const InT* __restrict__ vol, int64_t sz, int64_t sy, int64_t sx,
               const mmx_ds_chunk* __restrict__ chunks, const int32_t* __restrict__ idx,
               const double* __restrict__ wts, const double* __restrict__ mm, double mm_add, double mm_scale,
               OutT* __restrict__ out, int64_t dz, int64_t dy, int64_t dx)
{
    const mmx_ds_chunk bd = chunks[blockIdx.y];
    const int rows = bd.out_nz * bd.out_ny;
    // the conversion is monotonic: the converted chunk's range is the conversion of its raw extremes
    const double lo = (mm[2 * (int64_t)bd.slot] + mm_add) * mm_scale;
    const double hi = (mm[2 * (int64_t)bd.slot + 1] + mm_add) * mm_scale;
    const InT* src = vol + bd.src_off;
    OutT* dst = out + bd.dst_off;
    const int lane = threadIdx.x & 63;
    constexpr int WPG = MMX_WG / 64;
    const int2* it = reinterpret_cast<const int2*>(idx);
    const double2* wt = reinterpret_cast<const double2*>(wts);
    for (int row = __builtin_amdgcn_readfirstlane((int)blockIdx.x * WPG + ((int)threadIdx.x >> 6)); row < rows;
         row += (int)gridDim.x * WPG) {
        const int z = row / bd.out_ny, y = row - z * bd.out_ny;
        const int2 iz = it[bd.tz + z], iy = it[bd.ty + y];
        const double2 wz = wt[bd.tz + z], wy = wt[bd.ty + y];
        const InT* p00 = src + iz.x * sz + iy.x * sy;
        const InT* p01 = src + iz.x * sz + iy.y * sy;
        const InT* p10 = src + iz.y * sz + iy.x * sy;
        const InT* p11 = src + iz.y * sz + iy.y * sy;
        OutT* drow = dst + (int64_t)z * dz + (int64_t)y * dy;
        for (int x = lane; x < bd.out_nx; x += 64) {
            const int2 ix = it[bd.tx + x];
            const double2 wx = wt[bd.tx + x];
            const int64_t o0 = ix.x * sx, o1 = ix.y * sx;
            // the eight loads first (independent), then NI_ZoomShift's sum
            const double v000 = ds_load(p00 + o0), v001 = ds_load(p00 + o1);
            const double v010 = ds_load(p01 + o0), v011 = ds_load(p01 + o1);
            const double v100 = ds_load(p10 + o0), v101 = ds_load(p10 + o1);
            const double v110 = ds_load(p11 + o0), v111 = ds_load(p11 + o1);
            double acc = 0.0;
            acc += ((v000 * wz.x) * wy.x) * wx.x;
            acc += ((v001 * wz.x) * wy.x) * wx.y;
            acc += ((v010 * wz.x) * wy.y) * wx.x;
            acc += ((v011 * wz.x) * wy.y) * wx.y;
            acc += ((v100 * wz.y) * wy.x) * wx.x;
            acc += ((v101 * wz.y) * wy.x) * wx.y;
            acc += ((v110 * wz.y) * wy.y) * wx.x;
            acc += ((v111 * wz.y) * wy.y) * wx.y;
            // (a float32 image: SciPy rounds to float32, then np.clip in float32 against float32 bounds -- rounding is
            //  monotonic and the bounds are float32 values, so clip-then-round gives the same bits)
            drow[(int64_t)x * dx] = (OutT)fmin(fmax(acc, lo), hi);
        }
    }
}

template <typename InT, typename OutT>
__global__ void __launch_bounds__(MMX_WG)
ds_pick_kernel(const InT* __restrict__ vol, int64_t sz, int64_t sy, int64_t sx,
               const mmx_ds_chunk* __restrict__ chunks, int axis, const double* __restrict__ weights,
               const int32_t* __restrict__ radius, int w_pitch, const int32_t* __restrict__ pick,
               int64_t dst_sy, int64_t dst_sz, OutT* __restrict__ out)
{
    const mmx_ds_chunk bd = chunks[blockIdx.y];
    const int rows = bd.out_nz * bd.out_ny;
    const InT* src = vol + bd.src_off;
    OutT* dst = out + bd.dst_off;
    const double* w = weights + (int64_t)bd.slot * w_pitch;
    const int R = radius[bd.slot];
    const int n = axis == 0 ? bd.in_nz : (axis == 1 ? bd.in_ny : bd.in_nx);
    const int64_t st = axis == 0 ? sz : (axis == 1 ? sy : sx);
    const int32_t* pk = pick + (axis == 0 ? bd.tz : (axis == 1 ? bd.ty : bd.tx));
    const int period = 2 * n - 2;
    // SciPy's 'mirror' (d c b | a b c d | c b a) for any distance: a radius beyond the extent folds more than once
    auto ext = [&](int i) {
        if (n == 1) return 0;
        int m = i % period;
        if (m < 0) m += period;
        return m >= n ? period - m : m;
    };
    const int lane = threadIdx.x & 63;
    constexpr int WPG = MMX_WG / 64;
    for (int row = __builtin_amdgcn_readfirstlane((int)blockIdx.x * WPG + ((int)threadIdx.x >> 6)); row < rows;
         row += (int)gridDim.x * WPG) {
        const int zo = row / bd.out_ny, yo = row - zo * bd.out_ny;
        const int z = axis == 0 ? pk[zo] : zo, y = axis == 1 ? pk[yo] : yo;
        for (int xo = lane; xo < bd.out_nx; xo += 64) {
            const int x = axis == 2 ? pk[xo] : xo;
            const int c = axis == 0 ? z : (axis == 1 ? y : x);
            const InT* line = src + (int64_t)z * sz + (int64_t)y * sy + (int64_t)x * sx - (int64_t)c * st;
            double acc = ds_load(line + (int64_t)c * st) * w[0];
            for (int k = R; k >= 1; --k) {
                const double p = ds_load(line + (int64_t)ext(c - k) * st) + ds_load(line + (int64_t)ext(c + k) * st);
                acc += p * w[k];
            }
            dst[(int64_t)zo * dst_sz + (int64_t)yo * dst_sy + xo] = (OutT)acc;
        }
    }
}

inline int64_t ds_last(int64_t off, int nz, int ny, int nx, int64_t sz, int64_t sy, int64_t sx)
{
    return off + (nz - 1) * sz + (ny - 1) * sy + (nx - 1) * sx;
}

// the entries [t, t + n_out) of a host table of `width` indices each lie in the table and address [0, n_in)
inline bool ds_table_ok(const int32_t* h, int64_t n_table, int t, int n_out, int n_in, int width)
{
    if (t < 0 || (int64_t)t + n_out > n_table) return false;
    for (int64_t i = (int64_t)t * width; i < ((int64_t)t + n_out) * width; ++i)
        if (h[i] < 0 || h[i] >= n_in) return false;
    return true;
}

}  // namespace

extern "C" int mmx_ds_zoom_batch(const mmx_ds_view* src, const mmx_ds_view* dst, int64_t dst_elems,
                                 const mmx_ds_chunk* d_chunks, const mmx_ds_chunk* h_chunks, int n_chunks,
                                 const int32_t* d_index, const int32_t* h_index, int64_t n_index,
                                 const double* d_weight, const double* d_minmax, int raw_dtype, void* stream)
{
    if (!src || !src->d_data || !dst || !dst->d_data || !d_chunks || !h_chunks || n_chunks < 1 || !d_index ||
        !h_index || n_index < 1 || !d_weight || !d_minmax || dst_elems < 1)
        return MMX_ERR_ARG;
    const mmx_voxel_rec* raw = mmx_voxel(raw_dtype);
    if (!raw || n_chunks > MMX_MAX_BLOCKS) return MMX_ERR_UNSUPPORTED;
    const int mid = raw_dtype == MMX_F32 ? MMX_F32 : MMX_F64;      // what the pick passes leave behind, and the result
    if (dst->dtype != mid || (src->dtype != raw_dtype && src->dtype != mid)) return MMX_ERR_UNSUPPORTED;
    if (dst->stride_z < 0 || dst->stride_y < 0 || dst->stride_x < 1) return MMX_ERR_ARG;
    int64_t max_rows = 1;
    for (int i = 0; i < n_chunks; ++i) {
        const mmx_ds_chunk& b = h_chunks[i];
        if (b.in_nz < 1 || b.in_ny < 1 || b.in_nx < 1 || b.out_nz < 1 || b.out_ny < 1 || b.out_nx < 1 ||
            b.slot < 0 || b.slot >= n_chunks || b.dst_off < 0)
            return MMX_ERR_ARG;
        if ((int64_t)b.out_nz * b.out_ny >= (int64_t(1) << 31)) return MMX_ERR_UNSUPPORTED;
        if (ds_last(b.dst_off, b.out_nz, b.out_ny, b.out_nx, dst->stride_z, dst->stride_y, dst->stride_x) >= dst_elems)
            return MMX_ERR_ARG;
        if (!ds_table_ok(h_index, n_index, b.tz, b.out_nz, b.in_nz, 2) ||
            !ds_table_ok(h_index, n_index, b.ty, b.out_ny, b.in_ny, 2) ||
            !ds_table_ok(h_index, n_index, b.tx, b.out_nx, b.in_nx, 2))
            return MMX_ERR_ARG;
        max_rows = std::max<int64_t>(max_rows, (int64_t)b.out_nz * b.out_ny);
    }
    hipStream_t s = (hipStream_t)stream;
    // 4 rows per wave: a chunk's output rows are short (an eighth of its x extent and less)
    constexpr int WPG = MMX_WG / 64;
    dim3 grid((unsigned)std::min<int64_t>((max_rows + 4 * WPG - 1) / (4 * WPG), 65535), (unsigned)n_chunks);
    mmx_timed_scope ts(MMX_K_GENERIC, s);
    return mmx_for_voxel<MMX_VOX_ALL>(src->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
        using T = MMX_TAG_T(t);
        auto launch = [&](auto o) {
            using O = MMX_TAG_T(o);
            hipLaunchKernelGGL((ds_zoom_kernel<T, O>), grid, dim3(MMX_WG), 0, s, (const T*)src->d_data, src->stride_z,
                               src->stride_y, src->stride_x, d_chunks, d_index, d_weight, d_minmax, raw->in_add,
                               raw->in_scale, (O*)dst->d_data, dst->stride_z, dst->stride_y,
                               dst->stride_x);
            return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
        };
        return mid == MMX_F32 ? launch(mmx_tag<float>{}) : launch(mmx_tag<double>{});
    });
}

extern "C" int mmx_ds_gauss_pick_batch(const mmx_ds_view* src, const mmx_ds_chunk* d_chunks,
                                       const mmx_ds_chunk* h_chunks, int n_chunks, int axis, const double* d_weights,
                                       const int32_t* d_radius, const int32_t* h_radius, int w_pitch,
                                       const int32_t* d_pick, const int32_t* h_pick, int64_t n_pick, int64_t dst_sy,
                                       int64_t dst_sz, int64_t dst_elems, void* d_out, void* stream)
{
    if (!src || !src->d_data || !d_chunks || !h_chunks || n_chunks < 1 || axis < 0 || axis > 2 || !d_weights ||
        !d_radius || !h_radius || w_pitch < 1 || !d_pick || !h_pick || n_pick < 1 || dst_sy < 1 || dst_sz < 1 ||
        dst_elems < 1 || !d_out)
        return MMX_ERR_ARG;
    if (n_chunks > MMX_MAX_BLOCKS) return MMX_ERR_UNSUPPORTED;
    int64_t max_rows = 1;
    for (int i = 0; i < n_chunks; ++i) {
        const mmx_ds_chunk& b = h_chunks[i];
        const int in_n[3] = {b.in_nz, b.in_ny, b.in_nx}, out_n[3] = {b.out_nz, b.out_ny, b.out_nx};
        const int t[3] = {b.tz, b.ty, b.tx};
        for (int a = 0; a < 3; ++a)
            if (in_n[a] < 1 || out_n[a] < 1 || (a != axis && in_n[a] != out_n[a])) return MMX_ERR_ARG;
        if (b.slot < 0 || b.slot >= n_chunks || b.dst_off < 0 || h_radius[b.slot] < 0 || h_radius[b.slot] >= w_pitch)
            return MMX_ERR_ARG;
        if ((int64_t)b.out_nz * b.out_ny >= (int64_t(1) << 31)) return MMX_ERR_UNSUPPORTED;
        if (ds_last(b.dst_off, b.out_nz, b.out_ny, b.out_nx, dst_sz, dst_sy, 1) >= dst_elems) return MMX_ERR_ARG;
        if (!ds_table_ok(h_pick, n_pick, t[axis], out_n[axis], in_n[axis], 1)) return MMX_ERR_ARG;
        max_rows = std::max<int64_t>(max_rows, (int64_t)b.out_nz * b.out_ny);
    }
    hipStream_t s = (hipStream_t)stream;
    constexpr int WPG = MMX_WG / 64;
    dim3 grid((unsigned)std::min<int64_t>((max_rows + 4 * WPG - 1) / (4 * WPG), 65535), (unsigned)n_chunks);
    mmx_timed_scope ts(MMX_K_GENERIC, s);
    return mmx_for_voxel<MMX_VOX_ALL>(src->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
        using T = MMX_TAG_T(t);
        using O = typename std::conditional<std::is_same<T, float>::value, float, double>::type;   // SciPy filters a float32 image into float32 arrays
        hipLaunchKernelGGL((ds_pick_kernel<T, O>), grid, dim3(MMX_WG), 0, s, (const T*)src->d_data, src->stride_z,
                           src->stride_y, src->stride_x, d_chunks, axis, d_weights, d_radius, w_pitch, d_pick, dst_sy,
                           dst_sz, (O*)d_out);
        return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
    });
}
