// Blob-table kernels: sphere-overlap pairs (A5) and cross-block close pairs (A13).
//
// mmx_overlap_pairs  -- skimage/feature/blob.py:84-143 (_blob_overlap, 3-D branch :55-81)
//   evaluated for every pair of one block's blobs; pairs whose overlap fraction exceeds
//   `overlap - band` are returned (those within `band` of the limit are re-evaluated on the
//   host with the reference's exact libm calls).  The *sequential* part of _prune_blobs
//   (blob.py:172-186: zero the smaller sigma pair by pair) stays on the host: it is
//   order-dependent and touches a handful of pairs.
// mmx_close_pairs    -- magmap/cv/detector.py:1000-1006 (_find_close_blobs): integer
//   |dz|<=tz && |dy|<=ty && |dx|<=tx all-pairs test between a master and a check table;
//   returns for each master row the LAST matching check row (NumPy fancy-assignment
//   last-write-wins, detector.py:1077-1083) and a hit flag per check row (deleted rows,
//   detector.py:1069).
// Built with -ffp-contract=off so the float64 expressions round like the Python ones.

#include <algorithm>
#include <cstring>
#include <type_traits>

#include "mmx_common.h"

namespace {

// Candidate j of a block is tested against every earlier candidate i.  The block's centres are staged in LDS (as
// floats, for the cheap per-axis cut) chunk by chunk: the inner loop then never touches global memory, which it
// shares with the LoG kernels of the next batch -- read straight from global each of its ~1300 iterations per
// thread waited a microsecond for a saturated L2 (1.7 ms per launch; the host waits for the result).
__global__ void __launch_bounds__(MMX_WG)
overlap_pairs_kernel(const double* __restrict__ blobs, const int32_t* __restrict__ offsets,
                     double overlap, double band, double max_sigma, int32_t* __restrict__ pairs,
                     double* __restrict__ frac, uint32_t cap, uint32_t* __restrict__ count)
{
    constexpr int CH = 2048;
    __shared__ float cz[CH], cy[CH], cx[CH];
    const int b0 = offsets[blockIdx.y], b1 = offsets[blockIdx.y + 1];
    const int n = b1 - b0;
    const double root3 = sqrt(3.0);
    const double kPi = 3.141592653589793;  // math.pi
    // cheap cut first: no overlap beyond sqrt(3) (s_i + s_j) <= 2 sqrt(3) s_max on any one axis
    const float cut = (float)(2.0 * root3 * max_sigma) + 1.0f;
    const int rounds = (n + gridDim.x * MMX_WG - 1) / (gridDim.x * MMX_WG);
    for (int rd = 0; rd < rounds; ++rd) {
        const int i = (rd * gridDim.x + blockIdx.x) * MMX_WG + threadIdx.x;       // (may be >= n: still takes part in the staging)
        const int i_lo = (rd * gridDim.x + blockIdx.x) * MMX_WG;                  // first i of this workgroup
        double zi = 0, yi = 0, xi = 0, si = 0;
        if (i < n) {
            const double* bi = blobs + (int64_t)(b0 + i) * 4;
            zi = bi[0]; yi = bi[1]; xi = bi[2]; si = bi[3];
        }
        const float fz = (float)zi, fy = (float)yi, fx = (float)xi;
        for (int c0 = ((i_lo + 1) / CH) * CH; c0 < n; c0 += CH) {                 // chunks holding some j > i_lo
            const int nc = min(CH, n - c0);
            __syncthreads();
            for (int t = threadIdx.x; t < nc; t += MMX_WG) {
                const double* bj = blobs + (int64_t)(b0 + c0 + t) * 4;
                cz[t] = (float)bj[0]; cy[t] = (float)bj[1]; cx[t] = (float)bj[2];
            }
            __syncthreads();
            if (i >= n) continue;
            for (int t = max(0, i + 1 - c0); t < nc; ++t) {
                if (fabsf(cz[t] - fz) > cut || fabsf(cy[t] - fy) > cut || fabsf(cx[t] - fx) > cut) continue;
                const int j = c0 + t;
                const double* bj = blobs + (int64_t)(b0 + j) * 4;
                const double sj = bj[3];
                if (si == 0.0 && sj == 0.0) continue;
                double r1, r2, ms;
                if (si > sj) { ms = si; r1 = 1.0; r2 = sj / si; }
                else         { ms = sj; r2 = 1.0; r1 = si / sj; }
                const double den = ms * root3;
                const double d0 = bj[0] / den - zi / den;
                const double d1 = bj[1] / den - yi / den;
                const double d2 = bj[2] / den - xi / den;
                const double d = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
                if (d > r1 + r2) continue;
                double f;
                if (d <= fabs(r1 - r2)) {
                    f = 1.0;
                } else {
                    const double rs = r1 + r2;
                    const double tt = rs - d;
                    const double vol = kPi / (12 * d) * (tt * tt) *
                                       (d * d + 2 * d * rs - 3 * (r1 * r1 + r2 * r2) + 6 * r1 * r2);
                    const double rm = r1 < r2 ? r1 : r2;
                    f = vol / (4. / 3 * kPi * (rm * rm * rm));
                }
                if (f > overlap - band) {
                    const uint32_t pos = atomicAdd(count, 1u);
                    if (pos < cap) {
                        pairs[2 * (int64_t)pos] = b0 + i;
                        pairs[2 * (int64_t)pos + 1] = b0 + j;
                        frac[pos] = f;
                    }
                }
            }
        }
    }
}

__global__ void __launch_bounds__(MMX_WG)
close_pairs_kernel(const int32_t* __restrict__ master, int n_master,
                   const int32_t* __restrict__ check, int n_check, int tz, int ty, int tx,
                   int32_t* __restrict__ last, uint8_t* __restrict__ hit)
{
    __shared__ int32_t tile[MMX_WG * 3];
    const int m = blockIdx.x * MMX_WG + threadIdx.x;
    int mz = 0, my = 0, mx = 0;
    if (m < n_master) { mz = master[3 * m]; my = master[3 * m + 1]; mx = master[3 * m + 2]; }
    int best = -1;
    for (int c0 = 0; c0 < n_check; c0 += MMX_WG) {
        const int nc = min(MMX_WG, n_check - c0);
        __syncthreads();
        for (int t = threadIdx.x; t < nc * 3; t += MMX_WG) tile[t] = check[3 * (int64_t)c0 + t];
        __syncthreads();
        if (m < n_master) {
            for (int c = 0; c < nc; ++c) {
                const int dz = abs(mz - tile[3 * c]);
                const int dy = abs(my - tile[3 * c + 1]);
                const int dx = abs(mx - tile[3 * c + 2]);
                if (dz <= tz && dy <= ty && dx <= tx) {
                    best = c0 + c;  // ascending c: the last match survives
                    hit[c0 + c] = 1;
                }
            }
        }
    }
    if (m < n_master) last[m] = best;
}

}  // namespace

extern "C" int mmx_overlap_pairs(const double* d_blobs, const int32_t* d_offsets, int n_blocks,
                                 double overlap, double band, double max_sigma, int32_t* d_pairs, double* d_frac,
                                 uint32_t cap, uint32_t* d_count, void* stream)
{
    if (!d_blobs || !d_offsets || !d_pairs || !d_frac || !d_count || n_blocks < 1 || !(max_sigma > 0)) return MMX_ERR_ARG;
    if (n_blocks > MMX_MAX_BLOCKS) return MMX_ERR_UNSUPPORTED;
    dim3 grid(8, n_blocks);
    mmx_timed_scope ts(MMX_K_PAIRS, (hipStream_t)stream);
    hipLaunchKernelGGL(overlap_pairs_kernel, grid, dim3(MMX_WG), 0, (hipStream_t)stream, d_blobs, d_offsets,
                       overlap, band, max_sigma, d_pairs, d_frac, cap, d_count);
    return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
}

extern "C" int mmx_close_pairs(const int32_t* d_master, int n_master, const int32_t* d_check, int n_check,
                               const int32_t tol[3], int32_t* d_last, uint8_t* d_hit, void* stream)
{
    if (!d_master || !d_check || !tol || !d_last || !d_hit || n_master < 0 || n_check < 0) return MMX_ERR_ARG;
    if (n_master == 0) return MMX_OK;
    hipStream_t s = (hipStream_t)stream;
    if (n_check > 0) {
        hipError_t e = hipMemsetAsync(d_hit, 0, (size_t)n_check, s);
        if (e != hipSuccess) return MMX_ERR_HIP;
    }
    dim3 grid((n_master + MMX_WG - 1) / MMX_WG);
    mmx_timed_scope ts(MMX_K_CLOSE, s);
    hipLaunchKernelGGL(close_pairs_kernel, grid, dim3(MMX_WG), 0, s, d_master, n_master, d_check, n_check,
                       tol[0], tol[1], tol[2], d_last, d_hit);
    return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
}

// ---- intensity co-localisation: mean intensity of one image channel over the voxels each blob owns
// (magmap/cv/colocalizer.py:340-441).  The reference labels a volume per blob channel (row index at
// every blob centre, -1 elsewhere), grey-dilates it with ball(2) -- 33 voxels, so where two balls
// meet the HIGHER row index owns the voxel -- and takes np.mean(roi[label == b, c]).  Here one wave
// owns one blob: lanes 0..32 are the 33 offsets in C order (= the order boolean-mask indexing yields),
// the block's later blobs of the same channel are scanned for takers, and lane 0 sums the owned
// voxels in NumPy's pairwise order (n <= 33: eight accumulators over the first 8*floor(n/8), then the
// tail) so the mean is bit-equal.  The sum and the quotient are float64 for uint8 / uint16 / float64
// voxels (np.mean of an integer selection accumulates in float64) and float32 for float32 voxels (np.mean
// of a float32 selection stays in float32: same order, every step rounded to float); the float32 mean is
// widened into mean[], which loses nothing.  A blob that owns nothing gets 0/0 = NaN, as NumPy gives.
namespace {
// NumPy's pairwise sum of n <= 33 contiguous values (one block: n is below its 128-element split) behind the
// reduction's initial 0, divided by the count, all in AccT
template <typename AccT>
__device__ __forceinline__ AccT coloc_mean_of(const double* vals, int n)
{
    AccT res;
    if (n < 8) {
        res = (AccT)0;
        for (int i = 0; i < n; ++i) res += (AccT)vals[i];
    } else {
        AccT r[8];
        for (int j = 0; j < 8; ++j) r[j] = (AccT)vals[j];
        int i;
        for (i = 8; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += (AccT)vals[i + j];
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += (AccT)vals[i];
    }
    return ((AccT)0 + res) / (AccT)n;           // n == 0 -> NaN, like np.mean of an empty selection
}

template <typename InT>
__global__ void __launch_bounds__(64)
coloc_means_kernel(const InT* __restrict__ vol, int64_t sz, int64_t sy, int64_t sx,
                   const mmx_block* __restrict__ blocks, const int32_t* __restrict__ blobs,
                   const int32_t* __restrict__ offsets, int n_blobs, double* __restrict__ mean,
                   int32_t* __restrict__ count, double* __restrict__ voxels)
{
    __shared__ double vals[33];
    const int b = blockIdx.x;
    if (b >= n_blobs) return;
    const int lane = threadIdx.x;
    const int32_t* me = blobs + 5 * (int64_t)b;
    const int slot = me[0], pz = me[1], py = me[2], px = me[3], chl = me[4];
    const mmx_block bd = blocks[slot];
    // lane -> offset (dz, dy, dx) of ball(2) in lexicographic order
    int dz = 0, dy = 0, dx = 0;
    bool in_ball = false;
    {
        int k = 0;
        for (int a = -2; a <= 2; ++a)
            for (int c = -2; c <= 2; ++c)
                for (int d = -2; d <= 2; ++d)
                    if (a * a + c * c + d * d <= 4) {
                        if (k == lane) { dz = a; dy = c; dx = d; in_ball = true; }
                        ++k;
                    }
    }
    const int vz = pz + dz, vy = py + dy, vx = px + dx;
    bool owned = in_ball && vz >= 0 && vz < bd.nz && vy >= 0 && vy < bd.ny && vx >= 0 && vx < bd.nx &&
                 pz >= 0 && pz < bd.nz && py >= 0 && py < bd.ny && px >= 0 && px < bd.nx;
    // takers: later rows of the same block and channel whose ball reaches this voxel
    const int end = offsets[slot + 1];
    for (int t0 = b + 1; t0 < end; t0 += 64) {
        const int t = t0 + lane;
        bool near = false;
        int tz = 0, ty = 0, tx = 0;
        if (t < end) {
            const int32_t* o = blobs + 5 * (int64_t)t;
            tz = o[1]; ty = o[2]; tx = o[3];
            near = o[4] == chl && abs(tz - pz) <= 4 && abs(ty - py) <= 4 && abs(tx - px) <= 4 &&
                   tz >= 0 && tz < bd.nz && ty >= 0 && ty < bd.ny && tx >= 0 && tx < bd.nx;
        }
        unsigned long long m = __ballot(near);
        while (m) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int qz = __shfl(tz, src), qy = __shfl(ty, src), qx = __shfl(tx, src);
            const int ez = vz - qz, ey = vy - qy, ex = vx - qx;
            if (ez * ez + ey * ey + ex * ex <= 4) owned = false;
        }
    }
    const unsigned long long om = __ballot(owned);
    const int n = __popcll(om);
    if (owned) {
        const int rank = __popcll(om & ((1ull << lane) - 1ull));
        vals[rank] = (double)vol[bd.src_off + vz * sz + vy * sy + vx * sx];
    }
    __syncthreads();
    // (optional) the owned voxels themselves, in the selection's C order: percentile thresholds
    if (voxels && lane < n) voxels[(int64_t)b * MMX_COLOC_BALL + lane] = vals[lane];
    if (lane == 0) {
        if constexpr (std::is_same<InT, float>::value) mean[b] = (double)coloc_mean_of<float>(vals, n);
        else mean[b] = coloc_mean_of<double>(vals, n);
        count[b] = n;
    }
}
}  // namespace

extern "C" int mmx_coloc_voxels(const mmx_volume* vol, const mmx_block* d_blocks, int n_blocks,
                                const int32_t* d_blobs, const int32_t* d_offsets, int n_blobs,
                                double* d_mean, int32_t* d_count, double* d_voxels, void* stream)
{
    if (!vol || !vol->d_data || !d_blocks || n_blocks < 1 || !d_blobs || !d_offsets || n_blobs < 0 ||
        !d_mean || !d_count)
        return MMX_ERR_ARG;
    if (n_blobs == 0) return MMX_OK;
    if (n_blobs > MMX_MAX_GRID_X) return MMX_ERR_UNSUPPORTED;      // one workgroup per blob, one-dimensional grid
    hipStream_t s = (hipStream_t)stream;
    mmx_timed_scope ts(MMX_K_COLOC, s);
    return mmx_for_voxel<MMX_VOX_ALL>(vol->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
        using T = MMX_TAG_T(t);
        hipLaunchKernelGGL(coloc_means_kernel<T>, dim3(n_blobs), dim3(64), 0, s, (const T*)vol->d_data,
                           vol->stride_z, vol->stride_y, vol->stride_x, d_blocks, d_blobs, d_offsets, n_blobs,
                           d_mean, d_count, d_voxels);
        return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
    });
}

extern "C" int mmx_coloc_means(const mmx_volume* vol, const mmx_block* d_blocks, int n_blocks,
                               const int32_t* d_blobs, const int32_t* d_offsets, int n_blobs,
                               double* d_mean, int32_t* d_count, void* stream)
{
    return mmx_coloc_voxels(vol, d_blocks, n_blocks, d_blobs, d_offsets, n_blobs, d_mean, d_count, nullptr, stream);
}

// ---- spectral unmixing ahead of detection (magmap/cv/detector.py:910-921): for the detected channel
//     x = x - fac_k * roi[..., k]  ;  x[x < 0] = 0      for every (k, fac_k) in turn
// in float64 for uint8 / uint16 / float64 voxels (NumPy promotes `uint16 - float * uint16` to float64) and in
// float32 for float32 voxels (a Python-float factor does not widen a float32 array: the factor is rounded to
// float32, product, difference and clip stay float32; out64 then holds the float32 values widened).  One rounding
// for the product, one for the difference: no FMA, this file is built with -ffp-contract=off.  Streaming kernel:
// 1 + K voxels in, 8 + 4 bytes out per voxel, written in the uniform-stride slot layout the preprocessing uses.
#define MMX_UNMIX_MAX 8
struct unmix_args {
    const void* sub[MMX_UNMIX_MAX];
    double fac[MMX_UNMIX_MAX];
    int64_t sub_sz[MMX_UNMIX_MAX], sub_sy[MMX_UNMIX_MAX], sub_sx[MMX_UNMIX_MAX];
    int32_t n_subs, _pad;
};
namespace {
template <typename InT>
__global__ void __launch_bounds__(MMX_WG)
unmix_kernel(const InT* __restrict__ vol, int64_t sz, int64_t sy, int64_t sx, unmix_args U,
             const mmx_block* __restrict__ blocks, int64_t dst_slot, int64_t dst_sy, int64_t dst_sz,
             float* __restrict__ out32, double* __restrict__ out64)
{
    const mmx_block bd = blocks[blockIdx.y];
    const int64_t n = (int64_t)bd.nz * bd.ny * bd.nx;
    for (int64_t i = (int64_t)blockIdx.x * MMX_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * MMX_WG) {
        const int64_t t = i / bd.nx, x = i - t * bd.nx, z = t / bd.ny, y = t - z * bd.ny;
        // float32 voxels: NumPy takes the Python-float factor as a float32 and keeps the product, the difference
        // and the clip in float32; every other voxel type promotes to float64
        using AccT = typename std::conditional<std::is_same<InT, float>::value, float, double>::type;
        AccT v = (AccT)vol[bd.src_off + z * sz + y * sy + x * sx];
        for (int k = 0; k < U.n_subs; ++k) {
            const InT* sp = (const InT*)U.sub[k];
            const AccT m = (AccT)U.fac[k] * (AccT)sp[bd.src_off + z * U.sub_sz[k] + y * U.sub_sy[k] + x * U.sub_sx[k]];
            v = v - m;
            if (v < (AccT)0) v = (AccT)0;
        }
        const int64_t d = (int64_t)bd.slot * dst_slot + z * dst_sz + y * dst_sy + x;
        out64[d] = (double)v;
        out32[d] = (float)v;
    }
}
}  // namespace

extern "C" int mmx_unmix_batch(const mmx_volume* vol, const mmx_volume* h_subs, const double* h_facs, int n_subs,
                               const mmx_block* d_blocks, const mmx_block* h_blocks, int n_blocks,
                               int64_t dst_slot, int64_t dst_sy, int64_t dst_sz,
                               float* d_out32, double* d_out64, void* stream)
{
    if (!vol || !vol->d_data || (n_subs && (!h_subs || !h_facs)) || n_subs < 0 || !d_blocks || !h_blocks ||
        n_blocks < 1 || !d_out32 || !d_out64)
        return MMX_ERR_ARG;
    if (n_subs > MMX_UNMIX_MAX || n_blocks > MMX_MAX_BLOCKS) return MMX_ERR_UNSUPPORTED;
    unmix_args U;
    memset(&U, 0, sizeof U);
    U.n_subs = n_subs;
    for (int k = 0; k < n_subs; ++k) {
        if (!h_subs[k].d_data || h_subs[k].dtype != vol->dtype) return MMX_ERR_ARG;
        U.sub[k] = h_subs[k].d_data;
        U.fac[k] = h_facs[k];
        U.sub_sz[k] = h_subs[k].stride_z; U.sub_sy[k] = h_subs[k].stride_y; U.sub_sx[k] = h_subs[k].stride_x;
    }
    int64_t max_vox = 1;
    for (int i = 0; i < n_blocks; ++i) {
        if (h_blocks[i].nz < 1 || h_blocks[i].ny < 1 || h_blocks[i].nx < 1) return MMX_ERR_ARG;
        max_vox = std::max<int64_t>(max_vox, (int64_t)h_blocks[i].nz * h_blocks[i].ny * h_blocks[i].nx);
    }
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)std::min<int64_t>((max_vox + MMX_WG * 4 - 1) / (MMX_WG * 4), 65535), (unsigned)n_blocks);
    mmx_timed_scope ts(MMX_K_GENERIC, s);
    return mmx_for_voxel<MMX_VOX_ALL>(vol->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
        using T = MMX_TAG_T(t);
        hipLaunchKernelGGL(unmix_kernel<T>, grid, dim3(MMX_WG), 0, s, (const T*)vol->d_data, vol->stride_z,
                           vol->stride_y, vol->stride_x, U, d_blocks, dst_slot, dst_sy, dst_sz, d_out32, d_out64);
        return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
    });
}

// ---- isotropic rescale ahead of detection (magmap/cv/cv_nd.py:1070-1164 -> skimage.transform.resize ->
// scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True)).  SciPy precomputes, per axis and output
// index, the two source indices (border-mapped) and the two linear weights (w0 = 1 - frac, w1 = 1 - w0);
// the caller does the same on the host (bit-equal double arithmetic, preprocess.zoom_axis_table).  The
// kernel reproduces NI_ZoomShift's accumulation exactly: t = 0; for dz, dy, dx (dx fastest):
// t += ((v * wz) * wy) * wx; then scikit-image's clip to the input range and the cast back to the input
// dtype (truncation for integers).  No FMA (this file is built with -ffp-contract=off).
namespace {
__device__ __forceinline__ void atomic_min_f64(double* addr, double v)
{
    unsigned long long* a = (unsigned long long*)addr;
    unsigned long long old = *a;
    while (v < __longlong_as_double((long long)old)) {
        const unsigned long long prev = atomicCAS(a, old, (unsigned long long)__double_as_longlong(v));
        if (prev == old) break;
        old = prev;
    }
}
__device__ __forceinline__ void atomic_max_f64(double* addr, double v)
{
    unsigned long long* a = (unsigned long long*)addr;
    unsigned long long old = *a;
    while (v > __longlong_as_double((long long)old)) {
        const unsigned long long prev = atomicCAS(a, old, (unsigned long long)__double_as_longlong(v));
        if (prev == old) break;
        old = prev;
    }
}

template <typename InT>
__global__ void __launch_bounds__(MMX_WG)
minmax_kernel(const InT* __restrict__ vol, int64_t sz, int64_t sy, int64_t sx,
              const mmx_block* __restrict__ blocks, double* __restrict__ mm)
{
    __shared__ double s_lo[MMX_WG / 64], s_hi[MMX_WG / 64];
    const mmx_block bd = blocks[blockIdx.y];
    const int rows = bd.nz * bd.ny;
    double lo = __builtin_inf(), hi = -__builtin_inf();
    // one wave per (z, y) row, lanes along x, two rows in flight: no per-voxel index arithmetic
    const int lane = threadIdx.x & 63;
    constexpr int WPG = MMX_WG / 64;
    const int stride = (int)gridDim.x * WPG;
    for (int row = __builtin_amdgcn_readfirstlane((int)blockIdx.x * WPG + ((int)threadIdx.x >> 6)); row < rows;
         row += 2 * stride) {
        const int row2 = row + stride < rows ? row + stride : row;
        const int z = row / bd.ny, y = row - z * bd.ny;
        const int z2 = row2 / bd.ny, y2 = row2 - z2 * bd.ny;
        const InT* p = vol + bd.src_off + z * sz + y * sy;
        const InT* p2 = vol + bd.src_off + z2 * sz + y2 * sy;
        for (int x = lane; x < bd.nx; x += 128) {
            const int xb = x + 64 < bd.nx ? x + 64 : x;
            const double a = (double)p[x * sx], b = (double)p[xb * sx];
            const double c = (double)p2[x * sx], d = (double)p2[xb * sx];
            lo = fmin(fmin(lo, fmin(a, b)), fmin(c, d));
            hi = fmax(fmax(hi, fmax(a, b)), fmax(c, d));
        }
    }
    for (int d = 32; d >= 1; d >>= 1) { lo = fmin(lo, __shfl_down(lo, d)); hi = fmax(hi, __shfl_down(hi, d)); }
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < MMX_WG / 64; ++w) { lo = fmin(lo, s_lo[w]); hi = fmax(hi, s_hi[w]); }
        atomic_min_f64(mm + 2 * (int64_t)bd.slot, lo);
        atomic_max_f64(mm + 2 * (int64_t)bd.slot + 1, hi);
    }
}

// One wave per output row (z, y), lanes along x: the z / y table entries are wave-uniform (scalar loads),
// the x entries one 8-byte + one 16-byte load per lane, the eight samples four coalesced row reads -- no
// per-voxel index arithmetic.  The accumulation order is SciPy's (NI_ZoomShift: z outermost, x fastest).
template <typename InT, typename OutT>
__global__ void __launch_bounds__(MMX_WG)
resize_kernel(const InT* __restrict__ vol, int64_t sz, int64_t sy, int64_t sx,
              const mmx_resize_block* __restrict__ blocks, const int32_t* __restrict__ idx,
              const double* __restrict__ wts, const double* __restrict__ mm,
              int64_t dst_slot, int64_t dst_sy, int64_t dst_sz, OutT* __restrict__ out, float* __restrict__ out32)
{
    const mmx_resize_block bd = blocks[blockIdx.y];
    const int rows = bd.out_nz * bd.out_ny;
    const double lo = mm[2 * (int64_t)bd.slot], hi = mm[2 * (int64_t)bd.slot + 1];
    const InT* src = vol + bd.src_off;
    const int lane = threadIdx.x & 63;
    constexpr int WPG = MMX_WG / 64;
    const int2* ixt = reinterpret_cast<const int2*>(idx) + bd.tx;
    const double2* wxt = reinterpret_cast<const double2*>(wts) + bd.tx;
    // the x table entries of this lane's columns stay in registers across the rows of the wave (rows up to
    // kXC * 64 voxels wide; wider ones reload them per row)
    constexpr int kXC = 6;
    const int nxc = (bd.out_nx + 63) >> 6;
    int2 ixr[kXC];
    double2 wxr[kXC];
#pragma unroll
    for (int c = 0; c < kXC; ++c) {
        const int x = lane + 64 * c;
        const int xc = x < bd.out_nx ? x : bd.out_nx - 1;
        ixr[c] = ixt[xc];
        wxr[c] = wxt[xc];
    }
    // A sample whose weight is exactly 0 (an axis that keeps its length: frac = 0 everywhere) adds +-0 to a sum
    // that starts at +0: skipping it leaves every bit of the result unchanged for finite voxels, and an
    // unchanged axis is the common case (light-sheet stacks are rescaled along z only).  z2 / y2 / x2: the
    // second sample of that axis takes part (wave-uniform).
    bool x2 = false;
#pragma unroll
    for (int c = 0; c < kXC; ++c) x2 = x2 || wxr[c].y != 0.0;
    x2 = __any(x2) || nxc > kXC;
    auto one = [&](const InT* p00, const InT* p01, const InT* p10, const InT* p11, double2 wz, double2 wy,
                   bool z2, bool y2, int2 ix, double2 wx) __attribute__((always_inline)) {
        const int64_t o0 = ix.x * sx, o1 = ix.y * sx;
        double acc = 0.0;
        auto plane = [&](const InT* pa, const InT* pb, double w) __attribute__((always_inline)) {
            const double va0 = (double)pa[o0];
            if (x2) {
                const double va1 = (double)pa[o1];
                acc += ((va0 * w) * wy.x) * wx.x;
                acc += ((va1 * w) * wy.x) * wx.y;
            } else {
                acc += ((va0 * w) * wy.x) * wx.x;
            }
            if (y2) {
                const double vb0 = (double)pb[o0];
                if (x2) {
                    const double vb1 = (double)pb[o1];
                    acc += ((vb0 * w) * wy.y) * wx.x;
                    acc += ((vb1 * w) * wy.y) * wx.y;
                } else {
                    acc += ((vb0 * w) * wy.y) * wx.x;
                }
            }
        };
        plane(p00, p01, wz.x);
        if (z2) plane(p10, p11, wz.y);
        return fmin(fmax(acc, lo), hi);                       // np.clip(out, image.min(), image.max())
    };
    for (int row = __builtin_amdgcn_readfirstlane((int)blockIdx.x * WPG + ((int)threadIdx.x >> 6)); row < rows;
         row += (int)gridDim.x * WPG) {
        const int z = row / bd.out_ny, y = row - z * bd.out_ny;
        const int2 iz = reinterpret_cast<const int2*>(idx)[bd.tz + z];
        const int2 iy = reinterpret_cast<const int2*>(idx)[bd.ty + y];
        const double2 wz = reinterpret_cast<const double2*>(wts)[bd.tz + z];
        const double2 wy = reinterpret_cast<const double2*>(wts)[bd.ty + y];
        const InT* p00 = src + iz.x * sz + iy.x * sy;
        const InT* p01 = src + iz.x * sz + iy.y * sy;
        const InT* p10 = src + iz.y * sz + iy.x * sy;
        const InT* p11 = src + iz.y * sz + iy.y * sy;
        const int64_t drow = (int64_t)bd.slot * dst_slot + (int64_t)z * dst_sz + (int64_t)y * dst_sy;
        const bool z2 = wz.y != 0.0, y2 = wy.y != 0.0;
        if (nxc <= kXC) {
#pragma unroll
            for (int c = 0; c < kXC; c += 2) {
                if (c >= nxc) break;                          // uniform
                const int xa = lane + 64 * c, xb = xa + 64;
                const double ra = one(p00, p01, p10, p11, wz, wy, z2, y2, ixr[c], wxr[c]);
                const double rb = one(p00, p01, p10, p11, wz, wy, z2, y2, ixr[c + 1], wxr[c + 1]);
                if (xa < bd.out_nx) {
                    out[drow + xa] = (OutT)ra;                // .astype(dtype): truncation for integers
                    if (out32) out32[drow + xa] = (float)ra;
                }
                if (xb < bd.out_nx) {
                    out[drow + xb] = (OutT)rb;
                    if (out32) out32[drow + xb] = (float)rb;
                }
            }
        } else {
            for (int x = lane; x < bd.out_nx; x += 64) {
                const double r = one(p00, p01, p10, p11, wz, wy, z2, y2, ixt[x], wxt[x]);
                out[drow + x] = (OutT)r;
                if (out32) out32[drow + x] = (float)r;
            }
        }
    }
}
}  // namespace

extern "C" int mmx_minmax_batch(const mmx_volume* vol, const mmx_block* d_blocks, const mmx_block* h_blocks,
                                int n_blocks, double* d_minmax, void* stream)
{
    if (!vol || !vol->d_data || !d_blocks || !h_blocks || n_blocks < 1 || !d_minmax) return MMX_ERR_ARG;
    if (n_blocks > MMX_MAX_BLOCKS) return MMX_ERR_UNSUPPORTED;
    int64_t max_rows = 1;
    for (int i = 0; i < n_blocks; ++i)
        max_rows = std::max<int64_t>(max_rows, (int64_t)h_blocks[i].nz * h_blocks[i].ny);
    if (max_rows >= (int64_t(1) << 30) || n_blocks > MMX_MAX_BLOCKS) return MMX_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    // 16 rows per wave: few enough atomics, enough workgroups (4 waves each) to fill the chip
    dim3 grid((unsigned)std::min<int64_t>((max_rows + 63) / 64, 4096), (unsigned)n_blocks);
    mmx_timed_scope ts(MMX_K_GENERIC, s);
    return mmx_for_voxel<MMX_VOX_ALL>(vol->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
        using T = MMX_TAG_T(t);
        hipLaunchKernelGGL(minmax_kernel<T>, grid, dim3(MMX_WG), 0, s, (const T*)vol->d_data, vol->stride_z,
                           vol->stride_y, vol->stride_x, d_blocks, d_minmax);
        return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
    });
}

// ---- anti-aliasing ahead of a down-sampling resize: one exact float64 correlate1d pass along one axis,
// SciPy's symmetric branch (acc = in[c] w[0]; k = R .. 1: acc += (in[c-k] + in[c+k]) w[k]; no FMA), 'mirror'
// (d c b | a b c d | c b a) or 'nearest' extension, weights and radius per block (a truncated block has its
// own zoom factor).  Source: any supported voxel type at the volume's strides; output: float64 block slots.
namespace {
template <typename InT, typename OutT>
__global__ void __launch_bounds__(MMX_WG)
gauss_axis_kernel(const InT* __restrict__ vol, int64_t sz, int64_t sy, int64_t sx,
                  const mmx_block* __restrict__ blocks, int axis, const double* __restrict__ weights,
                  const int32_t* __restrict__ radius, int w_pitch, int nearest,
                  int64_t dst_slot, int64_t dst_sy, int64_t dst_sz, OutT* __restrict__ out)
{
    const mmx_block bd = blocks[blockIdx.y];
    const int rows = bd.nz * bd.ny;
    const InT* src = vol + bd.src_off;
    const double* w = weights + (int64_t)blockIdx.y * w_pitch;
    const int R = radius[blockIdx.y];
    const int n = axis == 0 ? bd.nz : (axis == 1 ? bd.ny : bd.nx);
    const int64_t st = axis == 0 ? sz : (axis == 1 ? sy : sx);
    const int period = 2 * n - 2;
    auto ext = [&](int i) {
        if (n == 1) return 0;
        if (nearest == 1 || (nearest == 2 && (bd._pad & 1))) return i < 0 ? 0 : (i >= n ? n - 1 : i);
        int m = i % period;
        if (m < 0) m += period;
        return m >= n ? period - m : m;
    };
    const int lane = threadIdx.x & 63;
    constexpr int WPG = MMX_WG / 64;
    for (int row = (int)blockIdx.x * WPG + ((int)threadIdx.x >> 6); row < rows; row += (int)gridDim.x * WPG) {
        const int z = row / bd.ny, y = row - z * bd.ny;
        for (int x = lane; x < bd.nx; x += 64) {
            const int c = axis == 0 ? z : (axis == 1 ? y : x);
            const InT* line = src + (int64_t)z * sz + (int64_t)y * sy + (int64_t)x * sx - (int64_t)c * st;
            double acc = (double)line[(int64_t)c * st] * w[0];
            for (int k = R; k >= 1; --k) {
                const double p = (double)line[(int64_t)ext(c - k) * st] + (double)line[(int64_t)ext(c + k) * st];
                acc += p * w[k];
            }
            out[(int64_t)bd.slot * dst_slot + (int64_t)z * dst_sz + (int64_t)y * dst_sy + x] = (OutT)acc;
        }
    }
}
}  // namespace

extern "C" int mmx_gauss_axis_batch(const mmx_volume* vol, const mmx_block* d_blocks, const mmx_block* h_blocks,
                                    int n_blocks, int axis, const double* d_weights, const int32_t* d_radius,
                                    int w_pitch, int nearest, int64_t dst_slot, int64_t dst_sy, int64_t dst_sz,
                                    void* d_out, void* stream)
{
    if (!vol || !vol->d_data || !d_blocks || !h_blocks || n_blocks < 1 || axis < 0 || axis > 2 || !d_weights ||
        !d_radius || w_pitch < 1 || !d_out)
        return MMX_ERR_ARG;
    int64_t max_rows = 1;
    for (int i = 0; i < n_blocks; ++i)
        max_rows = std::max<int64_t>(max_rows, (int64_t)h_blocks[i].nz * h_blocks[i].ny);
    if (max_rows >= (int64_t(1) << 30) || n_blocks > MMX_MAX_BLOCKS) return MMX_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)std::min<int64_t>((max_rows + 15) / 16, 65535), (unsigned)n_blocks);
    mmx_timed_scope ts(MMX_K_GENERIC, s);
    return mmx_for_voxel<MMX_VOX_ALL>(vol->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
        using T = MMX_TAG_T(t);
        using O = typename std::conditional<std::is_same<T, float>::value, float, double>::type;    // SciPy filters a float32 image into float32 arrays
        hipLaunchKernelGGL((gauss_axis_kernel<T, O>), grid, dim3(MMX_WG), 0, s, (const T*)vol->d_data, vol->stride_z,
                           vol->stride_y, vol->stride_x, d_blocks, axis, d_weights, d_radius, w_pitch, nearest,
                           dst_slot, dst_sy, dst_sz, (O*)d_out);
        return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
    });
}

extern "C" int mmx_resize_batch_as(const mmx_volume* vol, const mmx_resize_block* d_blocks,
                                   const mmx_resize_block* h_blocks, int n_blocks,
                                   const int32_t* d_index, const double* d_weight, const double* d_minmax,
                                   int64_t dst_slot, int64_t dst_sy, int64_t dst_sz,
                                   int out_dtype, void* d_out, float* d_out32, void* stream);

extern "C" int mmx_resize_batch(const mmx_volume* vol, const mmx_resize_block* d_blocks,
                                const mmx_resize_block* h_blocks, int n_blocks,
                                const int32_t* d_index, const double* d_weight, const double* d_minmax,
                                int64_t dst_slot, int64_t dst_sy, int64_t dst_sz,
                                void* d_out, float* d_out32, void* stream)
{
    return mmx_resize_batch_as(vol, d_blocks, h_blocks, n_blocks, d_index, d_weight, d_minmax, dst_slot, dst_sy,
                               dst_sz, vol ? vol->dtype : -1, d_out, d_out32, stream);
}

// out_dtype: the voxel type of the result (.astype(dtype) of the reference: truncation for integers).  It is
// the source's type, except after the anti-aliasing filter, whose float64 output stands in for an integer image.
extern "C" int mmx_resize_batch_as(const mmx_volume* vol, const mmx_resize_block* d_blocks,
                                   const mmx_resize_block* h_blocks, int n_blocks,
                                   const int32_t* d_index, const double* d_weight, const double* d_minmax,
                                   int64_t dst_slot, int64_t dst_sy, int64_t dst_sz,
                                   int out_dtype, void* d_out, float* d_out32, void* stream)
{
    if (!vol || !vol->d_data || !d_blocks || !h_blocks || n_blocks < 1 || !d_index || !d_weight ||
        !d_minmax || !d_out)
        return MMX_ERR_ARG;
    int64_t max_rows = 1;
    for (int i = 0; i < n_blocks; ++i) {
        const mmx_resize_block& b = h_blocks[i];
        if (b.in_nz < 1 || b.in_ny < 1 || b.in_nx < 1 || b.out_nz < 1 || b.out_ny < 1 || b.out_nx < 1)
            return MMX_ERR_ARG;                // (unit-thick axes: the caller's tables are 'nearest' mode)
        if ((int64_t)b.out_nz * b.out_ny >= (int64_t(1) << 31)) return MMX_ERR_UNSUPPORTED;
        max_rows = std::max<int64_t>(max_rows, (int64_t)b.out_nz * b.out_ny);
    }
    if (n_blocks > MMX_MAX_BLOCKS) return MMX_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    // 16 rows per wave: the per-wave set-up (block record, x tables) is three dependent memory round trips
    dim3 grid((unsigned)std::min<int64_t>((max_rows + 16 * (MMX_WG / 64) - 1) / (16 * (MMX_WG / 64)), 65535), (unsigned)n_blocks);
    mmx_timed_scope ts(MMX_K_GENERIC, s);
    auto launch = [&](auto in, auto out, float* o32) {
        using T = MMX_TAG_T(in);
        using O = MMX_TAG_T(out);
        hipLaunchKernelGGL((resize_kernel<T, O>), grid, dim3(MMX_WG), 0, s, (const T*)vol->d_data, vol->stride_z,
                           vol->stride_y, vol->stride_x, d_blocks, d_index, d_weight, d_minmax, dst_slot,
                           dst_sy, dst_sz, (O*)d_out, o32);
        return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
    };
    // the anti-aliasing filter's float64 output standing in for an integer image (truncation toward zero)
    if (vol->dtype == MMX_F64 && out_dtype != MMX_F64)
        return mmx_for_voxel<MMX_VOX_INTEGER>(out_dtype, MMX_ERR_UNSUPPORTED, [&](auto o) { return launch(mmx_tag<double>{}, o, nullptr); });
    if (out_dtype != vol->dtype) return MMX_ERR_UNSUPPORTED;
    if (vol->dtype == MMX_F64 && !d_out32) return MMX_ERR_ARG;
    // (float32: SciPy's float32 output array; float64: its float32 copy beside it)
    return mmx_for_voxel<MMX_VOX_ALL>(vol->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
        return launch(t, t, std::is_same<MMX_TAG_T(t), double>::value ? d_out32 : nullptr);
    });
}

// ---- PMC calibration kernels (tools/pmc_calib.py): streams of a known byte count with the
// access shapes the LoG kernels use, to turn rocprofv3 FETCH_SIZE / WRITE_SIZE into bytes.
namespace {
__global__ void __launch_bounds__(MMX_WG) calib_copy_b32(const float* __restrict__ in, float* __restrict__ out, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * MMX_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * MMX_WG)
        out[i] = in[i] + 1.0f;
}
__global__ void __launch_bounds__(MMX_WG) calib_copy_b128(const float4* __restrict__ in, float4* __restrict__ out, int64_t n4)
{
    for (int64_t i = (int64_t)blockIdx.x * MMX_WG + threadIdx.x; i < n4; i += (int64_t)gridDim.x * MMX_WG) {
        float4 v = in[i];
        v.x += 1.0f;
        out[i] = v;
    }
}
__global__ void __launch_bounds__(MMX_WG) calib_read_u16(const uint16_t* __restrict__ in, float* __restrict__ out, int64_t n)
{
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * MMX_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * MMX_WG)
        acc += (float)in[i];
    if (acc == 12345.678f) out[0] = acc;   // keep the loads alive, (almost) never store
}
}  // namespace

extern "C" int mmx_calib_stream(int kind, const void* d_in, void* d_out, int64_t n_elems, void* stream)
{
    if (!d_in || !d_out || n_elems < 1) return MMX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(256 * 8);
    if (kind == 0) hipLaunchKernelGGL(calib_copy_b32, grid, dim3(MMX_WG), 0, s, (const float*)d_in, (float*)d_out, n_elems);
    else if (kind == 1) hipLaunchKernelGGL(calib_copy_b128, grid, dim3(MMX_WG), 0, s, (const float4*)d_in, (float4*)d_out, n_elems / 4);
    else if (kind == 2) hipLaunchKernelGGL(calib_read_u16, grid, dim3(MMX_WG), 0, s, (const uint16_t*)d_in, (float*)d_out, n_elems);
    else return MMX_ERR_ARG;
    return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
}


// ------------------------------------------------------------------------------------------------ cdist
// Euclidean distance matrix of two small point sets (blobs of two channels in one ROI), float64, as
// scipy.spatial.distance.cdist computes it: s = 0; for k: d = a[k] - b[k]; s += d * d; sqrt(s) -- this file is
// compiled with -ffp-contract=off, so no FMA changes a bit.  One lane per (row, column) pair, both rows read from
// global memory: row i of `a` is the same for the whole workgroup (grid.y), row j of `b` is the lane's own.
__global__ void __launch_bounds__(MMX_WG)
cdist_kernel(const double* __restrict__ a, int64_t n, const double* __restrict__ b, int64_t m, int dim,
             double* __restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * MMX_WG + threadIdx.x;
    const int64_t i = blockIdx.y;
    if (j >= m || i >= n) return;
    double s = 0.0;
    for (int k = 0; k < dim; ++k) {
        const double d = a[i * dim + k] - b[j * dim + k];
        s += d * d;
    }
    out[i * m + j] = sqrt(s);
}

extern "C" int mmx_cdist_f64(const double* d_a, int64_t n, const double* d_b, int64_t m, int dim, double* d_out,
                             void* stream)
{
    if (n < 0 || m < 0 || dim < 1 || dim > 64) return MMX_ERR_ARG;    // (whole blob rows are 8 - 16 values wide)
    if (n == 0 || m == 0) return MMX_OK;
    if (!d_a || !d_b || !d_out || n > 65535) return n > 65535 ? MMX_ERR_UNSUPPORTED : MMX_ERR_ARG;
    mmx_timed_scope ts(MMX_K_COLOC, (hipStream_t)stream);
    dim3 grid((unsigned)((m + MMX_WG - 1) / MMX_WG), (unsigned)n);
    hipLaunchKernelGGL(cdist_kernel, grid, dim3(MMX_WG), 0, (hipStream_t)stream, d_a, n, d_b, m, dim, d_out);
    return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
}
