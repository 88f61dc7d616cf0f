// Whole-image preprocessing (transformer.preprocess_img): the device passes of skimage.exposure.equalize_adapthist
// (`remap`) and of plot_3d.saturate_roi's stretch (`saturate`) over a resident volume.
//
//   eq_hist_kernel     one histogram per kernel_size tile of the (virtually) reflect-padded image: voxels of the
//                      trailing padding are read at their mirrored source positions, no padded copy exists.  A voxel's
//                      bin is bins[key(voxel)], a host table over the 65536 values img_as_uint can give; counts are
//                      taken in LDS (one copy per wave while 4 nbins words fit, bins shared by many lanes of a wave
//                      are peeled off with a ballot and counted once) and flushed to the tiles x nbins table.
//   eq_apply_kernel    the eight-map interpolation, one wave per (z, y) row: per-axis tables from the host give every
//                      coordinate its two neighbouring tiles and the two coefficients arange(k) / k, 1 - arange(k) / k
//                      (no division here); every term is the float64 product map * ((cx cy) cz) rounded to float32,
//                      added in float32 in np.ndindex(2, 2, 2) order and truncated to uint16, as _clahe does.  It
//                      also folds the result's minimum and maximum.
//   eq_output_kernel   table[level]: img_as_float and the last rescale_intensity act on at most 16384 levels, the host
//                      states them in NumPy.
//   stretch_kernel     (clip(x, vmin, vmax) - vmin) / (vmax - vmin) in float64, IEEE division.
// clip_histogram / map_histogram run on the host between the launches (mmx_host.cpp: mmx_host_eq_maps).
// Built with -ffp-contract=off: NumPy's arithmetic has no FMA.
#include <algorithm>

#include "mmx_common.h"

namespace {

// np.pad(mode='reflect') (d c b | a b c d | c b a) for any distance
__device__ __forceinline__ int eq_mirror(int i, int n)
{
    if (i < n) return i;
    if (n == 1) return 0;
    const int period = 2 * n - 2;
    const int m = i % period;
    return m >= n ? period - m : m;
}

// The index of a voxel in the host's table: the value itself (uint8, uint16), the order-preserving key (int16), or
// img_as_uint of a float voxel -- np.multiply(v, 65535, dtype=<the voxel's type>), np.rint, np.clip(0, 65535).
template <typename T>
__device__ __forceinline__ unsigned eq_key(T v)
{
    if constexpr (std::is_same<T, float>::value) {
        const float u = fminf(fmaxf(rintf(v * 65535.0f), 0.0f), 65535.0f);
        return (unsigned)u;
    } else if constexpr (std::is_same<T, double>::value) {
        const double u = fmin(fmax(rint(v * 65535.0), 0.0), 65535.0);
        return (unsigned)u;
    } else if constexpr (std::is_signed<T>::value) {
        return (unsigned)(uint16_t)v ^ 0x8000u;
    } else {
        return (unsigned)v;
    }
}

template <typename T>
__global__ void __launch_bounds__(MMX_WG)
eq_hist_kernel(const T* __restrict__ vol, int64_t sz, int64_t sy, int64_t sx, mmx_eq_geom g,
               const uint16_t* __restrict__ bins, uint32_t* __restrict__ hist, int rows_per_part, int copies)
{
    extern __shared__ uint32_t s_hist[];
    const int nbins = g.nbins;
    for (int i = threadIdx.x; i < copies * nbins; i += MMX_WG) s_hist[i] = 0;
    __syncthreads();
    const unsigned tile = blockIdx.x;
    const int tx = (int)(tile % (unsigned)g.nt[2]);
    const int ty = (int)((tile / (unsigned)g.nt[2]) % (unsigned)g.nt[1]);
    const int tz = (int)(tile / ((unsigned)g.nt[2] * (unsigned)g.nt[1]));
    const int kz = g.k[0], ky = g.k[1], kx = g.k[2];
    const int64_t rows = (int64_t)kz * ky;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_part;
    const int64_t r1 = r0 + rows_per_part < rows ? r0 + rows_per_part : rows;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* h = s_hist + (copies > 1 ? wave * nbins : 0);
    for (int64_t row = r0 + wave; row < r1; row += MMX_WG / 64) {
        const int dz = (int)(row / ky), dy = (int)(row - (int64_t)dz * ky);
        const int z = eq_mirror(tz * kz + dz, g.n[0]), y = eq_mirror(ty * ky + dy, g.n[1]);
        const T* p = vol + z * sz + y * sy;
        for (int x0 = 0; x0 < kx; x0 += 64) {
            const int xo = x0 + lane;
            bool active = xo < kx;
            unsigned bin = 0;
            if (active) bin = bins[eq_key(p[eq_mirror(tx * kx + xo, g.n[2]) * sx])];
            // a nuclei image puts most of a row into two or three background bins: count those once per wave
            unsigned long long todo = __ballot(active);
            for (int round = 0; round < 3 && todo; ++round) {
                const int leader = __ffsll((long long)todo) - 1;
                const unsigned b0 = (unsigned)__builtin_amdgcn_readlane((int)bin, leader);
                const unsigned long long same = __ballot(active && bin == b0);
                if (lane == leader) atomicAdd(&h[b0], (uint32_t)__popcll(same));
                if (bin == b0) active = false;
                todo &= ~same;
            }
            if (active) atomicAdd(&h[bin], 1u);
        }
    }
    __syncthreads();
    uint32_t* dst = hist + (int64_t)tile * nbins;
    for (int b = threadIdx.x; b < nbins; b += MMX_WG) {
        uint32_t c = s_hist[b];
        for (int w = 1; w < copies; ++w) c += s_hist[w * nbins + b];
        if (c) atomicAdd(&dst[b], c);
    }
}

// One voxel from its eight map values: np.ndindex(2, 2, 2) order -- (ez, ey, ex), ex fastest --, the coefficient
// np.product([x, y, z]) = (x y) z, every float64 product rounded to float32, the sum in float32, truncated to uint16.
// (.x: the lower neighbour, edge 0, coefficient 1 - c; .y: the upper)
__device__ __forceinline__ unsigned eq_mix(double v000, double v001, double v010, double v011, double v100, double v101,
                                           double v110, double v111, double2 cx, double2 cy, double2 cz)
{
    float r = (float)(v000 * ((cx.x * cy.x) * cz.x));
    r += (float)(v001 * ((cx.y * cy.x) * cz.x));
    r += (float)(v010 * ((cx.x * cy.y) * cz.x));
    r += (float)(v011 * ((cx.y * cy.y) * cz.x));
    r += (float)(v100 * ((cx.x * cy.x) * cz.y));
    r += (float)(v101 * ((cx.y * cy.x) * cz.y));
    r += (float)(v110 * ((cx.x * cy.y) * cz.y));
    r += (float)(v111 * ((cx.y * cy.y) * cz.y));
    return (unsigned)(uint16_t)r;
}

// the result's minimum and maximum of a wave into d_minmax
__device__ __forceinline__ void eq_fold_minmax(unsigned lo, unsigned hi, uint32_t* mm)
{
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned l2 = (unsigned)__shfl_down((int)lo, d), h2 = (unsigned)__shfl_down((int)hi, d);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if ((threadIdx.x & 63) == 0 && lo <= hi) {
        atomicMin(&mm[0], lo);
        atomicMax(&mm[1], hi);
    }
}

// The same for one interpolation block per workgroup: block b of an axis covers the coordinates [b k - k / 2,
// (b + 1) k - k / 2) of the image, all of which share their two tiles, so the block's eight maps are staged in LDS
// once (16 nbins bytes) and read there by every voxel of the rows this workgroup takes (blockIdx.y: its share).
template <typename T>
__global__ void __launch_bounds__(MMX_WG)
eq_apply_lds_kernel(const T* __restrict__ vol, int64_t sz, int64_t sy, int64_t sx, mmx_eq_geom g,
                    const uint16_t* __restrict__ bins, const uint16_t* __restrict__ maps,
                    const int2* __restrict__ tiles, const double2* __restrict__ coef,
                    uint16_t* __restrict__ out, uint32_t* __restrict__ mm)
{
    extern __shared__ uint16_t s_maps[];
    const int nz = g.n[0], ny = g.n[1], nx = g.n[2];
    const int nbins = g.nbins;
    const unsigned nbx = (unsigned)g.nt[2] + 1, nby = (unsigned)g.nt[1] + 1;
    const int bx = (int)(blockIdx.x % nbx), by = (int)((blockIdx.x / nbx) % nby), bz = (int)(blockIdx.x / (nbx * nby));
    const int z0 = max(0, bz * g.k[0] - g.k[0] / 2), z1 = min(nz, (bz + 1) * g.k[0] - g.k[0] / 2);
    const int y0 = max(0, by * g.k[1] - g.k[1] / 2), y1 = min(ny, (by + 1) * g.k[1] - g.k[1] / 2);
    const int x0 = max(0, bx * g.k[2] - g.k[2] / 2), x1 = min(nx, (bx + 1) * g.k[2] - g.k[2] / 2);
    if (z0 >= z1 || y0 >= y1 || x0 >= x1) return;      // (the last block of an axis can lie behind the image)
    const int2 tz = tiles[z0], ty = tiles[nz + y0], tx = tiles[nz + ny + x0];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int64_t t = ((int64_t)((e & 4) ? tz.y : tz.x) * g.nt[1] + ((e & 2) ? ty.y : ty.x)) * g.nt[2] +
                          ((e & 1) ? tx.y : tx.x);
        const uint16_t* src = maps + t * nbins;
        for (int b = threadIdx.x; b < nbins; b += MMX_WG) s_maps[e * nbins + b] = src[b];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    constexpr int WPG = MMX_WG / 64;
    const int ny_b = y1 - y0, rows = (z1 - z0) * ny_b;
    unsigned lo = 0xffffu, hi = 0u;
    for (int r = __builtin_amdgcn_readfirstlane((int)blockIdx.y * WPG + ((int)threadIdx.x >> 6)); r < rows;
         r += (int)gridDim.y * WPG) {
        const int z = z0 + r / ny_b, y = y0 + r % ny_b;
        const double2 cz = coef[z], cy = coef[nz + y];
        const T* p = vol + z * sz + y * sy;
        uint16_t* drow = out + ((int64_t)z * ny + y) * nx;
        for (int x = x0 + lane; x < x1; x += 64) {
            const double2 cx = coef[nz + ny + x];
            const uint16_t* m = s_maps + bins[eq_key(p[x * sx])];
            const unsigned v = eq_mix(m[0], m[nbins], m[2 * nbins], m[3 * nbins], m[4 * nbins], m[5 * nbins],
                                      m[6 * nbins], m[7 * nbins], cx, cy, cz);
            drow[x] = (uint16_t)v;
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
    }
    eq_fold_minmax(lo, hi, mm);
}

template <typename T>
__global__ void __launch_bounds__(MMX_WG)
eq_apply_kernel(const T* __restrict__ vol, int64_t sz, int64_t sy, int64_t sx, mmx_eq_geom g,
                const uint16_t* __restrict__ bins, const uint16_t* __restrict__ maps,
                const int2* __restrict__ tiles, const double2* __restrict__ coef,
                uint16_t* __restrict__ out, uint32_t* __restrict__ mm)
{
    const int nz = g.n[0], ny = g.n[1], nx = g.n[2];
    const int nbins = g.nbins;
    const int rows = nz * ny;
    const int lane = threadIdx.x & 63;
    constexpr int WPG = MMX_WG / 64;
    unsigned lo = 0xffffu, hi = 0u;
    for (int row = __builtin_amdgcn_readfirstlane((int)blockIdx.x * WPG + ((int)threadIdx.x >> 6)); row < rows;
         row += (int)gridDim.x * WPG) {
        const int z = row / ny, y = row - z * ny;
        const int2 tz = tiles[z], ty = tiles[nz + y];
        const double2 cz = coef[z], cy = coef[nz + y];
        // the four (z, y) corners of the map table; .x: the lower neighbour (edge 0, coefficient 1 - c), .y: the upper
        const uint16_t* m00 = maps + ((int64_t)tz.x * g.nt[1] + ty.x) * g.nt[2] * nbins;
        const uint16_t* m01 = maps + ((int64_t)tz.x * g.nt[1] + ty.y) * g.nt[2] * nbins;
        const uint16_t* m10 = maps + ((int64_t)tz.y * g.nt[1] + ty.x) * g.nt[2] * nbins;
        const uint16_t* m11 = maps + ((int64_t)tz.y * g.nt[1] + ty.y) * g.nt[2] * nbins;
        const T* p = vol + z * sz + y * sy;
        uint16_t* drow = out + (int64_t)row * nx;
        for (int x = lane; x < nx; x += 64) {
            const int2 tx = tiles[nz + ny + x];
            const double2 cx = coef[nz + ny + x];
            const unsigned bin = bins[eq_key(p[x * sx])];
            const int64_t o0 = (int64_t)tx.x * nbins + bin, o1 = (int64_t)tx.y * nbins + bin;
            const unsigned v = eq_mix(m00[o0], m00[o1], m01[o0], m01[o1], m10[o0], m10[o1], m11[o0], m11[o1], cx, cy, cz);
            drow[x] = (uint16_t)v;
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
    }
    eq_fold_minmax(lo, hi, mm);
}

__global__ void __launch_bounds__(MMX_WG)
eq_output_kernel(const uint16_t* __restrict__ levels, int64_t n, const double* __restrict__ table,
                 double* __restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * MMX_WG + threadIdx.x; i < n; i += (int64_t)gridDim.x * MMX_WG) {
        const unsigned lv = levels[i];
        out[i] = table[lv < 16384u ? lv : 16383u];      // (a level is at most 16383: the bound only guards the table)
    }
}

template <typename T>
__global__ void __launch_bounds__(MMX_WG)
stretch_kernel(const T* __restrict__ vol, int64_t sz, int64_t sy, int64_t sx, int nz, int ny, int nx,
               double vmin, double vmax, double* __restrict__ out)
{
    const int rows = nz * ny;
    const int lane = threadIdx.x & 63;
    constexpr int WPG = MMX_WG / 64;
    const double span = vmax - vmin;
    for (int row = __builtin_amdgcn_readfirstlane((int)blockIdx.x * WPG + ((int)threadIdx.x >> 6)); row < rows;
         row += (int)gridDim.x * WPG) {
        const int z = row / ny, y = row - z * ny;
        const T* p = vol + z * sz + y * sy;
        double* drow = out + (int64_t)row * nx;
        for (int x = lane; x < nx; x += 64) {
            // np.clip = minimum(maximum(x, vmin), vmax) on the voxel converted to float64
            const double v = fmin(fmax((double)p[x * sx], vmin), vmax);
            drow[x] = (v - vmin) / span;
        }
    }
}

inline bool eq_geom_ok(const mmx_eq_geom* g)
{
    if (!g) return false;
    for (int a = 0; a < 3; ++a) {
        if (g->n[a] < 1 || g->k[a] < 1 || (int64_t)g->n[a] + 2 * (int64_t)g->k[a] >= (int64_t(1) << 31)) return false;
        if (g->nt[a] != (g->n[a] + g->k[a] - 1) / g->k[a]) return false;
    }
    return g->nbins >= 1 && g->nbins <= 16384;
}

inline unsigned eq_row_grid(int64_t rows)
{
    constexpr int WPG = MMX_WG / 64;
    return (unsigned)std::min<int64_t>((rows + 4 * WPG - 1) / (4 * WPG), 65535);
}

}  // namespace

extern "C" int mmx_eq_hist(const mmx_ds_view* src, const mmx_eq_geom* g, const uint16_t* d_bins, uint32_t* d_hist,
                           void* stream)
{
    if (!src || !src->d_data || !eq_geom_ok(g) || !d_bins || !d_hist) return MMX_ERR_ARG;
    const int64_t tiles = (int64_t)g->nt[0] * g->nt[1] * g->nt[2];
    const int64_t tile_vox = (int64_t)g->k[0] * g->k[1] * g->k[2];
    if (tiles > MMX_MAX_GRID_X || tile_vox >= (int64_t(1) << 31)) return MMX_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(d_hist, 0, (size_t)tiles * g->nbins * sizeof(uint32_t), s) != hipSuccess) return MMX_ERR_HIP;
    // enough workgroups to fill the chip whatever the number of tiles: a tile's rows are cut into parts of whole
    // rows, four at the least (one per wave)
    const int64_t rows = (int64_t)g->k[0] * g->k[1];
    int64_t parts = std::max<int64_t>(1, std::min<int64_t>(4096 / tiles, (rows + 3) / 4));
    parts = std::min<int64_t>(parts, 65535);
    const int rows_per_part = (int)((rows + parts - 1) / parts);
    parts = (rows + rows_per_part - 1) / rows_per_part;
    const int copies = g->nbins <= 1024 ? MMX_WG / 64 : 1;
    const size_t lds = (size_t)copies * g->nbins * sizeof(uint32_t);
    dim3 grid((unsigned)tiles, (unsigned)parts);
    mmx_timed_scope ts(MMX_K_PREPROC, s);
    return mmx_for_voxel<MMX_VOX_ALL>(src->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
        using T = MMX_TAG_T(t);
        hipLaunchKernelGGL(eq_hist_kernel<T>, grid, dim3(MMX_WG), lds, s, (const T*)src->d_data, src->stride_z,
                           src->stride_y, src->stride_x, *g, d_bins, d_hist, rows_per_part, copies);
        return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
    });
}

extern "C" int mmx_eq_apply(const mmx_ds_view* src, const mmx_eq_geom* g, const uint16_t* d_bins,
                            const uint16_t* d_maps, const int32_t* d_tiles, const int32_t* h_tiles,
                            const double* d_coef, uint16_t* d_out, uint32_t* d_minmax, void* stream)
{
    if (!src || !src->d_data || !eq_geom_ok(g) || !d_bins || !d_maps || !d_tiles || !h_tiles || !d_coef || !d_out ||
        !d_minmax)
        return MMX_ERR_ARG;
    if ((int64_t)g->n[0] * g->n[1] >= (int64_t(1) << 31)) return MMX_ERR_UNSUPPORTED;
    // every coordinate's two tiles lie in the map table
    int64_t at = 0;
    for (int a = 0; a < 3; ++a)
        for (int i = 0; i < g->n[a]; ++i, ++at)
            if (h_tiles[2 * at] < 0 || h_tiles[2 * at] >= g->nt[a] || h_tiles[2 * at + 1] < 0 ||
                h_tiles[2 * at + 1] >= g->nt[a])
                return MMX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(d_minmax, 0xff, sizeof(uint32_t), s) != hipSuccess ||
        hipMemsetAsync(d_minmax + 1, 0, sizeof(uint32_t), s) != hipSuccess)
        return MMX_ERR_HIP;
    // A block large enough to pay for staging its eight maps takes the LDS form (16 nbins bytes of LDS, at most 64 KiB);
    // small kernels and many bins read the maps through the caches, one wave per row of the image.
    const int64_t block_vox = (int64_t)g->k[0] * g->k[1] * g->k[2];
    const bool lds = g->nbins <= 4096 && g->k[2] >= 32 && block_vox >= 8 * (int64_t)g->nbins;
    const int64_t n_blocks = ((int64_t)g->nt[0] + 1) * (g->nt[1] + 1) * (g->nt[2] + 1);
    mmx_timed_scope ts(MMX_K_PREPROC, s);
    if (lds && n_blocks <= MMX_MAX_GRID_X) {
        // a workgroup's share of its block: at least 8 rows per wave, enough workgroups to fill the chip
        const int64_t rows = (int64_t)g->k[0] * g->k[1];
        const int64_t parts = std::max<int64_t>(1, std::min<int64_t>({4096 / n_blocks, rows / 32, (int64_t)65535}));
        dim3 grid_b((unsigned)n_blocks, (unsigned)parts);
        const size_t bytes = (size_t)8 * g->nbins * sizeof(uint16_t);
        return mmx_for_voxel<MMX_VOX_ALL>(src->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
            using T = MMX_TAG_T(t);
            hipLaunchKernelGGL(eq_apply_lds_kernel<T>, grid_b, dim3(MMX_WG), bytes, s, (const T*)src->d_data,
                               src->stride_z, src->stride_y, src->stride_x, *g, d_bins, d_maps, (const int2*)d_tiles,
                               (const double2*)d_coef, d_out, d_minmax);
            return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
        });
    }
    dim3 grid(eq_row_grid((int64_t)g->n[0] * g->n[1]));
    return mmx_for_voxel<MMX_VOX_ALL>(src->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
        using T = MMX_TAG_T(t);
        hipLaunchKernelGGL(eq_apply_kernel<T>, grid, dim3(MMX_WG), 0, s, (const T*)src->d_data, src->stride_z,
                           src->stride_y, src->stride_x, *g, d_bins, d_maps, (const int2*)d_tiles,
                           (const double2*)d_coef, d_out, d_minmax);
        return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
    });
}

extern "C" int mmx_eq_output(const uint16_t* d_levels, int64_t n, const double* d_table, double* d_out, void* stream)
{
    if (!d_levels || n < 1 || !d_table || !d_out) return MMX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)std::min<int64_t>((n + 4 * MMX_WG - 1) / (4 * MMX_WG), 1 << 20));
    mmx_timed_scope ts(MMX_K_PREPROC, s);
    hipLaunchKernelGGL(eq_output_kernel, grid, dim3(MMX_WG), 0, s, d_levels, n, d_table, d_out);
    return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
}

extern "C" int mmx_stretch(const mmx_ds_view* src, int nz, int ny, int nx, double vmin, double vmax, double* d_out,
                           void* stream)
{
    if (!src || !src->d_data || nz < 1 || ny < 1 || nx < 1 || !d_out || !(vmin < vmax)) return MMX_ERR_ARG;
    if ((int64_t)nz * ny >= (int64_t(1) << 31)) return MMX_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(eq_row_grid((int64_t)nz * ny));
    mmx_timed_scope ts(MMX_K_PREPROC, s);
    return mmx_for_voxel<MMX_VOX_ALL>(src->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
        using T = MMX_TAG_T(t);
        hipLaunchKernelGGL(stretch_kernel<T>, grid, dim3(MMX_WG), 0, s, (const T*)src->d_data, src->stride_z,
                           src->stride_y, src->stride_x, nz, ny, nx, vmin, vmax, d_out);
        return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
    });
}
