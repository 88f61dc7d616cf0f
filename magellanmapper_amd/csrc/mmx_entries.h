// The NMS entry contract of include/mmx.h (d_nms_mask) as code: where the entry and bit of a voxel lie in either
// layout, and how a Y pass decides them.  Every producer (y2_kernel, y6_kernel, ym_kernel, wide_y), the consumer
// (peaks_sparse_kernel) and the host's "do they fit" (mmx_batch_geom_make) take it from here; tools/route_check.cpp
// sweeps the host side.
//
// An entry is two 64-bit words about 64 voxels of one row y: word 0 (.x) one bit per candidate, word 1 (.y) one bit per
// voxel above nms_lo.  A voxel is a candidate when it is above nms_lo and neither of its y neighbours nor an x
// neighbour that shares its entry exceeds it by more than nms_eps -- a superset of the local maxima, decided on the
// float32 values the Y pass has in registers.  The 64 voxels of an entry whose word 1 is zero are not stored to d_log.
//   MMX_MASK_ROWS  : 64 consecutive columns c = z px + x of the (z, x) plane of row y
//   MMX_MASK_QUADS : 4 planes x 16 columns, the footprint of one wave of the tiled Y kernels
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mmx.h"

#define MMX_HD __host__ __device__ __forceinline__

// ---------------------------------------------------------------- host and device: the layouts
// entries per row y.  I = int inside the kernels; int64_t where a block has not been checked yet (mmx_entries_fit)
template <typename I>
MMX_HD I mmx_entries_per_row(int layout, I nz, int nx, int px)
{
    return layout == MMX_MASK_QUADS ? ((nz + 3) >> 2) * ((nx + 15) >> 4) : (nz * px + 63) >> 6;
}
// first entry of the block in `slot`
MMX_HD int64_t mmx_entry_base(int slot, int64_t slot_elems) { return ((int64_t)slot * slot_elems) >> 5; }
// whether the ny rows of a block fit its share of the slot, (slot_elems >> 5) entries less one
MMX_HD bool mmx_entries_fit(int layout, int nz, int ny, int nx, int px, int64_t slot_elems)
{
    return (int64_t)ny * mmx_entries_per_row<int64_t>(layout, nz, nx, px) <= (slot_elems >> 5) - 1;
}

struct mmx_entry_geom {
    int quads;      // layout == MMX_MASK_QUADS
    int ntx;        // quads: entries per 4 planes, ceil(nx / 16)
    int px;         // rows: the row pitch
    int per_row;    // entries per row y
};
MMX_HD mmx_entry_geom mmx_entry_geom_make(int layout, int nz, int nx, int px)
{
    return mmx_entry_geom{layout == MMX_MASK_QUADS, (nx + 15) >> 4, px, mmx_entries_per_row<int>(layout, nz, nx, px)};
}
// MMX_MASK_ROWS by column c = z px + x of the flattened (z, x) plane: its entry within row y
MMX_HD int mmx_rows_entry(int col) { return col >> 6; }
// MMX_MASK_QUADS by plane quad z >> 2 and column tile x >> 4: what a wave of the tiled Y kernels knows of its footprint
MMX_HD int mmx_quads_entry(const mmx_entry_geom& g, int zquad, int xtile) { return zquad * g.ntx + xtile; }
// entry of voxel (z, x) within its row y, and its bit there
MMX_HD int mmx_entry_index(const mmx_entry_geom& g, int z, int x)
{
    return g.quads ? mmx_quads_entry(g, z >> 2, x >> 4) : mmx_rows_entry(z * g.px + x);
}
MMX_HD int mmx_entry_bit(const mmx_entry_geom& g, int z, int x)
{
    return g.quads ? ((z & 3) << 4) | (x & 15) : (z * g.px + x) & 63;
}
// the inverse (bits of pitch columns and of planes past the block come back with x >= nx or z >= nz)
MMX_HD void mmx_entry_voxel(const mmx_entry_geom& g, int entry, int bit, int* z, int* x)
{
    if (g.quads) {
        const int zq = entry / g.ntx;
        *z = 4 * zq + (bit >> 4);
        *x = 16 * (entry - zq * g.ntx) + (bit & 15);
    } else {
        const int col = (entry << 6) + bit;
        *z = col / g.px;
        *x = col - *z * g.px;
    }
}

// ---------------------------------------------------------------- device: deciding a row
// word 1 of a row: the lanes whose value is above the threshold
__device__ __forceinline__ unsigned long long mmx_above_word(bool real, float v, float lo)
{
    return __ballot(real & (v > lo));
}
__device__ __forceinline__ float mmx_fmax(float a) { return a; }
template <typename... F>
__device__ __forceinline__ float mmx_fmax(float a, float b, F... more) { return mmx_fmax(fmaxf(a, b), more...); }
// the candidate rule; the neighbours tested: n0, more...
template <typename... F>
__device__ __forceinline__ bool mmx_candidate(bool real, float v, float lo, float eps, float n0, F... more)
{
    return real & (v > lo) & !(mmx_fmax(n0, more...) > v + eps);
}
// the larger x neighbour of every lane by DPP shifts (no LDS crossbar traffic), WAVE: across the 64 lanes
// (MMX_MASK_ROWS), else inside rows of 16 lanes (MMX_MASK_QUADS).  Lanes with no source keep v, which has_l / has_r
// discard: the first and last column of an entry are not tested against the next entry.
template <bool WAVE>
__device__ __forceinline__ float mmx_x_neighbours(float v, bool has_l, bool has_r)
{
    const int b = (int)__float_as_uint(v);
    const float l = __uint_as_float((unsigned)__builtin_amdgcn_update_dpp(b, b, WAVE ? 0x138 /* wave_shr:1 */ : 0x111 /* row_shr:1 */, 0xf, 0xf, false));
    const float r = __uint_as_float((unsigned)__builtin_amdgcn_update_dpp(b, b, WAVE ? 0x130 /* wave_shl:1 */ : 0x101 /* row_shl:1 */, 0xf, 0xf, false));
    return fmaxf(has_l ? l : -INFINITY, has_r ? r : -INFINITY);
}

// A wave marching along y decides row y - 1 when row y is known (y2_kernel; y6_kernel and ym_kernel keep the same state
// in locals of their own: in this struct it costs them two or three registers).  SKIP: a row with nothing above the
// threshold has no candidates, so its test is skipped (wave-uniform branch; the entry is the same).
template <bool SKIP>
struct mmx_pending_row {
    float prev1 = -INFINITY, prev2 = -INFINITY;     // values of rows y - 1, y - 2
    float nbx_prev = -INFINITY;                     // x-neighbour maximum of row y - 1
    unsigned long long ab_prev = 0;                 // word 1 of row y - 1
    int ydone = 0;                                  // rows pushed
    ulonglong2* mrow;                               // entry of row y - 1
    int stride;                                     // entries per row y
    bool real;                                      // this lane holds a voxel
    float lo, eps;
    __device__ __forceinline__ mmx_pending_row(ulonglong2* row0, int per_row, bool real_, float lo_, float eps_)
        : mrow(row0), stride(per_row), real(real_), lo(lo_), eps(eps_) {}

    // word 0 of row y - 1, its successor (and whatever else) among `more`
    template <typename... F>
    __device__ __forceinline__ unsigned long long decide(F... more) const
    {
        unsigned long long m = 0;
        if (!SKIP || ab_prev) m = __ballot(mmx_candidate(real, prev1, lo, eps, prev2, more...));
        return m;
    }
    __device__ __forceinline__ void push(float v, unsigned long long ab, float nbx)
    {
        if (ydone > 0) {
            const unsigned long long m = decide(v, nbx_prev);
            if ((threadIdx.x & 63) == 0) *mrow = make_ulonglong2(m, ab_prev);
            mrow += stride;
        }
        prev2 = prev1; prev1 = v; nbx_prev = nbx;
        ab_prev = ab;
        ++ydone;
    }
    // the last row has no successor
    __device__ __forceinline__ void finish()
    {
        const unsigned long long m = decide(nbx_prev);
        if ((threadIdx.x & 63) == 0) *mrow = make_ulonglong2(m, ab_prev);
    }
};
