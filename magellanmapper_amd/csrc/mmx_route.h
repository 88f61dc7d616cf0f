// Which kernel path takes a scale: the host-only predicates (geometry and radius in, yes / no out -- no launch, no
// device state), and the layout of a ladder that holds wide radii.  mmx_log_scale_f32 (mmx_api.hip) routes a call by
// them, mmx_log_scales_f32 (mmx_detect.hip) lays a batch out with them before its first launch, and
// tools/route_check.cpp runs them over a table of geometries under the host sanitizers.
// Included by mmx_common.h (it needs mmx_batch_geom).
#pragma once

// the register-ring column kernels prefetch this many steps ahead and reflect once
#define MMX_COL_PREFETCH 4
// widest row pitch (floats) zx2_kernel takes: 5 producer waves (mmx_fused2.hip, kMaxPx)
#define MMX_PACKED_MAX_PX 320

// "the wide passes take this radius on this geometry": radius 1 .. 64, u8 / u16 / f32 voxels, every extent of every
// block at least the radius (one reflection then covers every tap), any row width
inline bool mmx_wide_accepts(const mmx_volume* vol, const mmx_batch_geom& g, int radius)
{
    if (radius < 1 || radius > MMX_MAX_RADIUS_WIDE) return false;
    if (vol->dtype != MMX_U8 && vol->dtype != MMX_U16 && vol->dtype != MMX_F32) return false;
    return g.status == MMX_OK && g.min_nz >= radius && g.min_ny >= radius && g.min_nx >= radius;
}

// "the fused path (Z+X in one kernel, then Y) takes this radius on this geometry"
inline bool mmx_fused_accepts(const mmx_volume* vol, const mmx_batch_geom& g, int radius)
{
    const bool fast_r = radius >= 1 && radius <= MMX_MAX_RADIUS_FAST;
    const bool lane_ok = g.max_lane_in * 8 < (int64_t(1) << 31);
    return fast_r && lane_ok && g.min_ny >= radius + MMX_COL_PREFETCH && g.min_nz >= radius + 1 && g.min_nx >= radius &&
           g.max_px <= 512 && vol->stride_y < (1 << 30);
}

// ... and its packed-VALU kernel in particular (MMX_ZX_PACKED by name: zx2_kernel's own limits on top)
inline bool mmx_packed_accepts(const mmx_volume* vol, const mmx_batch_geom& g, int radius)
{
    return mmx_fused_accepts(vol, g, radius) && g.max_px <= MMX_PACKED_MAX_PX &&
           vol->stride_z * 8 * (int64_t)sizeof(double) < (int64_t(1) << 32);
}

// The ladder rule of mmx_log_scales_f32 under MMX_ZX_AUTO.  Returns false -- nothing written -- for a ladder without a
// radius above MMX_MAX_RADIUS_FAST that the wide passes accept: it runs the rounds it always ran.  Otherwise modes[s] is
// the mmx_zx_mode of scale s for the ONE round: radii above MMX_MAX_RADIUS_FAST go wide, the others MMX_ZX_PACKED where
// that kernel takes them and wide where it does not, a scale neither takes stays MMX_ZX_AUTO (it will end on the
// separate / generic passes); *entries: every scale writes row entries (they fit, and no scale stayed AUTO).
inline bool mmx_ladder_layout(const mmx_volume* vol, const mmx_batch_geom& g, const int32_t* radii, int n_sigma,
                              int32_t* modes, bool* entries)
{
    bool any_wide = false;
    for (int s = 0; s < n_sigma; ++s)
        if (radii[s] > MMX_MAX_RADIUS_FAST && mmx_wide_accepts(vol, g, radii[s])) any_wide = true;
    if (!any_wide) return false;
    *entries = g.rows_fit;
    for (int s = 0; s < n_sigma; ++s) {
        const int r = radii[s];
        if (r <= MMX_MAX_RADIUS_FAST && mmx_packed_accepts(vol, g, r)) modes[s] = MMX_ZX_PACKED;
        else if (mmx_wide_accepts(vol, g, r)) modes[s] = MMX_ZX_WIDE;
        else { modes[s] = MMX_ZX_AUTO; *entries = false; }
    }
    return true;
}
