// Which kernel path takes a scale: THE ONE STATEMENT of the rules.  Everything here is host-only and pure -- the volume
// header, the batch geometry, the radii and weights, the band and the requested mode in; a route record out; no launch,
// no device state.
//   mmx_*_accepts     : the conditions on which a launcher takes a call; the launcher's first line asks the same function
//   mmx_route_scale   : the route of one scale of one batch (what mmx_log_batch_f32 obeys)
//   mmx_route_ladder  : the routes of all scales of a batch, in one NMS entry layout or none (mmx_log_scales_f32)
// mmx_api.hip / mmx_detect.hip launch what a route says and decide nothing; tools/route_check.cpp tabulates the rules and
// sweeps them under the host sanitizers.  Included by mmx_common.h (it needs mmx_batch_geom).
#pragma once

#include <cmath>
#include <cstddef>
#include <vector>

// (MMX_COL_PREFETCH -- the register-ring column kernels prefetch this many steps ahead and reflect once -- and
//  MMX_FOLD_MAX_N: include/mmx.h)
// widest row pitch (floats) zx2_kernel takes: 5 producer waves
#define MMX_PACKED_MAX_PX 320
// (the tiled kernels take any row pitch: their voxel copy is made in x panels of 512 columns, and what bounds a block is
//  its plan -- 32-bit offsets inside a block's tiles and copy, the workspace, MMX_ZX4_MAXCLS width / depth classes)
// largest radius of the matrix-core Y pass (ym_kernel)
#define MMX_YM_MAX_RADIUS 24
// xpass_kernel: outputs per thread; 16-byte loads and halo loads per thread, array and row group
#define MMX_X_OUTPUTS 8
#define MMX_X_MAX_QUADS 2
#define MMX_X_MAX_HALO 2
#define MMX_X_THREADS 256
#define MMX_LDS_BYTES (64 * 1024)

// ---------------------------------------------------------------------------------------------------- the request
struct mmx_zx_request { int mode; bool y_valu, prepacked, edge_global; int rows; };
// zx_mode with its flags -> the mode and the flags; MMX_ERR_ARG for a value that names no kernel path
inline int mmx_zx_parse(int zx_mode, mmx_zx_request* q)
{
    q->y_valu = zx_mode >= 0 && (zx_mode & MMX_ZX_Y_VALU);
    if (q->y_valu) zx_mode &= ~MMX_ZX_Y_VALU;
    q->edge_global = zx_mode >= 0 && (zx_mode & MMX_ZX_EDGE_GLOBAL);
    if (q->edge_global) zx_mode &= ~MMX_ZX_EDGE_GLOBAL;
    q->rows = zx_mode >= 0 ? (zx_mode & MMX_ZX_ROWS_MASK) >> MMX_ZX_ROWS_SHIFT : 0;
    if (q->rows) zx_mode &= ~MMX_ZX_ROWS_MASK;
    q->prepacked = zx_mode == (MMX_ZX_TILED | MMX_ZX_PREPACKED) || zx_mode == (MMX_ZX_TILED_Q16 | MMX_ZX_PREPACKED);
    if (q->prepacked) zx_mode &= ~MMX_ZX_PREPACKED;
    q->mode = zx_mode;
    if (zx_mode < MMX_ZX_AUTO || zx_mode > MMX_ZX_THIN || zx_mode == 1 || (zx_mode >= 3 && zx_mode <= 5))
        return MMX_ERR_ARG;             // (3, 4, 5: retired experiment kernels)
    return MMX_OK;
}

// ---------------------------------------------------------------------------------------------------- the launchers
inline bool mmx_voxels_ok(const mmx_volume* vol) { return mmx_voxel_in(vol->dtype, MMX_VOX_LOG); }
// integer voxels: their value range is the type's (img_as_float), and its span -- 1 for the unsigned types' [0, 1],
// 2 for int16's [-1, 1], which the tiled path carries as [0, 2] (the copy holds x ^ 0x8000) less each scale's constant
inline bool mmx_voxels_integer(const mmx_volume* vol) { return mmx_voxel_in(vol->dtype, MMX_VOX_INTEGER); }
inline double mmx_integer_span(const mmx_volume* vol) { return mmx_voxel(vol->dtype)->span; }
inline bool mmx_ring_radius(int radius) { return radius >= 1 && radius <= MMX_MAX_RADIUS_FAST; }
// 32-bit lane offsets into the input plane of a block
inline bool mmx_lane_ok(const mmx_volume* vol, const mmx_batch_geom& g)
{
    return g.max_lane_in * 8 < (int64_t(1) << 31) && vol->stride_y < (1 << 30);
}

// "the wide passes take this radius on this geometry": radius 1 .. 64, u8 / u16 / f32 voxels, every extent of every
// block at least the radius (one reflection then covers every tap), any row width.  (mmx_launch_wide_pass keeps two
// guards of its own that no batch past the argument checks can meet -- a grid beyond 2^31 - 1 workgroups: a slot holds
// less than 2^29 elements; staged rows beyond the LDS: 16 rows x 265 pairs = 33 920 bytes at the most, radius 64.)
inline bool mmx_wide_launch_accepts(const mmx_volume* vol, int radius)
{
    return radius >= 1 && radius <= MMX_MAX_RADIUS_WIDE && mmx_voxels_ok(vol);
}
inline bool mmx_wide_accepts(const mmx_volume* vol, const mmx_batch_geom& g, int radius)
{
    return mmx_wide_launch_accepts(vol, radius) && g.status == MMX_OK && g.min_nz >= radius && g.min_ny >= radius && g.min_nx >= radius;
}

// the register-ring kernels of the separate passes, per pass
inline bool mmx_zpass_accepts(const mmx_volume* vol, const mmx_batch_geom& g, int radius)
{
    return mmx_ring_radius(radius) && mmx_voxels_ok(vol) && mmx_lane_ok(vol, g) && g.min_nz >= radius + MMX_COL_PREFETCH;
}
inline bool mmx_ypass_accepts(const mmx_batch_geom& g, int radius)
{
    return mmx_ring_radius(radius) && g.min_ny >= radius + MMX_COL_PREFETCH;
}
// xpass_kernel's launch shape for rows up to max_nx voxels: row pitch, staged pitch, rows per workgroup, LDS bytes
struct mmx_xpass_shape { int px, pw, ch, rg; size_t lds_bytes; };
inline mmx_xpass_shape mmx_xpass_shape_of(int max_nx, int R)
{
    mmx_xpass_shape x;
    const int lead = R & 1, s = (R + lead + 7) & ~7;
    x.px = (max_nx + MMX_ROW_ALIGN - 1) / MMX_ROW_ALIGN * MMX_ROW_ALIGN;
    const int span = s + x.px + R + lead;
    x.pw = ((span + 2 * (span >> 3)) + 3) & ~1;
    x.ch = (max_nx + MMX_X_OUTPUTS - 1) / MMX_X_OUTPUTS;
    // rows per group: as many as the threads cover, within the per-thread prefetch registers
    x.rg = x.ch > 0 ? MMX_X_THREADS / x.ch : 1;
    if (x.rg < 1) x.rg = 1;
    while (x.rg > 1 && (x.rg * (x.px / 4) > MMX_X_MAX_QUADS * MMX_X_THREADS || x.rg * 2 * R > MMX_X_MAX_HALO * MMX_X_THREADS)) --x.rg;
    x.lds_bytes = ((size_t)2 * x.rg * x.pw + (size_t)x.rg * x.px) * sizeof(float);
    return x;
}
inline bool mmx_xpass_launch_accepts(int max_nx, int radius)
{
    if (!mmx_ring_radius(radius) || max_nx < 1) return false;
    const mmx_xpass_shape x = mmx_xpass_shape_of(max_nx, radius);
    if (x.px / 4 > MMX_X_MAX_QUADS * MMX_X_THREADS || 2 * radius > MMX_X_MAX_HALO * MMX_X_THREADS) return false;
    if (x.ch > MMX_X_THREADS) return false;         // rows wider than 2048 voxels: the generic pass
    return x.lds_bytes <= MMX_LDS_BYTES;
}
inline bool mmx_xpass_accepts(const mmx_batch_geom& g, int radius)
{
    return g.min_nx >= radius && mmx_xpass_launch_accepts(g.max_nx, radius);
}

// "this batch is thin at this radius": a block shorter than radius + MMX_COL_PREFETCH along some axis -- what sends a
// pass of the separate passes off its register-ring kernel, and what MMX_ZX_THIN by name takes (a ladder: at its
// largest radius).  The folded pass that then runs (mmx_launch_fold_pass) takes any radius up to
// MMX_MAX_RADIUS_GENERIC and any extent: it folds the blocks of extent <= MMX_FOLD_MAX_N and runs the tap loop on the rest.
inline bool mmx_thin_accepts(const mmx_batch_geom& g, int radius)
{
    const int thin_below = radius + MMX_COL_PREFETCH;
    return radius >= 0 && radius <= MMX_MAX_RADIUS_GENERIC && g.status == MMX_OK &&
           (g.min_nz < thin_below || g.min_ny < thin_below || g.min_nx < thin_below);
}

// "the fused path (Z+X in one kernel, then Y) takes this radius on this geometry"
inline bool mmx_fused_accepts(const mmx_volume* vol, const mmx_batch_geom& g, int radius)
{
    return mmx_ring_radius(radius) && mmx_lane_ok(vol, g) && g.min_ny >= radius + MMX_COL_PREFETCH && g.min_nz >= radius + 1 &&
           g.min_nx >= radius;
}
// zx2_kernel's own limits: the row pitch its producer waves cover, 32-bit scalar plane offsets
inline bool mmx_zx2_launch_accepts(const mmx_volume* vol, int max_px, int radius)
{
    return mmx_ring_radius(radius) && mmx_voxels_ok(vol) && max_px <= MMX_PACKED_MAX_PX &&
           vol->stride_z * 8 * (int64_t)sizeof(double) < (int64_t(1) << 32);
}
// ... and the packed-VALU kernel of the fused path in particular (MMX_ZX_PACKED by name)
inline bool mmx_packed_accepts(const mmx_volume* vol, const mmx_batch_geom& g, int radius)
{
    return mmx_fused_accepts(vol, g, radius) && mmx_zx2_launch_accepts(vol, g.max_px, radius);
}
// ... and its tiled matrix-core kernels: the plan fits the workspace (which covers the Toeplitz tables of every radius
// class and the number of width / depth classes), one reflection covers every tap
inline bool mmx_zx6_launch_accepts(const mmx_volume* vol, int min_nz, int min_nx, int radius)
{
    return mmx_ring_radius(radius) && mmx_voxels_ok(vol) && min_nx >= radius && min_nz >= radius;
}
inline bool mmx_tiled_accepts(const mmx_volume* vol, const mmx_batch_geom& g, int radius)
{
    return mmx_fused_accepts(vol, g, radius) && g.plan_status == MMX_OK && mmx_zx6_launch_accepts(vol, g.min_nz, g.min_nx, radius);
}
// the matrix-core Y pass: 16-bit tiles (cp, cq: what a count of P / of Q is worth), weights float16 can hold once scaled
inline bool mmx_ym_accepts(const float* w0, const float* w2, int radius, float cp, float cq)
{
    if (radius < 1 || radius > MMX_YM_MAX_RADIUS || radius > MMX_MAX_RADIUS_FAST || !(cp > 0.f) || !(cq > 0.f)) return false;
    float mx = 0.f;
    for (int k = 0; k <= radius; ++k) mx = fmaxf(mx, fmaxf(fabsf(w2[k] * cp), fabsf(w0[k] * cq)));
    return mx > 1e-30f && mx < 1e30f;
}

// ---------------------------------------------------------------------------------------------------- 16-bit tiles
// Q16 tiles (MMX_ZX_TILED_Q16): P in [0, BP] as unorm16, Q in [-BQ, BQ] as snorm16.  For voxels in [0, 1] (integer
// types after img_as_float) the bounds follow from the weights alone.  |P| <= (sum w0)^2.  Q = sum K I with the 2-D
// kernel K(i, j) = w2(i) w0(j) + w0(i) w2(j) and every voxel I in [0, 1], so Q lies in [-sum of K's negative taps, sum of
// its positive taps] -- about HALF of sum|K| <= 2 sum|w2| sum w0 either way, a second-derivative kernel summing to ~0
// (round 6: BQ is that, the larger of the two one-sided sums; rounds 3-5 quantised Q over the two-sided 2 sum|w2| sum w0
// and carried twice the rounding error for it).  Folding reflected taps at a block face only merges weights, which
// can only shrink both one-sided sums.  The error the rounding leaves in the LoG value follows likewise:
//   norm (sum|w2| BP / 65535 + sum w0 BQ / 32767) / 2,
// i.e. 2.2e-5 whatever sigma (sum|w2| ~ 0.97 / sigma^2), plus the float32 arithmetic's own few 1e-7, the product
// term the 16-bit kernel leaves out (0.55e-5) and the rounding of its X accumulators, which run with the voxel
// pieces' exponent offsets still in them (values up to 8 instead of 1: four roundings of 2^-22 each, 0.2e-5):
// 3.0e-5; the Y pass on the matrix cores (mmx_ymfma.hip) leaves out its own low x low product -- low byte of a count x
// (weight - float16(weight)): 255 x 2^-12 = 0.062 counts per unit of weight against the 0.5 of the rounding -- which adds an
// eighth: 3.3e-5 in all (5.1e-5 with the two-sided BQ).
inline void mmx_q16_bounds(const double* w0, const double* w2, int radius, double norm, double* bp, double* bq, double* err)
{
    double s0 = w0[0], s2 = fabs(w2[0]);
    for (int k = 1; k <= radius; ++k) { s0 += 2.0 * w0[k]; s2 += 2.0 * fabs(w2[k]); }
    *bp = s0 * s0 * (1.0 + 1e-6);
    // one-sided sums of K over its (2 R + 1)^2 taps (K is symmetric in both indices: a quadrant, weighted)
    double pos = 0.0, neg = 0.0;
    for (int i = 0; i <= radius; ++i)
        for (int j = 0; j <= radius; ++j) {
            const double k = (w2[i] * w0[j] + w0[i] * w2[j]) * ((i ? 2.0 : 1.0) * (j ? 2.0 : 1.0));
            if (k > 0.0) pos += k; else neg -= k;
        }
    // (1e-4 of slack: the kernel's own float32 / split-float16 arithmetic may land a hair beyond the exact extreme, and
    //  a value beyond BQ would clamp)
    *bq = (pos > neg ? pos : neg) * (1.0 + 1e-4);
    // ... plus what the 16-bit kernel drops in the X pass (low voxel byte x low weight piece: 255 / 65536 x 2^-11 per
    // unit of weight): P off by 1.9e-6 s0^2, Q by 1.9e-6 x 2 s2 s0
    const double drop = 255.0 / 65536.0 / 2048.0;
    // ... and the float32 rounding of X accumulators that carry the pieces' offsets (<= 8: ulp 2^-21, half of it per
    // MFMA, four MFMAs into each; relative to the bounds, the fragments carry 1 / bound)
    const double biased = 4.0 * 0x1p-22;
    // ... and the Y pass's dropped product, in counts of P and of Q
    const double ydrop = 255.0 / 4096.0;
    *err = norm * (s2 * (*bp / 65535.0 * (0.5 + ydrop) + drop * s0 * s0 + biased * *bp) +
                   s0 * (*bq / 32767.0 * (0.5 + ydrop) + drop * 2.0 * s2 * s0 + biased * *bq)) + 1e-6;
}
// (what the ABI's mmx_tiled_q16_error_bound returns)
inline double mmx_q16_error_bound(const double* w0, const double* w2, int radius, double norm)
{
    if (!w0 || !w2 || radius < 0 || radius > MMX_MAX_RADIUS_GENERIC) return -1.0;
    double bp, bq, err;
    mmx_q16_bounds(w0, w2, radius, norm, &bp, &bq, &err);
    return err;
}

// The tile choice of the tiled path, float32 or 16-bit: unit_bound = mmx_q16_error_bound of the scale(s) the answer is
// for, band = the nomination band.  *value_scale: value units per unit of the [0, 1] range that bound is stated for -- 1
// for unsigned integer voxels (img_as_float), 2 for int16 (mmx_integer_span), m for float voxels that state a range
// [0, m], 0 when 16-bit tiles cannot hold the voxels.
inline bool mmx_tiles_q16(int zx_mode, const mmx_volume* vol, double unit_bound, double band, bool entries, double* value_scale)
{
    const bool ranged = vol->dtype == MMX_F32 && vol->value_range > 0.f && vol->value_range < 60000.f;
    *value_scale = mmx_voxels_integer(vol) ? mmx_integer_span(vol) : (ranged ? (double)vol->value_range : 0.0);
    if (!(*value_scale > 0.0)) return false;
    // (by name: taken whatever the band; the caller's run-time check of |float32 - float64| against eps / 4 on the
    //  re-scored candidates is what then widens it)
    if (zx_mode == MMX_ZX_TILED_Q16) return true;
    const double bound = unit_bound * *value_scale;
    return zx_mode == MMX_ZX_AUTO && entries && bound >= 0.0 && 4.0 * bound <= band && bound <= MMX_LOG_ABS_TOL;
}

// ---------------------------------------------------------------------------------------------------- one scale
enum mmx_route_family { MMX_ROUTE_SEPARATE = 0, MMX_ROUTE_WIDE, MMX_ROUTE_TILED, MMX_ROUTE_PACKED };
enum mmx_route_y { MMX_Y_NONE = 0, MMX_Y_YM, MMX_Y_Y6, MMX_Y_Y2 };
struct mmx_route {
    int family;                 // mmx_route_family
    bool q16;                   // tiled: 16-bit tiles (else float32)
    bool makes_copy;            // tiled: this scale makes the voxel copy itself ...
    bool trusts_copy;           // ... or trusts the batch's (MMX_ZX_PREPACKED)
    bool edge_global;           // tiled: edge z tiles take their Z fragments from global memory (MMX_ZX_EDGE_GLOBAL)
    int zx_rows;                // tiled: rows per wave of the Z+X row march (MMX_ZX_ROWS), 0 = chosen per block of the launch
    int y_kernel;               // mmx_route_y (fused families)
    bool ring_z, ring_y, ring_x;// separate: per pass, the register-ring kernel (else the generic one, or the folded one:)
    bool fold_z, fold_y, fold_x;// separate, MMX_ZX_THIN: per pass, the folded-reflection pass
    int layout;                 // NMS entry layout the scale writes: 0, MMX_MASK_ROWS, MMX_MASK_QUADS
    int path;                   // mmx_zx_mode reported through h_zx_path
    double bp, bq;              // q16: the bounds of P and Q in value units
};

// The route of one scale.  `zx_mode` with its flags as the caller passed it; `entries`: the caller wants NMS entries.
// The chain: the wide passes by name, or under MMX_ZX_AUTO above MMX_MAX_RADIUS_FAST, where they accept; else the fused
// path where it accepts (unless MMX_ZX_SEPARATE) -- tiled when named or, under AUTO, for integer or ranged float voxels,
// and the plan fits, on 16-bit tiles by mmx_tiles_q16's rule; else its packed kernel where that accepts; else the three
// separate passes, each on its register-ring kernel where that accepts and on the generic one where not.
// MMX_ZX_THIN by name: a batch that is thin at `thin_radius` (mmx_thin_accepts; < 0: at this scale's own radius -- a
// ladder passes its largest) takes the separate passes with the folded pass in the generic one's place, path
// MMX_ZX_THIN, no entries; any other batch goes on as under MMX_ZX_AUTO.
// Returns MMX_OK or the status the call ends with (bad mode / radius: MMX_ERR_ARG; radius above MMX_MAX_RADIUS_GENERIC,
// float64 voxels: MMX_ERR_UNSUPPORTED; else the geometry's).
inline int mmx_route_scale(const mmx_volume* vol, const mmx_batch_geom& g, int radius, const double* w0, const double* w2,
                           double norm, int zx_mode, double band, bool entries, mmx_route* r, int thin_radius = -1)
{
    *r = mmx_route{};
    r->path = MMX_ZX_SEPARATE;
    mmx_zx_request q;
    if (mmx_zx_parse(zx_mode, &q) != MMX_OK || radius < 0) return MMX_ERR_ARG;
    if (radius > MMX_MAX_RADIUS_GENERIC || !mmx_voxels_ok(vol)) return MMX_ERR_UNSUPPORTED;
    if (g.status != MMX_OK) return g.status;
    if (q.mode == MMX_ZX_THIN) {
        if (mmx_thin_accepts(g, thin_radius < 0 ? radius : thin_radius)) {
            r->family = MMX_ROUTE_SEPARATE;
            r->path = MMX_ZX_THIN;
            r->ring_z = mmx_zpass_accepts(vol, g, radius);
            r->ring_y = mmx_ypass_accepts(g, radius);
            r->ring_x = mmx_xpass_accepts(g, radius);
            r->fold_z = !r->ring_z;
            r->fold_y = !r->ring_y;
            r->fold_x = !r->ring_x;
            return MMX_OK;
        }
        q.mode = MMX_ZX_AUTO;
    }
    if ((q.mode == MMX_ZX_WIDE || (q.mode == MMX_ZX_AUTO && radius > MMX_MAX_RADIUS_FAST)) && mmx_wide_accepts(vol, g, radius)) {
        r->family = MMX_ROUTE_WIDE;
        r->path = MMX_ZX_WIDE;
        r->layout = entries && g.rows_fit ? MMX_MASK_ROWS : 0;
        return MMX_OK;
    }
    if (q.mode != MMX_ZX_SEPARATE && mmx_fused_accepts(vol, g, radius)) {
        // float voxels: the tiled path when the volume states its value range (or when asked for by name: the float16
        // pieces of its copy cover |v| < 65504), 16-bit tiles when that range is [0, m]: their bounds scale with m
        const bool integer = mmx_voxels_integer(vol);
        const bool ranged = vol->dtype == MMX_F32 && vol->value_range != 0.f && fabsf(vol->value_range) < 60000.f;
        double bp, bq, err, vscale;
        mmx_q16_bounds(w0, w2, radius, norm, &bp, &bq, &err);
        const bool q16 = mmx_tiles_q16(q.mode, vol, err, band, entries, &vscale);
        const bool named = q.mode == MMX_ZX_TILED || (q.mode == MMX_ZX_TILED_Q16 && vscale > 0.0);
        if ((named || (q.mode == MMX_ZX_AUTO && (integer || ranged))) && mmx_tiled_accepts(vol, g, radius)) {
            r->family = MMX_ROUTE_TILED;
            r->q16 = q16;
            r->trusts_copy = q.prepacked;
            r->makes_copy = !q.prepacked;
            r->edge_global = q.edge_global;
            r->zx_rows = q.rows;
            r->path = q16 ? MMX_ZX_TILED_Q16 : MMX_ZX_TILED;
            r->layout = entries && g.quads_fit ? MMX_MASK_QUADS : 0;
            r->y_kernel = MMX_Y_Y6;
            if (q16) {
                r->bp = bp * vscale;
                r->bq = bq * vscale;
                float y0[MMX_MAX_RADIUS_FAST + 1], y2[MMX_MAX_RADIUS_FAST + 1];     // the Y pass's weights, as it gets them
                for (int k = 0; k <= radius; ++k) { y0[k] = (float)(-norm * w0[k]); y2[k] = (float)(-norm * w2[k]); }
                if (!q.y_valu && mmx_ym_accepts(y0, y2, radius, (float)(r->bp / 65535.0), (float)(r->bq / 32767.0)))
                    r->y_kernel = MMX_Y_YM;
            }
            return MMX_OK;
        }
        if (mmx_packed_accepts(vol, g, radius)) {
            r->family = MMX_ROUTE_PACKED;
            r->path = MMX_ZX_PACKED;
            r->layout = entries && g.rows_fit ? MMX_MASK_ROWS : 0;
            r->y_kernel = MMX_Y_Y2;
            return MMX_OK;
        }
    }
    r->family = MMX_ROUTE_SEPARATE;
    r->ring_z = mmx_zpass_accepts(vol, g, radius);
    r->ring_y = mmx_ypass_accepts(g, radius);
    r->ring_x = mmx_xpass_accepts(g, radius);
    return MMX_OK;
}

// ---------------------------------------------------------------------------------------------------- a ladder
// What mmx_log_scales_f32 does for a batch, beside the route of every scale.
struct mmx_ladder_route {
    int n_configs;              // configurations the rules went through until the scales agreed (info->n_pass_rounds)
    int layout;                 // the one NMS entry layout of all scales (0: none)
    int zx_path;                // path of the last scale
    double q16_bound;           // error bound of the 16-bit tiles in value units (0: the last scale ran none)
    bool copy;                  // the batch makes the voxel copy of the tiled path before its first scale ...
    bool copy_on_side;          // ... on the copy's own stream when the caller gave one (only the first configuration does)
};

// One configuration: `mode` for every scale, or modes[s] when the ladder was laid out; returns the set of layouts as
// bits (1 << layout), or a negative status.
inline int mmx_route_config(const mmx_volume* vol, const mmx_batch_geom& g, const int32_t* radii, const double* w0_tab,
                            const double* w2_tab, const double* norms, int n_sigma, int mode, int zx_flags,
                            const int32_t* modes, double band, bool entries, mmx_route* routes, mmx_ladder_route* out,
                            int thin_radius = -1)
{
    const size_t tab = MMX_MAX_RADIUS_GENERIC + 1;
    const bool is_float = vol->dtype == MMX_F32;
    const bool float_ok = is_float && vol->value_range != 0.f;
    // float32 or 16-bit tiles: one answer for the batch, from the largest bound over its scales
    int tiled_mode = MMX_ZX_TILED;
    double q16_bound = 0.0;
    if (mode == MMX_ZX_AUTO || mode == MMX_ZX_TILED_Q16) {
        double bound = 0.0;
        for (int s = 0; s < n_sigma; ++s) {
            const double b = mmx_q16_error_bound(w0_tab + s * tab, w2_tab + s * tab, radii[s], norms[s]);
            if (b < 0) { bound = -1.0; break; }
            if (b > bound) bound = b;
        }
        double vscale;
        if (mmx_tiles_q16(mode, vol, bound, band, true, &vscale)) { tiled_mode = MMX_ZX_TILED_Q16; q16_bound = bound * vscale; }
    }
    // the voxel copy, when `mode` can take the tiled path and the plan fits (no scale of a laid-out ladder runs it)
    const bool may_tile = ((mode == MMX_ZX_AUTO || mode == MMX_ZX_TILED || mode == MMX_ZX_TILED_Q16) && !is_float) ||
                          ((mode == MMX_ZX_AUTO || mode == MMX_ZX_TILED) && float_ok);
    out->copy = !modes && may_tile && mmx_voxels_ok(vol) && !g.bad_block && g.plan_status == MMX_OK;
    // (the copy is trusted while every scale so far ran the tiled path: any other path uses that part of the workspace
    //  for something else)
    bool trusted = out->copy;
    int layouts = 0;
    for (int s = 0; s < n_sigma; ++s) {
        const int m = modes ? modes[s] : (trusted ? (tiled_mode | MMX_ZX_PREPACKED | zx_flags) : mode);
        const int rc = mmx_route_scale(vol, g, radii[s], w0_tab + s * tab, w2_tab + s * tab, norms[s], m, band, entries, &routes[s],
                                       thin_radius);
        if (rc != MMX_OK) return -rc;
        trusted = trusted && routes[s].path == tiled_mode;
        layouts |= 1 << routes[s].layout;
        out->zx_path = routes[s].path;
    }
    out->q16_bound = !modes && out->zx_path == MMX_ZX_TILED_Q16 ? q16_bound : 0.0;
    return layouts;
}

// The routes of all scales of a batch.  With entries the Y pass leaves whole segments of the cube unwritten, so it is
// all scales in one entry layout or none.  The configurations, in order, the first whose scales agree is taken:
//   1. under MMX_ZX_AUTO, a ladder that holds a radius above MMX_MAX_RADIUS_FAST which the wide passes accept is laid
//      out: radii above MMX_MAX_RADIUS_FAST wide, the others MMX_ZX_PACKED where that kernel takes them and wide where it
//      does not, a scale neither takes MMX_ZX_AUTO (it ends on the separate passes); with row entries if they fit and
//      no scale stayed AUTO; should the scales still disagree, every scale under AUTO without entries.  Such a ladder
//      tries nothing else;
//   2. the requested mode with entries: the voxel copy made once and trusted (MMX_ZX_PREPACKED, with the batch's tile
//      type by name) while every scale so far ran the tiled path;
//   3. MMX_ZX_PACKED with entries, when 2. mixed rows and quads;
//   4. the requested mode without entries.
// MMX_ZX_THIN by name: a batch that is thin at the ladder's largest radius gets that route for EVERY scale, in one
// configuration without entries; any other batch is routed as under MMX_ZX_AUTO.
// routes: [n_sigma].  Returns MMX_OK or the status of the first scale that has none.
inline int mmx_route_ladder(const mmx_volume* vol, const mmx_batch_geom& g, const int32_t* radii, const double* w0_tab,
                            const double* w2_tab, const double* norms, int n_sigma, int zx_mode, int zx_flags, double band,
                            mmx_route* routes, mmx_ladder_route* out)
{
    *out = mmx_ladder_route{};
    int layouts = 0;
    auto config = [&](int mode, const int32_t* modes, bool entries) {
        out->n_configs++;
        layouts = mmx_route_config(vol, g, radii, w0_tab, w2_tab, norms, n_sigma, mode, zx_flags, modes, band, entries, routes, out);
        return layouts < 0 || !(layouts & (layouts - 1));      // (a status, or one layout: done)
    };
    if (zx_mode == MMX_ZX_THIN) {
        int r_max = 0;
        for (int s = 0; s < n_sigma; ++s) if (radii[s] > r_max) r_max = radii[s];
        if (!mmx_thin_accepts(g, r_max)) zx_mode = MMX_ZX_AUTO;
        else {
            out->n_configs = 1;
            layouts = mmx_route_config(vol, g, radii, w0_tab, w2_tab, norms, n_sigma, zx_mode, zx_flags, nullptr, band, false,
                                       routes, out, r_max);
            if (layouts < 0) return -layouts;
            return MMX_OK;              // (layout 0, no copy)
        }
    }
    bool any_wide = false;
    if (zx_mode == MMX_ZX_AUTO && g.status == MMX_OK)
        for (int s = 0; s < n_sigma; ++s)
            if (radii[s] > MMX_MAX_RADIUS_FAST && mmx_wide_accepts(vol, g, radii[s])) any_wide = true;
    if (any_wide) {
        std::vector<int32_t> laid(n_sigma);
        int32_t* modes = laid.data();
        bool entries = g.rows_fit;
        for (int s = 0; s < n_sigma; ++s) {
            const int r = radii[s];
            if (r <= MMX_MAX_RADIUS_FAST && mmx_packed_accepts(vol, g, r)) modes[s] = MMX_ZX_PACKED;
            else if (mmx_wide_accepts(vol, g, r)) modes[s] = MMX_ZX_WIDE;
            else { modes[s] = MMX_ZX_AUTO; entries = false; }
        }
        if (!config(MMX_ZX_AUTO, modes, entries)) {
            for (int s = 0; s < n_sigma; ++s) modes[s] = MMX_ZX_AUTO;
            config(MMX_ZX_AUTO, modes, false);
        }
    } else if (!config(zx_mode, nullptr, true)) {
        if (layouts != ((1 << MMX_MASK_ROWS) | (1 << MMX_MASK_QUADS)) || !config(MMX_ZX_PACKED, nullptr, true))
            config(zx_mode, nullptr, false);
    }
    if (layouts < 0) return -layouts;
    out->layout = 0;
    while (!(layouts & (1 << out->layout))) ++out->layout;
    out->copy_on_side = out->copy && out->n_configs == 1;
    return MMX_OK;
}
