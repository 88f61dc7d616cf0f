// Stand-alone host check of the kernel-path predicates and the ladder layout (csrc/mmx_route.h) over a table of
// geometries, meant to run under the host sanitizers (the command: DESIGN.md, "Wide radii").  No device code, no HIP
// call: the batch geometry is filled in by hand.  Exit status 0 = every row matched.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../magellanmapper_amd/csrc/mmx_common.h"

namespace {

struct row {
    int dtype, nz, ny, nx, px;          // one block stands for the batch's extremes (min = max)
    bool rows_fit;
    std::vector<int32_t> radii;
    bool laid_out;                      // mmx_ladder_layout's return
    bool entries;
    std::vector<int32_t> modes;         // expected, when laid out
};

mmx_batch_geom geom(const row& r)
{
    mmx_batch_geom g{};
    g.status = MMX_OK;
    g.min_nz = r.nz; g.min_ny = g.max_ny = r.ny; g.min_nx = g.max_nx = r.nx; g.max_px = r.px;
    g.max_lane_in = (int64_t)(r.ny - 1) * r.px + r.nx - 1;
    g.rows_fit = r.rows_fit; g.quads_fit = true;
    g.plan_status = MMX_ERR_UNSUPPORTED;
    return g;
}

}  // namespace

int main()
{
    const int A = MMX_ZX_AUTO, P = MMX_ZX_PACKED, W = MMX_ZX_WIDE;
    const std::vector<row> table = {
        // the issue's ladder: radii 24, 25, 26 on 40 x 48 x 64 -- packed, wide, wide, entries
        {MMX_U16, 40, 48, 64, 64, true, {24, 25, 26}, true, true, {P, W, W}},
        // rows 530 wide: the radius-24 scale goes wide too
        {MMX_U16, 40, 48, 530, 544, true, {24, 25, 26}, true, true, {W, W, W}},
        // rows between the packed kernel's limit and the fused path's: wide as well
        {MMX_U16, 40, 48, 400, 416, true, {24, 25}, true, true, {W, W}},
        // no radius above 24: not laid out
        {MMX_U16, 40, 48, 64, 64, true, {20, 24}, false, false, {}},
        // a wide radius the blocks do not cover: not laid out (the generic passes, as before)
        {MMX_U16, 24, 48, 64, 64, true, {20, 25}, false, false, {}},
        // one radius above 64 beside a wide one: one round without entries, that scale left to AUTO
        {MMX_U16, 80, 80, 80, 96, true, {31, 64, 65}, true, false, {W, W, A}},
        // entries that do not fit their share of the slot: no entries
        {MMX_U8, 70, 70, 70, 96, false, {18, 31}, true, false, {P, W}},
        // float voxels, the 0.65 um ladder on 261^3 blocks
        {MMX_F32, 261, 261, 261, 288, true, {18, 20, 21, 22, 24, 25, 27, 28, 29, 31}, true, true,
         {P, P, P, P, P, W, W, W, W, W}},
        // a small radius on blocks too short for the packed kernel's prefetch but thick enough for the wide passes
        {MMX_U16, 26, 26, 40, 64, true, {24, 25}, true, true, {W, W}},
        // float64 voxels are nobody's
        {MMX_F64, 80, 80, 80, 96, true, {31}, false, false, {}},
        // the edges of the radius range
        {MMX_U16, 64, 64, 64, 64, true, {64}, true, true, {W}},
        {MMX_U16, 64, 64, 64, 64, true, {255}, false, false, {}},
    };
    int bad = 0;
    for (size_t i = 0; i < table.size(); ++i) {
        const row& r = table[i];
        mmx_volume vol{};
        vol.dtype = r.dtype;
        vol.stride_x = 1; vol.stride_y = r.nx; vol.stride_z = (int64_t)r.nx * r.ny;
        const mmx_batch_geom g = geom(r);
        std::vector<int32_t> modes(r.radii.size(), -99);
        bool entries = false;
        const bool laid = mmx_ladder_layout(&vol, g, r.radii.data(), (int)r.radii.size(), modes.data(), &entries);
        bool ok = laid == r.laid_out;
        if (ok && laid) ok = entries == r.entries && modes == r.modes;
        if (ok && !laid)
            for (int32_t m : modes) ok = ok && m == -99;            // nothing written
        // the predicates on their own, at every radius of the ABI
        for (int radius = -1; radius <= MMX_MAX_RADIUS_GENERIC + 1; ++radius) {
            const bool w = mmx_wide_accepts(&vol, g, radius);
            const bool want_w = radius >= 1 && radius <= MMX_MAX_RADIUS_WIDE && r.dtype != MMX_F64 && r.nz >= radius &&
                                r.ny >= radius && r.nx >= radius;
            if (w != want_w) ok = false;
            if (mmx_packed_accepts(&vol, g, radius) && !mmx_fused_accepts(&vol, g, radius)) ok = false;
            if (mmx_fused_accepts(&vol, g, radius) && (radius < 1 || radius > MMX_MAX_RADIUS_FAST)) ok = false;
        }
        printf("row %2zu: %s\n", i, ok ? "ok" : "MISMATCH");
        bad += !ok;
    }
    printf("%d of %zu rows mismatched\n", bad, table.size());
    return bad ? 1 : 0;
}
