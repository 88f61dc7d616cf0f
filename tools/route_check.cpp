// Stand-alone host check of the kernel-path rules (csrc/mmx_route.h): the table of the rules -- ladders and single calls
// with the full route they must get --, the by-name rows shared with tests/test_gpu_routes.py (tests/golden/
// route_by_name.txt, path in argv[1]), the by-name rows of MMX_ZX_THIN on thin and thick blocks (tests/golden/
// route_thin.txt, when argv[2] names it), the folded operator of that mode (csrc/mmx_fold.h) against a tap-by-tap
// reflection for every extent and radius the kernels fold, and a sweep over geometries, radii, voxel types and modes for two properties: no
// route selects a launcher whose predicate refuses it, and the route of a call agrees with the route of a one-scale
// ladder.  Before that sweep, one over the NMS entry layouts (csrc/mmx_entries.h, host side).  Meant to run under the
// host sanitizers (the command: DESIGN.md, "Wide radii").  No device code, no HIP call: the batch geometry is filled in
// by hand.  Exit status 0 = every row and the sweeps passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../magellanmapper_amd/csrc/mmx_common.h"
#include "../magellanmapper_amd/csrc/mmx_fold.h"

namespace {

constexpr size_t kTab = MMX_MAX_RADIUS_GENERIC + 1;
constexpr double kBandQ16 = 2.5e-4;     // blob_log's band for voxels that may take 16-bit tiles; 2e-5: its narrow one

// half kernels of sigma = radius / 4 (scipy's _gaussian_kernel1d, orders 0 and 2) and the scale normalisation
void gauss(int radius, double* w0, double* w2, double* norm)
{
    const double sigma = radius > 0 ? radius / 4.0 : 0.25, s2 = sigma * sigma;
    double sum = 0.0;
    for (int k = 0; k <= radius; ++k) { w0[k] = exp(-0.5 * k * k / s2); sum += (k ? 2.0 : 1.0) * w0[k]; }
    for (int k = 0; k <= radius; ++k) { w0[k] /= sum; w2[k] = w0[k] * (k * k / (s2 * s2) - 1.0 / s2); }
    *norm = s2;
}

struct geometry { int nz, ny, nx, px; bool rows_fit, quads_fit, plan_ok; };   // one block stands for the batch's extremes
mmx_batch_geom geom(const geometry& r)
{
    mmx_batch_geom g{};
    g.status = MMX_OK;
    g.min_nz = r.nz; g.min_ny = g.max_ny = r.ny; g.min_nx = g.max_nx = r.nx; g.max_px = r.px;
    g.max_lane_in = (int64_t)(r.ny - 1) * r.nx + r.nx - 1;
    g.max_zcols = r.ny * r.px; g.max_ycols = r.nz * r.px; g.max_rows = r.nz * r.ny; g.max_vox = r.nz * r.ny * r.px;
    g.rows_fit = r.rows_fit; g.quads_fit = r.quads_fit;
    g.plan_status = r.plan_ok ? MMX_OK : MMX_ERR_UNSUPPORTED;
    return g;
}
mmx_volume volume(int dtype, float vrange, const geometry& r)
{
    mmx_volume vol{};
    vol.dtype = dtype; vol.value_range = vrange;
    vol.stride_x = 1; vol.stride_y = r.nx; vol.stride_z = (int64_t)r.nx * r.ny;
    return vol;
}

// the full route of a scale, as the table states it
struct want { int family, q16, y, path, trusts, rings, folds = 0; };  // rings: 1 = z, 2 = y, 4 = x on the register-ring kernel;
                                                                      // folds: likewise, on the folded pass
const int SEP = MMX_ROUTE_SEPARATE, WID = MMX_ROUTE_WIDE, TIL = MMX_ROUTE_TILED, PAC = MMX_ROUTE_PACKED;
bool same(const mmx_route& r, const want& w)
{
    return r.family == w.family && r.q16 == (w.q16 != 0) && r.y_kernel == w.y && r.path == w.path &&
           r.trusts_copy == (w.trusts != 0) && (r.ring_z | r.ring_y << 1 | r.ring_x << 2) == w.rings &&
           (r.fold_z | r.fold_y << 1 | r.fold_x << 2) == w.folds;
}
void show(const mmx_route& r)
{
    printf("    got family %d q16 %d copy %d trusts %d y %d rings %d folds %d layout %d path %d\n", r.family, r.q16, r.makes_copy,
           r.trusts_copy, r.y_kernel, r.ring_z | r.ring_y << 1 | r.ring_x << 2, r.fold_z | r.fold_y << 1 | r.fold_x << 2,
           r.layout, r.path);
}

struct row {
    const char* what;
    int dtype; float vrange; geometry geo;
    int mode, flags; double band;
    std::vector<int32_t> radii;
    int status, rounds, layout; bool copy, q16_bound;       // the batch: configurations counted, its layout, copy, bound > 0
    std::vector<want> scales;
};

struct ladder_in {
    std::vector<double> w0, w2, norms;
    ladder_in(const std::vector<int32_t>& radii) : w0(radii.size() * kTab), w2(radii.size() * kTab), norms(radii.size())
    {
        for (size_t s = 0; s < radii.size(); ++s)
            if (radii[s] >= 0 && radii[s] <= MMX_MAX_RADIUS_GENERIC) gauss(radii[s], &w0[s * kTab], &w2[s * kTab], &norms[s]);
    }
};

int check_table()
{
    const int A = MMX_ZX_AUTO, ROWS = MMX_MASK_ROWS, QUADS = MMX_MASK_QUADS;
    const want T16 = {TIL, 1, MMX_Y_YM, MMX_ZX_TILED_Q16, 1, 0}, T16V = {TIL, 1, MMX_Y_Y6, MMX_ZX_TILED_Q16, 1, 0},
               T32 = {TIL, 0, MMX_Y_Y6, MMX_ZX_TILED, 1, 0}, P = {PAC, 0, MMX_Y_Y2, MMX_ZX_PACKED, 0, 0},
               W = {WID, 0, MMX_Y_NONE, MMX_ZX_WIDE, 0, 0}, G = {SEP, 0, MMX_Y_NONE, MMX_ZX_SEPARATE, 0, 0},
               S = {SEP, 0, MMX_Y_NONE, MMX_ZX_SEPARATE, 0, 7};
    const geometry small = {48, 40, 64, 64, true, true, true};
    const std::vector<row> table = {
        // ---- ladders with wide radii: laid out, one configuration
        {"radii 24, 25, 26 on 40 x 48 x 64: packed, wide, wide, row entries", MMX_U16, 0, {40, 48, 64, 64, true, true, false},
         A, 0, kBandQ16, {24, 25, 26}, MMX_OK, 1, ROWS, false, false, {P, W, W}},
        {"rows 530 wide: the radius-24 scale goes wide too", MMX_U16, 0, {40, 48, 530, 544, true, true, false},
         A, 0, kBandQ16, {24, 25, 26}, MMX_OK, 1, ROWS, false, false, {W, W, W}},
        {"row pitch 416, between the packed kernel's limit and the fused path's: wide as well", MMX_U16, 0,
         {40, 48, 400, 416, true, true, true}, A, 0, kBandQ16, {24, 25}, MMX_OK, 1, ROWS, false, false, {W, W}},
        {"a radius above 64 beside wide ones: no entries from the start, that scale on the generic passes", MMX_U16, 0,
         {80, 80, 80, 96, true, true, true}, A, 0, kBandQ16, {31, 64, 65}, MMX_OK, 1, 0, false, false, {W, W, G}},
        {"row entries that do not fit their share of the slot: none", MMX_U8, 0, {70, 70, 70, 96, false, true, true},
         A, 0, kBandQ16, {18, 31}, MMX_OK, 1, 0, false, false, {P, W}},
        {"float voxels, the 0.65 um ladder on 261^3 blocks", MMX_F32, 0, {261, 261, 261, 288, true, true, true},
         A, 0, kBandQ16, {18, 20, 21, 22, 24, 25, 27, 28, 29, 31}, MMX_OK, 1, ROWS, false, false, {P, P, P, P, P, W, W, W, W, W}},
        {"blocks too short for the packed kernel's prefetch but thick enough for the wide passes", MMX_U16, 0,
         {26, 26, 40, 64, true, true, true}, A, 0, kBandQ16, {24, 25}, MMX_OK, 1, ROWS, false, false, {W, W}},
        {"radius 64, the last wide one", MMX_U16, 0, {64, 64, 64, 64, true, true, true}, A, 0, kBandQ16, {64}, MMX_OK, 1, ROWS,
         false, false, {W}},
        // ---- ladders without: the requested mode with entries first
        {"no radius above 24, no plan: packed, rows", MMX_U16, 0, {40, 48, 64, 64, true, true, false}, A, 0, kBandQ16, {20, 24},
         MMX_OK, 1, ROWS, false, false, {P, P}},
        {"a plan that does not fit", MMX_U16, 0, {48, 40, 64, 64, true, true, false}, A, 0, kBandQ16, {4, 8, 12}, MMX_OK, 1, ROWS,
         false, false, {P, P, P}},
        {"a wide radius the blocks do not cover: that scale generic, so no entries -- two configurations", MMX_U16, 0,
         {24, 48, 64, 64, true, true, true}, A, 0, kBandQ16, {20, 25}, MMX_OK, 2, 0, true, false, {T16, G}},
        {"float64 voxels are nobody's", MMX_F64, 0, {80, 80, 80, 96, true, true, true}, A, 0, kBandQ16, {31}, MMX_ERR_UNSUPPORTED,
         1, 0, false, false, {}},
        {"radius 255: the generic passes", MMX_U16, 0, {64, 64, 64, 64, true, true, true}, A, 0, kBandQ16, {255}, MMX_OK, 1, 0,
         true, false, {G}},
        {"a uint16 ladder all on 16-bit tiles: quads, the copy trusted throughout", MMX_U16, 0, small, A, 0, kBandQ16, {4, 8, 12},
         MMX_OK, 1, QUADS, true, true, {T16, T16, T16}},
        {"... with the narrow band: float32 tiles", MMX_U16, 0, small, A, 0, 2e-5, {4, 8, 12}, MMX_OK, 1, QUADS, true, false,
         {T32, T32, T32}},
        {"... with MMX_ZX_Y_VALU in the flags: the Y pass on the VALU", MMX_U16, 0, small, A, MMX_ZX_Y_VALU, kBandQ16, {4, 8, 12},
         MMX_OK, 1, QUADS, true, true, {T16V, T16V, T16V}},
        {"float voxels with no stated range: packed, rows", MMX_F32, 0, small, A, 0, kBandQ16, {4, 8, 12}, MMX_OK, 1, ROWS, false,
         false, {P, P, P}},
        {"float voxels in [0, 1]: 16-bit tiles", MMX_F32, 1.f, small, A, 0, kBandQ16, {4, 8, 12}, MMX_OK, 1, QUADS, true, true,
         {T16, T16, T16}},
        {"float voxels in [-1, 1]: float32 tiles", MMX_F32, -1.f, small, A, 0, kBandQ16, {4, 8, 12}, MMX_OK, 1, QUADS, true, false,
         {T32, T32, T32}},
        {"MMX_ZX_TILED by name", MMX_U16, 0, small, MMX_ZX_TILED, 0, kBandQ16, {4, 8, 12}, MMX_OK, 1, QUADS, true, false,
         {T32, T32, T32}},
        {"MMX_ZX_TILED_Q16 by name, whatever the band", MMX_U16, 0, small, MMX_ZX_TILED_Q16, 0, 2e-5, {4, 8, 12}, MMX_OK, 1, QUADS,
         true, true, {T16, T16, T16}},
        {"MMX_ZX_TILED_Q16 by name on float voxels without a range: packed", MMX_F32, 0, small, MMX_ZX_TILED_Q16, 0, kBandQ16,
         {4, 8}, MMX_OK, 1, ROWS, false, false, {P, P}},
        {"MMX_ZX_PACKED by name", MMX_U16, 0, small, MMX_ZX_PACKED, 0, kBandQ16, {4, 8, 12}, MMX_OK, 1, ROWS, false, false,
         {P, P, P}},
        {"MMX_ZX_SEPARATE by name: the register-ring kernels, no entries", MMX_U16, 0, small, MMX_ZX_SEPARATE, 0, kBandQ16,
         {4, 8, 12}, MMX_OK, 1, 0, false, false, {S, S, S}},
        {"MMX_ZX_WIDE by name at small radii", MMX_U16, 0, small, MMX_ZX_WIDE, 0, kBandQ16, {4, 8, 12}, MMX_OK, 1, ROWS, false,
         false, {W, W, W}},
        {"a retired mode", MMX_U16, 0, small, 4, 0, kBandQ16, {4}, MMX_ERR_ARG, 1, 0, false, false, {}},
        {"row pitch 416 with a plan: tiled", MMX_U16, 0, {40, 48, 400, 416, true, true, true}, A, 0, kBandQ16, {8, 24}, MMX_OK, 1,
         QUADS, true, true, {T16, T16}},
        {"row pitch 416 without: neither fused kernel, the separate passes", MMX_U16, 0, {40, 48, 400, 416, true, true, false},
         A, 0, kBandQ16, {8, 24}, MMX_OK, 1, 0, false, false, {S, S}},
        {"rows 530 wide without a plan: the separate passes", MMX_U16, 0, {40, 48, 530, 544, true, true, false}, A, 0, kBandQ16,
         {8}, MMX_OK, 1, 0, false, false, {S}},
        // ---- rows beyond 512 floats with a plan: the tiled kernels at any pitch, one radius of each geometry class
        {"row pitch 544, uint16: 16-bit tiles, quads", MMX_U16, 0, {40, 48, 530, 544, true, true, true}, A, 0, kBandQ16,
         {8, 16, 24}, MMX_OK, 1, QUADS, true, true, {T16, T16, T16}},
        {"row pitch 1024, uint16", MMX_U16, 0, {40, 48, 1024, 1024, true, true, true}, A, 0, kBandQ16, {8, 16, 24}, MMX_OK, 1,
         QUADS, true, true, {T16, T16, T16}},
        {"row pitch 1056, uint16", MMX_U16, 0, {40, 48, 1025, 1056, true, true, true}, A, 0, kBandQ16, {8, 16, 24}, MMX_OK, 1,
         QUADS, true, true, {T16, T16, T16}},
        {"row pitch 2048, uint16", MMX_U16, 0, {40, 48, 2048, 2048, true, true, true}, A, 0, kBandQ16, {8, 16, 24}, MMX_OK, 1,
         QUADS, true, true, {T16, T16, T16}},
        {"row pitch 544, float voxels in [0, 1]", MMX_F32, 1.f, {40, 48, 530, 544, true, true, true}, A, 0, kBandQ16,
         {8, 16, 24}, MMX_OK, 1, QUADS, true, true, {T16, T16, T16}},
        {"row pitch 1024, float voxels in [0, 1]", MMX_F32, 1.f, {40, 48, 1024, 1024, true, true, true}, A, 0, kBandQ16,
         {8, 16, 24}, MMX_OK, 1, QUADS, true, true, {T16, T16, T16}},
        {"row pitch 1056, float voxels in [0, 1]", MMX_F32, 1.f, {40, 48, 1025, 1056, true, true, true}, A, 0, kBandQ16,
         {8, 16, 24}, MMX_OK, 1, QUADS, true, true, {T16, T16, T16}},
        {"row pitch 2048, float voxels in [0, 1]", MMX_F32, 1.f, {40, 48, 2048, 2048, true, true, true}, A, 0, kBandQ16,
         {8, 16, 24}, MMX_OK, 1, QUADS, true, true, {T16, T16, T16}},
        {"row pitch 544, float voxels with no stated range: the separate passes", MMX_F32, 0, {40, 48, 530, 544, true, true, true},
         A, 0, kBandQ16, {8, 16, 24}, MMX_OK, 1, 0, false, false, {S, S, S}},
        {"row pitch 1024, float voxels with no stated range", MMX_F32, 0, {40, 48, 1024, 1024, true, true, true}, A, 0, kBandQ16,
         {8, 16, 24}, MMX_OK, 1, 0, false, false, {S, S, S}},
        {"row pitch 1056, float voxels with no stated range", MMX_F32, 0, {40, 48, 1025, 1056, true, true, true}, A, 0, kBandQ16,
         {8, 16, 24}, MMX_OK, 1, 0, false, false, {S, S, S}},
        {"row pitch 2048, float voxels with no stated range", MMX_F32, 0, {40, 48, 2048, 2048, true, true, true}, A, 0, kBandQ16,
         {8, 16, 24}, MMX_OK, 1, 0, false, false, {S, S, S}},
        {"rows 530 wide with a plan, radii 24, 25, 26: laid out as before -- wide, never tiled", MMX_U16, 0,
         {40, 48, 530, 544, true, true, true}, A, 0, kBandQ16, {24, 25, 26}, MMX_OK, 1, ROWS, false, false, {W, W, W}},
        {"rows 2100 wide: the X pass generic", MMX_U16, 0, {40, 48, 2100, 2112, true, true, false}, A, 0, kBandQ16, {8}, MMX_OK, 1,
         0, false, false, {{SEP, 0, MMX_Y_NONE, MMX_ZX_SEPARATE, 0, 3}}},
        // (tests/test_gpu_routes.py, test A) radius 18 needs ny >= 22 for the fused path: quads and none -> no entries
        {"the mixed ladder: 16-bit tiles, then the separate passes with a generic Y pass; two configurations", MMX_U16, 0,
         {40, 20, 40, 64, true, true, true}, A, 0, kBandQ16, {6, 18}, MMX_OK, 2, 0, true, false,
         {T16, {SEP, 0, MMX_Y_NONE, MMX_ZX_SEPARATE, 0, 5}}},
        // ---- MMX_ZX_THIN by name: thin at the ladder's largest radius -> every scale the separate passes, folded where
        // no ring kernel takes the pass, one configuration, no entries, no copy
        {"thin by name, a shallow stack of 20 planes: Z folded from radius 17 on", MMX_U16, 0, {20, 261, 261, 288, true, true, true},
         MMX_ZX_THIN, 0, kBandQ16, {8, 12, 20}, MMX_OK, 1, 0, false, false,
         {{SEP, 0, MMX_Y_NONE, MMX_ZX_THIN, 0, 7, 0}, {SEP, 0, MMX_Y_NONE, MMX_ZX_THIN, 0, 7, 0}, {SEP, 0, MMX_Y_NONE, MMX_ZX_THIN, 0, 6, 1}}},
        {"thin by name, a 2-D image", MMX_U8, 0, {1, 562, 562, 576, true, true, true}, MMX_ZX_THIN, 0, kBandQ16, {8, 24}, MMX_OK,
         1, 0, false, false, {{SEP, 0, MMX_Y_NONE, MMX_ZX_THIN, 0, 6, 1}, {SEP, 0, MMX_Y_NONE, MMX_ZX_THIN, 0, 6, 1}}},
        {"thin by name, a remainder 10 wide (x folded; it is shorter than the radius 12 the X ring kernel needs)", MMX_U16, 0,
         {261, 261, 10, 32, true, true, true}, MMX_ZX_THIN, 0, kBandQ16, {8, 12}, MMX_OK, 1, 0, false, false,
         {{SEP, 0, MMX_Y_NONE, MMX_ZX_THIN, 0, 7, 0}, {SEP, 0, MMX_Y_NONE, MMX_ZX_THIN, 0, 3, 4}}},
        {"thin by name with wide radii: every pass folded above radius 24", MMX_F32, 0, {30, 40, 44, 64, true, true, true},
         MMX_ZX_THIN, 0, kBandQ16, {31}, MMX_OK, 1, 0, false, false, {{SEP, 0, MMX_Y_NONE, MMX_ZX_THIN, 0, 0, 7}}},
        {"thin by name on thick blocks: as MMX_ZX_AUTO", MMX_U16, 0, small, MMX_ZX_THIN, 0, kBandQ16, {4, 8, 12}, MMX_OK, 1,
         QUADS, true, true, {T16, T16, T16}},
        {"... and with wide radii the laid-out ladder of MMX_ZX_AUTO", MMX_U16, 0, {40, 48, 64, 64, true, true, false},
         MMX_ZX_THIN, 0, kBandQ16, {24, 25, 26}, MMX_OK, 1, ROWS, false, false, {P, W, W}},
    };
    int bad = 0;
    for (size_t i = 0; i < table.size(); ++i) {
        const row& r = table[i];
        const mmx_volume vol = volume(r.dtype, r.vrange, r.geo);
        const mmx_batch_geom g = geom(r.geo);
        const ladder_in in(r.radii);
        std::vector<mmx_route> routes(r.radii.size());
        mmx_ladder_route lad;
        const int rc = mmx_route_ladder(&vol, g, r.radii.data(), in.w0.data(), in.w2.data(), in.norms.data(), (int)r.radii.size(),
                                        r.mode, r.flags, r.band, routes.data(), &lad);
        bool ok = rc == r.status;
        if (ok && rc == MMX_OK) {
            ok = lad.n_configs == r.rounds && lad.layout == r.layout && lad.copy == r.copy && (lad.q16_bound > 0.0) == r.q16_bound &&
                 lad.zx_path == r.scales.back().path && lad.copy_on_side == (lad.copy && r.rounds == 1);
            for (size_t s = 0; s < routes.size(); ++s) {
                // the copy: made by the batch and trusted, never by a scale of these ladders
                ok = ok && same(routes[s], r.scales[s]) && routes[s].layout == r.layout && !routes[s].makes_copy;
            }
        }
        printf("row %2zu: %s  (%s)\n", i, ok ? "ok" : "MISMATCH", r.what);
        if (!ok) {
            printf("    status %d rounds %d layout %d copy %d bound %g\n", rc, lad.n_configs, lad.layout, lad.copy, lad.q16_bound);
            for (const auto& x : routes) show(x);
        }
        bad += !ok;
    }
    printf("%d of %zu rows mismatched\n", bad, table.size());
    return bad;
}

// ---- single calls by name: the rows tests/test_gpu_routes.py runs through mmx_log_batch_f32 on a 48 x 40 x 64 block at
// radius 8.  A line: dtype value_range mode y_valu prepacked entries band | family q16 copy y rings layout path
int check_by_name(const char* path)
{
    FILE* f = fopen(path, "r");
    if (!f) { printf("cannot open %s\n", path); return 1; }
    const geometry geo = {48, 40, 64, 64, true, true, true};
    const mmx_batch_geom g = geom(geo);
    double w0[kTab], w2[kTab], norm;
    gauss(8, w0, w2, &norm);
    char line[256];
    int bad = 0, n = 0;
    while (fgets(line, sizeof line, f)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        int dtype, mode, yv, pp, entries, family, q16, copy, y, rings, layout, zx;
        float vrange; double band;
        if (sscanf(line, "%d %f %d %d %d %d %lf | %d %d %d %d %d %d %d", &dtype, &vrange, &mode, &yv, &pp, &entries, &band, &family,
                   &q16, &copy, &y, &rings, &layout, &zx) != 14) { printf("bad line: %s", line); ++bad; continue; }
        const mmx_volume vol = volume(dtype, vrange, geo);
        const int zx_mode = mode | (yv ? MMX_ZX_Y_VALU : 0) | (pp ? MMX_ZX_PREPACKED : 0);
        mmx_route r;
        const int rc = mmx_route_scale(&vol, g, 8, w0, w2, norm, zx_mode, band, entries != 0, &r);
        const want w = {family, q16, y, zx, pp && family == TIL, rings};
        const bool ok = rc == MMX_OK && same(r, w) && r.layout == layout && r.makes_copy == (copy != 0);
        if (!ok) { printf("by name, MISMATCH (status %d): %s", rc, line); show(r); }
        bad += !ok; ++n;
    }
    fclose(f);
    printf("%d of %d by-name rows mismatched\n", bad, n);
    return bad + (n == 0);
}

// ---- single calls of MMX_ZX_THIN by name, on thin and on thick blocks: the rows tests/test_gpu_thin.py runs through
// mmx_log_batch_f32.  A line: nz ny nx dtype radius entries | family rings folds layout path  (value_range 0, the wide
// band, the plan and both entry layouts fit)
int check_thin_table(const char* path)
{
    FILE* f = fopen(path, "r");
    if (!f) { printf("cannot open %s\n", path); return 1; }
    char line[256];
    int bad = 0, n = 0;
    while (fgets(line, sizeof line, f)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        int nz, ny, nx, dtype, radius, entries, family, rings, folds, layout, zx;
        if (sscanf(line, "%d %d %d %d %d %d | %d %d %d %d %d", &nz, &ny, &nx, &dtype, &radius, &entries, &family, &rings, &folds,
                   &layout, &zx) != 11 || radius < 0 || radius > MMX_MAX_RADIUS_GENERIC) {
            printf("bad line: %s", line); ++bad; continue;
        }
        const geometry geo = {nz, ny, nx, (nx + MMX_ROW_ALIGN - 1) / MMX_ROW_ALIGN * MMX_ROW_ALIGN, true, true, true};
        const mmx_batch_geom g = geom(geo);
        const mmx_volume vol = volume(dtype, 0.f, geo);
        double w0[kTab], w2[kTab], norm;
        gauss(radius, w0, w2, &norm);
        mmx_route r;
        const int rc = mmx_route_scale(&vol, g, radius, w0, w2, norm, MMX_ZX_THIN, kBandQ16, entries != 0, &r);
        const bool ok = rc == MMX_OK && r.family == family && (r.ring_z | r.ring_y << 1 | r.ring_x << 2) == rings &&
                        (r.fold_z | r.fold_y << 1 | r.fold_x << 2) == folds && r.layout == layout && r.path == zx;
        if (!ok) { printf("thin by name, MISMATCH (status %d): %s", rc, line); show(r); }
        bad += !ok; ++n;
    }
    fclose(f);
    printf("%d of %d thin by-name rows mismatched\n", bad, n);
    return bad + (n == 0);
}

// ---- the folded operator (csrc/mmx_fold.h) for every extent the kernels fold and radius 1 .. 64: each row against the
// taps reflected one by one (mmx_reflect, summed in double) to one float32 ulp of the matrix's largest entry, its sum
// against the sum of the taps, and the matrix against its transpose (the operator is symmetric; the two entries are
// summed in opposite orders)
int sweep_fold()
{
    long entries = 0, bad = 0;
    std::vector<float> m((size_t)MMX_FOLD_MAX_N * MMX_FOLD_MAX_N);
    std::vector<double> ref((size_t)MMX_FOLD_MAX_N * MMX_FOLD_MAX_N);
    for (int radius = 1; radius <= MMX_MAX_RADIUS_WIDE; ++radius) {
        double w0[kTab], w2[kTab], norm;
        gauss(radius, w0, w2, &norm);
        for (const double* wd : {w0, w2}) {
            float w[kTab];
            double sum = 0.0;
            for (int k = 0; k <= radius; ++k) { w[k] = (float)wd[k]; sum += (k ? 2.0 : 1.0) * (double)w[k]; }
            for (int n = 1; n <= MMX_FOLD_MAX_N; ++n) {
                mmx_fold_matrix_host(w, radius, n, m.data());
                double top = 0.0;
                for (int i = 0; i < n; ++i) {
                    for (int j = 0; j < n; ++j) ref[(size_t)i * n + j] = 0.0;
                    for (int k = -radius; k <= radius; ++k) ref[(size_t)i * n + mmx_reflect(i + k, n)] += (double)w[k < 0 ? -k : k];
                    for (int j = 0; j < n; ++j) top = fmax(top, fabs(ref[(size_t)i * n + j]));
                }
                const double ulp = (double)nextafterf((float)top, INFINITY) - (double)(float)top;
                for (int i = 0; i < n; ++i) {
                    double row = 0.0;
                    for (int j = 0; j < n; ++j, ++entries) {
                        row += (double)m[(size_t)i * n + j];
                        if (fabs((double)m[(size_t)i * n + j] - ref[(size_t)i * n + j]) > ulp) ++bad;
                        if (fabs((double)m[(size_t)i * n + j] - (double)m[(size_t)j * n + i]) > ulp) ++bad;
                    }
                    if (fabs(row - sum) > 1e-6 * fmax(1.0, fabs(sum)) + n * ulp) ++bad;
                }
            }
        }
    }
    printf("fold: %ld matrix entries, %ld failures\n", entries, bad);
    return bad != 0;
}

// ---- the sweep
int sweep()
{
    static double W0[kTab][kTab], W2[kTab][kTab], NORM[kTab];
    for (int r = 0; r <= MMX_MAX_RADIUS_GENERIC; ++r) gauss(r, W0[r], W2[r], &NORM[r]);
    // extents 1 .. 80 on a coarse grid -- every radius below meets each limit (r, r + 1, r + MMX_COL_PREFETCH) on them --
    // and the rows around the pitch limit of the packed kernel (320), the panel of the tiled path's voxel copy (512: no limit
    // of any route) and the X pass's limit (2048)
    const int ext[] = {1, 12, 29, 80};
    const int wide[] = {1, 24, 28, 64, 320, 321, 512, 513, 2048, 2049};
    const int modes[] = {MMX_ZX_AUTO, MMX_ZX_SEPARATE, MMX_ZX_PACKED, MMX_ZX_TILED, MMX_ZX_TILED_Q16, MMX_ZX_WIDE,
                         MMX_ZX_TILED | MMX_ZX_PREPACKED, MMX_ZX_TILED_Q16 | MMX_ZX_PREPACKED, MMX_ZX_THIN, -2, 1, 3, 4, 5, 10};
    const int flags[] = {0, MMX_ZX_Y_VALU};
    struct vox { int dtype; float vrange; };
    const vox voxels[] = {{MMX_U8, 0}, {MMX_U16, 0}, {MMX_F32, 0}, {MMX_F32, 1.f}};         // (every other ranged one: [-3, 3])
    long n = 0, refused = 0, disagree = 0, rerouted = 0, ladders = 0;
    int variant = 0;
    for (int nz : ext) for (int ny : ext) for (int nx : wide) {
        ++variant;
        const geometry geo = {nz, ny, nx, (nx + MMX_ROW_ALIGN - 1) / MMX_ROW_ALIGN * MMX_ROW_ALIGN, variant % 5 != 0,
                              variant % 7 != 0, variant % 3 != 0};
        const mmx_batch_geom g = geom(geo);
        for (const vox& v : voxels) {
            mmx_volume vol = volume(v.dtype, v.vrange > 0.f && variant % 2 ? -3.f : v.vrange, geo);
            if (variant % 11 == 0) vol.stride_z = int64_t(1) << 27;       // (beyond zx2_kernel's scalar plane offsets)
            for (int radius = -1; radius <= MMX_MAX_RADIUS_GENERIC + 1; ++radius) {
                const bool valid = radius >= 0 && radius <= MMX_MAX_RADIUS_GENERIC;
                const double* w0 = W0[valid ? radius : 0]; const double* w2 = W2[valid ? radius : 0];
                const double norm = NORM[valid ? radius : 0];
                // the predicates against one another
                if (mmx_packed_accepts(&vol, g, radius) && !mmx_fused_accepts(&vol, g, radius)) ++refused;
                if (mmx_tiled_accepts(&vol, g, radius) && !mmx_fused_accepts(&vol, g, radius)) ++refused;
                if (mmx_fused_accepts(&vol, g, radius) && (!mmx_ring_radius(radius) || !mmx_wide_accepts(&vol, g, radius))) ++refused;
                // thin is what sends a column pass off its ring kernel; the fused path is not for thin batches
                if (mmx_thin_accepts(g, radius) && mmx_fused_accepts(&vol, g, radius) && g.min_nz >= radius + MMX_COL_PREFETCH &&
                    g.min_nx >= radius + MMX_COL_PREFETCH) ++refused;
                if (valid && mmx_ring_radius(radius) && !mmx_thin_accepts(g, radius) && !mmx_ypass_accepts(g, radius)) ++refused;
                // radii -1 .. 30 and the edges of the wide and generic ranges meet every mode, the others one mode each
                const bool every = radius <= 30 || (radius >= 63 && radius <= 66) || radius >= MMX_MAX_RADIUS_GENERIC - 1;
                const int n_modes = (int)(sizeof modes / sizeof *modes);
                for (int mi = 0; mi < n_modes; ++mi) for (int fl : flags) for (int entries = fl ? 1 : 0; entries < 2; ++entries) {
                    if (!every && mi != (variant + radius) % n_modes) continue;
                    const int mode = modes[mi];
                    const double band = (variant + radius) % 2 ? kBandQ16 : 2e-5;
                    mmx_route r;
                    const int zx_mode = mode >= 0 ? (mode | fl) : mode;
                    const int rc = mmx_route_scale(&vol, g, radius, w0, w2, norm, zx_mode, band, entries != 0, &r);
                    ++n;
                    if (rc != MMX_OK) {
                        mmx_zx_request q;
                        if (valid && mmx_zx_parse(zx_mode, &q) == MMX_OK) ++refused;      // (nothing else ends a call here)
                        continue;
                    }
                    // predicate consistency: every launcher the route names takes the call
                    bool ok = true;
                    if (r.family == WID) ok = mmx_wide_launch_accepts(&vol, radius) && mmx_wide_accepts(&vol, g, radius);
                    else if (r.family == TIL) {
                        ok = mmx_zx6_launch_accepts(&vol, g.min_nz, g.min_nx, radius) && g.plan_status == MMX_OK &&
                             r.makes_copy != r.trusts_copy;       // (at any row pitch: the plan is what bounds a block)
                        float y0[MMX_MAX_RADIUS_FAST + 1], y2[MMX_MAX_RADIUS_FAST + 1];
                        for (int k = 0; k <= radius; ++k) { y0[k] = (float)(-norm * w0[k]); y2[k] = (float)(-norm * w2[k]); }
                        if (r.y_kernel == MMX_Y_YM)
                            ok = ok && r.q16 && mmx_ym_accepts(y0, y2, radius, (float)(r.bp / 65535.0), (float)(r.bq / 32767.0));
                        else ok = ok && r.y_kernel == MMX_Y_Y6 && mmx_ring_radius(radius);
                        ok = ok && (!r.q16 || (r.bp > 0.0 && r.bq > 0.0));
                    } else if (r.family == PAC)
                        ok = mmx_zx2_launch_accepts(&vol, g.max_px, radius) && r.y_kernel == MMX_Y_Y2 && mmx_ring_radius(radius);
                    else
                        ok = (!r.ring_z || (mmx_ring_radius(radius) && mmx_voxels_ok(&vol) && mmx_zpass_accepts(&vol, g, radius))) &&
                             (!r.ring_y || mmx_ypass_accepts(g, radius)) &&
                             (!r.ring_x || mmx_xpass_launch_accepts(g.max_nx, radius)) && r.layout == 0 &&
                             // the folded passes: by name on a thin batch only, and then every pass no ring kernel takes
                             (r.path == MMX_ZX_THIN ? mode == MMX_ZX_THIN && mmx_thin_accepts(g, radius) &&
                                                      r.fold_z == !r.ring_z && r.fold_y == !r.ring_y && r.fold_x == !r.ring_x
                                                    : !(r.fold_z || r.fold_y || r.fold_x));
                    if (r.family != SEP && (r.fold_z || r.fold_y || r.fold_x || r.path == MMX_ZX_THIN)) ok = false;
                    ok = ok && (r.layout == 0 || entries) && (r.layout != MMX_MASK_ROWS || g.rows_fit) &&
                         (r.layout != MMX_MASK_QUADS || g.quads_fit);
                    if (!ok) { if (++refused < 10) { printf("refused: %d x %d x %d r %d mode %d\n", nz, ny, nx, radius, zx_mode); show(r); } }
                    // route agreement: the same call as a one-scale ladder (which wants entries, and applies its flags
                    // only to the copy it trusts)
                    if (!entries || fl) continue;
                    mmx_route lr;
                    mmx_ladder_route lad;
                    const int32_t rad = radius;
                    const int lrc = mmx_route_ladder(&vol, g, &rad, w0, w2, &norm, 1, zx_mode, 0, band, &lr, &lad);
                    ++ladders;
                    const bool agree = lrc == MMX_OK && lad.n_configs == 1 && lr.family == r.family && lr.q16 == r.q16 &&
                                       lr.y_kernel == r.y_kernel && lr.layout == r.layout && lr.path == r.path &&
                                       lr.ring_z == r.ring_z && lr.ring_y == r.ring_y && lr.ring_x == r.ring_x &&
                                       lr.fold_z == r.fold_z && lr.fold_y == r.fold_y && lr.fold_x == r.fold_x &&
                                       lad.layout == r.layout && lad.zx_path == r.path &&
                                       // (the copy: the batch's, trusted, where the ladder makes one; else as the call has it)
                                       lr.trusts_copy == (lr.family == TIL && (lad.copy || r.trusts_copy)) &&
                                       lr.makes_copy == (lr.family == TIL && !lr.trusts_copy);
                    if (!agree && ++disagree < 10) { printf("disagree: %d x %d x %d r %d mode %d\n", nz, ny, nx, radius, zx_mode); show(r); show(lr); }
                }
            }
            // ladders of three radii around every limit: how often is the MMX_ZX_PACKED re-route (rows and quads mixed) taken?
            const int32_t trios[][3] = {{4, 8, 12}, {8, 24, 25}, {20, 24, 28}, {6, 18, 30}, {24, 64, 65}, {1, 2, 3}};
            for (const auto& t : trios) for (int mode : {MMX_ZX_AUTO, MMX_ZX_TILED, MMX_ZX_TILED_Q16, MMX_ZX_PACKED, MMX_ZX_WIDE, MMX_ZX_THIN}) {
                const ladder_in in(std::vector<int32_t>(t, t + 3));
                mmx_route lr[3];
                mmx_ladder_route lad;
                for (double band : {kBandQ16, 2e-5}) {
                    if (mmx_route_ladder(&vol, g, t, in.w0.data(), in.w2.data(), in.norms.data(), 3, mode, 0, band, lr, &lad) != MMX_OK)
                        continue;
                    ++ladders;
                    if (lad.n_configs == 3 || (lad.n_configs == 2 && lad.layout != 0)) ++rerouted;
                    if (lad.n_configs < 1 || lad.n_configs > 3) ++disagree;
                    for (const auto& x : lr) if (x.layout != lad.layout) ++disagree;      // one layout, or none
                }
            }
        }
    }
    printf("sweep: %ld routes, %ld ladders; %ld refused by a predicate, %ld disagreements; the MMX_ZX_PACKED re-route was "
           "selected %ld times\n", n, ladders, refused, disagree, rerouted);
    return refused || disagree;
}

// ---- the NMS entry layouts (csrc/mmx_entries.h, host side): on ragged blocks -- planes no multiple of 4, columns no
// multiple of 16 or 64, a row pitch above nx, one block 530 wide -- every voxel has an (entry, bit) below the per-row
// count, no two voxels share one, both are what the prose of include/mmx.h says, the inverse returns the voxel, and
// "fits" equals the two expressions mmx_batch_geom_make computed inline before the header existed (stated below).
int sweep_entries()
{
    long voxels = 0, bad = 0;
    for (int nz : {1, 3, 4, 5, 17, 30}) for (int nx : {1, 15, 16, 17, 63, 64, 65, 100, 261, 530}) for (int pad : {0, 1}) {
        const int px = (nx + MMX_ROW_ALIGN - 1) / MMX_ROW_ALIGN * MMX_ROW_ALIGN + pad * MMX_ROW_ALIGN;
        for (int layout : {MMX_MASK_ROWS, MMX_MASK_QUADS}) {
            const mmx_entry_geom g = mmx_entry_geom_make(layout, nz, nx, px);
            if (g.per_row != mmx_entries_per_row<int>(layout, nz, nx, px) || g.per_row < 1) ++bad;
            // (mmx.h: ceil(nz * px / 64) entries per row y, or ceil(nz / 4) * ceil(nx / 16))
            if (g.per_row != (layout == MMX_MASK_ROWS ? (nz * px + 63) / 64 : ((nz + 3) / 4) * ((nx + 15) / 16))) ++bad;
            if (mmx_entry_base(3, 1000) != (3 * 1000) >> 5) ++bad;          // (the block in slot b starts at entry (b * slot_elems) >> 5)
            std::vector<char> seen((size_t)g.per_row * 64, 0);
            for (int z = 0; z < nz; ++z) for (int x = 0; x < nx; ++x, ++voxels) {
                const int e = mmx_entry_index(g, z, x), b = mmx_entry_bit(g, z, x);
                // the layouts as include/mmx.h states them (d_nms_mask), written out here independently of the header
                const int c = z * px + x;
                const int want_e = layout == MMX_MASK_ROWS ? c >> 6 : (z >> 2) * ((nx + 15) / 16) + (x >> 4);
                const int want_b = layout == MMX_MASK_ROWS ? c & 63 : ((z & 3) << 4) | (x & 15);
                if (e != want_e || b != want_b) ++bad;
                if (e < 0 || e >= g.per_row || b < 0 || b > 63) { ++bad; continue; }
                if (seen[(size_t)e * 64 + b]++) ++bad;
                int zi = -1, xi = -1;
                mmx_entry_voxel(g, e, b, &zi, &xi);
                if (zi != z || xi != x) ++bad;
            }
            // slots from far too small to ample, every multiple of 32 around the limit included
            for (int ny : {1, 7, 40}) {
                const int64_t need = ((int64_t)ny * g.per_row + 1) * 32;
                for (int64_t slot_elems : {int64_t(0), int64_t(31), need - 33, need - 32, need - 1, need, need + 31, need + 32,
                                           (int64_t)nz * ny * px, int64_t(1) << 40}) {
                    if (slot_elems < 0) continue;
                    const bool old_fit = layout == MMX_MASK_ROWS
                        ? !((int64_t)ny * (((int64_t)nz * px + 63) >> 6) > (slot_elems >> 5) - 1)
                        : !((int64_t)ny * ((nz + 3) >> 2) * ((nx + 15) >> 4) > (slot_elems >> 5) - 1);
                    if (mmx_entries_fit(layout, nz, ny, nx, px, slot_elems) != old_fit) ++bad;
                }
            }
        }
    }
    printf("entries: %ld voxels in two layouts, %ld failures\n", voxels, bad);
    return bad != 0;
}

}  // namespace

int main(int argc, char** argv)
{
    int bad = check_table();
    bad += check_by_name(argc > 1 ? argv[1] : "tests/golden/route_by_name.txt");
    if (argc > 2) bad += check_thin_table(argv[2]);
    bad += sweep_fold();
    bad += sweep_entries();
    bad += sweep();
    return bad ? 1 : 0;
}
