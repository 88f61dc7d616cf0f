// extern "C" entry points of libmmx_hip.so (see include/mmx.h for the contract).

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mmx_common.h"

int mmx_launch_generic_pass(int pass, const mmx_volume* vol, const mmx_block* d_blocks, int n_blocks,
                            int max_vox, int64_t slot_elems, const float* w0, const float* w2, int radius,
                            const float* in1, const float* in2, float* out1, float* out2, hipStream_t s);
int mmx_launch_fold_pass(int pass, const mmx_volume* vol, const mmx_block* d_blocks, int n_blocks,
                         int max_vox, int64_t slot_elems, const float* w0, const float* w2, int radius,
                         const float* in1, const float* in2, float* out1, float* out2, hipStream_t s);
int mmx_launch_peaks(const float* d_log, int n_sigma, int64_t sigma_stride, const mmx_block* d_blocks,
                     int n_blocks, int max_vox, int64_t slot_elems, float thr, float eps,
                     mmx_cand* d_cands, uint32_t cap, uint32_t* d_count, hipStream_t stream);
int mmx_launch_peaks_sparse(const float* d_log, const unsigned long long* d_mask, int n_sigma,
                            int64_t sigma_stride, const mmx_block* d_blocks, int n_blocks, int max_vox,
                            int64_t slot_elems, float thr, float eps, mmx_cand* d_cands, uint32_t cap,
                            uint32_t* d_count, int quads, hipStream_t stream);

#include <mutex>
#include <vector>

namespace {
thread_local char g_hip_err[256] = "";

struct span { hipEvent_t a, b; int kind; };
std::mutex g_tm;
bool g_timing = false;
uint32_t g_kinds = ~0u;              // kernel families that record events while g_timing is on
std::vector<span> g_spans;          // recorded spans of the current window
std::vector<hipEvent_t> g_pool;     // recycled events
hipEvent_t g_open[MMX_K_SLOTS];

hipEvent_t take_event()
{
    if (!g_pool.empty()) { hipEvent_t e = g_pool.back(); g_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    hipEventCreate(&e);
    return e;
}

int hip_fail(hipError_t e, const char* what)
{
    snprintf(g_hip_err, sizeof g_hip_err, "%s: %s", what, hipGetErrorString(e));
    return MMX_ERR_HIP;
}
}  // namespace

void mmx_time_begin(int kind, hipStream_t s)
{
    std::lock_guard<std::mutex> lk(g_tm);
    if (!g_timing || !((g_kinds >> kind) & 1u)) return;
    g_open[kind] = take_event();
    hipEventRecord(g_open[kind], s);
}

void mmx_time_end(int kind, hipStream_t s)
{
    std::lock_guard<std::mutex> lk(g_tm);
    if (!g_timing || !g_open[kind]) return;
    hipEvent_t b = take_event();
    hipEventRecord(b, s);
    g_spans.push_back({g_open[kind], b, kind});
    g_open[kind] = nullptr;
}

extern "C" {

int mmx_timing_enable(int on)
{
    std::lock_guard<std::mutex> lk(g_tm);
    for (auto& sp : g_spans) { g_pool.push_back(sp.a); g_pool.push_back(sp.b); }
    g_spans.clear();
    for (int k = 0; k < MMX_K_SLOTS; ++k) g_open[k] = nullptr;
    g_timing = on != 0;
    // 1: every family; any other non-zero value: bit (k + 1) selects family MMX_K_k
    g_kinds = on == 1 ? ~0u : ((uint32_t)on >> 1);
    return MMX_OK;
}

int mmx_timing_is_enabled(void)
{
    std::lock_guard<std::mutex> lk(g_tm);
    return g_timing ? 1 : 0;
}

int mmx_timing_read(double* ms, int64_t* launches, int n)
{
    if (!ms || !launches || n < MMX_K_COUNT) return MMX_ERR_ARG;
    std::lock_guard<std::mutex> lk(g_tm);
    for (int k = 0; k < n; ++k) { ms[k] = 0.0; launches[k] = 0; }
    for (auto& sp : g_spans) {
        if (sp.kind >= n) {             // (a family behind the ones this caller knows)
            g_pool.push_back(sp.a);
            g_pool.push_back(sp.b);
            continue;
        }
        hipError_t r = hipEventSynchronize(sp.b);
        if (r != hipSuccess) return hip_fail(r, "hipEventSynchronize");
        float t = 0.f;
        r = hipEventElapsedTime(&t, sp.a, sp.b);
        if (r != hipSuccess) return hip_fail(r, "hipEventElapsedTime");
        ms[sp.kind] += t;
        launches[sp.kind] += 1;
        g_pool.push_back(sp.a);
        g_pool.push_back(sp.b);
    }
    g_spans.clear();
    return MMX_OK;
}

int mmx_abi_version(void) { return MMX_ABI_VERSION; }
size_t mmx_workspace_bytes(int n_blocks, int64_t slot_elems, int n_sigma, int with_masks)
{
    if (n_blocks < 1 || slot_elems < 1 || n_sigma < 1) return 0;
    size_t bytes = (size_t)(4 + n_sigma) * (size_t)n_blocks * (size_t)slot_elems * sizeof(float);
    if (with_masks) {
        bytes = (bytes + 15) & ~(size_t)15;
        bytes += (size_t)n_sigma * (((size_t)n_blocks * (size_t)slot_elems) >> 5) * 16;
    }
    return bytes;
}

const char* mmx_strerror(int status)
{
    switch (status) {
        case MMX_OK: return "ok";
        case MMX_ERR_ARG: return "bad argument";
        case MMX_ERR_HIP: return "HIP runtime error";
        case MMX_ERR_NO_DEVICE: return "no gfx950 device";
        case MMX_ERR_WORKSPACE: return "workspace too small";
        case MMX_ERR_UNSUPPORTED: return "unsupported configuration";
        case MMX_DEFERRED: return "left to the caller";
        default: return "unknown status";
    }
}

const char* mmx_last_hip_error(void) { return g_hip_err; }


int mmx_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { hip_fail(e, "hipGetDeviceCount"); return -1; }
    int ok = 0;
    for (int i = 0; i < n; ++i) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, i) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0) ++ok;
    }
    return ok;
}

double mmx_tiled_q16_error_bound(const double* h_w0, const double* h_w2, int radius, double norm)
{
    return mmx_q16_error_bound(h_w0, h_w2, radius, norm);      // (mmx_route.h, with the bounds it follows from)
}

}  // extern "C"

void mmx_batch_geom_make(const mmx_volume* vol, const mmx_block* h_blocks, int n_blocks, int64_t slot_elems,
                         mmx_batch_geom* g)
{
    *g = mmx_batch_geom{};
    g->min_nz = g->min_ny = g->min_nx = 1 << 30;
    g->plan_status = MMX_ERR_UNSUPPORTED;
    g->rows_fit = g->quads_fit = true;
    if (n_blocks < 1 || n_blocks > MMX_MAX_BLOCKS) {       // (the callers' own checks come first: the table is not read)
        g->status = n_blocks < 1 ? MMX_ERR_ARG : MMX_ERR_UNSUPPORTED;
        return;
    }
    for (int i = 0; i < n_blocks; ++i) {
        const mmx_block& b = h_blocks[i];
        if (b.nz < 1 || b.ny < 1 || b.nx < 1 || b.slot != i || b.px < b.nx || b.px % MMX_ROW_ALIGN) {
            if (g->status == MMX_OK) g->status = MMX_ERR_ARG;
            g->bad_block = true;
            return;
        }
        if ((int64_t)b.nz * b.ny * b.px > slot_elems && g->status == MMX_OK) g->status = MMX_ERR_WORKSPACE;
        if (b.nz < g->min_nz) g->min_nz = b.nz;
        if (b.ny < g->min_ny) g->min_ny = b.ny;
        if (b.nx < g->min_nx) g->min_nx = b.nx;
        if (b.ny > g->max_ny) g->max_ny = b.ny;
        if (b.nx > g->max_nx) g->max_nx = b.nx;
        if (b.px > g->max_px) g->max_px = b.px;
        if (b.ny * b.px > g->max_zcols) g->max_zcols = b.ny * b.px;
        if (b.nz * b.px > g->max_ycols) g->max_ycols = b.nz * b.px;
        if (b.nz * b.ny > g->max_rows) g->max_rows = b.nz * b.ny;
        if (b.nz * b.ny * b.px > g->max_vox) g->max_vox = b.nz * b.ny * b.px;
        if (!mmx_entries_fit(MMX_MASK_ROWS, b.nz, b.ny, b.nx, b.px, slot_elems)) g->rows_fit = false;
        if (!mmx_entries_fit(MMX_MASK_QUADS, b.nz, b.ny, b.nx, b.px, slot_elems)) g->quads_fit = false;
        if (vol) {
            const int64_t lane = (int64_t)(b.ny - 1) * vol->stride_y + (int64_t)(b.nx - 1) * vol->stride_x;
            if (lane > g->max_lane_in) g->max_lane_in = lane;
        }
    }
    if (vol) g->plan_status = mmx_zx6_plan_make(h_blocks, n_blocks, slot_elems, vol->dtype, &g->plan);
}

namespace {

// weights per pass: input scale into the z pass, -norm into the x pass
struct pass_weights {
    float z0[MMX_MAX_RADIUS_GENERIC + 1], z2[MMX_MAX_RADIUS_GENERIC + 1];
    float y0[MMX_MAX_RADIUS_GENERIC + 1], y2[MMX_MAX_RADIUS_GENERIC + 1];
    float x0[MMX_MAX_RADIUS_GENERIC + 1], x2[MMX_MAX_RADIUS_GENERIC + 1];
};
void make_weights(const mmx_volume* vol, const double* h_w0, const double* h_w2, int radius, double norm, pass_weights* w)
{
    const double in_scale = mmx_voxel(vol->dtype)->in_scale;     // img_as_float's multiplier; the signed form's 0.5 is the load's
    for (int k = 0; k <= radius; ++k) {
        w->z0[k] = (float)(h_w0[k] * in_scale);
        w->z2[k] = (float)(h_w2[k] * in_scale);
        w->y0[k] = (float)h_w0[k];
        w->y2[k] = (float)h_w2[k];
        w->x0[k] = (float)(-norm * h_w0[k]);
        w->x2[k] = (float)(-norm * h_w2[k]);
    }
}
mmx_taps_f32 taps(const float* a, const float* b, int radius)
{
    mmx_taps_f32 t;
    for (int k = 0; k <= MMX_MAX_RADIUS_FAST; ++k) {
        t.w0[k] = k <= radius ? a[k] : 0.f;
        t.w2[k] = k <= radius ? b[k] : 0.f;
    }
    return t;
}

// A launcher's status where a route sent the call: a refusal means the launcher disagrees with mmx_route.h.
int launched(int rc, const char* launcher, const char* what)
{
    if (rc == MMX_ERR_HIP) return hip_fail(hipGetLastError(), what);
    if (rc == MMX_ERR_UNSUPPORTED) {
        char msg[128];
        snprintf(msg, sizeof msg, "%s refused a call its route accepted", launcher);
        mmx_detect_set_error(msg);
    }
    return rc;
}

// a timed scope, or none (kind < 0)
struct pass_scope {
    int kind; hipStream_t s;
    pass_scope(int k, hipStream_t st) : kind(k), s(st) { if (k >= 0) mmx_time_begin(k, st); }
    ~pass_scope() { if (kind >= 0) mmx_time_end(kind, s); }
};

// Fused path: Z and X in one kernel (Gz / Gzz never touch HBM), then Y -- the tiled matrix-core kernels on the voxel
// copy (made here unless the route trusts the batch's), or the packed-VALU kernel.
int fused_passes(const mmx_log_call& c, const mmx_route& r, const mmx_batch_geom& g, const pass_weights& w)
{
    const mmx_volume* vol = c.vol;
    const int radius = c.radius, n_blocks = c.n_blocks;
    const int64_t slot_elems = c.slot_elems;
    hipStream_t s = c.stream;
    float* t0 = c.d_work;                                   // P
    float* t1 = c.d_work + (int64_t)n_blocks * slot_elems;  // Q
    mmx_taps_f32 tzz = taps(w.z0, w.z2, radius), txx = taps(w.y0, w.y2, radius), tyy = taps(w.x0, w.x2, radius);
    const bool tiled = r.family == MMX_ROUTE_TILED;
    const mmx_zx6_plan& plan = g.plan;
    int rc;
    if (r.makes_copy) {
        mmx_timed_scope ts(MMX_K_ZXPACK, s);
        rc = mmx_launch_zx6_pack(vol, c.d_blocks, c.h_blocks, n_blocks, plan, c.d_work, s);
        if (rc != MMX_OK) return launched(rc, "mmx_launch_zx6_pack", "voxel copy of the tiled path");
    }
    { mmx_timed_scope ts(MMX_K_ZX, s);
      if (tiled)
          rc = mmx_launch_zx6(vol, c.d_blocks, c.h_blocks, n_blocks, plan, txx, radius, c.d_work,
                              r.q16 ? (float)(1.0 / r.bp) : 0.f, r.q16 ? (float)(1.0 / r.bq) : 0.f, r.edge_global, r.zx_rows, s);
      else
          rc = mmx_launch_zx2(vol, c.d_blocks, n_blocks, g.max_ny, g.max_px, slot_elems, tzz, txx, radius, t0, t1, s); }
    if (rc != MMX_OK) return launched(rc, tiled ? "mmx_launch_zx6" : "mmx_launch_zx2", "fused passes");
    { mmx_timed_scope ts(MMX_K_Y2, s);
      unsigned long long* d_mask = r.layout ? (unsigned long long*)c.d_nms_mask : nullptr;
      const float cp = r.q16 ? (float)(r.bp / 65535.0) : 0.f, cq = r.q16 ? (float)(r.bq / 32767.0) : 0.f;
      // int16 voxels on the tiled path: the copy holds u = x ^ 0x8000 and the kernels filter 2 u / 65535 in [0, 2], the image
      // plus one.  "reflect" keeps every tap's weight, so the LoG of that one is the same everywhere, 3 S0^2 S2 of the
      // float64 weight sums, and -norm times it is what the Y pass takes off again before anything looks at a value.
      float bias = 0.f;
      if (tiled && vol->dtype == MMX_I16) {
          double s0 = c.h_w0[0], s2 = c.h_w2[0];
          for (int k = 1; k <= radius; ++k) { s0 += 2.0 * c.h_w0[k]; s2 += 2.0 * c.h_w2[k]; }
          bias = (float)(c.norm * 3.0 * s0 * s0 * s2);
      }
      if (r.y_kernel == MMX_Y_YM)
          rc = mmx_launch_ym(c.d_blocks, n_blocks, plan, slot_elems, tyy, radius, c.d_work, cp, cq, bias, c.d_log, d_mask,
                             c.nms_lo, c.nms_eps, s);
      else if (r.y_kernel == MMX_Y_Y6)
          rc = mmx_launch_y6(c.d_blocks, n_blocks, plan, slot_elems, tyy, radius, c.d_work,
                             reinterpret_cast<const float*>(reinterpret_cast<const char*>(c.d_work) + plan.q_off), cp, cq, bias,
                             c.d_log, d_mask, c.nms_lo, c.nms_eps, s);
      else
          rc = mmx_launch_y2(c.d_blocks, n_blocks, g.max_ycols, slot_elems, tyy, radius, t0, t1, c.d_log, d_mask, c.nms_lo,
                             c.nms_eps, s); }
    return launched(rc, r.y_kernel == MMX_Y_YM ? "mmx_launch_ym" : (r.y_kernel == MMX_Y_Y6 ? "mmx_launch_y6" : "mmx_launch_y2"),
                    "fused passes");
}

// The wide passes (mmx_wide.hip): Z, X, Y on LDS-staged tiles, radius 1 .. MMX_MAX_RADIUS_WIDE, row entries from the Y
// pass.
int wide_passes(const mmx_log_call& c, const mmx_route& r, const pass_weights& w)
{
    const int radius = c.radius, n_blocks = c.n_blocks;
    const int64_t slot_elems = c.slot_elems;
    hipStream_t s = c.stream;
    float* t0 = c.d_work;                                   // P
    float* t1 = t0 + (int64_t)n_blocks * slot_elems;        // Q
    float* t2 = t1 + (int64_t)n_blocks * slot_elems;        // Gz
    float* t3 = t2 + (int64_t)n_blocks * slot_elems;        // Gzz
    unsigned long long* d_mask = r.layout ? (unsigned long long*)c.d_nms_mask : nullptr;
    int rc;
    { mmx_timed_scope ts(MMX_K_WIDE, s);
      rc = mmx_launch_wide_pass(0, c.vol, c.d_blocks, c.h_blocks, n_blocks, slot_elems, w.z0, w.z2, radius, nullptr, nullptr,
                                t2, t3, nullptr, 0.f, 0.f, s); }
    if (rc == MMX_OK) {
        mmx_timed_scope ts(MMX_K_WIDE, s);
        rc = mmx_launch_wide_pass(1, c.vol, c.d_blocks, c.h_blocks, n_blocks, slot_elems, w.y0, w.y2, radius, t2, t3, t0, t1,
                                  nullptr, 0.f, 0.f, s);
    }
    if (rc == MMX_OK) {
        mmx_timed_scope ts(MMX_K_WIDE, s);
        rc = mmx_launch_wide_pass(2, c.vol, c.d_blocks, c.h_blocks, n_blocks, slot_elems, w.x0, w.x2, radius, t0, t1, c.d_log,
                                  nullptr, d_mask, c.nms_lo, c.nms_eps, s);
    }
    return launched(rc, "mmx_launch_wide_pass", "wide passes");
}

// The three separate passes, Z, Y, X: per pass the register-ring kernel (ring bit), the folded-reflection pass (fold
// bit) or the generic one; bit 0 = Z, 1 = Y, 2 = X.  `timed`: under the timing scopes of their families.
int three_passes(const mmx_volume* vol, const mmx_block* d_blocks, int n_blocks, int64_t slot_elems, int radius,
                 float* d_work, float* d_log, const mmx_batch_geom& g, const pass_weights& w, int rings, int folds,
                 bool timed, hipStream_t s)
{
    float* t0 = d_work;                                     // Gz
    float* t1 = t0 + (int64_t)n_blocks * slot_elems;        // Gzz
    float* t2 = t1 + (int64_t)n_blocks * slot_elems;        // A
    float* t3 = t2 + (int64_t)n_blocks * slot_elems;        // BC
    const float* w0[3] = {w.z0, w.y0, w.x0};
    const float* w2[3] = {w.z2, w.y2, w.x2};
    const float* in1[3] = {nullptr, t0, t2};
    const float* in2[3] = {nullptr, t1, t3};
    float* out1[3] = {t0, t2, d_log};
    float* out2[3] = {t1, t3, nullptr};
    const int ring_kind[3] = {MMX_K_ZPASS, MMX_K_YPASS, MMX_K_XPASS};
    const char* ring_name[3] = {"mmx_launch_zpass", "mmx_launch_ypass", "mmx_launch_xpass"};
    const char* what[3] = {"z pass", "y pass", "x pass"};
    for (int p = 0; p < 3; ++p) {
        const bool ring = (rings >> p) & 1, fold = !ring && ((folds >> p) & 1);
        int rc;
        { pass_scope ts(!timed ? -1 : (ring ? ring_kind[p] : (fold ? MMX_K_THIN : MMX_K_GENERIC)), s);
        if (ring && p == 0) rc = mmx_launch_zpass(vol, d_blocks, n_blocks, g.max_zcols, slot_elems, taps(w.z0, w.z2, radius), radius, t0, t1, s);
        else if (ring && p == 1) rc = mmx_launch_ypass(d_blocks, n_blocks, g.max_ycols, slot_elems, taps(w.y0, w.y2, radius), radius, t0, t1, t2, t3, s);
        else if (ring) rc = mmx_launch_xpass(d_blocks, n_blocks, g.max_rows, g.max_nx, slot_elems, taps(w.x0, w.x2, radius), radius, t2, t3, d_log, s);
        else rc = (fold ? mmx_launch_fold_pass : mmx_launch_generic_pass)(p, vol, d_blocks, n_blocks, g.max_vox, slot_elems, w0[p], w2[p],
                                                                          radius, in1[p], in2[p], out1[p], out2[p], s); }
        if (rc != MMX_OK)
            return launched(rc, ring ? ring_name[p] : (fold ? "mmx_launch_fold_pass" : "mmx_launch_generic_pass"), what[p]);
    }
    return MMX_OK;
}

}  // namespace

// The argument checks of mmx_log_batch_f32, everything but the blocks (the mode: the route's parsing).
int mmx_log_scale_check(const mmx_log_call& c)
{
    mmx_zx_request q;
    if (mmx_zx_parse(c.zx_mode, &q) != MMX_OK) return MMX_ERR_ARG;
    if (!c.vol || !c.vol->d_data || !c.d_blocks || !c.h_blocks || !c.h_w0 || !c.h_w2 || !c.d_log || !c.d_work)
        return MMX_ERR_ARG;
    if (c.n_blocks < 1 || c.radius < 0 || c.slot_elems < 1) return MMX_ERR_ARG;
    if (c.n_blocks > MMX_MAX_BLOCKS) return MMX_ERR_UNSUPPORTED;
    if (c.radius > MMX_MAX_RADIUS_GENERIC) return MMX_ERR_UNSUPPORTED;
    if (c.slot_elems >= (int64_t(1) << 29)) return MMX_ERR_UNSUPPORTED;  // 32-bit byte offsets in a slot
    if (c.slot_elems % MMX_ROW_ALIGN) return MMX_ERR_ARG;
    if (!mmx_voxels_ok(c.vol)) return MMX_ERR_UNSUPPORTED;     // float64 volumes: pass a float32 copy
    return MMX_OK;
}

// One scale, launched as its route says: nothing is decided here.
int mmx_log_scale_run(const mmx_log_call& c, const mmx_batch_geom& g, const mmx_route& r)
{
    pass_weights w;
    make_weights(c.vol, c.h_w0, c.h_w2, c.radius, c.norm, &w);
    int rc;
    if (r.family == MMX_ROUTE_WIDE) rc = wide_passes(c, r, w);
    else if (r.family == MMX_ROUTE_SEPARATE)
        rc = three_passes(c.vol, c.d_blocks, c.n_blocks, c.slot_elems, c.radius, c.d_work, c.d_log, g, w,
                          r.ring_z | r.ring_y << 1 | r.ring_x << 2, r.fold_z | r.fold_y << 1 | r.fold_x << 2, true, c.stream);
    else rc = fused_passes(c, r, g, w);
    if (rc != MMX_OK) return rc;
    if (c.h_zx_path) *c.h_zx_path = r.path;
    if (c.h_mask_written) *c.h_mask_written = r.layout;
    return MMX_OK;
}

namespace {
// mmx_log_batch_f32 behind its mmx_batch_geom_make: check, route (mmx_route.h), run
int log_scale(const mmx_log_call& c, const mmx_batch_geom& g)
{
    if (c.h_mask_written) *c.h_mask_written = 0;
    if (c.h_zx_path) *c.h_zx_path = MMX_ZX_SEPARATE;
    int rc = mmx_log_scale_check(c);
    if (rc != MMX_OK) return rc;
    mmx_route r;
    rc = mmx_route_scale(c.vol, g, c.radius, c.h_w0, c.h_w2, c.norm, c.zx_mode, c.nms_eps, c.d_nms_mask && c.h_mask_written, &r);
    return rc != MMX_OK ? rc : mmx_log_scale_run(c, g, r);
}
}  // namespace

int mmx_zx_pack_geom(const mmx_volume* vol, const mmx_block* d_blocks, const mmx_block* h_blocks, int n_blocks,
                     int64_t slot_elems, const mmx_batch_geom& g, float* d_work, hipStream_t stream)
{
    if (!vol || !vol->d_data || !d_blocks || !h_blocks || !d_work || n_blocks < 1 || slot_elems < 1) return MMX_ERR_ARG;
    if (n_blocks > MMX_MAX_BLOCKS) return MMX_ERR_UNSUPPORTED;
    if (!mmx_voxels_ok(vol)) return MMX_ERR_UNSUPPORTED;
    if (g.bad_block) return MMX_ERR_ARG;
    if (g.plan_status != MMX_OK) return g.plan_status;
    mmx_timed_scope ts(MMX_K_ZXPACK, stream);
    const int rc = mmx_launch_zx6_pack(vol, d_blocks, h_blocks, n_blocks, g.plan, d_work, stream);
    return rc == MMX_ERR_HIP ? hip_fail(hipGetLastError(), "voxel copy of the tiled path") : rc;
}

extern "C" {

int mmx_log_batch_f32(const mmx_volume* vol, const mmx_block* d_blocks, const mmx_block* h_blocks,
                      int n_blocks, int64_t slot_elems,
                      const double* h_w0, const double* h_w2, int radius, double norm,
                      float* d_log, float* d_work, uint64_t* d_nms_mask, float nms_lo, float nms_eps,
                      int* h_mask_written, int zx_mode, int* h_zx_path, void* stream)
{
    mmx_batch_geom g{};
    if (vol && h_blocks) mmx_batch_geom_make(vol, h_blocks, n_blocks, slot_elems, &g);     // (NULL: refused below, g unread)
    return log_scale({vol, d_blocks, h_blocks, n_blocks, slot_elems, h_w0, h_w2, radius, norm, d_log, d_work,
                              d_nms_mask, nms_lo, nms_eps, h_mask_written, zx_mode, h_zx_path, (hipStream_t)stream}, g);
}

// Same as mmx_log_batch_f32 but always through the generic kernels (tests cross-check the
// register-ring kernels against it; also what very large sigmas take).
int mmx_log_batch_f32_generic(const mmx_volume* vol, const mmx_block* d_blocks, const mmx_block* h_blocks,
                              int n_blocks, int64_t slot_elems,
                              const double* h_w0, const double* h_w2, int radius, double norm,
                              float* d_log, float* d_work, void* stream)
{
    if (!vol || !vol->d_data || !d_blocks || !h_blocks || !h_w0 || !h_w2 || !d_log || !d_work)
        return MMX_ERR_ARG;
    if (n_blocks < 1 || radius < 0 || radius > MMX_MAX_RADIUS_GENERIC || slot_elems < 1) return MMX_ERR_ARG;
    if (n_blocks > MMX_MAX_BLOCKS) return MMX_ERR_UNSUPPORTED;
    if (!mmx_voxel_in(vol->dtype, MMX_VOX_ALL)) return MMX_ERR_UNSUPPORTED;    // (float64 voxels too: mmx_load_any)
    mmx_batch_geom g;
    mmx_batch_geom_make(vol, h_blocks, n_blocks, slot_elems, &g);
    if (g.status != MMX_OK) return g.status;
    pass_weights w;
    make_weights(vol, h_w0, h_w2, radius, norm, &w);
    return three_passes(vol, d_blocks, n_blocks, slot_elems, radius, d_work, d_log, g, w, 0, 0, false, (hipStream_t)stream);
}

int mmx_zx_pack(const mmx_volume* vol, const mmx_block* d_blocks, const mmx_block* h_blocks, int n_blocks,
                int64_t slot_elems, float* d_work, void* stream)
{
    mmx_batch_geom g{};
    if (vol && h_blocks) mmx_batch_geom_make(vol, h_blocks, n_blocks, slot_elems, &g);     // (NULL: refused below, g unread)
    return mmx_zx_pack_geom(vol, d_blocks, h_blocks, n_blocks, slot_elems, g, d_work, (hipStream_t)stream);
}

int mmx_peaks_batch(const float* d_log, const uint64_t* d_nms_mask, int mask_layout, int n_sigma, const mmx_block* d_blocks,
                    const mmx_block* h_blocks, int n_blocks, int64_t slot_elems,
                    float thr, float eps, mmx_cand* d_cands, uint32_t cap,
                    uint32_t* d_count, void* stream)
{
    if (!d_log || !d_blocks || !h_blocks || !d_cands || !d_count) return MMX_ERR_ARG;
    if (n_sigma < 1 || n_blocks < 1 || slot_elems < 1 || !(eps >= 0.f)) return MMX_ERR_ARG;
    if (n_blocks > MMX_MAX_BLOCKS) return MMX_ERR_UNSUPPORTED;
    if (slot_elems % MMX_ROW_ALIGN) return MMX_ERR_ARG;
    if (d_nms_mask && mask_layout != MMX_MASK_ROWS && mask_layout != MMX_MASK_QUADS) return MMX_ERR_ARG;
    mmx_batch_geom g;
    mmx_batch_geom_make(nullptr, h_blocks, n_blocks, slot_elems, &g);
    if (g.status != MMX_OK) return g.status;
    const int max_vox = g.max_vox;
    mmx_timed_scope ts(MMX_K_PEAKS, (hipStream_t)stream);
    int rc;
    if (d_nms_mask)
        rc = mmx_launch_peaks_sparse(d_log, (const unsigned long long*)d_nms_mask, n_sigma,
                                     (int64_t)n_blocks * slot_elems, d_blocks, n_blocks, max_vox, slot_elems,
                                     thr, eps, d_cands, cap, d_count, mask_layout == MMX_MASK_QUADS, (hipStream_t)stream);
    else
        rc = mmx_launch_peaks(d_log, n_sigma, (int64_t)n_blocks * slot_elems, d_blocks, n_blocks, max_vox,
                              slot_elems, thr, eps, d_cands, cap, d_count, (hipStream_t)stream);
    return rc == MMX_ERR_HIP ? hip_fail(hipGetLastError(), "peaks") : rc;
}

// A rectangle of a host image into its place in the device copy: `height` rows of `width` bytes, the rows spitch /
// dpitch bytes apart (hipMemcpy2DAsync, host -> device, on `stream`; the host side pinned for the copy to be
// asynchronous).  What lets a host volume go up block row by block row -- the y-band of a z-range is `planes` rows of
// (band rows x row bytes) bytes, one plane pitch apart -- instead of whole z-slabs (volume._SlabUpload).
int mmx_copy_rect_h2d(void* d_dst, size_t dpitch, const void* h_src, size_t spitch, size_t width, size_t height,
                      void* stream)
{
    if (!d_dst || !h_src || width > dpitch || width > spitch) return MMX_ERR_ARG;
    if (!width || !height) return MMX_OK;
    hipError_t r = hipMemcpy2DAsync(d_dst, dpitch, h_src, spitch, width, height, hipMemcpyHostToDevice, (hipStream_t)stream);
    return r == hipSuccess ? MMX_OK : hip_fail(r, "hipMemcpy2DAsync");
}

int mmx_event_create(void** ev)
{
    if (!ev) return MMX_ERR_ARG;
    hipEvent_t e;
    hipError_t r = hipEventCreate(&e);
    if (r != hipSuccess) return hip_fail(r, "hipEventCreate");
    *ev = (void*)e;
    return MMX_OK;
}

int mmx_event_destroy(void* ev)
{
    hipError_t r = hipEventDestroy((hipEvent_t)ev);
    return r == hipSuccess ? MMX_OK : hip_fail(r, "hipEventDestroy");
}

int mmx_event_record(void* ev, void* stream)
{
    hipError_t r = hipEventRecord((hipEvent_t)ev, (hipStream_t)stream);
    return r == hipSuccess ? MMX_OK : hip_fail(r, "hipEventRecord");
}

int mmx_event_elapsed_ms(void* start, void* stop, float* ms)
{
    if (!ms) return MMX_ERR_ARG;
    hipError_t r = hipEventSynchronize((hipEvent_t)stop);
    if (r != hipSuccess) return hip_fail(r, "hipEventSynchronize");
    r = hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop);
    return r == hipSuccess ? MMX_OK : hip_fail(r, "hipEventElapsedTime");
}

}  // extern "C"
