// Shared declarations for the gfx950 kernels of libmmx_hip.so.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mmx.h"

// What a voxel type is: its record, the accepted sets, the dispatcher and the device traits
#include "mmx_voxel.h"

#define MMX_WG 256  // workgroup size used by the streaming kernels (4 waves of 64)
#define MMX_MAX_GRID_X 2147483647  // workgroups along x of one launch

// Half kernels (index k = distance from the centre tap) passed BY VALUE in the
// kernarg segment, so that with a fully unrolled tap loop every weight is a scalar
// (SGPR) operand of its v_fma.
struct mmx_taps_f32 {
    float w0[MMX_MAX_RADIUS_FAST + 1];  // order-0 Gaussian
    float w2[MMX_MAX_RADIUS_FAST + 1];  // order-2 (second derivative) Gaussian
};

// scipy "reflect" (half-sample symmetric): d c b a | a b c d | d c b a.
// Valid for any i (also |i| >> n), as scipy's NI_ExtendLine is.
__host__ __device__ __forceinline__ int mmx_reflect(int i, int n)
{
    if (n == 1) return 0;
    const int period = 2 * n;
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - 1 - i;
}

// internal launchers (defined one per translation unit, called by mmx_api.hip)
int mmx_launch_zpass(const mmx_volume* vol, const mmx_block* d_blocks, int n_blocks, int max_cols,
                     int64_t slot_elems, const mmx_taps_f32& taps, int radius,
                     float* d_gz, float* d_gzz, hipStream_t stream);
int mmx_launch_ypass(const mmx_block* d_blocks, int n_blocks, int max_cols, int64_t slot_elems,
                     const mmx_taps_f32& taps, int radius, const float* d_gz, const float* d_gzz,
                     float* d_a, float* d_bc, hipStream_t stream);
int mmx_launch_xpass(const mmx_block* d_blocks, int n_blocks, int max_rows, int max_nx,
                     int64_t slot_elems, const mmx_taps_f32& taps, int radius,
                     const float* d_a, const float* d_bc, float* d_log, hipStream_t stream);

int mmx_launch_zx2(const mmx_volume* vol, const mmx_block* d_blocks, int n_blocks, int max_ny, int max_px,
                   int64_t slot_elems, const mmx_taps_f32& tz, const mmx_taps_f32& tx, int radius,
                   float* d_p, float* d_q, hipStream_t s);
// Tiled fused path (zx_mode 6): where its pieces live inside the four intermediate arrays of d_work
// (4 n_blocks slot_elems floats).  P and Q as 16 x 16 tiles (mmx_fused4.hip: zx4_kernel), the Toeplitz
// fragment tables of the current sigma, and the operand-ordered copy of the blocks' voxels (zx6_pack_kernel),
// which survives from one sigma of a batch to the next.
struct mmx_zx6_plan {
    int64_t tile_stride;    // floats per block of tiled P (and of Q): max over blocks of ntx ntz ny 256
    int64_t pack_stride;    // uint16 elements per block of packed voxels: max over blocks of ny ntz nch8 128
    int64_t q_off, tab_off, pack_off;      // byte offsets into d_work (P at 0)
    int64_t tab_bytes;
    int max_tiles;          // max ntx ntz
    int max_rowtiles;       // max ny ntz
};
int mmx_zx6_plan_make(const mmx_block* h_blocks, int n_blocks, int64_t slot_elems, int voxel_dtype, mmx_zx6_plan* plan);
int mmx_launch_zx6_pack(const mmx_volume* vol, const mmx_block* d_blocks, const mmx_block* h_blocks, int n_blocks,
                        const mmx_zx6_plan& plan, void* d_work, hipStream_t stream);
int mmx_launch_zx6(const mmx_volume* vol, const mmx_block* d_blocks, const mmx_block* h_blocks, int n_blocks,
                   const mmx_zx6_plan& plan, const mmx_taps_f32& tx, int radius, void* d_work, float qp, float qq,
                   bool edge_global, int rows, hipStream_t stream);
// The row march's schedule on the host, exported for tests and tools (not part of include/mmx.h): for a launch of n_blocks
// blocks with rows[b] rows and waves_per_row[b] waves per row on a device with `slots` resident waves of the row kernel
// (< 0: the current device's, asked of the runtime), nr[b] = the rows per wave of block b -- never growing from block to
// block, 1 on the last blocks and everywhere in small launches; forced > 0: that value everywhere.  cover (may be NULL):
// one counter per (block, row, wave of the row), blocks one after the other, raised by every wave of the flat grid that
// owns it, found as the kernel finds its rows -- all 1 when every row is marched once.  Returns the workgroups of the flat
// grid, or minus a status.
extern "C" int mmx_zx_rows_schedule(int n_blocks, const int32_t* rows, const int32_t* waves_per_row, int slots, int forced,
                                    int32_t* nr, int32_t* cover);
// cp, cq > 0: d_p holds Q16 tiles, P = unorm16 * cp, Q = snorm16 * cq (d_q unused); 0: float32 tiles
// bias: added to every output before the threshold and the entries (int16 voxels: the scale's constant; else 0)
int mmx_launch_y6(const mmx_block* d_blocks, int n_blocks, const mmx_zx6_plan& plan, int64_t slot_elems,
                  const mmx_taps_f32& taps, int radius, const float* d_p, const float* d_q, float cp, float cq, float bias,
                  float* d_log, unsigned long long* d_mask, float nms_lo, float nms_eps, hipStream_t stream);
// the same on the matrix cores (mmx_ymfma.hip): 16-bit tiles only, radius <= 24; MMX_ERR_UNSUPPORTED otherwise
int mmx_launch_ym(const mmx_block* d_blocks, int n_blocks, const mmx_zx6_plan& plan, int64_t slot_elems,
                  const mmx_taps_f32& taps, int radius, const float* d_p, float cp, float cq, float bias,
                  float* d_log, unsigned long long* d_mask, float nms_lo, float nms_eps, hipStream_t stream);
int mmx_launch_y2(const mmx_block* d_blocks, int n_blocks, int max_cols, int64_t slot_elems,
                  const mmx_taps_f32& taps, int radius, const float* d_p, const float* d_q,
                  float* d_log, unsigned long long* d_mask, float nms_lo, float nms_eps, hipStream_t stream);

// The wide passes (mmx_wide.hip): radius 1 .. MMX_MAX_RADIUS_WIDE.  pass 0 = Z (the volume -> out1, out2 = Gz, Gzz),
// 1 = X (in1, in2 -> out1, out2 = P, Q), 2 = Y (in1, in2 = P, Q -> out1 = the LoG array; d_mask: row entries or NULL).
int mmx_launch_wide_pass(int pass, const mmx_volume* vol, const mmx_block* d_blocks, const mmx_block* h_blocks, int n_blocks,
                         int64_t slot_elems, const float* w0, const float* w2, int radius,
                         const float* in1, const float* in2, float* out1, float* out2,
                         unsigned long long* d_mask, float nms_lo, float nms_eps, hipStream_t s);

// What the entry points derive from a batch's block table (mmx_batch_geom_make): nothing in it depends on sigma, so
// a whole batch (mmx_log_scales_f32) fills it once.
struct mmx_batch_geom {
    // the blocks checked in table order: MMX_ERR_ARG for an extent < 1, a slot other than the block's index or a row
    // pitch below nx / off MMX_ROW_ALIGN (bad_block: one was found, whatever came before it), MMX_ERR_WORKSPACE for a
    // block larger than its slot; entry points return it where their own checks of the blocks stood
    int status;
    bool bad_block;
    int min_nz, min_ny, min_nx, max_ny, max_nx, max_px;
    int max_zcols, max_ycols, max_rows, max_vox;        // ny px, nz px, nz ny, nz ny px
    int64_t max_lane_in;                                // largest (y, x) offset inside a block's input plane, in voxels
    bool rows_fit, quads_fit;                           // every block's NMS entries fit its slot / 32 words, per layout
    mmx_zx6_plan plan;                                  // the tiled path's share of d_work
    int plan_status;                                    // MMX_OK: it fits
};
// (vol: NULL for callers that read no voxels -- no plan, no input offsets)
void mmx_batch_geom_make(const mmx_volume* vol, const mmx_block* h_blocks, int n_blocks, int64_t slot_elems, mmx_batch_geom* g);

// The NMS entry layouts and the rule that decides an entry (host: the index arithmetic; device: the rule)
#include "mmx_entries.h"

// mmx_rescore.hip (internal; mmx_detect_batch calls it): mmx_rescore_f64 with the store type chosen per block.
//   d_block_f32 == NULL : every block alike, float32 intermediates where store_f32 is set and the voxels are float32
//   d_block_f32 != NULL : a device flag per block over a float64 volume (store_f32 is not read)
int mmx_rescore_per_block(const mmx_volume* vol, const mmx_block* d_blocks, int n_blocks, mmx_cand* d_pts, uint32_t cap,
                          const uint32_t* d_count, const double* d_w0, const double* d_w2, const int32_t* h_radius,
                          const double* h_norm, int n_sigma, int store_f32, const int32_t* d_block_f32, void* stream);

// The kernel-path rules: the launchers' predicates, the route of a scale and of a ladder (host-only, no launch)
#include "mmx_route.h"

// mmx_log_batch_f32 and mmx_zx_pack behind their mmx_batch_geom_make (mmx_api.hip): what mmx_log_scales_f32 calls.
struct mmx_log_call {       // (the arguments of mmx_log_batch_f32)
    const mmx_volume* vol; const mmx_block* d_blocks; const mmx_block* h_blocks; int n_blocks; int64_t slot_elems;
    const double* h_w0; const double* h_w2; int radius; double norm;
    float* d_log; float* d_work; uint64_t* d_nms_mask; float nms_lo, nms_eps; int* h_mask_written;
    int zx_mode; int* h_zx_path; hipStream_t stream;
};
int mmx_log_scale_check(const mmx_log_call& c);                                                 // its argument checks
int mmx_log_scale_run(const mmx_log_call& c, const mmx_batch_geom& g, const mmx_route& r);     // its launches, as routed
int mmx_zx_pack_geom(const mmx_volume* vol, const mmx_block* d_blocks, const mmx_block* h_blocks, int n_blocks,
                     int64_t slot_elems, const mmx_batch_geom& g, float* d_work, hipStream_t stream);
// what mmx_detect_last_error returns next on this thread (mmx_detect.hip)
void mmx_detect_set_error(const char* msg);

// ---- optional per-kernel-family timing with HIP events on the launch stream (bench.py) ----
enum mmx_kernel_kind {
    MMX_K_ZPASS = 0, MMX_K_YPASS, MMX_K_XPASS, MMX_K_GENERIC, MMX_K_PEAKS, MMX_K_RESCORE,
    MMX_K_PAIRS, MMX_K_CLOSE, MMX_K_ZX, MMX_K_Y2, MMX_K_PREPROC, MMX_K_COLOC, MMX_K_ZXPACK, MMX_K_WIDE, MMX_K_END
};
void mmx_time_begin(int kind, hipStream_t s);
void mmx_time_end(int kind, hipStream_t s);
static_assert(MMX_K_END == MMX_K_COUNT, "kernel kinds out of sync with mmx.h");
// (MMX_K_THIN, the folded passes, is the slot behind them: mmx.h, MMX_K_SLOTS)
static_assert(MMX_K_THIN == MMX_K_END && MMX_K_SLOTS == MMX_K_THIN + 1, "the thin family follows the counted ones");
struct mmx_timed_scope {
    int kind; hipStream_t s;
    mmx_timed_scope(int k, hipStream_t st) : kind(k), s(st) { mmx_time_begin(k, st); }
    ~mmx_timed_scope() { mmx_time_end(kind, s); }
};
