// Per-block preprocessing ahead of blob detection: contrast stretch + unsharp mask + erosion.
//
// What the reference does to every denoise sub-block of every detection block
// (magmap/cv/stack_detect.py:122-150) before `blob_log` sees it:
//   saturate_roi (magmap/plot/plot_3d.py:55-112)
//       vmin, vmax = np.percentile(roi, (clip_vmin, clip_vmax))          # linear interpolation
//       vmax = max(vmax, near_max * max_thresh_factor);  roi unchanged when vmin == vmax
//       sat  = (np.clip(roi, vmin, vmax) - vmin) / (vmax - vmin)
//   denoise_roi  (plot_3d.py:115-172)
//       mean = np.mean(sat);  den = np.clip(sat, clip_min, clip_max)
//       den  = den + (den - unsharp_strength * gaussian(den, sigma 8, 'nearest', truncate 4))
//       den  = grey_erosion(den, octahedron(1))  if  mean > erosion_threshold
// all in float64.  The result feeds an exact float64 re-score (mmx_rescore.hip), so it is
// reproduced BIT FOR BIT: the same IEEE operations in the same order as NumPy / SciPy
// (NI_Correlate1D symmetric branch: acc = in[c]*w0; for k = R..1: acc += (in[c-k]+in[c+k])*w[k]),
// no FMA contraction (this file is built with -ffp-contract=off), correctly rounded division.
// oracle/preprocess_oracle.py states the same on the CPU and is pinned to the real reference.
//
// Design (gfx950).  A stock sub-block is 25^3 voxels = 122 KiB of float64: it lives in LDS for
// its whole life, ONE workgroup per sub-block (a CU's 160 KiB holds exactly one), HBM is
// touched once for the 2-byte voxels and once for the 12 bytes of output per voxel.
//   1. voxels -> LDS as doubles + 256-bin histogram of the high byte (LDS atomics)
//   2. the 2x2 order statistics np.percentile needs: two-level radix select (wave scan over
//      the bins), then NumPy's _lerp in double
//   3. saturate, block-sum for the mean, clip -> LDS.  The mean only gates the erosion; it is
//      summed in parallel and, if that lands within 1e-9 of the threshold, re-summed by one
//      lane in NumPy's pairwise order (numpy/_core/src/umath/loops_utils.h.src) -- bit exact
//   4. three in-place Gaussian passes: a lane owns a whole line (<= 32 voxels) in registers,
//      'nearest' extension is the last register replicated, so all tap indices are
//      compile-time; the 33 weights sit in SGPRs (kernarg).  ~97 float64 ops per voxel and
//      axis: this stage is float64-ALU bound (about 30 us per sub-block and CU)
//   5. unsharp in place, then the 7-point minimum (reflect == skip outside) if eroding,
//      float64 + float32 copies out (the float32 copy feeds the LoG passes)
// Sub-blocks with a side above 32 or more voxels than LDS holds take pp_generic_kernel:
// same arithmetic, data in a global scratch, one output per lane and pass.


#include "mmx_pp_common.h"

namespace {

template <typename InT, int WG>
__global__ void __launch_bounds__(WG)
pp_fast_kernel(const InT* __restrict__ vol, int64_t sz, int64_t sy, int64_t sx,
               const mmx_subblock* __restrict__ subs, int n_subs,
               const mmx_quantile_class* __restrict__ qcs, const double* __restrict__ wts,
               pp_args A, float* __restrict__ out32, double* __restrict__ out64,
               mmx_subblock_info* __restrict__ info)
{
    extern __shared__ double tile[];
    __shared__ pp_ranks s_ranks;
    __shared__ double s_red[WG / 64];
    __shared__ double s_mean;
    __shared__ int s_flags;
    __shared__ pp_stack s_stack;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // Workgroups are dealt to the 8 XCDs round-robin; give each XCD a CONTIGUOUS run of tiles so
    // that x-neighbouring tiles (which share 128-byte lines of the source rows and of both
    // outputs) meet in one L2.
    const int per = (n_subs + 7) >> 3;
    const int sub_id = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (sub_id >= n_subs) return;
    const mmx_subblock sb = subs[sub_id];
    const int nz = sb.nz, ny = sb.ny, nx = sb.nx, n = nz * ny * nx;
    const int px = nx | 1;                        // odd row pitch: no LDS bank conflicts on x lines
    uint32_t* hist = (uint32_t*)(tile + nz * ny * px);
    uint16_t* raw = (uint16_t*)(hist + PP_HIST);  // the voxels themselves, dense index
    const InT* src = vol + sb.src_off;
    const float inv_nx = 1.0f / (float)nx, inv_ny = 1.0f / (float)ny;

    for (int i = tid; i < PP_HIST; i += WG) hist[i] = 0;
    __syncthreads();

    // Lane <-> voxel mapping of the element-wise stages: a lane keeps its x and walks rows
    // (z*ny + y) in steps of `rpi`, so no per-voxel index decoding; rpi * nx <= WG lanes work.
    const int nrows = nz * ny;
    const int rpi = WG / nx;
    const int r_first = (int)(((float)tid + 0.5f) * inv_nx);
    const int x = tid - r_first * nx;
    const int r0 = r_first < rpi ? r_first : nrows;          // idle lanes start past the end

    // 1. voxels -> LDS, histogram of the high byte.  Loads are issued PP_NB at a time: with one
    //    workgroup per CU nothing else hides their latency.
    for (int rb0 = 0; rb0 < nrows; rb0 += PP_NB_LOAD * rpi) {     // same trip count in every lane (ballots)
        const int rb = r0 + rb0;
        int v[PP_NB_LOAD];
#pragma unroll
        for (int j = 0; j < PP_NB_LOAD; ++j) {
            const int row = rb + j * rpi < nrows ? rb + j * rpi : 0;
            const int z = (int)(((float)row + 0.5f) * inv_ny);
            const int y = row - z * ny;
            v[j] = (int)src[z * sz + y * sy + (r0 < nrows ? x : 0) * sx] + pp_vox<InT>::bias;      // (keys)
        }
#pragma unroll
        for (int j = 0; j < PP_NB_LOAD; ++j) {
            const int row = rb + j * rpi;
            if (row < nrows) raw[row * nx + x] = (uint16_t)v[j];
            pp_hist_add(hist, v[j] >> 8, row < nrows);
        }
    }
    __syncthreads();

    // 2. order statistics: ranks lo_prev, lo_next, hi_prev, hi_next
    const mmx_quantile_class qc = qcs[sb.qclass];
    pp_select_high(hist, qc, &s_ranks);
    __syncthreads();
    {
        const pp_bins bins(&s_ranks);
        for (int i = tid; i < n; i += WG) bins.add(hist, raw[i]);
    }
    __syncthreads();
    pp_select_low(hist, &s_ranks);
    __syncthreads();

    const pp_bounds B = pp_key_bounds<InT>(&s_ranks, qc, A.max_thresh);
    const auto S = pp_sat_t<pp_vox<InT>::is_signed>::make(B.vmin, B.vmax, B.identity);

    // 3. saturate, sum, clip -> the float64 tile (PP_NB independent divisions in flight per lane)
    double part = 0.;
    for (int rb = r0; rb < nrows; rb += PP_NB * rpi) {
        double s[PP_NB];
#pragma unroll
        for (int j = 0; j < PP_NB; ++j) {
            const int row = rb + j * rpi < nrows ? rb + j * rpi : rb;
            s[j] = S((double)((int)raw[row * nx + x] - pp_vox<InT>::bias));
        }
#pragma unroll
        for (int j = 0; j < PP_NB; ++j) {
            const int row = rb + j * rpi;
            if (row < nrows) {
                part += s[j];
                tile[row * px + x] = pp_clip(s[j], A.clip_min, A.clip_max);
            }
        }
    }
    if (!S.fast) {                 // extreme span (never with integer voxels): plain division, same stores
        part = 0.;
        for (int row = r0; row < nrows; row += rpi) {
            const double sv = S.plain((double)((int)raw[row * nx + x] - pp_vox<InT>::bias));
            part += sv;
            tile[row * px + x] = pp_clip(sv, A.clip_min, A.clip_max);
        }
    }
    part = pp_wave_sum(part);
    if (lane == 0) s_red[wave] = part;
    __syncthreads();
    if (tid == 0) {
        double tot = 0.;
        for (int w = 0; w < WG / 64; ++w) tot += s_red[w];
        double mean = tot / (double)n;
        s_flags = pp_mean_verdict(mean, S.identity, A, [&](double& m) {
            auto val = [&](int i) { return S.plain((double)((int)raw[i] - pp_vox<InT>::bias)); };
            m = pp_pairwise(val, n, &s_stack) / (double)n;
            return pp_exact_verdict(m, A);
        });
        s_mean = mean;
    }
    __syncthreads();
    const int flags = s_flags;
    if (info && tid == 0) pp_write_info(info, sub_id, B.vmin, B.vmax, s_mean, flags);

    // 4. Gaussian blur, axis 0, 1, 2 in place (scipy gaussian_filter order)
    if (A.do_unsharp) {
        double wl[PP_R + 1];
#pragma unroll
        for (int k = 0; k <= PP_R; ++k) wl[k] = wts[k];          // uniform: scalar loads, SGPR resident
#pragma unroll 1
        for (int axis = 0; axis < 3; ++axis) {
            const int L = axis == 0 ? nz : axis == 1 ? ny : nx;
            if (axis == 2 && A.rgb_guess && nx == 3) break;
            const int nlines = n / L;
            for (int l = tid; l < nlines; l += WG) {
                int base, stride;
                if (axis == 2) { base = l * px; stride = 1; }
                else {
                    const int t = (int)(((float)l + 0.5f) * inv_nx);
                    const int x = l - t * nx;
                    if (axis == 0) { base = t * px + x; stride = ny * px; }
                    else { base = t * ny * px + x; stride = px; }
                }
                pp_line_pass(tile, base, stride, L, wl);
            }
            __syncthreads();
        }
    }

    // 5. unsharp mask (+ erosion), write out
    const bool erode = flags & MMX_PP_ERODED;
    for (int rb = r0; rb < nrows; rb += PP_NB * rpi) {
        double o[PP_NB];
#pragma unroll
        for (int j = 0; j < PP_NB; ++j) {
            const int row = rb + j * rpi < nrows ? rb + j * rpi : rb;
            const double blur = tile[row * px + x];
            if (A.do_unsharp) {
                const double den = pp_clip(S((double)((int)raw[row * nx + x] - pp_vox<InT>::bias)), A.clip_min, A.clip_max);
                o[j] = pp_unsharp(den, blur, A.strength);
            } else {
                o[j] = blur;
            }
        }
        if (A.do_unsharp && !S.fast) {
            for (int j = 0; j < PP_NB; ++j) {
                const int row = rb + j * rpi < nrows ? rb + j * rpi : rb;
                const double den = pp_clip(S.plain((double)((int)raw[row * nx + x] - pp_vox<InT>::bias)), A.clip_min, A.clip_max);
                o[j] = pp_unsharp(den, tile[row * px + x], A.strength);
            }
        }
#pragma unroll
        for (int j = 0; j < PP_NB; ++j) {
            const int row = rb + j * rpi;
            if (row >= nrows) continue;
            if (erode) tile[row * px + x] = o[j];
            else {
                const int z = (int)(((float)row + 0.5f) * inv_ny);
                const int y = row - z * ny;
                pp_put(out64, out32, sb.dst_off + z * A.dst_sz + y * A.dst_sy + x, o[j]);
            }
        }
    }
    if (!erode) return;
    __syncthreads();
    for (int row = r0; row < nrows; row += rpi) {
        const int z = (int)(((float)row + 0.5f) * inv_ny);
        const int y = row - z * ny;
        const double o = pp_erode7(tile, row * px + x, px, ny * px, x > 0, x < nx - 1, y > 0, y < ny - 1, z > 0, z < nz - 1);
        pp_put(out64, out32, sb.dst_off + z * A.dst_sz + y * A.dst_sy + x, o);
    }
}

// ---- tiles with every side <= 64 that do not fit LDS (finer-than-0.8-um voxels make the stock
// denoise_size 25 um a 33..64-voxel tile): the float64 working copy lives in a global scratch (L2),
// one 256-lane workgroup per tile.  Same register-resident line pass as the LDS kernel (64-register
// lines): z and y lines are read straight from the scratch (lanes along x: coalesced), x lines go
// through an LDS transpose in chunks of PP_MID_ROWS rows.
#define PP_MIDL 64
#define PP_WG_MID 256
#define PP_MID_ROWS 128

template <typename InT>
__global__ void __launch_bounds__(PP_WG_MID)
pp_mid_kernel(const InT* __restrict__ vol, int64_t sz, int64_t sy, int64_t sx,
              const mmx_subblock* __restrict__ subs, const mmx_quantile_class* __restrict__ qcs,
              const double* __restrict__ wts,
              pp_args A, float* __restrict__ out32, double* __restrict__ out64,
              mmx_subblock_info* __restrict__ info, double* __restrict__ scratch)
{
    extern __shared__ double xrows[];              // [PP_MID_ROWS][nx | 1] for the x pass
    __shared__ uint32_t hist[PP_HIST];
    __shared__ pp_ranks s_ranks;
    __shared__ double s_red[PP_WG_MID / 64];
    __shared__ double s_mean;
    __shared__ int s_flags;
    __shared__ pp_stack s_stack;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const mmx_subblock sb = subs[blockIdx.x];
    const int nz = sb.nz, ny = sb.ny, nx = sb.nx;
    const int n = nz * ny * nx;
    const int nrows = nz * ny;
    const InT* src = vol + sb.src_off;
    double* buf = scratch + sb.scratch_off;
    auto raw = [&](int i) {                 // (rare paths only: two integer divisions)
        const int t = i / nx, x = i - t * nx, z = t / ny, y = t - z * ny;
        return (int)src[z * sz + y * sy + x * sx] + pp_vox<InT>::bias;         // (keys, as raw_at)
    };
    // element-wise stages: a lane keeps its x and walks rows (z*ny + y) in steps of rpi, no per-voxel
    // index arithmetic; rows < 4096, so the float reciprocal gives row / ny exactly
    const float inv_nx = 1.0f / (float)nx, inv_ny = 1.0f / (float)ny;
    const int rpi = PP_WG_MID / nx;
    const int r_first = (int)(((float)tid + 0.5f) * inv_nx);
    const int x = tid - r_first * nx;
    const bool lane_on = r_first < rpi;
    auto raw_at = [&](int row) {
        const int z = (int)(((float)row + 0.5f) * inv_ny);
        const int y = row - z * ny;
        return (int)src[z * sz + y * sy + x * sx] + pp_vox<InT>::bias;
    };

    for (int i = tid; i < PP_HIST; i += PP_WG_MID) hist[i] = 0;
    __syncthreads();
    // (8 rows per lane in flight: with 8 waves per CU nothing else hides the load latency)
    for (int rb = 0; rb < nrows; rb += 8 * rpi) {          // same trip count in every lane (ballots)
        int v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int row = rb + j * rpi + r_first;
            v[j] = (lane_on && row < nrows) ? raw_at(row) : 0;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int row = rb + j * rpi + r_first;
            pp_hist_add(hist, v[j] >> 8, lane_on && row < nrows);
        }
    }
    __syncthreads();
    const mmx_quantile_class qc = qcs[sb.qclass];
    pp_select_high(hist, qc, &s_ranks);
    __syncthreads();
    {
        const pp_bins bins(&s_ranks);
        for (int rb = lane_on ? r_first : nrows; rb < nrows; rb += 8 * rpi) {
            int vv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) vv[j] = rb + j * rpi < nrows ? raw_at(rb + j * rpi) : -1;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (vv[j] >= 0) bins.add(hist, vv[j]);
            }
        }
    }
    __syncthreads();
    pp_select_low(hist, &s_ranks);
    __syncthreads();

    const pp_bounds B = pp_key_bounds<InT>(&s_ranks, qc, A.max_thresh);
    const auto S = pp_sat_t<pp_vox<InT>::is_signed>::make(B.vmin, B.vmax, B.identity);

    double part = 0.;
    for (int rb = lane_on ? r_first : nrows; rb < nrows; rb += 8 * rpi) {
        int vv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) vv[j] = rb + j * rpi < nrows ? raw_at(rb + j * rpi) : -1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (vv[j] < 0) continue;
            const double rv = (double)(vv[j] - pp_vox<InT>::bias);
            const double s = S.fast ? S(rv) : S.plain(rv);
            part += s;
            buf[(rb + j * rpi) * nx + x] = pp_clip(s, A.clip_min, A.clip_max);
        }
    }
    part = pp_wave_sum(part);
    if (lane == 0) s_red[wave] = part;
    __syncthreads();
    if (tid == 0) {
        double tot = 0.;
        for (int w = 0; w < PP_WG_MID / 64; ++w) tot += s_red[w];
        double mean = tot / (double)n;
        s_flags = pp_mean_verdict(mean, S.identity, A, [&](double& m) {
            auto val = [&](int i) { return S.plain((double)(raw(i) - pp_vox<InT>::bias)); };
            m = pp_pairwise(val, n, &s_stack) / (double)n;
            return pp_exact_verdict(m, A);
        });
        s_mean = mean;
    }
    __syncthreads();          // also orders the scratch writes above before the passes below
    const int flags = s_flags;
    if (info && tid == 0) pp_write_info(info, blockIdx.x, B.vmin, B.vmax, s_mean, flags);

    if (A.do_unsharp) {
        double wl[PP_R + 1];
#pragma unroll
        for (int k = 0; k <= PP_R; ++k) wl[k] = wts[k];
        // z lines, then y lines: lane <-> (row of the other axis, x), x fastest
#pragma unroll 1
        for (int axis = 0; axis < 2; ++axis) {
            const int L = axis == 0 ? nz : ny;
            const int nlines = n / L;
            for (int l = tid; l < nlines; l += PP_WG_MID) {
                int64_t base, stride;
                if (axis == 0) { base = l; stride = (int64_t)ny * nx; }
                else { const int z = l / nx, x = l - z * nx; base = (int64_t)z * ny * nx + x; stride = nx; }
                pp_line_pass<PP_MIDL>(buf, base, stride, L, wl);
            }
            __syncthreads();
        }
        // x lines through LDS: PP_MID_ROWS rows at a time, odd row pitch
        if (!(A.rgb_guess && nx == 3)) {
            const int pxl = nx | 1;
            for (int row0 = 0; row0 < nrows; row0 += PP_MID_ROWS) {
                const int nr = min(PP_MID_ROWS, nrows - row0);
                for (int i = tid; i < nr * nx; i += PP_WG_MID) {
                    const int r = i / nx, x = i - r * nx;
                    xrows[r * pxl + x] = buf[(int64_t)row0 * nx + i];
                }
                __syncthreads();
                if (tid < nr) pp_line_pass<PP_MIDL>(xrows, (int64_t)tid * pxl, 1, nx, wl);
                __syncthreads();
                for (int i = tid; i < nr * nx; i += PP_WG_MID) {
                    const int r = i / nx, x = i - r * nx;
                    buf[(int64_t)row0 * nx + i] = xrows[r * pxl + x];
                }
                __syncthreads();
            }
        }
    }

    const bool erode = flags & MMX_PP_ERODED;
    for (int rb = lane_on ? r_first : nrows; rb < nrows; rb += 8 * rpi) {
      int vv[8];
      double bl8[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
          const int row = rb + j * rpi;
          vv[j] = row < nrows ? (A.do_unsharp ? raw_at(row) : 0) : -1;
          bl8[j] = row < nrows ? buf[row * nx + x] : 0.;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (vv[j] < 0) continue;
        const int row = rb + j * rpi;
        const int z = (int)(((float)row + 0.5f) * inv_ny);
        const int y = row - z * ny;
        const int i = row * nx + x;
        double o;
        if (A.do_unsharp) {
            const double rv = (double)(vv[j] - pp_vox<InT>::bias);
            const double sv = S.fast ? S(rv) : S.plain(rv);
            o = pp_unsharp(pp_clip(sv, A.clip_min, A.clip_max), bl8[j], A.strength);
        } else {
            o = bl8[j];
        }
        if (erode) buf[i] = o;
        else pp_put(out64, out32, sb.dst_off + z * A.dst_sz + y * A.dst_sy + x, o);
      }
    }
    if (!erode) return;
    __syncthreads();
    for (int row = lane_on ? r_first : nrows; row < nrows; row += rpi) {
        const int z = (int)(((float)row + 0.5f) * inv_ny);
        const int y = row - z * ny;
        const double o = pp_erode7(buf, row * nx + x, nx, ny * nx, x > 0, x < nx - 1, y > 0, y < ny - 1, z > 0, z < nz - 1);
        pp_put(out64, out32, sb.dst_off + z * A.dst_sz + y * A.dst_sy + x, o);
    }
}

// ---- any extent: data in a global scratch (2 * n doubles per sub-block), one output per lane and pass
template <typename InT>
__global__ void __launch_bounds__(PP_WG_GENERIC)
pp_generic_kernel(const InT* __restrict__ vol, int64_t sz, int64_t sy, int64_t sx,
                  const mmx_subblock* __restrict__ subs, const mmx_quantile_class* __restrict__ qcs,
                  const double* __restrict__ wts,
                  pp_args A, float* __restrict__ out32, double* __restrict__ out64,
                  mmx_subblock_info* __restrict__ info, double* __restrict__ scratch)
{
    __shared__ uint32_t hist[PP_HIST];
    __shared__ pp_ranks s_ranks;
    __shared__ double s_red[PP_WG_GENERIC / 64];
    __shared__ double s_mean;
    __shared__ int s_flags;
    __shared__ pp_stack s_stack;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const mmx_subblock sb = subs[blockIdx.x];
    const int64_t nz = sb.nz, ny = sb.ny, nx = sb.nx, n = nz * ny * nx;
    const InT* src = vol + sb.src_off;
    double* bufA = scratch + sb.scratch_off;
    double* bufB = bufA + n;
    constexpr bool F32 = std::is_same<InT, float>::value;
    constexpr bool FLT = std::is_same<InT, double>::value || F32;      // float voxels: the select on the values' keys
    auto raw = [&](int64_t i) {
        const int64_t t = i / nx, x = i - t * nx, z = t / ny, y = t - z * ny;
        if constexpr (FLT) return (double)src[z * sz + y * sy + x * sx];
        else return (int)src[z * sz + y * sy + x * sx];
    };
    const mmx_quantile_class qc = qcs[sb.qclass];
    pp_bounds B;
    if constexpr (FLT) {
        // float64 voxels: an eight-level radix select on the order-preserving key of the doubles (mmx_key; no NaNs on
        // this path), the four ranks side by side -- one 256-bin histogram each per level, counted over the voxels
        // that share the rank's prefix so far.  float32 voxels: the same over the four bytes of the float's key (the
        // working copy holds the floats widened, so the narrowing is exact)
        __shared__ unsigned long long s_pre[4];
        constexpr int top = mmx_key<InT>::levels - 1;
        auto key = [](double v) {
            if constexpr (F32) return (unsigned long long)mmx_key<float>::flip(__float_as_uint((float)v + 0.0f));
            else return mmx_key<double>::flip((unsigned long long)__double_as_longlong(v + 0.0));     // (-0.0 sorts as +0.0)
        };
        for (int64_t i = tid; i < n; i += PP_WG_GENERIC) bufA[i] = raw(i);
        if (tid < 4) {
            s_pre[tid] = 0ull;
            s_ranks.res[tid] = tid == 0 ? qc.lo_prev : tid == 1 ? qc.lo_next : tid == 2 ? qc.hi_prev : qc.hi_next;
        }
        __syncthreads();
        for (int level = top; level >= 0; --level) {
            for (int i = tid; i < PP_HIST; i += PP_WG_GENERIC) hist[i] = 0;
            __syncthreads();
            const unsigned long long p0 = s_pre[0], p1 = s_pre[1], p2 = s_pre[2], p3 = s_pre[3];
            const int sh = 8 * level;
            for (int64_t i = tid; i < n; i += PP_WG_GENERIC) {
                const unsigned long long k = key(bufA[i]);
                const unsigned long long up = level == top ? 0ull : k >> (sh + 8);
                const unsigned b8 = (unsigned)(k >> sh) & 255u;
                if (up == p0) atomicAdd(&hist[256 + b8], 1u);
                if (up == p1) atomicAdd(&hist[512 + b8], 1u);
                if (up == p2) atomicAdd(&hist[768 + b8], 1u);
                if (up == p3) atomicAdd(&hist[1024 + b8], 1u);
            }
            __syncthreads();
            if (wave < 4) {
                int b; uint32_t r;
                pp_select(hist + 256 * (1 + wave), s_ranks.res[wave], b, r);
                if (lane == 0) { s_pre[wave] = (s_pre[wave] << 8) | (unsigned long long)b; s_ranks.res[wave] = r; }
            }
            __syncthreads();
        }
        // (the lerp of the type: float32 order statistics take their difference in float32)
        auto q = [&](int w) { return (InT)mmx_key<InT>::value(s_pre[w]); };
        B = pp_make_bounds(pp_lerp(q(0), q(1), qc.lo_gamma), pp_lerp(q(2), q(3), qc.hi_gamma), A.max_thresh);
    } else {
        for (int i = tid; i < PP_HIST; i += PP_WG_GENERIC) hist[i] = 0;
        __syncthreads();
        for (int64_t i = tid; i < n; i += PP_WG_GENERIC) {
            const int v = raw(i);
            bufA[i] = (double)v;
            atomicAdd(&hist[(v + pp_vox<InT>::bias) >> 8], 1u);
        }
        __syncthreads();
        pp_select_high(hist, qc, &s_ranks);
        __syncthreads();
        {
            const pp_bins bins(&s_ranks);
            for (int64_t i = tid; i < n; i += PP_WG_GENERIC) bins.add(hist, (int)bufA[i] + pp_vox<InT>::bias);
        }
        __syncthreads();
        pp_select_low(hist, &s_ranks);
        __syncthreads();
        B = pp_key_bounds<InT>(&s_ranks, qc, A.max_thresh);
    }
    const auto S = pp_sat_t<pp_vox<InT>::is_signed>::make(B.vmin, B.vmax, B.identity);

    // (an identity tile -- vmin == vmax: the reference leaves the voxels alone -- of a float64 image may hold negative
    //  values, which the vmin = 0 stand-in of pp_sat_t would clip)
    auto sat = [&](double v) { return (FLT && S.identity) ? v : S.plain(v); };
    // an identity tile of a float32 image stays float32 through denoise_roi (pp_clip32, pp_round32, pp_unsharp32)
    const bool id32 = F32 && S.identity;
    auto clip = [&](double s) { return id32 ? pp_clip32(s, A.clip_min, A.clip_max) : pp_clip(s, A.clip_min, A.clip_max); };
    double part = 0.;
    for (int64_t i = tid; i < n; i += PP_WG_GENERIC) {
        const double s = sat(bufA[i]);
        part += s;
        bufA[i] = clip(s);
    }
    part = pp_wave_sum(part);
    if (lane == 0) s_red[wave] = part;
    __syncthreads();
    if (tid == 0) {
        double tot = 0.;
        for (int w = 0; w < PP_WG_GENERIC / 64; ++w) tot += s_red[w];
        double mean = tot / (double)n;
        s_flags = pp_mean_verdict(mean, S.identity, A, [&](double& m) {
            if (n >= (1ll << 31)) return m > A.ero_thr ? MMX_PP_ERODED : 0;      // (pp_pairwise indexes with int: the parallel sum stands)
            auto val = [&](int i) { return sat((double)raw(i)); };
            m = pp_pairwise(val, (int)n, &s_stack) / (double)n;
            return pp_exact_verdict(m, A);
        });
        s_mean = mean;
    }
    __syncthreads();
    const int flags = s_flags;
    if (info && tid == 0) pp_write_info(info, blockIdx.x, B.vmin, B.vmax, s_mean, flags);

    // ---- total-variation denoising of the clipped tile (reference plot_3d.py:147-149 ->
    // skimage.restoration.denoise_tv_chambolle, restoration/_denoise.py:315-393): Chambolle's projection
    // iteration on the dual field p, every voxel operation and both energy sums (NumPy pairwise order) as
    // NumPy does them, so that the iteration stops where the reference's stops and returns the same bits.
    const bool tv = A.tv_weight != 0.0;
    double* p0 = bufB + n;
    if (tv) {
        __shared__ pp_leaves s_leaves;
        __shared__ int s_done;
        __shared__ double s_e[2];                         // E_init, E_previous
        double* img = bufA;
        double* outb = bufB;
        double* p1 = p0 + n;
        double* p2 = p1 + n;
        double* sq = p2 + n;                              // d^2, then the gradient norms
        double* nm = sq + n;
        const int64_t pl = ny * nx;
        const double tau = 1.0 / 6.0;                     // 1 / (2 * ndim)
        for (int64_t i = tid; i < n; i += PP_WG_GENERIC) { p0[i] = 0.0; p1[i] = 0.0; p2[i] = 0.0; }
        if (tid == 0) { pp_enum_leaves((int)n, &s_stack, &s_leaves); s_done = 0; }
        __syncthreads();
        const bool par = s_leaves.count <= PP_MAXLEAF;
#pragma unroll 1
        for (int it = 0; it < 200; ++it) {
            for (int64_t i = tid; i < n; i += PP_WG_GENERIC) {
                const int64_t t = i / nx, x = i - t * nx, z = t / ny, y = t - z * ny;
                double d = 0.0;
                if (it > 0) {
                    d = -((p0[i] + p1[i]) + p2[i]);               // -p.sum(0)
                    if (z > 0) d += p0[i - pl];
                    if (y > 0) d += p1[i - nx];
                    if (x > 0) d += p2[i - 1];
                }
                outb[i] = it > 0 ? img[i] + d : img[i];
                sq[i] = d * d;
            }
            __syncthreads();
            for (int64_t i = tid; i < n; i += PP_WG_GENERIC) {
                const int64_t t = i / nx, x = i - t * nx, z = t / ny, y = t - z * ny;
                const double o = outb[i];
                const double g0 = z < nz - 1 ? outb[i + pl] - o : 0.0;
                const double g1 = y < ny - 1 ? outb[i + nx] - o : 0.0;
                const double g2 = x < nx - 1 ? outb[i + 1] - o : 0.0;
                double nrm = sqrt((g0 * g0 + g1 * g1) + g2 * g2);
                nm[i] = nrm;
                nrm = nrm * A.tv_factor;
                nrm = nrm + 1.0;
                p0[i] = (p0[i] - tau * g0) / nrm;
                p1[i] = (p1[i] - tau * g1) / nrm;
                p2[i] = (p2[i] - tau * g2) / nrm;
            }
            __syncthreads();
            if (par) {
                const int nl = s_leaves.count;
                for (int k = tid; k < 2 * nl; k += PP_WG_GENERIC) {
                    const int w = k >= nl, l = w ? k - nl : k;
                    const double* a = w ? nm : sq;
                    auto val = [&](int i) { return a[i]; };
                    s_leaves.sum[w][l] = pp_pairwise_leaf(val, s_leaves.lo[l], s_leaves.n[l]);
                }
                __syncthreads();
            }
            if (tid == 0) {
                double e1, e2;
                if (par) { e1 = pp_fold_leaves((int)n, &s_stack, &s_leaves, 0); e2 = pp_fold_leaves((int)n, &s_stack, &s_leaves, 1); }
                else {
                    auto v1 = [&](int i) { return sq[i]; };
                    auto v2 = [&](int i) { return nm[i]; };
                    e1 = pp_pairwise(v1, (int)n, &s_stack);
                    e2 = pp_pairwise(v2, (int)n, &s_stack);
                }
                double E = e1;
                E = E + A.tv_weight * e2;
                E = E / (double)n;
                if (it == 0) { s_e[0] = E; s_e[1] = E; }
                else if (fabs(s_e[1] - E) < 2.e-4 * s_e[0]) s_done = 1;
                else s_e[1] = E;
            }
            __syncthreads();
            if (s_done) break;
        }
    }

    // buffers from here on: `cur` = blur input / result, t1 / t2 = the blur's ping-pong pair, `den_buf` = the
    // denoised tile the unsharp mask adds to (recomputed from the voxels without total-variation denoising)
    const double* den_buf = tv ? bufB : nullptr;
    double* cur = tv ? bufB : bufA;
    double* const t1 = tv ? p0 : bufB;
    double* const t2 = tv ? p0 + n : bufA;
    double* oth = tv ? p0 + 2 * n : bufB;
    if (A.do_unsharp) {
        int pass = 0;
#pragma unroll 1
        for (int axis = 0; axis < 3; ++axis) {
            if (axis == 2 && A.rgb_guess && nx == 3) break;
            double* const dstb = (pass & 1) ? t2 : t1;
            const int64_t L = axis == 0 ? nz : axis == 1 ? ny : nx;
            const int64_t stride = axis == 0 ? ny * nx : axis == 1 ? nx : 1;
            for (int64_t i = tid; i < n; i += PP_WG_GENERIC) {
                const int64_t c = (i / stride) % L;
                const double* line = cur + (i - c * stride);
                double acc = line[c * stride] * wts[0];
                for (int k = PP_R; k >= 1; --k) {
                    const int64_t a = c - k < 0 ? 0 : c - k;
                    const int64_t b = c + k > L - 1 ? L - 1 : c + k;
                    acc += (line[a * stride] + line[b * stride]) * wts[k];
                }
                dstb[i] = id32 ? pp_round32(acc) : acc;
            }
            __syncthreads();
            cur = dstb;
            ++pass;
        }
        if (!tv) oth = cur == bufA ? bufB : bufA;
    }

    const bool erode = flags & MMX_PP_ERODED;
    for (int64_t i = tid; i < n; i += PP_WG_GENERIC) {
        const int64_t t = i / nx, x = i - t * nx, z = t / ny, y = t - z * ny;
        double o;
        if (A.do_unsharp) {
            const double den = tv ? den_buf[i] : clip(sat((double)raw(i)));
            o = id32 ? pp_unsharp32(den, cur[i], A.strength) : pp_unsharp(den, cur[i], A.strength);
        } else {
            o = cur[i];
        }
        if (erode) oth[i] = o;
        else pp_put(out64, out32, sb.dst_off + z * A.dst_sz + y * A.dst_sy + x, o);
    }
    if (!erode) return;
    __syncthreads();
    for (int64_t i = tid; i < n; i += PP_WG_GENERIC) {
        const int64_t t = i / nx, x = i - t * nx, z = t / ny, y = t - z * ny;
        const double o = pp_erode7(oth, i, nx, ny * nx, x > 0, x < nx - 1, y > 0, y < ny - 1, z > 0, z < nz - 1);
        pp_put(out64, out32, sb.dst_off + z * A.dst_sz + y * A.dst_sy + x, o);
    }
}

// ---- float32 voxels (NumPy 2's rules, pp_generic_kernel), tiles with every side <= MAXL: the register-line forms.
//   LDS = true   the working copy is the float64 tile in LDS, as in pp_fast_kernel: the stock 25^3 tile's 122 KiB.  A
//                32-bit copy of the voxels does not fit beside it (pp_fast_kernel keeps a 16-bit one), so it is organised
//                differently: the raw values sit in the tile itself through the four-level select, and the unsharp stage
//                (and a knife-edge mean) read the voxels from the image again -- the second read of a tile a workgroup
//                has just streamed, an L2 hit.  Every mode of mmx_preprocess_batch_mode runs this one kernel for float32.
//   LDS = false  the working copy is the tile's global scratch (pp_mid_kernel's tiles: sides up to 64), lines straight
//                from the scratch.
// Arithmetic: pp_generic_kernel<float>'s, statement by statement (plain division, pp_clip32 / pp_round32 / pp_unsharp32
// on an identity tile), with the blur as pp_line_pass; the sum behind the mean is taken in another order, which the
// knife-edge replay in NumPy's order makes immaterial (an identity tile has none, as everywhere).
template <int WG, int MAXL, bool LDS>
__global__ void __launch_bounds__(WG)
pp_f32_kernel(const float* __restrict__ vol, int64_t sz, int64_t sy, int64_t sx,
              const mmx_subblock* __restrict__ subs, int n_subs,
              const mmx_quantile_class* __restrict__ qcs, const double* __restrict__ wts,
              pp_args A, float* __restrict__ out32, double* __restrict__ out64,
              mmx_subblock_info* __restrict__ info, double* __restrict__ scratch)
{
    extern __shared__ double tile_lds[];
    __shared__ uint32_t hist[PP_HIST];
    __shared__ unsigned long long s_pre[4];
    __shared__ pp_ranks s_ranks;
    __shared__ double s_red[WG / 64];
    __shared__ double s_mean;
    __shared__ int s_flags;
    __shared__ pp_stack s_stack;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int sub_id = blockIdx.x;
    if (LDS) {                                    // (8 XCD-contiguous runs of tiles, as pp_fast_kernel)
        const int per = (n_subs + 7) >> 3;
        sub_id = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    }
    if (sub_id >= n_subs) return;
    const mmx_subblock sb = subs[sub_id];
    const int nz = sb.nz, ny = sb.ny, nx = sb.nx, n = nz * ny * nx, nrows = nz * ny;
    const int px = LDS ? (nx | 1) : nx;
    double* __restrict__ t = LDS ? tile_lds : scratch + sb.scratch_off;
    const float* src = vol + sb.src_off;
    const float inv_nx = 1.0f / (float)nx, inv_ny = 1.0f / (float)ny;
    // a lane keeps its x and walks rows (z * ny + y) in steps of rpi (rows < 4096: the float reciprocals are exact)
    const int rpi = WG / nx;
    const int r_first = (int)(((float)tid + 0.5f) * inv_nx);
    const int x = tid - r_first * nx;
    const int r0 = r_first < rpi ? r_first : nrows;
    auto raw_at = [&](int row) {
        const int z = (int)(((float)row + 0.5f) * inv_ny);
        const int y = row - z * ny;
        return (double)src[z * sz + y * sy + x * sx];
    };

    // 1. voxels -> the working copy, widened
    for (int row = r0; row < nrows; row += rpi) t[row * px + x] = raw_at(row);
    if (tid < 4) {
        const mmx_quantile_class q0 = qcs[sb.qclass];
        s_pre[tid] = 0ull;
        s_ranks.res[tid] = tid == 0 ? q0.lo_prev : tid == 1 ? q0.lo_next : tid == 2 ? q0.hi_prev : q0.hi_next;
    }
    __syncthreads();

    // 2. the four order statistics: a four-level radix select on the floats' keys (-0.0 sorts as +0.0), the four ranks
    //    side by side
    const mmx_quantile_class qc = qcs[sb.qclass];
    for (int level = 3; level >= 0; --level) {
        for (int i = tid; i < PP_HIST; i += WG) hist[i] = 0;
        __syncthreads();
        const uint32_t p0 = (uint32_t)s_pre[0], p1 = (uint32_t)s_pre[1], p2 = (uint32_t)s_pre[2], p3 = (uint32_t)s_pre[3];
        const int sh = 8 * level;
        for (int row = r0; row < nrows; row += rpi) {
            const uint32_t k = mmx_key<float>::flip(__float_as_uint((float)t[row * px + x] + 0.0f));
            const uint32_t up = level == 3 ? 0u : k >> (sh + 8);
            const unsigned b8 = (k >> sh) & 255u;
            if (up == p0) atomicAdd(&hist[256 + b8], 1u);
            if (up == p1) atomicAdd(&hist[512 + b8], 1u);
            if (up == p2) atomicAdd(&hist[768 + b8], 1u);
            if (up == p3) atomicAdd(&hist[1024 + b8], 1u);
        }
        __syncthreads();
        if (wave < 4) {
            int b; uint32_t r;
            pp_select(hist + 256 * (1 + wave), s_ranks.res[wave], b, r);
            if (lane == 0) { s_pre[wave] = (s_pre[wave] << 8) | (unsigned long long)b; s_ranks.res[wave] = r; }
        }
        __syncthreads();
    }
    auto q = [&](int w) { return (float)mmx_key<float>::value(s_pre[w]); };
    const pp_bounds B = pp_make_bounds(pp_lerp(q(0), q(1), qc.lo_gamma), pp_lerp(q(2), q(3), qc.hi_gamma), A.max_thresh);
    const auto S = pp_sat_t<false>::make(B.vmin, B.vmax, B.identity);
    const bool id32 = S.identity;                       // the tile stays float32 through denoise_roi
    auto sat = [&](double v) { return id32 ? v : S.plain(v); };
    auto clip = [&](double s) { return id32 ? pp_clip32(s, A.clip_min, A.clip_max) : pp_clip(s, A.clip_min, A.clip_max); };

    // 3. saturate, sum, clip in place
    double part = 0.;
    for (int row = r0; row < nrows; row += rpi) {
        const double s = sat(t[row * px + x]);
        part += s;
        t[row * px + x] = clip(s);
    }
    part = pp_wave_sum(part);
    if (lane == 0) s_red[wave] = part;
    __syncthreads();
    if (tid == 0) {
        double tot = 0.;
        for (int w = 0; w < WG / 64; ++w) tot += s_red[w];
        double mean = tot / (double)n;
        s_flags = pp_mean_verdict(mean, S.identity, A, [&](double& m) {
            auto val = [&](int i) {
                const int tt = i / nx, xx = i - tt * nx, z = tt / ny, y = tt - z * ny;
                return sat((double)src[z * sz + y * sy + xx * sx]);
            };
            m = pp_pairwise(val, n, &s_stack) / (double)n;
            return pp_exact_verdict(m, A);
        });
        s_mean = mean;
    }
    __syncthreads();
    const int flags = s_flags;
    if (info && tid == 0) pp_write_info(info, sub_id, B.vmin, B.vmax, s_mean, flags);

    // 4. Gaussian blur, axis 0, 1, 2 in place; an identity tile stores float32 after every axis pass
    if (A.do_unsharp) {
        double wl[PP_R + 1];
#pragma unroll
        for (int k = 0; k <= PP_R; ++k) wl[k] = wts[k];
#pragma unroll 1
        for (int axis = 0; axis < 3; ++axis) {
            const int L = axis == 0 ? nz : axis == 1 ? ny : nx;
            if (axis == 2 && A.rgb_guess && nx == 3) break;
            const int nlines = n / L;
            for (int l = tid; l < nlines; l += WG) {
                int base, stride;
                if (axis == 2) { base = l * px; stride = 1; }
                else {
                    const int tt = (int)(((float)l + 0.5f) * inv_nx);
                    const int xx = l - tt * nx;
                    if (axis == 0) { base = tt * px + xx; stride = ny * px; }
                    else { base = tt * ny * px + xx; stride = px; }
                }
                pp_line_pass<MAXL>(t, base, stride, L, wl);
            }
            __syncthreads();
            if (id32) {
                for (int row = r0; row < nrows; row += rpi) t[row * px + x] = pp_round32(t[row * px + x]);
                __syncthreads();
            }
        }
    }

    // 5. unsharp mask on the voxels read again (+ erosion), write out
    const bool erode = flags & MMX_PP_ERODED;
    for (int row = r0; row < nrows; row += rpi) {
        double o = t[row * px + x];
        if (A.do_unsharp) {
            const double den = clip(sat(raw_at(row)));
            o = id32 ? pp_unsharp32(den, o, A.strength) : pp_unsharp(den, o, A.strength);
        }
        if (erode) t[row * px + x] = o;
        else {
            const int z = (int)(((float)row + 0.5f) * inv_ny);
            const int y = row - z * ny;
            pp_put(out64, out32, sb.dst_off + z * A.dst_sz + y * A.dst_sy + x, o);
        }
    }
    if (!erode) return;
    __syncthreads();
    for (int row = r0; row < nrows; row += rpi) {
        const int z = (int)(((float)row + 0.5f) * inv_ny);
        const int y = row - z * ny;
        const double o = pp_erode7(t, row * px + x, px, ny * px, x > 0, x < nx - 1, y > 0, y < ny - 1, z > 0, z < nz - 1);
        pp_put(out64, out32, sb.dst_off + z * A.dst_sz + y * A.dst_sy + x, o);
    }
}

// ---- float32 images: the dtype of the reference's merged block.  Its tile loop allocates the block from the FIRST
// tile's dtype (stack_detect.py: merged = np.zeros(shape, dtype=piece.dtype)): an identity first tile makes a float32
// block, into which every float64 piece is rounded.  Tiles run in different workgroups, so this pass follows them: it
// reads the first tile's record, states the block's flag and rounds out64 of a flagged block in place (out32 already
// is that rounding; a float32 piece of a float64 block widened exactly when it was stored).
__global__ void __launch_bounds__(256)
pp_block_dtype_kernel(const mmx_block* __restrict__ blocks, const int32_t* __restrict__ first_tile,
                      const mmx_subblock_info* __restrict__ info, int64_t dst_sy, int64_t dst_sz,
                      double* __restrict__ out64, int32_t* __restrict__ flags)
{
    const mmx_block b = blocks[blockIdx.y];
    const int f32 = (info[first_tile[blockIdx.y]].flags & MMX_PP_IDENTITY) ? 1 : 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) flags[blockIdx.y] = f32;
    if (!f32) return;
    const int64_t rows = (int64_t)b.nz * b.ny;
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const int64_t z = r / b.ny, y = r - z * b.ny;
        double* row = out64 + b.src_off + z * dst_sz + y * dst_sy;
        for (int x = threadIdx.x; x < b.nx; x += 256) row[x] = pp_round32(row[x]);
    }
}

}  // namespace

extern "C" {

int64_t mmx_preprocess_fast_lds(int nz, int ny, int nx)
{
    if (nz < 1 || ny < 1 || nx < 1 || nz > PP_MAXL || ny > PP_MAXL || nx > PP_MAXL) return 0;
    const int64_t n = (int64_t)nz * ny * nx;
    const int64_t b = (int64_t)nz * ny * (nx | 1) * (int64_t)sizeof(double) + PP_HIST * (int64_t)sizeof(uint32_t)
                      + ((n * 2 + 7) & ~7ll);      // float64 tile, histograms, the uint16 voxels
    return b <= MMX_PP_MAX_LDS - 1024 ? b : 0;     // < 1 KiB of static LDS (selection, recursion stack)
}

static int pp_check(const mmx_volume* vol, const mmx_subblock* d_subs, const mmx_subblock* h_subs, int n_subs,
                    const mmx_quantile_class* d_qc, int n_qc, const mmx_preproc_params* p, const double* h_w,
                    float* d_out32, double* d_out64)
{
    if (!vol || !vol->d_data || !d_subs || !h_subs || n_subs < 0 || !d_qc || n_qc < 1 || !p || !h_w ||
        !d_out32 || !d_out64)
        return MMX_ERR_ARG;
    if (p->radius != PP_R) return MMX_ERR_UNSUPPORTED;
    // (float64 and float32 images: the one-output-per-lane kernel of the generic entry only; float32 images under the
    //  casting rules of NumPy 2, which the caller opts into -- mmx_voxel.h)
    if (!mmx_voxel_in(vol->dtype, MMX_VOX_PREPROC)) return MMX_ERR_UNSUPPORTED;
    for (int i = 0; i < n_subs; ++i) {
        const mmx_subblock& b = h_subs[i];
        if (b.nz < 1 || b.ny < 1 || b.nx < 1 || b.qclass < 0 || b.qclass >= n_qc || b.src_off < 0 || b.dst_off < 0)
            return MMX_ERR_ARG;
    }
    return MMX_OK;
}

int64_t mmx_preprocess_work_bytes(const mmx_subblock* h_subs, int n_subs)
{
    if (!h_subs || n_subs < 0) return 0;
    return mmx_pp_pipe_work_bytes(h_subs, n_subs);
}

int mmx_preprocess_batch_mode(const mmx_volume* vol, const mmx_subblock* d_subs, const mmx_subblock* h_subs,
                              int n_subs, const mmx_quantile_class* d_qclasses, int n_qclasses,
                              const mmx_preproc_params* params, const double* d_weights,
                              int64_t dst_sy, int64_t dst_sz, float* d_out32, double* d_out64,
                              mmx_subblock_info* d_info, int mode, int tiles_per_wg,
                              void* d_work, int64_t work_bytes, void* stream)
{
    const int st = pp_check(vol, d_subs, h_subs, n_subs, d_qclasses, n_qclasses, params, d_weights, d_out32, d_out64);
    if (st != MMX_OK) return st;
    if (mode != MMX_PP_AUTO && mode != MMX_PP_SINGLE && mode != MMX_PP_PIPELINED) return MMX_ERR_ARG;
    if (params->tv_weight != 0.0) return MMX_ERR_UNSUPPORTED;      // total-variation denoising: the generic entry
    // (float64 voxels: the generic entry; float32 voxels: one LDS kernel of their own, whatever the mode)
    if (!mmx_voxel_in(vol->dtype, MMX_VOX_INTEGER) && vol->dtype != MMX_F32) return MMX_ERR_UNSUPPORTED;
    if (n_subs == 0) return MMX_OK;
    int64_t lds = 0;
    for (int i = 0; i < n_subs; ++i) {
        const int64_t b = mmx_preprocess_fast_lds(h_subs[i].nz, h_subs[i].ny, h_subs[i].nx);
        if (!b) return MMX_ERR_UNSUPPORTED;
        lds = b > lds ? b : lds;
    }
    const pp_args A = pp_make_args(params, dst_sy, dst_sz);
    hipStream_t s = (hipStream_t)stream;
    const int grid = ((n_subs + 7) / 8) * 8;       // 8 XCD-contiguous runs of tiles
    // small tiles (anisotropic voxels: 25 um is 4 x 23 x 23 voxels at 6.6 x 1.1 x 1.1 um): 256-lane
    // workgroups, so that LDS (not the 32-wave limit) decides how many tiles a CU works on at once
    int64_t max_vox = 0;
    for (int i = 0; i < n_subs; ++i)
        max_vox = std::max<int64_t>(max_vox, (int64_t)h_subs[i].nz * h_subs[i].ny * h_subs[i].nx);
    const bool small = max_vox <= 4096;
    mmx_timed_scope ts(MMX_K_PREPROC, s);
    if (vol->dtype == MMX_F32) {
        int64_t tile_bytes = 0;
        for (int i = 0; i < n_subs; ++i)
            tile_bytes = std::max<int64_t>(tile_bytes, (int64_t)h_subs[i].nz * h_subs[i].ny * (h_subs[i].nx | 1) * (int64_t)sizeof(double));
        auto launch = [&](auto k, int wg) {
            if (hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_bytes) != hipSuccess)
                return MMX_ERR_HIP;
            hipLaunchKernelGGL(k, dim3(grid), dim3(wg), (size_t)tile_bytes, s, (const float*)vol->d_data, vol->stride_z,
                               vol->stride_y, vol->stride_x, d_subs, n_subs, d_qclasses, d_weights, A,
                               d_out32, d_out64, d_info, (double*)nullptr);
            return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
        };
        return small ? launch(pp_f32_kernel<256, PP_MAXL, true>, 256) : launch(pp_f32_kernel<PP_WG, PP_MAXL, true>, PP_WG);
    }
    // tiles that fill a CU's LDS one at a time: statistics kernel + pipelined blur kernel (mmx_preproc_pipe.hip)
    if (mode == MMX_PP_PIPELINED || (mode == MMX_PP_AUTO && !small)) {
        const int64_t need = mmx_pp_pipe_work_bytes(h_subs, n_subs);
        if (d_work && work_bytes < need) return MMX_ERR_WORKSPACE;
        // (callers of the plain entry bring neither: both come from the stream's memory pool for the call)
        mmx_subblock_info* inf = d_info;
        void* work = d_work;
        if (!inf && hipMallocAsync((void**)&inf, (size_t)n_subs * sizeof(mmx_subblock_info), s) != hipSuccess)
            return MMX_ERR_HIP;
        if (!work && hipMallocAsync(&work, (size_t)need, s) != hipSuccess) {
            if (!d_info) (void)hipFreeAsync(inf, s);       // (the table just taken from the pool goes back)
            return MMX_ERR_HIP;
        }
        const int rc = mmx_launch_pp_pipe(vol, d_subs, h_subs, n_subs, d_qclasses, d_weights, A, d_out32, d_out64,
                                          inf, work, tiles_per_wg > 0 ? tiles_per_wg : MMX_PP_TILES_PER_WG, s);
        // (both are returned whatever the first one's status: a failed free must not strand the other block)
        const bool freed_inf = d_info || hipFreeAsync(inf, s) == hipSuccess;
        const bool freed_work = d_work || hipFreeAsync(work, s) == hipSuccess;
        if (!freed_inf || !freed_work) return MMX_ERR_HIP;
        if (rc != MMX_ERR_UNSUPPORTED || mode == MMX_PP_PIPELINED) return rc;
    }
    return mmx_for_voxel<MMX_VOX_INTEGER>(vol->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
        using T = MMX_TAG_T(t);
        auto launch = [&](auto k, int wg) {
            if (hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
                return MMX_ERR_HIP;
            hipLaunchKernelGGL(k, dim3(grid), dim3(wg), (size_t)lds, s, (const T*)vol->d_data, vol->stride_z,
                               vol->stride_y, vol->stride_x, d_subs, n_subs, d_qclasses, d_weights, A,
                               d_out32, d_out64, d_info);
            return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
        };
        return small ? launch(pp_fast_kernel<T, 256>, 256) : launch(pp_fast_kernel<T, PP_WG>, PP_WG);
    });
}

int mmx_preprocess_batch(const mmx_volume* vol, const mmx_subblock* d_subs, const mmx_subblock* h_subs,
                         int n_subs, const mmx_quantile_class* d_qclasses, int n_qclasses,
                         const mmx_preproc_params* params, const double* d_weights,
                         int64_t dst_sy, int64_t dst_sz, float* d_out32, double* d_out64,
                         mmx_subblock_info* d_info, void* stream)
{
    return mmx_preprocess_batch_mode(vol, d_subs, h_subs, n_subs, d_qclasses, n_qclasses, params, d_weights,
                                     dst_sy, dst_sz, d_out32, d_out64, d_info, MMX_PP_AUTO, 0, nullptr, 0, stream);
}

int mmx_preprocess_batch_generic(const mmx_volume* vol, const mmx_subblock* d_subs,
                                 const mmx_subblock* h_subs, int n_subs,
                                 const mmx_quantile_class* d_qclasses, int n_qclasses,
                                 const mmx_preproc_params* params, const double* d_weights,
                                 int64_t dst_sy, int64_t dst_sz, float* d_out32, double* d_out64,
                                 mmx_subblock_info* d_info, double* d_scratch, int64_t scratch_doubles,
                                 void* stream)
{
    const int st = pp_check(vol, d_subs, h_subs, n_subs, d_qclasses, n_qclasses, params, d_weights, d_out32, d_out64);
    if (st != MMX_OK) return st;
    if (n_subs == 0) return MMX_OK;
    if (!d_scratch) return MMX_ERR_ARG;
    // (total-variation denoising of a float32 identity tile would iterate in float32: not built)
    if (params->tv_weight != 0.0 && vol->dtype == MMX_F32) return MMX_ERR_UNSUPPORTED;
    for (int i = 0; i < n_subs; ++i) {
        const mmx_subblock& b = h_subs[i];
        const int64_t n = (int64_t)b.nz * b.ny * b.nx;
        const int64_t per_voxel = params->tv_weight != 0.0 ? PP_TV_SCRATCH : 2;
        if (b.scratch_off < 0 || b.scratch_off + per_voxel * n > scratch_doubles) return MMX_ERR_WORKSPACE;
        if (params->tv_weight != 0.0 && n >= (1ll << 31)) return MMX_ERR_UNSUPPORTED;
    }
    const pp_args A = pp_make_args(params, dst_sy, dst_sz);
    hipStream_t s = (hipStream_t)stream;
    mmx_timed_scope ts(MMX_K_PREPROC, s);
    // every side <= 64: register-resident lines over the scratch (pp_mid_kernel); else one output per lane
    // (the iteration, and float64 voxels, live in the one-output-per-lane kernel only)
    bool mid = params->tv_weight == 0.0 && (mmx_voxel_in(vol->dtype, MMX_VOX_INTEGER) || vol->dtype == MMX_F32);
    int max_nx = 1;
    for (int i = 0; i < n_subs; ++i) {
        const mmx_subblock& b = h_subs[i];
        if (b.nz > PP_MIDL || b.ny > PP_MIDL || b.nx > PP_MIDL || (int64_t)b.nz * b.ny * b.nx >= (1ll << 30)) mid = false;
        max_nx = b.nx > max_nx ? b.nx : max_nx;
    }
    if (mid && vol->dtype == MMX_F32) {
        hipLaunchKernelGGL((pp_f32_kernel<PP_WG_MID, PP_MIDL, false>), dim3(n_subs), dim3(PP_WG_MID), 0, s,
                           (const float*)vol->d_data, vol->stride_z, vol->stride_y, vol->stride_x, d_subs, n_subs,
                           d_qclasses, d_weights, A, d_out32, d_out64, d_info, d_scratch);
        return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
    }
    if (mid) {
        const size_t lds = (size_t)PP_MID_ROWS * (max_nx | 1) * sizeof(double);
        return mmx_for_voxel<MMX_VOX_INTEGER>(vol->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
            using T = MMX_TAG_T(t);
            auto k = pp_mid_kernel<T>;
            if (hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
                return MMX_ERR_HIP;
            hipLaunchKernelGGL(k, dim3(n_subs), dim3(PP_WG_MID), lds, s, (const T*)vol->d_data,
                               vol->stride_z, vol->stride_y, vol->stride_x, d_subs, d_qclasses, d_weights, A,
                               d_out32, d_out64, d_info, d_scratch);
            return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
        });
    }
    return mmx_for_voxel<MMX_VOX_PREPROC>(vol->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
        using T = MMX_TAG_T(t);
        hipLaunchKernelGGL(pp_generic_kernel<T>, dim3(n_subs), dim3(PP_WG_GENERIC), 0, s,
                           (const T*)vol->d_data, vol->stride_z, vol->stride_y, vol->stride_x, d_subs,
                           d_qclasses, d_weights, A, d_out32, d_out64, d_info, d_scratch);
        return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
    });
}

int mmx_preprocess_block_dtypes(const mmx_block* d_blocks, const mmx_block* h_blocks, int n_blocks,
                                const int32_t* d_first_tile, const int32_t* h_first_tile, int n_subs,
                                const mmx_subblock_info* d_info, int64_t dst_sy, int64_t dst_sz,
                                double* d_out64, int64_t out64_elems, int32_t* d_flags, void* stream)
{
    if (!d_blocks || !h_blocks || n_blocks < 0 || !d_first_tile || !h_first_tile || !d_info || !d_out64 || !d_flags ||
        dst_sy < 1 || dst_sz < dst_sy)
        return MMX_ERR_ARG;
    if (n_blocks > MMX_MAX_BLOCKS) return MMX_ERR_UNSUPPORTED;
    int64_t max_rows = 1;
    for (int i = 0; i < n_blocks; ++i) {
        const mmx_block& b = h_blocks[i];
        if (b.nz < 1 || b.ny < 1 || b.nx < 1 || b.src_off < 0 || b.nx > dst_sy || (int64_t)b.ny * dst_sy > dst_sz ||
            h_first_tile[i] < 0 || h_first_tile[i] >= n_subs)
            return MMX_ERR_ARG;
        if (b.src_off + (b.nz - 1) * dst_sz + (b.ny - 1) * dst_sy + b.nx > out64_elems) return MMX_ERR_WORKSPACE;
        max_rows = std::max<int64_t>(max_rows, (int64_t)b.nz * b.ny);
    }
    if (n_blocks == 0) return MMX_OK;
    hipStream_t s = (hipStream_t)stream;
    mmx_timed_scope ts(MMX_K_PREPROC, s);
    // (a wave stores half a row of a stock block: rows over grid.x, up to 1 024 workgroups a block)
    const int gx = (int)std::min<int64_t>(max_rows, 1024);
    hipLaunchKernelGGL(pp_block_dtype_kernel, dim3(gx, n_blocks), dim3(256), 0, s, d_blocks, d_first_tile, d_info,
                       dst_sy, dst_sz, d_out64, d_flags);
    return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
}

}  // extern "C"
