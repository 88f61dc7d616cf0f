// Exact float64 value of the scale-space cube at given points.
//
// skimage.feature.peak_local_max compares float64 cube values for exact equality and for
// `> threshold` (skimage/feature/peak.py:28-50); the float32 pipeline cannot settle ties or
// the descending-response order that feeds the overlap prune (peak.py:9-25,
// blob.py:146-187).  This kernel recomputes, for a list of (block, sigma, z, y, x) points,
//     -gaussian_laplace(img_as_float(block), sigma)[z, y, x] * mean(sigma)**2
// bit for bit as SciPy does (scipy/ndimage/_filters.py:644-707; C: NI_Correlate1D,
// symmetric branch):  per 1-D pass
//     acc = in[c] * w[0];  for k = R .. 1:  acc += (in[c-k] + in[c+k]) * w[k]
// in double, NO fused multiply-add (this file is built with -ffp-contract=off), results
// rounded to the array dtype after every pass (float64, or float32 when the image is
// float32), three terms (second derivative on axis 0, 1, 2) summed in that order.
// oracle/ndfilters.c states the same arithmetic on the CPU and is pinned to SciPy bit for
// bit; tests/test_gpu_parity.py checks this kernel against it.
//
// Design (gfx950): a 256-thread workgroup per point, a fixed number of workgroups walking the table.  The point needs a (2R+1)^2 window
// of axis-0 sums (two kernels sharing their loads), staged in LDS in column strips, then
// 3(2R+1) axis-1 sums, then 3 axis-2 sums.  Loads are L2/MALL hits (the block's voxels were
// just streamed by the float32 passes).  At R = 20 a point is 1681 columns of 20 tap pairs, each pair 5 float64
// operations and 4 of voxel conversion: ~3e5 per point, and the headline step re-scores 3-4 x 10^5 candidates and
// probes.  That is ~1e11 float64-rate instructions per step, a floor of about 3 ms of the whole device, which the kernel shares
// with the float32 passes of the next batch (DESIGN.md section 4b has the measured times).  What it must not do is
// wait for memory tap by tap or column by column: see z_phase.

#include <algorithm>
#include <type_traits>

#include "mmx_common.h"

#define MMX_MAX_SIGMAS 64

struct mmx_rescore_params {
    int32_t radius[MMX_MAX_SIGMAS];
    double norm[MMX_MAX_SIGMAS];
    int32_t strip;      // dx columns staged at once
    int32_t n_blocks;
};

namespace {

// one symmetric 1-D correlation at the centre of `vals` (length 2R+1, stride `st`), SciPy order
template <typename StoreT>
__device__ __forceinline__ double corr_at(const double* vals, int st, int R, const double* w)
{
    double acc = vals[R * st] * w[0];
    for (int k = R; k >= 1; --k) acc += (vals[(R - k) * st] + vals[(R + k) * st]) * w[k];
    return (double)(StoreT)acc;
}

// ---- the z phase: every column a thread owns marches through the taps side by side.
// A point's window has N sw columns for the 256 threads; a thread takes NC of them per pass (column e = pass base +
// c 256 + thread), issues the loads of TB tap pairs of all NC columns, and only then does the arithmetic, column by
// column in SciPy's order: the same 16 loads in flight per thread as one column at a time had, but a point at R = 20
// (7 columns a thread) waits for memory 22 times in series where it was about 30, and no load address costs vector arithmetic.
// NC is compiled in (the accumulators stay in registers); TB follows from a budget of kLoadRegs loaded voxels in flight
// (registers, but for float64 voxels).  Measured on the headline step (profiles/r13_tail_kernels.txt): budgets of 16 / 32 / 64 registers with up to
// 4 / 5 / 7 columns a pass all land within 0.3 ms of each other -- the kernel does not wait on the latency of its own
// loads -- and the smallest, which keeps five workgroups on a CU at R = 20, is the fastest.
constexpr int kLoadRegs = 16;
constexpr int kMaxCols = 4;
template <typename InT, int NC>
struct z_cfg {
    static constexpr int raw = kLoadRegs / (2 * NC);       // (float64 voxels too: half the loads in flight measured slower)
    static constexpr int TB = raw >= 8 ? 8 : raw >= 4 ? 4 : raw >= 2 ? 2 : 1;
};
// columns per thread and pass for a window of `ncols` columns: passes of at most kMaxCols, as even as the classes allow
__host__ __device__ __forceinline__ int rescore_col_class(int ncols)
{
    const int cols = (ncols + MMX_WG - 1) / MMX_WG;
    const int passes = (cols + kMaxCols - 1) / kMaxCols;
    const int per = (cols + passes - 1) / passes;
    return per <= 1 ? 1 : per <= 2 ? 2 : 4;
}

template <typename T> struct off_type { using type = T; };

// INTERIOR: the point's z window lies inside the block, plane k of it is (pt.z + k - R) sz -- scalar arithmetic on the
// point; otherwise the reflected planes come from the table zr[] in LDS.  (The choice is the workgroup's: the point is.)
// OffT: uint32_t where every (y, x) offset of the block fits 32 bits of BYTES (the loads then take a scalar plane base and
// one offset register per column; 64-bit addresses cost a register pair per load in flight), else int64_t elements.
template <typename InT, typename StoreT, int NC, bool INTERIOR, typename OffT>
__device__ __forceinline__ void z_phase(const InT* __restrict__ in, int nyb, int nxb, int pz, int py, int px0, int R, int N,
                                        int SW, int sw, int64_t sz, int64_t sy, int64_t sx,
                                        const int64_t* __restrict__ zr, const double* __restrict__ w0,
                                        const double* __restrict__ w2, double* __restrict__ zp0, double* __restrict__ zp2)
{
    constexpr int TB = z_cfg<InT, NC>::TB;
    const int ncols = N * sw;
    auto zoff = [&](int j) __attribute__((always_inline)) -> int64_t {
        if constexpr (INTERIOR) return (int64_t)(pz + j - R) * sz;
        else return zr[j];
    };
    constexpr bool kBytes = sizeof(OffT) == 4;
    auto ld = [&](OffT o, int64_t z) __attribute__((always_inline)) -> InT {
        if constexpr (kBytes) return *reinterpret_cast<const InT*>(reinterpret_cast<const char*>(in + z) + o);
        else return in[o + z];
    };
    for (int base = 0; base < ncols; base += MMX_WG * NC) {          // (uniform trip count)
        OffT off[NC];           // the column's (y, x) offset; columns past the window repeat its last one
        int at[NC];             // where its sums go, -1: nowhere
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int e = base + c * MMX_WG + (int)threadIdx.x;
            const int ec = e < ncols ? e : ncols - 1;
            const int dyi = ec / sw;
            const int dxi = ec - dyi * sw;
            const int yy = mmx_reflect(py + dyi - R, nyb);
            const int xx = mmx_reflect(px0 + dxi - R, nxb);
            off[c] = (OffT)(((int64_t)yy * sy + (int64_t)xx * sx) * (kBytes ? (int64_t)sizeof(InT) : 1));
            at[c] = e < ncols ? dyi * SW + dxi : -1;
        }
        double a0[NC], a2[NC];
        {
            const int64_t zc = zoff(R);
            InT ctr[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) ctr[c] = ld(off[c], zc);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const double cv = mmx_vox<InT>::exact(ctr[c]);
                a0[c] = cv * w0[0];
                a2[c] = cv * w2[0];
            }
        }
        // the taps in SciPy's order (k = R .. 1), TB at a time, then the remainder in halves: no tap-by-tap tail
        int k = R;
        auto batch = [&](auto nb) __attribute__((always_inline)) {
            constexpr int B = decltype(nb)::value;
            for (; k >= B; k -= B) {
                InT lo[NC][B], hi[NC][B];
                // (an empty statement the offsets pass through: hoisted out of this loop their 64-bit extensions would be
                //  formed once, and the loads would take 64-bit vector addresses instead of the scalar base + 32-bit offset)
                if constexpr (kBytes) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) asm volatile("" : "+v"(off[c]));
                }
#pragma unroll
                for (int j = 0; j < B; ++j) {
                    const int64_t zl = zoff(R - (k - j)), zh = zoff(R + (k - j));
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        lo[c][j] = ld(off[c], zl);
                        hi[c][j] = ld(off[c], zh);
                    }
                }
#pragma unroll
                for (int c = 0; c < NC; ++c) {
#pragma unroll
                    for (int j = 0; j < B; ++j) {
                        const double p = mmx_vox<InT>::exact(lo[c][j]) + mmx_vox<InT>::exact(hi[c][j]);
                        a0[c] += p * w0[k - j];
                        a2[c] += p * w2[k - j];
                    }
                }
            }
        };
        batch(std::integral_constant<int, TB>{});
        if constexpr (TB > 4) batch(std::integral_constant<int, 4>{});
        if constexpr (TB > 2) batch(std::integral_constant<int, 2>{});
        if constexpr (TB > 1) batch(std::integral_constant<int, 1>{});
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (at[c] >= 0) {
                zp0[at[c]] = (double)(StoreT)a0[c];
                zp2[at[c]] = (double)(StoreT)a2[c];
            }
        }
    }
}

// PER_BLOCK (preprocessed blocks of a float32 image: float32 or float64 block by block): `block_f32` holds a flag per
// block and this launch takes the points of the blocks whose flag equals `want` alone; the other instantiation, launched
// beside it, takes the rest.
template <typename InT, typename StoreT, bool PER_BLOCK = false>
__global__ void __launch_bounds__(MMX_WG)
rescore_kernel(const InT* __restrict__ vol, int64_t sz, int64_t sy, int64_t sx,
               const mmx_block* __restrict__ blocks, mmx_cand* __restrict__ pts, uint32_t cap,
               const uint32_t* __restrict__ count, const double* __restrict__ w0_tab,
               const double* __restrict__ w2_tab, mmx_rescore_params prm,
               const int32_t* __restrict__ block_f32 = nullptr, int want = 0)
{
    extern __shared__ double smem[];
    uint32_t n = cap;
    if (count) { const uint32_t c = *count; n = c < cap ? c : cap; }
    // A fixed number of workgroups walks the table (round 4).  One workgroup per table ENTRY used to be launched --
    // the table's capacity, ~10^6, for the ~3 x 10^4 points a batch really has: 97 % of the workgroups read the count and
    // left, which still cost each a wave slot for a few hundred cycles (~0.1 ms per launch).
    for (uint64_t idx64 = blockIdx.x; idx64 < n; idx64 += gridDim.x) {
    const uint32_t idx = (uint32_t)idx64;
    // (the point is the same for every lane: readfirstlane tells the compiler, so that the weight tables -- indexed by
    //  the point's scale -- are read by scalar loads next to their use instead of two vector loads per tap)
    const mmx_cand ptv = pts[idx];
    mmx_cand pt;
    pt.slot = __builtin_amdgcn_readfirstlane(ptv.slot);
    pt.s = __builtin_amdgcn_readfirstlane(ptv.s);
    pt.z = __builtin_amdgcn_readfirstlane(ptv.z);
    pt.y = __builtin_amdgcn_readfirstlane(ptv.y);
    pt.x = __builtin_amdgcn_readfirstlane(ptv.x);
    if (pt.slot < 0 || pt.slot >= prm.n_blocks || pt.s < 0 || pt.s >= MMX_MAX_SIGMAS) continue;     // (whole workgroup)
    if constexpr (PER_BLOCK) {
        if ((block_f32[pt.slot] != 0) != (want != 0)) continue;                                      // (whole workgroup)
    }
    const mmx_block bd = blocks[pt.slot];
    const int R = prm.radius[pt.s];
    const int N = 2 * R + 1;
    const int SW = prm.strip < N ? prm.strip : N;
    const double* w0 = w0_tab + (int64_t)pt.s * (MMX_MAX_RADIUS_GENERIC + 1);
    const double* w2 = w2_tab + (int64_t)pt.s * (MMX_MAX_RADIUS_GENERIC + 1);
    const InT* in = vol + bd.src_off;

    double* zp0 = smem;                 // [N][SW]  axis-0 sums, order-0 kernel
    double* zp2 = zp0 + (size_t)N * SW; // [N][SW]  axis-0 sums, order-2 kernel
    double* yp = zp2 + (size_t)N * SW;  // [3][N]   axis-1 sums of the three terms
    // [N] element offsets of the reflected z planes (as 64-bit products once per point: a 64-bit integer
    // multiply per load would cost as much issue time as the float64 arithmetic of the tap)
    int64_t* zr = (int64_t*)(yp + 3 * (size_t)N);

    const bool interior = pt.z - R >= 0 && pt.z + R < bd.nz;
    const int cls = rescore_col_class(N * SW);
    // (strides are in elements and may be anything the caller's view has: decided on the block's largest offset)
    const bool small = ((int64_t)(bd.ny - 1) * sy + (int64_t)(bd.nx - 1) * sx) * (int64_t)sizeof(InT) < (1ll << 31)
                       && sy >= 0 && sx >= 0;
    __syncthreads();                    // (the previous point's last reads of this memory)
    if (!interior) {
        for (int k = threadIdx.x; k < N; k += MMX_WG) zr[k] = (int64_t)mmx_reflect(pt.z + k - R, bd.nz) * sz;
        __syncthreads();
    }
    for (int dx0 = 0; dx0 < N; dx0 += SW) {
        const int sw = (N - dx0) < SW ? (N - dx0) : SW;
        // ---- axis 0 (z): two kernels share every load
        auto zrun = [&](auto nc, auto ot) __attribute__((always_inline)) {
            constexpr int NC = decltype(nc)::value;
            using OffT = typename decltype(ot)::type;
            if (interior)
                z_phase<InT, StoreT, NC, true, OffT>(in, bd.ny, bd.nx, pt.z, pt.y, pt.x + dx0, R, N, SW, sw, sz, sy, sx,
                                                     zr, w0, w2, zp0, zp2);
            else
                z_phase<InT, StoreT, NC, false, OffT>(in, bd.ny, bd.nx, pt.z, pt.y, pt.x + dx0, R, N, SW, sw, sz, sy, sx,
                                                      zr, w0, w2, zp0, zp2);
        };
        if (!small) zrun(std::integral_constant<int, 2>{}, off_type<int64_t>{});   // (any NC walks any window)
        else switch (cls) {                  // (the class of the point's full strip; a narrower last strip runs in it too)
            case 1: zrun(std::integral_constant<int, 1>{}, off_type<uint32_t>{}); break;
            case 2: zrun(std::integral_constant<int, 2>{}, off_type<uint32_t>{}); break;
            default: zrun(std::integral_constant<int, 4>{}, off_type<uint32_t>{}); break;
        }
        __syncthreads();
        // ---- axis 1 (y): term 0 = G(y) on G''(z);  term 1 = G''(y) on G(z);  term 2 = G(y) on G(z)
        for (int t = threadIdx.x; t < 3 * sw; t += MMX_WG) {
            const int term = t / sw;
            const int dxi = t - term * sw;
            const double* src = (term == 0 ? zp2 : zp0) + dxi;
            yp[term * N + dx0 + dxi] = corr_at<StoreT>(src, SW, R, term == 1 ? w2 : w0);
        }
        __syncthreads();
    }
    // ---- axis 2 (x) and the sum of the three terms, in SciPy's order
    if (threadIdx.x < 3)      // the three terms side by side (each a serial chain of R dependent LDS reads)
        zp0[threadIdx.x] = corr_at<StoreT>(yp + threadIdx.x * N, 1, R, threadIdx.x == 2 ? w2 : w0);
    __syncthreads();
    if (threadIdx.x == 0) {
        const StoreT t0 = (StoreT)zp0[0];
        const StoreT t1 = (StoreT)zp0[1];
        const StoreT t2 = (StoreT)zp0[2];
        StoreT sum = t0;
        sum += t1;
        sum += t2;
        const StoreT cube = (-sum) * (StoreT)prm.norm[pt.s];
        pts[idx].v64 = (double)cube;
    }
    }       // next point
}

template <typename InT, typename StoreT>
int launch_per_block(const mmx_volume* vol, const mmx_block* d_blocks, mmx_cand* d_pts, uint32_t cap,
                     const uint32_t* d_count, const double* d_w0, const double* d_w2,
                     const mmx_rescore_params& prm, size_t lds, hipStream_t s, const int32_t* d_block_f32, int want)
{
    const uint32_t gx = cap < 8192u ? cap : 8192u;
    hipLaunchKernelGGL((rescore_kernel<InT, StoreT, true>), dim3(gx), dim3(MMX_WG), lds, s,
                       (const InT*)vol->d_data, vol->stride_z, vol->stride_y, vol->stride_x, d_blocks,
                       d_pts, cap, d_count, d_w0, d_w2, prm, d_block_f32, want);
    return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
}

template <typename InT, typename StoreT>
int launch(const mmx_volume* vol, const mmx_block* d_blocks, mmx_cand* d_pts, uint32_t cap,
           const uint32_t* d_count, const double* d_w0, const double* d_w2,
           const mmx_rescore_params& prm, size_t lds, hipStream_t s)
{
    // (256 CUs x the workgroups a CU holds at 60 KiB of LDS each, a few times over: the points' costs differ with sigma)
    const uint32_t gx = cap < 8192u ? cap : 8192u;
    hipLaunchKernelGGL((rescore_kernel<InT, StoreT>), dim3(gx), dim3(MMX_WG), lds, s,
                       (const InT*)vol->d_data, vol->stride_z, vol->stride_y, vol->stride_x, d_blocks,
                       d_pts, cap, d_count, d_w0, d_w2, prm);
    return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
}

}  // namespace

// ---- probes: the neighbours whose exact values decide a contested candidate, appended to the candidate table
// itself so that ONE re-score launch and ONE copy bring the host everything it needs (the host used to build this
// list from the candidates, upload it and wait for a second re-score: two device round trips per batch).
namespace {
__global__ void __launch_bounds__(MMX_WG)
expand_probes_kernel(mmx_cand* __restrict__ tab, uint32_t cap, uint32_t* __restrict__ count,
                     const uint32_t* __restrict__ n_cands, const mmx_block* __restrict__ blocks, int n_blocks, int ns)
{
    const uint32_t n = *n_cands < cap ? *n_cands : cap;
    for (uint64_t i = (uint64_t)blockIdx.x * MMX_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * MMX_WG) {
        const mmx_cand c = tab[i];
        if (!(c.flags & MMX_CAND_CONTESTED) || c.slot < 0 || c.slot >= n_blocks) continue;
        const mmx_block bd = blocks[c.slot];
        const bool banded = (c.flags & MMX_CAND_BAND) != 0;
        int j = 0;
        for (int ds = -1; ds <= 1; ++ds)
            for (int dz = -1; dz <= 1; ++dz)
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        if ((ds | dz | dy | dx) == 0) continue;
                        const int bit = j++;
                        const int ss = c.s + ds, zz = c.z + dz, yy = c.y + dy, xx = c.x + dx;
                        if (ss < 0 || ss >= ns || zz < 0 || zz >= bd.nz || yy < 0 || yy >= bd.ny || xx < 0 || xx >= bd.nx)
                            continue;
                        if (banded && !(bit < 64 ? (c.band >> bit) & 1ull : (c.flags >> (16 + bit - 64)) & 1u)) continue;
                        const uint32_t pos = atomicAdd(count, 1u);
                        if (pos < cap) {
                            mmx_cand r;
                            r.slot = c.slot; r.s = ss; r.z = zz; r.y = yy; r.x = xx;
                            r.flags = MMX_CAND_PROBE;
                            r.v = 0.f; r.nbr_max = 0.f;
                            r.v64 = __longlong_as_double(0x7ff8000000000000LL);
                            r.band = i;                      // the candidate this neighbour may out-vote
                            tab[pos] = r;
                        }
                    }
    }
}
}  // namespace

extern "C" int mmx_expand_probes(mmx_cand* d_cands, uint32_t cap, uint32_t* d_count, uint32_t* d_n_cands,
                                 const mmx_block* d_blocks, int n_blocks, int n_sigma, void* stream)
{
    if (!d_cands || !d_count || !d_n_cands || !d_blocks || n_blocks < 1 || n_sigma < 1) return MMX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(d_n_cands, d_count, sizeof(uint32_t), hipMemcpyDeviceToDevice, s) != hipSuccess) return MMX_ERR_HIP;
    if (cap == 0) return MMX_OK;
    mmx_timed_scope ts(MMX_K_RESCORE, s);
    const uint32_t gx = std::min<uint32_t>(1024u, (cap + MMX_WG - 1) / MMX_WG);
    hipLaunchKernelGGL(expand_probes_kernel, dim3(gx), dim3(MMX_WG), 0, s, d_cands, cap, d_count, d_n_cands, d_blocks,
                       n_blocks, n_sigma);
    return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
}

extern "C" int mmx_rescore_f64(const mmx_volume* vol, const mmx_block* d_blocks, int n_blocks,
                               mmx_cand* d_pts, uint32_t cap, const uint32_t* d_count,
                               const double* d_w0, const double* d_w2, const int32_t* h_radius,
                               const double* h_norm, int n_sigma, int store_f32, void* stream)
{
    return mmx_rescore_per_block(vol, d_blocks, n_blocks, d_pts, cap, d_count, d_w0, d_w2, h_radius, h_norm, n_sigma,
                                 store_f32, nullptr, stream);
}

// mmx_rescore_f64 with the store type chosen PER BLOCK (mmx_detect_args.d_block_f32; called by mmx_detect_batch): `vol`
// is the float64 copy of preprocessed blocks, in which a float32 block already holds float32 values widened -- reading
// it as doubles is reading the float32 image -- so one volume serves both instantiations; each skips the other's blocks.
int mmx_rescore_per_block(const mmx_volume* vol, const mmx_block* d_blocks, int n_blocks,
                          mmx_cand* d_pts, uint32_t cap, const uint32_t* d_count,
                          const double* d_w0, const double* d_w2, const int32_t* h_radius,
                          const double* h_norm, int n_sigma, int store_f32, const int32_t* d_block_f32, void* stream)
{
    const bool per_block = d_block_f32 != nullptr;
    if (!vol || !vol->d_data || !d_blocks || !d_pts || !d_w0 || !d_w2 || !h_radius || !h_norm)
        return MMX_ERR_ARG;
    if (n_sigma < 1 || n_sigma > MMX_MAX_SIGMAS || n_blocks < 1) return MMX_ERR_ARG;
    if (cap == 0) return MMX_OK;
    mmx_rescore_params prm;
    int rmax = 0;
    for (int i = 0; i < MMX_MAX_SIGMAS; ++i) { prm.radius[i] = 0; prm.norm[i] = 0.0; }
    for (int i = 0; i < n_sigma; ++i) {
        if (h_radius[i] < 0 || h_radius[i] > MMX_MAX_RADIUS_GENERIC) return MMX_ERR_UNSUPPORTED;
        prm.radius[i] = h_radius[i];
        prm.norm[i] = h_norm[i];
        if (h_radius[i] > rmax) rmax = h_radius[i];
    }
    prm.n_blocks = n_blocks;
    const int N = 2 * rmax + 1;
    const size_t budget = 60 * 1024;
    const size_t fixed = (size_t)3 * N * sizeof(double) + (size_t)N * sizeof(int64_t) + 16;
    int strip = (int)((budget - fixed) / ((size_t)2 * N * sizeof(double)));
    if (strip < 1) return MMX_ERR_UNSUPPORTED;
    if (strip > N) strip = N;
    prm.strip = strip;
    const size_t lds = (size_t)2 * N * strip * sizeof(double) + fixed;
    hipStream_t s = (hipStream_t)stream;
    const bool f32s = store_f32 != 0;
    mmx_timed_scope ts(MMX_K_RESCORE, s);
    if (per_block) {
        if (vol->dtype != MMX_F64) return MMX_ERR_UNSUPPORTED;
        const int rc = launch_per_block<double, double>(vol, d_blocks, d_pts, cap, d_count, d_w0, d_w2, prm, lds, s,
                                                        d_block_f32, 0);
        if (rc != MMX_OK) return rc;
        return launch_per_block<double, float>(vol, d_blocks, d_pts, cap, d_count, d_w0, d_w2, prm, lds, s,
                                               d_block_f32, 1);
    }
    return mmx_for_voxel<MMX_VOX_ALL>(vol->dtype, MMX_ERR_ARG, [&](auto t) {
        using T = MMX_TAG_T(t);
        if constexpr (std::is_same<T, float>::value)
            if (f32s) return launch<T, float>(vol, d_blocks, d_pts, cap, d_count, d_w0, d_w2, prm, lds, s);
        return launch<T, double>(vol, d_blocks, d_pts, cap, d_count, d_w0, d_w2, prm, lds, s);
    });
}
