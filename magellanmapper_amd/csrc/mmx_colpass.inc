// (shared by mmx_colpass_z.hip and mmx_colpass_y.hip)
// Column ("marching") passes of the separable LoG: Z pass and Y pass.
//
// Replaces, in float32, the axis-0 and axis-1 `correlate1d` passes that
// scipy.ndimage.gaussian_laplace runs per sigma
// (scipy/ndimage/_filters.py:644-707 -> :327-430 -> :258-323 -> :126-182), which is
// where skimage.feature.blob_log spends 57 % of its time (SURVEY.md section 3.1).
//
// Design (gfx950): lanes run along the contiguous x axis (z-major layout), so every
// wave-level load/store is one coalesced 256-B row segment.  Each thread owns one
// column and marches along the filter axis keeping the last 2R+1 inputs in a
// REGISTER ring (fully unrolled, period 2R+1+D), so every input is read from HBM
// exactly once and every tap is a v_fma with an SGPR weight -- no LDS, no barriers.
// D extra ring slots hold loads that are in flight (software prefetch), which is
// what keeps ~40 KB per CU outstanding for the 8 TB/s HBM3E.
//
// Symmetric kernels: out = w[0]*c + sum_k w[k]*(in[c-k] + in[c+k]); the pair sum is
// shared by the order-0 and the order-2 kernel applied to the same input.
//
//   Z pass :  I (u8/u16/f32, read once)         -> Gz  = G(z) I,      Gzz = G''(z) I
//   Y pass :  Gz, Gzz                            -> A   = G(y) Gz,
//                                                   BC  = G''(y) Gz + G(y) Gzz
//   (X pass, mmx_xpass.hip:  LoG = G''(x) A + G(x) BC)
//
// Algorithmic HBM bytes per voxel: Z 2+8, Y 8+8 (DESIGN.md section 4).

#include <type_traits>

#include "mmx_device.h"

namespace {

#ifndef MMX_PREFETCH
#define MMX_PREFETCH 4
#endif
constexpr int kPrefetch = MMX_PREFETCH;  // D: loads kept in flight per thread beyond the live window

__device__ __forceinline__ void store_f32(float v, rsrc_t r, unsigned voff)
{
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, voff, 0, 0);
}

// ---------------------------------------------------------------- Z pass
// Thread = one (y, x) column of one block, lanes along x.
template <int R, typename InT>
__global__ void __launch_bounds__(MMX_WG)
zpass_kernel(const InT* __restrict__ vol, int64_t stride_z, int stride_y, int stride_x,
             const mmx_block* __restrict__ blocks, int64_t slot_elems,
             float* __restrict__ gz, float* __restrict__ gzz, mmx_taps_f32 taps)
{
    using io = mmx_vox<InT>;
    constexpr int N = 2 * R + 1;
    constexpr int M = N + kPrefetch;
    const mmx_block bd = blocks[blockIdx.y];
    const int ncol = bd.ny * bd.px;      // pitch columns included: whole 128-B lines per store
    const int col = blockIdx.x * MMX_WG + threadIdx.x;
    if (col >= ncol) return;
    const int y = col / bd.px;
    const int xp = col - y * bd.px;
    const int x = xp < bd.nx ? xp : bd.nx - 1;   // pitch lanes re-read the last column (in bounds)
    const int n = bd.nz;
    const unsigned voff_in = (unsigned)(y * stride_y + x * stride_x) * (unsigned)sizeof(InT);
    const unsigned voff_out = (unsigned)col * 4u;
    const InT* in = vol + bd.src_off;
    const float* o0 = gz + (int64_t)bd.slot * slot_elems;
    const float* o2 = gzz + (int64_t)bd.slot * slot_elems;

    float ring[M];
#pragma unroll
    for (int j = -R; j < R + kPrefetch; ++j) {
        const float raw = io::load(make_rsrc(in + (int64_t)reflect_once(j, n) * stride_z), voff_in);
        ring[(j + M) % M] = j < R ? io::act(raw) : raw;
    }

    const InT* pin = in + (int64_t)(R + kPrefetch) * stride_z;  // plane of the next prefetch
    auto step = [&](int s, auto reflecting, int z) __attribute__((always_inline)) {
        float nxt;
        if constexpr (decltype(reflecting)::value)
            nxt = io::load(make_rsrc(in + (int64_t)reflect_once(z + R + kPrefetch, n) * stride_z), voff_in);
        else
            nxt = io::load(make_rsrc(pin), voff_in);
        pin += stride_z;
        ring[(s + R) % M] = io::act(ring[(s + R) % M]);  // loaded kPrefetch steps ago
        const float c = ring[s];
        float a0 = c * taps.w0[0];
        float a2 = c * taps.w2[0];
#pragma unroll
        for (int k = 1; k <= R; ++k) {
            const float p = ring[(s - k + M) % M] + ring[(s + k) % M];
            a0 = fmaf(p, taps.w0[k], a0);
            a2 = fmaf(p, taps.w2[k], a2);
        }
        store_f32(a0, make_rsrc(o0), voff_out);
        store_f32(a2, make_rsrc(o2), voff_out);
        o0 += ncol;
        o2 += ncol;
        ring[(s + R + kPrefetch) % M] = nxt;
        __builtin_amdgcn_sched_barrier(0);  // keep each step's load / compute / stores together
    };
    // Interior periods: every prefetch index is < n: no reflection, no control flow inside the
    // unrolled body, so the prefetched loads stay in flight across steps (counted vmcnt).
    int z0 = 0;
#pragma unroll 1
    for (; z0 + M + R + kPrefetch <= n; z0 += M) {
#pragma unroll
        for (int s = 0; s < M; ++s) step(s, std::false_type{}, 0);
    }
    // Border periods (reflecting prefetch) and the ragged end.
#pragma unroll 1
    for (; z0 < n; z0 += M) {
#pragma unroll
        for (int s = 0; s < M; ++s) {
            if (z0 + s >= n) break;
            step(s, std::true_type{}, z0 + s);
        }
    }
}

// ---------------------------------------------------------------- Y pass
// Thread = one (z, x) column of one block (x fastest), marching along y.
template <int R>
__global__ void __launch_bounds__(MMX_WG)
ypass_kernel(const mmx_block* __restrict__ blocks, int64_t slot_elems,
             const float* __restrict__ gz, const float* __restrict__ gzz,
             float* __restrict__ oa, float* __restrict__ obc, mmx_taps_f32 taps)
{
    using io = mmx_vox<float>;
    constexpr int N = 2 * R + 1;
    constexpr int M = N + kPrefetch;
    const mmx_block bd = blocks[blockIdx.y];
    const int ncol = bd.nz * bd.px;
    const int col = blockIdx.x * MMX_WG + threadIdx.x;
    if (col >= ncol) return;
    const int z = col / bd.px;
    const int x = col - z * bd.px;
    const int n = bd.ny;
    const int nx = bd.px;                // row pitch (pitch columns are filtered too)
    const unsigned voff = (unsigned)(z * bd.ny * nx + x) * 4u;
    const int64_t sbase = (int64_t)bd.slot * slot_elems;
    const float* i1 = gz + sbase;
    const float* i2 = gzz + sbase;
    const float* w1 = oa + sbase;
    const float* w2 = obc + sbase;

    float r1[M];  // Gz window
    float r2[M];  // Gzz window
#pragma unroll
    for (int j = -R; j < R + kPrefetch; ++j) {
        const int row = reflect_once(j, n) * nx;
        r1[(j + M) % M] = io::load(make_rsrc(i1 + row), voff);
        r2[(j + M) % M] = io::load(make_rsrc(i2 + row), voff);
    }

    const float* q1 = i1 + (int64_t)(R + kPrefetch) * nx;
    const float* q2 = i2 + (int64_t)(R + kPrefetch) * nx;
    auto step = [&](int s, auto reflecting, int y) __attribute__((always_inline)) {
        float n1, n2;
        if constexpr (decltype(reflecting)::value) {
            const int rnext = reflect_once(y + R + kPrefetch, n) * nx;
            n1 = io::load(make_rsrc(i1 + rnext), voff);
            n2 = io::load(make_rsrc(i2 + rnext), voff);
        } else {
            n1 = io::load(make_rsrc(q1), voff);
            n2 = io::load(make_rsrc(q2), voff);
        }
        q1 += nx;
        q2 += nx;
        const float c1 = r1[s];
        const float c2 = r2[s];
        float a = c1 * taps.w0[0];
        float bc = fmaf(c2, taps.w0[0], c1 * taps.w2[0]);
#pragma unroll
        for (int k = 1; k <= R; ++k) {
            const float p1 = r1[(s - k + M) % M] + r1[(s + k) % M];
            const float p2 = r2[(s - k + M) % M] + r2[(s + k) % M];
            a = fmaf(p1, taps.w0[k], a);
            bc = fmaf(p1, taps.w2[k], bc);
            bc = fmaf(p2, taps.w0[k], bc);
        }
        store_f32(a, make_rsrc(w1), voff);
        store_f32(bc, make_rsrc(w2), voff);
        w1 += nx;
        w2 += nx;
        r1[(s + R + kPrefetch) % M] = n1;
        r2[(s + R + kPrefetch) % M] = n2;
        __builtin_amdgcn_sched_barrier(0);
    };
    int y0 = 0;
#pragma unroll 1
    for (; y0 + M + R + kPrefetch <= n; y0 += M) {
#pragma unroll
        for (int s = 0; s < M; ++s) step(s, std::false_type{}, 0);
    }
#pragma unroll 1
    for (; y0 < n; y0 += M) {
#pragma unroll
        for (int s = 0; s < M; ++s) {
            if (y0 + s >= n) break;
            step(s, std::true_type{}, y0 + s);
        }
    }
}

}  // namespace
