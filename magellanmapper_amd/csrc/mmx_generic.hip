// Generic (any radius, any extent) separable LoG passes: the slow, always-valid path.
//
// What it still serves: kernel radii above MMX_MAX_RADIUS_WIDE (sigma > 16 px), batches with a block thinner than the
// radius along some axis (the register-ring kernels need extent >= radius + prefetch, the wide passes of mmx_wide.hip
// extent >= radius; here SciPy's "reflect" may wrap several times), and the float64 cross-checks: it is the in-library
// reference the tests and blob_log.self_test hold every other kernel to (mmx_log_batch_f32_generic).  Radii 25 .. 64 on
// blocks at least that thick, which used to come here, take the wide passes.  Same math as mmx_colpass.hip /
// mmx_xpass.hip (scipy/ndimage/_filters.py:644-707 in float32), one thread per output voxel: the tap loops of
// mmx_taploop.h.

#include "mmx_taploop.h"

namespace {

__global__ void __launch_bounds__(MMX_WG)
gen_z(mmx_volume vol, const mmx_block* __restrict__ blocks, int64_t slot_elems, int R,
      float* __restrict__ gz, float* __restrict__ gzz, mmx_taps_generic t)
{
    const mmx_block bd = blocks[blockIdx.y];
    mmx_taploop_z(vol, bd, slot_elems, R, gz, gzz, t, blockIdx.x * MMX_WG + threadIdx.x, gridDim.x * MMX_WG);
}

__global__ void __launch_bounds__(MMX_WG)
gen_y(const mmx_block* __restrict__ blocks, int64_t slot_elems, int R,
      const float* __restrict__ gz, const float* __restrict__ gzz,
      float* __restrict__ oa, float* __restrict__ obc, mmx_taps_generic t)
{
    const mmx_block bd = blocks[blockIdx.y];
    mmx_taploop_y(bd, slot_elems, R, gz, gzz, oa, obc, t, blockIdx.x * MMX_WG + threadIdx.x, gridDim.x * MMX_WG);
}

__global__ void __launch_bounds__(MMX_WG)
gen_x(const mmx_block* __restrict__ blocks, int64_t slot_elems, int R,
      const float* __restrict__ ga, const float* __restrict__ gbc, float* __restrict__ out,
      mmx_taps_generic t)
{
    const mmx_block bd = blocks[blockIdx.y];
    mmx_taploop_x(bd, slot_elems, R, ga, gbc, out, t, blockIdx.x * MMX_WG + threadIdx.x, gridDim.x * MMX_WG);
}

}  // namespace

// pass: 0 = z, 1 = y, 2 = x.  Weights already scaled by the caller.
int mmx_launch_generic_pass(int pass, const mmx_volume* vol, const mmx_block* d_blocks, int n_blocks,
                            int max_vox, int64_t slot_elems, const float* w0, const float* w2, int radius,
                            const float* in1, const float* in2, float* out1, float* out2, hipStream_t s)
{
    if (radius < 0 || radius > MMX_MAX_RADIUS_GENERIC) return MMX_ERR_UNSUPPORTED;
    mmx_taps_generic t;
    for (int k = 0; k <= MMX_MAX_RADIUS_GENERIC; ++k) {
        t.w0[k] = k <= radius ? w0[k] : 0.f;
        t.w2[k] = k <= radius ? w2[k] : 0.f;
    }
    int gx = (max_vox + MMX_WG - 1) / MMX_WG;
    if (gx > 8192) gx = 8192;
    if (gx < 1) gx = 1;
    dim3 grid(gx, n_blocks);
    if (pass == 0)
        hipLaunchKernelGGL(gen_z, grid, dim3(MMX_WG), 0, s, *vol, d_blocks, slot_elems, radius, out1, out2, t);
    else if (pass == 1)
        hipLaunchKernelGGL(gen_y, grid, dim3(MMX_WG), 0, s, d_blocks, slot_elems, radius, in1, in2, out1, out2, t);
    else
        hipLaunchKernelGGL(gen_x, grid, dim3(MMX_WG), 0, s, d_blocks, slot_elems, radius, in1, in2, out1, t);
    return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
}
