// Y pass instantiations (see mmx_colpass.inc for the kernel and its design notes).
#include "mmx_colpass.inc"

namespace {
template <int R>
int launch_y(const mmx_block* d_blocks, int n_blocks, int max_cols, int64_t slot_elems,
             const mmx_taps_f32& taps, const float* d_gz, const float* d_gzz, float* d_a,
             float* d_bc, hipStream_t s)
{
    dim3 grid((max_cols + MMX_WG - 1) / MMX_WG, n_blocks);
    hipLaunchKernelGGL(ypass_kernel<R>, grid, dim3(MMX_WG), 0, s, d_blocks, slot_elems, d_gz, d_gzz, d_a, d_bc, taps);
    return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
}
}  // namespace

int mmx_launch_ypass(const mmx_block* d_blocks, int n_blocks, int max_cols, int64_t slot_elems,
                     const mmx_taps_f32& taps, int radius, const float* d_gz, const float* d_gzz,
                     float* d_a, float* d_bc, hipStream_t stream)
{
    if (!mmx_ring_radius(radius)) return MMX_ERR_UNSUPPORTED;
    switch (radius) {
#define X(R) case R: return launch_y<R>(d_blocks, n_blocks, max_cols, slot_elems, taps, d_gz, d_gzz, d_a, d_bc, stream);
        MMX_FOR_EACH_RADIUS(X)
#undef X
        default: return MMX_ERR_UNSUPPORTED;
    }
}
