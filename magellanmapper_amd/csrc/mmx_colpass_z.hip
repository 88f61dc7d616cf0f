// Z pass instantiations (see mmx_colpass.inc for the kernel and its design notes).
#include "mmx_colpass.inc"

namespace {
template <int R>
int launch_z(const mmx_volume* vol, const mmx_block* d_blocks, int n_blocks, int max_cols,
             int64_t slot_elems, const mmx_taps_f32& taps, float* d_gz, float* d_gzz, hipStream_t s)
{
    dim3 grid((max_cols + MMX_WG - 1) / MMX_WG, n_blocks);
    const int sy = (int)vol->stride_y, sx = (int)vol->stride_x;
    return mmx_for_voxel<MMX_VOX_LOG>(vol->dtype, MMX_ERR_UNSUPPORTED, [&](auto t) {
        using T = MMX_TAG_T(t);
        hipLaunchKernelGGL((zpass_kernel<R, T>), grid, dim3(MMX_WG), 0, s, (const T*)vol->d_data, vol->stride_z, sy, sx,
                           d_blocks, slot_elems, d_gz, d_gzz, taps);
        return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
    });
}
}  // namespace

int mmx_launch_zpass(const mmx_volume* vol, const mmx_block* d_blocks, int n_blocks, int max_cols,
                     int64_t slot_elems, const mmx_taps_f32& taps, int radius,
                     float* d_gz, float* d_gzz, hipStream_t stream)
{
    if (!mmx_ring_radius(radius) || !mmx_voxels_ok(vol)) return MMX_ERR_UNSUPPORTED;
    switch (radius) {
#define X(R) case R: return launch_z<R>(vol, d_blocks, n_blocks, max_cols, slot_elems, taps, d_gz, d_gzz, stream);
        MMX_FOR_EACH_RADIUS(X)
#undef X
        default: return MMX_ERR_UNSUPPORTED;
    }
}
