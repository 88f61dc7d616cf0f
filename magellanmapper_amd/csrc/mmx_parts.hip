// A block detected as several overlapping parts: the candidates of the parts folded back into
// their parent block, between the sparse NMS (which ran on the parts) and the probe expansion / exact re-score (which
// run on the parent).
//
// A LoG value at voxel p depends on the voxels within the kernel radius R of p along each axis only, so a part -- a core
// plus a halo of R_max + 1 voxels, clipped to the parent -- holds at every voxel of its core, and at that voxel's 80
// scale-space neighbours, the values the whole block would hold.  What the NMS nominates inside a core is therefore what
// it would nominate there in the whole block; what it nominates in a halo is either a duplicate of a neighbouring part's
// candidate or an artefact of the part's artificial faces.  This kernel keeps the first kind and drops the second.
//
// In place, one workgroup: the table is walked front to back in chunks; every lane of the workgroup has its entries of
// the chunk in registers before the first kept one is written back, and a kept entry never lands behind the place it was
// read from, so no entry is overwritten before it is read.  Kept entries are placed by wave ballot: one LDS atomic per
// wave and chunk reserves the wave's range, the lanes' ranks inside it come from the ballot.  A table is 1e4 .. 1e6
// entries of 48 bytes against 1e8 .. 1e9 voxels the passes before it streamed several times.

#include <cstddef>

#include "mmx_common.h"

namespace {

static_assert(sizeof(mmx_part) == 40 && sizeof(mmx_cand) == 48 && offsetof(mmx_cand, z) == 8 && offsetof(mmx_cand, x) == 16 &&
              offsetof(mmx_part, core_lo) == 16, "mmx_part / mmx_cand layout");

constexpr int kFoldWG = 1024;     // one workgroup, 16 waves: a chunk is 1024 entries, one per lane

__global__ void __launch_bounds__(kFoldWG)
fold_parts_kernel(mmx_cand* __restrict__ tab, uint32_t cap, uint32_t* __restrict__ count,
                  const mmx_part* __restrict__ parts, int n_parts)
{
    __shared__ uint32_t kept;       // entries written so far
    const uint32_t n_in = *count;
    if (n_in > cap) return;         // (uniform) an overflowed table: the caller nominates again with a larger one
    if (threadIdx.x == 0) kept = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (uint64_t base = 0; base < n_in; base += kFoldWG) {      // (64 bits: n_in may be close to 2^32)
        const uint64_t i = base + threadIdx.x;
        bool keep = i < n_in;
        // an entry as three 16-byte words (tables are 16-byte aligned, entries 48 bytes): {slot, s, z, y}, {x, flags, v,
        // nbr_max}, {v64, band}
        uint4* e = reinterpret_cast<uint4*>(tab) + 3 * (keep ? i : 0);
        uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0, q2 = q0;
        if (keep) {
            q0 = e[0]; q1 = e[1]; q2 = e[2];
            keep = (int32_t)q0.x >= 0 && (int32_t)q0.x < n_parts;
        }
        if (keep) {
            const int32_t* p = reinterpret_cast<const int32_t*>(parts + q0.x);       // parent, off[3], core_lo[3], core_hi[3]
            const int32_t z = (int32_t)q0.z, y = (int32_t)q0.w, x = (int32_t)q1.x;
            keep = z >= p[4] && z < p[7] && y >= p[5] && y < p[8] && x >= p[6] && x < p[9];
            if (keep) {
                q0.x = (uint32_t)p[0];
                q0.z = (uint32_t)(z + p[1]);
                q0.w = (uint32_t)(y + p[2]);
                q1.x = (uint32_t)(x + p[3]);
            }
        }
        __syncthreads();            // every entry of this chunk has been read
        const unsigned long long mask = __ballot(keep);
        uint32_t at = 0;
        if (lane == 0 && mask) at = atomicAdd(&kept, (uint32_t)__popcll(mask));
        at = __shfl(at, 0);
        // (kept entries so far <= entries read so far: `at + rank` is at most this entry's own index)
        if (keep) {
            uint4* o = reinterpret_cast<uint4*>(tab) + 3 * (uint64_t)(at + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)));
            o[0] = q0; o[1] = q1; o[2] = q2;
        }
        __syncthreads();            // (every wave's reservation is in `kept`: the count below, the next chunk's ranges)
    }
    if (threadIdx.x == 0) *count = kept;
}

}  // namespace

extern "C" int mmx_fold_parts(mmx_cand* d_cands, uint32_t cap, uint32_t* d_count, const mmx_part* d_parts, int n_parts,
                              void* stream)
{
    if (!d_cands || !d_count || !d_parts || n_parts < 1 || cap < 1 || (reinterpret_cast<uintptr_t>(d_cands) & 15))
        return MMX_ERR_ARG;
    if (n_parts > MMX_MAX_BLOCKS) return MMX_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    mmx_timed_scope ts(MMX_K_PEAKS, s);
    hipLaunchKernelGGL(fold_parts_kernel, dim3(1), dim3(kFoldWG), 0, s, d_cands, cap, d_count, d_parts, n_parts);
    return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
}
