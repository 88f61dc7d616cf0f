// Device helpers shared by the LoG kernels (gfx950): each kernel file used to carry its own copy.
#pragma once

#include "mmx_common.h"

typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef _Float16 v2h __attribute__((ext_vector_type(2)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));

// the kernel radii of the register-resident kernels, 1 .. MMX_MAX_RADIUS_FAST: one template instantiation each
#define MMX_FOR_EACH_RADIUS(X) \
    X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) \
    X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24)

namespace {

// scipy "reflect" for -n <= i < 2n: one reflection is enough when the extent is at least the reach of the
// loads (the host routes thinner blocks to the generic kernel; mmx_reflect takes any i)
__device__ __forceinline__ int reflect_once(int i, int n)
{
    i = i < 0 ? -1 - i : i;
    return i >= n ? 2 * n - 1 - i : i;
}
// reflect, then clamp: for loads that run past the last needed input (prefetches, rows with zero weights)
__device__ __forceinline__ int reflect_clamped(int i, int n)
{
    i = reflect_once(i, n);
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// Buffer descriptors: wave-uniform 48-bit base in SGPRs + one constant 32-bit per-lane byte
// offset in a VGPR.  The per-step address change is pure SALU work on the base or on a scalar offset.
using rsrc_t = __amdgpu_buffer_rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const void* p)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, 0x00020000);
}

// two floats as one dword of float16 (round to nearest even)
__device__ __forceinline__ unsigned pack_h2(float a, float b)
{
    const v2f v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, v2h));
}
// v_mfma_f32_16x16x32_f16 on operands held as four dwords
__device__ __forceinline__ v4f mfma16(const v4u& a, const v4u& b, const v4f& c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8h, a), __builtin_bit_cast(v8h, b), c, 0, 0, 0);
}

}  // namespace
