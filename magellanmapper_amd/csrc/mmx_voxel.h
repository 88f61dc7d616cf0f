// What a voxel type IS: THE ONE STATEMENT.  Host: a constexpr record per mmx_dtype, the sets of types the kernel
// families accept, and the one dispatcher from a dtype code to a C++ type.  Device: the two traits every kernel takes its
// conversions from -- a raw voxel as a float (mmx_vox) and the order-preserving key (mmx_key).
// Included by mmx_common.h (behind hip_runtime.h); the host part is all a host-only program reads (tools/route_check.cpp).
#pragma once

#include <stdint.h>

#include <type_traits>

#include "../../include/mmx.h"

// ------------------------------------------------------------------------------------------------------ the record
struct mmx_voxel_rec {
    int bytes;
    bool integer, is_signed;
    double in_scale;    // skimage img_as_float: (x + in_add) * in_scale; 1 for the float types
    double in_add;      // the 0.5 of the signed form, (x + 0.5) * (2 / (imax - imin))
    double span;        // the value span after img_as_float: [0, 1] -> 1, int16's [-1, 1] -> 2 (1 for the float types)
    int pieces;         // float16 pieces per voxel in the tiled path's copy
};
constexpr int MMX_DTYPE_COUNT = 5;
constexpr mmx_voxel_rec mmx_voxel_table[MMX_DTYPE_COUNT] = {
    /* MMX_U8  */ {1, true, false, 1.0 / 255.0, 0.0, 1.0, 1},
    /* MMX_U16 */ {2, true, false, 1.0 / 65535.0, 0.0, 1.0, 1},
    /* MMX_F32 */ {4, false, true, 1.0, 0.0, 1.0, 2},
    /* MMX_F64 */ {8, false, true, 1.0, 0.0, 1.0, 1},      // (never copied: the LoG passes refuse it)
    /* MMX_I16 */ {2, true, true, 2.0 / 65535.0, 0.5, 2.0, 1},
};
static_assert(MMX_U8 == 0 && MMX_U16 == 1 && MMX_F32 == 2 && MMX_F64 == 3 && MMX_I16 == 4, "mmx_voxel_table follows mmx_dtype");
// the record of a dtype code; null for a code that names no type
constexpr const mmx_voxel_rec* mmx_voxel(int dtype)
{
    return dtype >= 0 && dtype < MMX_DTYPE_COUNT ? &mmx_voxel_table[dtype] : nullptr;
}
// the tiled path's pieces carry v / 2^16 of the voxel widened to 16 bits: img_as_float's scale on top of that
// (float voxels: as they are)
constexpr double mmx_voxel_xscale(int dtype)
{
    return mmx_voxel(dtype)->integer ? mmx_voxel(dtype)->in_scale * (double)(1 << (8 * mmx_voxel(dtype)->bytes)) : 1.0;
}
static_assert(mmx_voxel_xscale(MMX_U8) == 65536.0 / (255.0 * 256.0) && (float)mmx_voxel_xscale(MMX_U8) == (float)(65536.0 / (255.0 * 256.0)), "");
static_assert(mmx_voxel_xscale(MMX_U16) == 65536.0 / 65535.0 && (float)mmx_voxel_xscale(MMX_U16) == (float)(65536.0 / 65535.0), "");
static_assert(mmx_voxel_xscale(MMX_I16) == 2.0 * 65536.0 / 65535.0 && (float)mmx_voxel_xscale(MMX_I16) == (float)(2.0 * 65536.0 / 65535.0), "");
static_assert(mmx_voxel_xscale(MMX_F32) == 1.0 && (float)mmx_voxel_xscale(MMX_F32) == 1.f, "");

// ------------------------------------------------------------------------------------------- the accepted sets
constexpr unsigned mmx_vox_bit(int dtype) { return 1u << dtype; }
constexpr unsigned MMX_VOX_ALL = mmx_vox_bit(MMX_U8) | mmx_vox_bit(MMX_U16) | mmx_vox_bit(MMX_F32) | mmx_vox_bit(MMX_F64) | mmx_vox_bit(MMX_I16);
constexpr unsigned MMX_VOX_LOG = MMX_VOX_ALL & ~mmx_vox_bit(MMX_F64);                         // the float32 LoG passes
constexpr unsigned MMX_VOX_INTEGER = mmx_vox_bit(MMX_U8) | mmx_vox_bit(MMX_U16) | mmx_vox_bit(MMX_I16);
// the preprocessing: every type.  float64 voxels take the one-output-per-lane kernel only, float32 voxels the register-
// line forms of their own as well (pp_f32_kernel); a float32 image is computed
// under the casting rules of NumPy 2 (non-identity tiles in float64, identity tiles in float32), which the host layer
// makes its caller opt into (preprocess.FLOAT32_RULES): the library itself has one arithmetic per type
constexpr unsigned MMX_VOX_PREPROC = MMX_VOX_INTEGER | mmx_vox_bit(MMX_F64) | mmx_vox_bit(MMX_F32);
constexpr bool mmx_voxel_in(int dtype, unsigned mask) { return mmx_voxel(dtype) && ((mask >> dtype) & 1u); }

// ------------------------------------------------------------------------------------------------ the dispatcher
template <typename T> struct mmx_tag { using type = T; };
#define MMX_TAG_T(t) typename decltype(t)::type
// f(mmx_tag<T>{}) for the type a code of MASK names; `refusal` for every other code, a code that names no type included.
// No branch of it falls to a type: a code outside MASK instantiates nothing and calls nothing.
template <unsigned MASK, typename R = int, typename F>
__host__ __device__ inline R mmx_for_voxel(int dtype, typename std::common_type<R>::type refusal, F&& f)
{
    switch (dtype) {
        case MMX_U8:  if constexpr ((MASK & mmx_vox_bit(MMX_U8)) != 0) return f(mmx_tag<uint8_t>{}); break;
        case MMX_U16: if constexpr ((MASK & mmx_vox_bit(MMX_U16)) != 0) return f(mmx_tag<uint16_t>{}); break;
        case MMX_F32: if constexpr ((MASK & mmx_vox_bit(MMX_F32)) != 0) return f(mmx_tag<float>{}); break;
        case MMX_F64: if constexpr ((MASK & mmx_vox_bit(MMX_F64)) != 0) return f(mmx_tag<double>{}); break;
        case MMX_I16: if constexpr ((MASK & mmx_vox_bit(MMX_I16)) != 0) return f(mmx_tag<int16_t>{}); break;
    }
    return refusal;
}
// the code of a C++ voxel type
template <typename T> struct mmx_dtype_of;
template <> struct mmx_dtype_of<uint8_t>  { static constexpr int code = MMX_U8; };
template <> struct mmx_dtype_of<uint16_t> { static constexpr int code = MMX_U16; };
template <> struct mmx_dtype_of<float>    { static constexpr int code = MMX_F32; };
template <> struct mmx_dtype_of<double>   { static constexpr int code = MMX_F64; };
template <> struct mmx_dtype_of<int16_t>  { static constexpr int code = MMX_I16; };

// ---------------------------------------------------------------------------------------- device: a voxel as a float
// The value the float32 kernels filter: the voxel itself, plus the 0.5 of img_as_float's signed form for int16 (exact in
// float32, 17 significant bits); img_as_float's multiplier rides in the weights.  Three instruction forms, one arithmetic:
//   of(v)        a voxel loaded through a pointer
//   load / act   raw bits through a buffer descriptor (r: wave-uniform base, o: per-lane byte offset, so: scalar byte
//                offset), converted ("activated") when first needed, some steps after the load was issued, so that the
//                conversion does not pull the s_waitcnt forward
//   exact(v)     img_as_float in float64 with its own roundings: x * (1 / imax), or (x + 0.5) * (2 / (imax - imin)) --
//                out = x + 0.5 (exact), out *= the multiplier
template <typename T> struct mmx_vox {
    static constexpr mmx_voxel_rec rec = mmx_voxel_table[mmx_dtype_of<T>::code];
    static __device__ __forceinline__ float of(T v)
    {
        if constexpr (rec.integer && rec.is_signed) return (float)v + (float)rec.in_add;
        else return (float)v;
    }
    static __device__ __forceinline__ float load(__amdgpu_buffer_rsrc_t r, unsigned o, unsigned so = 0)
    {
        static_assert(sizeof(T) <= 4, "buffer loads of 1, 2 and 4 bytes");
        if constexpr (sizeof(T) == 1) return __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b8(r, o, so, 0));
        else if constexpr (sizeof(T) == 2) return __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b16(r, o, so, 0));
        else return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, o, so, 0));
    }
    static __device__ __forceinline__ float act(float raw)
    {
        if constexpr (!rec.integer) return raw;
        else if constexpr (rec.is_signed) return (float)(int)(T)__float_as_uint(raw) + (float)rec.in_add;
        else return (float)__float_as_uint(raw);
    }
    static __device__ __forceinline__ double exact(T v)
    {
        if constexpr (!rec.integer) return (double)v;
        else if constexpr (rec.is_signed) return ((double)v + rec.in_add) * rec.in_scale;
        else return (double)v * rec.in_scale;
    }
};

// ------------------------------------------------------------------------------ device: the order-preserving key
// Histograms, radix selects and "no voxel" sentinels work on a non-negative key that sorts as the values do:
//   integers   value + bias (the value itself for the unsigned types, x ^ 0x8000 as uint16 for int16)
//   floats     the sign-flip key of the bits (flip); make puts every NaN last, np.sort's place for it
// levels: bytes of the key, most significant first; value(): the voxel of a key, as a double.
template <typename T, bool INTEGER = std::is_integral<T>::value> struct mmx_key;
template <typename T> struct mmx_key<T, true> {
    using type = uint32_t;
    static constexpr int levels = (int)sizeof(T);
    static constexpr int bias = std::is_signed<T>::value ? 1 << (8 * sizeof(T) - 1) : 0;
    static __device__ __forceinline__ type make(T v, bool& nan)
    {
        using U = typename std::make_unsigned<T>::type;
        if constexpr (bias != 0) return (uint32_t)(U)v ^ (uint32_t)bias;
        else return v;
    }
    static __device__ __forceinline__ double value(unsigned long long k)
    {
        if constexpr (bias != 0) return (double)(T)((uint32_t)k ^ (uint32_t)bias);
        else return (double)k;
    }
};
template <> struct mmx_key<float, false> {
    using type = uint32_t;
    static constexpr int levels = 4, bias = 0;
    static __device__ __forceinline__ type flip(uint32_t b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
    static __device__ __forceinline__ type make(float v, bool& nan)
    {
        const uint32_t b = __float_as_uint(v);
        if ((b & 0x7fffffffu) > 0x7f800000u) { nan = true; return 0xffffffffu; }
        return flip(b);
    }
    static __device__ __forceinline__ double value(unsigned long long k)
    {
        const uint32_t key = (uint32_t)k;
        return (double)__uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
    }
};
template <> struct mmx_key<double, false> {
    using type = unsigned long long;
    static constexpr int levels = 8, bias = 0;
    static __device__ __forceinline__ type flip(unsigned long long b) { return (b >> 63) ? ~b : (b | 0x8000000000000000ull); }
    static __device__ __forceinline__ type make(double v, bool& nan)
    {
        const unsigned long long b = (unsigned long long)__double_as_longlong(v);
        if ((b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) { nan = true; return ~0ull; }
        return flip(b);
    }
    static __device__ __forceinline__ double value(unsigned long long k)
    {
        return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k));
    }
};
