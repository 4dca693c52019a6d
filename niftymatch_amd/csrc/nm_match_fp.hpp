// nm_match_fp.hpp -- number formats of the matcher's screens: bf16 / fp16 pieces of a float and the screens' domains.
#pragma once
#include <hip/hip_runtime.h>

namespace nm_match {

constexpr float MIN2_INIT = 2139095040.0f;   // (float)0x7f800000, match.cu:91
// Domain of the MFMA screens: descriptors whose squared norms are finite and below NORM_LIMIT (every distance is then finite,
// <= 4e37). A query row outside it, or ANY candidate outside it, is matched by the exact fallback alone -- the reference's
// scan, whose behaviour on NaN / inf distances (match.cu:91-116: comparisons with a NaN are false) is reproduced there.
constexpr float NORM_LIMIT = 1.0e37f;
// The fp16 coarse pass of the two-stage screen needs |2 x| <= 65504 for every element: squared norms below 1e9 (|x| < 31623).
constexpr float F16_NORM_LIMIT = 1.0e9f;

// bf16 pieces. rne: round to nearest even (the guide's integer form; finite inputs). The split x = hi + lo + r has
// |x - hi| <= 2^-8 |x| and |r| <= 2^-16 |x|  (bf16 carries 8 significant bits).
__device__ __forceinline__ unsigned bf16_rne(float x)
{
    const unsigned u = __float_as_uint(x);
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ void bf16_split(float x, unsigned &hi, unsigned &lo)
{
    hi = bf16_rne(x);
    lo = bf16_rne(x - __uint_as_float(hi << 16));          // the difference is exact
}
// A non-negative float as the EXACT sum of three bf16 values (8 + 8 + 8 significant bits, by truncation).
__device__ __forceinline__ void bf16_three(float n, unsigned &h, unsigned &m, unsigned &l)
{
    const unsigned uh = __float_as_uint(n) & 0xFFFF0000u;
    const float r1 = n - __uint_as_float(uh);
    const unsigned um = __float_as_uint(r1) & 0xFFFF0000u;
    const float r2 = r1 - __uint_as_float(um);
    h = uh >> 16; m = um >> 16; l = __float_as_uint(r2) >> 16;
}
constexpr unsigned BF16_ONE = 0x3F80u;
constexpr unsigned BF16_BIG = 0x7F7Fu;      // largest finite bf16: the "norm" of the rows that pad the last tile
__device__ __forceinline__ unsigned f16_bits(float x)
{
    const _Float16 h = (_Float16)x;                      // v_cvt_f16_f32: round to nearest even (the kernels never change the mode)
    return (unsigned)__builtin_bit_cast(unsigned short, h);
}
__device__ __forceinline__ float f16_value(unsigned bits)
{
    return (float)__builtin_bit_cast(_Float16, (unsigned short)bits);
}

}  // namespace nm_match
