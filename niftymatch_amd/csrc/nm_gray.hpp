// nm_gray.hpp -- the BGRA -> gray arithmetic shared by nm_image.hip (nm_grayscale_f32) and nm_ingest.hip (the batched
// ingest), so that the ingest's gray plane equals nm_grayscale_f32 of its uchar4 result by construction.
#pragma once
#include "nm_common.hpp"

namespace nmg {

__device__ __forceinline__ float gray_of(uchar4 p)
{
    // 0.07*B + 0.72*G + 0.21*R in double (the literals are double), narrowed to float (bgra_2_gray.cu:16);
    // contraction written out: fma(0.21, R, fma(0.07, B, 0.72*G))
    const double b = (double)(int)p.x, g = (double)(int)p.y, r = (double)(int)p.z;
    return (float)__builtin_fma(0.21, r, __builtin_fma(0.07, b, 0.72 * g));
}

}  // namespace nmg
