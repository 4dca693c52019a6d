// nm_desc_finish_math.hpp -- the per-row operation sequence of the descriptor finish (include/nm_abi.h,
// nm_sift_desc_finish_batch_dev), written once for the kernel and its host twin. A row of 128 floats is held as 64 pairs:
// pair l = elements (2 l, 2 l + 1). On the device a wave holds one row, one pair per lane (Row = LaneRow: one pair, sums
// by the xor butterfly over the lanes); on the host one object holds all 64 pairs (HostRow: the same butterfly over an
// array). Every operation is IEEE binary32, fused only where fmaf is written; the translation unit is compiled with
// -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt (nm_fpspec.hpp), so both sides agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/nm_abi.h"

namespace nmdf {

constexpr int DIM = 128;
constexpr int PAIRS = 64;
constexpr float CLIP = 0.2f;
constexpr float QUANT = 512.0f;

// The butterfly: p[l] <- p[l] + p[l ^ d] for d = 32, 16, 8, 4, 2, 1. Addition commutes, so after every step the lanes l and
// l ^ d hold the same value and after the last all 64 hold the same sum.
struct HostRow {
    static constexpr int N = PAIRS;
    float a[PAIRS], b[PAIRS];
    float sum(const float (&p)[PAIRS]) const
    {
        float cur[PAIRS], nxt[PAIRS];
        for (int l = 0; l < PAIRS; ++l) cur[l] = p[l];
        for (int d = 32; d >= 1; d >>= 1) {
            for (int l = 0; l < PAIRS; ++l) nxt[l] = cur[l] + cur[l ^ d];
            for (int l = 0; l < PAIRS; ++l) cur[l] = nxt[l];
        }
        return cur[0];
    }
};

struct LaneRow {
    static constexpr int N = 1;
    float a[1], b[1];
    __device__ __forceinline__ float sum(const float (&p)[1]) const
    {
        float v = p[0];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d);
        return v;
    }
};

__host__ __device__ __forceinline__ bool usable(float s) { return s > 0.0f && __builtin_isfinite(s); }

// u8 = min(255, (int)rintf(512 v)), round half to even; anything not above zero (a negative element, the NaN RootSIFT makes
// of one) is code 0.
__host__ __device__ __forceinline__ unsigned char quantise(float v)
{
    const float q = __builtin_rintf(QUANT * v);
    if (!(q > 0.0f)) return 0;
    return q >= 255.0f ? (unsigned char)255 : (unsigned char)(int)q;
}

// v <- v / sqrt(sum v^2): lane partial fmaf(b, b, a * a), butterfly, one sqrt, one division per element.
// Returns false (row untouched) when the sum is zero or not finite.
template <class Row> __host__ __device__ __forceinline__ bool l2_normalise(Row &r)
{
    float p[Row::N];
    for (int l = 0; l < Row::N; ++l) p[l] = __builtin_fmaf(r.b[l], r.b[l], r.a[l] * r.a[l]);
    const float s = r.sum(p);
    if (!usable(s)) return false;
    const float d = __builtin_sqrtf(s);
    for (int l = 0; l < Row::N; ++l) { r.a[l] = r.a[l] / d; r.b[l] = r.b[l] / d; }
    return true;
}

// The whole sequence. Returns false when the row is to be written as zeros (the zero rule); r then holds no result.
template <class Row> __host__ __device__ __forceinline__ bool finish(Row &r, int mode)
{
    if (!l2_normalise(r)) return false;
    for (int l = 0; l < Row::N; ++l) { r.a[l] = __builtin_fminf(r.a[l], CLIP); r.b[l] = __builtin_fminf(r.b[l], CLIP); }
    if (!l2_normalise(r)) return false;
    if (mode == NM_DESC_ROOT) {
        float p[Row::N];
        for (int l = 0; l < Row::N; ++l) p[l] = r.a[l] + r.b[l];
        const float t = r.sum(p);
        if (!usable(t)) return false;
        for (int l = 0; l < Row::N; ++l) { r.a[l] = __builtin_sqrtf(r.a[l] / t); r.b[l] = __builtin_sqrtf(r.b[l] / t); }
    }
    return true;
}

}  // namespace nmdf
