// nm_mosaic_median_math.hpp -- the arithmetic of the median mosaic composite (include/nm_abi.h, "Median mosaic composite"),
// shared by the kernel of nm_mosaic_median.hip and its host twin: the key of a sample, its validity, the rank rule, the
// inlier test and the two finishes. Which frames take part is nmb::frame_used of the two-band blend. The key is three
// products and two sums, each rounded on its own: the build's -ffp-contract=off must keep it so (a contracted key would
// differ from the written one in its last bit, and with it the median frame); the mean's multiply-add is an explicit
// fmaf and the division is correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt), so device and host agree bit for
// bit.
#pragma once
#include <cfloat>

#include "nm_mosaic_bands_math.hpp"

namespace nmmd {

constexpr int MODES = 2;                        // NM_MEDIAN_SELECT, NM_MEDIAN_MEAN

// y = (0.07 C_B + 0.72 C_G) + 0.21 C_R in fp32, no fma
__host__ __device__ __forceinline__ float key_of(const float4 &t)
{
    const float b = 0.07f * t.x, g = 0.72f * t.y, r = 0.21f * t.z;
    const float bg = b + g;
    return bg + r;
}

// w > w_min, w <= FLT_MAX (no infinite weight, no NaN) and a finite key (so every colour is finite)
__host__ __device__ __forceinline__ bool valid(float w, float y, float w_min)
{
    return w > w_min && w <= FLT_MAX && __builtin_fabsf(y) <= FLT_MAX;
}

// The rank rule: whether valid frame j (key yj) comes before valid frame k (key yk). Total: equal keys fall to the index.
__host__ __device__ __forceinline__ bool before(float yj, int j, float yk, int k) { return yj < yk || (yj == yk && j < k); }

// rank of the lower median among m >= 1 valid frames
__host__ __device__ __forceinline__ int median_rank(int m) { return (m - 1) >> 1; }

__host__ __device__ __forceinline__ bool inlier(float y, float y_med, float tau) { return __builtin_fabsf(y - y_med) <= tau; }

__host__ __device__ __forceinline__ uchar4 store_of(float b, float g, float r)
{
    return make_uchar4(nm_u8_sat(b * 255.9999f), nm_u8_sat(g * 255.9999f), nm_u8_sat(r * 255.9999f), 255);
}

// NM_MEDIAN_SELECT: the median frame's own sample
__host__ __device__ __forceinline__ uchar4 finish_select(const float4 &t, float &weight)
{
    weight = t.w;
    return store_of(t.x, t.y, t.z);
}

// NM_MEDIAN_MEAN: the weighted mean of the inliers, added in index order from 0
struct Mean {
    float num[3] = {0.f, 0.f, 0.f}, den = 0.f;
    __host__ __device__ __forceinline__ void add(const float4 &t)
    {
        num[0] = __builtin_fmaf(t.w, t.x, num[0]);
        num[1] = __builtin_fmaf(t.w, t.y, num[1]);
        num[2] = __builtin_fmaf(t.w, t.z, num[2]);
        den = den + t.w;
    }
    __host__ __device__ __forceinline__ uchar4 finish(float &weight) const
    {
        weight = den;
        return store_of(num[0] / den, num[1] / den, num[2] / den);
    }
};

}  // namespace nmmd
