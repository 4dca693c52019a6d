// nm_match_guided_math.hpp -- homography-guided matching (nm_sift_match_guided_batch_dev_f32 and its host twin), for gfx950.
// No reference counterpart: the reference matches blind (kernels/match.cu) and never returns to the descriptors once it has
// a model. Everything here is __host__ __device__ and is the ONLY arithmetic of both entries, so host and device agree bit
// for bit: the projection of a source row, the gate (nmr_is_inlier's fp32 sequence, csrc/nm_ransac_math.hpp, with the
// projection hoisted out of the candidate loop: the same operations, the same bits), the 128-D distance in the reference's
// chain (kernels/match.cu:36-47: acc = fma(t, t, acc), t = a_k - b_k, k ascending) and get_sift_matches' scan
// (match.cu:88-116) restricted to the gated candidates. All fp32, fma explicit (-ffp-contract=off), IEEE divide.
#pragma once
#include <hip/hip_runtime.h>

#include "nm_pair_batch.hpp"

namespace nmg {

using nmp::clip;
using nmp::finite9;

struct Scan {
    float min1, min2;
    int idx;
    int seen;                               // gated candidates met so far (0 / 1)
};

/* Where H sends (ax, ay): the first half of nmr_is_inlier */
__host__ __device__ __forceinline__ void project(const float H[9], float ax, float ay, float &px, float &py)
{
    const float x = __builtin_fmaf(H[0], ax, H[1] * ay) + H[2];
    const float y = __builtin_fmaf(H[3], ax, H[4] * ay) + H[5];
    const float z = __builtin_fmaf(H[6], ax, H[7] * ay) + H[8];
    px = x / z; py = y / z;
}

/* The second half: candidate (bx, by) against the projected row. NaN never passes. */
__host__ __device__ __forceinline__ bool gate(float px, float py, float bx, float by, float radius2)
{
    const float ex = bx - px, ey = by - py;
    return __builtin_fmaf(ex, ex, ey * ey) < radius2;
}

struct __attribute__((aligned(4))) Quad { float v[4]; };

/* Squared L2 distance of two 128-D rows, the chain of nm_bf_distance_f32: sequential in k */
__host__ __device__ __forceinline__ float distance128(const float *a, const float *b)
{
    float acc = 0.f;
#pragma unroll 8
    for (int q = 0; q < 32; ++q) {
        const Quad ua = reinterpret_cast<const Quad *>(a)[q], ub = reinterpret_cast<const Quad *>(b)[q];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float t = ua.v[u] - ub.v[u];
            acc = __builtin_fmaf(t, t, acc);
        }
    }
    return acc;
}

/* fp32 rows as the guided kernel and its host twin see them (the u8 rows: nmg8::RowsU8). A lane keeps where its row lies,
 * not the row: distance128 reads it again for every noted candidate */
struct RowsF32 {
    using Elem = float;
    struct Own { const float *A; int i; };
    __host__ __device__ __forceinline__ static void own(Own &o, const float *A, int i, bool) { o.A = A; o.i = i; }
    __host__ __device__ __forceinline__ static float distance(const Own &o, const float *B, int j)
    {
        return distance128(o.A + (size_t)o.i * 128, B + (size_t)j * 128);
    }
};

__host__ __device__ __forceinline__ void scan_init(Scan &s)
{
    s.min1 = __builtin_inff(); s.min2 = 2139095040.0f; s.idx = -1; s.seen = 0;     /* (float)0x7f800000, not +inf (match.cu:91) */
}

/* One gated candidate, in ascending j: the first one is the minimum whatever its value (match.cu:90), then strict < */
__host__ __device__ __forceinline__ void scan_step(Scan &s, int j, float d)
{
    if (!s.seen) { s.min1 = d; s.idx = j; s.seen = 1; }
    else if (d < s.min1) { s.min2 = s.min1; s.idx = j; s.min1 = d; }
    else if (d < s.min2) s.min2 = d;
}

/* The row's result: -1 without a candidate, when the scan leaves the row undecided (min2 <= 0) or a test fails */
__host__ __device__ __forceinline__ int decide(const Scan &s, float ambiguity, float max_distance)
{
    if (!s.seen || !(s.min2 > 0.f)) return -1;
    const float a = s.min1 / s.min2;
    return (a < ambiguity && s.min1 < max_distance) ? s.idx : -1;
}

}  // namespace nmg
