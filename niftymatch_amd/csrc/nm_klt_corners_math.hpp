// nm_klt_corners_math.hpp -- the arithmetic of the Shi-Tomasi corner detector (nm_klt_corners.hip), compiled for the device
// kernels and for the host twin alike. include/nm_abi.h, "Corner detection", has the written semantics. The score is the
// tracker's own level-0 texture gate (nmk::flat of nm_klt_math.hpp) at an integer pixel centre, where a sample is the
// pixel's level itself: the sums are integers, so they do not depend on how a window is summed (a separable box sum on the
// device, a plain double loop on the host); the fp64 steps are those of nmk::flat, followed by one rounding to fp32.
#pragma once
#include "nm_klt_math.hpp"

namespace nmkc {

using nmk::i64;
using nmk::u64;

constexpr int MAX_NMS = NM_KLT_CORNERS_MAX_NMS;
constexpr int MAX_LEVEL = 255 * nmk::LEVELS_PER_UNIT;
// A pixel as 16 bits: its level (at most 4080, 12 bits), or NO_LEVEL for a pixel without one: bit 15 says so and the level
// bits are 0, so that a difference of two such words' level bits always fits 16 bits signed.
constexpr int NO_LEVEL = 0x8000, LEVEL_BITS = 0x0FFF;
// Gxx, Gyy <= 225 x 4080^2 = 3 745 440 000: an unsigned 32-bit word holds them, a signed one does not; |Gxy| has the same
// bound and so needs 33 bits signed (the kernels hold it in 64). A row of 15 products stays below 2^31.
static_assert(MAX_LEVEL == 4080 && (i64)nmk::MAX_TAPS * MAX_LEVEL * MAX_LEVEL == 3745440000ll, "the sums' bound of nm_abi.h");
static_assert((i64)nmk::MAX_TAPS * MAX_LEVEL * MAX_LEVEL <= 0xFFFFFFFFll && (i64)nmk::MAX_TAPS * MAX_LEVEL * MAX_LEVEL > 0x7FFFFFFFll,
              "Gxx and Gyy fit an unsigned 32-bit word and no signed one");
static_assert((i64)(2 * nmk::MAX_RADIUS + 1) * MAX_LEVEL * MAX_LEVEL < 0x7FFFFFFFll, "a row of products fits a signed word");

// the level of a pixel as 16 bits: NO_LEVEL when the value holds none or the mask byte (seen: the pixel has one) is 0
__host__ __device__ __forceinline__ int level16(float v, bool seen)
{
    int q;
    return (nmk::level_of(v, q) && seen) ? q : NO_LEVEL;
}

// the score of a pixel that has a window, from its sums: -1 where the tracker's gate calls the window flat
__host__ __device__ __forceinline__ float score_of(i64 Gxx, i64 Gxy, i64 Gyy, int r, double min_eig)
{
    double det, eig;
    if (nmk::flat(Gxx, Gxy, Gyy, r, min_eig, det, eig)) return -1.f;
    return (float)eig;
}

__host__ __device__ __forceinline__ bool scored(float s) { return s >= 0.f; }

// The order of the non-maximum suppression as one 64-bit key: a scored pixel's score (fp32 bits of a value >= 0 ascend with
// the value) above the complement of `ordinal`, a number that ascends in raster order over the pixels that compete. The
// larger key wins, so of equal scores the pixel that comes first does. 0: not scored, never wins.
__host__ __device__ __forceinline__ u64 nms_key(float s, unsigned ordinal)
{
    if (!scored(s)) return 0ull;
    unsigned bits;
    __builtin_memcpy(&bits, &s, sizeof bits);
    return ((u64)(bits + 1u) << 32) | (u64)(0xFFFFFFFFu - ordinal);
}

// A held row's pixel; false when the row is not tried or lies further than MAX_NMS outside the fw x fh frame, where it is
// within reach of no pixel
__host__ __device__ __forceinline__ bool held_pixel(float hx, float hy, int fw, int fh, int &px, int &py)
{
    px = py = 0;
    if (!nmk::row_tried(hx, hy)) return false;
    const float rx = __builtin_rintf(hx), ry = __builtin_rintf(hy);
    if (!(rx >= (float)-MAX_NMS && rx < (float)(fw + MAX_NMS) && ry >= (float)-MAX_NMS && ry < (float)(fh + MAX_NMS))) return false;
    px = (int)rx; py = (int)ry;
    return true;
}

inline bool params_ok(int n, int fw, int fh, int radius, int nms, float min_eig, int cap)
{
    return n >= 1 && n <= NM_KLT_MAX_BATCH && nm_size_ok(fw) && nm_size_ok(fh) && radius >= 1 && radius <= nmk::MAX_RADIUS &&
           nms >= 1 && nms <= MAX_NMS && __builtin_isfinite(min_eig) && min_eig >= 0.f && nmp::cap_ok(cap);
}

}  // namespace nmkc
