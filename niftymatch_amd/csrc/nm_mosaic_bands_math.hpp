// nm_mosaic_bands_math.hpp -- the arithmetic of the two-band mosaic blend (include/nm_abi.h, "Two-band mosaic blend"),
// shared by the kernels of nm_mosaic_bands.hip and their host twin: which frames take part, the label rule, the five
// planes of a tile pixel, the ONE tap summation order of the blur, and the compose step. The build uses
// -ffp-contract=off and correctly rounded fp32 division; every multiply-add is an explicit fmaf (as nm_fpspec.hpp asks),
// so device and host agree bit for bit.
#pragma once
#include <cmath>

#include "nm_common.hpp"
#include "../../include/nm_abi.h"

namespace nmb {

constexpr int MAX_R = NM_BANDS_MAX_RADIUS;
constexpr int PLANES = 5;                       // L_B, L_G, L_R, V, M
constexpr unsigned char NO_LABEL = 255;
constexpr long long MAX_TILE_CAP = 1ll << 30;

struct Taps { float g[MAX_R + 1]; };            // travels as a kernel argument

// g[i] = (float)(t_i / S), t_i = exp(-i^2 / (2 sigma^2)), S = t_0 + 2 (t_1 + .. + t_R) added in ascending i, all in
// double; g[i] = 0 beyond R. Host only: exp is never evaluated on the device. R = 0 gives g[0] = 1 whatever sigma is.
inline void taps_of(int R, double sigma, Taps &T)
{
    double t[MAX_R + 1], S = 1.0;
    t[0] = 1.0;
    for (int i = 1; i <= R; ++i) {
        t[i] = std::exp(-(double)(i * i) / (2.0 * sigma * sigma));
        S += 2.0 * t[i];
    }
    for (int i = 0; i <= MAX_R; ++i) T.g[i] = i <= R ? (float)(t[i] / S) : 0.f;
}

// Whether frame k has a tile: placed, a non-empty rectangle, and nw x nh (in 64-bit) within the slot
__host__ __device__ __forceinline__ bool frame_used(int placed, int nw, int nh, long long tile_cap)
{
    return placed != 0 && nw > 0 && nh > 0 && (long long)nw * (long long)nh <= tile_cap;
}

// Label rule: frame k of weight w replaces the current winner only when w > 0 and w > best (frames come in index order, so
// ties stay with the lowest index)
__host__ __device__ __forceinline__ void label_step(int k, float w, int &label, float &best)
{
    if (w > 0.f && (label == NO_LABEL || w > best)) { label = k; best = w; }
}

// The five plane values of one tile pixel t = (C_B, C_G, C_R, w): v C (C is 0 where v is false), v, I
__host__ __device__ __forceinline__ void planes_of(const float4 &t, bool is_label, float p[PLANES])
{
    const bool v = t.w > 0.f;
    p[0] = v ? t.x : 0.f; p[1] = v ? t.y : 0.f; p[2] = v ? t.z : 0.f;
    p[3] = v ? 1.f : 0.f;
    p[4] = is_label ? 1.f : 0.f;
}

// THE tap summation order, one pass, one plane: g[0] s(0), then for i = 1 .. R  acc = fma(g[i], s(-i) + s(i), acc).
// at(i) is the plane's value i pixels along the pass direction from the output pixel, 0 outside the frame's rectangle.
template <class At>
__host__ __device__ __forceinline__ float tap_sum(const float *g, int R, At at)
{
    float acc = g[0] * at(0);
    for (int i = 1; i <= R; ++i) acc = __builtin_fmaf(g[i], at(-i) + at(i), acc);
    return acc;
}

// Compose of one labelled canvas pixel: begin with the winner's blurred (L, V), add every frame valid at the pixel in
// index order (the winner included: its difference is exactly 0), finish on the winner's own colour.
struct Compose {
    float ls[3], num[3], den;
    __host__ __device__ __forceinline__ void begin(const float4 &LV)
    {
        ls[0] = LV.x / LV.w; ls[1] = LV.y / LV.w; ls[2] = LV.z / LV.w;
        num[0] = num[1] = num[2] = 0.f;
        den = 0.f;
    }
    __host__ __device__ __forceinline__ void add(const float4 &LV, float M)
    {
        num[0] = __builtin_fmaf(M, LV.x / LV.w - ls[0], num[0]);
        num[1] = __builtin_fmaf(M, LV.y / LV.w - ls[1], num[1]);
        num[2] = __builtin_fmaf(M, LV.z / LV.w - ls[2], num[2]);
        den = den + M;
    }
    __host__ __device__ __forceinline__ uchar4 finish(const float4 &Cs) const
    {
        return make_uchar4(nm_u8_sat((Cs.x + num[0] / den) * 255.9999f), nm_u8_sat((Cs.y + num[1] / den) * 255.9999f),
                           nm_u8_sat((Cs.z + num[2] / den) * 255.9999f), 255);
    }
};

// Workspace layout: the label plane (one byte per canvas pixel, rounded up to 256 bytes), then for the row pass and for
// the column pass n x tile_cap float4 (L_B, L_G, L_R, V) and n x tile_cap float (M).
struct Workspace {
    unsigned char *label;
    float4 *lv[2];
    float *m[2];
};
__host__ __device__ __forceinline__ size_t label_bytes(int cw, int ch) { return ((size_t)cw * ch + 255) & ~(size_t)255; }
inline size_t workspace_bytes(int n, long long tile_cap, int cw, int ch)
{
    return label_bytes(cw, ch) + (size_t)n * (size_t)tile_cap * 40;
}
inline Workspace carve(void *base, int n, long long tile_cap, int cw, int ch)
{
    Workspace W;
    unsigned char *p = static_cast<unsigned char *>(base);
    const size_t slots = (size_t)n * (size_t)tile_cap;
    W.label = p; p += label_bytes(cw, ch);
    W.lv[0] = reinterpret_cast<float4 *>(p); p += slots * 16;
    W.lv[1] = reinterpret_cast<float4 *>(p); p += slots * 16;
    W.m[0] = reinterpret_cast<float *>(p); p += slots * 4;
    W.m[1] = reinterpret_cast<float *>(p);
    return W;
}

}  // namespace nmb
