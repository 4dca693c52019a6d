// nm_warp_math.hpp -- the warp arithmetic shared by nm_warp.hip (per-frame entries), nm_mosaic.hip (mosaic plan and
// batched blend) and nm_ingest.hip (batched frame ingest): the software bilinear sampler, the projective map, the 3x3
// inverse and the per-pixel blend step of transform_blend. One copy, so that the batched blend equals n per-frame
// transform_blend calls, and the ingest equals per-frame resamples, by construction. The build uses -ffp-contract=off
// and correctly rounded fp32 division; every multiply-add here is an explicit fmaf.
// project / invert3x3 / blend_combine are __host__ __device__: the mosaic plan's host twin runs the same sequence; so is
// tex_setup, for the host twin of the link verification (nm_link_verify_math.hpp).
#pragma once
#include "nm_common.hpp"
#include "../../include/nm_abi.h"

namespace nmw {

struct Tex { const void *data; int w, h, fmt; };

__host__ __device__ __forceinline__ float fmaf_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

template <int FMT>
__device__ __forceinline__ float texel(const Tex &t, int i, int j, int ch)
{
    if (i < 0 || i >= t.w || j < 0 || j >= t.h) return 0.f;
    const size_t p = (size_t)j * t.w + i;
    if (FMT == NM_TEX_F32) return ((const float *)t.data)[p];
    if (FMT == NM_TEX_U8N) return (float)((const unsigned char *)t.data)[p] / 255.0f;
    return (float)((const unsigned char *)t.data)[4 * p + ch] / 255.0f;
}

__host__ __device__ __forceinline__ bool tex_setup(const Tex &t, float x, float y, int &i, int &j, float w[4])
{
    const float xb = x - 0.5f, yb = y - 0.5f;
    if (!(xb >= -1.0f && xb < (float)t.w && yb >= -1.0f && yb < (float)t.h)) return false;
    const float fi = __builtin_floorf(xb), fj = __builtin_floorf(yb);
    const float a = __builtin_floorf((xb - fi) * 256.0f + 0.5f) * 0.00390625f;
    const float b = __builtin_floorf((yb - fj) * 256.0f + 0.5f) * 0.00390625f;
    i = (int)fi; j = (int)fj;
    w[0] = (1.0f - a) * (1.0f - b); w[1] = a * (1.0f - b); w[2] = (1.0f - a) * b; w[3] = a * b;
    return true;
}

template <int FMT>
__device__ __forceinline__ float tex2d(const Tex &t, float x, float y)
{
    int i, j; float w[4];
    if (!tex_setup(t, x, y, i, j, w)) return 0.f;
    return ((w[0] * texel<FMT>(t, i, j, 0) + w[1] * texel<FMT>(t, i + 1, j, 0)) + w[2] * texel<FMT>(t, i, j + 1, 0)) +
           w[3] * texel<FMT>(t, i + 1, j + 1, 0);
}

__device__ __forceinline__ float tex2d_any(const Tex &t, float x, float y)
{
    return t.fmt == NM_TEX_F32 ? tex2d<NM_TEX_F32>(t, x, y) : tex2d<NM_TEX_U8N>(t, x, y);
}

// uchar4 texture: one 4-byte load per tap, the four channels share the weights. Three steps, so that the batched
// ingest (nm_ingest.hip) runs setup and tap addressing once per pixel and the fetch and filter once per frame:
//   tex_taps_u8x4   the texel index and in-frame test of the 4 taps of tex_setup's (i, j)
//   tex_fetch_u8x4  the 4 loads (an out-of-frame tap reads as 0)
//   tex_filter_u8x4 c / 255 per channel, then the weighted sum in a fixed order
__device__ __forceinline__ void tex_taps_u8x4(const Tex &t, int i, int j, size_t off[4], bool in[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ii = i + (k & 1), jj = j + (k >> 1);
        in[k] = ii >= 0 && ii < t.w && jj >= 0 && jj < t.h;
        off[k] = in[k] ? (size_t)jj * t.w + ii : 0;
    }
}

__device__ __forceinline__ void tex_fetch_u8x4(const uchar4 *data, const size_t off[4], const bool in[4], uchar4 p[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = in[k] ? data[off[k]] : make_uchar4(0, 0, 0, 0);
}

__device__ __forceinline__ void tex_filter_u8x4(const uchar4 p[4], const float w[4], float out[4])
{
    float tap[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        tap[k][0] = (float)p[k].x / 255.0f; tap[k][1] = (float)p[k].y / 255.0f;
        tap[k][2] = (float)p[k].z / 255.0f; tap[k][3] = (float)p[k].w / 255.0f;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) out[c] = ((w[0] * tap[0][c] + w[1] * tap[1][c]) + w[2] * tap[2][c]) + w[3] * tap[3][c];
}

__device__ __forceinline__ void tex2d_u8x4(const Tex &t, float x, float y, float out[4])
{
    int i, j; float w[4];
    out[0] = out[1] = out[2] = out[3] = 0.f;
    if (!tex_setup(t, x, y, i, j, w)) return;
    size_t off[4]; bool in[4]; uchar4 p[4];
    tex_taps_u8x4(t, i, j, off, in);
    tex_fetch_u8x4((const uchar4 *)t.data, off, in, p);
    tex_filter_u8x4(p, w, out);
}

// the uchar4 result pixel of a sample, as resample_2D<uchar4> writes it
__device__ __forceinline__ uchar4 u8x4_of(const float s[4])
{
    return make_uchar4(nm_u8_sat(s[0] * 255.9999f), nm_u8_sat(s[1] * 255.9999f),
                       nm_u8_sat(s[2] * 255.9999f), nm_u8_sat(s[3] * 255.9999f));
}

// the denominator of project(m, x, y), same operations
__host__ __device__ __forceinline__ float project_den(const float *m, float x, float y)
{
    return fmaf_(m[6], x, m[7] * y) + m[8];
}

__host__ __device__ __forceinline__ void project(const float *m, float x, float y, float &xp, float &yp)
{
    const float a = fmaf_(m[0], x, m[1] * y) + m[2];
    const float b = fmaf_(m[3], x, m[4] * y) + m[5];
    const float s = fmaf_(m[6], x, m[7] * y) + m[8];
    xp = a / s; yp = b / s;
}

__host__ __device__ __forceinline__ void invert3x3(const float *t, float *inv)
{
    const float c0 = fmaf_(t[4], t[8], -(t[7] * t[5]));
    const float c1 = fmaf_(t[3], t[8], -(t[5] * t[6]));
    const float c2 = fmaf_(t[3], t[7], -(t[4] * t[6]));
    const float det = fmaf_(t[2], c2, fmaf_(t[0], c0, -(t[1] * c1)));
    const float invdet = 1.0f / det;
    inv[0] = c0 * invdet;
    inv[1] = fmaf_(t[2], t[7], -(t[1] * t[8])) * invdet;
    inv[2] = fmaf_(t[1], t[5], -(t[2] * t[4])) * invdet;
    inv[3] = fmaf_(t[5], t[6], -(t[3] * t[8])) * invdet;
    inv[4] = fmaf_(t[0], t[8], -(t[2] * t[6])) * invdet;
    inv[5] = fmaf_(t[3], t[2], -(t[0] * t[5])) * invdet;
    inv[6] = fmaf_(t[3], t[7], -(t[6] * t[4])) * invdet;
    inv[7] = fmaf_(t[6], t[1], -(t[0] * t[7])) * invdet;
    inv[8] = fmaf_(t[0], t[4], -(t[3] * t[1])) * invdet;
}

// The per-pixel blend step of transform_blend, in two halves so that a caller loads the canvas pixel only when the frame
// contributes. blend_sample: local grid pixel (x, y) under the map m; false when the frame gives this pixel nothing
// (projected at or beyond the frame's right / bottom edge, or mask <= 0.5), else the frame's colour r and weight nwt.
__device__ __forceinline__ bool blend_sample(const float *m, const Tex &frame, const Tex &mask, const Tex &wts, int x,
                                             int y, float r[4], float &nwt)
{
    float xp, yp;
    project(m, (float)x, (float)y, xp, yp);
    if (xp >= (float)frame.w || yp >= (float)frame.h) return false;
    const float u = xp + 0.5f, v = yp + 0.5f;
    if (tex2d_any(mask, u, v) <= 0.5f) return false;
    nwt = tex2d_any(wts, u, v);
    tex2d_u8x4(frame, u, v, r);
    return true;
}

// blend_combine: that sample into canvas pixel c of weight cwt (c is read only when cwt != 0)
__host__ __device__ __forceinline__ void blend_combine(const float r[4], float nwt, uchar4 &c, float &cwt)
{
    if (cwt == 0) {
        c = make_uchar4(nm_u8_sat(r[0] * 255.9999f), nm_u8_sat(r[1] * 255.9999f),
                        nm_u8_sat(r[2] * 255.9999f), 255);
        cwt = nwt;
    } else {
        const uchar4 cur = c;
        const float sum = cwt + nwt;
        c.x = nm_u8_sat(fmaf_(r[0] * nwt, 255.9999f, (float)cur.x * cwt) / sum);
        c.y = nm_u8_sat(fmaf_(r[1] * nwt, 255.9999f, (float)cur.y * cwt) / sum);
        c.z = nm_u8_sat(fmaf_(r[2] * nwt, 255.9999f, (float)cur.z * cwt) / sum);
        c.w = 255;
        cwt = sum;
    }
}

}  // namespace nmw
