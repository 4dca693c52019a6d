// nm_frame_quality_math.hpp -- the arithmetic of the frame-quality statistics and of the keyframe choice, written once for
// the kernels of nm_frame_quality.hip and the host twins (include/nm_abi.h, "Frame quality and keyframe choice", has the
// written definition). The statistics are integers; the choice is fp64 / fp32 in a fixed order, every operation a single
// IEEE operation (the build has -ffp-contract=off), so device and host agree bit for bit.
#pragma once
#include "nm_pair_batch.hpp"
#include "nm_warp_math.hpp"
#include "../../include/nm_abi.h"

namespace nmfq {

constexpr int MAX_FRAMES = NM_FRAME_QUALITY_MAX_BATCH, MAX_GRID = NM_FRAME_QUALITY_MAX_GRID;
constexpr int MAX_CELLS = MAX_GRID * MAX_GRID, WORDS = 8;
static_assert(MAX_FRAMES == 64 && MAX_CELLS == 64, "one lane per frame, one lane per cell in a wave of 64");
typedef unsigned long long u64;

enum { ELIG = 1, DARK = 2, BRIGHT = 4, GOOD = 8, HGOOD = 16 };      // a pixel's bits (HGOOD: both row neighbours good)

__host__ __device__ __forceinline__ int luma(int b, int g, int r) { return (7 * b + 72 * g + 21 * r + 50) / 100; }
__host__ __device__ __forceinline__ bool mask_u8(unsigned char m) { return m >= 128; }
__host__ __device__ __forceinline__ bool mask_f32(float m) { return m > 0.5f; }
__host__ __device__ __forceinline__ int cell_of(int x, int g, int f) { return (x * g) / f; }     // x < 2^15, g <= 8

__host__ __device__ __forceinline__ int classify(int b, int g, int r, bool elig, int lo, int hi)
{
    if (!elig) return 0;
    const int mg = b > g ? b : g, mx = mg > r ? mg : r;
    return ELIG | (mx < lo ? DARK : (mx > hi ? BRIGHT : GOOD));
}

// One measured pixel: Ya / Yb / Yc above, at and below it, hs = Y(x-1) + Y(x+1), hd = Y(x+1) - Y(x-1)
__host__ __device__ __forceinline__ void measure(int Ya, int Yb, int Yc, int hs, int hd, unsigned &L2, unsigned &G2)
{
    const int L = hs + (Ya + Yc) - 4 * Yb, dv = Yc - Ya;
    L2 = (unsigned)(L * L);                       // <= 1020^2 = 1 040 400
    G2 = (unsigned)(hd * hd + dv * dv);           // <= 2 * 255^2 = 130 050
}

// ---- the choice ----
struct Pick {
    int n, fw, fh, keep, gx, gy, w, carry;
    long long cell_min, min_pixels;
    double max_bad, rel;
    float d_min, d_max;
};

inline bool pick_ok(const Pick &p)
{
    return p.n >= 1 && p.n <= MAX_FRAMES && p.keep >= 1 && p.keep <= MAX_FRAMES && nm_size_ok(p.fw) && nm_size_ok(p.fh) &&
           p.gx >= 1 && p.gx <= MAX_GRID && p.gy >= 1 && p.gy <= MAX_GRID && p.w >= 0 && p.w <= 8 && p.cell_min >= 1 &&
           p.min_pixels >= 0 && p.max_bad >= 0.0 && p.max_bad <= 1.0 && p.rel >= 0.0 && p.rel <= 1.0 &&
           __builtin_isfinite(p.d_min) && __builtin_isfinite(p.d_max) && p.d_min >= 0.f && p.d_min <= p.d_max;
}

__host__ __device__ __forceinline__ bool cell_ok(u64 measured, long long cell_min) { return measured >= (u64)cell_min; }
__host__ __device__ __forceinline__ double sharp_of(u64 sumL2, u64 measured) { return (double)sumL2 / (double)measured; }
// the order of the median: by (value, cell index)
__host__ __device__ __forceinline__ bool before(double va, int ia, double vb, int ib) { return va < vb || (va == vb && ia < ib); }

__host__ __device__ __forceinline__ bool chain_row_ok(const float *M)
{
    bool zero = true;
    for (int q = 0; q < 9; ++q) zero = zero && M[q] == 0.f;
    return nmp::finite9(M) && !zero;
}

// A frame's flags before the blur test and sc[0 .. 2] = score, mean Y, bad fraction. cells: the frame's gy * gx * 8 words;
// score and nq: the lower median of the qualifying cells and their number.
__host__ __device__ inline int frame_flags(const Pick &p, const u64 *cells, double score, int nq, int status, const float *M,
                                           double *sc)
{
    u64 t0 = 0, t1 = 0, bad = 0, t7 = 0;
    for (int c = 0; c < p.gx * p.gy; ++c) {
        const u64 *w = cells + (size_t)c * WORDS;
        t0 += w[0]; t1 += w[1]; bad += w[5] + w[6]; t7 += w[7];
    }
    int f = 0;
    if (status != 1 || !chain_row_ok(M)) f |= NM_KEYFRAME_STATUS;
    if (nq == 0 || t0 < (u64)p.min_pixels) f |= NM_KEYFRAME_FEW;
    if (!((double)bad <= p.max_bad * (double)t7)) f |= NM_KEYFRAME_BAD;
    sc[0] = nq ? score : 0.0;
    sc[1] = t0 ? (double)t1 / (double)t0 : 0.0;
    sc[2] = t7 ? (double)bad / (double)t7 : 0.0;
    return f;
}

__host__ __device__ __forceinline__ bool usable0(int f) { return !(f & (NM_KEYFRAME_STATUS | NM_KEYFRAME_FEW | NM_KEYFRAME_BAD)); }
__host__ __device__ __forceinline__ bool usable(int f) { return usable0(f) && !(f & NM_KEYFRAME_BLURRED); }

// ref of frame k (the largest score of a frame usable before the blur test within w frames; 0 without one) and whether k
// is blurred. flags: the n pre-blur flags; score(j) = sc[4 j].
__host__ __device__ inline bool blurred(const Pick &p, int k, const int *flags, const double *sc, double &ref)
{
    ref = 0.0;
    const int j0 = k - p.w < 0 ? 0 : k - p.w, j1 = k + p.w > p.n - 1 ? p.n - 1 : k + p.w;
    for (int j = j0; j <= j1; ++j)
        if (usable0(flags[j]) && sc[4 * j] > ref) ref = sc[4 * j];
    return usable0(flags[k]) && sc[4 * k] < p.rel * ref;
}

// d(a, b): how far frame a's corners move between frame a and frame b, in pixels; +inf across a broken or degenerate map
__host__ __device__ inline float motion(const float *Ma, const float *Mb, int fw, int fh)
{
    float W[9];
    nmw::invert3x3(Ma, W);
    const float cx[4] = {0.f, (float)(fw - 1), 0.f, (float)(fw - 1)};
    const float cy[4] = {0.f, 0.f, (float)(fh - 1), (float)(fh - 1)};
    float d = 0.f;
    for (int k = 0; k < 4; ++k) {
        float px, py, qx, qy;
        const float s1 = nmw::project_den(W, cx[k], cy[k]);
        nmw::project(W, cx[k], cy[k], px, py);
        const float s2 = nmw::project_den(Mb, px, py);
        nmw::project(Mb, px, py, qx, qy);
        const float ex = __builtin_fabsf(qx - cx[k]), ey = __builtin_fabsf(qy - cy[k]);
        if (!(s1 > 0.f) || !(s2 > 0.f) || !__builtin_isfinite(ex) || !__builtin_isfinite(ey)) return __builtin_inff();
        d = ex > d ? ex : d;
        d = ey > d ? ey : d;
    }
    return d;
}

// H = (M_b W_a) / (M_b W_a)[8], the product in the order of the mosaic plan's link step; false (and a zero row) when a value
// is not finite or the normaliser is zero
__host__ __device__ inline bool key_map(const float *Ma, const float *Mb, float *H)
{
    float W[9], p[9];
    nmw::invert3x3(Ma, W);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            p[3 * r + c] = nmw::fmaf_(Mb[3 * r + 2], W[6 + c], nmw::fmaf_(Mb[3 * r + 1], W[3 + c], Mb[3 * r] * W[c]));
    const float s = p[8];
    bool ok = s != 0.f;
    for (int q = 0; q < 9; ++q) {
        H[q] = p[q] / s;
        ok = ok && __builtin_isfinite(p[q]) && __builtin_isfinite(H[q]);
    }
    if (!ok)
        for (int q = 0; q < 9; ++q) H[q] = 0.f;
    return ok;
}

}  // namespace nmfq
