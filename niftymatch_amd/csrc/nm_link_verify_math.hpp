// nm_link_verify_math.hpp -- the arithmetic of the link verification (nm_link_verify.hip), compiled for the device kernels
// and for the host twin alike: the usable test, the corner geometry, one lattice pixel and the finalize from the seven
// integer sums. The semantics are written out in include/nm_abi.h. Everything a pair accumulates is an integer, so its sums
// do not depend on the order in which pixels are added; the fp64 finalize is one sequence with explicit fma.
#pragma once
#include "nm_common.hpp"
#include "nm_pair_batch.hpp"
#include "nm_warp_math.hpp"
#include "../../include/nm_abi.h"

namespace nml {

constexpr int SUMS = 7;                     // L, N, sum qa, sum qb, sum qa^2, sum qb^2, sum qa qb
constexpr int STATS = 8;                    // N, L, overlap, ncc, gain, bias, mean_a, mean_b
constexpr int LEVELS_PER_UNIT = 16;         // a gray value v in [0, 255] has the level rintf(16 v) in [0, 4080]

typedef unsigned long long u64;

struct Frames { const float *a, *b, *mask; int fw, fh; };

__host__ __device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }

// gate 1
__host__ __device__ __forceinline__ bool usable(int status_in, const float H[9]) { return status_in == 1 && nmp::finite9(H); }

// gate 3: the frame's corners through the map keep their orientation, stay convex and keep the area within the ratio
__host__ __device__ __forceinline__ bool geometry_ok(const float H[9], int fw, int fh, float max_area_ratio)
{
    const float cx[4] = {0.f, (float)fw, (float)fw, 0.f}, cy[4] = {0.f, 0.f, (float)fh, (float)fh};
    double x[4], y[4];
    bool ok = true;
    for (int c = 0; c < 4; ++c) {
        const float den = nmw::project_den(H, cx[c], cy[c]);
        ok = ok && __builtin_isfinite(den) && den > 0.f;
        float xp, yp;
        nmw::project(H, cx[c], cy[c], xp, yp);
        x[c] = (double)xp; y[c] = (double)yp;
    }
    if (!ok) return false;
    double ex[4], ey[4];
    for (int c = 0; c < 4; ++c) { ex[c] = x[(c + 1) & 3] - x[c]; ey[c] = y[(c + 1) & 3] - y[c]; }
    double S = 0.0;
    for (int c = 0; c < 4; ++c) {
        const int d = (c + 1) & 3;
        const double turn = fma_(ex[c], ey[d], -(ey[c] * ex[d]));
        ok = ok && turn > 0.0;                                   // a NaN fails
        S = S + fma_(x[c], y[d], -(x[d] * y[c]));
    }
    const double r = (0.5 * S) / ((double)fw * (double)fh);
    return ok && r >= 1.0 / (double)max_area_ratio && r <= (double)max_area_ratio;
}

__host__ __device__ __forceinline__ bool level_of(float v, int &q)
{
    if (!(v >= 0.f && v <= 255.f)) return false;                 // a NaN fails
    q = (int)__builtin_rintf(v * (float)LEVELS_PER_UNIT);
    return true;
}

__host__ __device__ __forceinline__ bool mask_ok(const float *mask, size_t p) { return !mask || mask[p] > 0.5f; }

// The projection half of lattice pixel (x, y), shared with the exposure sums (nm_mosaic_exposure_math.hpp): true when the
// denominator is finite and positive, the sampler accepts the projection on a fw x fh frame and its four taps (i, j),
// (i+1, j), (i, j+1), (i+1, j+1) lie inside it; w are the sampler's weights, multiples of 2^-16.
__host__ __device__ __forceinline__ bool lattice_taps(const float H[9], int fw, int fh, int x, int y, int &i, int &j,
                                                      float w[4])
{
    const float den = nmw::project_den(H, (float)x, (float)y);
    if (!(__builtin_isfinite(den) && den > 0.f)) return false;
    float xp, yp;
    nmw::project(H, (float)x, (float)y, xp, yp);
    const nmw::Tex tex{nullptr, fw, fh, NM_TEX_F32};
    if (!nmw::tex_setup(tex, xp + 0.5f, yp + 0.5f, i, j, w)) return false;
    return !(i < 0 || j < 0 || i + 1 >= fw || j + 1 >= fh);
}

// Lattice pixel (x, y) of A. 0: it counts nowhere; 1: into L; 2: into L and N, with its levels qa and qb.
__host__ __device__ __forceinline__ int pixel(const Frames &F, const float H[9], int x, int y, int &qa, int &qb)
{
    const size_t p = (size_t)y * F.fw + x;
    if (!mask_ok(F.mask, p) || !level_of(F.a[p], qa)) return 0;
    int i, j;
    float w[4];
    if (!lattice_taps(H, F.fw, F.fh, x, y, i, j, w)) return 1;
    unsigned acc = 32768u;
    for (int t = 0; t < 4; ++t) {
        const size_t q = (size_t)(j + (t >> 1)) * F.fw + (i + (t & 1));
        int qt;
        if (!mask_ok(F.mask, q) || !level_of(F.b[q], qt)) return 1;
        acc += (unsigned)(int)(w[t] * 65536.0f) * (unsigned)qt;  // w[t] is a multiple of 2^-16: the product is exact
    }
    qb = (int)(acc >> 16);                                       // acc <= 65536 * 4080 + 32768 < 2^32
    return 2;
}

__host__ __device__ __forceinline__ void add_pixel(const Frames &F, const float H[9], int x, int y, u64 s[SUMS])
{
    int qa = 0, qb = 0;
    const int c = pixel(F, H, x, y, qa, qb);
    if (c >= 1) s[0] += 1;
    if (c == 2) {
        s[1] += 1;
        s[2] += (u64)qa; s[3] += (u64)qb;
        s[4] += (u64)(qa * qa); s[5] += (u64)(qb * qb); s[6] += (u64)(qa * qb);
    }
}

// stats from the sums (each below 2^53: nm_abi.h bounds the lattice), and gate 4's two bits
__host__ __device__ __forceinline__ int finalize(const u64 s[SUMS], float min_overlap, float min_ncc, double out[STATS])
{
    const double L = (double)s[0], N = (double)s[1], Sa = (double)s[2], Sb = (double)s[3], Saa = (double)s[4],
                 Sbb = (double)s[5], Sab = (double)s[6];
    const double cov = fma_(N, Sab, -(Sa * Sb)), va = fma_(N, Saa, -(Sa * Sa)), vb = fma_(N, Sbb, -(Sb * Sb));
    const double overlap = s[0] ? N / L : 0.0;
    const double ncc = (s[1] >= 2 && va > 0.0 && vb > 0.0) ? cov / __builtin_sqrt(va * vb) : 0.0;
    const double gain = (s[1] >= 1 && va > 0.0) ? cov / va : 0.0;
    const double unit = (double)LEVELS_PER_UNIT * N;
    out[0] = N; out[1] = L; out[2] = overlap; out[3] = ncc; out[4] = gain;
    out[5] = s[1] ? fma_(-gain, Sa, Sb) / unit : 0.0;
    out[6] = s[1] ? Sa / unit : 0.0;
    out[7] = s[1] ? Sb / unit : 0.0;
    return (overlap < (double)min_overlap ? NM_LINK_LOW_OVERLAP : 0) | (ncc < (double)min_ncc ? NM_LINK_LOW_NCC : 0);
}

}  // namespace nml
