// nm_mosaic_exposure_math.hpp -- the arithmetic of the mosaic exposure compensation (nm_mosaic_exposure.hip), compiled for
// the device kernels and for the host twins alike: one lattice pixel of the per-channel overlap sums, and the gain solve's
// link terms, matrix rows, costs and outputs. The semantics are written out in include/nm_abi.h. A link's sums are
// integers, so they do not depend on the order in which pixels are added; every fp64 value of the solve is one written
// chain with explicit fma, run by one thread on the device and by one loop on the host.
#pragma once
#include "nm_chol_math.hpp"
#include "nm_common.hpp"
#include "nm_link_verify_math.hpp"
#include "../../include/nm_abi.h"

namespace nmx {

typedef unsigned long long u64;

constexpr int SUMS = NM_EXPOSURE_SUMS;      // N, Sa_B, Sa_G, Sa_R, Sb_B, Sb_G, Sb_R
constexpr int STATS = NM_EXPOSURE_STATS;    // cost at 1 (B, G, R), cost at the solution (B, G, R), links, frames, end
constexpr int MAX_FRAMES = NM_MOSAIC_MAX_BATCH, MAX_LINKS = NM_EXPOSURE_MAX_LINKS;
constexpr int LD = MAX_FRAMES + 1;          // leading dimension of the normal matrix: n columns and the right-hand side

struct Frames { const uchar4 *a, *b; const float *mask; int fw, fh; };
struct LinkIdx { unsigned char a[MAX_LINKS], b[MAX_LINKS]; };    // the host's link_a, link_b as kernel arguments
struct Params { int n, L, min_pixels, mode; double sigma_n, sigma_g; float g_min, g_max; };

__host__ __device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }

__host__ __device__ __forceinline__ bool in_range(uchar4 p, int lo, int hi)
{
    return p.x >= lo && p.x <= hi && p.y >= lo && p.y <= hi && p.z >= lo && p.z <= hi;
}

// Lattice pixel (x, y) of frame a into the link's seven sums. The gates are the verification's (mask at the pixel, the
// projection, the sampler, four taps inside b and seen by the mask), then the range test on all fifteen bytes.
__host__ __device__ __forceinline__ void add_pixel(const Frames &F, const float H[9], int lo, int hi, int x, int y,
                                                   u64 s[SUMS])
{
    const size_t p = (size_t)y * F.fw + x;
    if (!nml::mask_ok(F.mask, p)) return;
    int i, j;
    float w[4];
    if (!nml::lattice_taps(H, F.fw, F.fh, x, y, i, j, w)) return;
    const uchar4 pa = F.a[p];
    uchar4 pt[4];
    bool seen = true;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const size_t q = (size_t)(j + (t >> 1)) * F.fw + (i + (t & 1));
        pt[t] = F.b[q];
        seen = seen && nml::mask_ok(F.mask, q);
    }
    bool ok = seen && in_range(pa, lo, hi);
    unsigned acc[3] = {32768u, 32768u, 32768u};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const unsigned wt = (unsigned)(int)(w[t] * 65536.0f);    // w[t] is a multiple of 2^-16: exact
        ok = ok && in_range(pt[t], lo, hi);
        acc[0] += wt * pt[t].x; acc[1] += wt * pt[t].y; acc[2] += wt * pt[t].z;   // <= 65536 * 255 + 32768 < 2^32
    }
    if (!ok) return;
    s[0] += 1;
    s[1] += pa.x; s[2] += pa.y; s[3] += pa.z;
    s[4] += acc[0] >> 16; s[5] += acc[1] >> 16; s[6] += acc[2] >> 16;
}

// ---- the gain solve ----
__host__ __device__ __forceinline__ bool link_usable(const int *link_status, const u64 *sums, int l, int min_pixels)
{
    return (!link_status || link_status[l] == 1) && sums[(size_t)l * SUMS] >= (u64)min_pixels;
}

// What a usable link adds for system c (channel c, or the common system): abar, bbar, wn = N / sigma_n^2, wg = N / sigma_g^2
struct Terms { double abar, bbar, wn, wg; };
__host__ __device__ __forceinline__ Terms link_terms(const Params &P, const u64 *S, int c)
{
    const double N = (double)S[0];
    Terms T;
    if (P.mode == NM_EXPOSURE_COMMON) {
        T.abar = (((double)S[1] + (double)S[2]) + (double)S[3]) / (3.0 * N);
        T.bbar = (((double)S[4] + (double)S[5]) + (double)S[6]) / (3.0 * N);
    } else {
        T.abar = (double)S[1 + c] / N;
        T.bbar = (double)S[4 + c] / N;
    }
    T.wn = N / (P.sigma_n * P.sigma_n);
    T.wg = N / (P.sigma_g * P.sigma_g);
    return T;
}

// Row i of system c: the matrix entries M[i][0 .. n) and the right-hand side M[i][n], from +0, the usable links in
// ascending order. usable[l] != 0 marks them; deg[i] != 0 a frame with at least one. A frame with none gets 1 and 1.
__host__ __device__ inline void assemble_row(const Params &P, const LinkIdx &X, const u64 *sums, const unsigned char *usable,
                                             int c, int i, double *row)
{
    for (int q = 0; q <= P.n; ++q) row[q] = 0.0;
    bool any = false;
    for (int l = 0; l < P.L; ++l) {
        if (!usable[l]) continue;
        const int a = X.a[l], b = X.b[l];
        if (a != i && b != i) continue;
        const Terms T = link_terms(P, sums + (size_t)l * SUMS, c);
        const double own = a == i ? T.abar : T.bbar;
        row[i] = row[i] + fma_(T.wn * own, own, T.wg);
        row[a == i ? b : a] = row[a == i ? b : a] - (T.wn * T.abar) * T.bbar;
        row[P.n] = row[P.n] + T.wg;
        any = true;
    }
    if (!any) { row[i] = 1.0; row[P.n] = 1.0; }
}

// The cost of system c at the gains g (g == nullptr: all 1), the usable links in ascending order
__host__ __device__ inline double cost_of(const Params &P, const LinkIdx &X, const u64 *sums, const unsigned char *usable,
                                          int c, const double *g)
{
    double cost = 0.0;
    for (int l = 0; l < P.L; ++l) {
        if (!usable[l]) continue;
        const Terms T = link_terms(P, sums + (size_t)l * SUMS, c);
        const double ga = g ? g[X.a[l]] : 1.0, gb = g ? g[X.b[l]] : 1.0;
        const double e = fma_(ga, T.abar, -(gb * T.bbar)), da = 1.0 - ga, db = 1.0 - gb;
        cost = cost + fma_(T.wn * e, e, T.wg * fma_(da, da, db * db));
    }
    return cost;
}

__host__ __device__ __forceinline__ float clamp_gain(double g, float g_min, float g_max)
{
    const float f = (float)g;
    return f < g_min ? g_min : (f > g_max ? g_max : f);          // g is finite
}

// usable[], and the counts of usable links and of frames with one
__host__ __device__ inline void mark_links(const Params &P, const LinkIdx &X, const u64 *sums, const int *link_status,
                                           unsigned char *usable, int &links, int &frames)
{
    unsigned char deg[MAX_FRAMES];
    for (int k = 0; k < P.n; ++k) deg[k] = 0;
    links = 0;
    for (int l = 0; l < P.L; ++l) {
        usable[l] = link_usable(link_status, sums, l, P.min_pixels) ? 1 : 0;
        if (usable[l]) { ++links; deg[X.a[l]] = 1; deg[X.b[l]] = 1; }
    }
    frames = 0;
    for (int k = 0; k < P.n; ++k) frames += deg[k];
}

// The outputs of a call that ends without gains (NO_LINK, SINGULAR): all gains 1, both costs as given
__host__ __device__ inline void write_unit(const Params &P, float *gains, double *stats, const double cost1[3], int links,
                                           int frames, int end)
{
    for (int q = 0; q < 3 * P.n; ++q) gains[q] = 1.0f;
    for (int c = 0; c < 3; ++c) { stats[c] = cost1[c]; stats[3 + c] = cost1[c]; }
    stats[6] = (double)links; stats[7] = (double)frames; stats[8] = (double)end;
}

}  // namespace nmx
