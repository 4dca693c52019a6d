// nm_ransac_refit_math.hpp -- least-squares refit of a RANSAC winner over its inliers (nm_ransac_refit_batch_dev_f32 and its
// host twin), for gfx950. No reference counterpart. Everything here is __host__ __device__ and is the ONLY arithmetic of
// both entries, so host and device agree bit for bit: per-lane accumulation (lane l of nmf::LANES virtual lanes takes rows
// l, l + LANES, ... in ascending order), the moment matrix, the rotation parameters and the element updates of the
// Jacobi eigen-solve, and the three fits. All of it is fp64 with explicit fma (-ffp-contract=off); fp64 divide and sqrt
// are IEEE on both sides. The inlier test is nmr_is_inlier itself on the device and its literal sequence on the host.
// The eigenvector comes from a cyclic Jacobi in round-robin order written for this project (the reference's
// kernels/svd.cu is a GPL port of GSL and is not reproduced).
#pragma once
#include <hip/hip_runtime.h>

#include "nm_pair_batch.hpp"
#include "nm_ransac_math.hpp"

namespace nmf {

using nmp::clip;
using nmp::finite9;

constexpr int LANES = 512;                  // virtual lanes of the summation order = threads of the device workgroup
constexpr int WAVES = LANES / 64;
constexpr int NACC = 24;                    // the widest pass: the 24 moments of the DLT
constexpr int JACOBI_MAX_SWEEPS = 30;

enum { PASS_SUMS = 0, PASS_DIST = 1, PASS_SIM = 2, PASS_DLT = 3, PASS_RMS = 4 };
__host__ __device__ constexpr int pass_width(int kind)
{
    return kind == PASS_SUMS ? 5 : kind == PASS_DIST ? 2 : kind == PASS_SIM ? 3 : kind == PASS_DLT ? 24 : 1;
}

struct Pair {
    const float *sx, *sy, *dx, *dy;
    const int *mt;
    int nA;                                 // already clamped to [0, capA]
};

__host__ __device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }

__host__ __device__ __forceinline__ bool is_inlier(const float H[9], float sx, float sy, float dx, float dy, float thr)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return nmr_is_inlier(H, sx, sy, dx, dy, thr);
#else                                       /* nmr_is_inlier's sequence, for the host twin */
    float x = __builtin_fmaf(H[0], sx, H[1] * sy) + H[2];
    float y = __builtin_fmaf(H[3], sx, H[4] * sy) + H[5];
    const float z = __builtin_fmaf(H[6], sx, H[7] * sy) + H[8];
    x /= z; y /= z;
    const float ex = dx - x, ey = dy - y;
    return __builtin_fmaf(ex, ex, ey * ey) < thr;
#endif
}

/* Row i of the pair when it is a valid row (RANSAC's rule) and an inlier of H */
__host__ __device__ __forceinline__ bool inlier_row(const Pair &P, int i, const float H[9], float thr, float &x, float &y,
                                                    float &u, float &v)
{
    const int j = P.mt[i];
    x = P.sx[i];
    if (!(j >= 0 && x >= 0.f)) return false;
    y = P.sy[i]; u = P.dx[j]; v = P.dy[j];
    return is_inlier(H, x, y, u, v, thr);
}

/* One virtual lane's share of a pass: rows lane, lane + LANES, ... below nA, ascending. prm by kind:
 *   PASS_SUMS  -                       acc = count, sum sx, sum sy, sum dx, sum dy
 *   PASS_DIST  cx1 cy1 cx2 cy2         acc = sum |s - c1|, sum |d - c2|
 *   PASS_SIM   cx1 cy1 cx2 cy2         acc = sum Re conj(s_c) d_c, sum Im conj(s_c) d_c, sum |s_c|^2
 *   PASS_DLT   cx1 cy1 cx2 cy2 s1 s2   acc = P, bx P, by P, (bx^2 + by^2) P with P = (ax^2, ax ay, ax, ay^2, ay, 1)
 *   PASS_RMS   -                       acc = sum of squared fp64 reprojection distances                               */
template <int KIND>
__host__ __device__ __forceinline__ void accumulate(const Pair &P, const float H[9], float thr, int lane, const double *prm,
                                                    double *acc)
{
#pragma unroll
    for (int q = 0; q < pass_width(KIND); ++q) acc[q] = 0.0;
    for (int i = lane; i < P.nA; i += LANES) {
        float xf, yf, uf, vf;
        if (!inlier_row(P, i, H, thr, xf, yf, uf, vf)) continue;
        const double x = xf, y = yf, u = uf, v = vf;
        if (KIND == PASS_SUMS) {
            acc[0] += 1.0; acc[1] += x; acc[2] += y; acc[3] += u; acc[4] += v;
        } else if (KIND == PASS_DIST) {
            const double ax = x - prm[0], ay = y - prm[1], bx = u - prm[2], by = v - prm[3];
            acc[0] += __builtin_sqrt(fma_(ax, ax, ay * ay));
            acc[1] += __builtin_sqrt(fma_(bx, bx, by * by));
        } else if (KIND == PASS_SIM) {
            const double ax = x - prm[0], ay = y - prm[1], bx = u - prm[2], by = v - prm[3];
            acc[0] += fma_(ax, bx, ay * by);
            acc[1] += fma_(ax, by, -(ay * bx));
            acc[2] += fma_(ax, ax, ay * ay);
        } else if (KIND == PASS_DLT) {
            const double ax = (x - prm[0]) * prm[4], ay = (y - prm[1]) * prm[4];
            const double bx = (u - prm[2]) * prm[5], by = (v - prm[3]) * prm[5];
            const double w = fma_(bx, bx, by * by);
            const double p[6] = {ax * ax, ax * ay, ax, ay * ay, ay, 1.0};
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                acc[q] += p[q];
                acc[6 + q] = fma_(bx, p[q], acc[6 + q]);
                acc[12 + q] = fma_(by, p[q], acc[12 + q]);
                acc[18 + q] = fma_(w, p[q], acc[18 + q]);
            }
        } else {
            const double z = fma_((double)H[6], x, fma_((double)H[7], y, (double)H[8]));
            const double ex = u - fma_((double)H[0], x, fma_((double)H[1], y, (double)H[2])) / z;
            const double ey = v - fma_((double)H[3], x, fma_((double)H[4], y, (double)H[5])) / z;
            acc[0] += fma_(ex, ex, ey * ey);
        }
    }
}

/* ---- the fits, from the totals of the passes; each writes nine fp32 values (non-finite = unusable) ---- */
__host__ __device__ __forceinline__ void store9(const double h[9], float H[9])
{
    for (int q = 0; q < 9; ++q) H[q] = (float)h[q];
}

/* sums = count, sum sx, sum sy, sum dx, sum dy */
__host__ __device__ inline void fit_translation(const double *sums, float H[9])
{
    const double h[9] = {1.0, 0.0, (sums[3] - sums[1]) / sums[0], 0.0, 1.0, (sums[4] - sums[2]) / sums[0], 0.0, 0.0, 1.0};
    store9(h, H);
}

__host__ __device__ __forceinline__ void centroids(const double *sums, double *prm)
{
    prm[0] = sums[1] / sums[0]; prm[1] = sums[2] / sums[0]; prm[2] = sums[3] / sums[0]; prm[3] = sums[4] / sums[0];
}

/* a = m0 + i m1 over m2, t = c2 - a c1 */
__host__ __device__ inline void fit_similarity(const double *prm, const double *m, float H[9])
{
    const double ar = m[0] / m[2], ai = m[1] / m[2];
    const double tx = prm[2] - fma_(ar, prm[0], -(ai * prm[1]));
    const double ty = prm[3] - fma_(ai, prm[0], ar * prm[1]);
    const double h[9] = {ar, -ai, tx, ai, ar, ty, 0.0, 0.0, 1.0};
    store9(h, H);
}

/* Hartley scales from the totals of PASS_DIST: mean distance from the centroid -> sqrt(2) */
__host__ __device__ __forceinline__ void hartley_scales(const double *sums, const double *dist, double *prm)
{
    prm[4] = __builtin_sqrt(2.0) / (dist[0] / sums[0]);
    prm[5] = __builtin_sqrt(2.0) / (dist[1] / sums[0]);
}

/* Entry (r, c) of the 9 x 9 moment matrix A^T A of the DLT (rows (0, -p, by p) and (p, 0, -bx p) per inlier) from the 24 totals */
__host__ __device__ inline double dlt_entry(const double *m, int r, int c)
{
    const int br = r / 3, bc = c / 3, pr = r % 3, pc = c % 3;
    const int lo = pr < pc ? pr : pc, hi = pr < pc ? pc : pr;
    const int idx = lo == 0 ? hi : (lo == 1 ? 2 + hi : 5);          /* (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) -> 0..5 */
    if (br == bc) return br < 2 ? m[idx] : m[18 + idx];
    if (br + bc == 1) return 0.0;
    return (br + bc == 2) ? -m[6 + idx] : -m[12 + idx];
}

/* Round-robin order on 9 indices: in step t (0 .. 8) index t rests and (t + k) % 9 meets (t - k) % 9, k = 1 .. 4; the nine
 * steps of a sweep visit each of the 36 pairs once, and the four rotations of a step touch disjoint rows and columns. */
__host__ __device__ __forceinline__ int jacobi_partner(int t, int i)
{
    if (i == t) return i;
    const int k = (i - t + 9) % 9;
    return k <= 4 ? (t - k + 9) % 9 : (t + 9 - k) % 9;
}

/* Rotation that annihilates a_pq (Golub & Van Loan, Matrix Computations, 8.5: J^T A J with J_pp = J_qq = c, J_pq = s,
 * J_qp = -s). false (c = 1, s = 0) when a_pq is already negligible against its diagonal entries. */
__host__ __device__ inline bool jacobi_rotation(double app, double aqq, double apq, double &c, double &s)
{
    c = 1.0; s = 0.0;
    if (apq == 0.0 || !(__builtin_fabs(apq) > 0x1p-52 * __builtin_sqrt(__builtin_fabs(app) * __builtin_fabs(aqq))))
        return false;
    const double zeta = (aqq - app) / (2.0 * apq);
    const double t = ((zeta >= 0.0) ? 1.0 : -1.0) / (__builtin_fabs(zeta) + __builtin_sqrt(fma_(zeta, zeta, 1.0)));
    if (!__builtin_isfinite(t)) return false;
    c = 1.0 / __builtin_sqrt(fma_(t, t, 1.0));
    s = c * t;
    return true;
}

/* New value of the element in column (or row) `self` of a pair (p < q), from the old elements xp, xq of columns (rows) p, q */
__host__ __device__ __forceinline__ double jacobi_mix(bool self_is_p, double xp, double xq, double c, double s)
{
    return self_is_p ? fma_(c, xp, -(s * xq)) : fma_(s, xp, c * xq);
}

/* From the eigenvector h (normalised coordinates) to the fp32 map: inv(T2) Hn T1, then divided by its last entry.
 * prm = cx1 cy1 cx2 cy2 s1 s2 */
__host__ __device__ inline void denormalise(const double *hn, const double *prm, float H[9])
{
    const double cx1 = prm[0], cy1 = prm[1], cx2 = prm[2], cy2 = prm[3], s1 = prm[4], s2 = prm[5];
    double M[9], o[9];
    for (int r = 0; r < 3; ++r) {
        M[3 * r] = s1 * hn[3 * r];
        M[3 * r + 1] = s1 * hn[3 * r + 1];
        M[3 * r + 2] = hn[3 * r + 2] - s1 * fma_(hn[3 * r], cx1, hn[3 * r + 1] * cy1);
    }
    for (int c = 0; c < 3; ++c) {
        o[c] = fma_(cx2, M[6 + c], M[c] / s2);
        o[3 + c] = fma_(cy2, M[6 + c], M[3 + c] / s2);
        o[6 + c] = M[6 + c];
    }
    double h[9];
    for (int q = 0; q < 8; ++q) h[q] = o[q] / o[8];
    h[8] = (o[8] == 0.0 || !__builtin_isfinite(o[8])) ? o[8] / o[8] : 1.0;     /* NaN marks the unusable map */
    store9(h, H);
}

/* Index of the smallest diagonal entry (first minimum) */
__host__ __device__ __forceinline__ int smallest_diagonal(const double *A)
{
    int best = 0;
    for (int j = 1; j < 9; ++j)
        if (A[10 * j] < A[10 * best]) best = j;
    return best;
}

/* The fp32 RMS reprojection distance from the total of PASS_RMS */
__host__ __device__ __forceinline__ float rms_of(double total, double count)
{
    return count > 0.0 ? (float)__builtin_sqrt(total / count) : 0.f;
}

}  // namespace nmf
