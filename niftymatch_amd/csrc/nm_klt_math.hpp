// nm_klt_math.hpp -- the arithmetic of the gray pyramid and the pyramidal KLT point tracker (nm_klt.hip), compiled for the
// device kernels and for the host twins alike. include/nm_abi.h, "Gray pyramid and point tracking", has the written
// semantics. Everything that is summed is an integer, so the sums do not depend on how the taps of a window are divided
// among lanes or in which order they are added; the fp64 steps are single operations in the written order (the build has
// -ffp-contract=off). The tracker body `track` is written once over an executor X that says how many lanes share a point:
//   X::L              lanes per point; lane x.lane takes taps lane, lane + L, ... of a window
//   X::MAXT           taps per lane at the largest radius
//   x.sum(v)          the point's total of a 64-bit value, returned to every lane of the point
//   x.any(b)          true on every lane of the point when b holds on one of them
//   x.any_point(b)    true when b holds for any point that runs in lockstep with this one (the device's wave; the host: b)
// Every call of x.sum / x.any / x.any_point is reached by all lanes in lockstep: what a lost or absent point skips it skips
// by predicates, never by a branch round a reduction.
#pragma once
#include "nm_common.hpp"
#include "nm_pair_batch.hpp"
#include "nm_warp_math.hpp"
#include "../../include/nm_abi.h"

namespace nmk {

typedef long long i64;
typedef unsigned long long u64;

constexpr int MAX_LEVELS = NM_KLT_MAX_LEVELS, MAX_RADIUS = NM_KLT_MAX_RADIUS;
constexpr int MAX_TAPS = (2 * MAX_RADIUS + 1) * (2 * MAX_RADIUS + 1);
constexpr int LEVELS_PER_UNIT = 16;         // a gray value v in [0, 255] has the level rintf(16 v) in [0, 4080]
constexpr int SUMS = 6;                     // Gxx, Gxy, Gyy, bx, by, sum |e|
static_assert((i64)MAX_TAPS * 8160 * 8160 < (1ll << 34), "the sums' bound of nm_abi.h");

// ---- pyramid geometry: w_l = ceil(fw / 2^l); a level starts at the running sum of w h rounded up to 4 ----
__host__ __device__ __forceinline__ int level_size(int s, int l) { return (s + (1 << l) - 1) >> l; }
__host__ __device__ __forceinline__ i64 level_offset(int fw, int fh, int l)
{
    i64 off = 0;
    for (int j = 0; j < l; ++j) off += (((i64)level_size(fw, j) * level_size(fh, j)) + 3) & ~3ll;
    return off;
}
inline bool shape_ok(int fw, int fh, int levels)
{
    return nm_size_ok(fw) && nm_size_ok(fh) && levels >= 1 && levels <= MAX_LEVELS && level_size(fw, levels - 1) >= 2 &&
           level_size(fh, levels - 1) >= 2;
}

__host__ __device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the binomial filter (1 4 6 4 1) / 16 of five values, five single fp32 operations
__host__ __device__ __forceinline__ float binom5(float m2, float m1, float c, float p1, float p2)
{
    return (((m2 + p2) + 4.0f * (m1 + p1)) + 6.0f * c) * 0.0625f;
}

__host__ __device__ __forceinline__ bool seen_f32(float m) { return m > 0.5f; }

// ---- levels and the sampler ----
__host__ __device__ __forceinline__ bool level_of(float v, int &q)
{
    q = 0;
    if (!(v >= 0.f && v <= 255.f)) return false;                 // a NaN fails
    q = (int)__builtin_rintf(v * (float)LEVELS_PER_UNIT);
    return true;
}

// A window: the centre rounded to fp32 once, its integer part, and the four integer weights of its fractional part (a
// multiple of 1/256 per axis, the weights sum to 65536). Every tap of the window sits a whole number of pixels from the
// centre and shares the weights.
struct Win { int i0, j0; unsigned w00, w10, w01, w11; };

// false when the centre is not inside the w x h plane (a NaN fails) or a tap of the window of radius R would leave it
__host__ __device__ __forceinline__ bool window(int w, int h, float cx, float cy, int R, Win &W)
{
    W.i0 = W.j0 = 0; W.w00 = 65536u; W.w10 = W.w01 = W.w11 = 0u;
    if (!(cx >= 0.f && cx < (float)w && cy >= 0.f && cy < (float)h)) return false;
    const float fi = __builtin_floorf(cx), fj = __builtin_floorf(cy);
    const unsigned ax = (unsigned)(int)__builtin_floorf((cx - fi) * 256.0f + 0.5f);
    const unsigned ay = (unsigned)(int)__builtin_floorf((cy - fj) * 256.0f + 0.5f);
    W.i0 = (int)fi; W.j0 = (int)fj;
    W.w00 = (256u - ax) * (256u - ay); W.w10 = ax * (256u - ay); W.w01 = (256u - ax) * ay; W.w11 = ax * ay;
    return W.i0 - R >= 0 && W.i0 + R + 1 < w && W.j0 - R >= 0 && W.j0 + R + 1 < h;
}

// The sample at tap (u, v) of a window that lies inside the plane; bad is set when one of the four pixels holds no level or
// is not seen by the level's mask bytes m (NULL: no mask).
__host__ __device__ __forceinline__ int sample(const float *pl, const unsigned char *m, int w, const Win &W, int u, int v,
                                               bool &bad)
{
    const size_t o = (size_t)(W.j0 + v) * w + (size_t)(W.i0 + u);
    int q00, q10, q01, q11;
    bool ok = level_of(pl[o], q00);
    ok = level_of(pl[o + 1], q10) && ok;
    ok = level_of(pl[o + w], q01) && ok;
    ok = level_of(pl[o + w + 1], q11) && ok;
    if (m) ok = ok && (m[o] & m[o + 1] & m[o + w] & m[o + w + 1]) != 0;
    if (!ok) bad = true;
    // at most 65536 * 4080 + 32768 < 2^32
    return (int)((W.w00 * (unsigned)q00 + W.w10 * (unsigned)q10 + W.w01 * (unsigned)q01 + W.w11 * (unsigned)q11 + 32768u) >> 16);
}

// ---- the fp64 steps ----
__host__ __device__ __forceinline__ bool finite_pos(double v) { return __builtin_isfinite(v) && v > 0.0; }

// the texture gate; det is returned for the step, eig (the smaller eigenvalue per tap, gray^2; 0 where det fails) for the
// corner detector's score (nm_klt_corners_math.hpp)
__host__ __device__ __forceinline__ bool flat(i64 Gxx, i64 Gxy, i64 Gyy, int r, double min_eig, double &det, double &eig)
{
    const double a = (double)Gxx, b = (double)Gxy, c = (double)Gyy;
    const double t1 = a * c, t2 = b * b;
    det = t1 - t2;
    eig = 0.0;
    if (!finite_pos(det)) return true;
    const double s = a + c, dd = a - c, q = dd * dd, f = 4.0 * t2, root = __builtin_sqrt(q + f);
    const double lam = (s - root) / 2.0;
    eig = lam / (double)(1024 * (2 * r + 1) * (2 * r + 1));
    return eig < min_eig;
}
__host__ __device__ __forceinline__ bool flat(i64 Gxx, i64 Gxy, i64 Gyy, int r, double min_eig, double &det)
{
    double eig;
    return flat(Gxx, Gxy, Gyy, r, min_eig, det, eig);
}

__host__ __device__ __forceinline__ void step(i64 Gxx, i64 Gxy, i64 Gyy, i64 bx, i64 by, double det, double &sx, double &sy)
{
    const double a = (double)Gxx, b = (double)Gxy, c = (double)Gyy, x = (double)bx, y = (double)by;
    const double m1 = c * x, m2 = b * y, m3 = a * y, m4 = b * x;
    sx = 2.0 * (m1 - m2) / det;
    sy = 2.0 * (m3 - m4) / det;
}

__host__ __device__ __forceinline__ double absd(double v) { return v < 0.0 ? -v : v; }
__host__ __device__ __forceinline__ double maxabs(double a, double b) { a = absd(a); b = absd(b); return b > a ? b : a; }

// the start displacement of a row from a usable map; false: NM_KLT_START
__host__ __device__ __forceinline__ bool start_from(const float H[9], float sx, float sy, double &dx, double &dy)
{
    const float den = nmw::project_den(H, sx, sy);
    if (!(__builtin_isfinite(den) && den > 0.f)) return false;
    float xp, yp;
    nmw::project(H, sx, sy, xp, yp);
    if (!(__builtin_isfinite(xp) && __builtin_isfinite(yp))) return false;
    dx = (double)xp - (double)sx;
    dy = (double)yp - (double)sy;
    return true;
}

__host__ __device__ __forceinline__ bool row_tried(float sx, float sy)
{
    return sx >= 0.f && __builtin_isfinite(sx) && __builtin_isfinite(sy);
}

struct Params {
    int fw, fh, levels, r, iterations;
    double eps, max_step, min_eig, max_residual, fb_max;
};

inline bool params_ok(int fw, int fh, int levels, int r, int iterations, float eps, float max_step, float min_eig,
                      float max_residual, float fb_max)
{
    const bool fin = __builtin_isfinite(eps) && __builtin_isfinite(max_step) && __builtin_isfinite(min_eig) &&
                     __builtin_isfinite(max_residual) && __builtin_isfinite(fb_max);
    return shape_ok(fw, fh, levels) && r >= 1 && r <= MAX_RADIUS && iterations >= 1 && iterations <= NM_KLT_MAX_ITERATIONS &&
           fin && eps > 0.f && max_step > 0.f && min_eig >= 0.f && max_residual >= 0.f && fb_max >= 0.f;
}

inline Params params_of(int fw, int fh, int levels, int r, int iterations, float eps, float max_step, float min_eig,
                        float max_residual, float fb_max)
{
    Params q;
    q.fw = fw; q.fh = fh; q.levels = levels; q.r = r; q.iterations = iterations;
    q.eps = (double)eps; q.max_step = (double)max_step; q.min_eig = (double)min_eig; q.max_residual = (double)max_residual;
    q.fb_max = (double)fb_max;
    return q;
}

// The lane's taps of a template: T, gx, gy per tap, and the lane's part of Gxx, Gxy, Gyy. on: this lane's point is at work.
template <class X>
__host__ __device__ __forceinline__ void take_template(const X &x, bool on, const float *pl, const unsigned char *m, int w,
                                                       const Win &W, int r, int (&T)[X::MAXT], int (&gx)[X::MAXT],
                                                       int (&gy)[X::MAXT], i64 &Gxx, i64 &Gxy, i64 &Gyy, bool &bad)
{
    const int n1 = 2 * r + 1, taps = n1 * n1;
    Gxx = Gxy = Gyy = 0;
#pragma unroll
    for (int j = 0; j < X::MAXT; ++j) {
        const int t = x.lane + j * X::L;
        T[j] = gx[j] = gy[j] = 0;
        if (on && t < taps) {
            const int v = t / n1 - r, u = t - (v + r) * n1 - r;
            T[j] = sample(pl, m, w, W, u, v, bad);
            gx[j] = sample(pl, m, w, W, u + 1, v, bad) - sample(pl, m, w, W, u - 1, v, bad);
            gy[j] = sample(pl, m, w, W, u, v + 1, bad) - sample(pl, m, w, W, u, v - 1, bad);
            Gxx += (i64)(gx[j] * gx[j]); Gxy += (i64)(gx[j] * gy[j]); Gyy += (i64)(gy[j] * gy[j]);
        }
    }
}

// The lane's part of one evaluation against the other plane: bx = sum e gx, by = sum e gy, sabs = sum |e|, e = qb - T
template <class X>
__host__ __device__ __forceinline__ void take_mismatch(const X &x, bool on, const float *pl, const unsigned char *m, int w,
                                                       const Win &W, int r, const int (&T)[X::MAXT], const int (&gx)[X::MAXT],
                                                       const int (&gy)[X::MAXT], i64 &bx, i64 &by, i64 &sabs, bool &bad)
{
    const int n1 = 2 * r + 1, taps = n1 * n1;
    bx = by = sabs = 0;
#pragma unroll
    for (int j = 0; j < X::MAXT; ++j) {
        const int t = x.lane + j * X::L;
        if (on && t < taps) {
            const int v = t / n1 - r, u = t - (v + r) * n1 - r;
            const int e = sample(pl, m, w, W, u, v, bad) - T[j];
            bx += (i64)(e * gx[j]); by += (i64)(e * gy[j]); sabs += (i64)(e < 0 ? -e : e);
        }
    }
}

// One track of the point p (level-0 pixels of plane block A) into plane block B from the start displacement (dx, dy), in
// level-0 pixels. live: the point is tracked at all; the others walk along idle. On return reason is 0 or the NM_KLT_*
// code that lost the point, (dx, dy) the final displacement and resid the residual in gray values (where it was formed,
// else -1).
template <class X>
__host__ __device__ __forceinline__ void track(const X &x, const Params &q, const float *A, const float *B,
                                               const unsigned char *M, bool live, double px, double py, double &dx, double &dy,
                                               int &reason, double &resid)
{
    int T[X::MAXT], gx[X::MAXT], gy[X::MAXT];
    i64 Gxx = 0, Gxy = 0, Gyy = 0;
    const int r = q.r;
    const double down = 1.0 / (double)(1 << (q.levels - 1));
    dx = dx * down; dy = dy * down;
    reason = 0;
    resid = -1.0;
    bool run = live;
    for (int l = q.levels - 1; l >= 0; --l) {
        const int w = level_size(q.fw, l), h = level_size(q.fh, l);
        const i64 off = level_offset(q.fw, q.fh, l);
        const float *pa = A + off, *pb = B + off;
        const unsigned char *pm = M ? M + off : nullptr;
        const double s = 1.0 / (double)(1 << l), plx = px * s, ply = py * s, ex = dx, ey = dy;
        Win W;
        const bool okA = window(w, h, (float)plx, (float)ply, r + 1, W);
        bool bad = false;
        take_template(x, run && okA, pa, pm, w, W, r, T, gx, gy, Gxx, Gxy, Gyy, bad);
        Gxx = x.sum(Gxx); Gxy = x.sum(Gxy); Gyy = x.sum(Gyy);
        bad = x.any(bad);
        double det = 0.0;
        int fail = 0;
        if (!okA || bad) fail = NM_KLT_BORDER;
        else if (flat(Gxx, Gxy, Gyy, r, q.min_eig, det)) fail = NM_KLT_FLAT;
        bool iter = run && fail == 0;
        int it = 0;
        while (x.any_point(iter)) {
            const bool okB = window(w, h, (float)(plx + dx), (float)(ply + dy), r, W);
            i64 bx, by, sa;
            bad = false;
            take_mismatch(x, iter && okB, pb, pm, w, W, r, T, gx, gy, bx, by, sa, bad);
            bx = x.sum(bx); by = x.sum(by);
            bad = x.any(bad);
            if (iter) {
                double sx, sy;
                step(Gxx, Gxy, Gyy, bx, by, det, sx, sy);
                const double big = maxabs(sx, sy);
                if (!okB || bad) {
                    fail = NM_KLT_BORDER;
                    iter = false;
                } else if (!(__builtin_isfinite(sx) && __builtin_isfinite(sy)) || big > q.max_step) {
                    fail = NM_KLT_STEP;
                    iter = false;
                } else {
                    dx = dx - sx; dy = dy - sy;
                    ++it;
                    if (big < q.eps || it >= q.iterations) iter = false;
                }
            }
        }
        if (run && fail) {
            if (l > 0) { dx = ex; dy = ey; }
            else reason = fail;
        }
        run = live && reason == 0;
        if (l > 0) { dx = dx * 2.0; dy = dy * 2.0; }
    }
    // the residual at the final displacement, against level 0's template
    {
        Win W;
        const bool okB = window(q.fw, q.fh, (float)(px + dx), (float)(py + dy), r, W);
        i64 bx, by, sa;
        bool bad = false;
        take_mismatch(x, run && okB, B, M, q.fw, W, r, T, gx, gy, bx, by, sa, bad);
        sa = x.sum(sa);
        bad = x.any(bad);
        if (run) {
            if (!okB || bad) reason = NM_KLT_BORDER;
            else {
                resid = (double)sa / (double)(LEVELS_PER_UNIT * (2 * r + 1) * (2 * r + 1));
                if (q.max_residual > 0.0 && resid > q.max_residual) reason = NM_KLT_RESIDUAL;
            }
        }
    }
}

struct RowOut { float dst_x, dst_y, residual, fb_error; int reason; };

// One row: the start, the forward track, the result position and the forward-backward check. tried: the row exists and
// row_tried holds; H: the pair's usable start map or NULL.
template <class X>
__host__ __device__ __forceinline__ RowOut track_row(const X &x, const Params &q, const float *A, const float *B,
                                                     const unsigned char *M, bool tried, float sx, float sy, const float *H)
{
    RowOut o;
    o.dst_x = o.dst_y = o.residual = o.fb_error = -1.f;
    o.reason = tried ? 0 : NM_KLT_ABSENT;
    double dx = 0.0, dy = 0.0;
    if (tried && H && !start_from(H, sx, sy, dx, dy)) {
        o.reason = NM_KLT_START;
        dx = dy = 0.0;
    }
    const double px = (double)sx, py = (double)sy;
    int reason;
    double resid;
    track(x, q, A, B, M, o.reason == 0, px, py, dx, dy, reason, resid);
    if (o.reason == 0) {
        o.reason = reason;
        o.residual = (float)resid;
    }
    const float qx = (float)(px + dx), qy = (float)(py + dy);
    if (q.fb_max > 0.0) {                                           // the same for every row of a call
        double bx = -dx, by = -dy, back;
        track(x, q, B, A, M, o.reason == 0, (double)qx, (double)qy, bx, by, reason, back);
        if (o.reason == 0) {
            if (reason) o.reason = NM_KLT_FB;
            else {
                const float rx = (float)((double)qx + bx), ry = (float)((double)qy + by);
                const double err = maxabs((double)rx - (double)sx, (double)ry - (double)sy);
                o.fb_error = (float)err;
                if (err > q.fb_max) o.reason = NM_KLT_FB;
            }
        }
    }
    if (o.reason == 0) { o.dst_x = qx; o.dst_y = qy; }
    return o;
}

// the host's executor: one lane holds every tap
struct HostX {
    static constexpr int L = 1, MAXT = MAX_TAPS;
    int lane;
    i64 sum(i64 v) const { return v; }
    bool any(bool b) const { return b; }
    bool any_point(bool b) const { return b; }
};

}  // namespace nmk
