// nm_link_refine_math.hpp -- the arithmetic of the direct link refinement (nm_link_refine.hip), compiled for the device
// kernels and for the host twin alike: one lattice pixel's share of the 67 sums, one virtual lane's walk, the Cholesky
// solve, the step and the stop rule. The semantics are written out in include/nm_abi.h. The sums are fp64, so the order in
// which they are added is part of the result: walk_lane fixes a lane's order, the callers combine lanes, waves and rows of
// partials in the order nm_abi.h states. The accumulation multiplies and adds separately (the build has -ffp-contract=off);
// the solve and the step use explicit fma. Lattice, mask rule, levels and the sample of B are nml::pixel.
#pragma once
#include "nm_lattice.hpp"
#include "nm_link_verify_math.hpp"

namespace nmlr {

using nml::Frames;
using nml::fma_;

constexpr int COLS = 10;                    // Jacobian columns: 8 geometric, gain, bias
constexpr int TRI = COLS * (COLS + 1) / 2;  // upper triangle of J^T J, row-major (i <= j); entry (9, 9) is BIAS^2 N
constexpr int S_JTR = TRI, S_RR = TRI + COLS, S_L = S_RR + 1;
constexpr int SUMS = S_L + 1;               // 67
constexpr int STATS = NM_LINK_REFINE_STATS;
using nmlat::THREADS; using nmlat::WAVES; using nmlat::TILE_W; using nmlat::TILE_H; using nmlat::Lattice;
constexpr int PARTS = 256;                  // virtual workgroups = rows of partials per pair
constexpr int WORK = COLS * COLS + 2 * COLS;  // doubles of scratch for solve_system
constexpr double GAIN_SCALE = NM_LINK_REFINE_GAIN_SCALE, BIAS_SCALE = NM_LINK_REFINE_BIAS_SCALE;
constexpr double CONVERGED_STEP = NM_LINK_REFINE_CONVERGED_STEP;

struct Norm { double cx, cy, h; };          // X = (x - cx) / h, Y = (y - cy) / h
struct Params { int fw, fh, model, min_pixels; float max_step; };
struct State {                              // a pair's iterate between launches (workspace), 128 bytes
    double H[9];
    double rms_first;
    float Hf[9];                            // H rounded to fp32: what the next walk uses, and H_out
    int active, applied, pad;
};

__host__ __device__ __forceinline__ Norm norm_of(int fw, int fh)
{
    return Norm{0.5 * (double)(fw - 1), 0.5 * (double)(fh - 1), 0.5 * (double)(fw > fh ? fw : fh)};
}

__host__ __device__ __forceinline__ int tri(int i, int j) { return i * COLS - i * (i - 1) / 2 + (j - i); }  // i <= j

// a neighbour of a lattice pixel: inside A, seen by the mask, with a level
__host__ __device__ __forceinline__ bool neighbour(const Frames &F, int x, int y, int &q)
{
    if (x < 0 || x >= F.fw || y < 0 || y >= F.fh) return false;
    const size_t p = (size_t)y * F.fw + x;
    return nml::mask_ok(F.mask, p) && nml::level_of(F.a[p], q);
}

// Lattice pixel (x, y) with the normalised coordinates (X, Y) into the running sums of one virtual lane.
__host__ __device__ __forceinline__ void add_pixel(const Frames &F, const Norm &G, const float H[9], int x, int y, double X,
                                                   double Y, double s[SUMS])
{
    int qa = 0, qb = 0, qw = 0, qe = 0, qn = 0, qs = 0;
    const int c = nml::pixel(F, H, x, y, qa, qb);
    if (c >= 1) s[S_L] = s[S_L] + 1.0;
    if (c != 2) return;
    if (!(neighbour(F, x - 1, y, qw) && neighbour(F, x + 1, y, qe) && neighbour(F, x, y - 1, qn) &&
          neighbour(F, x, y + 1, qs)))
        return;
    const double gX = G.h * (0.5 * (double)(qe - qw)), gY = G.h * (0.5 * (double)(qs - qn));
    const double d = gX * X + gY * Y;
    const double J[COLS] = {gX * X, gX * Y, gX, gY * X, gY * Y, gY, -(X * d), -(Y * d), GAIN_SCALE * (double)qa, BIAS_SCALE};
    const double r = (double)(qb - qa);
    int e = 0;
#pragma unroll
    for (int i = 0; i < COLS; ++i)
#pragma unroll
        for (int j = i; j < COLS; ++j, ++e) s[e] = s[e] + J[i] * J[j];
#pragma unroll
    for (int i = 0; i < COLS; ++i) s[S_JTR + i] = s[S_JTR + i] + J[i] * r;
    s[S_RR] = s[S_RR] + r * r;
}

// Virtual lane (g, wave, lane) of the lattice walk, step PARTS, X once per column (one of three copies: nm_lattice.hpp)
__host__ __device__ __forceinline__ void walk_lane(const Frames &F, const Norm &G, const float H[9], int stride,
                                                   const Lattice L, int g, int wave, int lane, double s[SUMS])
{
    for (int t = g; t < L.tiles; t += PARTS) {
        const int u = (t % L.tiles_x) * TILE_W + lane, v0 = (t / L.tiles_x) * TILE_H;
        if (u >= L.lw) continue;
        const int x = stride * u + stride / 2;
        const double X = ((double)x - G.cx) / G.h;
        for (int r = wave; r < TILE_H && v0 + r < L.lh; r += WAVES) {
            const int y = stride * (v0 + r) + stride / 2;
            add_pixel(F, G, H, x, y, X, ((double)y - G.cy) / G.h, s);
        }
    }
}

__host__ __device__ __forceinline__ double count_of(const double tot[SUMS]) { return tot[TRI - 1] / (BIAS_SCALE * BIAS_SCALE); }

__host__ __device__ __forceinline__ int model_columns(int model, int idx[COLS])
{
    if (model == NM_LINK_REFINE_TRANSLATION) { idx[0] = 2; idx[1] = 5; idx[2] = 8; idx[3] = 9; return 4; }
    if (model == NM_LINK_REFINE_AFFINE) {
        for (int q = 0; q < 6; ++q) idx[q] = q;
        idx[6] = 8; idx[7] = 9;
        return 8;
    }
    for (int q = 0; q < COLS; ++q) idx[q] = q;
    return COLS;
}

// Cholesky of the model's rows and columns of J^T J, then the two substitutions. work: WORK doubles. false: a pivot that
// is not positive and finite, or a solution that is not finite. p: the eight geometric parameters (0 outside the model).
__host__ __device__ inline bool solve_system(const double tot[SUMS], int model, double *work, double p[8], double &alpha,
                                             double &beta)
{
    int idx[COLS];
    const int m = model_columns(model, idx);
    double *Lm = work, *y = work + COLS * COLS, *x = y + COLS;
    for (int j = 0; j < m; ++j) {
        double d = tot[tri(idx[j], idx[j])];
        for (int k = 0; k < j; ++k) d = fma_(-Lm[j * COLS + k], Lm[j * COLS + k], d);
        if (!(d > 0.0 && __builtin_isfinite(d))) return false;
        const double piv = __builtin_sqrt(d);
        Lm[j * COLS + j] = piv;
        for (int i = j + 1; i < m; ++i) {
            double v = tot[tri(idx[j], idx[i])];
            for (int k = 0; k < j; ++k) v = fma_(-Lm[i * COLS + k], Lm[j * COLS + k], v);
            Lm[i * COLS + j] = v / piv;
        }
    }
    for (int i = 0; i < m; ++i) {
        double v = tot[S_JTR + idx[i]];
        for (int k = 0; k < i; ++k) v = fma_(-Lm[i * COLS + k], y[k], v);
        y[i] = v / Lm[i * COLS + i];
    }
    for (int i = m - 1; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < m; ++k) v = fma_(-Lm[k * COLS + i], x[k], v);
        x[i] = v / Lm[i * COLS + i];
    }
    for (int q = 0; q < 8; ++q) p[q] = 0.0;
    bool ok = true;
    for (int i = 0; i < m; ++i) {
        ok = ok && __builtin_isfinite(x[i]);
        if (idx[i] < 8) p[idx[i]] = x[i];
    }
    alpha = x[m - 2]; beta = x[m - 1];
    return ok;
}

__host__ __device__ __forceinline__ void mul3(const double *P, const double *Q, double *R)
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = fma_(P[3 * r + 2], Q[6 + c], fma_(P[3 * r + 1], Q[3 + c], P[3 * r] * Q[c]));
}

// the adjugate of t: det(t) t^-1
__host__ __device__ __forceinline__ void adjugate3(const double *t, double *a)
{
    a[0] = fma_(t[4], t[8], -(t[7] * t[5]));
    a[1] = fma_(t[2], t[7], -(t[1] * t[8]));
    a[2] = fma_(t[1], t[5], -(t[2] * t[4]));
    a[3] = fma_(t[5], t[6], -(t[3] * t[8]));
    a[4] = fma_(t[0], t[8], -(t[2] * t[6]));
    a[5] = fma_(t[3], t[2], -(t[0] * t[5]));
    a[6] = fma_(t[3], t[7], -(t[6] * t[4]));
    a[7] = fma_(t[6], t[1], -(t[0] * t[7]));
    a[8] = fma_(t[0], t[4], -(t[3] * t[1]));
}

// M = T^-1 W T: the step in pixel coordinates, from the parameters in normalised ones
__host__ __device__ __forceinline__ void step_map(const double p[8], const Norm &G, double M[9])
{
    const double W[9] = {1.0 + p[0], p[1], p[2], p[3], 1.0 + p[4], p[5], p[6], p[7], 1.0};
    const double T[9] = {1.0 / G.h, 0.0, -(G.cx / G.h), 0.0, 1.0 / G.h, -(G.cy / G.h), 0.0, 0.0, 1.0};
    const double Ti[9] = {G.h, 0.0, G.cx, 0.0, G.h, G.cy, 0.0, 0.0, 1.0};
    double WT[9];
    mul3(W, T, WT);
    mul3(Ti, WT, M);
}

// the largest displacement of the four frame corners under M, in pixels; +inf when a corner does not stay in front
__host__ __device__ __forceinline__ double corner_step(const double M[9], int fw, int fh)
{
    const double cx[4] = {0.0, (double)fw, (double)fw, 0.0}, cy[4] = {0.0, 0.0, (double)fh, (double)fh};
    double step = 0.0;
    bool ok = true;
    for (int c = 0; c < 4; ++c) {
        const double den = fma_(M[6], cx[c], fma_(M[7], cy[c], M[8]));
        const double dx = fma_(M[0], cx[c], fma_(M[1], cy[c], M[2])) / den - cx[c];
        const double dy = fma_(M[3], cx[c], fma_(M[4], cy[c], M[5])) / den - cy[c];
        const double dist = __builtin_sqrt(fma_(dx, dx, dy * dy));
        ok = ok && den > 0.0 && __builtin_isfinite(dist);
        if (dist > step) step = dist;
    }
    return ok ? step : (double)__builtin_inff();
}

__host__ __device__ __forceinline__ void finish(const State &st, const float *H_in, int end, const double out[STATS],
                                                float *H_out, int *status_out, double *stats)
{
    for (int q = 0; q < 9; ++q) H_out[q] = st.applied > 0 ? st.Hf[q] : H_in[q];
    *status_out = st.applied > 0 ? 1 : 0;
    for (int q = 0; q < STATS; ++q) stats[q] = out[q];
    stats[6] = (double)st.applied;
    stats[8] = (double)end;
}

// Iteration `it` of `last + 1` for one pair, after its walk: tot are the 67 totals at st.Hf (at H_in when it == 0, where st
// is set up). A pair that ends here gets its outputs and st.active = 0; the caller skips an inactive pair from then on.
__host__ __device__ inline void step(const Params &P, int it, int last, const float *H_in, int status_in, const double tot[SUMS],
                                     double *work, State &st, float *H_out, int *status_out, double *stats)
{
    double out[STATS];
    for (int q = 0; q < STATS; ++q) out[q] = 0.0;
    if (it == 0) {
        st.applied = 0; st.pad = 0; st.rms_first = 0.0;
        for (int q = 0; q < 9; ++q) { st.H[q] = (double)H_in[q]; st.Hf[q] = H_in[q]; }
        st.active = nml::usable(status_in, H_in) ? 1 : 0;
        if (!st.active) {
            finish(st, H_in, NM_LINK_REFINE_END_UNUSABLE, out, H_out, status_out, stats);
            return;
        }
    }
    const Norm G = norm_of(P.fw, P.fh);
    const double N = count_of(tot);
    const double rms = N > 0.0 ? __builtin_sqrt(tot[S_RR] / N) / (double)nml::LEVELS_PER_UNIT : 0.0;
    if (it == 0) st.rms_first = rms;
    out[0] = N; out[1] = tot[S_L]; out[2] = st.rms_first; out[3] = rms;
    int end = -1;
    double p[8], alpha = 0.0, beta = 0.0;
    if (!(N >= (double)P.min_pixels)) {
        end = NM_LINK_REFINE_END_FEW_PIXELS;
    } else if (!solve_system(tot, P.model, work, p, alpha, beta)) {
        end = NM_LINK_REFINE_END_SINGULAR;
    } else {
        out[4] = fma_(GAIN_SCALE, alpha, 1.0);
        out[5] = (BIAS_SCALE * beta) / (double)nml::LEVELS_PER_UNIT;
        double M[9], A[9], Hn[9];
        step_map(p, G, M);
        const double size = corner_step(M, P.fw, P.fh);
        out[7] = size;
        adjugate3(M, A);
        mul3(st.H, A, Hn);
        bool ok = size <= (double)P.max_step;                    // a NaN fails
        const double s = Hn[8];
        for (int q = 0; q < 9; ++q) { Hn[q] = Hn[q] / s; ok = ok && __builtin_isfinite((float)Hn[q]); }   // also fp32 overflow
        if (!ok) {
            end = NM_LINK_REFINE_END_STEP;
        } else {
            for (int q = 0; q < 9; ++q) { st.H[q] = Hn[q]; st.Hf[q] = (float)Hn[q]; }
            st.applied += 1;
            if (size < CONVERGED_STEP) end = NM_LINK_REFINE_END_CONVERGED;
        }
    }
    if (end < 0 && it == last) end = NM_LINK_REFINE_END_ITERATIONS;
    if (end >= 0) {
        finish(st, H_in, end, out, H_out, status_out, stats);
        st.active = 0;
    }
}

}  // namespace nmlr
