// nm_mosaic_adjust_math.hpp -- the arithmetic of the global adjustment of a mosaic's frame maps (nm_mosaic_adjust.hip),
// compiled for the device kernels and for the host twin alike: a frame's normalised map from its chain row and back, one
// row's residual and Jacobians, one virtual lane's walk over a slice of the 153 sums, and the two serial halves of a round
// (begin_round: totals, cost rule, end reasons, outputs; finish_round: step size and update). The semantics are written
// out in include/nm_abi.h. The sums are fp64, so the order in which they are added is part of the result: walk_lane fixes
// a lane's order, the callers combine lanes and waves as nm_abi.h states. The accumulation multiplies and adds separately
// (the build has -ffp-contract=off); maps, solve and step use explicit fma.
#pragma once
#include "nm_link_refine_math.hpp"
#include "nm_pair_batch.hpp"

namespace nmma {

using nml::fma_;
using nmlr::adjugate3;
using nmlr::mul3;

constexpr int MAX_FRAMES = 64, MAX_LINKS = NM_MOSAIC_ADJUST_MAX_LINKS;
constexpr int GROUP = nmp::MAX_BATCH;       // links per accumulate launch
constexpr int LANES = 512, WAVES = LANES / 64;   // the refit's virtual lanes
constexpr int COLS = 16;                    // Jacobian columns of a link: frame a's eight, then frame b's eight
constexpr int TRI = COLS * (COLS + 1) / 2;  // upper triangle of J^T J by rows (i <= j)
constexpr int S_JTR = TRI, S_RR = TRI + COLS, SUMS = S_RR + 1;   // 153
constexpr int S_COUNT = SUMS, ROW = SUMS + 1;                    // a link's row in the workspace: the sums, then the count
constexpr int SLICES = 4, SLICE_W = 39;     // slice s accumulates the sums [39 s, 39 s + 39)
constexpr int MAX_UNKNOWNS = 8 * (MAX_FRAMES - 1);
constexpr int STATS = NM_MOSAIC_ADJUST_STATS;
constexpr double CONVERGED_STEP = NM_MOSAIC_ADJUST_CONVERGED_STEP;
static_assert(SUMS == NM_MOSAIC_ADJUST_SUMS && SLICES * SLICE_W >= SUMS && MAX_UNKNOWNS + 1 <= LANES, "layout of nm_abi.h");

struct Norm { double cx, cy, h; };          // X = (x - cx) / h, Y = (y - cy) / h, for pixels and mosaic coordinates alike
struct Params { int n, L, anchor, fw, fh, iterations, min_rows; double damping, max_step; };
struct LinkIdx { unsigned char a[MAX_LINKS], b[MAX_LINKS]; };    // the host's link_a, link_b as kernel arguments
struct Link {                               // one link's rows
    const float *sx, *sy, *dx, *dy;
    const int *mt;
    const unsigned char *mask;              // the link's capA bytes, or null
    int nA;                                 // already clipped to [0, capA]
};
struct Out { float *chain_out; int *frame_status; double *link_rms; double *stats; };
struct State {
    double cost_first, cost_cur, last_step;
    long long rows;
    int ended, reason, applied, pending, unknowns, usable_links;
};
struct Small {                              // the part of the workspace behind the link rows and the normal matrix
    double cur[MAX_FRAMES][9], prev[MAX_FRAMES][9];              // the iterate and the one before: normalised maps
    double delta[LANES];
    double rms_first[MAX_LINKS], rms_cur[MAX_LINKS], rms_prev[MAX_LINKS];
    int usable[MAX_LINKS], fstat[MAX_FRAMES], slot[MAX_FRAMES];
    State st;
};

__host__ __device__ __forceinline__ Norm norm_of(int fw, int fh)
{
    return Norm{0.5 * (double)fw, 0.5 * (double)fh, 0.5 * (double)(fw > fh ? fw : fh)};
}

__host__ __device__ __forceinline__ int tri(int i, int j) { return i * COLS - i * (i - 1) / 2 + (j - i); }  // i <= j

// column c has an entry in the Jacobian's x row / y row (the others are structurally zero)
__host__ __device__ constexpr bool has_x(int c) { return (c & 7) < 3 || (c & 7) >= 6; }
__host__ __device__ constexpr bool has_y(int c) { return (c & 7) >= 3; }

__host__ __device__ __forceinline__ bool finite9d(const double *m)
{
    bool ok = true;
    for (int q = 0; q < 9; ++q) ok = ok && __builtin_isfinite(m[q]);
    return ok;
}

__host__ __device__ __forceinline__ void norm_maps(const Norm &N, double T[9], double Ti[9])
{
    const double t[9] = {1.0 / N.h, 0.0, -(N.cx / N.h), 0.0, 1.0 / N.h, -(N.cy / N.h), 0.0, 0.0, 1.0};
    const double ti[9] = {N.h, 0.0, N.cx, 0.0, N.h, N.cy, 0.0, 0.0, 1.0};
    for (int q = 0; q < 9; ++q) { T[q] = t[q]; Ti[q] = ti[q]; }
}

// inv = adj(m) / det(m), then every element over inv[8]
__host__ __device__ __forceinline__ void inverse_scaled(const double *m, double *out)
{
    double a[9];
    adjugate3(m, a);
    const double det = fma_(m[0], a[0], fma_(m[1], a[3], m[2] * a[6]));
    for (int q = 0; q < 9; ++q) a[q] = a[q] / det;
    const double s = a[8];
    for (int q = 0; q < 9; ++q) out[q] = a[q] / s;
}

// A chain row (mosaic coordinates -> frame pixels) to the frame's normalised map; 1: the frame participates
__host__ __device__ inline int init_frame(const float *row, const Norm &N, double Gh[9])
{
    double m[9], G[9], T[9], Ti[9], GTi[9], P[9];
    for (int q = 0; q < 9; ++q) m[q] = (double)row[q];
    inverse_scaled(m, G);
    norm_maps(N, T, Ti);
    mul3(G, Ti, GTi);
    mul3(T, GTi, P);
    const double s = P[8];
    for (int q = 0; q < 9; ++q) Gh[q] = P[q] / s;
    return (nmp::finite9(row) && finite9d(G) && finite9d(Gh)) ? 1 : 0;
}

// A normalised map back to the chain row, rounded to fp32; false when a value is not finite in fp32
__host__ __device__ inline bool row_of(const double Gh[9], const Norm &N, float row[9])
{
    double T[9], Ti[9], GT[9], G[9], M[9];
    norm_maps(N, T, Ti);
    mul3(Gh, T, GT);
    mul3(Ti, GT, G);
    inverse_scaled(G, M);
    bool ok = true;
    for (int q = 0; q < 9; ++q) { row[q] = (float)M[q]; ok = ok && __builtin_isfinite(row[q]); }
    return ok;
}

// The largest displacement in pixels of the frame's corners between two normalised maps; +inf when a corner is not in
// front of both or a displacement is not finite
__host__ __device__ inline double frame_step(const double *Go, const double *Gn, const Norm &N, int fw, int fh)
{
    const double cx[4] = {0.0, (double)fw, (double)fw, 0.0}, cy[4] = {0.0, 0.0, (double)fh, (double)fh};
    double step = 0.0;
    bool ok = true;
    for (int c = 0; c < 4; ++c) {
        const double X = (cx[c] - N.cx) / N.h, Y = (cy[c] - N.cy) / N.h;
        const double d0 = fma_(Go[6], X, fma_(Go[7], Y, Go[8])), d1 = fma_(Gn[6], X, fma_(Gn[7], Y, Gn[8]));
        const double dx = fma_(Gn[0], X, fma_(Gn[1], Y, Gn[2])) / d1 - fma_(Go[0], X, fma_(Go[1], Y, Go[2])) / d0;
        const double dy = fma_(Gn[3], X, fma_(Gn[4], Y, Gn[5])) / d1 - fma_(Go[3], X, fma_(Go[4], Y, Go[5])) / d0;
        const double dist = N.h * __builtin_sqrt(fma_(dx, dx, dy * dy));
        ok = ok && d0 > 0.0 && d1 > 0.0 && __builtin_isfinite(dist);
        if (dist > step) step = dist;
    }
    return ok ? step : (double)__builtin_inff();
}

// Row i of a link: false when it does not contribute (outside V_k, masked out, or a denominator that is not finite and > 0)
__host__ __device__ __forceinline__ bool row_jacobian(const Link &K, const Norm &N, const double *Ga, const double *Gb, int i,
                                                      double Jx[COLS], double Jy[COLS], double &rx, double &ry)
{
    const int j = K.mt[i];
    const float xf = K.sx[i];
    if (!(j >= 0 && xf >= 0.f)) return false;
    if (K.mask && K.mask[i] == 0) return false;
    const double px = ((double)xf - N.cx) / N.h, py = ((double)K.sy[i] - N.cy) / N.h;
    const double qx = ((double)K.dx[j] - N.cx) / N.h, qy = ((double)K.dy[j] - N.cy) / N.h;
    const double da = (Ga[6] * px + Ga[7] * py) + Ga[8], db = (Gb[6] * qx + Gb[7] * qy) + Gb[8];
    if (!(da > 0.0 && __builtin_isfinite(da) && db > 0.0 && __builtin_isfinite(db))) return false;
    const double ux = ((Ga[0] * px + Ga[1] * py) + Ga[2]) / da, uy = ((Ga[3] * px + Ga[4] * py) + Ga[5]) / da;
    const double vx = ((Gb[0] * qx + Gb[1] * qy) + Gb[2]) / db, vy = ((Gb[3] * qx + Gb[4] * qy) + Gb[5]) / db;
    rx = ux - vx; ry = uy - vy;
    const double ax = px / da, ay = py / da, a1 = 1.0 / da, bx = qx / db, by = qy / db, b1 = 1.0 / db;
    Jx[0] = ax; Jx[1] = ay; Jx[2] = a1; Jx[3] = 0.0; Jx[4] = 0.0; Jx[5] = 0.0;
    Jx[6] = (-(ux * px)) / da; Jx[7] = (-(ux * py)) / da;
    Jy[0] = 0.0; Jy[1] = 0.0; Jy[2] = 0.0; Jy[3] = ax; Jy[4] = ay; Jy[5] = a1;
    Jy[6] = (-(uy * px)) / da; Jy[7] = (-(uy * py)) / da;
    Jx[8] = -bx; Jx[9] = -by; Jx[10] = -b1; Jx[11] = 0.0; Jx[12] = 0.0; Jx[13] = 0.0;
    Jx[14] = -((-(vx * qx)) / db); Jx[15] = -((-(vx * qy)) / db);
    Jy[8] = 0.0; Jy[9] = 0.0; Jy[10] = 0.0; Jy[11] = -bx; Jy[12] = -by; Jy[13] = -b1;
    Jy[14] = -((-(vy * qx)) / db); Jy[15] = -((-(vy * qy)) / db);
    return true;
}

// One contributing row into the running sums of slice SLICE: s[e - SLICE_W SLICE] for the sums e of the slice. An entry
// whose columns share neither the x row nor the y row is structurally zero and is skipped (it stays +0).
template <int SLICE>
__host__ __device__ __forceinline__ void add_row(const double Jx[COLS], const double Jy[COLS], double rx, double ry,
                                                 double s[SLICE_W])
{
    constexpr int E0 = SLICE * SLICE_W, E1 = E0 + SLICE_W;
    int e = 0;
#pragma unroll
    for (int i = 0; i < COLS; ++i)
#pragma unroll
        for (int j = i; j < COLS; ++j, ++e) {
            const bool x = has_x(i) && has_x(j), y = has_y(i) && has_y(j);
            if (e < E0 || e >= E1 || !(x || y)) continue;
            double t = x ? Jx[i] * Jx[j] : Jy[i] * Jy[j];
            if (x && y) t = t + Jy[i] * Jy[j];
            s[e - E0] = s[e - E0] + t;
        }
#pragma unroll
    for (int i = 0; i < COLS; ++i) {
        const int q = S_JTR + i;
        if (q < E0 || q >= E1) continue;
        double t = has_x(i) ? Jx[i] * rx : Jy[i] * ry;
        if (has_x(i) && has_y(i)) t = t + Jy[i] * ry;
        s[q - E0] = s[q - E0] + t;
    }
    if (S_RR >= E0 && S_RR < E1) s[S_RR - E0] = s[S_RR - E0] + (rx * rx + ry * ry);
}

// Virtual lane `lane` of LANES: the rows lane, lane + LANES, .. below nA, ascending; returns its contributing rows
template <int SLICE>
__host__ __device__ __forceinline__ int walk_lane(const Link &K, const Norm &N, const double *Ga, const double *Gb, int lane,
                                                  double s[SLICE_W])
{
#pragma unroll
    for (int q = 0; q < SLICE_W; ++q) s[q] = 0.0;
    int count = 0;
    for (int i = lane; i < K.nA; i += LANES) {
        double Jx[COLS], Jy[COLS], rx, ry;
        if (!row_jacobian(K, N, Ga, Gb, i, Jx, Jy, rx, ry)) continue;
        add_row<SLICE>(Jx, Jy, rx, ry, s);
        ++count;
    }
    return count;
}

// ---- the serial halves of a round, run by one lane on the device and as they are on the host ----

__host__ __device__ inline bool end_call(const Params &P, int reason, const float *chain_in, Small &W, const Out &O)
{
    State &st = W.st;
    st.ended = 1;
    st.reason = reason;
    const Norm N = norm_of(P.fw, P.fh);
    for (int k = 0; k < P.n; ++k) {
        float row[9];
        const bool moved = st.applied > 0 && W.fstat[k] && k != P.anchor;
        if (moved) row_of(W.cur[k], N, row);
        for (int q = 0; q < 9; ++q) O.chain_out[9 * k + q] = moved ? row[q] : chain_in[9 * k + q];
        O.frame_status[k] = W.fstat[k];
    }
    for (int l = 0; l < P.L; ++l) {
        O.link_rms[2 * l] = W.usable[l] ? W.rms_first[l] : 0.0;
        O.link_rms[2 * l + 1] = W.usable[l] ? W.rms_cur[l] : 0.0;
    }
    const double out[STATS] = {st.cost_first, st.cost_cur, (double)st.rows, (double)st.usable_links, (double)st.unknowns,
                               (double)st.applied, st.last_step, (double)reason};
    for (int q = 0; q < STATS; ++q) O.stats[q] = out[q];
    return false;
}

// Before the solve of round t: `rows` hold the sums at the current iterate. true: assemble and solve; false: the call has
// ended (now or earlier) and its outputs are written.
__host__ __device__ inline bool begin_round(const Params &P, int t, const LinkIdx &X, const int *link_status,
                                            const float *chain_in, const double *rows, Small &W, const Out &O)
{
    State &st = W.st;
    const Norm N = norm_of(P.fw, P.fh);
    if (t == 0) {
        st.cost_first = st.cost_cur = st.last_step = 0.0;
        st.rows = 0;
        st.ended = st.reason = st.applied = st.pending = st.unknowns = st.usable_links = 0;
        for (int k = 0; k < P.n; ++k) {
            W.fstat[k] = init_frame(chain_in + 9 * k, N, W.cur[k]);
            for (int q = 0; q < 9; ++q) W.prev[k][q] = W.cur[k][q];
            W.slot[k] = (W.fstat[k] && k != P.anchor) ? st.unknowns++ : -1;
        }
        for (int l = 0; l < P.L; ++l) {
            W.usable[l] = 0;
            W.rms_first[l] = W.rms_cur[l] = W.rms_prev[l] = 0.0;
        }
        if (!W.fstat[P.anchor]) return end_call(P, NM_MOSAIC_ADJUST_END_UNUSABLE, chain_in, W, O);
    } else if (st.ended) {
        return false;
    }
    double cost = 0.0;
    long long count = 0;
    int usable = 0;
    for (int l = 0; l < P.L; ++l) {
        if (t == 0)
            W.usable[l] = ((!link_status || link_status[l] == 1) && W.fstat[X.a[l]] && W.fstat[X.b[l]] &&
                           rows[(size_t)l * ROW + S_COUNT] >= (double)P.min_rows) ? 1 : 0;
        if (!W.usable[l]) continue;
        const double rr = rows[(size_t)l * ROW + S_RR], c = rows[(size_t)l * ROW + S_COUNT];
        cost = cost + rr;
        count += (long long)c;
        ++usable;
        W.rms_prev[l] = W.rms_cur[l];
        W.rms_cur[l] = c > 0.0 ? N.h * __builtin_sqrt(rr / c) : 0.0;
        if (t == 0) W.rms_first[l] = W.rms_cur[l];
    }
    if (t == 0) {
        st.cost_first = st.cost_cur = cost;
        st.rows = count;
        st.usable_links = usable;
        if (usable == 0) return end_call(P, NM_MOSAIC_ADJUST_END_NO_LINK, chain_in, W, O);
    } else if (!(cost <= st.cost_cur) || count != st.rows) {        // the cost rose (a NaN counts as risen): back one iterate
        for (int k = 0; k < P.n; ++k)
            for (int q = 0; q < 9; ++q) W.cur[k][q] = W.prev[k][q];
        for (int l = 0; l < P.L; ++l) W.rms_cur[l] = W.rms_prev[l];
        st.applied -= 1;
        return end_call(P, NM_MOSAIC_ADJUST_END_COST_ROSE, chain_in, W, O);
    } else {
        st.cost_cur = cost;
    }
    if (st.pending) return end_call(P, NM_MOSAIC_ADJUST_END_CONVERGED, chain_in, W, O);
    if (t == P.iterations) return end_call(P, NM_MOSAIC_ADJUST_END_ITERATIONS, chain_in, W, O);
    return true;
}

// After the solve of round t: W.delta holds the solution (8 per unknown frame, in slot order) unless `singular`
__host__ __device__ inline void finish_round(const Params &P, bool singular, const float *chain_in, Small &W, const Out &O)
{
    State &st = W.st;
    const Norm N = norm_of(P.fw, P.fh);
    for (int q = 0; q < 8 * st.unknowns; ++q) singular = singular || !__builtin_isfinite(W.delta[q]);
    if (singular) {
        end_call(P, NM_MOSAIC_ADJUST_END_SINGULAR, chain_in, W, O);
        return;
    }
    double size = 0.0;
    for (int k = 0; k < P.n; ++k) {
        if (W.slot[k] < 0) continue;
        double Gn[9];
        float row[9];
        for (int q = 0; q < 8; ++q) Gn[q] = W.cur[k][q] - W.delta[8 * W.slot[k] + q];
        Gn[8] = W.cur[k][8];
        double s = frame_step(W.cur[k], Gn, N, P.fw, P.fh);
        if (!row_of(Gn, N, row)) s = (double)__builtin_inff();
        if (!(s <= size)) size = s;                                  // a NaN is kept and fails below
    }
    st.last_step = size;
    if (!(size <= P.max_step)) {
        end_call(P, NM_MOSAIC_ADJUST_END_STEP, chain_in, W, O);
        return;
    }
    for (int k = 0; k < P.n; ++k) {
        for (int q = 0; q < 9; ++q) W.prev[k][q] = W.cur[k][q];
        if (W.slot[k] < 0) continue;
        for (int q = 0; q < 8; ++q) W.cur[k][q] = W.cur[k][q] - W.delta[8 * W.slot[k] + q];
    }
    st.applied += 1;
    if (size < CONVERGED_STEP) st.pending = 1;
}

}  // namespace nmma
