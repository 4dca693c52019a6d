// nm_ransac_refit.hip -- batched least-squares refit of RANSAC winners over their inliers, with inlier masks, for gfx950
// (no reference counterpart: the reference hands out the minimal-sample hypothesis, kernels/ransac.cu:523-694).
// ONE launch per call whatever n and rounds are, on the caller's stream, no allocation, no synchronisation, no workspace:
// one workgroup of nmf::LANES threads per pair runs all rounds. A pass is lane-strided over the pair's rows straight from
// the input arrays (L2-resident), fp64 partials in registers -> xor-butterfly per wave -> waves in ascending order through
// LDS: a fixed order that depends on the pair's inputs alone (no atomics). The 9 x 9 eigen-solve of the homography runs
// on the first wave with both matrices in LDS: the lanes of the nine indices compute the step's four rotations side by
// side (fp64 divide and sqrt are long sequences: four for the price of one), then 81 elements are updated in parallel.
// The arithmetic is nm_ransac_refit_math.hpp, shared with the host twin below: both agree bit for bit.
#include <cmath>

#include "nm_common.hpp"
#include "nm_ransac_refit_math.hpp"
#include "nm_pair_batch.hpp"
#include "../../include/nm_abi.h"

namespace {

using namespace nmf;

static_assert(NM_RANSAC_REFIT_MAX_ROUNDS == 4, "header and kernel disagree");

static_assert(sizeof(nmp::PointTables) + 96 < 4096, "refit kernel arguments exceed 4 KB");

struct RfShared {
    double part[WAVES][NACC];
    double tot[NACC];
    double A[81], V[81];
    double c[9], s[9];
    int rot[9];
    float H[9];
};

// Wave-synchronous LDS hand-off inside the first wave: all DS operations of the wave have completed and the compiler
// moves no LDS access across.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Totals of a pass in sh.tot[0 .. N): butterfly inside each wave, then the waves in ascending order.
template <int N>
__device__ __forceinline__ void reduce(double *acc, RfShared &sh, double *out)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int q = 0; q < N; ++q)                          // hand-written: with nmw::wave_sum the refit with mask and rms timed outside the parent's spread
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc[q] = acc[q] + __shfl_xor(acc[q], d);
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < N; ++q) sh.part[wave][q] = acc[q];
    __syncthreads();
    if (tid < N) {
        double t = sh.part[0][tid];
        for (int w = 1; w < WAVES; ++w) t = t + sh.part[w][tid];
        sh.tot[tid] = t;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < N; ++q) out[q] = sh.tot[q];
}

template <int KIND>
__device__ __forceinline__ void pass(const Pair &P, const float H[9], float thr, const double *prm, RfShared &sh, double *out)
{
    double acc[pass_width(KIND)];
    accumulate<KIND>(P, H, thr, (int)threadIdx.x, prm, acc);
    reduce<pass_width(KIND)>(acc, sh, out);
}

// The first wave: eigenvector of the smallest eigenvalue of the moment matrix in sh.A, then the fp32 map in sh.H.
__device__ void solve_homography(const double *prm, RfShared &sh)
{
    const int lane = threadIdx.x;          // < 64
    for (int e = lane; e < 81; e += 64) {
        sh.A[e] = dlt_entry(sh.tot, e / 9, e % 9);          // the totals of PASS_DLT are still in place
        sh.V[e] = (e / 9 == e % 9) ? 1.0 : 0.0;
    }
    wave_sync();
    for (int sweep = 0; sweep < JACOBI_MAX_SWEEPS; ++sweep) {
        bool any = false;
        for (int t = 0; t < 9; ++t) {
            if (lane < 9) {
                const int o = jacobi_partner(t, lane), p = lane < o ? lane : o, q = lane < o ? o : lane;
                double c = 1.0, s = 0.0;
                const bool r = (o != lane) && jacobi_rotation(sh.A[10 * p], sh.A[10 * q], sh.A[9 * p + q], c, s);
                sh.c[lane] = c; sh.s[lane] = s; sh.rot[lane] = r ? 1 : 0;
            }
            wave_sync();
            double na[2], nv[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {                      // columns: A <- A J, V <- V J
                const int e = lane + 64 * u;
                if (e < 81) {
                    const int r = e / 9, j = e % 9, o = jacobi_partner(t, j), p = j < o ? j : o, q = j < o ? o : j;
                    na[u] = sh.A[e]; nv[u] = sh.V[e];
                    if (sh.rot[j]) {
                        na[u] = jacobi_mix(j == p, sh.A[9 * r + p], sh.A[9 * r + q], sh.c[j], sh.s[j]);
                        nv[u] = jacobi_mix(j == p, sh.V[9 * r + p], sh.V[9 * r + q], sh.c[j], sh.s[j]);
                    }
                }
            }
            wave_sync();
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int e = lane + 64 * u;
                if (e < 81) { sh.A[e] = na[u]; sh.V[e] = nv[u]; }
            }
            wave_sync();
#pragma unroll
            for (int u = 0; u < 2; ++u) {                      // rows: A <- J^T A; the annihilated entries are set to 0
                const int e = lane + 64 * u;
                if (e < 81) {
                    const int i = e / 9, j = e % 9, o = jacobi_partner(t, i), p = i < o ? i : o, q = i < o ? o : i;
                    na[u] = sh.A[e];
                    if (sh.rot[i]) na[u] = (j == o) ? 0.0 : jacobi_mix(i == p, sh.A[9 * p + j], sh.A[9 * q + j], sh.c[i], sh.s[i]);
                }
            }
            wave_sync();
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int e = lane + 64 * u;
                if (e < 81) sh.A[e] = na[u];
            }
            any = any || (__ballot(lane < 9 && sh.rot[lane < 9 ? lane : 0]) != 0ull);
            wave_sync();
        }
        if (!any) break;
    }
    if (lane == 0) {
        const int best = smallest_diagonal(sh.A);
        double hn[9];
        for (int q = 0; q < 9; ++q) hn[q] = sh.V[9 * q + best];
        float H[9];
        denormalise(hn, prm, H);
        for (int q = 0; q < 9; ++q) sh.H[q] = H[q];
    }
}

template <int MODEL>
__global__ __launch_bounds__(LANES) void ransac_refit_kernel(const nmp::PointTables a, int capA, float thr, int rounds,
                                                             const float *H_in,
                                                             const int *__restrict__ status_in,
                                                             float *H_out, int *__restrict__ count_out,
                                                             int *__restrict__ status_out, int *__restrict__ rounds_done,
                                                             unsigned char *__restrict__ mask, float *__restrict__ rms)
{
    __shared__ RfShared sh;
    const int k = blockIdx.x, tid = threadIdx.x;
    unsigned char *mk = mask ? mask + (size_t)k * capA : nullptr;
    float H[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) H[q] = H_in[k * 9 + q];
    if ((status_in && status_in[k] != 1) || !finite9(H)) {          // uniform: the unusable pair
        if (tid < 9) H_out[k * 9 + tid] = 0.f;
        if (tid == 0) {
            count_out[k] = 0; status_out[k] = 0; rounds_done[k] = 0;
            if (rms) rms[k] = 0.f;
        }
        if (mk)
            for (int i = tid; i < capA; i += LANES) mk[i] = 0;
        return;
    }
    Pair P;
    P.sx = a.sx[k]; P.sy = a.sy[k]; P.dx = a.dx[k]; P.dy = a.dy[k]; P.mt = a.matches[k];
    P.nA = clip(*a.d_nA[k], capA);
    double sums[5];
    pass<PASS_SUMS>(P, H, thr, nullptr, sh, sums);
    int done = 0;
    for (int r = 0; r < rounds; ++r) {                               // every branch below is uniform over the workgroup
        if (sums[0] < (double)nmr_samples(MODEL)) break;
        float Hn[9];
        if (MODEL == 0) {
            fit_translation(sums, Hn);
        } else {
            double prm[6];
            centroids(sums, prm);
            if (MODEL == 1) {
                double m[3];
                pass<PASS_SIM>(P, H, thr, prm, sh, m);
                fit_similarity(prm, m, Hn);
            } else {
                double dist[2], m[24];
                pass<PASS_DIST>(P, H, thr, prm, sh, dist);
                hartley_scales(sums, dist, prm);
                pass<PASS_DLT>(P, H, thr, prm, sh, m);
                if (tid < 64) solve_homography(prm, sh);
                __syncthreads();
#pragma unroll
                for (int q = 0; q < 9; ++q) Hn[q] = sh.H[q];
            }
        }
        if (!finite9(Hn)) break;
        double sums_new[5];
        pass<PASS_SUMS>(P, Hn, thr, nullptr, sh, sums_new);
        if (sums_new[0] < sums[0]) break;
#pragma unroll
        for (int q = 0; q < 9; ++q) H[q] = Hn[q];
#pragma unroll
        for (int q = 0; q < 5; ++q) sums[q] = sums_new[q];
        ++done;
    }
    if (tid < 9) H_out[k * 9 + tid] = H[tid];
    if (tid == 0) { count_out[k] = (int)sums[0]; status_out[k] = 1; rounds_done[k] = done; }
    if (mk)
        for (int i = tid; i < capA; i += LANES) {
            float x, y, u, v;
            mk[i] = (i < P.nA && inlier_row(P, i, H, thr, x, y, u, v)) ? 1 : 0;
        }
    if (rms) {
        double tot[1];
        pass<PASS_RMS>(P, H, thr, nullptr, sh, tot);
        if (tid == 0) rms[k] = rms_of(tot[0], sums[0]);
    }
}

// ---- the host twin: the same functions, the lanes and the reduction tree walked serially ----
template <int KIND>
void host_pass(const Pair &P, const float H[9], float thr, const double *prm, double *out)
{
    constexpr int N = pass_width(KIND);
    static thread_local double part[LANES][NACC];
    for (int l = 0; l < LANES; ++l) accumulate<KIND>(P, H, thr, l, prm, part[l]);
    for (int q = 0; q < N; ++q) {
        double total = 0.0;
        for (int w = 0; w < WAVES; ++w) {
            double v[64];
            for (int l = 0; l < 64; ++l) v[l] = part[64 * w + l][q];
            for (int d = 32; d >= 1; d >>= 1)
                for (int l = 0; l < d; ++l) v[l] = v[l] + v[l + d];
            total = w == 0 ? v[0] : total + v[0];
        }
        out[q] = total;
    }
}

void host_solve_homography(const double *m, const double *prm, float H[9])
{
    double A[81], V[81], nA[81], nV[81], c[9], s[9];
    bool rot[9];
    for (int e = 0; e < 81; ++e) {
        A[e] = dlt_entry(m, e / 9, e % 9);
        V[e] = (e / 9 == e % 9) ? 1.0 : 0.0;
    }
    for (int sweep = 0; sweep < JACOBI_MAX_SWEEPS; ++sweep) {
        bool any = false;
        for (int t = 0; t < 9; ++t) {
            for (int i = 0; i < 9; ++i) {
                const int o = jacobi_partner(t, i), p = i < o ? i : o, q = i < o ? o : i;
                c[i] = 1.0; s[i] = 0.0;
                rot[i] = (o != i) && jacobi_rotation(A[10 * p], A[10 * q], A[9 * p + q], c[i], s[i]);
                any = any || rot[i];
            }
            for (int e = 0; e < 81; ++e) {
                const int r = e / 9, j = e % 9, o = jacobi_partner(t, j), p = j < o ? j : o, q = j < o ? o : j;
                nA[e] = A[e]; nV[e] = V[e];
                if (rot[j]) {
                    nA[e] = jacobi_mix(j == p, A[9 * r + p], A[9 * r + q], c[j], s[j]);
                    nV[e] = jacobi_mix(j == p, V[9 * r + p], V[9 * r + q], c[j], s[j]);
                }
            }
            for (int e = 0; e < 81; ++e) { A[e] = nA[e]; V[e] = nV[e]; }
            for (int e = 0; e < 81; ++e) {
                const int i = e / 9, j = e % 9, o = jacobi_partner(t, i), p = i < o ? i : o, q = i < o ? o : i;
                nA[e] = A[e];
                if (rot[i]) nA[e] = (j == o) ? 0.0 : jacobi_mix(i == p, A[9 * p + j], A[9 * q + j], c[i], s[i]);
            }
            for (int e = 0; e < 81; ++e) A[e] = nA[e];
        }
        if (!any) break;
    }
    const int best = smallest_diagonal(A);
    double hn[9];
    for (int q = 0; q < 9; ++q) hn[q] = V[9 * q + best];
    denormalise(hn, prm, H);
}

void host_refit_pair(int model, const Pair &P, int capA, float thr, int rounds, const float *H_in, int status_in, float *H_out,
                     int *count_out, int *status_out, int *rounds_done, unsigned char *mk, float *rms)
{
    float H[9];
    for (int q = 0; q < 9; ++q) H[q] = H_in[q];
    if (status_in != 1 || !finite9(H)) {
        for (int q = 0; q < 9; ++q) H_out[q] = 0.f;
        *count_out = 0; *status_out = 0; *rounds_done = 0;
        if (rms) *rms = 0.f;
        if (mk)
            for (int i = 0; i < capA; ++i) mk[i] = 0;
        return;
    }
    double sums[5];
    host_pass<PASS_SUMS>(P, H, thr, nullptr, sums);
    int done = 0;
    for (int r = 0; r < rounds; ++r) {
        if (sums[0] < (double)nmr_samples(model)) break;
        float Hn[9];
        if (model == 0) {
            fit_translation(sums, Hn);
        } else {
            double prm[6];
            centroids(sums, prm);
            if (model == 1) {
                double m[3];
                host_pass<PASS_SIM>(P, H, thr, prm, m);
                fit_similarity(prm, m, Hn);
            } else {
                double dist[2], m[24];
                host_pass<PASS_DIST>(P, H, thr, prm, dist);
                hartley_scales(sums, dist, prm);
                host_pass<PASS_DLT>(P, H, thr, prm, m);
                host_solve_homography(m, prm, Hn);
            }
        }
        if (!finite9(Hn)) break;
        double sums_new[5];
        host_pass<PASS_SUMS>(P, Hn, thr, nullptr, sums_new);
        if (sums_new[0] < sums[0]) break;
        for (int q = 0; q < 9; ++q) H[q] = Hn[q];
        for (int q = 0; q < 5; ++q) sums[q] = sums_new[q];
        ++done;
    }
    for (int q = 0; q < 9; ++q) H_out[q] = H[q];
    *count_out = (int)sums[0]; *status_out = 1; *rounds_done = done;
    if (mk)
        for (int i = 0; i < capA; ++i) {
            float x, y, u, v;
            mk[i] = (i < P.nA && inlier_row(P, i, H, thr, x, y, u, v)) ? 1 : 0;
        }
    if (rms) {
        double tot[1];
        host_pass<PASS_RMS>(P, H, thr, nullptr, tot);
        *rms = rms_of(tot[0], sums[0]);
    }
}

bool rf_args_ok(int model, int n, const float *const *src_x, const float *const *src_y, const int *const *d_nA, int capA,
                const float *const *dst_x, const float *const *dst_y, const int *const *matches, const float *H_in,
                float thr, int rounds, const float *H_out, const int *count, const int *status, const int *rounds_done)
{
    if (model < 0 || model > 2 || rounds < 0 || rounds > NM_RANSAC_REFIT_MAX_ROUNDS || !std::isfinite(thr)) return false;
    return nmp::range_ok(n, capA) && nmp::tables_ok(n, {src_x, src_y, d_nA, dst_x, dst_y, matches}, {},
                                                    {H_in, H_out, count, status, rounds_done});
}

}  // namespace

extern "C" int nm_ransac_refit_batch_dev_f32(int model, int n, const float *const *src_x, const float *const *src_y,
                                             const int *const *d_nA, int capA, const float *const *dst_x,
                                             const float *const *dst_y, const int *const *matches, const float *H_in,
                                             const int *status_in, float inlier_threshold, int rounds, float *H_out,
                                             int *count, int *status, int *rounds_done, unsigned char *mask, float *rms,
                                             void *stream)
{
    if (!rf_args_ok(model, n, src_x, src_y, d_nA, capA, dst_x, dst_y, matches, H_in, inlier_threshold, rounds, H_out, count,
                    status, rounds_done))
        return (int)hipErrorInvalidValue;
    nmp::PointTables a;
    a.fill(n, src_x, src_y, dst_x, dst_y, matches, d_nA);
    const auto kernel = model == 0 ? ransac_refit_kernel<0> : model == 1 ? ransac_refit_kernel<1> : ransac_refit_kernel<2>;
    hipLaunchKernelGGL(kernel, dim3(n), dim3(LANES), 0, nm_stream(stream), a, capA, inlier_threshold, rounds, H_in,
                       status_in, H_out, count, status, rounds_done, mask, rms);
    NM_LAUNCH_CHECK();
    return 0;
}

extern "C" int nm_ransac_refit_host_f32(int model, int n, const float *const *src_x, const float *const *src_y,
                                        const int *const *nA, int capA, const float *const *dst_x,
                                        const float *const *dst_y, const int *const *matches, const float *H_in,
                                        const int *status_in, float inlier_threshold, int rounds, float *H_out, int *count,
                                        int *status, int *rounds_done, unsigned char *mask, float *rms)
{
    if (!rf_args_ok(model, n, src_x, src_y, nA, capA, dst_x, dst_y, matches, H_in, inlier_threshold, rounds, H_out, count,
                    status, rounds_done))
        return (int)hipErrorInvalidValue;
    for (int k = 0; k < n; ++k) {
        Pair P;
        P.sx = src_x[k]; P.sy = src_y[k]; P.dx = dst_x[k]; P.dy = dst_y[k]; P.mt = matches[k];
        P.nA = clip(*nA[k], capA);
        host_refit_pair(model, P, capA, inlier_threshold, rounds, H_in + 9 * k, status_in ? status_in[k] : 1, H_out + 9 * k,
                        count + k, status + k, rounds_done + k, mask ? mask + (size_t)k * capA : nullptr, rms ? rms + k : nullptr);
    }
    return 0;
}
