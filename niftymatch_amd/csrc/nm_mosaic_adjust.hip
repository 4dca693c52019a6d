// nm_mosaic_adjust.hip -- global adjustment of a mosaic's frame maps over all verified links, loop closures included, for
// gfx950: Gauss-Newton with Levenberg damping on the maps frame pixels -> mosaic coordinates, one anchor frame fixed
// (include/nm_abi.h has the written semantics). No reference counterpart. (iterations + 1) x (ceil(L / 64) + 1) launches
// on the caller's stream, no allocation, no synchronisation, no host read; a round boundary is a launch boundary, no
// kernel waits for another workgroup:
//   accumulate  grid (4 slices, up to 64 links), 512 threads = the refit's virtual lanes. A workgroup walks its link's
//               rows lane-strided with one slice (39) of the link's 153 fp64 sums in registers (all of them do not fit a
//               lane; a row is 20 bytes and cheap to read four times), then nmw::wave_reduce per sum and the eight waves
//               through LDS in ascending order: one row of sums per link in the workspace, plain vector stores, no
//               atomics. Round 0 takes the maps from chain_in, the later rounds from the iterate in the workspace; the
//               workgroups of a call that has ended leave at once.
//   solve       one workgroup of 512. One lane runs begin_round (totals, cost rule, end reasons, outputs); the workgroup
//               adds the usable links into the normal matrix in ascending link order, thread i runs row i of the
//               left-looking Cholesky (thread N the right-hand side as one more row, which is the forward substitution);
//               the matrix is kept symmetric in the workspace, so both the own row and the pivot row are read coalesced;
//               one lane runs the backward chains out of LDS and finish_round (step size, update).
// The arithmetic is nm_mosaic_adjust_math.hpp, shared with the host twin below, which walks the same virtual lanes and the
// same per-element chains serially: both agree bit for bit.
#include <algorithm>
#include <cmath>
#include <vector>

#include "nm_chol_math.hpp"
#include "nm_common.hpp"
#include "nm_mosaic_adjust_math.hpp"
#include "nm_pair_batch.hpp"
#include "nm_wave_dev.hpp"
#include "../../include/nm_abi.h"

namespace {

using namespace nmma;

struct AccArgs {                            // 6 x 64 pointers and the links' frames: 3.2 KB of kernel arguments
    nmp::PointTables p;
    unsigned char a[GROUP], b[GROUP];
};
static_assert(sizeof(AccArgs) + 128 < 4096, "accumulate kernel arguments exceed 4 KB");
static_assert(sizeof(LinkIdx) + sizeof(Params) + sizeof(Out) + 128 < 4096, "solve kernel arguments exceed 4 KB");

__host__ __device__ __forceinline__ int leading(int n) { return 8 * n; }     // >= 8 (n - 1) + 1 columns

template <int SLICE>
__device__ __forceinline__ void accumulate_slice(const Link &K, const Norm &N, const double *Ga, const double *Gb,
                                                 double (*part)[SLICE_W], double *__restrict__ row)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double s[SLICE_W];
    int count = walk_lane<SLICE>(K, N, Ga, Gb, tid, s);
#pragma unroll
    for (int q = 0; q < SLICE_W; ++q) {
        const double v = nmw::wave_reduce(s[q], nmw::Sum());
        if (lane == 0) part[wave][q] = v;
    }
    __syncthreads();
    if (tid < SLICE_W && SLICE * SLICE_W + tid < SUMS) {
        double t = part[0][tid];
        for (int w = 1; w < WAVES; ++w) t = t + part[w][tid];
        row[SLICE * SLICE_W + tid] = t;
    }
    if (SLICE == 0) {                                            // integers: any order
        __shared__ int cnt[WAVES];
        count = nmw::wave_reduce(count, nmw::Sum());
        if (lane == 0) cnt[wave] = count;
        __syncthreads();
        if (tid == 0) {
            int c = 0;
            for (int w = 0; w < WAVES; ++w) c += cnt[w];
            row[S_COUNT] = (double)c;
        }
    }
}

__global__ __launch_bounds__(LANES) void mosaic_adjust_accumulate_kernel(const AccArgs A, int first, int links, int capA,
                                                                         const unsigned char *__restrict__ mask,
                                                                         const int *__restrict__ link_status,
                                                                         const float *__restrict__ chain_in, int fw, int fh,
                                                                         int t, const Small *__restrict__ W,
                                                                         double *__restrict__ rows)
{
    __shared__ double part[WAVES][SLICE_W];
    const int s = blockIdx.y, l = first + s;                     // slot in the launch, link of the call
    if (s >= links) return;
    const Norm N = norm_of(fw, fh);
    double Ga[9], Gb[9];
    const int fa = A.a[s], fb = A.b[s];
    if (t == 0) {                                                // uniform over the workgroup, as every branch here
        if (link_status && link_status[l] != 1) return;
        if (!init_frame(chain_in + 9 * fa, N, Ga) || !init_frame(chain_in + 9 * fb, N, Gb)) return;
    } else {
        if (W->st.ended || !W->usable[l]) return;
#pragma unroll
        for (int q = 0; q < 9; ++q) { Ga[q] = W->cur[fa][q]; Gb[q] = W->cur[fb][q]; }
    }
    Link K;
    K.sx = A.p.sx[s]; K.sy = A.p.sy[s]; K.dx = A.p.dx[s]; K.dy = A.p.dy[s]; K.mt = A.p.matches[s];
    K.mask = mask ? mask + (size_t)l * capA : nullptr;
    K.nA = nmp::clip(*A.p.d_nA[s], capA);
    double *row = rows + (size_t)l * ROW;
    switch (blockIdx.x) {
    case 0: accumulate_slice<0>(K, N, Ga, Gb, part, row); break;
    case 1: accumulate_slice<1>(K, N, Ga, Gb, part, row); break;
    case 2: accumulate_slice<2>(K, N, Ga, Gb, part, row); break;
    default: accumulate_slice<3>(K, N, Ga, Gb, part, row); break;
    }
}

__global__ __launch_bounds__(LANES) void mosaic_adjust_solve_kernel(const Params P, int t, const LinkIdx Xarg,
                                                                    const int *__restrict__ link_status,
                                                                    const float *__restrict__ chain_in,
                                                                    const double *__restrict__ rows, double *M, Small *W,
                                                                    const Out O)
{
    __shared__ nmc::CholShared<LANES> s_chol;
    __shared__ int s_go;
    __shared__ LinkIdx s_X;                                      // indexed at run time: out of the kernel arguments
    const int tid = threadIdx.x;
    if (tid < MAX_LINKS) { s_X.a[tid] = Xarg.a[tid]; s_X.b[tid] = Xarg.b[tid]; }
    __syncthreads();
    const LinkIdx &X = s_X;
    if (tid == 0) {
        s_go = begin_round(P, t, X, link_status, chain_in, rows, *W, O) ? 1 : 0;
    }
    __syncthreads();
    if (!s_go) return;
    const int N = 8 * W->st.unknowns, ld = leading(P.n);         // 8 <= N <= 8 (n - 1) < ld
    for (int e = tid; e < N * ld; e += LANES) M[e] = 0.0;
    __syncthreads();
    // A and g (column N): the usable links in ascending order; within a link every entry has its own thread
    for (int l = 0; l < P.L; ++l) {
        if (!W->usable[l]) continue;
        const double *S = rows + (size_t)l * ROW;
        if (tid < COLS * COLS) {
            const int r = tid >> 4, c = tid & 15;
            const int sr = W->slot[r < 8 ? X.a[l] : X.b[l]], sc = W->slot[c < 8 ? X.a[l] : X.b[l]];
            if (sr >= 0 && sc >= 0) {
                double *m = M + (size_t)(8 * sr + (r & 7)) * ld + 8 * sc + (c & 7);
                *m = *m + S[r <= c ? tri(r, c) : tri(c, r)];
            }
        } else if (tid < COLS * COLS + COLS) {
            const int r = tid - COLS * COLS, sr = W->slot[r < 8 ? X.a[l] : X.b[l]];
            if (sr >= 0) {
                double *m = M + (size_t)(8 * sr + (r & 7)) * ld + N;
                *m = *m + S[S_JTR + r];
            }
        }
        __syncthreads();
    }
    if (tid < N) {
        double d = M[(size_t)tid * ld + tid] * (1.0 + P.damping);
        if (d == 0.0) d = 1.0;
        M[(size_t)tid * ld + tid] = d;
    }
    __syncthreads();
    // Cholesky by columns; thread i owns row i, thread N the right-hand side (nm_chol_math.hpp)
    const bool solved = nmc::chol_solve_block(M, ld, N, s_chol);
    if (solved) {
        if (tid < N) W->delta[tid] = s_chol.x[tid];
        __syncthreads();
    }
    if (tid == 0) finish_round(P, !solved, chain_in, *W, O);
}

// ---- the host twin: the same functions, the virtual lanes, the trees and the chains walked serially ----
template <int SLICE>
int host_slice(const Link &K, const Norm &N, const double *Ga, const double *Gb, double *row)
{
    static thread_local double v[64][SLICE_W];
    double tot[SLICE_W];
    int count = 0;
    for (int w = 0; w < WAVES; ++w) {
        for (int l = 0; l < 64; ++l) count += walk_lane<SLICE>(K, N, Ga, Gb, 64 * w + l, v[l]);
        for (int d = 32; d >= 1; d >>= 1)
            for (int l = 0; l < d; ++l)
                for (int q = 0; q < SLICE_W; ++q) v[l][q] = v[l][q] + v[l + d][q];
        for (int q = 0; q < SLICE_W; ++q) tot[q] = w == 0 ? v[0][q] : tot[q] + v[0][q];
    }
    for (int q = 0; q < SLICE_W && SLICE * SLICE_W + q < SUMS; ++q) row[SLICE * SLICE_W + q] = tot[q];
    return count;
}

void host_link_sums(const Link &K, const Norm &N, const double *Ga, const double *Gb, double *row)
{
    row[S_COUNT] = (double)host_slice<0>(K, N, Ga, Gb, row);
    host_slice<1>(K, N, Ga, Gb, row);
    host_slice<2>(K, N, Ga, Gb, row);
    host_slice<3>(K, N, Ga, Gb, row);
}

bool host_solve(const Params &P, const LinkIdx &X, const double *rows, std::vector<double> &M, Small &W)
{
    const int N = 8 * W.st.unknowns, ld = leading(P.n);
    std::fill(M.begin(), M.end(), 0.0);
    for (int l = 0; l < P.L; ++l) {
        if (!W.usable[l]) continue;
        const double *S = rows + (size_t)l * ROW;
        for (int r = 0; r < COLS; ++r) {
            const int sr = W.slot[r < 8 ? X.a[l] : X.b[l]];
            if (sr < 0) continue;
            for (int c = 0; c < COLS; ++c) {
                const int sc = W.slot[c < 8 ? X.a[l] : X.b[l]];
                if (sc < 0) continue;
                double &m = M[(size_t)(8 * sr + (r & 7)) * ld + 8 * sc + (c & 7)];
                m = m + S[r <= c ? tri(r, c) : tri(c, r)];
            }
            double &g = M[(size_t)(8 * sr + (r & 7)) * ld + N];
            g = g + S[S_JTR + r];
        }
    }
    for (int i = 0; i < N; ++i) {
        double d = M[(size_t)i * ld + i] * (1.0 + P.damping);
        M[(size_t)i * ld + i] = d == 0.0 ? 1.0 : d;
    }
    return nmc::chol_solve_serial(M.data(), ld, N, W.delta);
}

bool sizes_ok(int capA, int fw, int fh)
{
    return nmp::cap_ok(capA) && nm_size_ok(fw) && nm_size_ok(fh);
}

bool ma_args_ok(int n, int L, const int *link_a, const int *link_b, const float *const *src_x, const float *const *src_y,
                const int *const *d_nA, int capA, const float *const *dst_x, const float *const *dst_y,
                const int *const *matches, const float *chain_in, int anchor, int fw, int fh, int iterations, int min_rows,
                double damping, double max_step, const float *chain_out, const int *frame_status, const double *link_rms,
                const double *stats)
{
    if (n < 2 || n > MAX_FRAMES || L < 1 || L > MAX_LINKS || !sizes_ok(capA, fw, fh) || anchor < 0 || anchor >= n ||
        iterations < 1 || iterations > NM_MOSAIC_ADJUST_MAX_ITERATIONS || min_rows < 4 || !std::isfinite(damping) ||
        !(damping >= 0.0) || !std::isfinite(max_step) || !(max_step > 0.0) || !link_a || !link_b)
        return false;
    for (int l = 0; l < L; ++l)
        if (link_a[l] < 0 || link_a[l] >= n || link_b[l] < 0 || link_b[l] >= n || link_a[l] == link_b[l]) return false;
    return nmp::tables_ok(L, {src_x, src_y, d_nA, dst_x, dst_y, matches}, {},
                          {chain_in, chain_out, frame_status, link_rms, stats});
}

LinkIdx link_index(int L, const int *link_a, const int *link_b)
{
    LinkIdx X;
    for (int l = 0; l < MAX_LINKS; ++l) {
        X.a[l] = (unsigned char)(l < L ? link_a[l] : 0);
        X.b[l] = (unsigned char)(l < L ? link_b[l] : 0);
    }
    return X;
}

size_t matrix_doubles(int n) { return (size_t)8 * (n - 1) * leading(n); }

}  // namespace

extern "C" size_t nm_mosaic_adjust_workspace_bytes(int n, int L)
{
    if (n < 2 || n > MAX_FRAMES || L < 1 || L > MAX_LINKS) return 0;
    return ((size_t)L * ROW + matrix_doubles(n)) * sizeof(double) + sizeof(Small);
}

extern "C" int nm_mosaic_adjust_dev_f32(int n, int L, const int *link_a, const int *link_b, const float *const *src_x,
                                        const float *const *src_y, const int *const *d_nA, int capA,
                                        const float *const *dst_x, const float *const *dst_y, const int *const *matches,
                                        const unsigned char *mask, const int *link_status, const float *chain_in, int anchor,
                                        int fw, int fh, int iterations, int min_rows, double damping, double max_step,
                                        float *chain_out, int *frame_status, double *link_rms, double *stats,
                                        void *workspace, void *stream)
{
    if (!ma_args_ok(n, L, link_a, link_b, src_x, src_y, d_nA, capA, dst_x, dst_y, matches, chain_in, anchor, fw, fh,
                    iterations, min_rows, damping, max_step, chain_out, frame_status, link_rms, stats) ||
        !workspace)
        return (int)hipErrorInvalidValue;
    double *rows = static_cast<double *>(workspace);
    double *M = rows + (size_t)L * ROW;
    Small *W = reinterpret_cast<Small *>(M + matrix_doubles(n));
    const Params P{n, L, anchor, fw, fh, iterations, min_rows, damping, max_step};
    const LinkIdx X = link_index(L, link_a, link_b);
    const Out O{chain_out, frame_status, link_rms, stats};
    for (int t = 0; t <= iterations; ++t) {
        for (int first = 0; first < L; first += GROUP) {
            const int links = L - first < GROUP ? L - first : GROUP;
            AccArgs A;
            nmp::fill_slots(A.p.sx, src_x, first, L); nmp::fill_slots(A.p.sy, src_y, first, L);
            nmp::fill_slots(A.p.dx, dst_x, first, L); nmp::fill_slots(A.p.dy, dst_y, first, L);
            nmp::fill_slots(A.p.matches, matches, first, L); nmp::fill_slots(A.p.d_nA, d_nA, first, L);
            for (int s = 0; s < GROUP; ++s) {
                A.a[s] = first + s < L ? X.a[first + s] : 0;
                A.b[s] = first + s < L ? X.b[first + s] : 0;
            }
            hipLaunchKernelGGL(mosaic_adjust_accumulate_kernel, dim3(SLICES, links), dim3(LANES), 0, nm_stream(stream), A,
                               first, links, capA, mask, link_status, chain_in, fw, fh, t, W, rows);
            NM_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(mosaic_adjust_solve_kernel, dim3(1), dim3(LANES), 0, nm_stream(stream), P, t, X, link_status,
                           chain_in, rows, M, W, O);
        NM_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int nm_mosaic_adjust_host_f32(int n, int L, const int *link_a, const int *link_b, const float *const *src_x,
                                         const float *const *src_y, const int *const *nA, int capA,
                                         const float *const *dst_x, const float *const *dst_y, const int *const *matches,
                                         const unsigned char *mask, const int *link_status, const float *chain_in,
                                         int anchor, int fw, int fh, int iterations, int min_rows, double damping,
                                         double max_step, float *chain_out, int *frame_status, double *link_rms,
                                         double *stats)
{
    if (!ma_args_ok(n, L, link_a, link_b, src_x, src_y, nA, capA, dst_x, dst_y, matches, chain_in, anchor, fw, fh, iterations,
                    min_rows, damping, max_step, chain_out, frame_status, link_rms, stats))
        return (int)hipErrorInvalidValue;
    std::vector<double> rows((size_t)L * ROW, 0.0), M(matrix_doubles(n), 0.0);
    std::vector<Small> small(1);
    Small &W = small[0];
    const Params P{n, L, anchor, fw, fh, iterations, min_rows, damping, max_step};
    const LinkIdx X = link_index(L, link_a, link_b);
    const Out O{chain_out, frame_status, link_rms, stats};
    const Norm N = norm_of(fw, fh);
    for (int t = 0; t <= iterations; ++t) {
        if (t > 0 && W.st.ended) break;
        for (int l = 0; l < L; ++l) {
            double Ga[9], Gb[9];
            if (t == 0) {
                if (link_status && link_status[l] != 1) continue;
                if (!init_frame(chain_in + 9 * X.a[l], N, Ga) || !init_frame(chain_in + 9 * X.b[l], N, Gb)) continue;
            } else {
                if (!W.usable[l]) continue;
                for (int q = 0; q < 9; ++q) { Ga[q] = W.cur[X.a[l]][q]; Gb[q] = W.cur[X.b[l]][q]; }
            }
            const Link K{src_x[l], src_y[l], dst_x[l], dst_y[l], matches[l], mask ? mask + (size_t)l * capA : nullptr,
                         nmp::clip(*nA[l], capA)};
            host_link_sums(K, N, Ga, Gb, rows.data() + (size_t)l * ROW);
        }
        if (!begin_round(P, t, X, link_status, chain_in, rows.data(), W, O)) break;
        finish_round(P, !host_solve(P, X, rows.data(), M, W), chain_in, W, O);
    }
    return 0;
}

extern "C" int nm_mosaic_adjust_sums_host_f32(const float *src_x, const float *src_y, int nA, int capA, const float *dst_x,
                                              const float *dst_y, const int *matches, const unsigned char *mask, int fw,
                                              int fh, const double *Ga, const double *Gb, double *sums, int *count)
{
    if (!sizes_ok(capA, fw, fh) || !src_x || !src_y || !dst_x || !dst_y || !matches || !Ga || !Gb || !sums || !count)
        return (int)hipErrorInvalidValue;
    double row[ROW];
    const Link K{src_x, src_y, dst_x, dst_y, matches, mask, nmp::clip(nA, capA)};
    host_link_sums(K, norm_of(fw, fh), Ga, Gb, row);
    for (int q = 0; q < SUMS; ++q) sums[q] = row[q];
    *count = (int)row[S_COUNT];
    return 0;
}
