// nm_mosaic_exposure.hip -- exposure compensation of a mosaic for gfx950: per-link, per-channel overlap sums from the BGRA
// frames, and the per-frame gains that level them (include/nm_abi.h has the written semantics). No reference counterpart.
// The gained blend that applies the gains is nm_transform_blend_batch_gain (nm_mosaic.hip). On the caller's stream, no
// allocation, no synchronisation, no host read, no workspace; no kernel waits for another workgroup:
//   measure  TWO launches whatever L is, the first one workgroup that zeroes the L x 7 sums (nmp::launch_zero_u64, a
//            kernel and not a memset node: see there). The 64 frame pointers (512 B) and the links' frame indices
//            (2 x 256 B) travel as kernel arguments. Grid (parts, L): the lattice walk over frame a
//            (one of three copies: nm_lattice.hpp), a link's tiles dealt to its `parts` workgroups of four waves (parts x
//            L ~ 4096 workgroups when the lattice has that many tiles, so one link alone spreads over up to 256). A wave
//            takes a lattice row, its lanes 64 neighbouring lattice columns: one uchar4 of frame a (at stride 1
//            a coalesced 256-byte read), one projection, four gathered uchar4 taps of frame b. The seven sums are integers:
//            u64 per lane -> nmw::block_totals -> one vector atomic add per workgroup and sum. Integer adds commute, so
//            the totals do not depend on arrival order.
//   solve    one launch of one workgroup of 128. One lane marks the usable links; lane i assembles row i of the n x n
//            system in ascending link order into LDS; the workgroup runs the written-order Cholesky of the adjustment
//            (nm_chol_math.hpp), per channel; six lanes evaluate the six costs, each one chain; lane k writes frame k's
//            gains.
// The arithmetic is nm_mosaic_exposure_math.hpp, shared with the host twins below: both agree bit for bit.
#include <cmath>
#include <vector>

#include "nm_common.hpp"
#include "nm_lattice.hpp"
#include "nm_mosaic_exposure_math.hpp"
#include "nm_pair_batch.hpp"
#include "../../include/nm_abi.h"

namespace {

using namespace nmx;
using namespace nmlat;

static_assert(NM_EXPOSURE_MAX_LINKS == NM_MOSAIC_ADJUST_MAX_LINKS, "exposure links follow the adjustment's convention");

constexpr int MAX_PARTS = 256;              // workgroups per link at most
constexpr int GRID_TARGET = 4096;           // workgroups per launch aimed at: 16 per CU
constexpr int SOLVE_THREADS = 128;          // > MAX_FRAMES: thread n owns the right-hand side

struct SumsArgs {                           // 64 pointers and the links' frames: 1 KB of kernel arguments
    const uchar4 *frames[MAX_FRAMES];
    LinkIdx X;
};
static_assert(sizeof(SumsArgs) + 128 < 4096, "measure kernel arguments exceed 4 KB");

__global__ __launch_bounds__(THREADS) void mosaic_exposure_sums_kernel(const SumsArgs A, int fw, int fh,
                                                                       const float *__restrict__ mask,
                                                                       const float *__restrict__ H,
                                                                       const int *__restrict__ link_status, int stride,
                                                                       int lo, int hi, int lw, int lh, int tiles_x, int tiles,
                                                                       u64 *__restrict__ sums)
{
    __shared__ u64 part[WAVES][SUMS];
    const int l = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float Hl[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) Hl[q] = H[l * 9 + q];
    if (!nml::usable(link_status ? link_status[l] : 1, Hl)) return;      // uniform: the zeroing's zeros stay
    const Frames F{A.frames[A.X.a[l]], A.frames[A.X.b[l]], mask, fw, fh};
    u64 s[SUMS] = {0, 0, 0, 0, 0, 0, 0};
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {        // the lattice walk: one of three copies (nm_lattice.hpp)
        const int u = (t % tiles_x) * TILE_W + lane, v0 = (t / tiles_x) * TILE_H;
        if (u < lw)
            for (int r = wave; r < TILE_H && v0 + r < lh; r += WAVES)
                add_pixel(F, Hl, lo, hi, stride * u + stride / 2, stride * (v0 + r) + stride / 2, s);
    }
    const u64 total = nmw::block_totals<WAVES>(s, part);
    if (tid < SUMS && total) atomicAdd(sums + (size_t)l * SUMS + tid, total);
}

__global__ __launch_bounds__(SOLVE_THREADS) void mosaic_gains_kernel(const Params P, const LinkIdx Xarg,
                                                                     const u64 *__restrict__ sums,
                                                                     const int *__restrict__ link_status,
                                                                     float *__restrict__ gains, double *__restrict__ stats)
{
    __shared__ double s_M[MAX_FRAMES * LD];
    __shared__ nmc::CholShared<SOLVE_THREADS> s_chol;
    __shared__ double s_g[3][MAX_FRAMES], s_cost[6];
    __shared__ LinkIdx s_X;                                      // indexed at run time: out of the kernel arguments
    __shared__ unsigned char s_usable[MAX_LINKS];
    __shared__ int s_links, s_frames;
    const int tid = threadIdx.x;
    for (int l = tid; l < MAX_LINKS; l += SOLVE_THREADS) { s_X.a[l] = Xarg.a[l]; s_X.b[l] = Xarg.b[l]; }
    __syncthreads();
    const LinkIdx &X = s_X;
    if (tid == 0) mark_links(P, X, sums, link_status, s_usable, s_links, s_frames);
    __syncthreads();
    const int systems = P.mode == NM_EXPOSURE_COMMON ? 1 : 3;
    bool solved = s_links > 0;
    for (int c = 0; c < systems && solved; ++c) {                // uniform
        if (tid < P.n) assemble_row(P, X, sums, s_usable, c, tid, s_M + tid * LD);
        __syncthreads();
        solved = nmc::chol_solve_block(s_M, LD, P.n, s_chol);
        if (solved && tid < P.n) s_g[c][tid] = s_chol.x[tid];
        __syncthreads();
    }
    if (tid < 6) {
        const int c = tid % 3, sys = systems == 1 ? 0 : c;
        s_cost[tid] = cost_of(P, X, sums, s_usable, sys, (tid < 3 || !solved) ? nullptr : s_g[sys]);
    }
    __syncthreads();
    if (solved)
        for (int q = 0; q < systems * P.n; ++q) solved = solved && __builtin_isfinite(s_g[q / P.n][q % P.n]);   // uniform
    if (!solved) {
        if (tid == 0)
            write_unit(P, gains, stats, s_cost, s_links, s_frames, s_links > 0 ? NM_EXPOSURE_END_SINGULAR : NM_EXPOSURE_END_NO_LINK);
        return;
    }
    if (tid < P.n)
        for (int c = 0; c < 3; ++c) gains[3 * tid + c] = clamp_gain(s_g[systems == 1 ? 0 : c][tid], P.g_min, P.g_max);
    if (tid < 6) stats[tid] = s_cost[tid];
    if (tid == 0) { stats[6] = (double)s_links; stats[7] = (double)s_frames; stats[8] = (double)NM_EXPOSURE_END_OK; }
}

// ---- the host twins: the same functions, the lattice walked row by row, the rows and chains walked serially ----
bool links_ok(int n, int L, const int *link_a, const int *link_b)
{
    if (n < 1 || n > MAX_FRAMES || L < 1 || L > MAX_LINKS || !link_a || !link_b) return false;
    for (int l = 0; l < L; ++l)
        if (link_a[l] < 0 || link_a[l] >= n || link_b[l] < 0 || link_b[l] >= n || link_a[l] == link_b[l]) return false;
    return true;
}

bool sums_args_ok(int n, int L, const unsigned char *const *frames, const int *link_a, const int *link_b, int fw, int fh,
                  const float *H, int stride, int lo, int hi, const void *sums)
{
    if (!links_ok(n, L, link_a, link_b) || !lattice_ok(fw, fh, stride) || lo < 0 || lo > hi || hi > 255) return false;
    return nmp::tables_ok(n, {frames}, {}, {H, sums});
}

bool gains_args_ok(int n, int L, const int *link_a, const int *link_b, const void *sums, int min_pixels, double sigma_n,
                   double sigma_g, float g_min, float g_max, int mode, const void *gains, const void *stats)
{
    const auto sigma_ok = [](double s) { return s >= NM_EXPOSURE_SIGMA_MIN && s <= NM_EXPOSURE_SIGMA_MAX; };   // a NaN fails
    return links_ok(n, L, link_a, link_b) && sums && gains && stats && min_pixels >= 1 && sigma_ok(sigma_n) &&
           sigma_ok(sigma_g) && std::isfinite(g_min) && std::isfinite(g_max) && g_min > 0.f && g_min <= 1.f && g_max >= 1.f &&
           (mode == NM_EXPOSURE_PER_CHANNEL || mode == NM_EXPOSURE_COMMON);
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

}  // namespace

extern "C" int nm_mosaic_exposure_sums_dev(int n, int L, const unsigned char *const *frames, const int *link_a,
                                           const int *link_b, int fw, int fh, const float *mask, const float *H,
                                           const int *link_status, int stride, int lo, int hi, unsigned long long *sums,
                                           void *stream)
{
    if (!sums_args_ok(n, L, frames, link_a, link_b, fw, fh, H, stride, lo, hi, sums)) return (int)hipErrorInvalidValue;
    NM_RETURN_IF(nmp::launch_zero_u64(sums, (size_t)L * SUMS, nm_stream(stream)));
    const Lattice T = lattice_of(fw, fh, stride);
    if (T.tiles == 0) return 0;                                    // a stride beyond the frame: an empty lattice, all sums 0
    int parts = nm_divup(GRID_TARGET, L);
    parts = parts > MAX_PARTS ? MAX_PARTS : parts;
    parts = parts > T.tiles ? T.tiles : parts;
    SumsArgs A;
    nmp::fill_slots_as(A.frames, frames, 0, n);
    A.X = link_index(L, link_a, link_b);
    hipLaunchKernelGGL(mosaic_exposure_sums_kernel, dim3(parts, L), dim3(THREADS), 0, nm_stream(stream), A, fw, fh, mask, H,
                       link_status, stride, lo, hi, T.lw, T.lh, T.tiles_x, T.tiles, sums);
    NM_LAUNCH_CHECK();
    return 0;
}

extern "C" int nm_mosaic_exposure_sums_host(int n, int L, const unsigned char *const *frames, const int *link_a,
                                            const int *link_b, int fw, int fh, const float *mask, const float *H,
                                            const int *link_status, int stride, int lo, int hi, unsigned long long *sums)
{
    if (!sums_args_ok(n, L, frames, link_a, link_b, fw, fh, H, stride, lo, hi, sums)) return (int)hipErrorInvalidValue;
    const Lattice T = lattice_of(fw, fh, stride);
    for (int l = 0; l < L; ++l) {
        u64 *s = sums + (size_t)l * SUMS;
        for (int q = 0; q < SUMS; ++q) s[q] = 0;
        if (!nml::usable(link_status ? link_status[l] : 1, H + 9 * l)) continue;
        const Frames F{reinterpret_cast<const uchar4 *>(frames[link_a[l]]), reinterpret_cast<const uchar4 *>(frames[link_b[l]]),
                       mask, fw, fh};
        for (int v = 0; v < T.lh; ++v)
            for (int u = 0; u < T.lw; ++u) add_pixel(F, H + 9 * l, lo, hi, stride * u + stride / 2, stride * v + stride / 2, s);
    }
    return 0;
}

extern "C" int nm_mosaic_gains_dev(int n, int L, const int *link_a, const int *link_b, const unsigned long long *sums,
                                   const int *link_status, int min_pixels, double sigma_n, double sigma_g, float g_min,
                                   float g_max, int mode, float *gains, double *stats, void *stream)
{
    if (!gains_args_ok(n, L, link_a, link_b, sums, min_pixels, sigma_n, sigma_g, g_min, g_max, mode, gains, stats))
        return (int)hipErrorInvalidValue;
    const Params P{n, L, min_pixels, mode, sigma_n, sigma_g, g_min, g_max};
    hipLaunchKernelGGL(mosaic_gains_kernel, dim3(1), dim3(SOLVE_THREADS), 0, nm_stream(stream), P,
                       link_index(L, link_a, link_b), sums, link_status, gains, stats);
    NM_LAUNCH_CHECK();
    return 0;
}

extern "C" int nm_mosaic_gains_host(int n, int L, const int *link_a, const int *link_b, const unsigned long long *sums,
                                    const int *link_status, int min_pixels, double sigma_n, double sigma_g, float g_min,
                                    float g_max, int mode, float *gains, double *stats)
{
    if (!gains_args_ok(n, L, link_a, link_b, sums, min_pixels, sigma_n, sigma_g, g_min, g_max, mode, gains, stats))
        return (int)hipErrorInvalidValue;
    const Params P{n, L, min_pixels, mode, sigma_n, sigma_g, g_min, g_max};
    const LinkIdx X = link_index(L, link_a, link_b);
    unsigned char usable[MAX_LINKS];
    int links = 0, frames = 0;
    mark_links(P, X, sums, link_status, usable, links, frames);
    const int systems = mode == NM_EXPOSURE_COMMON ? 1 : 3;
    std::vector<double> M((size_t)MAX_FRAMES * LD), g((size_t)3 * MAX_FRAMES, 0.0);
    bool solved = links > 0;
    for (int c = 0; c < systems && solved; ++c) {
        for (int i = 0; i < n; ++i) assemble_row(P, X, sums, usable, c, i, M.data() + (size_t)i * LD);
        solved = nmc::chol_solve_serial(M.data(), LD, n, g.data() + (size_t)c * MAX_FRAMES);
    }
    double cost[6];
    for (int t = 0; t < 6; ++t) {
        const int c = t % 3, sys = systems == 1 ? 0 : c;
        cost[t] = cost_of(P, X, sums, usable, sys, (t < 3 || !solved) ? nullptr : g.data() + (size_t)sys * MAX_FRAMES);
    }
    if (solved)
        for (int q = 0; q < systems * n; ++q) solved = solved && std::isfinite(g[(size_t)(q / n) * MAX_FRAMES + q % n]);
    if (!solved) {
        write_unit(P, gains, stats, cost, links, frames, links > 0 ? NM_EXPOSURE_END_SINGULAR : NM_EXPOSURE_END_NO_LINK);
        return 0;
    }
    for (int k = 0; k < n; ++k)
        for (int c = 0; c < 3; ++c)
            gains[3 * k + c] = clamp_gain(g[(size_t)(systems == 1 ? 0 : c) * MAX_FRAMES + k], g_min, g_max);
    for (int t = 0; t < 6; ++t) stats[t] = cost[t];
    stats[6] = (double)links; stats[7] = (double)frames; stats[8] = (double)NM_EXPOSURE_END_OK;
    return 0;
}
