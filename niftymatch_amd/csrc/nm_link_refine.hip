// nm_link_refine.hip -- batched direct (photometric) refinement of link maps for gfx950: a few inverse compositional
// Gauss-Newton steps on the level difference of two gray planes over the verification's lattice, started from the refit's
// map, with gain and bias (include/nm_abi.h has the written semantics). No reference counterpart. TWO launches per
// iteration whatever n is, on the caller's stream, no allocation, no synchronisation, no host read; an iteration boundary
// is a launch boundary, no kernel waits for another workgroup:
//   accumulate  grid (min(tiles, 256), n), 256 threads. Workgroup g walks the lattice tiles g, g + 256, .., wave w the
//               tile rows w, w + 4, .., a lane one column. Each lane keeps its 67 fp64 sums in registers across its
//               tiles; then nmw::wave_reduce per sum, the four waves through LDS in ascending order, one row of
//               partials per workgroup in the workspace (plain vector stores, no atomics, no reset). The first
//               iteration reads H_in and status_in, the later ones the pair's state in the workspace; the workgroups
//               of a pair that has ended leave at once.
//   solve       grid n. Thread q < 67 adds column q of the pair's rows of partials in ascending order; one lane runs the
//               Cholesky solve, the step and the stop rule, writes the state and, for a pair that ends, its outputs.
// The arithmetic is nm_link_refine_math.hpp, shared with the host twin below, which walks the same virtual lanes and
// the same trees serially: both agree bit for bit.
#include <cmath>

#include "nm_common.hpp"
#include "nm_link_refine_math.hpp"
#include "nm_pair_batch.hpp"
#include "nm_wave_dev.hpp"
#include "../../include/nm_abi.h"

namespace {

using namespace nmlr;

static_assert(NM_LINK_REFINE_MAX_BATCH == nmp::MAX_BATCH, "public header and pair-batch convention disagree");
static_assert(SUMS == 67 && sizeof(State) == 128, "the workspace layout of nm_abi.h");

constexpr int ROW = 68;                     // doubles per row of partials: the 67 sums and one of padding
constexpr int SOLVE_THREADS = 128;
using nmlat::FrameTables; using nmlat::frames_ok; using nmlat::lattice_of;

__global__ __launch_bounds__(THREADS) void link_refine_accumulate_kernel(const FrameTables T, int fw, int fh,
                                                                         const float *__restrict__ mask,
                                                                         const float *__restrict__ H_in,
                                                                         const int *__restrict__ status_in,
                                                                         const State *__restrict__ states, int first,
                                                                         int stride, int lw, int lh, int tiles_x, int tiles,
                                                                         double *__restrict__ partials)
{
    __shared__ double part[WAVES][SUMS];
    const int k = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float Hk[9];
    bool active;                                                 // uniform over the workgroup
    if (first) {
#pragma unroll
        for (int q = 0; q < 9; ++q) Hk[q] = H_in[k * 9 + q];
        active = nml::usable(status_in ? status_in[k] : 1, Hk);
    } else {
#pragma unroll
        for (int q = 0; q < 9; ++q) Hk[q] = states[k].Hf[q];
        active = states[k].active != 0;
    }
    if (!active) return;                                         // the solve does not read this pair's rows
    const Frames F{T.a[k], T.b[k], mask, fw, fh};
    const Norm G = norm_of(fw, fh);
    double s[SUMS];
#pragma unroll
    for (int q = 0; q < SUMS; ++q) s[q] = 0.0;
    walk_lane(F, G, Hk, stride, Lattice{lw, lh, tiles_x, tiles}, blockIdx.x, wave, lane, s);
#pragma unroll
    for (int q = 0; q < SUMS; ++q) {
        const double v = nmw::wave_reduce(s[q], nmw::Sum());
        if (lane == 0) part[wave][q] = v;
    }
    __syncthreads();
    if (tid < SUMS) {
        double t = 0.0;
        for (int w = 0; w < WAVES; ++w) t = t + part[w][tid];
        partials[((size_t)k * PARTS + blockIdx.x) * ROW + tid] = t;
    }
}

__global__ __launch_bounds__(SOLVE_THREADS) void link_refine_solve_kernel(const Params P, int it, int last,
                                                                          const float *__restrict__ H_in,
                                                                          const int *__restrict__ status_in, int parts,
                                                                          const double *__restrict__ partials, State *states,
                                                                          float *__restrict__ H_out,
                                                                          int *__restrict__ status_out,
                                                                          double *__restrict__ stats)
{
    __shared__ double tot[SUMS];
    __shared__ double work[WORK];
    const int k = blockIdx.x, tid = threadIdx.x;
    float Hk[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) Hk[q] = H_in[k * 9 + q];
    const int allowed = status_in ? status_in[k] : 1;
    const bool walked = it == 0 ? nml::usable(allowed, Hk) : states[k].active != 0;   // uniform
    if (it > 0 && !walked) return;                               // ended earlier: its outputs are written
    if (tid < SUMS) {
        double t = 0.0;
        if (walked)
            for (int r = 0; r < parts; ++r) t = t + partials[((size_t)k * PARTS + r) * ROW + tid];
        tot[tid] = t;
    }
    __syncthreads();
    if (tid == 0) {
        State st;
        if (it > 0) st = states[k];
        step(P, it, last, Hk, allowed, tot, work, st, H_out + 9 * k, status_out + k, stats + (size_t)STATS * k);
        states[k] = st;
    }
}

// ---- the host twin: the same functions, the virtual lanes, the trees and the rows walked serially ----
void host_sums(const Frames &F, const float *H, int stride, double tot[SUMS])
{
    const Lattice L = lattice_of(F.fw, F.fh, stride);
    const int parts = L.tiles < PARTS ? L.tiles : PARTS;
    const Norm G = norm_of(F.fw, F.fh);
    for (int q = 0; q < SUMS; ++q) tot[q] = 0.0;
    static thread_local double v[64][SUMS];
    for (int g = 0; g < parts; ++g) {
        double row[SUMS];
        for (int q = 0; q < SUMS; ++q) row[q] = 0.0;
        for (int w = 0; w < WAVES; ++w) {
            for (int l = 0; l < 64; ++l) {
                for (int q = 0; q < SUMS; ++q) v[l][q] = 0.0;
                walk_lane(F, G, H, stride, L, g, w, l, v[l]);
            }
            for (int d = 32; d >= 1; d >>= 1)
                for (int l = 0; l < d; ++l)
                    for (int q = 0; q < SUMS; ++q) v[l][q] = v[l][q] + v[l + d][q];
            for (int q = 0; q < SUMS; ++q) row[q] = row[q] + v[0][q];
        }
        for (int q = 0; q < SUMS; ++q) tot[q] = tot[q] + row[q];
    }
}

bool lr_args_ok(int n, const float *const *grayA, const float *const *grayB, int fw, int fh, const float *H, int model,
                int stride, int iterations, int min_pixels, float max_step, const float *H_out, const int *status_out,
                const double *stats)
{
    if (model < NM_LINK_REFINE_TRANSLATION || model > NM_LINK_REFINE_HOMOGRAPHY || iterations < 1 ||
        iterations > NM_LINK_REFINE_MAX_ITERATIONS || min_pixels < 1 || !std::isfinite(max_step) || !(max_step > 0.0f))
        return false;
    return frames_ok(n, grayA, grayB, fw, fh, H, stride) && nmp::tables_ok(n, {}, {}, {H_out, status_out, stats});
}

}  // namespace

extern "C" size_t nm_link_refine_workspace_bytes(int n)
{
    return (n >= 1 && n <= nmp::MAX_BATCH) ? (size_t)n * ((size_t)PARTS * ROW * sizeof(double) + sizeof(State)) : 0;
}

extern "C" int nm_link_refine_batch_dev_f32(int n, const float *const *grayA, const float *const *grayB, int fw, int fh,
                                            const float *mask, const float *H_in, const int *status_in, int model, int stride,
                                            int iterations, int min_pixels, float max_step, float *H_out, int *status_out,
                                            double *stats, void *workspace, void *stream)
{
    if (!lr_args_ok(n, grayA, grayB, fw, fh, H_in, model, stride, iterations, min_pixels, max_step, H_out, status_out, stats) ||
        !workspace)
        return (int)hipErrorInvalidValue;
    const Lattice L = lattice_of(fw, fh, stride);
    const int parts = L.tiles < PARTS ? L.tiles : PARTS;
    double *partials = static_cast<double *>(workspace);
    State *states = reinterpret_cast<State *>(partials + (size_t)n * PARTS * ROW);
    const Params P{fw, fh, model, min_pixels, max_step};
    FrameTables T;
    nmp::fill_slots(T.a, grayA, 0, n);
    nmp::fill_slots(T.b, grayB, 0, n);
    for (int it = 0; it < iterations; ++it) {
        if (parts > 0) {                                         // a stride beyond the frame: an empty lattice, all sums 0
            hipLaunchKernelGGL(link_refine_accumulate_kernel, dim3(parts, n), dim3(THREADS), 0, nm_stream(stream), T, fw, fh,
                               mask, H_in, status_in, states, it == 0 ? 1 : 0, stride, L.lw, L.lh, L.tiles_x, L.tiles, partials);
            NM_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(link_refine_solve_kernel, dim3(n), dim3(SOLVE_THREADS), 0, nm_stream(stream), P, it, iterations - 1,
                           H_in, status_in, parts, partials, states, H_out, status_out, stats);
        NM_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int nm_link_refine_host_f32(int n, const float *const *grayA, const float *const *grayB, int fw, int fh,
                                       const float *mask, const float *H_in, const int *status_in, int model, int stride,
                                       int iterations, int min_pixels, float max_step, float *H_out, int *status_out,
                                       double *stats)
{
    if (!lr_args_ok(n, grayA, grayB, fw, fh, H_in, model, stride, iterations, min_pixels, max_step, H_out, status_out, stats))
        return (int)hipErrorInvalidValue;
    const Params P{fw, fh, model, min_pixels, max_step};
    for (int k = 0; k < n; ++k) {
        const Frames F{grayA[k], grayB[k], mask, fw, fh};
        const int allowed = status_in ? status_in[k] : 1;
        State st;
        double tot[SUMS], work[WORK];
        for (int it = 0; it < iterations; ++it) {
            const bool walked = it == 0 ? nml::usable(allowed, H_in + 9 * k) : st.active != 0;
            if (it > 0 && !walked) break;
            for (int q = 0; q < SUMS; ++q) tot[q] = 0.0;
            if (walked) host_sums(F, it == 0 ? H_in + 9 * k : st.Hf, stride, tot);
            step(P, it, iterations - 1, H_in + 9 * k, allowed, tot, work, st, H_out + 9 * k, status_out + k,
                 stats + (size_t)STATS * k);
        }
    }
    return 0;
}

extern "C" int nm_link_refine_sums_host_f32(int n, const float *const *grayA, const float *const *grayB, int fw, int fh,
                                            const float *mask, const float *H, int stride, double *sums)
{
    if (!frames_ok(n, grayA, grayB, fw, fh, H, stride) || !sums) return (int)hipErrorInvalidValue;
    for (int k = 0; k < n; ++k) {
        double *s = sums + (size_t)k * SUMS;
        for (int q = 0; q < SUMS; ++q) s[q] = 0.0;
        if (nmp::finite9(H + 9 * k)) host_sums(Frames{grayA[k], grayB[k], mask, fw, fh}, H + 9 * k, stride, s);
    }
    return 0;
}
