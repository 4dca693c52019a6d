// nm_link_verify.hip -- batched link verification for gfx950: is the map of a frame pair fit to be chained by the mosaic
// plan? Four gates per pair (usable, support, geometry, photometric; include/nm_abi.h has the written semantics). No
// reference counterpart. TWO launches per call whatever n is, on the caller's stream, no allocation, no synchronisation,
// no host read:
//   accumulate  grid (parts, n). The lattice walk over A (one of three copies: nm_lattice.hpp): a workgroup of four waves
//               walks the tiles blockIdx.x, blockIdx.x + parts, ..: a wave takes a lattice row, its lanes 64 neighbouring
//               lattice columns (at stride 1 one coalesced 256-byte read of A), each lane gathers its four taps of B. The
//               seven sums are integers: u64 per lane -> nmw::wave_reduce -> the four waves through LDS -> one row of
//               partials per workgroup in the workspace (plain vector stores, no atomics, no reset).
//   finalize    grid n. A workgroup adds its pair's rows of partials (integers: any order gives the same totals), one
//               lane runs gates 1-3 and the fp64 finalize and writes status_out, reason and stats.
// The arithmetic is nm_link_verify_math.hpp, shared with the host twin below: both agree bit for bit.
#include <cmath>

#include "nm_common.hpp"
#include "nm_lattice.hpp"
#include "nm_link_verify_math.hpp"
#include "nm_pair_batch.hpp"
#include "../../include/nm_abi.h"

namespace {

using namespace nml;
using namespace nmlat;

static_assert(NM_LINK_VERIFY_MAX_BATCH == nmp::MAX_BATCH, "public header and pair-batch convention disagree");

constexpr int MAX_PARTS = 256;              // workgroups (rows of partials) per pair
constexpr int PART_STRIDE = 8;              // u64 per row of partials: the seven sums and one of padding (64 bytes)

__global__ __launch_bounds__(THREADS) void link_verify_accumulate_kernel(const FrameTables T, int fw, int fh,
                                                                         const float *__restrict__ mask,
                                                                         const float *__restrict__ H,
                                                                         const int *__restrict__ status_in, int stride,
                                                                         int lw, int lh, int tiles_x, int tiles,
                                                                         u64 *__restrict__ partials)
{
    __shared__ u64 part[WAVES][SUMS];
    const int k = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float Hk[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) Hk[q] = H[k * 9 + q];
    if (!usable(status_in ? status_in[k] : 1, Hk)) return;      // uniform: the finalize does not read this pair's rows
    const Frames F{T.a[k], T.b[k], mask, fw, fh};
    u64 s[SUMS] = {0, 0, 0, 0, 0, 0, 0};
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {        // the lattice walk: one of three copies (nm_lattice.hpp)
        const int u = (t % tiles_x) * TILE_W + lane, v0 = (t / tiles_x) * TILE_H;
        if (u < lw)
            for (int r = wave; r < TILE_H && v0 + r < lh; r += WAVES)
                add_pixel(F, Hk, stride * u + stride / 2, stride * (v0 + r) + stride / 2, s);
    }
    const u64 total = nmw::block_totals<WAVES>(s, part);
    if (tid < SUMS) partials[((size_t)k * MAX_PARTS + blockIdx.x) * PART_STRIDE + tid] = total;
}

__global__ __launch_bounds__(THREADS) void link_verify_finalize_kernel(int fw, int fh, const float *__restrict__ H,
                                                                       const int *__restrict__ status_in,
                                                                       const int *__restrict__ inliers, int min_inliers,
                                                                       float max_area_ratio, float min_overlap,
                                                                       float min_ncc, int parts,
                                                                       const u64 *__restrict__ partials,
                                                                       int *__restrict__ status_out,
                                                                       int *__restrict__ reason, double *__restrict__ stats)
{
    __shared__ u64 part[WAVES][SUMS];
    __shared__ u64 tot[SUMS];
    const int k = blockIdx.x, tid = threadIdx.x;
    float Hk[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) Hk[q] = H[k * 9 + q];
    if (!usable(status_in ? status_in[k] : 1, Hk)) {            // uniform
        if (tid < STATS) stats[k * STATS + tid] = 0.0;
        if (tid == 0) { status_out[k] = 0; reason[k] = NM_LINK_UNUSABLE; }
        return;
    }
    u64 s[SUMS] = {0, 0, 0, 0, 0, 0, 0};
    for (int r = tid; r < parts; r += THREADS)
#pragma unroll
        for (int q = 0; q < SUMS; ++q) s[q] += partials[((size_t)k * MAX_PARTS + r) * PART_STRIDE + q];
    const u64 total = nmw::block_totals<WAVES>(s, part);
    if (tid < SUMS) tot[tid] = total;
    __syncthreads();
    if (tid == 0) {
        u64 sums[SUMS];
        for (int q = 0; q < SUMS; ++q) sums[q] = tot[q];
        double out[STATS];
        int why = finalize(sums, min_overlap, min_ncc, out);
        if (inliers && inliers[k] < min_inliers) why |= NM_LINK_FEW_INLIERS;
        if (!geometry_ok(Hk, fw, fh, max_area_ratio)) why |= NM_LINK_BAD_GEOMETRY;
        for (int q = 0; q < STATS; ++q) stats[k * STATS + q] = out[q];
        reason[k] = why; status_out[k] = why == 0 ? 1 : 0;
    }
}

// ---- the host twin: the same functions, the lattice walked row by row ----
void host_sums(const Frames &F, const float *H, int stride, u64 s[SUMS])
{
    const Lattice L = lattice_of(F.fw, F.fh, stride);
    for (int q = 0; q < SUMS; ++q) s[q] = 0;
    for (int v = 0; v < L.lh; ++v)
        for (int u = 0; u < L.lw; ++u) add_pixel(F, H, stride * u + stride / 2, stride * v + stride / 2, s);
}

bool lv_args_ok(int n, const float *const *grayA, const float *const *grayB, int fw, int fh, const float *H, int stride,
                int min_inliers, float max_area_ratio, float min_overlap, float min_ncc, const int *status_out,
                const int *reason, const double *stats)
{
    if (!std::isfinite(max_area_ratio) || !std::isfinite(min_overlap) || !std::isfinite(min_ncc) || max_area_ratio < 1.0f ||
        min_inliers < 0)
        return false;
    return frames_ok(n, grayA, grayB, fw, fh, H, stride) && nmp::tables_ok(n, {}, {}, {status_out, reason, stats});
}

}  // namespace

extern "C" size_t nm_link_verify_workspace_bytes(int n)
{
    return (n >= 1 && n <= nmp::MAX_BATCH) ? (size_t)n * MAX_PARTS * PART_STRIDE * sizeof(u64) : 0;
}

extern "C" int nm_link_verify_batch_dev_f32(int n, const float *const *grayA, const float *const *grayB, int fw, int fh,
                                            const float *mask, const float *H, const int *status_in, const int *inliers,
                                            int stride, int min_inliers, float max_area_ratio, float min_overlap,
                                            float min_ncc, int *status_out, int *reason, double *stats, void *workspace,
                                            void *stream)
{
    if (!lv_args_ok(n, grayA, grayB, fw, fh, H, stride, min_inliers, max_area_ratio, min_overlap, min_ncc, status_out, reason,
                    stats) || !workspace)
        return (int)hipErrorInvalidValue;
    const Lattice L = lattice_of(fw, fh, stride);
    const int parts = L.tiles < MAX_PARTS ? L.tiles : MAX_PARTS;
    u64 *partials = static_cast<u64 *>(workspace);
    if (parts > 0) {                                             // a stride beyond the frame: an empty lattice, all sums 0
        FrameTables T;
        nmp::fill_slots(T.a, grayA, 0, n);
        nmp::fill_slots(T.b, grayB, 0, n);
        hipLaunchKernelGGL(link_verify_accumulate_kernel, dim3(parts, n), dim3(THREADS), 0, nm_stream(stream), T, fw, fh, mask,
                           H, status_in, stride, L.lw, L.lh, L.tiles_x, L.tiles, partials);
        NM_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(link_verify_finalize_kernel, dim3(n), dim3(THREADS), 0, nm_stream(stream), fw, fh, H, status_in,
                       inliers, min_inliers, max_area_ratio, min_overlap, min_ncc, parts, partials, status_out, reason, stats);
    NM_LAUNCH_CHECK();
    return 0;
}

extern "C" int nm_link_verify_host_f32(int n, const float *const *grayA, const float *const *grayB, int fw, int fh,
                                       const float *mask, const float *H, const int *status_in, const int *inliers,
                                       int stride, int min_inliers, float max_area_ratio, float min_overlap, float min_ncc,
                                       int *status_out, int *reason, double *stats)
{
    if (!lv_args_ok(n, grayA, grayB, fw, fh, H, stride, min_inliers, max_area_ratio, min_overlap, min_ncc, status_out, reason,
                    stats))
        return (int)hipErrorInvalidValue;
    for (int k = 0; k < n; ++k) {
        double *out = stats + (size_t)k * STATS;
        if (!usable(status_in ? status_in[k] : 1, H + 9 * k)) {
            for (int q = 0; q < STATS; ++q) out[q] = 0.0;
            status_out[k] = 0; reason[k] = NM_LINK_UNUSABLE;
            continue;
        }
        u64 s[SUMS];
        host_sums(Frames{grayA[k], grayB[k], mask, fw, fh}, H + 9 * k, stride, s);
        int why = finalize(s, min_overlap, min_ncc, out);
        if (inliers && inliers[k] < min_inliers) why |= NM_LINK_FEW_INLIERS;
        if (!geometry_ok(H + 9 * k, fw, fh, max_area_ratio)) why |= NM_LINK_BAD_GEOMETRY;
        reason[k] = why; status_out[k] = why == 0 ? 1 : 0;
    }
    return 0;
}

extern "C" int nm_link_verify_sums_host_f32(int n, const float *const *grayA, const float *const *grayB, int fw, int fh,
                                            const float *mask, const float *H, int stride, unsigned long long *sums)
{
    if (!frames_ok(n, grayA, grayB, fw, fh, H, stride) || !sums) return (int)hipErrorInvalidValue;
    for (int k = 0; k < n; ++k) {
        u64 *s = sums + (size_t)k * SUMS;
        for (int q = 0; q < SUMS; ++q) s[q] = 0;
        if (nmp::finite9(H + 9 * k)) host_sums(Frames{grayA[k], grayB[k], mask, fw, fh}, H + 9 * k, stride, s);
    }
    return 0;
}
