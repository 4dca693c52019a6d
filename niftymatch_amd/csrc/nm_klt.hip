// nm_klt.hip -- the gray pyramid of up to NM_KLT_MAX_BATCH frames and the pyramidal Lucas-Kanade point tracker between frame
// pairs, for gfx950 (include/nm_abi.h, "Gray pyramid and point tracking", has the written semantics). No reference
// counterpart. On the caller's stream, no allocation, no synchronisation, no host read; no workgroup waits for another.
//   pyramid   max(levels - 1, 1) launches for all frames. A workgroup of four waves takes a unit = (frame, tile of 32 x 8
//             pixels of level l + 1), grid-stride over the units: the 72 x 19 source pixels of the tile go to LDS (16-byte
//             loads where the plane's width is a multiple of 4 and every block is 16-byte aligned, clamped scalars at the
//             plane's edge and otherwise), the row pass writes 32 x 19 values to a second tile, the column pass one pixel
//             per thread. The first launch reads the caller's gray planes and also stores them as level 0, each tile the
//             64 x 16 source pixels it is centred on (the only launch when levels = 1).
//   mask      ONE launch for the whole block of byte planes: a thread per byte. A pixel of level l is 1 exactly when the
//             level-0 rectangle its 25-tap chain reaches is seen everywhere (clamping keeps the chain's reach a rectangle),
//             so no level waits for the one below. Once per camera, not per frame.
//   tracker   nmp::launch_zero_u64 on count, then ONE launch per 32 pair slots (n <= 32: one; eleven pointer tables of 64
//             slots would be 5.5 KB of the 4 KB of kernel arguments, the guided matcher's split). A wave takes a unit =
//             (pair, chunk of 16 rows) in four trips of four rows: 16 lanes per point (8 and 32 are compiled too:
//             nm_klt_set_lanes). A lane holds taps lane, lane + 16, ... of T, gx, gy in registers (15 at radius 7) and
//             gathers its samples from the planes, four pixels a sample (that the patch stays in the vector L1 is a
//             supposition: no counter was read); the integer sums are reduced inside the 16 lanes with nmw::wave_sum<8>.
//             Lanes of finished points idle; the wave leaves the iteration loop on a ballot.
//             Lanes per point, MEASURED (tools/kklt.py on one MI355X, 1080p, levels 4, no gates, median us of 5 rounds;
//             VGPRs / waves per SIMD of the three kernels: 8 lanes 256 / 1, 16 lanes 210 / 2, 32 lanes 156 / 3):
//               pairs x points, radius    8 lanes   16 lanes   32 lanes
//               16 x  4 096, r = 3           972        642        712
//               16 x  4 096, r = 7         2 813      1 697      1 837
//               64 x 12 288, r = 3        11 259      7 577      7 352
//               64 x 12 288, r = 7        31 101     19 891     18 842
//             8 lanes lose everywhere by 1.5 to 1.7 x (29 taps a lane, one wave per SIMD). 16 against 32 is close: 16 is
//             8 to 11 % faster on 16 pairs of 4 096 points, 32 is 3 to 8 % faster on 64 pairs. 16 stays the default: a
//             mosaic chunk links tens of pairs of a few thousand points more often than 64 pairs of 12 288.
//             Sums: 64-bit words (v_mad_i64_i32 per tap); two 32-bit halves were NOT measured. A lane's part of sum e gx
//             is at most 15 x 4080^2 < 2^28, but the point's total reaches 225 x 4080^2 > 2^31, so the reduction must be
//             64 bits wide; keeping the lane's part in 64 bits as well costs no second code path and lets the host twin
//             (one lane, 225 taps) run the same body.
// The arithmetic is nm_klt_math.hpp, shared with the host twins below: all agree bit for bit.
#include <atomic>
#include <cstring>
#include <vector>

#include "../../include/nm_abi.h"
#include "nm_common.hpp"
#include "nm_klt_math.hpp"
#include "nm_pair_batch.hpp"

namespace {

using namespace nmk;

constexpr int THREADS = 256, WAVES = 4, BLOCKS_PER_CU = 8;
constexpr int OW = 32, OH = 8, IW = 2 * OW + 8, IH = 2 * OH + 3;       // a pyramid tile and its source pixels
constexpr int HALF = 32;                                               // pair slots per tracker launch
constexpr int CHUNK = 16;                                              // rows per unit
constexpr int DEFAULT_GROUP = 16;                                      // lanes per point: 8, 16 or 32 (nm_klt_set_lanes)

std::atomic<int> g_grid_cap{0};                                        // nm_klt_set_grid_cap; 0: the default
std::atomic<int> g_lanes{0};                                           // nm_klt_set_lanes; 0: the default

struct PyrArgs {                                                       // 1 KB of the 4 KB of kernel arguments
    const float *src[nmp::MAX_BATCH];
    float *dst[nmp::MAX_BATCH];
};
struct KltArgs {                                                       // 2.75 KB
    const float *pyrA[HALF], *pyrB[HALF], *sx[HALF], *sy[HALF];
    const int *d_nA[HALF];
    float *dx[HALF], *dy[HALF];
    int *matches[HALF];
    unsigned char *reason[HALF];
    float *residual[HALF], *fb[HALF];
};
static_assert(sizeof(PyrArgs) + 128 < 4096 && sizeof(KltArgs) + 256 < 4096, "kernel arguments exceed 4 KB");

int grid_of(long long units)
{
    const int cap = g_grid_cap.load();                 // nm_klt_set_grid_cap: tests make small grids walk far
    return cap > 0 ? (int)(units < cap ? units : cap) : nm_fill_grid(units, BLOCKS_PER_CU);
}

// Level l + 1 from level l (w x h) of every frame. COPY: the source is the caller's plane a.src[k], stored as level 0 too;
// else it is level l of the block a.dst[k]. levels1: only the copy (levels = 1). WIDE: 16-byte loads and stores.
template <bool COPY, bool WIDE>
__global__ __launch_bounds__(THREADS) void pyramid_kernel(const PyrArgs a, int n, int w, int h, long long off_src,
                                                          long long off_dst, int only_copy)
{
    __shared__ __attribute__((aligned(16))) float s_in[IH][IW];
    __shared__ float s_h[IH][OW];
    const int tid = threadIdx.x;
    const int w1 = (w + 1) >> 1, h1 = (h + 1) >> 1;
    const int tx = (w1 + OW - 1) / OW, ty = (h1 + OH - 1) / OH;
    const long long units = (long long)n * tx * ty;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const int bx = (int)(u % tx);
        const long long t = u / tx;
        const int by = (int)(t % ty), k = (int)(t / ty);
        const float *src = COPY ? a.src[k] : a.dst[k] + off_src;
        float *block = a.dst[k];
        const int X0 = bx * OW, Y0 = by * OH, x_first = 2 * X0 - 4, y_first = 2 * Y0 - 2;
        __syncthreads();                                           // the previous unit's tiles are read out
        for (int i = tid; i < IH * (IW / 4); i += THREADS) {
            const int ry = i / (IW / 4), c4 = i - ry * (IW / 4);
            const int y = clampi(y_first + ry, h - 1), x = x_first + 4 * c4;
            const float *row = src + (size_t)y * w;
            float4 v;
            if (WIDE && x >= 0 && x + 3 < w) v = *reinterpret_cast<const float4 *>(row + x);
            else v = make_float4(row[clampi(x, w - 1)], row[clampi(x + 1, w - 1)], row[clampi(x + 2, w - 1)], row[clampi(x + 3, w - 1)]);
            *reinterpret_cast<float4 *>(&s_in[ry][4 * c4]) = v;
        }
        __syncthreads();
        if (COPY) {                                                // level 0: the 64 x 16 pixels this tile is centred on
            const int ry = tid >> 4, c4 = tid & 15, y = 2 * Y0 + ry, x = 2 * X0 + 4 * c4;
            if (y < h && x < w) {
                const float4 v = *reinterpret_cast<const float4 *>(&s_in[ry + 2][4 * c4 + 4]);
                float *out = block + (size_t)y * w + x;
                if (WIDE && x + 3 < w) *reinterpret_cast<float4 *>(out) = v;
                else {
                    out[0] = v.x;
                    if (x + 1 < w) out[1] = v.y;
                    if (x + 2 < w) out[2] = v.z;
                    if (x + 3 < w) out[3] = v.w;
                }
            }
        }
        if (only_copy) continue;                                   // workgroup-uniform
        for (int i = tid; i < IH * OW; i += THREADS) {
            const int ry = i / OW, X = i - ry * OW, c = 2 * X + 4;
            s_h[ry][X] = binom5(s_in[ry][c - 2], s_in[ry][c - 1], s_in[ry][c], s_in[ry][c + 1], s_in[ry][c + 2]);
        }
        __syncthreads();
        const int X = tid & (OW - 1), Y = tid / OW;
        if (X0 + X < w1 && Y0 + Y < h1)
            block[off_dst + (size_t)(Y0 + Y) * w1 + (X0 + X)] =
                binom5(s_h[2 * Y][X], s_h[2 * Y + 1][X], s_h[2 * Y + 2][X], s_h[2 * Y + 3][X], s_h[2 * Y + 4][X]);
    }
}

// the mask block: byte g of it, for every g below its size (pad bytes between levels are 0)
__global__ __launch_bounds__(THREADS) void mask_pyramid_kernel(const float *__restrict__ mask, int fw, int fh, int levels,
                                                               unsigned char *__restrict__ out, long long total)
{
    for (long long g = (long long)blockIdx.x * THREADS + threadIdx.x; g < total; g += (long long)gridDim.x * THREADS) {
        int l = 0;
        long long base = 0;                                        // the level of byte g, by one running sum of the level sizes
        for (;; ++l) {
            const long long next = base + ((((long long)level_size(fw, l) * level_size(fh, l)) + 3) & ~3ll);
            if (l + 1 >= levels || next > g) break;
            base = next;
        }
        const long long idx = g - base;
        const int w = level_size(fw, l), h = level_size(fh, l);
        unsigned char seen = 0;
        if (idx < (long long)w * h) {
            int xlo = (int)(idx % w), xhi = xlo, ylo = (int)(idx / w), yhi = ylo;
            for (int j = l - 1; j >= 0; --j) {
                xlo = clampi(2 * xlo - 2, level_size(fw, j) - 1); xhi = clampi(2 * xhi + 2, level_size(fw, j) - 1);
                ylo = clampi(2 * ylo - 2, level_size(fh, j) - 1); yhi = clampi(2 * yhi + 2, level_size(fh, j) - 1);
            }
            bool all = true;
            for (int y = ylo; y <= yhi && all; ++y)
                for (int x = xlo; x <= xhi; ++x) all = all && seen_f32(mask[(size_t)y * fw + x]);
            seen = all ? 1 : 0;
        }
        out[g] = seen;
    }
}

// the device's executor: GROUP lanes per point, 64 / GROUP points per wave
template <int GROUP> struct DevX {
    static constexpr int L = GROUP, MAXT = (MAX_TAPS + GROUP - 1) / GROUP;
    int lane;                                                      // within the point's lanes
    int shift;                                                     // the first lane of the point in the wave
    __device__ __forceinline__ i64 sum(i64 v) const { return nmw::wave_sum<GROUP / 2>(v); }
    __device__ __forceinline__ bool any(bool b) const { return ((__ballot(b) >> shift) & ((1ull << GROUP) - 1ull)) != 0ull; }
    __device__ __forceinline__ bool any_point(bool b) const { return __ballot(b) != 0ull; }
};

template <int GROUP>
__global__ __launch_bounds__(THREADS) void klt_track_kernel(const KltArgs a, const Params q, int n, int capA,
                                                            const unsigned char *__restrict__ mask,
                                                            const float *__restrict__ H_in, const int *__restrict__ status_in,
                                                            u64 *__restrict__ count)
{
    const int tid = threadIdx.x, wl = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int TRIPS = CHUNK / (64 / GROUP);
    DevX<GROUP> x;
    x.lane = wl & (GROUP - 1);
    x.shift = wl & ~(GROUP - 1);
    const int g = wl / GROUP;
    const int chunks = (capA + CHUNK - 1) / CHUNK;
    const long long units = (long long)n * chunks, stride = (long long)gridDim.x * WAVES;
    for (long long u = (long long)blockIdx.x * WAVES + wave; u < units; u += stride) {      // wave-uniform
        const int k = (int)(u / chunks), c = (int)(u - (long long)k * chunks);
        const int nA = nmp::clip(*a.d_nA[k], capA);
        const float *A = a.pyrA[k], *B = a.pyrB[k], *sxp = a.sx[k], *syp = a.sy[k];
        float *dxp = a.dx[k], *dyp = a.dy[k], *rsp = a.residual[k], *fbp = a.fb[k];
        int *mt = a.matches[k];
        unsigned char *rp = a.reason[k];
        const float *H = H_in ? H_in + 9 * (size_t)k : nullptr;    // read in place: a local copy would live in scratch
        if (H && !((!status_in || status_in[k] == 1) && nmp::finite9(H))) H = nullptr;
        int tracked = 0;
        for (int trip = 0; trip < TRIPS; ++trip) {
            const int i = c * CHUNK + trip * (64 / GROUP) + g;
            const bool in_cap = i < capA, exists = i < nA;
            const float sx = exists ? sxp[i] : -1.f, sy = exists ? syp[i] : -1.f;
            const RowOut o = track_row(x, q, A, B, mask, exists && row_tried(sx, sy), sx, sy, H);
            const bool lead = in_cap && x.lane == 0;
            if (lead) {
                dxp[i] = o.dst_x; dyp[i] = o.dst_y;
                mt[i] = o.reason == 0 ? i : -1;
                if (rp) rp[i] = (unsigned char)o.reason;
                if (rsp) rsp[i] = o.residual;
                if (fbp) fbp[i] = o.fb_error;
            }
            tracked += nmw::wave_count(lead && o.reason == 0);
        }
        if (wl == 0 && tracked) atomicAdd(count + k, (u64)tracked);
    }
}

bool pyramid_ok(int n, const float *const *gray, int fw, int fh, int levels, float *const *pyr, const float *mask,
                const unsigned char *mask_pyr)
{
    if (n < 1 || n > nmp::MAX_BATCH || !shape_ok(fw, fh, levels) || (mask == nullptr) != (mask_pyr == nullptr)) return false;
    return nmp::tables_ok(n, {gray, pyr}, {}, {});
}

bool track_ok(int n, const float *const *pyrA, const float *const *pyrB, int fw, int fh, int levels,
              const float *const *src_x, const float *const *src_y, const int *const *d_nA, int capA, const float *H_in,
              const int *status_in, int radius, int iterations, float eps, float max_step, float min_eig, float max_residual,
              float fb_max, float *const *dst_x, float *const *dst_y, int *const *matches, const u64 *count,
              unsigned char *const *reason, float *const *residual, float *const *fb_error)
{
    if (!nmp::range_ok(n, capA) || !params_ok(fw, fh, levels, radius, iterations, eps, max_step, min_eig, max_residual, fb_max) ||
        (status_in && !H_in))
        return false;
    return nmp::tables_ok(n, {pyrA, pyrB, src_x, src_y, d_nA, dst_x, dst_y, matches}, {reason, residual, fb_error}, {count});
}

void pyramid_host_plane(const float *src, int w, int h, float *dst)
{
    const int w1 = (w + 1) >> 1, h1 = (h + 1) >> 1;
    std::vector<float> row((size_t)w1 * h);
    for (int y = 0; y < h; ++y)
        for (int X = 0; X < w1; ++X) {
            const float *s = src + (size_t)y * w;
            const int c = 2 * X;
            row[(size_t)y * w1 + X] = binom5(s[clampi(c - 2, w - 1)], s[clampi(c - 1, w - 1)], s[c], s[clampi(c + 1, w - 1)],
                                             s[clampi(c + 2, w - 1)]);
        }
    for (int Y = 0; Y < h1; ++Y)
        for (int X = 0; X < w1; ++X) {
            const int c = 2 * Y;
            dst[(size_t)Y * w1 + X] = binom5(row[(size_t)clampi(c - 2, h - 1) * w1 + X], row[(size_t)clampi(c - 1, h - 1) * w1 + X],
                                             row[(size_t)c * w1 + X], row[(size_t)clampi(c + 1, h - 1) * w1 + X],
                                             row[(size_t)clampi(c + 2, h - 1) * w1 + X]);
        }
}

}  // namespace

extern "C" {

int nm_klt_set_grid_cap(int cap) { return g_grid_cap.exchange(cap < 1 ? 0 : cap); }

int nm_klt_set_lanes(int lanes) { return g_lanes.exchange(lanes == 8 || lanes == 16 || lanes == 32 ? lanes : 0); }

size_t nm_gray_pyramid_floats(int fw, int fh, int levels)
{
    return shape_ok(fw, fh, levels) ? (size_t)level_offset(fw, fh, levels) : 0;
}

size_t nm_gray_pyramid_offset(int fw, int fh, int level)
{
    return (nm_size_ok(fw) && nm_size_ok(fh) && level >= 0 && level <= MAX_LEVELS) ? (size_t)level_offset(fw, fh, level) : 0;
}

int nm_gray_pyramid_batch_f32(int n, const float *const *gray, int fw, int fh, int levels, float *const *pyr, const float *mask,
                              unsigned char *mask_pyr, void *stream)
{
    if (!pyramid_ok(n, gray, fw, fh, levels, pyr, mask, mask_pyr)) return (int)hipErrorInvalidValue;
    PyrArgs a;
    nmp::fill_slots(a.src, gray, 0, n);
    nmp::fill_slots(a.dst, pyr, 0, n);
    size_t low = 0;
    for (int k = 0; k < n; ++k) low |= reinterpret_cast<size_t>(gray[k]) | reinterpret_cast<size_t>(pyr[k]);
    const hipStream_t st = nm_stream(stream);
    for (int l = 0; l < (levels > 1 ? levels - 1 : 1); ++l) {
        const int w = level_size(fw, l), h = level_size(fh, l);
        const bool wide = !(low & 15) && !(w & 3);
        const long long units = (long long)n * nm_divup((w + 1) >> 1, OW) * nm_divup((h + 1) >> 1, OH);
        const auto kernel = l == 0 ? (wide ? pyramid_kernel<true, true> : pyramid_kernel<true, false>)
                                   : (wide ? pyramid_kernel<false, true> : pyramid_kernel<false, false>);
        hipLaunchKernelGGL(kernel, dim3(grid_of(units)), dim3(THREADS), 0, st, a, n, w, h, level_offset(fw, fh, l),
                           level_offset(fw, fh, l + 1), levels == 1 ? 1 : 0);
        NM_LAUNCH_CHECK();
    }
    if (mask) {
        const long long total = level_offset(fw, fh, levels);
        hipLaunchKernelGGL(mask_pyramid_kernel, dim3(grid_of((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, mask, fw, fh,
                           levels, mask_pyr, total);
        NM_LAUNCH_CHECK();
    }
    return 0;
}

int nm_gray_pyramid_host_f32(int n, const float *const *gray, int fw, int fh, int levels, float *const *pyr, const float *mask,
                             unsigned char *mask_pyr)
{
    if (!pyramid_ok(n, gray, fw, fh, levels, pyr, mask, mask_pyr)) return (int)hipErrorInvalidValue;
    for (int k = 0; k < n; ++k) {
        std::memmove(pyr[k], gray[k], sizeof(float) * (size_t)fw * fh);
        for (int l = 0; l + 1 < levels; ++l)
            pyramid_host_plane(pyr[k] + level_offset(fw, fh, l), level_size(fw, l), level_size(fh, l),
                               pyr[k] + level_offset(fw, fh, l + 1));
    }
    if (mask) {                                                    // level by level, as the definition reads
        std::memset(mask_pyr, 0, (size_t)level_offset(fw, fh, levels));
        for (size_t p = 0; p < (size_t)fw * fh; ++p) mask_pyr[p] = seen_f32(mask[p]) ? 1 : 0;
        for (int l = 0; l + 1 < levels; ++l) {
            const int w = level_size(fw, l), h = level_size(fh, l), w1 = level_size(fw, l + 1), h1 = level_size(fh, l + 1);
            const unsigned char *s = mask_pyr + level_offset(fw, fh, l);
            unsigned char *d = mask_pyr + level_offset(fw, fh, l + 1);
            for (int Y = 0; Y < h1; ++Y)
                for (int X = 0; X < w1; ++X) {
                    unsigned char all = 1;
                    for (int v = -2; v <= 2; ++v)
                        for (int u = -2; u <= 2; ++u) all &= s[(size_t)clampi(2 * Y + v, h - 1) * w + clampi(2 * X + u, w - 1)];
                    d[(size_t)Y * w1 + X] = all;
                }
        }
    }
    return 0;
}

int nm_klt_track_batch_dev_f32(int n, const float *const *pyrA, const float *const *pyrB, int fw, int fh, int levels,
                               const unsigned char *mask_pyr, const float *const *src_x, const float *const *src_y,
                               const int *const *d_nA, int capA, const float *H_in, const int *status_in, int radius,
                               int iterations, float eps, float max_step, float min_eig, float max_residual, float fb_max,
                               float *const *dst_x, float *const *dst_y, int *const *matches, unsigned long long *count,
                               unsigned char *const *reason, float *const *residual, float *const *fb_error, void *stream)
{
    if (!track_ok(n, pyrA, pyrB, fw, fh, levels, src_x, src_y, d_nA, capA, H_in, status_in, radius, iterations, eps, max_step,
                  min_eig, max_residual, fb_max, dst_x, dst_y, matches, count, reason, residual, fb_error))
        return (int)hipErrorInvalidValue;
    const Params q = params_of(fw, fh, levels, radius, iterations, eps, max_step, min_eig, max_residual, fb_max);
    const hipStream_t st = nm_stream(stream);
    NM_RETURN_IF(nmp::launch_zero_u64(count, (size_t)n, st));
    const int lanes = g_lanes.load();
    const auto kernel = lanes == 8 ? klt_track_kernel<8> : (lanes == 32 ? klt_track_kernel<32> : klt_track_kernel<DEFAULT_GROUP>);
    for (int first = 0; first < n; first += HALF) {
        const int m = n - first < HALF ? n - first : HALF;
        KltArgs a;
        nmp::fill_slots(a.pyrA, pyrA, first, n); nmp::fill_slots(a.pyrB, pyrB, first, n);
        nmp::fill_slots(a.sx, src_x, first, n); nmp::fill_slots(a.sy, src_y, first, n);
        nmp::fill_slots(a.d_nA, d_nA, first, n);
        nmp::fill_slots(a.dx, dst_x, first, n); nmp::fill_slots(a.dy, dst_y, first, n);
        nmp::fill_slots(a.matches, matches, first, n);
        nmp::fill_slots(a.reason, reason, first, n);
        nmp::fill_slots(a.residual, residual, first, n); nmp::fill_slots(a.fb, fb_error, first, n);
        const long long units = (long long)m * nm_divup(capA, CHUNK);
        hipLaunchKernelGGL(kernel, dim3(grid_of((units + WAVES - 1) / WAVES)), dim3(THREADS), 0, st, a, q, m, capA,
                           mask_pyr, H_in ? H_in + 9 * (size_t)first : nullptr, status_in ? status_in + first : nullptr,
                           count + first);
        NM_LAUNCH_CHECK();
    }
    return 0;
}

int nm_klt_track_host_f32(int n, const float *const *pyrA, const float *const *pyrB, int fw, int fh, int levels,
                          const unsigned char *mask_pyr, const float *const *src_x, const float *const *src_y,
                          const int *const *nA, int capA, const float *H_in, const int *status_in, int radius, int iterations,
                          float eps, float max_step, float min_eig, float max_residual, float fb_max, float *const *dst_x,
                          float *const *dst_y, int *const *matches, unsigned long long *count, unsigned char *const *reason,
                          float *const *residual, float *const *fb_error)
{
    if (!track_ok(n, pyrA, pyrB, fw, fh, levels, src_x, src_y, nA, capA, H_in, status_in, radius, iterations, eps, max_step,
                  min_eig, max_residual, fb_max, dst_x, dst_y, matches, count, reason, residual, fb_error))
        return (int)hipErrorInvalidValue;
    const Params q = params_of(fw, fh, levels, radius, iterations, eps, max_step, min_eig, max_residual, fb_max);
    HostX x;
    x.lane = 0;
    for (int k = 0; k < n; ++k) {
        const int rows = nmp::clip(*nA[k], capA);
        const bool haveH = H_in && (!status_in || status_in[k] == 1) && nmp::finite9(H_in + 9 * (size_t)k);
        count[k] = 0;
        for (int i = 0; i < capA; ++i) {
            const bool exists = i < rows;
            const float sx = exists ? src_x[k][i] : -1.f, sy = exists ? src_y[k][i] : -1.f;
            const RowOut o = track_row(x, q, pyrA[k], pyrB[k], mask_pyr, exists && row_tried(sx, sy), sx, sy,
                                       haveH ? H_in + 9 * (size_t)k : nullptr);
            dst_x[k][i] = o.dst_x; dst_y[k][i] = o.dst_y;
            matches[k][i] = o.reason == 0 ? i : -1;
            count[k] += o.reason == 0 ? 1 : 0;
            if (reason) reason[k][i] = (unsigned char)o.reason;
            if (residual) residual[k][i] = o.residual;
            if (fb_error) fb_error[k][i] = o.fb_error;
        }
    }
    return 0;
}

int nm_klt_sums_host(const float *pyrA, const float *pyrB, const unsigned char *mask_pyr, int fw, int fh, int levels, int level,
                     int radius, double px, double py, double dx, double dy, long long *sums, int *flags)
{
    if (!pyrA || !pyrB || !sums || !flags || !shape_ok(fw, fh, levels) || level < 0 || level >= levels || radius < 1 ||
        radius > MAX_RADIUS)
        return (int)hipErrorInvalidValue;
    int T[MAX_TAPS], gx[MAX_TAPS], gy[MAX_TAPS];
    HostX x;
    x.lane = 0;
    const int w = level_size(fw, level), h = level_size(fh, level);
    const i64 off = level_offset(fw, fh, level);
    const unsigned char *pm = mask_pyr ? mask_pyr + off : nullptr;
    const double s = 1.0 / (double)(1 << level), plx = px * s, ply = py * s;
    Win W;
    bool bad = false;
    const bool okA = window(w, h, (float)plx, (float)ply, radius + 1, W);
    take_template(x, okA, pyrA + off, pm, w, W, radius, T, gx, gy, sums[0], sums[1], sums[2], bad);
    *flags = (!okA || bad) ? 1 : 0;
    bad = false;
    const bool okB = window(w, h, (float)(plx + dx), (float)(ply + dy), radius, W);
    take_mismatch(x, okA && okB, pyrB + off, pm, w, W, radius, T, gx, gy, sums[3], sums[4], sums[5], bad);
    *flags |= (!okB || bad) ? 2 : 0;
    return 0;
}

}  // extern "C"
