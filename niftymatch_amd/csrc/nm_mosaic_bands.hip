// nm_mosaic_bands.hip -- two-band blend of up to NM_MOSAIC_MAX_BATCH placed frames into one canvas, for gfx950
// (include/nm_abi.h, "Two-band mosaic blend", has the written semantics). No reference counterpart. On the caller's
// stream, no allocation, no synchronisation, no host read; no kernel waits for another workgroup; no memset node.
//   warp tiles  ONE launch. Every workgroup stages the n records in LDS, counts each used frame's 64 x 4 tiles and walks
//               the running total grid-stride: a wave takes a tile row, a lane one local pixel, through blend_sample and
//               the gain multiply exactly as the batched blend calls them; one float4 store per pixel.
//   bands       FOUR launches whatever n is:
//     label     a copy of the batched blend's canvas walk (nm_mosaic.hip; 64-bit clipping, ballot of covering frames per wave
//               row, grid-stride over 64 x 4 tiles): the covering frame of largest weight, one byte per pixel.
//     blur x 2  the hot path. Separable, so two launches: a fused 2-D pass would carry a (2R + 1)^2 halo (at R = 32 a
//               64 x 64 tile would load 4x its pixels and need 5 x 128 x 128 x 4 B = 320 KB of LDS), while two 1-D passes
//               cost one extra write and read of the five planes. All frames share one grid: a workgroup walks the
//               running total of the frames' tiles grid-stride. A tile and its halo along the pass direction go into LDS
//               once, plane-major with the pass's lanes along consecutive floats (64 consecutive 4-byte words: one word
//               per bank, no conflict), every pixel read from HBM once per tile, and each output is (R + 1) LDS-fed fmas
//               per plane in the ONE order of nmb::tap_sum.
//                 row pass     128 x 8 outputs, halo 32 columns each side:  5 x 8 x 192 x 4 B = 30 KB of LDS
//                 column pass  32 x 32 outputs, halo 32 rows each side:     5 x 96 x 32 x 4 B = 60 KB of LDS
//               The row pass reads the tile slot and the label plane and forms the five planes on the fly (I_k is never
//               materialised); the column pass reads the row pass's planes.
//     compose   the canvas walk again: the winner's colour plus the M-weighted mean of the low-band differences.
// The arithmetic is nm_mosaic_bands_math.hpp, shared with the host twin below: both agree bit for bit.
#include <climits>
#include <cmath>

#include "nm_mosaic_bands_math.hpp"
#include "nm_mosaic_batch.hpp"
#include "nm_warp_math.hpp"

namespace {

using namespace nmb;
using namespace nmmb;

constexpr int THREADS = CANVAS_THREADS, BLOCKS_PER_CU = 8;

// ---- the walk over the frames' own rectangles: every used frame's tiles on one running total ----
struct Walk {
    int4 box[MAX_FRAMES];                       // tx, ty, nw, nh; nw = 0 when the frame has no tile
    long long end[MAX_FRAMES];                  // tiles of frames 0 .. k
};

template <int TW, int TH>
__device__ __forceinline__ void walk_stage(Walk &W, int n, const nm_mosaic_record *__restrict__ records, long long tile_cap)
{
    const int tid = threadIdx.x;
    if (tid < MAX_FRAMES) {
        int4 b = make_int4(0, 0, 0, 0);
        long long tiles = 0;
        if (tid < n) {
            const nm_mosaic_record *rec = records + tid;
            if (frame_used(rec->placed, rec->nw, rec->nh, tile_cap)) {
                b = make_int4(rec->tx, rec->ty, rec->nw, rec->nh);
                tiles = (long long)((b.z + TW - 1) / TW) * ((b.w + TH - 1) / TH);
            }
        }
        W.box[tid] = b;
        W.end[tid] = tiles;
    }
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        for (int k = 0; k < MAX_FRAMES; ++k) { run += W.end[k]; W.end[k] = run; }
    }
    __syncthreads();
}

// tile t of the running total -> frame k and its tile (tx_, ty_); my_end is W.end[lane]. t is uniform over the wave.
template <int TW>
__device__ __forceinline__ void walk_find(const Walk &W, long long t, long long my_end, int &k, int &tx_, int &ty_)
{
    k = __builtin_popcountll(__ballot(my_end <= t));          // the ends do not decrease: frames wholly before t
    const long long local = t - (k ? W.end[k - 1] : 0);
    const int tiles_x = (W.box[k].z + TW - 1) / TW;
    ty_ = (int)(local / tiles_x);
    tx_ = (int)(local - (long long)ty_ * tiles_x);
}

template <bool GAIN>
__global__ __launch_bounds__(THREADS) void mosaic_warp_tiles_kernel(const FrameArgs a, int n, int fw, int fh, int mask_format,
                                                                    int wts_format,
                                                                    const nm_mosaic_record *__restrict__ records,
                                                                    const float *__restrict__ gains, long long tile_cap,
                                                                    float4 *__restrict__ tiles, int *__restrict__ stats)
{
    __shared__ Walk W;
    __shared__ float s_m[MAX_FRAMES][9];
    __shared__ float s_gain[GAIN ? MAX_FRAMES : 1][3];
    __shared__ const void *s_ptr[3][MAX_FRAMES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < n) {
        for (int q = 0; q < 9; ++q) s_m[tid][q] = records[tid].m[q];
        s_ptr[0][tid] = a.frames[tid];
        s_ptr[1][tid] = a.masks[tid];
        s_ptr[2][tid] = a.wts[tid];
        if (GAIN)
            for (int c = 0; c < 3; ++c) s_gain[tid][c] = gains[3 * tid + c];
    }
    walk_stage<CANVAS_TILE_W, CANVAS_TILE_H>(W, n, records, tile_cap);
    if (blockIdx.x == 0 && tid < 64) {
        const int used = __builtin_popcountll(__ballot(tid < n && W.box[tid].z > 0));
        if (tid == 0) { stats[0] = used; stats[1] = n - used; }
    }
    const long long total = W.end[MAX_FRAMES - 1], my_end = W.end[lane];
    const nmw::Tex none{nullptr, fw, fh, 0};
    for (long long t = blockIdx.x; t < total; t += gridDim.x) {
        int k, tx_, ty_;
        walk_find<CANVAS_TILE_W>(W, t, my_end, k, tx_, ty_);
        const int4 b = W.box[k];
        const int x = tx_ * CANVAS_TILE_W + lane, y = ty_ * CANVAS_TILE_H + wave;
        if (x >= b.z || y >= b.w) continue;
        nmw::Tex frame = none, mask = none, wts = none;
        frame.data = s_ptr[0][k]; frame.fmt = NM_TEX_U8X4N;
        mask.data = s_ptr[1][k]; mask.fmt = mask_format;
        wts.data = s_ptr[2][k]; wts.fmt = wts_format;
        float rgb[4], w = 0.f;
        float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
        if (nmw::blend_sample(s_m[k], frame, mask, wts, x, y, rgb, w) && w > 0.f) {
            if (GAIN) {
                rgb[0] = rgb[0] * s_gain[k][0]; rgb[1] = rgb[1] * s_gain[k][1]; rgb[2] = rgb[2] * s_gain[k][2];
            }
            out = make_float4(rgb[0], rgb[1], rgb[2], w);
        }
        tiles[(size_t)k * (size_t)tile_cap + (size_t)y * b.z + x] = out;     // y * nw + x < nw * nh <= tile_cap
    }
}

// ---- the canvas walk of the batched blend: label pass and compose pass ----
template <bool COMPOSE>
__global__ __launch_bounds__(THREADS) void mosaic_bands_canvas_kernel(int n, const nm_mosaic_record *__restrict__ records,
                                                                      long long tile_cap, const float4 *__restrict__ tiles,
                                                                      int cw, int ch, unsigned char *__restrict__ label,
                                                                      const float4 *__restrict__ lv,
                                                                      const float *__restrict__ mk,
                                                                      uchar4 *__restrict__ canvas,
                                                                      float *__restrict__ canvas_wts)
{
    __shared__ int4 s_box[MAX_FRAMES];           // tx, ty, nw, nh
    __shared__ int4 s_rect[MAX_FRAMES];          // clipped (x0, y0, x1, y1); (0, 0, 0, 0) when empty
    __shared__ int4 s_union;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 64) {
        int4 r = make_int4(0, 0, 0, 0), b = r;
        if (tid < n) {
            const nm_mosaic_record *rec = records + tid;
            const int tx = rec->tx, ty = rec->ty, nw = rec->nw, nh = rec->nh;
            if (frame_used(rec->placed, nw, nh, tile_cap)) {
                b = make_int4(tx, ty, nw, nh);
                const long long x0 = tx > 0 ? tx : 0, y0 = ty > 0 ? ty : 0;
                const long long x1 = (long long)tx + nw < cw ? (long long)tx + nw : cw;
                const long long y1 = (long long)ty + nh < ch ? (long long)ty + nh : ch;
                if (x1 > x0 && y1 > y0) r = make_int4((int)x0, (int)y0, (int)x1, (int)y1);
            }
        }
        s_box[tid] = b;
        s_rect[tid] = r;
        const bool empty = r.z == 0;
        int ux0 = empty ? INT_MAX : r.x, uy0 = empty ? INT_MAX : r.y, ux1 = empty ? 0 : r.z, uy1 = empty ? 0 : r.w;
        ux0 = nmw::wave_min(ux0); uy0 = nmw::wave_min(uy0); ux1 = nmw::wave_max(ux1); uy1 = nmw::wave_max(uy1);
        if (tid == 0) s_union = make_int4(ux0, uy0, ux1, uy1);
    }
    __syncthreads();
    const int4 U = s_union;
    if (U.z <= U.x) return;                            // no frame touches the canvas (uniform)
    const int4 mine = s_rect[lane];
    const int tiles_x = (U.z - U.x + CANVAS_TILE_W - 1) / CANVAS_TILE_W;
    const int ntiles = tiles_x * ((U.w - U.y + CANVAS_TILE_H - 1) / CANVAS_TILE_H);
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int ty_ = t / tiles_x, tx_ = t - ty_ * tiles_x;
        const int row = U.y + ty_ * CANVAS_TILE_H + wave, xs = U.x + tx_ * CANVAS_TILE_W;
        const int px = xs + lane;
        unsigned long long fm = __ballot(mine.y <= row && row < mine.w && mine.x < xs + CANVAS_TILE_W && xs < mine.z);
        if (!fm) continue;                             // wave-uniform
        const size_t idx = (size_t)row * cw + px;      // used only where a rectangle holds (px, row): inside the canvas
        bool covered = false;
        int lab = NO_LABEL;
        float best = 0.f;
        Compose cmp;
        float4 Cs = make_float4(0.f, 0.f, 0.f, 0.f);
        while (fm) {
            const int k = __builtin_ctzll(fm);
            fm &= fm - 1ull;
            const int4 r = s_rect[k];
            if (px < r.x || px >= r.z) continue;
            const int4 b = s_box[k];
            const size_t at = (size_t)k * (size_t)tile_cap + (size_t)(row - b.y) * b.z + (px - b.x);
            if (!COMPOSE) {
                covered = true;
                label_step(k, tiles[at].w, lab, best);
            } else {
                if (!covered) {                        // the first covering frame: fetch the winner once
                    covered = true;
                    lab = label[idx];
                    if (lab != NO_LABEL) {
                        const int4 bs = s_box[lab];
                        const size_t as = (size_t)lab * (size_t)tile_cap + (size_t)(row - bs.y) * bs.z + (px - bs.x);
                        Cs = tiles[as];
                        cmp.begin(lv[as]);
                    }
                }
                if (lab != NO_LABEL && tiles[at].w > 0.f) cmp.add(lv[at], mk[at]);
            }
        }
        if (!covered) continue;
        if (!COMPOSE) {
            label[idx] = (unsigned char)lab;
        } else if (lab != NO_LABEL) {
            canvas[idx] = cmp.finish(Cs);
            if (canvas_wts) canvas_wts[idx] = Cs.w;
        }
    }
}

// ---- the blur: one 1-D pass over every used frame's rectangle ----
template <bool VERT>
struct BlurShape {
    static constexpr int TW = VERT ? 32 : 128, TH = VERT ? 32 : 8;
    static constexpr int HX = VERT ? 0 : MAX_R, HY = VERT ? MAX_R : 0;
    static constexpr int COLS = TW + 2 * HX, ROWS = TH + 2 * HY;
};

template <bool VERT>
__global__ __launch_bounds__(THREADS) void mosaic_bands_blur_kernel(const Taps taps, int R, int n,
                                                                    const nm_mosaic_record *__restrict__ records,
                                                                    long long tile_cap, int cw, int ch,
                                                                    const float4 *__restrict__ tiles,
                                                                    const unsigned char *__restrict__ label,
                                                                    const float4 *__restrict__ src_lv,
                                                                    const float *__restrict__ src_m,
                                                                    float4 *__restrict__ dst_lv, float *__restrict__ dst_m)
{
    using S = BlurShape<VERT>;
    __shared__ float s[PLANES][S::ROWS][S::COLS];
    __shared__ Walk W;
    __shared__ float s_g[MAX_R + 1];                  // indexed at run time: out of the kernel arguments
    static_assert(sizeof(float) * PLANES * S::ROWS * S::COLS + sizeof(Walk) + sizeof(float) * (MAX_R + 1) <= 65536, "LDS");
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid <= MAX_R) s_g[tid] = taps.g[tid];
    walk_stage<S::TW, S::TH>(W, n, records, tile_cap);
    const long long total = W.end[MAX_FRAMES - 1], my_end = W.end[lane];
    const int rx = VERT ? 0 : R, ry = VERT ? R : 0;
    const int wcols = S::TW + 2 * rx, count = wcols * (S::TH + 2 * ry);
    for (long long t = blockIdx.x; t < total; t += gridDim.x) {
        int k, tx_, ty_;
        walk_find<S::TW>(W, t, my_end, k, tx_, ty_);
        const int4 b = W.box[k];
        const int x0 = tx_ * S::TW, y0 = ty_ * S::TH;
        const size_t slot = (size_t)k * (size_t)tile_cap;
        for (int i = tid; i < count; i += THREADS) {
            const int r = i / wcols, c = i - r * wcols;
            const int lx = x0 - rx + c, ly = y0 - ry + r;
            float p[PLANES] = {0.f, 0.f, 0.f, 0.f, 0.f};
            if (lx >= 0 && lx < b.z && ly >= 0 && ly < b.w) {
                const size_t at = slot + (size_t)ly * b.z + lx;
                if (!VERT) {
                    const long long gx = (long long)b.x + lx, gy = (long long)b.y + ly;
                    const bool in = gx >= 0 && gx < cw && gy >= 0 && gy < ch;
                    planes_of(tiles[at], in && label[(size_t)gy * cw + (size_t)gx] == k, p);
                } else {
                    const float4 v = src_lv[at];
                    p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w; p[4] = src_m[at];
                }
            }
#pragma unroll
            for (int q = 0; q < PLANES; ++q) s[q][r][c] = p[q];
        }
        __syncthreads();
        for (int o = tid; o < S::TW * S::TH; o += THREADS) {
            const int r = o / S::TW, c = o - r * S::TW;
            const int lx = x0 + c, ly = y0 + r;
            if (lx >= b.z || ly >= b.w) continue;
            float out[PLANES];
#pragma unroll
            for (int q = 0; q < PLANES; ++q)
                out[q] = tap_sum(s_g, R, [&](int i) { return VERT ? s[q][r + ry + i][c] : s[q][r][c + rx + i]; });
            const size_t at = slot + (size_t)ly * b.z + lx;
            dst_lv[at] = make_float4(out[0], out[1], out[2], out[3]);
            dst_m[at] = out[4];
        }
        __syncthreads();
    }
}

// ---- refusals ----
bool tile_cap_ok(long long tile_cap) { return tile_cap >= 1 && tile_cap <= MAX_TILE_CAP; }

bool bands_args_ok(int n, const void *tiles, long long tile_cap, const void *records, const void *canvas, int cw, int ch,
                   int R, double sigma, const void *workspace)
{
    return n >= 1 && n <= MAX_FRAMES && tile_cap_ok(tile_cap) && nm_size_ok(cw) && nm_size_ok(ch) && R >= 0 && R <= MAX_R &&
           (R == 0 || (std::isfinite(sigma) && sigma > 0.0)) && tiles && records && canvas && workspace && ((reinterpret_cast<size_t>(workspace) | reinterpret_cast<size_t>(tiles)) & 15) == 0;
}

// the grid of the kernels that stride over the frames' own tiles, whose number only the device knows: the whole fill
int fill_grid() { return nm_fill_grid(LLONG_MAX, BLOCKS_PER_CU); }

// ---- the host twin's pieces: the same functions, walked serially ----
void host_blur(const Taps &T, int R, bool vert, const int4 &b, int k, int cw, int ch, const float4 *tile,
               const unsigned char *label, const float4 *src_lv, const float *src_m, float4 *dst_lv, float *dst_m)
{
    for (int y = 0; y < b.w; ++y)
        for (int x = 0; x < b.z; ++x) {
            float out[PLANES];
            for (int q = 0; q < PLANES; ++q)
                out[q] = tap_sum(T.g, R, [&](int i) {
                    const int lx = vert ? x : x + i, ly = vert ? y + i : y;
                    if (lx < 0 || lx >= b.z || ly < 0 || ly >= b.w) return 0.f;
                    const size_t at = (size_t)ly * b.z + lx;
                    if (vert) {
                        const float4 v = src_lv[at];
                        return q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.z : q == 3 ? v.w : src_m[at];
                    }
                    const long long gx = (long long)b.x + lx, gy = (long long)b.y + ly;
                    const bool in = gx >= 0 && gx < cw && gy >= 0 && gy < ch;
                    float p[PLANES];
                    planes_of(tile[at], in && label[(size_t)gy * cw + (size_t)gx] == k, p);
                    return p[q];
                });
            const size_t at = (size_t)y * b.z + x;
            dst_lv[at] = make_float4(out[0], out[1], out[2], out[3]);
            dst_m[at] = out[4];
        }
}

}  // namespace

extern "C" {

size_t nm_mosaic_bands_workspace_bytes(int n, long long tile_cap, int cw, int ch)
{
    if (n < 1 || n > MAX_FRAMES || !tile_cap_ok(tile_cap) || !nm_size_ok(cw) || !nm_size_ok(ch)) return 0;
    return workspace_bytes(n, tile_cap, cw, ch);
}

int nm_mosaic_bands_taps(int R, double sigma, float *g)
{
    if (R < 0 || R > MAX_R || !g || (R > 0 && !(std::isfinite(sigma) && sigma > 0.0))) return (int)hipErrorInvalidValue;
    Taps T;
    taps_of(R, sigma, T);
    for (int i = 0; i <= R; ++i) g[i] = T.g[i];
    return 0;
}

int nm_mosaic_warp_tiles(int n, const unsigned char *const *frames, int fw, int fh, const void *const *masks,
                         int mask_format, const void *const *wts, int wts_format, const nm_mosaic_record *records,
                         const float *gains, float *tiles, long long tile_cap, int *stats, void *stream)
{
    if (n < 1 || n > MAX_FRAMES || !nm_size_ok(fw) || !nm_size_ok(fh) || !scalar_fmt(mask_format) || !scalar_fmt(wts_format) ||
        !tile_cap_ok(tile_cap))
        return (int)hipErrorInvalidValue;
    if (!records || !tiles || !stats || (reinterpret_cast<size_t>(tiles) & 15)) return (int)hipErrorInvalidValue;
    FrameArgs a;
    if (!fill_frame_args(a, n, frames, masks, wts)) return (int)hipErrorInvalidValue;
    const auto kernel = gains ? mosaic_warp_tiles_kernel<true> : mosaic_warp_tiles_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(fill_grid()), dim3(THREADS), 0, nm_stream(stream), a, n, fw, fh, mask_format, wts_format,
                       records, gains, tile_cap, reinterpret_cast<float4 *>(tiles), stats);
    NM_LAUNCH_CHECK();
    return 0;
}

int nm_mosaic_bands_dev(int n, const float *tiles, long long tile_cap, const nm_mosaic_record *records,
                        unsigned char *canvas, int cw, int ch, float *canvas_wts, int R, double sigma, void *workspace,
                        void *stream)
{
    if (!bands_args_ok(n, tiles, tile_cap, records, canvas, cw, ch, R, sigma, workspace))
        return (int)hipErrorInvalidValue;
    Taps T;
    taps_of(R, sigma, T);
    const Workspace W = carve(workspace, n, tile_cap, cw, ch);
    const float4 *t4 = reinterpret_cast<const float4 *>(tiles);
    uchar4 *cv = reinterpret_cast<uchar4 *>(canvas);
    const int fill = fill_grid();
    const int cgrid = nm_fill_grid((long long)nm_divup(cw, CANVAS_TILE_W) * nm_divup(ch, CANVAS_TILE_H), BLOCKS_PER_CU);
    hipStream_t st = nm_stream(stream);
    hipLaunchKernelGGL(mosaic_bands_canvas_kernel<false>, dim3(cgrid), dim3(THREADS), 0, st, n, records, tile_cap, t4, cw, ch,
                       W.label, (const float4 *)nullptr, (const float *)nullptr, (uchar4 *)nullptr, (float *)nullptr);
    NM_LAUNCH_CHECK();
    hipLaunchKernelGGL(mosaic_bands_blur_kernel<false>, dim3(fill), dim3(THREADS), 0, st, T, R, n, records, tile_cap, cw, ch,
                       t4, W.label, (const float4 *)nullptr, (const float *)nullptr, W.lv[0], W.m[0]);
    NM_LAUNCH_CHECK();
    hipLaunchKernelGGL(mosaic_bands_blur_kernel<true>, dim3(fill), dim3(THREADS), 0, st, T, R, n, records, tile_cap, cw, ch,
                       t4, W.label, W.lv[0], W.m[0], W.lv[1], W.m[1]);
    NM_LAUNCH_CHECK();
    hipLaunchKernelGGL(mosaic_bands_canvas_kernel<true>, dim3(cgrid), dim3(THREADS), 0, st, n, records, tile_cap, t4, cw, ch,
                       W.label, W.lv[1], W.m[1], cv, canvas_wts);
    NM_LAUNCH_CHECK();
    return 0;
}

int nm_mosaic_bands_host(int n, const float *tiles, long long tile_cap, const nm_mosaic_record *records,
                         unsigned char *canvas, int cw, int ch, float *canvas_wts, int R, double sigma, void *workspace)
{
    if (!bands_args_ok(n, tiles, tile_cap, records, canvas, cw, ch, R, sigma, workspace))
        return (int)hipErrorInvalidValue;
    Taps T;
    taps_of(R, sigma, T);
    const Workspace W = carve(workspace, n, tile_cap, cw, ch);
    const float4 *t4 = reinterpret_cast<const float4 *>(tiles);
    uchar4 *cv = reinterpret_cast<uchar4 *>(canvas);
    int4 box[MAX_FRAMES], rect[MAX_FRAMES];
    for (int k = 0; k < n; ++k) {
        const nm_mosaic_record &rec = records[k];
        box[k] = rect[k] = make_int4(0, 0, 0, 0);
        if (!frame_used(rec.placed, rec.nw, rec.nh, tile_cap)) continue;
        box[k] = make_int4(rec.tx, rec.ty, rec.nw, rec.nh);
        rect[k] = clip_rect(rec.tx, rec.ty, rec.nw, rec.nh, cw, ch);
    }
    const auto slot_at = [&](int k, int px, int row) {
        return (size_t)k * (size_t)tile_cap + (size_t)(row - box[k].y) * box[k].z + (px - box[k].x);
    };
    const auto covers = [&](int k, int px, int row) {
        return px >= rect[k].x && px < rect[k].z && row >= rect[k].y && row < rect[k].w;
    };
    for (int k = 0; k < n; ++k)                                    // label, frame by frame in index order
        for (int row = rect[k].y; row < rect[k].w; ++row)
            for (int px = rect[k].x; px < rect[k].z; ++px) {
                bool first = true;
                for (int j = 0; j < k && first; ++j) first = !covers(j, px, row);
                if (!first) continue;                              // the lowest covering frame labels the pixel
                int lab = NO_LABEL;
                float best = 0.f;
                for (int j = k; j < n; ++j)
                    if (covers(j, px, row)) label_step(j, t4[slot_at(j, px, row)].w, lab, best);
                W.label[(size_t)row * cw + px] = (unsigned char)lab;
            }
    for (int k = 0; k < n; ++k) {
        if (box[k].z == 0) continue;
        const size_t slot = (size_t)k * (size_t)tile_cap;
        host_blur(T, R, false, box[k], k, cw, ch, t4 + slot, W.label, nullptr, nullptr, W.lv[0] + slot, W.m[0] + slot);
        host_blur(T, R, true, box[k], k, cw, ch, t4 + slot, W.label, W.lv[0] + slot, W.m[0] + slot, W.lv[1] + slot,
                  W.m[1] + slot);
    }
    for (int k = 0; k < n; ++k)                                    // compose, each covered pixel once
        for (int row = rect[k].y; row < rect[k].w; ++row)
            for (int px = rect[k].x; px < rect[k].z; ++px) {
                bool first = true;
                for (int j = 0; j < k && first; ++j) first = !covers(j, px, row);
                const size_t idx = (size_t)row * cw + px;
                const int lab = W.label[idx];
                if (!first || lab == NO_LABEL) continue;
                const float4 Cs = t4[slot_at(lab, px, row)];
                Compose cmp;
                cmp.begin(W.lv[1][slot_at(lab, px, row)]);
                for (int j = k; j < n; ++j)
                    if (covers(j, px, row) && t4[slot_at(j, px, row)].w > 0.f)
                        cmp.add(W.lv[1][slot_at(j, px, row)], W.m[1][slot_at(j, px, row)]);
                cv[idx] = cmp.finish(Cs);
                if (canvas_wts) canvas_wts[idx] = Cs.w;
            }
    return 0;
}

}  // extern "C"
