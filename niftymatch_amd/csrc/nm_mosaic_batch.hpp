// nm_mosaic_batch.hpp -- what the mosaic's blend kernels (nm_mosaic.hip, nm_mosaic_bands.hip, nm_mosaic_median.hip) take the
// same way: n <= MAX_FRAMES frames, canvas tiles of CANVAS_TILE_W x CANVAS_TILE_H pixels (a canvas row per wave), and the
// sampler's three pointer tables as kernel arguments, on nm_pair_batch.hpp's helpers, and clip_rect, a frame's rectangle on
// the canvas. The canvas walk (staging, tile step, ballot) is NOT here: transform_blend_batch_kernel,
// mosaic_bands_canvas_kernel and mosaic_median_kernel (two waves: 64 x 2 tiles) each write it out. clip_rect serves
// mosaic_median_kernel and the host twins of bands and median; the kernels of nm_mosaic.hip and nm_mosaic_bands.hip keep the
// 64-bit clipping written out, because a shared clip_rect or walk changed their register counts and cost microseconds when
// it was measured (CHANGELOG.md, "Mosaic and link stages: one size limit ..."). Change one, change the others.
#pragma once
#include "nm_pair_batch.hpp"
#include "../../include/nm_abi.h"

namespace nmmb {
constexpr int MAX_FRAMES = NM_MOSAIC_MAX_BATCH;
constexpr int CANVAS_THREADS = 256;                             // 4 waves: a tile is 64 x 4 canvas pixels, one row per wave
constexpr int CANVAS_TILE_W = 64, CANVAS_TILE_H = CANVAS_THREADS / 64;
static_assert(sizeof(nm_mosaic_record) == 64, "nm_mosaic_record must stay 64 bytes");
static_assert(MAX_FRAMES == 64 && MAX_FRAMES == nmp::MAX_BATCH, "one lane per frame in a wave of 64");
struct FrameArgs {                                       // 3 x 64 pointers: 1.5 KB of the 4 KB of kernel arguments
    const void *frames[MAX_FRAMES];
    const void *masks[MAX_FRAMES];
    const void *wts[MAX_FRAMES];
};
static_assert(sizeof(FrameArgs) + 128 < 4096, "kernel arguments exceed 4 KB");
inline bool scalar_fmt(int f) { return f == NM_TEX_U8N || f == NM_TEX_F32; }   // the formats of masks and weights

// (x0, y0, x1, y1) of a used frame's rectangle on the canvas, clipped in 64-bit; (0, 0, 0, 0) when empty
__host__ __device__ __forceinline__ int4 clip_rect(int tx, int ty, int nw, int nh, int cw, int ch)
{
    const long long x0 = tx > 0 ? tx : 0, y0 = ty > 0 ? ty : 0;
    const long long x1 = (long long)tx + nw < cw ? (long long)tx + nw : cw;
    const long long y1 = (long long)ty + nh < ch ? (long long)ty + nh : ch;
    return x1 > x0 && y1 > y0 ? make_int4((int)x0, (int)y0, (int)x1, (int)y1) : make_int4(0, 0, 0, 0);
}

// false: a table or one of its n slots is null (reads host memory only; call it after the range check of n)
inline bool fill_frame_args(FrameArgs &a, int n, const unsigned char *const *frames, const void *const *masks,
                            const void *const *wts)
{
    if (!nmp::tables_ok(n, {frames, masks, wts}, {}, {})) return false;
    nmp::fill_slots(a.frames, frames, 0, n); nmp::fill_slots(a.masks, masks, 0, n); nmp::fill_slots(a.wts, wts, 0, n);
    return true;
}
}  // namespace nmmb
