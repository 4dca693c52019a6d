// nm_mosaic.hip -- mosaic plan (pairwise homographies -> per-frame placement records) and the batched blend of up to
// NM_MOSAIC_MAX_BATCH frames into one canvas, for gfx950. No reference counterpart: the reference's client chains the
// homographies and places each frame on the host, then calls transform_blend (kernels/resample.cu:7-66) per frame.
//   plan  (1 launch, 1 workgroup): lane 0 chains the n-1 links serially (63 3x3 products at most), then one lane per
//         frame computes its footprint, record and chain row; the extent is a wave min / max. The same __host__
//         __device__ functions build the host twin, so the two agree bit for bit.
//   place (1 launch, 1 workgroup): the plan's placement half on a given chain (e.g. the adjusted one of
//         nm_mosaic_adjust.hip): one lane per frame through the same mp_frame, the same extent.
//   blend (1 launch, fixed grid; this walk is repeated in mosaic_bands_canvas_kernel, see nm_mosaic_batch.hpp): every
//         workgroup stages the n records and frame pointers in LDS and clips the rectangles; a grid-stride loop walks
//         the 64 x 4 tiles of the rectangles' bounding box, one canvas row of 64 pixels per wave. A wave ballots the
//         frames whose rectangle meets its row (a wave-uniform 64-bit mask) and walks the set bits in index order; each
//         lane runs transform_blend's per-pixel step (nm_warp_math.hpp) for every covering frame with the canvas pixel
//         and weight in registers: one load, at most one store per pixel.
//         nm_transform_blend_batch_gain is the same kernel body with a per-frame, per-channel gain on the frame's colour
//         (the exposure compensation of nm_mosaic_exposure.hip), a compile-time switch.
#include <climits>
#include <cmath>

#include "nm_mosaic_batch.hpp"
#include "nm_warp_math.hpp"

namespace {

using namespace nmw;
using namespace nmmb;

constexpr int MP_OFFSET_LIMIT = 1 << 20;        // |ox|, |oy|
constexpr int MB_BLOCKS_PER_CU = 8;

__host__ __device__ __forceinline__ bool mp_finite(float v) { return __builtin_isfinite(v); }

// M_out = (H M) / (H M)[8]; false when the link breaks (non-finite H, or a zero / non-finite normaliser)
__host__ __device__ __forceinline__ bool mp_link(const float *h, const float *M, float *out)
{
    bool ok = true;
    for (int q = 0; q < 9; ++q) ok = ok && mp_finite(h[q]);
    if (!ok) return false;
    float p[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            p[3 * r + c] = fmaf_(h[3 * r + 2], M[6 + c], fmaf_(h[3 * r + 1], M[3 + c], h[3 * r] * M[c]));
    const float s = p[8];
    if (s == 0.f || !mp_finite(s)) return false;
    for (int q = 0; q < 9; ++q) out[q] = p[q] / s;
    return true;
}

// The chain M_0 .. M_{n-1} and whether frame k is still chained (ok[k]); rows of broken frames are zero.
__host__ __device__ inline void mp_chain(int n, const float *H, const int *status, const float *M_first, float (*M)[9],
                                         int *ok)
{
    for (int q = 0; q < 9; ++q) M[0][q] = M_first ? M_first[q] : ((q & 3) == 0 ? 1.f : 0.f);
    ok[0] = 1;
    for (int k = 1; k < n; ++k) {
        bool v = ok[k - 1] && (!status || status[k - 1] == 1) && mp_link(H + 9 * (k - 1), M[k - 1], M[k]);
        ok[k] = v ? 1 : 0;
        if (!v)
            for (int q = 0; q < 9; ++q) M[k][q] = 0.f;
    }
}

__host__ __device__ __forceinline__ float mp_clamp(float v, float hi) { return v < 0.f ? 0.f : (v > hi ? hi : v); }

// Footprint and local map of a chained frame. false: a corner is behind the camera or not finite (frame unplaced).
__host__ __device__ inline bool mp_place(const float *M, int fw, int fh, int cw, int ch, int ox, int oy,
                                         nm_mosaic_record &rec, float box[4])
{
    float W[9];
    invert3x3(M, W);
    const float cx[4] = {-1.f, (float)fw, -1.f, (float)fw};
    const float cy[4] = {-1.f, -1.f, (float)fh, (float)fh};
    float x0 = 0.f, y0 = 0.f, x1 = 0.f, y1 = 0.f;
    for (int k = 0; k < 4; ++k) {
        const float s = project_den(W, cx[k], cy[k]);
        float xp, yp;
        project(W, cx[k], cy[k], xp, yp);
        if (!(s > 0.f) || !mp_finite(xp) || !mp_finite(yp)) return false;
        x0 = (k == 0 || xp < x0) ? xp : x0;
        y0 = (k == 0 || yp < y0) ? yp : y0;
        x1 = (k == 0 || xp > x1) ? xp : x1;
        y1 = (k == 0 || yp > y1) ? yp : y1;
    }
    box[0] = __builtin_floorf(x0) - 1.f;
    box[1] = __builtin_floorf(y0) - 1.f;
    box[2] = __builtin_ceilf(x1) + 1.f;
    box[3] = __builtin_ceilf(y1) + 1.f;
    const int X0 = (int)mp_clamp(box[0] + (float)ox, (float)cw), X1 = (int)mp_clamp(box[2] + (float)ox, (float)cw);
    const int Y0 = (int)mp_clamp(box[1] + (float)oy, (float)ch), Y1 = (int)mp_clamp(box[3] + (float)oy, (float)ch);
    rec.tx = X0;
    rec.ty = Y0;
    rec.nw = X1 > X0 ? X1 - X0 : 0;
    rec.nh = Y1 > Y0 ? Y1 - Y0 : 0;
    const float dx = (float)(X0 - ox), dy = (float)(Y0 - oy);
    for (int r = 0; r < 3; ++r) {
        rec.m[3 * r] = M[3 * r];
        rec.m[3 * r + 1] = M[3 * r + 1];
        rec.m[3 * r + 2] = fmaf_(M[3 * r], dx, fmaf_(M[3 * r + 1], dy, M[3 * r + 2]));
    }
    rec.placed = 1;
    rec.reserved[0] = rec.reserved[1] = 0;
    return true;
}

__host__ __device__ __forceinline__ void mp_zero(nm_mosaic_record &rec)
{
    for (int q = 0; q < 9; ++q) rec.m[q] = 0.f;
    rec.tx = rec.ty = rec.nw = rec.nh = rec.placed = 0;
    rec.reserved[0] = rec.reserved[1] = 0;
}

// One frame's record, chain row and box; returns whether it is placed
__host__ __device__ inline bool mp_frame(const float *M, int chained, int fw, int fh, int cw, int ch, int ox, int oy,
                                         nm_mosaic_record &rec, float box[4])
{
    if (chained && mp_place(M, fw, fh, cw, ch, ox, oy, rec, box)) return true;
    mp_zero(rec);
    return false;
}

// Whether a frame of a given chain (nm_mosaic_place_f32) is to be placed: status 1 and a finite row
__host__ __device__ __forceinline__ int mp_given(const float *M, int status)
{
    bool ok = status == 1;
    for (int q = 0; q < 9; ++q) ok = ok && mp_finite(M[q]);
    return ok ? 1 : 0;
}

inline bool mp_sizes_ok(int n, int fw, int fh, int cw, int ch, int ox, int oy, const void *records)
{
    return n >= 1 && n <= NM_MOSAIC_MAX_BATCH && nm_size_ok(fw) && nm_size_ok(fh) && nm_size_ok(cw) && nm_size_ok(ch) &&
           ox > -MP_OFFSET_LIMIT && ox < MP_OFFSET_LIMIT && oy > -MP_OFFSET_LIMIT && oy < MP_OFFSET_LIMIT && records;
}

// A frame's box into the extent of the frames placed before it, in index order (the host twins)
inline void mp_extent_add(bool &any, float e[4], const float box[4])
{
    for (int q = 0; q < 2; ++q) e[q] = (!any || box[q] < e[q]) ? box[q] : e[q];
    for (int q = 2; q < 4; ++q) e[q] = (!any || box[q] > e[q]) ? box[q] : e[q];
    any = true;
}

// The extent of a wave's placed frames, lane k with frame k's box. Every box value is an integer-valued finite float (no
// -0), so min / max are order-independent: equal to mp_extent_add's in-order loop.
__device__ __forceinline__ void mp_extent_store(bool placed, const float box[4], int k, float *__restrict__ extent)
{
    float e[4] = {placed ? box[0] : INFINITY, placed ? box[1] : INFINITY, placed ? box[2] : -INFINITY,
                  placed ? box[3] : -INFINITY};
    e[0] = nmw::wave_min(e[0]); e[1] = nmw::wave_min(e[1]); e[2] = nmw::wave_max(e[2]); e[3] = nmw::wave_max(e[3]);
    const bool any = __ballot(placed) != 0ull;
    if (k < 4) extent[k] = any ? e[k] : 0.f;
}

__global__ __launch_bounds__(64) void mosaic_plan_kernel(int n, const float *__restrict__ H, const int *__restrict__ status,
                                                         int fw, int fh, int cw, int ch, int ox, int oy,
                                                         const float *__restrict__ M_first,
                                                         nm_mosaic_record *__restrict__ records,
                                                         float *__restrict__ chain, float *__restrict__ extent)
{
    __shared__ float s_M[NM_MOSAIC_MAX_BATCH][9];
    __shared__ int s_ok[NM_MOSAIC_MAX_BATCH];
    __shared__ float s_H[(NM_MOSAIC_MAX_BATCH - 1) * 9 + 9];   // the links, then M_first
    __shared__ int s_status[NM_MOSAIC_MAX_BATCH];
    const int k = threadIdx.x;
    // every lane stages the inputs first: the serial chain then reads LDS, not one dependent global load per link
    for (int q = k; q < (n - 1) * 9; q += 64) s_H[q] = H[q];
    if (k < n - 1 && status) s_status[k] = status[k];
    if (k < 9 && M_first) s_H[(NM_MOSAIC_MAX_BATCH - 1) * 9 + k] = M_first[k];
    __syncthreads();
    if (k == 0)
        mp_chain(n, s_H, status ? s_status : nullptr, M_first ? s_H + (NM_MOSAIC_MAX_BATCH - 1) * 9 : nullptr, s_M, s_ok);
    __syncthreads();
    bool placed = false;
    float box[4] = {0.f, 0.f, 0.f, 0.f};
    if (k < n) {
        nm_mosaic_record rec;
        placed = mp_frame(s_M[k], s_ok[k], fw, fh, cw, ch, ox, oy, rec, box);
        records[k] = rec;
        if (chain)
            for (int q = 0; q < 9; ++q) chain[9 * k + q] = s_M[k][q];
    }
    if (!extent) return;                                  // uniform
    mp_extent_store(placed, box, k, extent);
}

// The placement half of the plan on a given chain: one lane per frame, the extent as in the plan
__global__ __launch_bounds__(64) void mosaic_place_kernel(int n, const float *__restrict__ chain,
                                                          const int *__restrict__ frame_status, int fw, int fh, int cw,
                                                          int ch, int ox, int oy, nm_mosaic_record *__restrict__ records,
                                                          float *__restrict__ extent)
{
    const int k = threadIdx.x;
    bool placed = false;
    float box[4] = {0.f, 0.f, 0.f, 0.f};
    if (k < n) {
        float M[9];
        for (int q = 0; q < 9; ++q) M[q] = chain[9 * k + q];
        nm_mosaic_record rec;
        placed = mp_frame(M, mp_given(M, frame_status ? frame_status[k] : 1), fw, fh, cw, ch, ox, oy, rec, box);
        records[k] = rec;
    }
    if (!extent) return;                                  // uniform
    mp_extent_store(placed, box, k, extent);
}

// GAIN: frame k's colour is multiplied by gains[3 k + c] between blend_sample and blend_combine (the gains staged in LDS
// beside the records); without it the body is the ungained blend's, operation for operation.
template <bool GAIN>
__global__ __launch_bounds__(CANVAS_THREADS) void transform_blend_batch_kernel(const FrameArgs a, int n, uchar4 *__restrict__ canvas,
                                                                        int cw, int ch, float *__restrict__ canvas_wts,
                                                                        int fw, int fh, int mask_format, int wts_format,
                                                                        const nm_mosaic_record *__restrict__ records,
                                                                        const float *__restrict__ gains)
{
    __shared__ float s_gain[GAIN ? NM_MOSAIC_MAX_BATCH : 1][3];
    __shared__ float s_m[NM_MOSAIC_MAX_BATCH][9];
    __shared__ int2 s_t[NM_MOSAIC_MAX_BATCH];          // the records' tx, ty
    __shared__ int4 s_rect[NM_MOSAIC_MAX_BATCH];       // clipped (x0, y0, x1, y1); (0, 0, 0, 0) when empty
    __shared__ const void *s_ptr[3][NM_MOSAIC_MAX_BATCH];
    __shared__ int4 s_union;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 64) {
        int4 r = make_int4(0, 0, 0, 0);
        if (tid < n) {
            const nm_mosaic_record *rec = records + tid;
            for (int q = 0; q < 9; ++q) s_m[tid][q] = rec->m[q];
            const int tx = rec->tx, ty = rec->ty, nw = rec->nw, nh = rec->nh;
            s_t[tid] = make_int2(tx, ty);
            const long long x0 = tx > 0 ? tx : 0, y0 = ty > 0 ? ty : 0;
            const long long x1 = (long long)tx + nw < cw ? (long long)tx + nw : cw;
            const long long y1 = (long long)ty + nh < ch ? (long long)ty + nh : ch;
            if (nw > 0 && nh > 0 && x1 > x0 && y1 > y0) r = make_int4((int)x0, (int)y0, (int)x1, (int)y1);
            s_ptr[0][tid] = a.frames[tid];
            s_ptr[1][tid] = a.masks[tid];
            s_ptr[2][tid] = a.wts[tid];
            if (GAIN)
                for (int c = 0; c < 3; ++c) s_gain[tid][c] = gains[3 * tid + c];
        }
        s_rect[tid] = r;
        const bool empty = r.z == 0;                   // x1 > x0 >= 0 for every non-empty rectangle
        int ux0 = empty ? INT_MAX : r.x, uy0 = empty ? INT_MAX : r.y, ux1 = empty ? 0 : r.z, uy1 = empty ? 0 : r.w;
        ux0 = nmw::wave_min(ux0); uy0 = nmw::wave_min(uy0); ux1 = nmw::wave_max(ux1); uy1 = nmw::wave_max(uy1);
        if (tid == 0) s_union = make_int4(ux0, uy0, ux1, uy1);
    }
    __syncthreads();
    const int4 U = s_union;
    if (U.z <= U.x) return;                            // no frame touches the canvas (uniform)
    const int4 mine = s_rect[lane];                    // lane l tests frame l's rectangle (empty beyond n)
    const int tiles_x = (U.z - U.x + CANVAS_TILE_W - 1) / CANVAS_TILE_W;
    const int tiles = tiles_x * ((U.w - U.y + CANVAS_TILE_H - 1) / CANVAS_TILE_H);
    const Tex none{nullptr, fw, fh, 0};
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int ty_ = t / tiles_x, tx_ = t - ty_ * tiles_x;
        const int row = U.y + ty_ * CANVAS_TILE_H + wave, xs = U.x + tx_ * CANVAS_TILE_W;
        const int px = xs + lane;
        unsigned long long fm = __ballot(mine.y <= row && row < mine.w && mine.x < xs + CANVAS_TILE_W && xs < mine.z);
        if (!fm) continue;                             // wave-uniform
        const size_t idx = (size_t)row * cw + px;
        bool have = false;
        uchar4 c = make_uchar4(0, 0, 0, 0);
        float cwt = 0.f;
        while (fm) {
            const int k = __builtin_ctzll(fm);
            fm &= fm - 1ull;
            const int4 r = s_rect[k];
            if (px < r.x || px >= r.z) continue;
            const int2 t0 = s_t[k];
            Tex frame = none, mask = none, wts = none;
            frame.data = s_ptr[0][k]; frame.fmt = NM_TEX_U8X4N;
            mask.data = s_ptr[1][k]; mask.fmt = mask_format;
            wts.data = s_ptr[2][k]; wts.fmt = wts_format;
            float rgb[4], nwt;
            if (!blend_sample(s_m[k], frame, mask, wts, px - t0.x, row - t0.y, rgb, nwt)) continue;
            if (GAIN) {
                rgb[0] = rgb[0] * s_gain[k][0]; rgb[1] = rgb[1] * s_gain[k][1]; rgb[2] = rgb[2] * s_gain[k][2];
            }
            if (!have) {
                cwt = canvas_wts[idx];
                c = canvas[idx];
                have = true;
            }
            blend_combine(rgb, nwt, c, cwt);
        }
        if (have) {
            canvas_wts[idx] = cwt;
            canvas[idx] = c;
        }
    }
}

}  // namespace

extern "C" {

int nm_mosaic_plan_host_f32(int n, const float *H, const int *status, int fw, int fh, int cw, int ch, int ox, int oy,
                            const float *M_first, nm_mosaic_record *records, float *chain, float *extent)
{
    if (!mp_sizes_ok(n, fw, fh, cw, ch, ox, oy, records) || !(H || n == 1)) return (int)hipErrorInvalidValue;
    float M[NM_MOSAIC_MAX_BATCH][9];
    int ok[NM_MOSAIC_MAX_BATCH];
    mp_chain(n, H, status, M_first, M, ok);
    bool any = false;
    float e[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < n; ++k) {
        float box[4];
        const bool placed = mp_frame(M[k], ok[k], fw, fh, cw, ch, ox, oy, records[k], box);
        if (chain)
            for (int q = 0; q < 9; ++q) chain[9 * k + q] = M[k][q];
        if (placed) mp_extent_add(any, e, box);
    }
    if (extent)
        for (int q = 0; q < 4; ++q) extent[q] = e[q];
    return 0;
}

int nm_mosaic_plan_f32(int n, const float *H, const int *status, int fw, int fh, int cw, int ch, int ox, int oy,
                       const float *M_first, nm_mosaic_record *records, float *chain, float *extent, void *stream)
{
    if (!mp_sizes_ok(n, fw, fh, cw, ch, ox, oy, records) || !(H || n == 1)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(mosaic_plan_kernel, dim3(1), dim3(64), 0, nm_stream(stream), n, H, status, fw, fh, cw, ch, ox, oy,
                       M_first, records, chain, extent);
    NM_LAUNCH_CHECK();
    return 0;
}

int nm_mosaic_place_host_f32(int n, const float *chain, const int *frame_status, int fw, int fh, int cw, int ch, int ox,
                             int oy, nm_mosaic_record *records, float *extent)
{
    if (!mp_sizes_ok(n, fw, fh, cw, ch, ox, oy, records) || !chain) return (int)hipErrorInvalidValue;
    bool any = false;
    float e[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < n; ++k) {
        float box[4];
        const float *M = chain + 9 * k;
        if (!mp_frame(M, mp_given(M, frame_status ? frame_status[k] : 1), fw, fh, cw, ch, ox, oy, records[k], box)) continue;
        mp_extent_add(any, e, box);
    }
    if (extent)
        for (int q = 0; q < 4; ++q) extent[q] = e[q];
    return 0;
}

int nm_mosaic_place_f32(int n, const float *chain, const int *frame_status, int fw, int fh, int cw, int ch, int ox, int oy,
                        nm_mosaic_record *records, float *extent, void *stream)
{
    if (!mp_sizes_ok(n, fw, fh, cw, ch, ox, oy, records) || !chain) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(mosaic_place_kernel, dim3(1), dim3(64), 0, nm_stream(stream), n, chain, frame_status, fw, fh, cw, ch,
                       ox, oy, records, extent);
    NM_LAUNCH_CHECK();
    return 0;
}

int nm_transform_blend_batch_gain(unsigned char *canvas, int cw, int ch, float *canvas_wts, int n,
                                  const unsigned char *const *frames, int fw, int fh, const void *const *masks,
                                  int mask_format, const void *const *wts, int wts_format, const nm_mosaic_record *records,
                                  const float *gains, void *stream)
{
    if (n < 1 || n > NM_MOSAIC_MAX_BATCH || !nm_size_ok(cw) || !nm_size_ok(ch) || fw < 1 || fh < 1 || !scalar_fmt(mask_format) ||
        !scalar_fmt(wts_format))
        return (int)hipErrorInvalidValue;
    if (!canvas || !canvas_wts || !records) return (int)hipErrorInvalidValue;
    FrameArgs a;
    if (!fill_frame_args(a, n, frames, masks, wts)) return (int)hipErrorInvalidValue;
    // The grid is fixed here, before the rectangles exist: enough workgroups to fill the chip, never more than the
    // canvas has tiles. A workgroup whose tiles lie outside every rectangle returns after staging the records.
    const int grid = nm_fill_grid((long long)nm_divup(cw, CANVAS_TILE_W) * nm_divup(ch, CANVAS_TILE_H), MB_BLOCKS_PER_CU);
    const auto kernel = gains ? transform_blend_batch_kernel<true> : transform_blend_batch_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(CANVAS_THREADS), 0, nm_stream(stream), a, n,
                       reinterpret_cast<uchar4 *>(canvas), cw, ch, canvas_wts, fw, fh, mask_format, wts_format, records, gains);
    NM_LAUNCH_CHECK();
    return 0;
}

int nm_transform_blend_batch(unsigned char *canvas, int cw, int ch, float *canvas_wts, int n,
                             const unsigned char *const *frames, int fw, int fh, const void *const *masks, int mask_format,
                             const void *const *wts, int wts_format, const nm_mosaic_record *records, void *stream)
{
    return nm_transform_blend_batch_gain(canvas, cw, ch, canvas_wts, n, frames, fw, fh, masks, mask_format, wts, wts_format,
                                         records, nullptr, stream);
}

}  // extern "C"
