// nm_frame_weights.hip -- per-frame validity masks and feather weights of up to NM_FRAME_WEIGHTS_MAX_BATCH BGRA frames, for
// gfx950 (include/nm_abi.h, "Frame masks and feather weights", has the written semantics). No reference counterpart. On the
// caller's stream, no allocation, no synchronisation, no host read; no workgroup waits for another. TWO launches whatever n
// is, and one more of a single workgroup that zeroes counts, only when counts is given (a kernel, not a memset node:
// nm_mosaic_median.hip says why). The transform is the separable exact one: D(p) = min over rows of dy^2 + g^2, where g is
// the distance along a row to its nearest seed.
//   row pass     a workgroup of four waves takes a unit = (frame, strip of ROW_SR rows, chunk of up to ROW_CB 64-pixel
//                blocks), grid-stride over the units. Three phases with a barrier between them, each a walk of the waves
//                over (row, block) items with a lane per pixel:
//                1  the raw-bad bits: coalesced uchar4 loads, ROW_UNROLL items' loads in flight per wave, one ballot per
//                   item into LDS. With min_count > 1 the strip has a one-row halo and the chunk a two-block one (the 3 x 3
//                   count of a seed one block out needs the bit of a pixel one further); blocks and rows outside the frame
//                   are zero words and cost no load.
//                2  the seed bits of the chunk and one block either side: the 3 x 3 count from nine shifts of the words in
//                   LDS (row3), the base plane's byte, the seed rule, one ballot per item into LDS.
//                3  g from the three seed words round the lane's block with shifts and clz / ctz (g_of), no scan over taps;
//                   one byte per pixel to the workspace, rows padded to whole blocks (pad pixels hold R + 1).
//   column pass  a unit = (frame, strip of COL_CR rows, one 64-pixel block). The strip's g and R rows above and below go to
//                LDS as dwords (rows outside the frame as R + 1). A wave takes every fourth row, a lane a pixel, and walks dy
//                outward from 0 until no lane's dy^2 is below its running minimum (one compare into a ballot). A tile with no
//                g <= R anywhere (the inside of a clean frame) skips the walk: D = R^2 there. Mask, weight and dist2 are
//                written with lanes along x. Counts: a ballot's population count per wave row into a wave-uniform register;
//                when a workgroup's walk moves to another frame, and at its end, the four waves' registers are added in LDS
//                and each non-zero total costs one vector atomic add.
// Per-frame pointers travel as kernel arguments, as in the ingest and warp-tile launches. The arithmetic is
// nm_frame_weights_math.hpp, shared with the host twin below: both agree bit for bit.
#include <atomic>
#include <vector>

#include "../../include/nm_abi.h"
#include "nm_common.hpp"
#include "nm_frame_weights_math.hpp"
#include "nm_pair_batch.hpp"

namespace {

using namespace nmfw;

constexpr int WAVES = 4, THREADS = 64 * WAVES, BLOCKS_PER_CU = 8;
constexpr int ROW_SR = 8, ROW_CB = 32, ROW_UNROLL = 4;
constexpr int COL_CR = 128, COL_ROWS = COL_CR + 2 * MAX_RADIUS;
constexpr size_t WS_ALIGN = 64;

std::atomic<int> g_grid_cap{0};                 // nm_frame_weights_set_grid_cap; 0: the default

struct FwFrames { const uchar4 *frames[MAX_FRAMES]; };                      // 512 B of the 4 KB of kernel arguments
struct FwOut {                                                              // 1.5 KB
    void *masks[MAX_FRAMES];
    float *wts[MAX_FRAMES];
    unsigned short *dist2[MAX_FRAMES];
};
static_assert(sizeof(FwOut) + 128 < 4096, "frame-weights kernel arguments exceed 4 KB");

__host__ __device__ __forceinline__ int pitch_of(int fw) { return (fw + 63) & ~63; }

// COUNT3: min_count > 1, the 3 x 3 count is needed (else every raw-bad pixel is a seed and the halo rows are not read)
template <bool COUNT3>
__global__ __launch_bounds__(THREADS) void frame_weights_row_kernel(const FwFrames a, int n, int fw, int fh,
                                                                    const unsigned char *__restrict__ base, int lo, int hi,
                                                                    int min_count, int border, int R,
                                                                    unsigned char *__restrict__ g, int strips, int chunks)
{
    __shared__ unsigned long long s_bad[ROW_SR + 2][ROW_CB + 4];   // row y0 - 1 + i, block b0 - 2 + j
    __shared__ unsigned long long s_seed[ROW_SR][ROW_CB + 2];      // row y0 + i, block b0 - 1 + j
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nblk = (fw + 63) >> 6, pitch = nblk << 6;
    const size_t plane = (size_t)pitch * fh;
    const long long units = (long long)n * strips * chunks;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const int c = (int)(u % chunks);
        const long long t = u / chunks;
        const int s = (int)(t % strips), k = (int)(t / strips);
        const int y0 = s * ROW_SR, b0 = c * ROW_CB;
        const int nb = nblk - b0 < ROW_CB ? nblk - b0 : ROW_CB;
        const int rows = fh - y0 < ROW_SR ? fh - y0 : ROW_SR;
        const uchar4 *__restrict__ f = a.frames[k];
        // phase 1: the raw-bad words
        const int r_first = COUNT3 ? 0 : 1, r_count = COUNT3 ? rows + 2 : rows, cols = nb + 4;
        const int items = r_count * cols;
        for (int it0 = wave * ROW_UNROLL; it0 < items; it0 += WAVES * ROW_UNROLL) {
            uchar4 px[ROW_UNROLL];
            bool in[ROW_UNROLL];
#pragma unroll
            for (int j = 0; j < ROW_UNROLL; ++j) {
                const int it = it0 + j, rr = r_first + it / cols, cc = it % cols;
                const int y = y0 - 1 + rr, b = b0 - 2 + cc, x = (b << 6) + lane;
                in[j] = it < items && y >= 0 && y < fh && b >= 0 && x < fw;
                px[j] = make_uchar4(0, 0, 0, 0);
                if (in[j]) px[j] = f[(size_t)y * fw + x];
            }
#pragma unroll
            for (int j = 0; j < ROW_UNROLL; ++j) {
                const int it = it0 + j;
                if (it >= items) break;                            // wave-uniform
                const unsigned long long w = __ballot(in[j] && raw_bad(px[j].x, px[j].y, px[j].z, lo, hi));
                if (lane == 0) s_bad[r_first + it / cols][it % cols] = w;
            }
        }
        __syncthreads();
        // phase 2: the seed words of blocks b0 - 1 .. b0 + nb
        const int cols2 = nb + 2;
        for (int it = wave; it < rows * cols2; it += WAVES) {
            const int r = it / cols2, cc = it % cols2;
            const int y = y0 + r, b = b0 - 1 + cc, x = (b << 6) + lane;
            unsigned long long w = 0;
            if (b >= 0 && b < nblk) {                              // wave-uniform
                const unsigned long long(*row)[ROW_CB + 4] = &s_bad[r + 1];
                const bool bad = (row[0][cc + 1] >> lane) & 1ull;
                int count = bad;
                if (COUNT3) {
                    count = 0;
#pragma unroll
                    for (int d = -1; d <= 1; ++d) count += row3(row[d][cc], row[d][cc + 1], row[d][cc + 2], lane);
                }
                const bool base_zero = base && x < fw && base[(size_t)y * fw + x] == 0;
                w = __ballot(x < fw && seed_rule(base_zero, bad, count, min_count));
            }
            if (lane == 0) s_seed[r][cc] = w;
        }
        __syncthreads();
        // phase 3: g, one byte per pixel, whole blocks
        for (int it = wave; it < rows * nb; it += WAVES) {
            const int r = it / nb, cc = it % nb;
            const int y = y0 + r, x = ((b0 + cc) << 6) + lane;
            int gv = g_of(s_seed[r][cc], s_seed[r][cc + 1], s_seed[r][cc + 2], lane, R);
            if (border) gv = g_border(gv, x, fw);
            if (x >= fw) gv = R + 1;                               // the pad of the last block
            g[(size_t)k * plane + (size_t)y * pitch + x] = (unsigned char)gv;
        }
        __syncthreads();                                           // the next unit rewrites both arrays
    }
}

template <bool COUNTS>
__device__ __forceinline__ void flush_counts(unsigned (*s_cnt)[2], unsigned long long *counts, int k, unsigned n_seed,
                                             unsigned n_valid)
{
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) {
        s_cnt[tid >> 6][0] = n_seed;
        s_cnt[tid >> 6][1] = n_valid;
    }
    __syncthreads();
    if (tid < 2) {
        unsigned long long total = 0;
        for (int w = 0; w < WAVES; ++w) total += s_cnt[w][tid];
        if (total) atomicAdd(counts + 2 * k + tid, total);
    }
    __syncthreads();
}

template <bool COUNTS>
__global__ __launch_bounds__(THREADS) void frame_weights_col_kernel(const FwOut o, int n, int fw, int fh, int border, int R,
                                                                    int margin, int mask_format,
                                                                    const unsigned char *__restrict__ g,
                                                                    unsigned long long *__restrict__ counts, int strips)
{
    __shared__ __align__(16) unsigned char s_g[COL_ROWS][64];      // row y0 - R + i of the unit's block
    __shared__ unsigned s_cnt[WAVES][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nblk = (fw + 63) >> 6, pitch = nblk << 6, R2 = R * R;
    const size_t plane = (size_t)pitch * fh;
    const unsigned fill = (unsigned)(R + 1) * 0x01010101u;
    const long long units = (long long)n * strips * nblk;
    int cur = -1;                                                  // the frame the two registers count for
    unsigned n_seed = 0, n_valid = 0;                              // wave-uniform
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const int bx = (int)(u % nblk);
        const long long t = u / nblk;
        const int s = (int)(t % strips), k = (int)(t / strips);
        if (COUNTS && k != cur) {                                  // workgroup-uniform
            if (cur >= 0) flush_counts<COUNTS>(s_cnt, counts, cur, n_seed, n_valid);
            cur = k;
            n_seed = n_valid = 0;
        }
        const int y0 = s * COL_CR;
        const int rows = fh - y0 < COL_CR ? fh - y0 : COL_CR, trows = rows + 2 * R;
        const unsigned char *__restrict__ gk = g + (size_t)k * plane + ((size_t)bx << 6);
        int any = 0;                                               // a g <= R in the tile
#pragma unroll 4
        for (int i = tid; i < trows * 16; i += THREADS) {
            const int tr = i >> 4, q = i & 15, y = y0 - R + tr;
            unsigned v = fill;
            if (y >= 0 && y < fh) v = *reinterpret_cast<const unsigned *>(gk + (size_t)y * pitch + (q << 2));
            *reinterpret_cast<unsigned *>(&s_g[tr][q << 2]) = v;
            const unsigned b0 = v & 255u, b1 = (v >> 8) & 255u, b2 = (v >> 16) & 255u, b3 = v >> 24;
            const unsigned m01 = b0 < b1 ? b0 : b1, m23 = b2 < b3 ? b2 : b3;
            any |= (int)((m01 < m23 ? m01 : m23) <= (unsigned)R);
        }
        const int near = __syncthreads_or(any);
        const int x = (bx << 6) + lane;
        const bool in = x < fw;
        for (int r = wave; r < rows; r += WAVES) {
            const int y = y0 + r, tr = r + R;
            int best = d_init(s_g[tr][lane], R2);
            if (near)
                for (int dy = 1; dy <= R; ++dy) {
                    if (!__ballot(in && dy * dy < best)) break;    // no lane can still improve
                    best = d_step(best, dy, s_g[tr - dy][lane], s_g[tr + dy][lane]);
                }
            if (border) best = d_border(best, y, fh);
            const bool ok = valid(best, margin);
            if (in) {
                const size_t idx = (size_t)y * fw + x;
                if (o.masks[k]) {
                    if (mask_format == NM_TEX_F32) static_cast<float *>(o.masks[k])[idx] = ok ? 1.f : 0.f;
                    else static_cast<unsigned char *>(o.masks[k])[idx] = ok ? 255 : 0;
                }
                if (o.wts[k]) o.wts[k][idx] = weight_of(best, margin, R);
                if (o.dist2[k]) o.dist2[k][idx] = (unsigned short)best;
            }
            if (COUNTS) {
                n_seed += nmw::wave_count(in && best == 0);
                n_valid += nmw::wave_count(in && ok);
            }
        }
        __syncthreads();                                           // the next unit rewrites the tile
    }
    if (COUNTS && cur >= 0) flush_counts<COUNTS>(s_cnt, counts, cur, n_seed, n_valid);
}

bool shape_ok(int n, int fw, int fh) { return n >= 1 && n <= MAX_FRAMES && nm_size_ok(fw) && nm_size_ok(fh); }

bool args_ok(int n, const unsigned char *const *frames, int fw, int fh, int lo, int hi, int min_count, int R, int margin,
             void *const *masks, int mask_format, float *const *wts, unsigned short *const *dist2,
             const unsigned long long *counts)
{
    if (!shape_ok(n, fw, fh) || lo < 0 || lo > 255 || hi < 0 || hi > 255 || min_count < 1 || min_count > 9 || R < 1 ||
        R > MAX_RADIUS || margin < 0 || margin >= R || (mask_format != NM_TEX_U8N && mask_format != NM_TEX_F32) ||
        !(masks || wts || dist2 || counts))
        return false;
    return nmp::tables_ok(n, {frames}, {masks, wts, dist2}, {});
}

int grid_of(long long units)
{
    const int cap = g_grid_cap.load();                 // nm_frame_weights_set_grid_cap: tests make small grids walk far
    return cap > 0 ? (int)(units < cap ? units : cap) : nm_fill_grid(units, BLOCKS_PER_CU);
}

}  // namespace

extern "C" {

int nm_frame_weights_set_grid_cap(int cap) { return g_grid_cap.exchange(cap < 1 ? 0 : cap); }

size_t nm_frame_weights_workspace_bytes(int n, int fw, int fh)
{
    if (!shape_ok(n, fw, fh)) return 0;
    return (size_t)n * pitch_of(fw) * fh + WS_ALIGN;
}

int nm_frame_weights_batch_dev(int n, const unsigned char *const *frames, int fw, int fh, const unsigned char *base, int lo,
                               int hi, int min_count, int border, int R, int margin, void *const *masks, int mask_format,
                               float *const *wts, unsigned short *const *dist2, unsigned long long *counts, void *workspace,
                               void *stream)
{
    if (!args_ok(n, frames, fw, fh, lo, hi, min_count, R, margin, masks, mask_format, wts, dist2, counts) || !workspace)
        return (int)hipErrorInvalidValue;
    FwFrames a;
    FwOut o;
    nmp::fill_slots_as(a.frames, frames, 0, n);
    nmp::fill_slots(o.masks, masks, 0, n); nmp::fill_slots(o.wts, wts, 0, n); nmp::fill_slots(o.dist2, dist2, 0, n);
    unsigned char *g = reinterpret_cast<unsigned char *>((reinterpret_cast<size_t>(workspace) + WS_ALIGN - 1) & ~(WS_ALIGN - 1));
    const hipStream_t st = nm_stream(stream);
    if (counts) NM_RETURN_IF(nmp::launch_zero_u64(counts, 2 * (size_t)n, st));
    const int nblk = nm_divup(fw, 64);
    const int strips = nm_divup(fh, ROW_SR), chunks = nm_divup(nblk, ROW_CB);
    const auto row = min_count > 1 ? frame_weights_row_kernel<true> : frame_weights_row_kernel<false>;
    hipLaunchKernelGGL(row, dim3(grid_of((long long)n * strips * chunks)), dim3(THREADS), 0, st, a, n, fw, fh, base, lo, hi,
                       min_count, border, R, g, strips, chunks);
    NM_LAUNCH_CHECK();
    const int cstrips = nm_divup(fh, COL_CR);
    const auto col = counts ? frame_weights_col_kernel<true> : frame_weights_col_kernel<false>;
    hipLaunchKernelGGL(col, dim3(grid_of((long long)n * cstrips * nblk)), dim3(THREADS), 0, st, o, n, fw, fh, border, R, margin,
                       mask_format, g, counts, cstrips);
    NM_LAUNCH_CHECK();
    return 0;
}

int nm_frame_weights_host(int n, const unsigned char *const *frames, int fw, int fh, const unsigned char *base, int lo, int hi,
                          int min_count, int border, int R, int margin, void *const *masks, int mask_format,
                          float *const *wts, unsigned short *const *dist2, unsigned long long *counts)
{
    if (!args_ok(n, frames, fw, fh, lo, hi, min_count, R, margin, masks, mask_format, wts, dist2, counts))
        return (int)hipErrorInvalidValue;
    const int nblk = nm_divup(fw, 64), wpr = nblk + 2;             // a zero word either side of every row of words
    std::vector<unsigned long long> bad((size_t)(fh + 2) * wpr), seed((size_t)fh * wpr);
    std::vector<unsigned char> g((size_t)fw * fh);
    for (int k = 0; k < n; ++k) {
        std::fill(bad.begin(), bad.end(), 0ull);
        std::fill(seed.begin(), seed.end(), 0ull);
        const unsigned char *f = frames[k];
        for (int y = 0; y < fh; ++y)
            for (int x = 0; x < fw; ++x) {
                const unsigned char *p = f + 4 * ((size_t)y * fw + x);
                if (raw_bad(p[0], p[1], p[2], lo, hi)) bad[(size_t)(y + 1) * wpr + 1 + (x >> 6)] |= 1ull << (x & 63);
            }
        for (int y = 0; y < fh; ++y)
            for (int x = 0; x < fw; ++x) {
                const int b = x >> 6, lane = x & 63;
                const unsigned long long *row = &bad[(size_t)(y + 1) * wpr + b];      // word b - 1 of row y
                int count = 0;
                for (int d = -1; d <= 1; ++d) count += row3(row[d * wpr], row[d * wpr + 1], row[d * wpr + 2], lane);
                const bool base_zero = base && base[(size_t)y * fw + x] == 0;
                if (seed_rule(base_zero, (row[1] >> lane) & 1ull, count, min_count))
                    seed[(size_t)y * wpr + 1 + b] |= 1ull << lane;
            }
        for (int y = 0; y < fh; ++y)
            for (int x = 0; x < fw; ++x) {
                const unsigned long long *w = &seed[(size_t)y * wpr + (x >> 6)];
                int gv = g_of(w[0], w[1], w[2], x & 63, R);
                if (border) gv = g_border(gv, x, fw);
                g[(size_t)y * fw + x] = (unsigned char)gv;
            }
        unsigned long long n_seed = 0, n_valid = 0;
        for (int y = 0; y < fh; ++y)
            for (int x = 0; x < fw; ++x) {
                int best = d_init(g[(size_t)y * fw + x], R * R);
                for (int dy = 1; dy <= R && dy * dy < best; ++dy) {
                    const int above = y - dy >= 0 ? g[(size_t)(y - dy) * fw + x] : R + 1;
                    const int below = y + dy < fh ? g[(size_t)(y + dy) * fw + x] : R + 1;
                    best = d_step(best, dy, above, below);
                }
                if (border) best = d_border(best, y, fh);
                const bool ok = valid(best, margin);
                const size_t idx = (size_t)y * fw + x;
                if (masks) {
                    if (mask_format == NM_TEX_F32) static_cast<float *>(masks[k])[idx] = ok ? 1.f : 0.f;
                    else static_cast<unsigned char *>(masks[k])[idx] = ok ? 255 : 0;
                }
                if (wts) wts[k][idx] = weight_of(best, margin, R);
                if (dist2) dist2[k][idx] = (unsigned short)best;
                n_seed += best == 0;
                n_valid += ok;
            }
        if (counts) {
            counts[2 * k] = n_seed;
            counts[2 * k + 1] = n_valid;
        }
    }
    return 0;
}

}  // extern "C"
