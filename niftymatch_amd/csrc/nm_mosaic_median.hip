// nm_mosaic_median.hip -- median composite of up to NM_MOSAIC_MAX_BATCH placed frames' tiles into one canvas, for gfx950
// (include/nm_abi.h, "Median mosaic composite", has the written semantics). No reference counterpart. On the caller's
// stream, no allocation, no synchronisation, no host read, no workspace; no workgroup waits for another. ONE launch, and one
// more of a single workgroup that zeroes counts, only when counts is given. (A memset node would do, but the HIP runtime
// this was measured on replays a captured memset node correctly once and writes other values from the second replay on:
// DESIGN.md section 7, "Median composite". A kernel node replays like every other launch.)
//   The canvas walk is the two-band blend's (mosaic_bands_canvas_kernel: 64-bit clipping, the n records staged in LDS, one
//   ballot over the frames whose rectangle meets the wave's row of the tile, grid-stride over the tiles of the rectangles'
//   union), with a workgroup of TWO waves: a tile is 64 x 2 canvas pixels, a row per wave, a pixel per lane.
//   pass 1   a lane reads its float4 from every covering frame (lanes along x: coalesced) and appends the key and the frame
//            index of each VALID one to its own list in LDS, lane-strided [slot][lane]: 64 slots x 128 lanes x 4 B = 32 KB
//            of keys (a lane's slot s is word s * 128 + lane: one bank per lane, no conflict) and 8 KB of indices. The list
//            holds all 64 frames, so there is one route whatever m is; an array indexed at run time would go to scratch.
//            The list is in index order, so the rank rule's tie-break is the slot order.
//   rank     by counting over the list, m^2 compares from LDS, stopping at the slot of rank (m - 1) / 2.
//   pass 2   the covering frames again, wave-uniform, with a per-lane cursor into the list: the inlier test on the listed
//            key, the support, and (MEAN) a second read of the inliers' samples for the weighted mean; SELECT reads the
//            median frame's sample once more. No sample is kept in registers across the walk.
//   counts   per frame, a ballot's population count per wave row (nmw::wave_count) into lane k's register; after the walk the
//            two waves' registers are added in LDS and each non-zero total costs one vector atomic add.
// A lane touches only its own column of the list, so the walk needs no barrier. The arithmetic is
// nm_mosaic_median_math.hpp, shared with the host twin below: both agree bit for bit.
#include <climits>
#include <cmath>

#include "nm_mosaic_batch.hpp"
#include "nm_mosaic_median_math.hpp"
#include "nm_wave_dev.hpp"

namespace {

using namespace nmb;
using namespace nmmb;
using namespace nmmd;

constexpr int WAVES = 2, THREADS = 64 * WAVES, TILE_W = 64, TILE_H = WAVES, BLOCKS_PER_CU = 8;

__host__ __device__ __forceinline__ size_t sample_at(int k, long long tile_cap, const int4 &b, int px, int row)
{
    return (size_t)k * (size_t)tile_cap + (size_t)(row - b.y) * b.z + (px - b.x);
}

template <int MODE, bool COUNTS>
__global__ __launch_bounds__(THREADS) void mosaic_median_kernel(int n, const nm_mosaic_record *__restrict__ records,
                                                                long long tile_cap, const float4 *__restrict__ tiles, int cw,
                                                                int ch, float w_min, float tau, uchar4 *__restrict__ canvas,
                                                                float *__restrict__ canvas_wts,
                                                                unsigned char *__restrict__ support,
                                                                unsigned char *__restrict__ label,
                                                                unsigned long long *__restrict__ counts)
{
    __shared__ float s_key[MAX_FRAMES][THREADS];          // the lane's keys of its valid frames, in index order
    __shared__ unsigned char s_idx[MAX_FRAMES][THREADS];  // and their frame indices
    __shared__ int4 s_box[MAX_FRAMES];                    // tx, ty, nw, nh
    __shared__ int4 s_rect[MAX_FRAMES];                   // clipped (x0, y0, x1, y1); (0, 0, 0, 0) when empty
    __shared__ int4 s_union;
    __shared__ unsigned s_cnt[COUNTS ? WAVES : 1][MAX_FRAMES][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 64) {
        int4 r = make_int4(0, 0, 0, 0), b = r;
        if (tid < n) {
            const nm_mosaic_record *rec = records + tid;
            const int tx = rec->tx, ty = rec->ty, nw = rec->nw, nh = rec->nh;
            if (frame_used(rec->placed, nw, nh, tile_cap)) {
                b = make_int4(tx, ty, nw, nh);
                r = clip_rect(tx, ty, nw, nh, cw, ch);
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
    if (U.z <= U.x) return;                            // no frame touches the canvas (uniform): the counts stay zero
    const int4 mine = s_rect[lane];
    const int tiles_x = (U.z - U.x + TILE_W - 1) / TILE_W;
    const int ntiles = tiles_x * ((U.w - U.y + TILE_H - 1) / TILE_H);
    unsigned n_valid = 0, n_out = 0;                   // of frame `lane`, over this wave's rows
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int ty_ = t / tiles_x, tx_ = t - ty_ * tiles_x;
        const int row = U.y + ty_ * TILE_H + wave, xs = U.x + tx_ * TILE_W;
        const int px = xs + lane;
        const unsigned long long fm = __ballot(mine.y <= row && row < mine.w && mine.x < xs + TILE_W && xs < mine.z);
        if (!fm) continue;                             // wave-uniform
        int m = 0;
        for (unsigned long long f = fm; f; f &= f - 1ull) {            // pass 1: the keys of the valid frames
            const int k = __builtin_ctzll(f);
            const int4 r = s_rect[k];
            bool v = false;
            if (px >= r.x && px < r.z) {
                const float4 s = tiles[sample_at(k, tile_cap, s_box[k], px, row)];
                const float y = key_of(s);
                v = valid(s.w, y, w_min);
                if (v) {
                    s_key[m][tid] = y;
                    s_idx[m][tid] = (unsigned char)k;
                    ++m;
                }
            }
            if (COUNTS) {
                const unsigned c = nmw::wave_count(v);
                if (lane == k) n_valid += c;
            }
        }
        int med = 0;                                   // the slot of the lower median
        if (m > 1) {
            const int target = median_rank(m);
            for (int i = 0; i < m; ++i) {
                const float yi = s_key[i][tid];
                int rank = 0;
                for (int j = 0; j < m; ++j) rank += before(s_key[j][tid], j, yi, i);
                if (rank == target) { med = i; break; }
            }
        }
        const float y_med = m ? s_key[med][tid] : 0.f;
        int cur = 0, s_in = 0;
        Mean mean;
        for (unsigned long long f = fm; f; f &= f - 1ull) {            // pass 2: inliers
            const int k = __builtin_ctzll(f);
            const bool listed = cur < m && s_idx[cur][tid] == k;
            bool in = false;
            if (listed) {
                in = inlier(s_key[cur][tid], y_med, tau);
                if (in) {
                    ++s_in;
                    if (MODE == NM_MEDIAN_MEAN) mean.add(tiles[sample_at(k, tile_cap, s_box[k], px, row)]);
                }
                ++cur;
            }
            if (COUNTS) {
                const unsigned c = nmw::wave_count(listed && !in);
                if (lane == k) n_out += c;
            }
        }
        if (!m) continue;                              // no valid frame here: every output keeps its contents
        const int k_med = s_idx[med][tid];
        const size_t idx = (size_t)row * cw + px;      // m > 0: a rectangle holds (px, row), inside the canvas
        float weight;
        uchar4 out;
        if (MODE == NM_MEDIAN_MEAN) out = mean.finish(weight);
        else out = finish_select(tiles[sample_at(k_med, tile_cap, s_box[k_med], px, row)], weight);
        canvas[idx] = out;
        if (canvas_wts) canvas_wts[idx] = weight;
        if (support) support[idx] = (unsigned char)s_in;
        if (label) label[idx] = (unsigned char)k_med;
    }
    if (COUNTS) {
        s_cnt[wave][lane][0] = n_valid;
        s_cnt[wave][lane][1] = n_out;
        __syncthreads();
        unsigned long long total = 0;
        for (int w = 0; w < WAVES; ++w) total += s_cnt[w][tid >> 1][tid & 1];
        if (total) atomicAdd(counts + tid, total);     // tid = 2 k + q; frames >= n count nothing
    }
}

bool median_args_ok(int n, const void *tiles, long long tile_cap, const void *records, const void *canvas, int cw, int ch,
                    int mode, float w_min, float tau)
{
    return n >= 1 && n <= MAX_FRAMES && tile_cap >= 1 && tile_cap <= MAX_TILE_CAP && nm_size_ok(cw) && nm_size_ok(ch) &&
           mode >= 0 && mode < MODES && std::isfinite(w_min) && w_min >= 0.f && tau >= 0.f && tiles && records && canvas &&
           (reinterpret_cast<size_t>(tiles) & 15) == 0;
}

}  // namespace

extern "C" {

int nm_mosaic_median_dev(int n, const float *tiles, long long tile_cap, const nm_mosaic_record *records,
                         unsigned char *canvas, int cw, int ch, float *canvas_wts, int mode, float w_min, float tau,
                         unsigned char *support, unsigned char *label, unsigned long long *counts, void *stream)
{
    if (!median_args_ok(n, tiles, tile_cap, records, canvas, cw, ch, mode, w_min, tau)) return (int)hipErrorInvalidValue;
    hipStream_t st = nm_stream(stream);
    if (counts) NM_RETURN_IF(nmp::launch_zero_u64(counts, 2 * (size_t)n, st));
    const int grid = nm_fill_grid((long long)nm_divup(cw, TILE_W) * nm_divup(ch, TILE_H), BLOCKS_PER_CU);
    const auto kernel = mode == NM_MEDIAN_MEAN
                            ? (counts ? mosaic_median_kernel<NM_MEDIAN_MEAN, true> : mosaic_median_kernel<NM_MEDIAN_MEAN, false>)
                            : (counts ? mosaic_median_kernel<NM_MEDIAN_SELECT, true> : mosaic_median_kernel<NM_MEDIAN_SELECT, false>);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(THREADS), 0, st, n, records, tile_cap, reinterpret_cast<const float4 *>(tiles), cw,
                       ch, w_min, tau, reinterpret_cast<uchar4 *>(canvas), canvas_wts, support, label, counts);
    NM_LAUNCH_CHECK();
    return 0;
}

int nm_mosaic_median_host(int n, const float *tiles, long long tile_cap, const nm_mosaic_record *records,
                          unsigned char *canvas, int cw, int ch, float *canvas_wts, int mode, float w_min, float tau,
                          unsigned char *support, unsigned char *label, unsigned long long *counts)
{
    if (!median_args_ok(n, tiles, tile_cap, records, canvas, cw, ch, mode, w_min, tau)) return (int)hipErrorInvalidValue;
    const float4 *t4 = reinterpret_cast<const float4 *>(tiles);
    uchar4 *cv = reinterpret_cast<uchar4 *>(canvas);
    int4 box[MAX_FRAMES], rect[MAX_FRAMES];
    int ux0 = INT_MAX, uy0 = INT_MAX, ux1 = 0, uy1 = 0;
    for (int k = 0; k < n; ++k) {
        const nm_mosaic_record &rec = records[k];
        box[k] = rect[k] = make_int4(0, 0, 0, 0);
        if (counts) counts[2 * k] = counts[2 * k + 1] = 0;
        if (!frame_used(rec.placed, rec.nw, rec.nh, tile_cap)) continue;
        box[k] = make_int4(rec.tx, rec.ty, rec.nw, rec.nh);
        rect[k] = clip_rect(rec.tx, rec.ty, rec.nw, rec.nh, cw, ch);
        if (rect[k].z == 0) continue;
        ux0 = rect[k].x < ux0 ? rect[k].x : ux0; uy0 = rect[k].y < uy0 ? rect[k].y : uy0;
        ux1 = rect[k].z > ux1 ? rect[k].z : ux1; uy1 = rect[k].w > uy1 ? rect[k].w : uy1;
    }
    for (int row = uy0; row < uy1; ++row)
        for (int px = ux0; px < ux1; ++px) {
            float key[MAX_FRAMES];
            int frame[MAX_FRAMES], m = 0;
            for (int k = 0; k < n; ++k) {
                if (px < rect[k].x || px >= rect[k].z || row < rect[k].y || row >= rect[k].w) continue;
                const float4 s = t4[sample_at(k, tile_cap, box[k], px, row)];
                const float y = key_of(s);
                if (!valid(s.w, y, w_min)) continue;
                key[m] = y;
                frame[m++] = k;
            }
            if (!m) continue;
            int med = 0;
            for (int i = 0; i < m; ++i) {
                int rank = 0;
                for (int j = 0; j < m; ++j) rank += before(key[j], frame[j], key[i], frame[i]);
                if (rank == median_rank(m)) med = i;
            }
            int s_in = 0;
            Mean mean;
            for (int j = 0; j < m; ++j) {
                const bool in = inlier(key[j], key[med], tau);
                if (counts) { counts[2 * frame[j]] += 1; counts[2 * frame[j] + 1] += !in; }
                if (!in) continue;
                ++s_in;
                if (mode == NM_MEDIAN_MEAN) mean.add(t4[sample_at(frame[j], tile_cap, box[frame[j]], px, row)]);
            }
            const size_t idx = (size_t)row * cw + px;
            float weight;
            cv[idx] = mode == NM_MEDIAN_MEAN
                          ? mean.finish(weight)
                          : finish_select(t4[sample_at(frame[med], tile_cap, box[frame[med]], px, row)], weight);
            if (canvas_wts) canvas_wts[idx] = weight;
            if (support) support[idx] = (unsigned char)s_in;
            if (label) label[idx] = (unsigned char)frame[med];
        }
    return 0;
}

}  // extern "C"
