// nm_frame_quality.hip -- per-frame, per-cell exact quality statistics of up to NM_FRAME_QUALITY_MAX_BATCH BGRA frames, the
// keyframe choice on them and the gather that compacts any per-frame table by that choice, for gfx950 (include/nm_abi.h,
// "Frame quality and keyframe choice", has the written semantics). No reference counterpart. On the caller's stream, no
// allocation, no synchronisation, no host read; no workgroup waits for another.
//   statistics  TWO launches: nmp::launch_zero_u64 on stats, then the walk. A workgroup of four waves takes a unit = (frame,
//               strip of STRIP rows, block of 64 columns), grid-stride over the units; each wave takes WAVE_ROWS rows of the
//               strip and a lane owns a column. The wave walks down with the rows above, at and below the centre row in
//               registers (luminance and class bits packed in one word per row), UNROLL rows' coalesced uchar4 loads in flight;
//               the row neighbours come from the lanes either side, lanes 0 and 63 load the one-column halo. A lane adds its
//               eight sums in 32-bit registers (at most WAVE_ROWS pixels of 1 040 400); when the centre row enters another
//               cell row, and at the end of the wave's rows, the registers are summed over the wave per cell column (at most
//               64 x WAVE_ROWS pixels: still 32 bits) and added into the workgroup's LDS table of 64-bit words per cell.
//               When the workgroup's walk moves to another frame, and at its end, each non-zero word of the table costs one
//               64-bit vector atomic add (the counts scheme of nm_frame_weights.hip).
//   pick        ONE launch of one workgroup of four waves: a wave per frame with a lane per cell ranks the cells' sharpness
//               by counting; a lane per frame forms totals, flags and the blur window; wave 0 then walks, a round per
//               keyframe: every lane its own d(last, lane), two ballots and a wave maximum.
//   gather      ONE launch: a unit is (slot, chunk of CHUNK bytes); 16-byte loads and stores when every pointer and the
//               size allow, bytes otherwise.
// The arithmetic is nm_frame_quality_math.hpp, shared with the host twins below: all agree bit for bit.
#include <atomic>
#include <cstring>
#include <vector>

#include "../../include/nm_abi.h"
#include "nm_common.hpp"
#include "nm_frame_quality_math.hpp"
#include "nm_pair_batch.hpp"

namespace {

using namespace nmfq;

constexpr int WAVES = 4, THREADS = 64 * WAVES, BLOCKS_PER_CU = 8;
constexpr int WAVE_ROWS = 32, STRIP = WAVES * WAVE_ROWS, UNROLL = 4;
static_assert(64ll * WAVE_ROWS * 1040400ll < (1ll << 32), "a wave's sums of a cell row must fit 32 bits");
constexpr long long GATHER_CHUNK = 16 * THREADS * 4;      // bytes per gather unit: four 16-byte words per thread

std::atomic<int> g_grid_cap{0};                           // nm_frame_quality_set_grid_cap; 0: the default

struct FqArgs {                                           // 1 KB of the 4 KB of kernel arguments
    const uchar4 *frames[MAX_FRAMES];
    const void *masks[MAX_FRAMES];
};
struct GatherArgs {
    const void *src[MAX_FRAMES];
    void *dst[MAX_FRAMES];
};
static_assert(sizeof(FqArgs) + 128 < 4096 && sizeof(GatherArgs) + 128 < 4096, "kernel arguments exceed 4 KB");

template <int MASK> __device__ __forceinline__ bool eligible_at(const void *m, size_t idx)
{
    if (MASK == NM_TEX_U8N) return mask_u8(static_cast<const unsigned char *>(m)[idx]);
    if (MASK == NM_TEX_F32) return mask_f32(static_cast<const float *>(m)[idx]);
    return true;
}

// the lanes' eight sums into the LDS table, per cell column of the wave's block (cx_lo .. cx_hi, wave-uniform)
__device__ __forceinline__ void wave_flush(unsigned (&c)[WORDS], int cx, int cx_lo, int cx_hi, int cy, int gx, u64 *s_tab)
{
    const int lane = threadIdx.x & 63;
    for (int cc = cx_lo; cc <= cx_hi; ++cc) {
        unsigned mine = 0;
#pragma unroll
        for (int q = 0; q < WORDS; ++q) {
            const unsigned t = nmw::wave_sum(cx == cc ? c[q] : 0u);
            if (lane == q) mine = t;
        }
        if (lane < WORDS && mine) atomicAdd(&s_tab[(cy * gx + cc) * WORDS + lane], (u64)mine);
    }
#pragma unroll
    for (int q = 0; q < WORDS; ++q) c[q] = 0;
}

// the workgroup's table into frame k's words of stats; the table is zero afterwards
__device__ __forceinline__ void table_flush(u64 *s_tab, u64 *__restrict__ stats, int k, int cells)
{
    __syncthreads();
    for (int i = threadIdx.x; i < cells * WORDS; i += THREADS) {
        const u64 v = s_tab[i];
        if (v) {
            atomicAdd(stats + (size_t)k * cells * WORDS + i, v);
            s_tab[i] = 0;
        }
    }
    __syncthreads();
}

// MASK: -1 no masks, else the masks' format
template <int MASK>
__global__ __launch_bounds__(THREADS) void frame_quality_kernel(const FqArgs a, int n, int fw, int fh, int lo, int hi, int gx,
                                                                int gy, u64 *__restrict__ stats, int strips)
{
    __shared__ u64 s_tab[MAX_CELLS * WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nblk = (fw + 63) >> 6, cells = gx * gy;
    const long long units = (long long)n * strips * nblk;
    for (int i = tid; i < MAX_CELLS * WORDS; i += THREADS) s_tab[i] = 0;
    __syncthreads();
    int cur = -1;                                                  // the frame the table counts for
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const int bx = (int)(u % nblk);
        const long long t = u / nblk;
        const int s = (int)(t % strips), k = (int)(t / strips);
        if (k != cur) {                                            // workgroup-uniform
            if (cur >= 0) table_flush(s_tab, stats, cur, cells);
            cur = k;
        }
        const int x0 = bx << 6, x = x0 + lane, y0 = s * STRIP + wave * WAVE_ROWS;
        const int rows = fh - y0 < WAVE_ROWS ? fh - y0 : WAVE_ROWS;
        if (rows <= 0) continue;                                   // wave-uniform; the loop holds no barrier of its own
        const bool in_x = x < fw, edge = lane == 0 || lane == 63;
        const int hx = lane == 0 ? x0 - 1 : x0 + 64;               // the halo column of the two edge lanes
        const bool in_h = edge && hx >= 0 && hx < fw;
        const int x_last = x0 + 63 < fw ? x0 + 63 : fw - 1;
        const int cx = in_x ? cell_of(x, gx, fw) : -1, cx_lo = cell_of(x0, gx, fw), cx_hi = cell_of(x_last, gx, fw);
        const uchar4 *__restrict__ f = a.frames[k];
        const void *__restrict__ m = a.masks[k];
        unsigned c[WORDS];
#pragma unroll
        for (int q = 0; q < WORDS; ++q) c[q] = 0;
        int cy = -1;                                               // the cell row the registers count for
        int pa = 0, pb = 0, pc = 0, hsb = 0, hdb = 0, hsc = 0, hdc = 0;     // rows above / at / below the centre
        const int slots = rows + 2;                                // slot i is row y0 - 1 + i
        for (int i0 = 0; i0 < slots; i0 += UNROLL) {
            uchar4 px[UNROLL], ph[UNROLL];
            bool el[UNROLL], eh[UNROLL];
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                const int y = y0 - 1 + i0 + j;
                const bool row = i0 + j < slots && y >= 0 && y < fh;
                px[j] = ph[j] = make_uchar4(0, 0, 0, 0);
                el[j] = row && in_x;
                eh[j] = row && in_h;
                if (el[j]) px[j] = f[(size_t)y * fw + x];
                if (eh[j]) ph[j] = f[(size_t)y * fw + hx];
                if (MASK >= 0) {
                    if (el[j]) el[j] = eligible_at<MASK>(m, (size_t)y * fw + x);
                    if (eh[j]) eh[j] = eligible_at<MASK>(m, (size_t)y * fw + hx);
                }
            }
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                const int i = i0 + j;
                if (i >= slots) break;                             // wave-uniform
                const int own = luma(px[j].x, px[j].y, px[j].z) | (classify(px[j].x, px[j].y, px[j].z, el[j], lo, hi) << 8);
                const int halo = luma(ph[j].x, ph[j].y, ph[j].z) | (classify(ph[j].x, ph[j].y, ph[j].z, eh[j], lo, hi) << 8);
                int left = __shfl_up(own, 1), right = __shfl_down(own, 1);
                if (lane == 0) left = halo;
                if (lane == 63) right = halo;
                pa = pb; pb = pc; hsb = hsc; hdb = hdc;
                pc = own | ((left & right & (GOOD << 8)) ? (HGOOD << 8) : 0);
                hsc = (left & 255) + (right & 255);
                hdc = (right & 255) - (left & 255);
                if (i < 2) continue;                               // the centre is slot i - 1, a row of the wave's own
                const int ycen = y0 + i - 2, cyc = cell_of(ycen, gy, fh);
                if (cyc != cy) {                                   // wave-uniform
                    if (cy >= 0) wave_flush(c, cx, cx_lo, cx_hi, cy, gx, s_tab);
                    cy = cyc;
                }
                const int bits = pb >> 8;
                if ((bits & GOOD) && (bits & HGOOD) && (pa & pc & (GOOD << 8))) {
                    const int Y = pb & 255;
                    unsigned L2, G2;
                    measure(pa & 255, Y, pc & 255, hsb, hdb, L2, G2);
                    c[0] += 1u; c[1] += (unsigned)Y; c[2] += (unsigned)(Y * Y); c[3] += L2; c[4] += G2;
                }
                c[5] += (bits & DARK) ? 1u : 0u;
                c[6] += (bits & BRIGHT) ? 1u : 0u;
                c[7] += (bits & ELIG) ? 1u : 0u;
            }
        }
        wave_flush(c, cx, cx_lo, cx_hi, cy, gx, s_tab);
    }
    if (cur >= 0) table_flush(s_tab, stats, cur, cells);
}

__global__ __launch_bounds__(THREADS) void keyframe_pick_kernel(const Pick p, const u64 *__restrict__ stats,
                                                                const float *__restrict__ chain,
                                                                const int *__restrict__ frame_status, int *__restrict__ keys,
                                                                int *__restrict__ key_count, int *__restrict__ key_status,
                                                                int *__restrict__ flags, double *__restrict__ scores,
                                                                float *__restrict__ H_keys, int *__restrict__ H_status)
{
    __shared__ float s_M[MAX_FRAMES][9];
    __shared__ double s_sc[MAX_FRAMES * 4];
    __shared__ int s_flags[MAX_FRAMES], s_nq[MAX_FRAMES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = p.n, cells = p.gx * p.gy;
    for (int q = tid; q < n * 9; q += THREADS) s_M[q / 9][q % 9] = chain[q];
    // a wave per frame, a lane per cell: the lower median of the qualifying cells by (value, cell index)
    for (int k = wave; k < n; k += WAVES) {
        const u64 *w = stats + ((size_t)k * cells + (lane < cells ? lane : 0)) * WORDS;
        const u64 m0 = w[0], m3 = w[3];
        const bool ok = lane < cells && cell_ok(m0, p.cell_min);
        const double sharp = ok ? sharp_of(m3, m0) : 0.0;
        const u64 okm = __ballot(ok);
        int rank = 0;
        for (int j = 0; j < cells; ++j) {
            const double vj = __shfl(sharp, j);
            if (((okm >> j) & 1ull) && before(vj, j, sharp, lane)) ++rank;
        }
        const int nq = __popcll(okm);
        const u64 sel = __ballot(ok && rank == (nq - 1) / 2);
        const double score = __shfl(sharp, sel ? __ffsll((long long)sel) - 1 : 0);
        if (lane == 0) {
            s_sc[4 * k] = score;
            s_nq[k] = nq;
        }
    }
    __syncthreads();
    // a lane per frame: totals, flags, then the blur window on the flags of all
    if (tid < n) {
        double sc[3];
        s_flags[tid] = frame_flags(p, stats + (size_t)tid * cells * WORDS, s_sc[4 * tid], s_nq[tid],
                                   frame_status ? frame_status[tid] : 1, s_M[tid], sc);
        s_sc[4 * tid] = sc[0]; s_sc[4 * tid + 1] = sc[1]; s_sc[4 * tid + 2] = sc[2];
    }
    __syncthreads();
    bool blur = false;
    if (tid < n) {
        double ref;
        blur = blurred(p, tid, s_flags, s_sc, ref);
        s_sc[4 * tid + 3] = ref;
    }
    __syncthreads();
    if (tid < n && blur) s_flags[tid] |= NM_KEYFRAME_BLURRED;
    __syncthreads();
    if (wave != 0) return;
    // the walk: lane j is frame j
    int fl = lane < n ? s_flags[lane] : 0;
    const bool use = lane < n && usable(fl);
    const double score = use ? s_sc[4 * lane] : -1.0;
    const u64 um = __ballot(use);
    int last = p.carry ? 0 : (um ? __ffsll((long long)um) - 1 : -1), jump = 0, count = 0, truncated = 0;
    int key = -1;                                                  // lane i holds keyframe i
    while (last >= 0) {                                            // every value here is wave-uniform
        if (count == p.keep) {
            truncated = 1;
            break;
        }
        if (lane == count) key = last;
        if (lane == last) fl |= NM_KEYFRAME_KEY | (jump ? NM_KEYFRAME_JUMP : 0);
        ++count;
        const bool after = use && lane > last;
        const float d = after ? motion(s_M[last], s_M[lane], p.fw, p.fh) : 0.f;
        const u64 beyond = __ballot(after && d > p.d_max);
        const int close = beyond ? __ffsll((long long)beyond) - 1 : 64;
        const bool cand = after && lane < close && d >= p.d_min;
        if (__ballot(cand)) {
            const double best = nmw::wave_max(cand ? score : -1.0);
            last = __ffsll((long long)__ballot(cand && score == best)) - 1;
            jump = 0;
        } else {
            last = close < 64 ? close : -1;
            jump = 1;
        }
    }
    if (lane < p.keep) {
        keys[lane] = key;
        if (key_status) key_status[lane] = key >= 0 ? 1 : 0;
    }
    if (lane == 0) {
        key_count[0] = count;
        key_count[1] = truncated;
    }
    if (lane < n) {
        if (flags) flags[lane] = fl;
        if (scores)
            for (int q = 0; q < 4; ++q) scores[4 * lane + q] = s_sc[4 * lane + q];
    }
    const int next = __shfl_down(key, 1);
    if (lane < p.keep - 1 && (H_keys || H_status)) {
        float H[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const bool ok = lane + 1 < count && key_map(s_M[key], s_M[next], H);
        if (H_keys)
            for (int q = 0; q < 9; ++q) H_keys[9 * lane + q] = H[q];
        if (H_status) H_status[lane] = ok ? 1 : 0;
    }
}

// WIDE: 16-byte words (every pointer and bytes are multiples of 16), else bytes
template <bool WIDE>
__global__ __launch_bounds__(THREADS) void slots_gather_kernel(const GatherArgs a, int n, int keep, const int *__restrict__ keys,
                                                               long long bytes, int fill, long long chunks)
{
    const long long units = (long long)keep * chunks;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const int i = (int)(u / chunks);
        const long long b0 = (u % chunks) * GATHER_CHUNK;
        const long long b1 = b0 + GATHER_CHUNK < bytes ? b0 + GATHER_CHUNK : bytes;
        const int key = __builtin_amdgcn_readfirstlane(keys[i]);
        const bool have = key >= 0 && key < n;
        const void *src = a.src[have ? key : 0];
        if (WIDE) {
            const unsigned f4 = (unsigned)(fill & 255) * 0x01010101u;
            const uint4 *s = static_cast<const uint4 *>(src);
            uint4 *d = static_cast<uint4 *>(a.dst[i]);
            for (long long q = (b0 >> 4) + threadIdx.x; q < (b1 >> 4); q += THREADS) d[q] = have ? s[q] : make_uint4(f4, f4, f4, f4);
        } else {
            const unsigned char *s = static_cast<const unsigned char *>(src);
            unsigned char *d = static_cast<unsigned char *>(a.dst[i]);
            for (long long q = b0 + threadIdx.x; q < b1; q += THREADS) d[q] = have ? s[q] : (unsigned char)fill;
        }
    }
}

bool quality_ok(int n, const unsigned char *const *frames, int fw, int fh, const void *const *masks, int mask_format, int lo,
                int hi, int gx, int gy, const u64 *stats)
{
    if (n < 1 || n > MAX_FRAMES || !nm_size_ok(fw) || !nm_size_ok(fh) || lo < 0 || lo > 255 || hi < 0 || hi > 255 || gx < 1 ||
        gx > (fw < MAX_GRID ? fw : MAX_GRID) || gy < 1 || gy > (fh < MAX_GRID ? fh : MAX_GRID) ||
        (masks && mask_format != NM_TEX_U8N && mask_format != NM_TEX_F32))
        return false;
    return nmp::tables_ok(n, {frames}, {masks}, {stats});
}

Pick pick_of(int n, int gx, int gy, int fw, int fh, int keep, long long cell_min, long long min_pixels, double max_bad,
             double rel, int w, float d_min, float d_max, int carry)
{
    Pick p;
    p.n = n; p.fw = fw; p.fh = fh; p.keep = keep; p.gx = gx; p.gy = gy; p.w = w; p.carry = carry ? 1 : 0;
    p.cell_min = cell_min; p.min_pixels = min_pixels; p.max_bad = max_bad; p.rel = rel; p.d_min = d_min; p.d_max = d_max;
    return p;
}

bool gather_ok(int n, const void *const *src, int keep, void *const *dst, const int *keys, long long bytes)
{
    if (n < 1 || n > MAX_FRAMES || keep < 1 || keep > MAX_FRAMES || bytes < 1 || bytes >= (1ll << 31) || !src || !dst || !keys)
        return false;
    return nmp::tables_ok(n, {src}, {}, {}) && nmp::tables_ok(keep, {dst}, {}, {});
}

int grid_of(long long units)
{
    const int cap = g_grid_cap.load();                 // nm_frame_quality_set_grid_cap: tests make small grids walk far
    return cap > 0 ? (int)(units < cap ? units : cap) : nm_fill_grid(units, BLOCKS_PER_CU);
}

}  // namespace

extern "C" {

int nm_frame_quality_set_grid_cap(int cap) { return g_grid_cap.exchange(cap < 1 ? 0 : cap); }

int nm_frame_quality_batch_dev(int n, const unsigned char *const *frames, int fw, int fh, const void *const *masks,
                               int mask_format, int lo, int hi, int gx, int gy, unsigned long long *stats, void *stream)
{
    if (!quality_ok(n, frames, fw, fh, masks, mask_format, lo, hi, gx, gy, stats)) return (int)hipErrorInvalidValue;
    FqArgs a;
    nmp::fill_slots_as(a.frames, frames, 0, n);
    nmp::fill_slots(a.masks, masks, 0, n);
    const hipStream_t st = nm_stream(stream);
    NM_RETURN_IF(nmp::launch_zero_u64(stats, (size_t)n * gx * gy * WORDS, st));
    const int strips = nm_divup(fh, STRIP);
    const auto kernel = !masks ? frame_quality_kernel<-1>
                               : (mask_format == NM_TEX_F32 ? frame_quality_kernel<NM_TEX_F32> : frame_quality_kernel<NM_TEX_U8N>);
    hipLaunchKernelGGL(kernel, dim3(grid_of((long long)n * strips * nm_divup(fw, 64))), dim3(THREADS), 0, st, a, n, fw, fh, lo, hi,
                       gx, gy, stats, strips);
    NM_LAUNCH_CHECK();
    return 0;
}

int nm_frame_quality_host(int n, const unsigned char *const *frames, int fw, int fh, const void *const *masks, int mask_format,
                          int lo, int hi, int gx, int gy, unsigned long long *stats)
{
    if (!quality_ok(n, frames, fw, fh, masks, mask_format, lo, hi, gx, gy, stats)) return (int)hipErrorInvalidValue;
    std::vector<int> pk((size_t)fw * fh);                          // luminance | class bits << 8
    for (int k = 0; k < n; ++k) {
        u64 *out = stats + (size_t)k * gx * gy * WORDS;
        std::fill(out, out + (size_t)gx * gy * WORDS, 0ull);
        const unsigned char *f = frames[k];
        for (int y = 0; y < fh; ++y)
            for (int x = 0; x < fw; ++x) {
                const size_t idx = (size_t)y * fw + x;
                const unsigned char *q = f + 4 * idx;
                bool elig = true;
                if (masks)
                    elig = mask_format == NM_TEX_F32 ? mask_f32(static_cast<const float *>(masks[k])[idx])
                                                     : mask_u8(static_cast<const unsigned char *>(masks[k])[idx]);
                pk[idx] = luma(q[0], q[1], q[2]) | (classify(q[0], q[1], q[2], elig, lo, hi) << 8);
            }
        for (int y = 0; y < fh; ++y)
            for (int x = 0; x < fw; ++x) {
                const size_t idx = (size_t)y * fw + x;
                u64 *w = out + (size_t)(cell_of(y, gy, fh) * gx + cell_of(x, gx, fw)) * WORDS;
                const int bits = pk[idx] >> 8;
                w[5] += (bits & DARK) ? 1 : 0; w[6] += (bits & BRIGHT) ? 1 : 0; w[7] += (bits & ELIG) ? 1 : 0;
                if (x < 1 || y < 1 || x + 1 >= fw || y + 1 >= fh) continue;
                const int l = pk[idx - 1], r = pk[idx + 1], a = pk[idx - fw], b = pk[idx + fw];
                if (!(pk[idx] & l & r & a & b & (GOOD << 8))) continue;
                const int Y = pk[idx] & 255;
                unsigned L2, G2;
                measure(a & 255, Y, b & 255, (l & 255) + (r & 255), (r & 255) - (l & 255), L2, G2);
                w[0] += 1; w[1] += (u64)Y; w[2] += (u64)(Y * Y); w[3] += L2; w[4] += G2;
            }
    }
    return 0;
}

int nm_keyframe_pick_dev(int n, const unsigned long long *stats, int gx, int gy, const float *chain, const int *frame_status,
                         int fw, int fh, int keep, long long cell_min, long long min_pixels, double max_bad, double rel, int w,
                         float d_min, float d_max, int carry, int *keys, int *key_count, int *key_status, int *flags,
                         double *scores, float *H_keys, int *H_status, void *stream)
{
    const Pick p = pick_of(n, gx, gy, fw, fh, keep, cell_min, min_pixels, max_bad, rel, w, d_min, d_max, carry);
    if (!pick_ok(p) || !stats || !chain || !keys || !key_count) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(keyframe_pick_kernel, dim3(1), dim3(THREADS), 0, nm_stream(stream), p, stats, chain, frame_status, keys,
                       key_count, key_status, flags, scores, H_keys, H_status);
    NM_LAUNCH_CHECK();
    return 0;
}

int nm_keyframe_pick_host(int n, const unsigned long long *stats, int gx, int gy, const float *chain, const int *frame_status,
                          int fw, int fh, int keep, long long cell_min, long long min_pixels, double max_bad, double rel, int w,
                          float d_min, float d_max, int carry, int *keys, int *key_count, int *key_status, int *flags,
                          double *scores, float *H_keys, int *H_status)
{
    const Pick p = pick_of(n, gx, gy, fw, fh, keep, cell_min, min_pixels, max_bad, rel, w, d_min, d_max, carry);
    if (!pick_ok(p) || !stats || !chain || !keys || !key_count) return (int)hipErrorInvalidValue;
    const int cells = gx * gy;
    int fl[MAX_FRAMES], pre[MAX_FRAMES];
    double sc[MAX_FRAMES * 4];
    for (int k = 0; k < n; ++k) {
        const u64 *cw = stats + (size_t)k * cells * WORDS;
        int nq = 0;
        for (int c = 0; c < cells; ++c) nq += cell_ok(cw[c * WORDS], cell_min) ? 1 : 0;
        double score = 0.0;
        for (int c = 0; c < cells; ++c) {
            if (!cell_ok(cw[c * WORDS], cell_min)) continue;
            const double v = sharp_of(cw[c * WORDS + 3], cw[c * WORDS]);
            int rank = 0;
            for (int j = 0; j < cells; ++j)
                if (cell_ok(cw[j * WORDS], cell_min) && before(sharp_of(cw[j * WORDS + 3], cw[j * WORDS]), j, v, c)) ++rank;
            if (rank == (nq - 1) / 2) score = v;
        }
        pre[k] = frame_flags(p, cw, score, nq, frame_status ? frame_status[k] : 1, chain + 9 * k, sc + 4 * k);
    }
    for (int k = 0; k < n; ++k) fl[k] = pre[k] | (blurred(p, k, pre, sc, sc[4 * k + 3]) ? NM_KEYFRAME_BLURRED : 0);
    int first = -1;
    for (int k = n - 1; k >= 0; --k)
        if (usable(fl[k])) first = k;
    int sel[MAX_FRAMES];
    int last = carry ? 0 : first, jump = 0, count = 0, truncated = 0;
    while (last >= 0) {
        if (count == keep) {
            truncated = 1;
            break;
        }
        sel[count++] = last;
        fl[last] |= NM_KEYFRAME_KEY | (jump ? NM_KEYFRAME_JUMP : 0);
        int close = -1, best = -1;
        for (int j = last + 1; j < n && close < 0; ++j) {
            if (!usable(fl[j])) continue;
            const float d = motion(chain + 9 * last, chain + 9 * j, fw, fh);
            if (d > d_max) close = j;
            else if (d >= d_min && (best < 0 || sc[4 * j] > sc[4 * best])) best = j;
        }
        jump = best < 0;
        last = best >= 0 ? best : close;
    }
    for (int i = 0; i < keep; ++i) {
        keys[i] = i < count ? sel[i] : -1;
        if (key_status) key_status[i] = i < count ? 1 : 0;
    }
    key_count[0] = count;
    key_count[1] = truncated;
    for (int k = 0; k < n; ++k) {
        if (flags) flags[k] = fl[k];
        if (scores)
            for (int q = 0; q < 4; ++q) scores[4 * k + q] = sc[4 * k + q];
    }
    for (int i = 0; i + 1 < keep; ++i) {
        float H[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const bool ok = i + 1 < count && key_map(chain + 9 * sel[i], chain + 9 * sel[i + 1], H);
        if (H_keys)
            for (int q = 0; q < 9; ++q) H_keys[9 * i + q] = H[q];
        if (H_status) H_status[i] = ok ? 1 : 0;
    }
    return 0;
}

int nm_slots_gather_dev(int n, const void *const *src, int keep, void *const *dst, const int *keys, long long bytes, int fill,
                        void *stream)
{
    if (!gather_ok(n, src, keep, dst, keys, bytes)) return (int)hipErrorInvalidValue;
    GatherArgs a;
    nmp::fill_slots(a.src, src, 0, n);
    nmp::fill_slots(a.dst, dst, 0, keep);
    size_t low = (size_t)bytes;
    for (int k = 0; k < n; ++k) low |= reinterpret_cast<size_t>(src[k]);
    for (int i = 0; i < keep; ++i) low |= reinterpret_cast<size_t>(dst[i]);
    const long long chunks = (bytes + GATHER_CHUNK - 1) / GATHER_CHUNK;
    const auto kernel = (low & 15) ? slots_gather_kernel<false> : slots_gather_kernel<true>;
    hipLaunchKernelGGL(kernel, dim3(nm_fill_grid((long long)keep * chunks, BLOCKS_PER_CU)), dim3(THREADS), 0, nm_stream(stream), a,
                       n, keep, keys, bytes, fill, chunks);
    NM_LAUNCH_CHECK();
    return 0;
}

int nm_slots_gather_host(int n, const void *const *src, int keep, void *const *dst, const int *keys, long long bytes, int fill)
{
    if (!gather_ok(n, src, keep, dst, keys, bytes)) return (int)hipErrorInvalidValue;
    for (int i = 0; i < keep; ++i) {
        if (keys[i] >= 0 && keys[i] < n) std::memcpy(dst[i], src[keys[i]], (size_t)bytes);
        else std::memset(dst[i], fill & 255, (size_t)bytes);
    }
    return 0;
}

}  // extern "C"
