// nm_klt_corners.hip -- Shi-Tomasi ("good features to track") corners of up to NM_KLT_MAX_BATCH gray planes, for gfx950
// (include/nm_abi.h, "Corner detection", has the written semantics). No reference counterpart. The score is the tracker's
// own level-0 texture gate at integer pixel centres, so the corners are points the tracker does not call FLAT or BORDER. On
// the caller's stream, no allocation, no synchronisation, no host read; no workgroup waits for another; nothing is zeroed
// by a separate launch (every word that is read is written by the call first). THREE launches whatever n is, FOUR with held
// points:
//   response  a workgroup of four waves takes a unit = (frame, tile of 64 x 16 pixels), grid-stride over the units. The
//             tile's pixels and a halo (12 columns either side, r + 1 rows above, r + 2 below) go to LDS as 16-bit levels
//             (16-byte loads where the width is a multiple of 4 and every plane is 16-byte aligned, scalars at the plane's
//             edge and otherwise; bit 15 marks a pixel without a level). gx, gy are formed once per pixel and packed into one
//             word; the box sum runs separably through LDS: a row pass of the three products (a row of 15 stays below 2^31),
//             then a column pass in which a lane walks down four rows with running sums (Gxx, Gyy in unsigned 32-bit words,
//             Gxy in 64 bits). "Has a window" comes from one 88-bit word of no-level bits per tile row (two ballots), OR-ed
//             over the window's rows by the wave and tested by a lane with two shifts. One fp64 gate per pixel, one fp32 store
//             to the score plane. With held points the unit also zeroes its part of the frame's mark plane.
//   mark      (held points only) a thread per held row: one byte store of 1 at the row's pixel into the mark plane, which
//             has a border of 16 pixels so that rows outside the frame still count. Equal values race harmlessly.
//   nms       a unit = (frame, tile of 64 x 16 pixels): the scores of the tile and a halo of nms go to LDS as 64-bit keys
//             (score bits above the complement of the raster ordinal: the larger key wins, the tie rule included); the
//             window maximum runs separably (rows, then columns); a pixel is a corner when it is scored and its key is the
//             maximum. For each of the few candidates the wave reads the (2 nms + 1)^2 marks round it together. One ballot per tile row is
//             stored: word (y, x / 64) of the frame's flag plane, every word written.
//   emit      a workgroup per frame walks the flag words in raster order, 1024 words a trip: population counts, one
//             workgroup scan (nmw::wave_inclusive_scan and four wave totals in LDS), a running base; a thread writes the
//             corners of its four words at their ranks while rank < cap. count and total at the end. The order comes from
//             the scan alone, never from an atomic.
// The arithmetic is nm_klt_corners_math.hpp, shared with the host twin below: both agree bit for bit.
#include <atomic>
#include <vector>

#include "../../include/nm_abi.h"
#include "nm_common.hpp"
#include "nm_klt_corners_math.hpp"
#include "nm_pair_batch.hpp"

namespace {

using namespace nmkc;

constexpr int THREADS = 256, WAVES = 4, BLOCKS_PER_CU = 8;
constexpr int TX = 64, TY = 16;                                        // a tile of either tiled pass; TX is the wave
constexpr int ROWS_PER_WAVE = TY / WAVES;
constexpr int HL = 12;                                                 // columns loaded either side: >= MAX_RADIUS + 2, a multiple of 4
constexpr int QW = TX + 2 * HL, QH = TY + 2 * nmk::MAX_RADIUS + 3;     // the level tile
constexpr int GW = TX + 2 * nmk::MAX_RADIUS, GH = TY + 2 * nmk::MAX_RADIUS;   // the gradient tile
constexpr int PAD = MAX_NMS;                                           // the mark plane's border
constexpr int EMIT_WORDS = 4;                                          // flag words per thread and trip
constexpr size_t WS_ALIGN = 64;
static_assert(HL >= nmk::MAX_RADIUS + 2 && HL % 4 == 0 && QW % 4 == 0 && QW <= 128, "the level tile");
static_assert(TX == 64 && TY % WAVES == 0, "a tile row is one wave and one flag word");

std::atomic<int> g_grid_cap{0};                                        // nm_klt_corners_set_grid_cap; 0: the default

struct PlaneArgs {                                                     // 1 KB of the 4 KB of kernel arguments
    const float *gray[nmp::MAX_BATCH];
    float *plane[nmp::MAX_BATCH];
};
struct HeldArgs {                                                      // 1.5 KB
    const float *hx[nmp::MAX_BATCH], *hy[nmp::MAX_BATCH];
    const int *d_held[nmp::MAX_BATCH];
};
struct EmitArgs {                                                      // 2 KB
    const float *plane[nmp::MAX_BATCH];
    float *x[nmp::MAX_BATCH], *y[nmp::MAX_BATCH], *score[nmp::MAX_BATCH];
};
struct ScoreArgs { const float *plane[nmp::MAX_BATCH]; };
static_assert(sizeof(EmitArgs) + 128 < 4096, "kernel arguments exceed 4 KB");

// the parts of the workspace, for n frames of fw x fh
struct Layout {
    int wpr;                                                           // flag words (tiles) per row
    size_t mark_pitch, mark_plane;                                     // bytes per row and per frame of the mark planes
    size_t scores, flags, marks, total;                                // byte offsets, and the size
};
__host__ __device__ __forceinline__ int words_per_row(int fw) { return (fw + TX - 1) / TX; }
Layout layout_of(int n, int fw, int fh)
{
    Layout L;
    L.wpr = words_per_row(fw);
    L.mark_pitch = (size_t)L.wpr * TX + 2 * PAD;
    L.mark_plane = L.mark_pitch * (size_t)(fh + 2 * PAD);
    L.scores = 0;
    L.flags = (((size_t)n * fw * fh * sizeof(float)) + WS_ALIGN - 1) & ~(WS_ALIGN - 1);
    L.marks = L.flags + (size_t)n * fh * L.wpr * sizeof(u64);
    L.marks = (L.marks + WS_ALIGN - 1) & ~(WS_ALIGN - 1);
    L.total = L.marks + (size_t)n * L.mark_plane + WS_ALIGN;
    return L;
}

int grid_of(long long units)
{
    const int cap = g_grid_cap.load();                 // nm_klt_corners_set_grid_cap: tests make small grids walk far
    return cap > 0 ? (int)(units < cap ? units : cap) : nm_fill_grid(units, BLOCKS_PER_CU);
}

// bits [lo, lo + len) of the 128-bit word (m1 : m0) hold a set bit; 1 <= lo, lo + len <= 128, len <= 32
__device__ __forceinline__ bool any_bit(u64 m0, u64 m1, int lo, int len)
{
    const u64 v = lo < 64 ? ((m0 >> lo) | (m1 << (64 - lo))) : (m1 >> (lo - 64));
    return (v & ((1ull << len) - 1ull)) != 0ull;
}

// WIDE: 16-byte loads of the planes (and 4-byte loads of the mask) where a group of four pixels lies inside a row
template <bool WIDE>
__global__ __launch_bounds__(THREADS) void corners_response_kernel(const PlaneArgs a, int n, int fw, int fh,
                                                                   const unsigned char *__restrict__ mask, int r,
                                                                   double min_eig, unsigned char *__restrict__ marks,
                                                                   size_t mark_pitch, size_t mark_plane)
{
    __shared__ __attribute__((aligned(16))) unsigned short s_q[QH][QW];      // row y0 - (r + 1) + i, column x0 - HL + j
    __shared__ unsigned s_g[GH][GW];                                         // gx | gy << 16 of row y0 - r + i, column x0 - r + j
    __shared__ int s_rxx[GH][TX], s_rxy[GH][TX], s_ryy[GH][TX];              // the row sums of row y0 - r + i, column x0 + j
    __shared__ u64 s_bad[QH][2];                                             // the no-level bits of a row of s_q
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tx = words_per_row(fw), ty = (fh + TY - 1) / TY;
    const int qrows = TY + 2 * r + 3, grows = TY + 2 * r, gcols = TX + 2 * r;
    const long long units = (long long)n * tx * ty;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const int bx = (int)(u % tx);
        const long long t = u / tx;
        const int by = (int)(t % ty), k = (int)(t / ty);
        const int x0 = bx * TX, y0 = by * TY;
        const float *__restrict__ src = a.gray[k];
        __syncthreads();                                           // the previous unit's tiles are read out
        // the levels
        for (int i = tid; i < qrows * (QW / 4); i += THREADS) {
            const int ry = i / (QW / 4), c4 = i - ry * (QW / 4);
            const int y = y0 - (r + 1) + ry, x = x0 - HL + 4 * c4;
            unsigned short q[4] = {NO_LEVEL, NO_LEVEL, NO_LEVEL, NO_LEVEL};
            if (y >= 0 && y < fh) {
                const size_t o = (size_t)y * fw + x;               // not used as an address where x < 0
                if (WIDE && x >= 0 && x + 3 < fw) {
                    const float4 v = *reinterpret_cast<const float4 *>(src + o);
                    unsigned m = 0x01010101u;
                    if (mask) m = *reinterpret_cast<const unsigned *>(mask + o);
                    q[0] = (unsigned short)level16(v.x, (m & 0xFFu) != 0u);
                    q[1] = (unsigned short)level16(v.y, (m & 0xFF00u) != 0u);
                    q[2] = (unsigned short)level16(v.z, (m & 0xFF0000u) != 0u);
                    q[3] = (unsigned short)level16(v.w, (m & 0xFF000000u) != 0u);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (x + j >= 0 && x + j < fw)
                            q[j] = (unsigned short)level16(src[(size_t)y * fw + (x + j)], !mask || mask[(size_t)y * fw + (x + j)] != 0);
                }
            }
            uint2 w;
            w.x = (unsigned)q[0] | ((unsigned)q[1] << 16);
            w.y = (unsigned)q[2] | ((unsigned)q[3] << 16);
            *reinterpret_cast<uint2 *>(&s_q[ry][4 * c4]) = w;
        }
        if (marks) {                                               // this tile's part of the mark plane, border included
            const int cx0 = bx == 0 ? 0 : x0 + PAD, cx1 = bx == tx - 1 ? (int)mark_pitch : x0 + TX + PAD;
            const int cy0 = by == 0 ? 0 : y0 + PAD, cy1 = by == ty - 1 ? fh + 2 * PAD : y0 + TY + PAD;
            const int c16 = (cx1 - cx0) >> 4;                      // cx0, cx1 and the pitch are multiples of 16
            unsigned char *mk = marks + (size_t)k * mark_plane;
            for (int i = tid; i < (cy1 - cy0) * c16; i += THREADS) {
                const int ry = i / c16, c = i - ry * c16;
                *reinterpret_cast<uint4 *>(mk + (size_t)(cy0 + ry) * mark_pitch + cx0 + 16 * c) = make_uint4(0u, 0u, 0u, 0u);
            }
        }
        __syncthreads();
        // the no-level bits of every row, and the gradients
        for (int ry = wave; ry < qrows; ry += WAVES) {
            const u64 m0 = __ballot((s_q[ry][lane] & NO_LEVEL) != 0);
            const u64 m1 = __ballot(lane < QW - 64 && (s_q[ry][lane < QW - 64 ? 64 + lane : 0] & NO_LEVEL) != 0);
            if (lane == 0) { s_bad[ry][0] = m0; s_bad[ry][1] = m1; }
        }
        for (int i = tid; i < grows * gcols; i += THREADS) {
            const int gy_i = i / gcols, gx_i = i - gy_i * gcols;
            const int ry = gy_i + 1, cx = gx_i + HL - r;
            const int gx = (int)(s_q[ry][cx + 1] & LEVEL_BITS) - (int)(s_q[ry][cx - 1] & LEVEL_BITS);
            const int gy = (int)(s_q[ry + 1][cx] & LEVEL_BITS) - (int)(s_q[ry - 1][cx] & LEVEL_BITS);
            s_g[gy_i][gx_i] = ((unsigned)gx & 0xFFFFu) | ((unsigned)gy << 16);
        }
        __syncthreads();
        // the row sums of the three products
        for (int i = tid; i < grows * TX; i += THREADS) {
            const int gy_i = i >> 6, X = i & 63;
            int sxx = 0, sxy = 0, syy = 0;
            for (int tap = 0; tap <= 2 * r; ++tap) {
                const unsigned g = s_g[gy_i][X + tap];
                const int gx = (int)(short)(g & 0xFFFFu), gy = (int)(short)(g >> 16);
                sxx += gx * gx; sxy += gx * gy; syy += gy * gy;
            }
            s_rxx[gy_i][X] = sxx; s_rxy[gy_i][X] = sxy; s_ryy[gy_i][X] = syy;
        }
        __syncthreads();
        // the column sums, the gate and the store: a wave takes ROWS_PER_WAVE rows, a lane walks down a column
        {
            const int Y_first = wave * ROWS_PER_WAVE, x = x0 + lane;
            unsigned Gxx = 0, Gyy = 0;
            i64 Gxy = 0;
            for (int tap = 0; tap <= 2 * r; ++tap) {
                Gxx += (unsigned)s_rxx[Y_first + tap][lane]; Gxy += (i64)s_rxy[Y_first + tap][lane];
                Gyy += (unsigned)s_ryy[Y_first + tap][lane];
            }
            float *__restrict__ out = a.plane[k];
            for (int j = 0; j < ROWS_PER_WAVE; ++j) {
                const int Y = Y_first + j, y = y0 + Y;
                if (j > 0) {
                    Gxx += (unsigned)s_rxx[Y + 2 * r][lane] - (unsigned)s_rxx[Y - 1][lane];
                    Gxy += (i64)s_rxy[Y + 2 * r][lane] - (i64)s_rxy[Y - 1][lane];
                    Gyy += (unsigned)s_ryy[Y + 2 * r][lane] - (unsigned)s_ryy[Y - 1][lane];
                }
                if (y >= fh) break;                                // wave-uniform
                u64 m0 = 0, m1 = 0;                                // rows Y .. Y + 2r + 3 of s_q are the window's
                for (int v = 0; v < 2 * r + 4; ++v) { m0 |= s_bad[Y + v][0]; m1 |= s_bad[Y + v][1]; }
                const bool has = !any_bit(m0, m1, lane + HL - (r + 1), 2 * r + 4);
                const float s = has ? score_of((i64)Gxx, Gxy, (i64)Gyy, r, min_eig) : -1.f;
                if (x < fw) out[(size_t)y * fw + x] = s;
            }
        }
    }
}

__global__ __launch_bounds__(THREADS) void corners_mark_kernel(const HeldArgs h, int n, int cap_held, int fw, int fh,
                                                               unsigned char *__restrict__ marks, size_t mark_pitch,
                                                               size_t mark_plane)
{
    const long long rows = (long long)n * cap_held;
    for (long long g = (long long)blockIdx.x * THREADS + threadIdx.x; g < rows; g += (long long)gridDim.x * THREADS) {
        const int k = (int)(g / cap_held), i = (int)(g - (long long)k * cap_held);
        if (i >= nmp::clip(*h.d_held[k], cap_held)) continue;
        int px, py;
        if (held_pixel(h.hx[k][i], h.hy[k][i], fw, fh, px, py))
            marks[(size_t)k * mark_plane + (size_t)(py + PAD) * mark_pitch + (size_t)(px + PAD)] = 1;
    }
}

__global__ __launch_bounds__(THREADS) void corners_nms_kernel(const ScoreArgs a, int n, int fw, int fh, int nms,
                                                              const unsigned char *__restrict__ marks, size_t mark_pitch,
                                                              size_t mark_plane, u64 *__restrict__ flags)
{
    extern __shared__ __attribute__((aligned(16))) u64 s_dyn[];
    const int pw = TX + 2 * nms, ph = TY + 2 * nms;
    u64 *s_key = s_dyn;                                            // [ph][pw]: row y0 - nms + i, column x0 - nms + j
    u64 *s_row = s_dyn + (size_t)ph * pw;                          // [ph][TX]: the row maxima
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tx = words_per_row(fw), ty = (fh + TY - 1) / TY;
    const long long units = (long long)n * tx * ty;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const int bx = (int)(u % tx);
        const long long t = u / tx;
        const int by = (int)(t % ty), k = (int)(t / ty);
        const int x0 = bx * TX, y0 = by * TY;
        const float *__restrict__ plane = a.plane[k];
        __syncthreads();                                           // the previous unit's tiles are read out
        for (int i = tid; i < ph * pw; i += THREADS) {
            const int ly = i / pw, lx = i - ly * pw;
            const int y = y0 - nms + ly, x = x0 - nms + lx;
            float s = -1.f;
            if (y >= 0 && y < fh && x >= 0 && x < fw) s = plane[(size_t)y * fw + x];
            s_key[i] = nms_key(s, (unsigned)i);
        }
        __syncthreads();
        for (int i = tid; i < ph * TX; i += THREADS) {
            const int ly = i >> 6, X = i & 63;
            const u64 *row = s_key + (size_t)ly * pw + X;
            u64 m = 0;
            for (int tap = 0; tap <= 2 * nms; ++tap) m = row[tap] > m ? row[tap] : m;
            s_row[i] = m;
        }
        __syncthreads();
        for (int j = 0; j < ROWS_PER_WAVE; ++j) {
            const int Y = wave * ROWS_PER_WAVE + j, y = y0 + Y, x = x0 + lane;
            if (y >= fh) break;                                    // wave-uniform
            u64 m = 0;
            for (int tap = 0; tap <= 2 * nms; ++tap) {
                const u64 v = s_row[(size_t)(Y + tap) * TX + lane];
                m = v > m ? v : m;
            }
            const u64 own = s_key[(size_t)(Y + nms) * pw + (lane + nms)];
            u64 word = __ballot(own != 0ull && own == m && x < fw);    // wave-uniform
            if (marks) {                                           // a held row within nms of a candidate: the wave reads the
                const int side = 2 * nms + 1, cells = side * side;  // candidate's (2 nms + 1)^2 marks together, 64 a trip
                const unsigned char *row = marks + (size_t)k * mark_plane + (size_t)(y + PAD - nms) * mark_pitch + (x0 + PAD - nms);
                u64 held = 0;
                for (u64 c = word; c != 0ull; c &= c - 1ull) {
                    const int l = __builtin_ctzll(c);
                    bool any = false;
                    for (int i = lane; i < cells; i += 64) {
                        const int dy = i / side, dx = i - dy * side;
                        any = any || row[(size_t)dy * mark_pitch + (l + dx)] != 0;
                    }
                    if (__ballot(any) != 0ull) held |= 1ull << l;
                }
                word &= ~held;
            }
            if (lane == 0) flags[((size_t)k * fh + y) * tx + bx] = word;
        }
    }
}

__global__ __launch_bounds__(THREADS) void corners_emit_kernel(const EmitArgs a, int n, int fw, int fh, int cap,
                                                               const u64 *__restrict__ flags, int *__restrict__ d_count,
                                                               int *__restrict__ d_total)
{
    __shared__ int s_tot[2][WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wpr = words_per_row(fw);
    const long long words = (long long)fh * wpr;
    for (int k = blockIdx.x; k < n; k += gridDim.x) {
        const u64 *__restrict__ f = flags + (size_t)k * words;
        const float *__restrict__ plane = a.plane[k];
        float *__restrict__ ox = a.x[k], *__restrict__ oy = a.y[k], *__restrict__ os = a.score[k];
        int base = 0, parity = 0;                                  // workgroup-uniform
        __syncthreads();                                           // the previous frame's totals are read out
        for (long long first = 0; first < words; first += (long long)THREADS * EMIT_WORDS, parity ^= 1) {
            u64 w[EMIT_WORDS];
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < EMIT_WORDS; ++j) {
                const long long idx = first + (long long)tid * EMIT_WORDS + j;
                w[j] = idx < words ? f[idx] : 0ull;
                cnt += __popcll(w[j]);
            }
            const int incl = nmw::wave_inclusive_scan(cnt);
            if (lane == 63) s_tot[parity][wave] = incl;
            __syncthreads();
            int before = 0, total = 0;
#pragma unroll
            for (int q = 0; q < WAVES; ++q) {
                const int c = s_tot[parity][q];
                if (q < wave) before += c;
                total += c;
            }
            int pos = base + before + incl - cnt;
#pragma unroll
            for (int j = 0; j < EMIT_WORDS; ++j) {
                const long long idx = first + (long long)tid * EMIT_WORDS + j;
                const int y = (int)(idx / wpr), xw = (int)(idx - (long long)y * wpr) * TX;
                for (u64 m = w[j]; m != 0ull && pos < cap; m &= m - 1ull, ++pos) {
                    const int x = xw + __builtin_ctzll(m);
                    ox[pos] = (float)x; oy[pos] = (float)y; os[pos] = plane[(size_t)y * fw + x];
                }
            }
            base += total;
        }
        if (tid == 0) {
            d_count[k] = base < cap ? base : cap;
            if (d_total) d_total[k] = base;
        }
    }
}

bool args_ok(int n, const float *const *gray, int fw, int fh, const float *const *held_x, const float *const *held_y,
             const int *const *d_held, int cap_held, int radius, int nms, float min_eig, int cap, float *const *x,
             float *const *y, float *const *score, const int *d_count, float *const *score_plane)
{
    if (!params_ok(n, fw, fh, radius, nms, min_eig, cap)) return false;
    const int given = (held_x != nullptr) + (held_y != nullptr) + (d_held != nullptr);
    if (given != 0 && given != 3) return false;
    if (given == 3 && !nmp::cap_ok(cap_held)) return false;
    return nmp::tables_ok(n, {gray, x, y, score}, {held_x, held_y, d_held, score_plane}, {d_count});
}

// the host twin of one frame
void corners_host_frame(const float *gray, int fw, int fh, const unsigned char *mask, const float *hx, const float *hy, int nH,
                        int r, int nms, double min_eig, int cap, float *ox, float *oy, float *os, int *count, int *total,
                        float *plane_out)
{
    const size_t px = (size_t)fw * fh;
    std::vector<int> q(px);                                        // the level, -1: none
    for (size_t p = 0; p < px; ++p) {
        const int v = level16(gray[p], !mask || mask[p] != 0);
        q[p] = v == NO_LEVEL ? -1 : v;
    }
    std::vector<float> own;
    if (!plane_out) { own.resize(px); plane_out = own.data(); }
    for (int y = 0; y < fh; ++y)
        for (int x = 0; x < fw; ++x) {
            bool has = x - (r + 1) >= 0 && x + r + 2 < fw && y - (r + 1) >= 0 && y + r + 2 < fh;
            for (int v = -(r + 1); has && v <= r + 2; ++v)
                for (int u = -(r + 1); u <= r + 2; ++u) has = has && q[(size_t)(y + v) * fw + (x + u)] >= 0;
            float s = -1.f;
            if (has) {
                i64 Gxx = 0, Gxy = 0, Gyy = 0;
                for (int v = -r; v <= r; ++v)
                    for (int u = -r; u <= r; ++u) {
                        const size_t o = (size_t)(y + v) * fw + (x + u);
                        const int gx = q[o + 1] - q[o - 1], gy = q[o + fw] - q[o - fw];
                        Gxx += (i64)(gx * gx); Gxy += (i64)(gx * gy); Gyy += (i64)(gy * gy);
                    }
                s = score_of(Gxx, Gxy, Gyy, r, min_eig);
            }
            plane_out[(size_t)y * fw + x] = s;
        }
    const size_t mp = (size_t)fw + 2 * PAD;
    std::vector<unsigned char> marks;
    if (hx) {
        marks.assign(mp * (size_t)(fh + 2 * PAD), 0);
        for (int i = 0; i < nH; ++i) {
            int mx, my;
            if (held_pixel(hx[i], hy[i], fw, fh, mx, my)) marks[(size_t)(my + PAD) * mp + (size_t)(mx + PAD)] = 1;
        }
    }
    int found = 0;
    for (int y = 0; y < fh; ++y)
        for (int x = 0; x < fw; ++x) {
            const float s = plane_out[(size_t)y * fw + x];
            if (!scored(s)) continue;
            const u64 key = nms_key(s, (unsigned)((size_t)y * fw + x));
            bool corner = true;
            for (int v = -nms; corner && v <= nms; ++v)
                for (int u = -nms; u <= nms; ++u) {
                    const int yy = y + v, xx = x + u;
                    if (yy < 0 || yy >= fh || xx < 0 || xx >= fw) continue;
                    if (nms_key(plane_out[(size_t)yy * fw + xx], (unsigned)((size_t)yy * fw + xx)) > key) { corner = false; break; }
                }
            if (corner && hx)
                for (int v = -nms; corner && v <= nms; ++v)
                    for (int u = -nms; u <= nms; ++u)
                        if (marks[(size_t)(y + v + PAD) * mp + (size_t)(x + u + PAD)]) { corner = false; break; }
            if (!corner) continue;
            if (found < cap) { ox[found] = (float)x; oy[found] = (float)y; os[found] = s; }
            ++found;
        }
    *count = found < cap ? found : cap;
    if (total) *total = found;
}

}  // namespace

extern "C" {

int nm_klt_corners_set_grid_cap(int cap) { return g_grid_cap.exchange(cap < 1 ? 0 : cap); }

size_t nm_klt_corners_workspace_bytes(int n, int fw, int fh)
{
    if (n < 1 || n > nmp::MAX_BATCH || !nm_size_ok(fw) || !nm_size_ok(fh)) return 0;
    return layout_of(n, fw, fh).total;
}

int nm_klt_corners_batch_dev_f32(int n, const float *const *gray, int fw, int fh, const unsigned char *mask,
                                 const float *const *held_x, const float *const *held_y, const int *const *d_held, int cap_held,
                                 int radius, int nms, float min_eig, int cap, float *const *x, float *const *y,
                                 float *const *score, int *d_count, int *d_total, float *const *score_plane, void *workspace,
                                 void *stream)
{
    if (!args_ok(n, gray, fw, fh, held_x, held_y, d_held, cap_held, radius, nms, min_eig, cap, x, y, score, d_count, score_plane) ||
        !workspace)
        return (int)hipErrorInvalidValue;
    const Layout L = layout_of(n, fw, fh);
    unsigned char *ws = reinterpret_cast<unsigned char *>((reinterpret_cast<size_t>(workspace) + WS_ALIGN - 1) & ~(WS_ALIGN - 1));
    float *own = reinterpret_cast<float *>(ws + L.scores);
    u64 *flags = reinterpret_cast<u64 *>(ws + L.flags);
    unsigned char *marks = held_x ? ws + L.marks : nullptr;
    PlaneArgs p;
    ScoreArgs sc;
    EmitArgs e;
    nmp::fill_slots(p.gray, gray, 0, n);
    for (int k = 0; k < nmp::MAX_BATCH; ++k) {
        p.plane[k] = k < n ? (score_plane ? score_plane[k] : own + (size_t)k * fw * fh) : nullptr;
        sc.plane[k] = e.plane[k] = p.plane[k];
    }
    nmp::fill_slots(e.x, x, 0, n); nmp::fill_slots(e.y, y, 0, n); nmp::fill_slots(e.score, score, 0, n);
    size_t low = mask ? (reinterpret_cast<size_t>(mask) & 3) * 4 : 0;      // the mask is read four bytes at a time
    for (int k = 0; k < n; ++k) low |= reinterpret_cast<size_t>(gray[k]);
    const bool wide = !(low & 15) && !(fw & 3);
    const hipStream_t st = nm_stream(stream);
    const long long units = (long long)n * L.wpr * nm_divup(fh, TY);
    hipLaunchKernelGGL(wide ? corners_response_kernel<true> : corners_response_kernel<false>, dim3(grid_of(units)), dim3(THREADS),
                       0, st, p, n, fw, fh, mask, radius, (double)min_eig, marks, L.mark_pitch, L.mark_plane);
    NM_LAUNCH_CHECK();
    if (held_x) {
        HeldArgs h;
        nmp::fill_slots(h.hx, held_x, 0, n); nmp::fill_slots(h.hy, held_y, 0, n); nmp::fill_slots(h.d_held, d_held, 0, n);
        const long long rows = (long long)n * cap_held;
        hipLaunchKernelGGL(corners_mark_kernel, dim3(grid_of((rows + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, h, n,
                           cap_held, fw, fh, marks, L.mark_pitch, L.mark_plane);
        NM_LAUNCH_CHECK();
    }
    const size_t lds = sizeof(u64) * (size_t)(TY + 2 * nms) * (size_t)(2 * TX + 2 * nms);
    hipLaunchKernelGGL(corners_nms_kernel, dim3(grid_of(units)), dim3(THREADS), lds, st, sc, n, fw, fh, nms, marks, L.mark_pitch,
                       L.mark_plane, flags);
    NM_LAUNCH_CHECK();
    hipLaunchKernelGGL(corners_emit_kernel, dim3(grid_of(n)), dim3(THREADS), 0, st, e, n, fw, fh, cap, flags, d_count, d_total);
    NM_LAUNCH_CHECK();
    return 0;
}

int nm_klt_corners_host_f32(int n, const float *const *gray, int fw, int fh, const unsigned char *mask,
                            const float *const *held_x, const float *const *held_y, const int *const *held, int cap_held,
                            int radius, int nms, float min_eig, int cap, float *const *x, float *const *y, float *const *score,
                            int *count, int *total, float *const *score_plane)
{
    if (!args_ok(n, gray, fw, fh, held_x, held_y, held, cap_held, radius, nms, min_eig, cap, x, y, score, count, score_plane))
        return (int)hipErrorInvalidValue;
    for (int k = 0; k < n; ++k)
        corners_host_frame(gray[k], fw, fh, mask, held_x ? held_x[k] : nullptr, held_x ? held_y[k] : nullptr,
                           held_x ? nmp::clip(*held[k], cap_held) : 0, radius, nms, (double)min_eig, cap, x[k], y[k], score[k],
                           count + k, total ? total + k : nullptr, score_plane ? score_plane[k] : nullptr);
    return 0;
}

}  // extern "C"
