// nm_match_distance.hip -- distances in the reference's own arithmetic: the tiled exact kernels (the matcher's fallback for
// unproven rows and the API building blocks transpose / bf_distance / get_sift_matches, which keep the reference's layouts)
// and the materialised distance matrix of nm_sift_match_f32.
#include <atomic>
#include <cstdlib>
#include <cstring>

#include "nm_match_select.hpp"
#include "../../include/nm_abi.h"

namespace nm_match {
namespace {

// Exact squared distances, the reference's own arithmetic (match.cu:36-42): for every (row vector x, column vector y)
//   acc = 0;  for k = 0..127:  t = x_k - y_k;  acc = fma(t, t, acc)
// (fl(x - y) = -fl(y - x) exactly, so which operand is the query does not matter). This is VALU work by nature -- the
// difference has to be formed per pair, so it is not a contraction an MFMA could take -- and its floor is two VALU
// operations per (pair, k): 2 * 128 * rows * cols / 78.6e12 lane-ops/s = 481 us at 12k x 12k. A workgroup owns a 128 x 128
// tile of the output, a thread an 8 x 8 register tile; the operands stream through LDS k-major in chunks of 32 k (two
// b128 reads per operand feed 128 VALU operations: 1 LDS read per 32 VALU instead of the 17 per 32 of the round-1 kernel).
// X: row-side set (nX vectors), Y: column-side set. Element (v, k) is S[v * 128 + k], or S[k * n + v] when K_MAJOR.
// out[row * ld + col].
constexpr int XD_TILE = 128, XD_KC = 32, XD_PITCH = XD_TILE + 4;

template <bool K_MAJOR>
__device__ __forceinline__ void xd_stage(float *__restrict__ dst, const float *__restrict__ S, int n, int v0, int kc, int tid)
{
    if (K_MAJOR) {           // S[k][v]: rows of the LDS image are contiguous in memory
#pragma unroll
        for (int it = 0; it < (XD_KC * XD_TILE) / 256; ++it) {
            const int e = tid + 256 * it;
            const int k = e >> 7, v = e & 127;
            dst[k * XD_PITCH + v] = (v0 + v < n) ? S[(size_t)(kc + k) * n + v0 + v] : 0.f;
        }
    } else {                 // S[v][k]: 8 lanes read the 32 k of one vector (128 contiguous bytes), scattered k-major into LDS
#pragma unroll
        for (int it = 0; it < (XD_KC * XD_TILE) / (256 * 4); ++it) {
            const int e = tid + 256 * it;
            const int v = e >> 3, k4 = (e & 7) * 4;
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (v0 + v < n) x = *reinterpret_cast<const float4 *>(S + (size_t)(v0 + v) * DIM + kc + k4);
            dst[(k4 + 0) * XD_PITCH + v] = x.x; dst[(k4 + 1) * XD_PITCH + v] = x.y;
            dst[(k4 + 2) * XD_PITCH + v] = x.z; dst[(k4 + 3) * XD_PITCH + v] = x.w;
        }
    }
}

// Exact fallback for the queries the finalize pass could not prove: the listed rows are re-scanned against ALL candidates
// with the reference's arithmetic, as a tiled exact-distance computation (128 listed rows x 128 candidates per step, 8 x 8
// register tiles as in exact_distance_kernel) that keeps only the running (min1, lowest index, second minimum) of every
// row. A workgroup owns one 128-row chunk of the list and one of FB_SPLIT contiguous candidate slices; slice results go to
// `part` and match_fallback_merge_kernel combines them in ascending slice order. A candidate row is read once per chunk,
// not once per listed row (the round-1 kernel scanned row by row: 9 ms for the 1.5 % of rows listed at 100k x 100k).
constexpr int FB_SPLIT = 64;
constexpr int FB_CHUNKS = 16;          // chunk loops in flight (gridDim.y); a workgroup strides over the chunks
constexpr int FB_ROWWISE_MAX = 24;     // up to this many listed rows: one pass per row instead of 128-row tiles

__global__ __launch_bounds__(256) void match_fallback_kernel(MatchBatch bt)
{
    const MatchPair &c = bt.p[blockIdx.z];
    const float *__restrict__ A = c.A, *__restrict__ B = c.B;
    const int nB = pair_nB(c);
    const int *__restrict__ fb_list = c.fb_list;
    float4 *__restrict__ part = c.partial;
    __shared__ __attribute__((aligned(16))) float sXY[2 * XD_KC * XD_PITCH];
    float *const sX = sXY, *const sY = sXY + XD_KC * XD_PITCH;
    const int count = *c.fb_count;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int slice = nm_divup_dev(nB, FB_SPLIT);
    const int j0 = blockIdx.x * slice, j1 = min(j0 + slice, nB);
    if (count <= FB_ROWWISE_MAX) {
        // A handful of rows (the usual case: 0-10 of 12k on SIFT descriptors): a 128-row tile would be almost empty. The
        // listed rows wait in LDS; the slice's candidates pass through LDS 64 at a time (coalesced loads -- a lane that
        // streams its own 512-byte candidate row touches 64 cache lines per load instruction, which made this path
        // ~25 us per listed row); thread (candidate = tid % 64, wave w) then holds its candidate in registers and runs
        // the exact chain against the rows w, w + 4, ... (broadcast LDS reads). One workgroup per slice (blockIdx.y = 0).
        constexpr int RW = (FB_ROWWISE_MAX + 3) / 4;          // rows per wave
        __shared__ __attribute__((aligned(16))) float sQ[FB_ROWWISE_MAX * DIM];
        static_assert(64 * KP <= 2 * XD_KC * XD_PITCH, "64 candidates at pitch KP fit the tile buffers");
        if (blockIdx.y != 0 || count <= 0) return;
        for (int q = tid; q < count * (DIM / 4); q += 256) {
            const int e = q >> 5, k4 = q & 31;
            reinterpret_cast<float4 *>(sQ)[q] = reinterpret_cast<const float4 *>(A + (size_t)fb_list[e] * DIM)[k4];
        }
        const int cand = tid & 63, w = tid >> 6;
        float m1[RW], m2[RW]; int i1[RW];
#pragma unroll
        for (int s2 = 0; s2 < RW; ++s2) { m1[s2] = __builtin_inff(); m2[s2] = __builtin_inff(); i1[s2] = 0x7fffffff; }
        for (int c0 = j0; c0 < j1; c0 += 64) {
            __syncthreads();
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                const int row = (tid >> 5) + 8 * it, k4 = tid & 31;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c0 + row < j1) v = reinterpret_cast<const float4 *>(B + (size_t)(c0 + row) * DIM)[k4];
                *reinterpret_cast<float4 *>(&sXY[row * KP + 4 * k4]) = v;
            }
            __syncthreads();
            const int j = c0 + cand;
            float4 y[DIM / 4];
#pragma unroll
            for (int k = 0; k < DIM / 4; ++k) y[k] = *reinterpret_cast<const float4 *>(&sXY[cand * KP + 4 * k]);
#pragma unroll
            for (int s2 = 0; s2 < RW; ++s2) {
                const int e = w + 4 * s2;
                if (e < count) {                                 // uniform per wave
                    const float4 *x = reinterpret_cast<const float4 *>(sQ + e * DIM);
                    float acc = 0.0f;
#pragma unroll
                    for (int k = 0; k < DIM / 4; ++k) {
                        const float4 xv = x[k];
                        float tt;
                        tt = xv.x - y[k].x; acc = __builtin_fmaf(tt, tt, acc);
                        tt = xv.y - y[k].y; acc = __builtin_fmaf(tt, tt, acc);
                        tt = xv.z - y[k].z; acc = __builtin_fmaf(tt, tt, acc);
                        tt = xv.w - y[k].w; acc = __builtin_fmaf(tt, tt, acc);
                    }
                    if (j < j1) {
                        if (acc < m1[s2]) { m2[s2] = m1[s2]; m1[s2] = acc; i1[s2] = j; }
                        else if (acc < m2[s2]) m2[s2] = acc;
                    }
                }
            }
        }
#pragma unroll
        for (int s2 = 0; s2 < RW; ++s2) {
            const int e = w + 4 * s2;
            if (e >= count) continue;
            float a1 = m1[s2], a2 = m2[s2]; int ai = i1[s2];
#pragma unroll
            for (int sft = 1; sft < 64; sft <<= 1) {
                const float o1 = __shfl_xor(a1, sft), o2 = __shfl_xor(a2, sft);
                const int oi = __shfl_xor(ai, sft);
                top2_merge(a1, ai, a2, o1, oi, o2);
            }
            if (cand == 0) part[(size_t)e * FB_SPLIT + blockIdx.x] = make_float4(a1, __int_as_float(ai), a2, 0.f);
        }
        return;
    }
    for (int e0 = blockIdx.y * XD_TILE; e0 < count; e0 += gridDim.y * XD_TILE) {
        float m1[8], m2[8]; int i1[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) { m1[i] = __builtin_inff(); m2[i] = __builtin_inff(); i1[i] = 0x7fffffff; }
        for (int c0 = j0; c0 < j1; c0 += XD_TILE) {
            float acc[8][8];
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
            for (int kc = 0; kc < DIM; kc += XD_KC) {
                __syncthreads();
#pragma unroll
                for (int it = 0; it < (XD_KC * XD_TILE) / (256 * 4); ++it) {       // listed query rows, gathered
                    const int e = tid + 256 * it;
                    const int v = e >> 3, k4 = (e & 7) * 4;
                    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (e0 + v < count) x = *reinterpret_cast<const float4 *>(A + (size_t)fb_list[e0 + v] * DIM + kc + k4);
                    sX[(k4 + 0) * XD_PITCH + v] = x.x; sX[(k4 + 1) * XD_PITCH + v] = x.y;
                    sX[(k4 + 2) * XD_PITCH + v] = x.z; sX[(k4 + 3) * XD_PITCH + v] = x.w;
                }
                xd_stage<false>(sY, B, j1, c0, kc, tid);
                __syncthreads();
#pragma unroll 4
                for (int k = 0; k < XD_KC; ++k) {
                    const float4 xa = *reinterpret_cast<const float4 *>(&sX[k * XD_PITCH + ty * 8]);
                    const float4 xb = *reinterpret_cast<const float4 *>(&sX[k * XD_PITCH + ty * 8 + 4]);
                    const float4 ya = *reinterpret_cast<const float4 *>(&sY[k * XD_PITCH + tx * 8]);
                    const float4 yb = *reinterpret_cast<const float4 *>(&sY[k * XD_PITCH + tx * 8 + 4]);
                    const float xv[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
                    const float yv[8] = {ya.x, ya.y, ya.z, ya.w, yb.x, yb.y, yb.z, yb.w};
#pragma unroll
                    for (int i = 0; i < 8; ++i)
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const float t = xv[i] - yv[j];
                            acc[i][j] = __builtin_fmaf(t, t, acc[i][j]);
                        }
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {                       // ascending candidate index within the thread
                const int col = c0 + tx * 8 + j;
                if (col < j1) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const float d = acc[i][j];
                        if (d < m1[i]) { m2[i] = m1[i]; m1[i] = d; i1[i] = col; }
                        else if (d < m2[i]) m2[i] = d;
                    }
                }
            }
        }
        // the 16 threads that share a row: butterfly over tx (lanes of one wave), index breaks ties
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int sft = 1; sft < 16; sft <<= 1) {
                const float o1 = __shfl_xor(m1[i], sft), o2 = __shfl_xor(m2[i], sft);
                const int oi = __shfl_xor(i1[i], sft);
                top2_merge(m1[i], i1[i], m2[i], o1, oi, o2);
            }
            const int e = e0 + ty * 8 + i;
            if (tx == 0 && e < count) part[(size_t)e * FB_SPLIT + blockIdx.x] = make_float4(m1[i], __int_as_float(i1[i]), m2[i], 0.f);
        }
    }
}

__global__ __launch_bounds__(256) void match_fallback_merge_kernel(MatchBatch bt)
{
    const MatchPair &c = bt.p[blockIdx.y];
    const int *__restrict__ fb_count = c.fb_count, *__restrict__ fb_list = c.fb_list;
    const float4 *__restrict__ part = c.partial;
    const int mode = c.mode, index_offset = c.index_offset;
    const float ambiguity = bt.ambiguity;
    int *__restrict__ result = c.result;
    float *__restrict__ min1_out = c.min1, *__restrict__ min2_out = c.min2;
    int *__restrict__ idx_out = c.idx1;
    const int count = *fb_count;
    const bool holds0 = (mode == 0) || (index_offset == 0);      // this call's candidate 0 is the scan's candidate 0
    for (int e = blockIdx.x * 256 + threadIdx.x; e < count; e += gridDim.x * 256) {
        // the slices left NaN distances out and never record +inf (strict < from +inf): the scan's view of candidates >= 1
        float m1 = __builtin_inff(), m2 = __builtin_inff(); int i1 = 0x7fffffff;
        for (int sl = 0; sl < FB_SPLIT; ++sl) {
            const float4 p = part[(size_t)e * FB_SPLIT + sl];
            top2_merge(m1, i1, m2, p.x, __float_as_int(p.y), p.z);
        }
        const int row = fb_list[e];
        int idx = (i1 == 0x7fffffff) ? (holds0 ? 0 : -1) : i1 + index_offset;
        if (holds0) {
            // match.cu:90: the scan STARTS from the distance to candidate 0; a NaN there is never replaced
            const float d0 = exact_dist(reinterpret_cast<const float4 *>(c.A + (size_t)row * DIM), reinterpret_cast<const float4 *>(c.B));
            if (d0 != d0) { m2 = m1; m1 = d0; idx = 0; }
        }
        emit_match(row, m1, idx, m2, mode, ambiguity, result, min1_out, idx_out, min2_out);
    }
}

// ---- exact API building blocks ----
__global__ __launch_bounds__(256) void transpose_kernel(float *__restrict__ odata, const float *__restrict__ idata,
                                                       int width, int height)
{
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;       // 32 x 8
    int x = blockIdx.x * 32 + tx;
    for (int k = 0; k < 32; k += 8) {
        const int y = blockIdx.y * 32 + ty + k;
        if (x < width && y < height) tile[ty + k][tx] = idata[(size_t)y * width + x];
    }
    __syncthreads();
    x = blockIdx.y * 32 + tx;                                     // output column = input row
    for (int k = 0; k < 32; k += 8) {
        const int y = blockIdx.x * 32 + ty + k;                   // output row = input column
        if (x < height && y < width) odata[(size_t)y * height + x] = tile[tx][ty + k];
    }
}

// t = x - y and acc = fma(t, t, acc) for TWO column elements per instruction (v_pk_add_f32 with the x element broadcast by
// op_sel and y negated by neg_lo / neg_hi, then v_pk_fma_f32): the same IEEE operations per element as the scalar pair, in
// the same order -- half the VALU instructions, so one wave alone keeps its SIMD's vector pipe busy (a wave issues one
// vector instruction per ~4 cycles whatever its width).
typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void xd_step(v2f &acc, v2f xpair, v2f y, bool hi)
{
    v2f t;
    if (hi) asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(t) : "v"(xpair), "v"(y));
    else asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(t) : "v"(xpair), "v"(y));
    asm("v_pk_fma_f32 %0, %1, %1, %0" : "+v"(acc) : "v"(t));
}

template <bool X_KMAJOR, bool Y_KMAJOR>
__global__ __launch_bounds__(256) void exact_distance_kernel(const float *__restrict__ X, int nX,
                                                            const float *__restrict__ Y, int nY,
                                                            float *__restrict__ out, size_t ld,
                                                            const int *__restrict__ only_if_above, int threshold)
{
    // (behind the MFMA distance pass: runs only when that pass's list of uncovered entries overflowed -- uniform scalar load)
    if (only_if_above && *only_if_above <= threshold) return;
    __shared__ __attribute__((aligned(16))) float sX[XD_KC * XD_PITCH];
    __shared__ __attribute__((aligned(16))) float sY[XD_KC * XD_PITCH];
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;                 // 16 x 16 threads, 8 x 8 outputs each
    const int c0 = blockIdx.x * XD_TILE, r0 = blockIdx.y * XD_TILE;
    v2f acc[8][4];                                          // [row][column pair]
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (v2f){0.f, 0.f};
    for (int kc = 0; kc < DIM; kc += XD_KC) {
        __syncthreads();
        xd_stage<X_KMAJOR>(sX, X, nX, r0, kc, tid);
        xd_stage<Y_KMAJOR>(sY, Y, nY, c0, kc, tid);
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < XD_KC; ++k) {
            const float4 xa = *reinterpret_cast<const float4 *>(&sX[k * XD_PITCH + ty * 8]);
            const float4 xb = *reinterpret_cast<const float4 *>(&sX[k * XD_PITCH + ty * 8 + 4]);
            const float4 ya = *reinterpret_cast<const float4 *>(&sY[k * XD_PITCH + tx * 8]);
            const float4 yb = *reinterpret_cast<const float4 *>(&sY[k * XD_PITCH + tx * 8 + 4]);
            const v2f xp[4] = {{xa.x, xa.y}, {xa.z, xa.w}, {xb.x, xb.y}, {xb.z, xb.w}};
            const v2f yp[4] = {{ya.x, ya.y}, {ya.z, ya.w}, {yb.x, yb.y}, {yb.z, yb.w}};
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) xd_step(acc[i][j], xp[i >> 1], yp[j], (i & 1) != 0);
        }
    }
    const int col = c0 + tx * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int row = r0 + ty * 8 + i;
        if (row >= nX) continue;
        float *o = out + (size_t)row * ld + col;
        if (col + 7 < nY && ((reinterpret_cast<uintptr_t>(o) & 15) == 0)) {
            *reinterpret_cast<float4 *>(o) = make_float4(acc[i][0].x, acc[i][0].y, acc[i][1].x, acc[i][1].y);
            *reinterpret_cast<float4 *>(o + 4) = make_float4(acc[i][2].x, acc[i][2].y, acc[i][3].x, acc[i][3].y);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (col + j < nY) o[j] = (j & 1) ? acc[i][j >> 1].y : acc[i][j >> 1].x;
        }
    }
}

// ---- the materialised distance matrix on the fp32 MFMA (round 5; reference: kernels/match.cu:14-80, siftfunctions.cu:28-34) ----
// D[i][j] = |x_i - y_j|^2 as |x'_i|^2 + |y'_j|^2 - 2 x'_i . y'_j on v_mfma_f32_32x32x2_f32 with the store fused into the
// kernel, where x' = x - mu, y' = y - mu are the rows CENTRED on the mean row of Y: distances are translation-invariant, and
// the contraction's rounding error scales with the norms of what is multiplied, not with the distance (rows that share a large
// common component -- an offset, a dominant mean descriptor -- would otherwise all fail the test below).
// Every entry is within 1e-4 relative of the reference's chain (acc = fma(t, t, acc), t = x_k - y_k, match.cu:36-42):
//   * the value v is the sum of TWO accumulator chains (k = 0..63 with the norm pair, k = 64..127): no term passes through more
//     than 67 roundings (2 + 64 steps of a chain, the final add), and the tabulated norms carry 8 (distance_center_kernel), so
//     with d' the exact distance of the centred rows  |v - d'| <= (gamma_67 + gamma_8) (sqrt nx + sqrt ny)^2 = 4.47e-6 (..)^2;
//     DIST_C = 5.15e-6 is that with 15 % of slack. (Premise, as for the matcher's fp32 screen: an instruction is two fused
//     steps, C + a0 b0 + a1 b1 with at most two roundings -- nm_selftest_mfma_model(f32) measures it.)
//   * centring rounds once per element, |x'_k - (x_k - mu_k)| <= u |x'_k|: sqrt d differs from sqrt d' by at most
//     u (sqrt nx + sqrt ny);
//   * the reference's own chain is within gamma_130 d <= 7.8e-6 d of the true d.
//   An entry is ACCEPTED iff v >= K (sqrt nx + sqrt ny)^2, K = DIST_C / 7.8e-5 = 0.066: then |v - d'| <= 7.8e-5 v, the centring
//   moves d by < 4.7e-7 d', and |v - d_ref| < (7.8e-5 + 4.7e-7 + 7.8e-6 + products) d_ref < 8.7e-5 d_ref.
//   Every other entry -- near-duplicates, exact copies, negative or NaN values from cancellation or overflow -- belongs to a
//   32 x 32 block that is LISTED; distance_fixup_kernel re-applies the test to the block's stored values and recomputes what
//   fails it by the reference's own chain: bit-equal to the exact kernel. If the list overflows, the whole matrix is
//   (exact_distance_kernel launched behind it runs only then). Uncorrelated rows have d' ~ nx + ny >= (sqrt nx + sqrt ny)^2 / 2;
//   only pairs whose centred rows correlate above ~0.87 fail (1.7e-4 of the pairs of two 1080p frames' descriptors, 5 % of the
//   blocks). The test is v_add + v_mul + v_cmp per entry (sqrt(K n) is tabulated, rounded up).
// Layout: rows of the MFMA result = the STREAMED set X (128-row tiles through LDS, registers), columns = the RESIDENT set Y
// (32 rows per wave, fragments in VGPRs, lanes): a store instruction writes 128 contiguous bytes of D per half wave.
struct DistArgs {
    const float *Xc, *Yc;         // centred rows (n x 128)
    const float *nx, *ny;         // their squared norms
    const float *tx, *ty;         // sqrt(K norm), rounded up: the acceptance test is v >= (tx_i + ty_j)^2
    float *D; size_t ldd;         // D[i * ldd + j], i over X, j over Y
    int nX, nY;
    int *fix_count; int2 *fix_list; int fix_cap;
    int *fix_report;              // where the fix-up pass leaves the number of listed blocks (the list's memory is reused)
};
constexpr int DIST_P = 64;        // row slices of the column-sum pass
constexpr float DIST_C = 5.15e-6f;                    // |v - d'| <= DIST_C (sqrt nx + sqrt ny)^2
constexpr float DIST_K = DIST_C / 7.8e-5f;            // acceptance: v >= DIST_K (sqrt nx + sqrt ny)^2

// column sums of Y in DIST_P slices: part[slice][k] = sum of y[r][k] over rows r = slice, slice + DIST_P, ... (fixed order)
__global__ __launch_bounds__(128) void distance_colsum_kernel(const float *__restrict__ Y, int nY, float *__restrict__ part)
{
    const int k = threadIdx.x, sl = blockIdx.x;
    float s = 0.f;
    for (int r = sl; r < nY; r += DIST_P) s += Y[(size_t)r * DIM + k];
    part[sl * DIM + k] = s;
}

// blockIdx.y = 0: X, 1: Y. One wave per row: x' = x - mu, |x'|^2 (fma pair + wave tree: 8 roundings), sqrt(K |x'|^2) rounded up.
__global__ __launch_bounds__(256) void distance_center_kernel(const float *__restrict__ X, int nX, const float *__restrict__ Y, int nY,
                                                             const float *__restrict__ part, float *__restrict__ Xc,
                                                             float *__restrict__ Yc, float *__restrict__ nx, float *__restrict__ ny,
                                                             float *__restrict__ tx, float *__restrict__ ty, int *__restrict__ fix_count)
{
    __shared__ float mu[DIM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < DIM) {
        float s = 0.f;
        for (int p = 0; p < DIST_P; ++p) s += part[p * DIM + tid];
        mu[tid] = s / (float)nY;
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) *fix_count = 0;
    __syncthreads();
    const bool second = blockIdx.y != 0;
    const float *S = second ? Y : X;
    float *Sc = second ? Yc : Xc, *nn = second ? ny : nx, *tt = second ? ty : tx;
    const int n = second ? nY : nX;
    const float2 m2 = *reinterpret_cast<const float2 *>(&mu[2 * lane]);
    for (int r = blockIdx.x * 4 + wave; r < n; r += gridDim.x * 4) {
        const float2 v = *reinterpret_cast<const float2 *>(S + (size_t)r * DIM + 2 * lane);
        const float2 c = make_float2(v.x - m2.x, v.y - m2.y);
        *reinterpret_cast<float2 *>(Sc + (size_t)r * DIM + 2 * lane) = c;
        float q = __builtin_fmaf(c.x, c.x, c.y * c.y);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) q += __shfl_xor(q, d);
        if (lane == 0) { nn[r] = q; tt[r] = __builtin_sqrtf(q * DIST_K) * 1.000002f; }
    }
}

// Epilogue of one 32 x 32 accumulator: register e holds tile row rb + 8 (e / 4) + 4 h + (e % 4), column = this lane's j.
// Every value is stored. If ANY value of the 32 x 32 block is outside the bound, the BLOCK is listed (one atomic by one lane):
// distance_fixup_kernel reads the block's stored values back, applies the same test to the same values and recomputes exactly
// what fails it. FULL: all 128 rows of the tile exist (only the last row tile of X is ragged; its missing rows are masked).
template <bool FULL>
__device__ __forceinline__ void dist_emit(const f32x16 &acc, const DistArgs &a, __amdgpu_buffer_rsrc_t rsD, const float *tab,
                                          int rb, int h, unsigned long long jmask, float tyj, unsigned vo, unsigned ld4,
                                          int i_blk, int j_blk, int rows_here)
{
    // vo: this lane's byte offset inside the tile's rows of D, 0x80000000 for a lane whose column does not exist -- beyond any
    // tile's byte range (< 2^31), so the descriptor's range check drops that lane's stores whatever soffset adds (the probe
    // tools/micro/buffer_range.hip shows voffset + soffset checked on this device). jmask = lanes with a column.
    unsigned long long listed = 0;
#pragma unroll
    for (int e4 = 0; e4 < 4; ++e4) {
        const float4 t4 = *reinterpret_cast<const float4 *>(tab + rb + 8 * e4 + 4 * h);
        const float tv[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
        for (int e1 = 0; e1 < 4; ++e1) {
            const int e = 4 * e4 + e1;
            // lanes whose value is NOT >= the acceptance term (unordered-or-less-than: a NaN is listed), as a wave mask
            const float sq = tv[e1] + tyj;
            const unsigned long long below = __builtin_amdgcn_fcmpf(acc[e], sq * sq, 12 /* FCMP_ULT */);
            if (FULL) {
                listed |= below;
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[e]), rsD, vo, (rb + 8 * e4 + e1) * ld4, 0);
            } else {                                        // last row tile of X: rows >= rows_here do not exist
                const bool ok = rb + 8 * e4 + 4 * h + e1 < rows_here;
                listed |= below & __ballot(ok);
                if (ok) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[e]), rsD, vo, (rb + 8 * e4 + e1) * ld4, 0);
            }
        }
    }
    if (__builtin_expect((listed & jmask) != 0, 0)) {       // near-duplicates, cancellation, non-finite values
        if ((threadIdx.x & 63) == 0) {
            const int at = atomicAdd(a.fix_count, 1);
            if (at < a.fix_cap) a.fix_list[at] = make_int2(i_blk, j_blk);
        }
    }
}

__global__ __launch_bounds__(512, 1) void distance_mfma_kernel(DistArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *const tabuf = lds + 2 * TILE_C * KP;             // 2 x 128 acceptance terms of the streamed rows
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int srow = tid >> 5, scol = (tid & 31) * 4;       // staging coordinates: 16 rows x 32 float4 per pass
    const int nX = a.nX, nY = a.nY;
    const int n_rt = nm_divup_dev(nX, TILE_C), n_cb = nm_divup_dev(nY, QB);
    const long long U = (long long)n_rt * n_cb;
    const long long u0 = U * blockIdx.x / gridDim.x, u1 = U * (blockIdx.x + 1) / gridDim.x;
    if (u0 >= u1) return;
    const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.Xc), 0, nX * (DIM * 4), 0x00020000);
    const int voff = (srow * DIM + scol) * 4;

    u32x4 st[8];
    float stn = 0.f, stt = 0.f;
    auto stage_load = [&](int rt) {                         // rows rt * 128 .. + 127 of X -> registers (rows >= nX read as zeros)
        const int ib = rt * TILE_C;
        // (the row offset rides in voffset, which every reading of the ISA includes in the descriptor's range check; on this
        // device soffset is included too -- tools/micro/buffer_range.hip, profiles/r05_b_buffer_range_probe.txt)
#pragma unroll
        for (int it = 0; it < 8; ++it) st[it] = __builtin_amdgcn_raw_buffer_load_b128(rsX, voff + (ib + 16 * it) * (DIM * 4), 0, 0);
        if (tid < TILE_C) {
            const bool ok = ib + tid < nX;
            stn = ok ? a.nx[ib + tid] : 0.f;
            stt = ok ? a.tx[ib + tid] : 0.f;
        }
    };
    auto stage_write = [&](int b) {
        float *buf = lds + b * (TILE_C * KP);
#pragma unroll
        for (int it = 0; it < 8; ++it) *reinterpret_cast<u32x4 *>(&buf[(srow + 16 * it) * KP + scol]) = st[it];
        if (tid < TILE_C) {                                 // augmented k-pair (|x'|^2, 1) and the row's acceptance term
            *reinterpret_cast<float2 *>(&buf[tid * KP + DIM]) = make_float2(stn, 1.0f);
            tabuf[b * TILE_C + tid] = stt;
        }
    };

    float4 qf[16];
    float nq = 0.f, tyj = 0.f;
    int cb_held = -1;
    const int jw = wave * 32 + r;                           // this lane's column inside the 256-column block
    stage_load((int)(u0 % n_rt));
    stage_write(0);
    __syncthreads();
    int b = 0;
    for (long long u = u0; u < u1; ++u) {
        const int cb = (int)(u / n_rt), rt = (int)(u - (long long)cb * n_rt);
        if (u + 1 < u1) stage_load((int)((u + 1) % n_rt));
        const int j = cb * QB + jw;
        const bool j_ok = j < nY;
        if (cb != cb_held) {                                // resident fragments of this wave's 32 columns, scaled by -2 (exact)
            cb_held = cb;
            const float4 *yr = reinterpret_cast<const float4 *>(a.Yc + (size_t)(j_ok ? j : 0) * DIM) + h;
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const float4 v = j_ok ? yr[2 * t] : make_float4(0.f, 0.f, 0.f, 0.f);
                qf[t] = make_float4(-2.f * v.x, -2.f * v.y, -2.f * v.z, -2.f * v.w);
            }
            const float nyj = j_ok ? a.ny[j] : 0.f;
            tyj = j_ok ? a.ty[j] : 0.f;
            nq = (h == 0) ? 1.0f : nyj;
        }
        const int i0 = rt * TILE_C;
        const float *buf = lds + b * (TILE_C * KP);
        const float *rowp = buf + r * KP + 4 * h, *normp = buf + r * KP + DIM + h;
        const float *tab = tabuf + b * TILE_C;
        // the tile's rows of D as a range-checked view: rows >= nX are dropped by the hardware (32-bit byte range: 128 ldd 4)
        const int rows_here = min(TILE_C, nX - i0);
        const __amdgpu_buffer_rsrc_t rsD = __builtin_amdgcn_make_buffer_rsrc(a.D + (size_t)i0 * a.ldd, 0,
                                                                             (int)((size_t)rows_here * a.ldd * 4), 0x00020000);
        unsigned ld4 = (unsigned)(a.ldd * 4);
        asm volatile("" : "+s"(ld4));                       // per unit: keeps the 128 row offsets (row x ld4) out of loop-invariant SGPRs
        const unsigned vo = j_ok ? (unsigned)j * 4u + (unsigned)(4 * h) * ld4 : 0x80000000u;
        const unsigned long long jmask = __ballot(j_ok);
        f32x16 a0, a1;
        const bool full = rows_here == TILE_C;              // uniform: only the last row tile of X is ragged
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            // two chains per accumulator: k = 0..63 with the norm pair, k = 64..127 from zero, one add (the error bound above)
            f32x16 b0, b1;
            mfma_kgroups<0, 8, true>(a0, a1, rowp + 64 * half * KP, normp + 64 * half * KP, qf, nq);
            mfma_kgroups<8, 16, false>(b0, b1, rowp + 64 * half * KP, normp + 64 * half * KP, qf, nq);
            a0 += b0; a1 += b1;
            const int jb = cb * QB + wave * 32;
            if (full) {
                dist_emit<true>(a0, a, rsD, tab, 64 * half, h, jmask, tyj, vo, ld4, i0 + 64 * half, jb, rows_here);
                dist_emit<true>(a1, a, rsD, tab, 64 * half + 32, h, jmask, tyj, vo, ld4, i0 + 64 * half + 32, jb, rows_here);
            } else {
                dist_emit<false>(a0, a, rsD, tab, 64 * half, h, jmask, tyj, vo, ld4, i0 + 64 * half, jb, rows_here);
                dist_emit<false>(a1, a, rsD, tab, 64 * half + 32, h, jmask, tyj, vo, ld4, i0 + 64 * half + 32, jb, rows_here);
            }
        }
        if (u + 1 < u1) stage_write(b ^ 1);
        __syncthreads();
        b ^= 1;
    }
}

// The listed 32 x 32 blocks: one wave per block reads the block's stored values back, applies the acceptance test of the MFMA
// pass to them (same values, same tabulated terms: the same decision) and overwrites what fails it with the reference's own
// chain (the rows come from L2).
__global__ __launch_bounds__(256) void distance_fixup_kernel(const float *__restrict__ X, const float *__restrict__ Y, DistArgs a)
{
    const int n = *a.fix_count;
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.fix_report) *a.fix_report = n;
    if (n > a.fix_cap) return;                              // overflow: the exact kernel behind this launch fills everything
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int jl = lane & 31, ih = lane >> 5;
    for (int q = blockIdx.x * 4 + wave; q < n; q += gridDim.x * 4) {
        const int2 blk = a.fix_list[q];
        const int j = blk.y + jl;
        if (j >= a.nY) continue;
        const float tyj = a.ty[j];
        for (int rr = ih; rr < 32; rr += 2) {
            const int i = blk.x + rr;
            if (i >= a.nX) break;
            float *d = a.D + (size_t)i * a.ldd + j;
            const float sq = a.tx[i] + tyj;
            if (!(*d >= sq * sq))
                *d = exact_dist(reinterpret_cast<const float4 *>(X + (size_t)i * DIM), reinterpret_cast<const float4 *>(Y + (size_t)j * DIM));
        }
    }
}

// One wave per row: lane-local ascending scan + wave merge of (min1, lowest index, multiset second minimum).
__global__ __launch_bounds__(256) void set_matches_kernel(int *__restrict__ result, const float *__restrict__ distance,
                                                         int rows, int cols, int buffer_width, float ambiguity)
{
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float *d = distance + (size_t)row * buffer_width;
    float m1 = __builtin_inff(), m2 = __builtin_inff(); int i1 = 0x7fffffff;
    for (int j = lane; j < cols; j += 64) {
        const float c = d[j];
        if (c < m1) { m2 = m1; m1 = c; i1 = j; }
        else if (c < m2) m2 = c;
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const float o1 = __shfl_xor(m1, s), o2 = __shfl_xor(m2, s);
        const int oi = __shfl_xor(i1, s);
        const bool take = (o1 < m1) || (o1 == m1 && oi < i1);
        const float lo = take ? o1 : m1, hi = take ? m1 : o1;        // hi = the larger of the two minima
        const float s2 = take ? o2 : m2;                              // second of the winner's own list
        i1 = take ? oi : i1;
        m1 = lo;
        m2 = (hi < s2) ? hi : s2;                                     // the loser's own second is >= hi
    }
    if (lane == 0) {
        // (m1, i1, m2): what the scan's comparisons see -- NaN entries left out, +inf never recorded (strict < from +inf)
        int idx = (i1 == 0x7fffffff) ? 0 : i1;
        const float d0 = d[0];                                        // match.cu:90: a NaN at column 0 is never replaced
        if (d0 != d0) { m2 = m1; m1 = d0; idx = 0; }
        emit_match(row, m1, idx, m2, 0, ambiguity, result, nullptr, nullptr, nullptr);
    }
}

// How nm_sift_match_f32 fills a requested `distance` matrix: 1 = on the fp32 MFMA (distance_mfma_kernel: every entry within
// 1e-4 relative of the reference's chain, listed entries bit-equal to it), 0 = exact_distance_kernel (VALU; every entry
// bit-equal). NM_MATCH_DISTANCE=exact|mfma or nm_sift_match_set_distance_mode() select it (process-wide). The match indexes do
// not depend on it: they are decided on exactly recomputed distances either way.
static std::atomic<int> g_dist_mode{-1};
static int distance_mode()
{
    int v = g_dist_mode.load(std::memory_order_relaxed);
    if (v < 0) {
        const char *e = getenv("NM_MATCH_DISTANCE");
        v = (e && (!strcmp(e, "exact") || !strcmp(e, "0"))) ? 0 : 1;
        g_dist_mode.store(v, std::memory_order_relaxed);
    }
    return v;
}

// The scratch of the MFMA distance pass lives INSIDE the matcher's workspace of the same (nA, nB): the pass runs before the
// fused matcher on the same stream, and every region it uses is (re)written by the matcher's own prep / screen kernels
// afterwards -- centred copies in the bf16 split images (same 512 bytes per row), norms and acceptance terms in the fp16
// images, column sums + counter + list in the partial lists. Returns false when the partial-list pool is too small for that
// (a few dozen query rows): the caller then takes the exact kernel.
static bool distance_scratch(const MatchWs &w, int nA, DistArgs &a, float **part)
{
    char *pool = reinterpret_cast<char *>(w.partial);
    const size_t pool_bytes = align256((size_t)nA * MAX_CHUNKS * sizeof(float4)) + align256((size_t)nA * MAX_CHUNKS * sizeof(float));
    const size_t head = (size_t)DIST_P * DIM * sizeof(float) + 256;
    if (pool_bytes < head + 65536) return false;
    *part = reinterpret_cast<float *>(pool);
    a.fix_count = reinterpret_cast<int *>(pool + (size_t)DIST_P * DIM * sizeof(float));
    a.fix_list = reinterpret_cast<int2 *>(pool + head);
    const size_t cap = (pool_bytes - head) / sizeof(int2);
    a.fix_cap = (int)(cap > 0x3fffffff ? 0x3fffffff : cap);
    a.Xc = reinterpret_cast<const float *>(w.As); a.Yc = reinterpret_cast<const float *>(w.Bs);
    a.nx = reinterpret_cast<const float *>(w.Ah); a.tx = a.nx + nA;                 // nA x 256 bytes available
    a.ny = reinterpret_cast<const float *>(w.Bh); a.ty = nullptr;                   // set by the caller (needs nB)
    a.fix_report = w.fb_count + CB_DIST_REPORT;
    return true;
}

// More than a quarter of the 32 x 32 blocks listed (one NaN or inf in B makes the mean row NaN and lists EVERY block; so do sets of
// near-duplicates): the per-block fix-up -- one wave per block, the rows from L2 -- is then far slower than exact_distance_kernel,
// so the list counts as overflowed from there on and the exact kernel behind it fills the whole matrix (ADVICE r5;
// tests/test_gpu_match.py::test_distance_with_one_nan_takes_the_exact_kernel).
static int distance_list_cap(int pool_cap, int nA, int nB)
{
    const long long blocks = (long long)nm_divup(nA, 32) * nm_divup(nB, 32);
    const long long quarter = blocks / 4 > 1 ? blocks / 4 : 1;
    return pool_cap > quarter ? (int)quarter : pool_cap;
}

}  // namespace

int launch_fallback(const MatchBatch &bt, hipStream_t st)
{
    static_assert(FB_SPLIT <= MAX_CHUNKS, "fallback slices reuse the partial area");
    // few rows are ever listed (0-2 of 12k on SIFT data): a small grid drains fastest when the list is empty, and its
    // workgroups loop over the entries when it is not
    // (~1 000 workgroups whatever the number of pairs: with 16 chunk loops for each of 16 pairs the launch spent ~150 us
    // dispatching 16 384 workgroups that found their lists empty)
    hipLaunchKernelGGL(match_fallback_kernel, dim3(FB_SPLIT, max(1, FB_CHUNKS / bt.n), bt.n), dim3(256), 0, st, bt);
    NM_LAUNCH_CHECK();
    hipLaunchKernelGGL(match_fallback_merge_kernel, dim3(8, bt.n), dim3(256), 0, st, bt);
    NM_LAUNCH_CHECK();
    return 0;
}

int run_distance(const float *A, int nA, const float *B, int nB, float *distance, const MatchWs &w, hipStream_t st)
{
    DistArgs a{};
    float *part = nullptr;
    const dim3 xgrid(nm_divup(nB, XD_TILE), nm_divup(nA, XD_TILE));
    if (distance_mode() == 0 || nA >= MATCH_MAX_ROWS || nB >= MATCH_MAX_ROWS || !distance_scratch(w, nA, a, &part)) {
        hipLaunchKernelGGL((exact_distance_kernel<false, false>), xgrid, dim3(256), 0, st, A, nA, B, nB, distance, (size_t)nB, nullptr, 0);
        NM_LAUNCH_CHECK();
        return 0;
    }
    a.ty = a.ny + nB;
    a.D = distance; a.ldd = (size_t)nB; a.nX = nA; a.nY = nB;
    a.fix_cap = distance_list_cap(a.fix_cap, nA, nB);
    hipLaunchKernelGGL(distance_colsum_kernel, dim3(DIST_P), dim3(128), 0, st, B, nB, part);
    NM_LAUNCH_CHECK();
    hipLaunchKernelGGL(distance_center_kernel, dim3(min(1024, nm_divup(max(nA, nB), 4)), 2), dim3(256), 0, st, A, nA, B, nB, part,
                       const_cast<float *>(a.Xc), const_cast<float *>(a.Yc), const_cast<float *>(a.nx), const_cast<float *>(a.ny),
                       const_cast<float *>(a.tx), const_cast<float *>(a.ty), a.fix_count);
    NM_LAUNCH_CHECK();
    const size_t lds_bytes = (size_t)2 * TILE_C * KP * sizeof(float) + 2 * TILE_C * sizeof(float);
    NM_RETURN_IF(hipFuncSetAttribute(reinterpret_cast<const void *>(distance_mfma_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds_bytes));
    const long long units = (long long)nm_divup(nA, TILE_C) * nm_divup(nB, QB);
    const int grid = (int)std::min<long long>(units, nm_cu_count());
    nm_prof_begin(NM_PROF_DISTANCE, st);
    hipLaunchKernelGGL(distance_mfma_kernel, dim3(grid), dim3(512), lds_bytes, st, a);
    nm_prof_end(NM_PROF_DISTANCE, st);
    NM_LAUNCH_CHECK();
    hipLaunchKernelGGL(distance_fixup_kernel, dim3(2048), dim3(256), 0, st, A, B, a);
    NM_LAUNCH_CHECK();
    // a list that overflowed (more 32 x 32 blocks with an entry outside the bound than the partial-list pool holds): the exact kernel fills the whole matrix;
    // otherwise its workgroups return at once
    hipLaunchKernelGGL((exact_distance_kernel<false, false>), xgrid, dim3(256), 0, st, A, nA, B, nB, distance, (size_t)nB,
                       a.fix_count, a.fix_cap);
    NM_LAUNCH_CHECK();
    return 0;
}

}  // namespace nm_match
using namespace nm_match;

extern "C" {

int nm_transpose_f32(float *odata, const float *idata, int width, int height, void *stream)
{
    if (width <= 0 || height <= 0) return 0;
    dim3 grid(nm_divup(width, 32), nm_divup(height, 32));
    hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, nm_stream(stream), odata, idata, width, height);
    NM_LAUNCH_CHECK();
    return 0;
}

int nm_bf_distance_f32(const float *A, int size_A, const float *B, int size_B, int sift_vector_size, float *result,
                       void *stream)
{
    if (sift_vector_size != DIM) return (int)hipErrorInvalidValue;
    if (size_A <= 0 || size_B <= 0) return 0;
    // rows of the (transposed) output = candidates j, columns = queries i: result[j * size_A + i]; A arrives k-major
    dim3 grid(nm_divup(size_A, XD_TILE), nm_divup(size_B, XD_TILE));
    hipLaunchKernelGGL((exact_distance_kernel<false, true>), grid, dim3(256), 0, nm_stream(stream), B, size_B, A, size_A,
                       result, (size_t)size_A, nullptr, 0);
    NM_LAUNCH_CHECK();
    return 0;
}

int nm_get_sift_matches_f32(const float *distance, int rows, int cols, int buffer_width, int *result, float ambiguity,
                            void *stream)
{
    if (rows <= 0 || cols <= 0) return 0;
    hipLaunchKernelGGL(set_matches_kernel, dim3(nm_divup(rows, 4)), dim3(256), 0, nm_stream(stream), result, distance,
                       rows, cols, buffer_width, ambiguity);
    NM_LAUNCH_CHECK();
    return 0;
}

float nm_sift_match_distance_budget(void) { return DIST_C; }

int nm_sift_match_set_distance_mode(int mode)
{
    if (mode < 0 || mode > 1) return (int)hipErrorInvalidValue;
    g_dist_mode.store(mode, std::memory_order_relaxed);
    return 0;
}
int nm_sift_match_get_distance_mode(void) { return distance_mode(); }
// Diagnostics: entries of the last MFMA distance pass on `workspace` (same nA, nB) that were listed for the exact recomputation,
// and the capacity of the list (more listed than that = the whole matrix was filled by the exact kernel). Synchronises.
int nm_sift_match_distance_listed(const void *workspace, int nA, int nB, int *listed, int *capacity, void *stream)
{
    if (!workspace || !listed || nA <= 0 || nB <= 0) return (int)hipErrorInvalidValue;
    DistArgs a{};
    float *part = nullptr;
    *listed = -1;
    if (capacity) *capacity = 0;
    if (!distance_scratch(carve(const_cast<void *>(workspace), nA, nB), nA, a, &part)) return 0;
    if (capacity) *capacity = distance_list_cap(a.fix_cap, nA, nB);
    NM_RETURN_IF(hipStreamSynchronize(nm_stream(stream)));
    return (int)hipMemcpy(listed, a.fix_report, sizeof(int), hipMemcpyDeviceToHost);
}

}  // extern "C"
