// nm_select.hip -- batched keypoint selection for gfx950 (no reference counterpart: the reference keeps the first
// `capacity` rows in octave / level / raster order, sift/siftdata.h:12-15). Strongest `keep` rows of each frame, spread over
// a gx x gy grid: every cell's best first, then every cell's second best, ... (include/nm_abi.h, nm_sift_select_batch_dev).
// FOUR launches for 1..64 frames, the frame a grid dimension, no allocation, no synchronisation, no host read:
//   1. score   one wave per row (one float2 per lane, the nmdf butterfly) or one lane per row when scores are given:
//              key[i] = (bits of u_i, ~i), cell[i];
//   2. group   one workgroup per frame: cell histogram in LDS (integer LDS atomics), exclusive scan, scatter of the keys into
//              cell segments (the order inside a segment is arbitrary and nothing depends on it), and the cut: with
//              f(R) = sum over cells of min(size, R) = rows of round < R, the last round R* with f(R*) <= count, found by
//              bisection over the cell sizes, and rem = count - f(R*) rows still to take from round R*;
//   3. round   one lane per row of the grouped order: r = keys of the own segment above the own key, counted through LDS tiles
//              of 1024 keys (a segment longer than a tile loops); flag 1 for r < R*, and the rows of round R* (at most one per
//              cell) are appended to the frame's list (integer atomic on the list length; the list's order is arbitrary);
//   4. gather  up to 64 workgroups per frame, each owning a range of output rows: the threshold key (the rem-th largest of
//              the list, by counting), a ballot scan over the flags in source order that finds the source rows of the own
//              range, then one wave per output row copies the payload.
// The tables of the payload exceed the 4 KB of kernel arguments (14 x 64 pointers), and launch 4 needs them all: launches
// 1-3 carry them in their own arguments and park each frame's pointers in the frame's workspace record, which launch 4 reads.
// No float atomics; every store is a vector store from plain C++.
#include <algorithm>
#include <vector>

#include "nm_common.hpp"
#include "nm_pair_batch.hpp"
#include "nm_select_math.hpp"
#include "../../include/nm_abi.h"

namespace {

constexpr int B = NM_SELECT_MAX_BATCH;
constexpr int TILE = 1024;                  // keys per LDS tile of the round kernel (8 KB)
constexpr int GROUP_TB = 1024, ROUND_TB = 256, GATHER_TB = 256, SCORE_TB = 256;
constexpr int GATHER_BLOCKS = 64;           // workgroups per frame at most
constexpr int GATHER_ROWS = nmsel::MAX_CAPACITY / GATHER_BLOCKS;   // output rows per workgroup at most (1024)
enum { M_ROUND = 0, M_REM = 1, M_COUNT = 2, M_LIST = 3, M_ROWS = 4, M_INTS = 8 };

struct FramePtrs {                          // a frame's payload, parked by launches 1-3 for launch 4
    const float *x, *y, *desc;
    const unsigned char *desc_u8;
    const float *kpts, *orients;
    float *out_x, *out_y, *out_desc;
    unsigned char *out_desc_u8;
    float *out_kpts, *out_orients;
    int *out_index, *d_out;
};

constexpr int PTRS_BYTES = 128;             // the record of the parked pointers
static_assert(sizeof(FramePtrs) <= PTRS_BYTES, "the parked pointers outgrow their record");

// A frame's part of the workspace (8-byte aligned, widest members first)
struct Frame {
    uint64_t *key, *skey, *list;            // source order; grouped by cell; the rows of round R*
    int *cstart, *meta;                     // MAX_CELLS + 1 segment starts; M_* ints
    FramePtrs *ptrs;
    unsigned short *cell;
    unsigned char *flag;                    // 0 out, 1 in, 2 round R*: in when the key reaches the threshold
    // The one layout: every member in order, each starting where the one before it ends (the element sizes only shrink, so
    // each is aligned). Sets the members when there is a base; returns the frame's stride, a multiple of 16 bytes.
    __host__ __device__ size_t layout(char *base, int cap)
    {
        size_t off = 0;
        auto take = [&](auto *&p, size_t bytes) {
            if (base) p = reinterpret_cast<decltype(+p)>(base + off);
            off += bytes;
        };
        take(key, (size_t)cap * 8);
        take(skey, (size_t)cap * 8);
        take(list, (size_t)nmsel::MAX_CELLS * 8);
        take(cstart, (size_t)(nmsel::MAX_CELLS + 8) * 4);
        take(meta, (size_t)M_INTS * 4);
        take(ptrs, PTRS_BYTES);
        take(cell, (size_t)cap * 2);
        take(flag, (size_t)cap);
        return (off + 15) / 16 * 16;
    }
    __host__ __device__ Frame(char *base, int cap)
    {
        __builtin_assume(base != nullptr);  // the entry refuses a null workspace: no test of base is left in a kernel
        layout(base, cap);
    }
    static __host__ __device__ size_t bytes(int cap) { Frame f; return f.layout(nullptr, cap); }

private:
    Frame() = default;
};

struct Geometry { int capacity, width, height, gx, gy, keep; };

struct ScoreArgs {                          // 6 x 64 pointers: 3 KB of kernel arguments
    const int *d_num[B];
    const float *x[B], *y[B], *scores[B], *desc[B];
    int *d_out[B];
};
struct GroupArgs {                          // 7 x 64 pointers: 3.5 KB
    const int *d_num[B];
    const float *x[B], *y[B], *desc[B];
    const unsigned char *desc_u8[B];
    const float *kpts[B], *orients[B];
};
struct RoundArgs {                          // 7 x 64 pointers: 3.5 KB
    float *out_x[B], *out_y[B], *out_desc[B];
    unsigned char *out_desc_u8[B];
    float *out_kpts[B], *out_orients[B];
    int *out_index[B];
};
static_assert(sizeof(ScoreArgs) + 64 < 4096 && sizeof(GroupArgs) + 64 < 4096 && sizeof(RoundArgs) + 64 < 4096,
              "select kernel arguments exceed 4 KB");

struct __attribute__((aligned(2))) U8x2 { unsigned char v[2]; };

__global__ __launch_bounds__(SCORE_TB) void select_score_kernel(const ScoreArgs a, const Geometry g, int by_desc, char *ws,
                                                                 size_t stride)
{
    const int k = blockIdx.y, lane = threadIdx.x & 63;
    const Frame f(ws + k * stride, g.capacity);
    if (blockIdx.x == 0 && threadIdx.x == 0) f.ptrs->d_out = a.d_out[k];
    const int m = nmp::clip(*a.d_num[k], g.capacity);
    const int row = by_desc ? blockIdx.x * (SCORE_TB / 64) + (threadIdx.x >> 6) : blockIdx.x * SCORE_TB + threadIdx.x;
    if (row >= m) return;                                            // by_desc: uniform over the wave
    float s;
    if (by_desc) {
        const float2 v = *reinterpret_cast<const float2 *>(a.desc[k] + (size_t)row * nmdf::DIM + 2 * lane);
        nmdf::LaneRow r;
        r.a[0] = v.x; r.b[0] = v.y;
        s = nmsel::raw_score(r);                                     // every lane holds the same sum
        if (lane != 0) return;
    } else {
        s = a.scores[k][row];
    }
    f.key[row] = nmsel::make_key(nmsel::rank_score(s), row);
    f.cell[row] = (unsigned short)nmsel::cell_of(a.x[k][row], a.y[k][row], g.width, g.height, g.gx, g.gy);
}

// Sum of v over the 1024 threads of the group kernel, the same value in every thread. Two barriers: red is free on return.
__device__ __forceinline__ int group_sum(int v, int *red)
{
    v = nmw::wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < GROUP_TB / 64; ++w) s += red[w];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(GROUP_TB) void select_group_kernel(const GroupArgs a, int capacity, int keep, char *ws, size_t stride)
{
    __shared__ int size[nmsel::MAX_CELLS], cursor[nmsel::MAX_CELLS], red[GROUP_TB / 64];
    constexpr int PER = nmsel::MAX_CELLS / GROUP_TB;                 // four consecutive cells per thread
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Frame f(ws + k * stride, capacity);
    if (tid == 0) {
        FramePtrs *p = f.ptrs;
        p->x = a.x[k]; p->y = a.y[k]; p->desc = a.desc[k]; p->desc_u8 = a.desc_u8[k]; p->kpts = a.kpts[k]; p->orients = a.orients[k];
    }
    const int m = nmp::clip(*a.d_num[k], capacity);
    for (int c = tid; c < nmsel::MAX_CELLS; c += GROUP_TB) size[c] = 0;
    __syncthreads();
    for (int i = tid; i < m; i += GROUP_TB) atomicAdd(&size[f.cell[i]], 1);
    __syncthreads();

    // exclusive scan of the sizes: own four, a shuffle scan over the wave, the waves' totals through LDS
    int own[PER], local = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) { own[j] = size[PER * tid + j]; local += own[j]; }
    const int incl = nmw::wave_inclusive_scan(local);
    if (lane == 63) red[wave] = incl;
    __syncthreads();
    int start = incl - local;
    for (int w = 0; w < wave; ++w) start += red[w];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        cursor[PER * tid + j] = start;
        f.cstart[PER * tid + j] = start;
        start += own[j];
    }
    if (tid == GROUP_TB - 1) f.cstart[nmsel::MAX_CELLS] = start;     // = m

    // the cut: the last R in [0, capacity] with f(R) <= count; f(0) = 0, f grows with R and f(capacity) = m
    const int count = keep < m ? keep : m;
    int lo = 0, f_lo = 0, hi = capacity + 1;
    while (hi - lo > 1) {                                            // uniform: at most 17 rounds
        const int mid = lo + (hi - lo) / 2;
        int part = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) part += own[j] < mid ? own[j] : mid;
        const int below = group_sum(part, red);
        if (below <= count) { lo = mid; f_lo = below; } else hi = mid;
    }
    if (tid == 0) {
        f.meta[M_ROUND] = lo; f.meta[M_REM] = count - f_lo; f.meta[M_COUNT] = count; f.meta[M_LIST] = 0; f.meta[M_ROWS] = m;
    }
    __syncthreads();                                                 // cursor is complete
    for (int i = tid; i < m; i += GROUP_TB) {
        const int at = atomicAdd(&cursor[f.cell[i]], 1);             // < the next segment's start <= m
        f.skey[at] = f.key[i];
    }
}

__global__ __launch_bounds__(ROUND_TB) void select_round_kernel(const RoundArgs a, int capacity, char *ws, size_t stride)
{
    __shared__ uint64_t tile[TILE];
    __shared__ int range[2];
    const int k = blockIdx.y, tid = threadIdx.x;
    const Frame f(ws + k * stride, capacity);
    if (blockIdx.x == 0 && tid == 0) {
        FramePtrs *p = f.ptrs;
        p->out_x = a.out_x[k]; p->out_y = a.out_y[k]; p->out_desc = a.out_desc[k]; p->out_desc_u8 = a.out_desc_u8[k];
        p->out_kpts = a.out_kpts[k]; p->out_orients = a.out_orients[k]; p->out_index = a.out_index[k];
    }
    const int m = f.meta[M_ROWS], first = blockIdx.x * ROUND_TB;
    if (first >= m) return;                                          // uniform over the workgroup
    const int at = first + tid;
    const bool live = at < m;
    uint64_t key = 0;
    int src = 0, lo = 0, hi = 0;
    if (live) {
        key = f.skey[at];
        src = nmsel::key_row(key);
        const int c = f.cell[src];
        lo = f.cstart[c]; hi = f.cstart[c + 1];
    }
    if (tid == 0) range[0] = lo;                                     // segments are in cell order: the first row's start and
    if (live && (at == m - 1 || tid == ROUND_TB - 1)) range[1] = hi; // the last row's end enclose every row's segment
    __syncthreads();
    const int r_lo = range[0], r_hi = range[1];
    int r = 0;
    for (int t0 = r_lo; t0 < r_hi; t0 += TILE) {
        for (int j = tid; j < TILE && t0 + j < r_hi; j += ROUND_TB) tile[j] = f.skey[t0 + j];
        __syncthreads();
        const int from = lo > t0 ? lo : t0, to = hi < t0 + TILE ? hi : t0 + TILE;
        for (int j = from; j < to; ++j) r += tile[j - t0] > key;
        __syncthreads();
    }
    if (!live) return;
    const int cut = f.meta[M_ROUND], rem = f.meta[M_REM];
    const int flag = r < cut ? 1 : (r == cut && rem > 0 ? 2 : 0);
    f.flag[src] = (unsigned char)flag;
    if (flag == 2) {
        const int e = atomicAdd(&f.meta[M_LIST], 1);                 // one row per cell at the most
        if (e < nmsel::MAX_CELLS) f.list[e] = key;
    }
}

__global__ __launch_bounds__(GATHER_TB) void select_gather_kernel(int capacity, int rows_per_block, char *ws, size_t stride)
{
    __shared__ uint64_t list[nmsel::MAX_CELLS];
    __shared__ uint64_t threshold;
    __shared__ int sel[GATHER_ROWS], wave_count[GATHER_TB / 64];
    const int k = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Frame f(ws + k * stride, capacity);
    const FramePtrs P = *f.ptrs;
    const int count = f.meta[M_COUNT], m = f.meta[M_ROWS], t0 = blockIdx.x * rows_per_block;
    if (blockIdx.x == 0 && tid == 0) *P.d_out = count;
    if (t0 >= count) return;                                         // uniform over the workgroup
    const int t1 = t0 + rows_per_block < count ? t0 + rows_per_block : count;

    // the rem-th largest key of round R*: the one with rem - 1 keys above it (keys are distinct, rem < list length)
    const int rem = f.meta[M_REM];
    const int len = f.meta[M_LIST] < nmsel::MAX_CELLS ? f.meta[M_LIST] : nmsel::MAX_CELLS;
    if (tid == 0) threshold = ~(uint64_t)0;
    if (rem > 0) {
        for (int e = tid; e < len; e += GATHER_TB) list[e] = f.list[e];
        __syncthreads();
        for (int e = tid; e < len; e += GATHER_TB) {
            const uint64_t mine = list[e];
            int above = 0;
            for (int j = 0; j < len; ++j) above += list[j] > mine;
            if (above == rem - 1) threshold = mine;
        }
    }
    __syncthreads();
    const uint64_t thr = threshold;

    // output position of every selected row, in source order; the rows of the own range go to sel
    for (int e = tid; e < GATHER_ROWS; e += GATHER_TB) sel[e] = -1;
    __syncthreads();
    int base = 0;
    for (int c0 = 0; c0 < m && base < t1; c0 += GATHER_TB) {
        const int i = c0 + tid;
        bool in = false;
        if (i < m) {
            const int flag = f.flag[i];
            in = flag == 1 || (flag == 2 && f.key[i] >= thr);
        }
        int total;
        const int pos = base + nmw::block_rank<GATHER_TB / 64>(in, wave_count, total);
        if (in && pos >= t0 && pos < t1) sel[pos - t0] = i;
        base += total;
        __syncthreads();                                             // wave_count is rewritten by the next chunk
    }

    for (int t = t0 + wave; t < t1; t += GATHER_TB / 64) {           // one wave per output row
        const int i = sel[t - t0];
        if (i < 0) continue;                                         // never: exactly `count` rows are selected
        if (P.desc) {
            const size_t from = (size_t)i * nmdf::DIM + 2 * lane, to = (size_t)t * nmdf::DIM + 2 * lane;
            *reinterpret_cast<float2 *>(P.out_desc + to) = *reinterpret_cast<const float2 *>(P.desc + from);
        }
        if (P.desc_u8) {
            const size_t from = (size_t)i * nmdf::DIM + 2 * lane, to = (size_t)t * nmdf::DIM + 2 * lane;
            *reinterpret_cast<U8x2 *>(P.out_desc_u8 + to) = *reinterpret_cast<const U8x2 *>(P.desc_u8 + from);
        }
        if (P.kpts && lane < 4) P.out_kpts[(size_t)t * 4 + lane] = P.kpts[(size_t)i * 4 + lane];
        if (P.orients && lane < 2) P.out_orients[(size_t)t * 2 + lane] = P.orients[(size_t)i * 2 + lane];
        if (lane == 0) {
            P.out_x[t] = P.x[i];
            P.out_y[t] = P.y[i];
            if (P.out_index) P.out_index[t] = i;
        }
    }
}

struct Tables {
    const int *const *num;
    const float *const *x, *const *y, *const *scores, *const *desc;
    const unsigned char *const *desc_u8;
    const float *const *kpts, *const *orients;
    float *const *out_x, *const *out_y, *const *out_desc;
    unsigned char *const *out_desc_u8;
    float *const *out_kpts, *const *out_orients;
    int *const *out_index, *const *out_items;
};

template <class I, class O> bool pair_ok(int n, I *const *in, O *const *out)
{
    if ((in == nullptr) != (out == nullptr)) return false;
    for (int k = 0; in && k < n; ++k)
        if (static_cast<const void *>(in[k]) == static_cast<const void *>(out[k])) return false;
    return true;
}

bool select_args_ok(int n, const Geometry &g, const Tables &t)
{
    if (n < 1 || n > B || g.capacity < 1 || g.capacity > nmsel::MAX_CAPACITY) return false;
    if (g.gx < 1 || g.gx > nmsel::MAX_GRID || g.gy < 1 || g.gy > nmsel::MAX_GRID) return false;
    if (g.keep < 1 || g.keep > g.capacity || g.width < 1 || g.height < 1) return false;
    if (!t.scores && !t.desc) return false;
    if (!nmp::tables_ok(n, {t.num, t.x, t.y, t.out_x, t.out_y, t.out_items},
                        {t.scores, t.desc, t.desc_u8, t.kpts, t.orients, t.out_desc, t.out_desc_u8, t.out_kpts, t.out_orients,
                         t.out_index}, {}))
        return false;
    return pair_ok(n, t.x, t.out_x) && pair_ok(n, t.y, t.out_y) && pair_ok(n, t.desc, t.out_desc) &&
           pair_ok(n, t.desc_u8, t.out_desc_u8) && pair_ok(n, t.kpts, t.out_kpts) && pair_ok(n, t.orients, t.out_orients);
}

}  // namespace

extern "C" size_t nm_sift_select_workspace_bytes(int n, int capacity, int gx, int gy)
{
    if (n < 1 || n > B || capacity < 1 || capacity > nmsel::MAX_CAPACITY) return 0;
    if (gx < 1 || gx > nmsel::MAX_GRID || gy < 1 || gy > nmsel::MAX_GRID) return 0;
    return (size_t)n * Frame::bytes(capacity);
}

extern "C" int nm_sift_select_batch_dev(int n, int capacity, int width, int height, int gx, int gy, int keep,
                                        const int *const *d_num_items, const float *const *x, const float *const *y,
                                        const float *const *scores, const float *const *desc,
                                        const unsigned char *const *desc_u8, const float *const *kpts,
                                        const float *const *orients, float *const *out_x, float *const *out_y,
                                        float *const *out_desc, unsigned char *const *out_desc_u8, float *const *out_kpts,
                                        float *const *out_orients, int *const *out_index, int *const *d_out_items,
                                        void *workspace, void *stream)
{
    const Geometry g = {capacity, width, height, gx, gy, keep};
    const Tables t = {d_num_items, x, y, scores, desc, desc_u8, kpts, orients, out_x, out_y, out_desc, out_desc_u8, out_kpts,
                      out_orients, out_index, d_out_items};
    if (!select_args_ok(n, g, t) || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 7)) return (int)hipErrorInvalidValue;
    char *ws = static_cast<char *>(workspace);
    const size_t stride = Frame::bytes(capacity);
    hipStream_t st = nm_stream(stream);
    const int by_desc = scores ? 0 : 1;

    ScoreArgs sa;
    nmp::fill_slots(sa.d_num, d_num_items, 0, n); nmp::fill_slots(sa.x, x, 0, n); nmp::fill_slots(sa.y, y, 0, n);
    nmp::fill_slots(sa.scores, scores, 0, n); nmp::fill_slots(sa.desc, desc, 0, n); nmp::fill_slots(sa.d_out, d_out_items, 0, n);
    hipLaunchKernelGGL(select_score_kernel, dim3(nm_divup(capacity, by_desc ? SCORE_TB / 64 : SCORE_TB), n), dim3(SCORE_TB), 0, st,
                       sa, g, by_desc, ws, stride);
    NM_LAUNCH_CHECK();

    GroupArgs ga;
    nmp::fill_slots(ga.d_num, d_num_items, 0, n); nmp::fill_slots(ga.x, x, 0, n); nmp::fill_slots(ga.y, y, 0, n);
    nmp::fill_slots(ga.desc, desc, 0, n); nmp::fill_slots(ga.desc_u8, desc_u8, 0, n); nmp::fill_slots(ga.kpts, kpts, 0, n);
    nmp::fill_slots(ga.orients, orients, 0, n);
    hipLaunchKernelGGL(select_group_kernel, dim3(n), dim3(GROUP_TB), 0, st, ga, capacity, keep, ws, stride);
    NM_LAUNCH_CHECK();

    RoundArgs ra;
    nmp::fill_slots(ra.out_x, out_x, 0, n); nmp::fill_slots(ra.out_y, out_y, 0, n); nmp::fill_slots(ra.out_desc, out_desc, 0, n);
    nmp::fill_slots(ra.out_desc_u8, out_desc_u8, 0, n); nmp::fill_slots(ra.out_kpts, out_kpts, 0, n);
    nmp::fill_slots(ra.out_orients, out_orients, 0, n); nmp::fill_slots(ra.out_index, out_index, 0, n);
    hipLaunchKernelGGL(select_round_kernel, dim3(nm_divup(capacity, ROUND_TB), n), dim3(ROUND_TB), 0, st, ra, capacity, ws, stride);
    NM_LAUNCH_CHECK();

    const int blocks = std::min(GATHER_BLOCKS, nm_divup(keep, 64));
    hipLaunchKernelGGL(select_gather_kernel, dim3(blocks, n), dim3(GATHER_TB), 0, st, capacity, nm_divup(keep, blocks), ws, stride);
    NM_LAUNCH_CHECK();
    return 0;
}

// The host twin: the same score, cell and key functions, the rule itself by two sorts
extern "C" int nm_sift_select_host(int n, int capacity, int width, int height, int gx, int gy, int keep,
                                   const int *const *num_items, const float *const *x, const float *const *y,
                                   const float *const *scores, const float *const *desc, const unsigned char *const *desc_u8,
                                   const float *const *kpts, const float *const *orients, float *const *out_x,
                                   float *const *out_y, float *const *out_desc, unsigned char *const *out_desc_u8,
                                   float *const *out_kpts, float *const *out_orients, int *const *out_index,
                                   int *const *out_items)
{
    const Geometry g = {capacity, width, height, gx, gy, keep};
    const Tables t = {num_items, x, y, scores, desc, desc_u8, kpts, orients, out_x, out_y, out_desc, out_desc_u8, out_kpts,
                      out_orients, out_index, out_items};
    if (!select_args_ok(n, g, t)) return (int)hipErrorInvalidValue;
    struct Item { uint64_t key; int cell, round; };
    for (int k = 0; k < n; ++k) {
        const int m = nmp::clip(*num_items[k], capacity), count = std::min(keep, m);
        std::vector<Item> rows(m);
        for (int i = 0; i < m; ++i) {
            float s;
            if (scores) s = scores[k][i];
            else {
                nmdf::HostRow r;
                for (int l = 0; l < nmdf::PAIRS; ++l) { r.a[l] = desc[k][(size_t)i * nmdf::DIM + 2 * l]; r.b[l] = desc[k][(size_t)i * nmdf::DIM + 2 * l + 1]; }
                s = nmsel::raw_score(r);
            }
            rows[i] = {nmsel::make_key(nmsel::rank_score(s), i), nmsel::cell_of(x[k][i], y[k][i], width, height, gx, gy), 0};
        }
        std::sort(rows.begin(), rows.end(), [](const Item &p, const Item &q) { return p.cell != q.cell ? p.cell < q.cell : p.key > q.key; });
        for (int i = 0, r = 0; i < m; ++i) { r = (i > 0 && rows[i].cell == rows[i - 1].cell) ? r + 1 : 0; rows[i].round = r; }
        std::sort(rows.begin(), rows.end(), [](const Item &p, const Item &q) { return p.round != q.round ? p.round < q.round : p.key > q.key; });
        std::vector<int> chosen(count);
        for (int e = 0; e < count; ++e) chosen[e] = nmsel::key_row(rows[e].key);
        std::sort(chosen.begin(), chosen.end());
        for (int e = 0; e < count; ++e) {
            const int i = chosen[e];
            out_x[k][e] = x[k][i];
            out_y[k][e] = y[k][i];
            if (desc) std::copy(desc[k] + (size_t)i * nmdf::DIM, desc[k] + (size_t)(i + 1) * nmdf::DIM, out_desc[k] + (size_t)e * nmdf::DIM);
            if (desc_u8) std::copy(desc_u8[k] + (size_t)i * nmdf::DIM, desc_u8[k] + (size_t)(i + 1) * nmdf::DIM, out_desc_u8[k] + (size_t)e * nmdf::DIM);
            if (kpts) std::copy(kpts[k] + (size_t)i * 4, kpts[k] + (size_t)(i + 1) * 4, out_kpts[k] + (size_t)e * 4);
            if (orients) std::copy(orients[k] + (size_t)i * 2, orients[k] + (size_t)(i + 1) * 2, out_orients[k] + (size_t)e * 2);
            if (out_index) out_index[k][e] = i;
        }
        *out_items[k] = count;
    }
    return 0;
}
