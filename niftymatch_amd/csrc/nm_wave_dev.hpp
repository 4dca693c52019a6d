// nm_wave_dev.hpp -- the cross-lane idioms of the kernels, each stated once (device only, no state): the xor butterfly, the
// shuffle scan and the ordered rank of a workgroup's flagged threads. Wave = 64 lanes; workgroups are one-dimensional, so a
// thread's lane is threadIdx.x & 63 and its wave threadIdx.x >> 6.
#pragma once
#include <hip/hip_runtime.h>

namespace nmw {

struct Sum { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct Max {
    template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return b > a ? b : a; }
    __device__ __forceinline__ int operator()(int a, int b) const { return max(a, b); }
    __device__ __forceinline__ float operator()(float a, float b) const { return __builtin_fmaxf(a, b); }
};
struct Min {
    template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return b < a ? b : a; }
    __device__ __forceinline__ int operator()(int a, int b) const { return min(a, b); }
    __device__ __forceinline__ float operator()(float a, float b) const { return __builtin_fminf(a, b); }
};

// v = op(v, v of lane ^ d) for d = FIRST, FIRST / 2, ..., 1: every lane of a group of 2 * FIRST lanes returns the group's
// result (FIRST = 32: the wave). The step order is part of a float or double result and is the same everywhere.
template <int FIRST = 32, class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op)
{
#pragma unroll
    for (int d = FIRST; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d));
    return v;
}
template <int FIRST = 32, class T> __device__ __forceinline__ T wave_sum(T v) { return wave_reduce<FIRST>(v, Sum()); }
template <class T> __device__ __forceinline__ T wave_max(T v) { return wave_reduce(v, Max()); }
template <class T> __device__ __forceinline__ T wave_min(T v) { return wave_reduce(v, Min()); }

// Sum of v over the lanes up to and including the own one (steps 1, 2, ..., 32).
template <class T>
__device__ __forceinline__ T wave_inclusive_scan(T v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T up = __shfl_up(v, d);
        if (lane >= d) v += up;
    }
    return v;
}

// Number of the wave's active lanes whose flag is set (every lane returns it): the sum of a flag without a butterfly.
__device__ __forceinline__ int wave_count(bool flag) { return __popcll(__ballot(flag)); }

// Set bits of a ballot below the own lane: the lane's rank among the wave's flagged lanes.
__device__ __forceinline__ int lane_rank(unsigned long long ballot)
{
    return __popcll(ballot & ((1ull << (threadIdx.x & 63)) - 1ull));
}

// Rank of this thread among the workgroup's flagged threads, in thread order, and their number (total), for a workgroup of
// WAVES waves; every thread calls it. s_cnt is the caller's int[WAVES] in LDS.
// Barriers: ONE, inside, between the waves' writes of s_cnt and the reads. There is none after the reads: s_cnt may be
// rewritten (the next call with the same s_cnt included) only after the caller's next barrier. Whatever else the caller
// stored to LDS before the call is visible to the workgroup on return.
template <int WAVES>
__device__ __forceinline__ int block_rank(bool flag, int *s_cnt, int &total)
{
    const unsigned long long m = __ballot(flag);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const int c = s_cnt[w];
        if (w < wave) before += c;
        total += c;
    }
    return before + lane_rank(m);
}

// The workgroup's totals of N per-lane sums, for a workgroup of WAVES waves; every thread calls it. Thread q < N returns
// the total of sum q (the other threads return T()). part is the caller's T[WAVES][N] in LDS. Barriers: ONE, inside,
// between the waves' writes of part and the reads. The wave step is the butterfly, the waves are added in ascending order.
template <int WAVES, int N, class T>
__device__ __forceinline__ T block_totals(T (&s)[N], T (*part)[N])
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int q = 0; q < N; ++q) s[q] = wave_reduce(s[q], Sum());
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < N; ++q) part[wave][q] = s[q];
    __syncthreads();
    T t = T();
    if (tid < N)
        for (int w = 0; w < WAVES; ++w) t += part[w][tid];
    return t;
}

}  // namespace nmw
