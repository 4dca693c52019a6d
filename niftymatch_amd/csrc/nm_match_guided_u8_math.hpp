// nm_match_guided_u8_math.hpp -- the distance and the row policy of homography-guided matching over unsigned-char descriptors
// (nm_sift_match_guided_u8_batch_dev and its host twin, nm_match_guided.hip), for gfx950. No reference counterpart. Projection, gate and scan are
// nm_match_guided_math.hpp as they are; what is new is d(i, j) = sum over q of (A[i][q] - B[j][q])^2 as an exact integer,
// formed as |a|^2 + |b|^2 - 2 a.b from dot products of four bytes at a time: v_dot4_u32_u8 on the device, a plain loop on
// the host. Every term is an integer <= 128 * 255^2 = 8 323 200 < 2^23, so the unsigned 32-bit sum is exact in any order,
// the host and the device agree, and (float)d is exact: the value the fp32 entry's fmaf chain reaches on float copies of the
// same bytes (differences <= 255, partial sums < 2^24: every step of that chain is exact).
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>

namespace nmg8 {

constexpr int DIM = 128;                    // bytes per row
constexpr int QUADS = DIM / 16;             // 16-byte parts per row
static_assert(DIM * 255 * 255 < (1 << 23), "a distance and each of its three terms is an exact float");

struct Row { uint4 q[QUADS]; };             // one row: 32 dwords, registers on the device

/* acc + a0 b0 + a1 b1 + a2 b2 + a3 b3 over the four bytes of a and b */
__host__ __device__ __forceinline__ unsigned dot4(unsigned a, unsigned b, unsigned acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(a, b, acc, false);
#else
    for (int s = 0; s < 32; s += 8) acc += ((a >> s) & 255u) * ((b >> s) & 255u);
    return acc;
#endif
}

/* The device reads a row as eight 16-byte loads (the entry's alignment rule); the host has no alignment rule */
__host__ __device__ __forceinline__ void load_row(Row &r, const unsigned char *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int q = 0; q < QUADS; ++q) r.q[q] = reinterpret_cast<const uint4 *>(p)[q];
#else
    std::memcpy(&r, p, sizeof r);
#endif
}

__host__ __device__ __forceinline__ unsigned norm2(const Row &a)
{
    unsigned s0 = 0, s1 = 0;
#pragma unroll
    for (int q = 0; q < QUADS; ++q) {
        s0 = dot4(a.q[q].x, a.q[q].x, s0); s1 = dot4(a.q[q].y, a.q[q].y, s1);
        s0 = dot4(a.q[q].z, a.q[q].z, s0); s1 = dot4(a.q[q].w, a.q[q].w, s1);
    }
    return s0 + s1;
}

/* d = |a|^2 + |b|^2 - 2 a.b with aa = norm2(a) formed once per row of A; |b|^2 inline. Two chains per sum: the order is free */
__host__ __device__ __forceinline__ unsigned distance(const Row &a, unsigned aa, const Row &b)
{
    unsigned ab0 = 0, ab1 = 0, bb0 = 0, bb1 = 0;
#pragma unroll
    for (int q = 0; q < QUADS; ++q) {
        ab0 = dot4(a.q[q].x, b.q[q].x, ab0); bb0 = dot4(b.q[q].x, b.q[q].x, bb0);
        ab1 = dot4(a.q[q].y, b.q[q].y, ab1); bb1 = dot4(b.q[q].y, b.q[q].y, bb1);
        ab0 = dot4(a.q[q].z, b.q[q].z, ab0); bb0 = dot4(b.q[q].z, b.q[q].z, bb0);
        ab1 = dot4(a.q[q].w, b.q[q].w, ab1); bb1 = dot4(b.q[q].w, b.q[q].w, bb1);
    }
    return aa + (bb0 + bb1) - 2u * (ab0 + ab1);
}

/* u8 rows as the guided kernel and its host twin see them (the fp32 rows: nmg::RowsF32). A lane keeps its own row, read
 * once (a row that is not valid: never, it stays zero), and |a|^2; (float)d is exact */
struct RowsU8 {
    using Elem = unsigned char;
    struct Own { Row row; unsigned aa; };
    __host__ __device__ __forceinline__ static void own(Own &o, const unsigned char *A, int i, bool valid)
    {
        o.row = {};
        if (valid) load_row(o.row, A + (size_t)i * DIM);
        o.aa = norm2(o.row);
    }
    __host__ __device__ __forceinline__ static float distance(const Own &o, const unsigned char *B, int j)
    {
        Row b;
        load_row(b, B + (size_t)j * DIM);
        return (float)nmg8::distance(o.row, o.aa, b);
    }
};

}  // namespace nmg8
