// nm_select_math.hpp -- the per-row rules of the keypoint selection (include/nm_abi.h, nm_sift_select_batch_dev), written
// once for the kernels and the host twin: the default score (step 1 of the descriptor finish on nmdf's rows and butterfly),
// the usable-score rule, the pixel and cell of a coordinate, and the 64-bit key whose unsigned order is "beats". Compiled
// with -ffp-contract=off (nm_fpspec.hpp), fused only where fmaf is written, so the 128-element sum agrees bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nm_desc_finish_math.hpp"

namespace nmsel {

constexpr int MAX_GRID = 64;                    // cells per axis
constexpr int MAX_CELLS = MAX_GRID * MAX_GRID;  // 4096: one LDS histogram (16 KB)
constexpr int MAX_CAPACITY = 65536;             // rows per frame: bounds the one-cell worst case (capacity^2 key compares)

// s = sum(fmaf(v[2l+1], v[2l+1], v[2l] * v[2l])): the squared norm of the raw histogram, nmdf::l2_normalise's sum
template <class Row> __host__ __device__ __forceinline__ float raw_score(const Row &r)
{
    float p[Row::N];
    for (int l = 0; l < Row::N; ++l) p[l] = __builtin_fmaf(r.b[l], r.b[l], r.a[l] * r.a[l]);
    return r.sum(p);
}

// u = s where s > 0 and finite, else +0: NaN, negatives, zeros and infinities rank last, and u >= +0 always
__host__ __device__ __forceinline__ float rank_score(float s) { return nmdf::usable(s) ? s : 0.0f; }

// The pixel of a coordinate: 0 unless v >= 0 (NaN included), size - 1 from v >= size on, else (int)v
__host__ __device__ __forceinline__ int pixel(float v, int size)
{
    if (!(v >= 0.0f)) return 0;
    if (v >= 2147483648.0f) return size - 1;    // (int)v is not defined up there
    const int p = (int)v;                       // v >= size exactly when (int)v >= size: size is an integer
    return p >= size ? size - 1 : p;
}

__host__ __device__ __forceinline__ int cell_of(float x, float y, int width, int height, int gx, int gy)
{
    const int cw = (width + gx - 1) / gx, ch = (height + gy - 1) / gy;
    return (pixel(y, height) / ch) * gx + pixel(x, width) / cw;
}

// Row i beats row j exactly when key(u_i, i) > key(u_j, j) as unsigned integers: u >= +0, so its bits order like its
// value, and the complemented index makes the earlier row the larger key among equal scores. Keys of one frame are distinct.
__host__ __device__ __forceinline__ uint64_t make_key(float u, int i)
{
    return ((uint64_t)__builtin_bit_cast(uint32_t, u) << 32) | (uint32_t)~(uint32_t)i;
}
__host__ __device__ __forceinline__ int key_row(uint64_t key) { return (int)~(uint32_t)key; }

}  // namespace nmsel
