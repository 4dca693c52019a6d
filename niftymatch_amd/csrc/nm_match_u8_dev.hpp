// nm_match_u8_dev.hpp -- what the two users of v_mfma_i32_32x32x32_i8 on unsigned-char descriptors share (nm_match_u8.hip, the
// matcher, and nm_match_mutual_u8.hip, the mutual filter): the operand fragments of a 128-byte row (bytes - 128 as signed
// i8), the integer row norm |row - 128|^2, the norm of a row that does not exist, and the alignment test of the entries.
// A fragment is one lane's share of a row for the four k steps of a 32 x 32 x 128 product: lane (r = lane & 31, h = lane >>
// 5) holds bytes 32 t + 16 h .. + 15 of row r in step t. The accumulator holds the B operand's row on its column (lane & 31)
// and the A operand's rows (e & 3) + 8 (e >> 2) + 4 (lane >> 5) in its 16 registers e (tools/micro/mfma_i8_model.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace nmu8 {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int DIM = 128;
constexpr int TILE = 32;                    // rows of the A operand per MFMA tile
constexpr int PAD_NORM = 1 << 25;           // norm of a streamed row that does not exist: d >= 2^25 - 2^22 > 2^23
constexpr int KEY_INF = 0x7fffffff;
static_assert(DIM * 255 * 255 < (1 << 23) && ((PAD_NORM + (1 << 23)) >> 27) == 0, "keys (d << 4 | e) stay positive ints");

__device__ __forceinline__ int row_norm(const unsigned char *__restrict__ row)
{
    int s = 0;
#pragma unroll
    for (int q = 0; q < DIM / 16; ++q) {
        const uint4 u = reinterpret_cast<const uint4 *>(row)[q];
        const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int v = (int)((w[e] >> (8 * b)) & 255u) - 128;
                s += v * v;
            }
    }
    return s;
}

struct Frag { i32x4 s[4]; };                // one lane's 4 k steps of a row: bytes 32 t + 16 h .. + 15, minus 128

__device__ __forceinline__ Frag load_frag(const unsigned char *__restrict__ row, int h)
{
    Frag f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const i32x4 u = *reinterpret_cast<const i32x4 *>(row + 32 * t + 16 * h);
        f.s[t] = u ^ (int)0x80808080;       // byte - 128 as a signed byte
    }
    return f;
}

struct Norm16 { i32x4 g[4]; };              // the tile's 16 streamed-row norms of this lane half: rows 8 g + 4 h + 0..3

__device__ __forceinline__ Norm16 load_norms(const int *__restrict__ nb, int c0, int h)
{
    Norm16 n;
#pragma unroll
    for (int g = 0; g < 4; ++g) n.g[g] = *reinterpret_cast<const i32x4 *>(nb + c0 + 8 * g + 4 * h);
    return n;
}

inline bool aligned16(int n, const unsigned char *const *t)
{
    for (int k = 0; k < n; ++k)
        if (reinterpret_cast<uintptr_t>(t[k]) & 15u) return false;
    return true;
}

}  // namespace nmu8
