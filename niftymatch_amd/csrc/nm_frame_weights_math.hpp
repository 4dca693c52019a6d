// nm_frame_weights_math.hpp -- the arithmetic of the frame-weights stage (include/nm_abi.h, "Frame masks and feather
// weights"), shared by the kernels of nm_frame_weights.hip and their host twin: the photometric test, the 3 x 3 count on
// rows of bits, the seed rule, the horizontal distance g from three 64-bit seed words, the column recurrence of the clipped
// squared distance D and the weight. Everything up to D is integer; the weight is one fp32 square root, one subtraction and
// one division, each rounded on its own (-ffp-contract=off, -fhip-fp32-correctly-rounded-divide-sqrt), so device and host
// agree bit for bit.
//   Rows of bits. A row of a plane of flags is kept as 64-bit words: bit i of word b is pixel x = 64 b + i. Pixels outside
//   the frame are 0 bits, and so are whole words outside it.
#pragma once
#include <hip/hip_runtime.h>

namespace nmfw {

constexpr int MAX_FRAMES = 64;                  // NM_FRAME_WEIGHTS_MAX_BATCH
constexpr int MAX_RADIUS = 64;                  // NM_FRAME_WEIGHTS_MAX_RADIUS: three words hold every seed within it

// raw-bad: darker than lo (outside the optics) or brighter than hi (saturated); alpha plays no part
__host__ __device__ __forceinline__ bool raw_bad(int b, int g, int r, int lo, int hi)
{
    const int bg = b > g ? b : g, mx = bg > r ? bg : r;
    return mx < lo || mx > hi;
}

// how many of the pixels x - 1, x, x + 1 of one row are flagged, for x = 64 b + lane: `left`, `mid`, `right` are the words
// b - 1, b, b + 1 of that row
__host__ __device__ __forceinline__ int row3(unsigned long long left, unsigned long long mid, unsigned long long right,
                                             int lane)
{
    const int l = (int)((lane ? mid >> (lane - 1) : left >> 63) & 1ull);
    const int c = (int)((mid >> lane) & 1ull);
    const int r = (int)((lane < 63 ? mid >> (lane + 1) : right) & 1ull);
    return l + c + r;
}

// the seed rule: base says "not scene" unconditionally; a raw-bad pixel needs min_count raw-bad pixels in its 3 x 3 window
__host__ __device__ __forceinline__ bool seed_rule(bool base_zero, bool bad, int count, int min_count)
{
    return base_zero || (bad && count >= min_count);
}

// g = min(R + 1, distance along the row from x = 64 b + lane to the nearest seed), from the seed words b - 1, b, b + 1 of
// the row. R <= 64, so no seed that matters lies outside them.
__host__ __device__ __forceinline__ int g_of(unsigned long long left, unsigned long long mid, unsigned long long right,
                                             int lane, int R)
{
    int g = R + 1;
    const unsigned long long at_or_below = mid << (63 - lane);          // bit 63 is x itself, bit 63 - d is x - d
    const unsigned long long at_or_above = mid >> lane;                 // bit 0 is x itself, bit d is x + d
    int d = R + 1;
    if (at_or_below) d = __builtin_clzll(at_or_below);
    else if (left) d = lane + 1 + __builtin_clzll(left);
    g = d < g ? d : g;
    d = R + 1;
    if (at_or_above) d = __builtin_ctzll(at_or_above);
    else if (right) d = 64 - lane + __builtin_ctzll(right);
    return d < g ? d : g;
}

// with `border`, the lattice points left and right of the frame are seeds too
__host__ __device__ __forceinline__ int g_border(int g, int x, int fw)
{
    const int l = x + 1, r = fw - x, lr = l < r ? l : r;
    return lr < g ? lr : g;
}

// D over the rows y + dy, |dy| <= R: starts from the own row, then one step per dy with the rows above and below (a row
// outside the frame enters as g = R + 1, which cannot lower D). A step with dy * dy >= D cannot lower D either, so a walk
// may stop there.
__host__ __device__ __forceinline__ int d_init(int g, int R2)
{
    const int s = g * g;
    return s < R2 ? s : R2;
}

__host__ __device__ __forceinline__ int d_step(int best, int dy, int g_above, int g_below)
{
    const int m = g_above < g_below ? g_above : g_below, s = dy * dy + m * m;
    return s < best ? s : best;
}

// with `border`, the lattice points above and below the frame are seeds too
__host__ __device__ __forceinline__ int d_border(int best, int y, int fh)
{
    const int t = (y + 1) * (y + 1), b = (fh - y) * (fh - y), tb = t < b ? t : b;
    return tb < best ? tb : best;
}

__host__ __device__ __forceinline__ bool valid(int D, int margin) { return D > margin * margin; }

// (sqrtf(D) - margin) / (R - margin) in fp32, three roundings, no fma; 0 where the pixel is not valid
__host__ __device__ __forceinline__ float weight_of(int D, int margin, int R)
{
    if (!valid(D, margin)) return 0.f;
    const float s = __builtin_sqrtf((float)D);
    const float a = s - (float)margin;
    return a / (float)(R - margin);
}

}  // namespace nmfw
