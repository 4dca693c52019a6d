// nm_match_u8_dev.hpp -- what the users of v_mfma_i32_32x32x32_i8 on unsigned-char descriptors share (the matcher and
// the k-NN entry, which are one scan kernel with two outputs in nm_match_u8.hip, the mutual filter's scan in
// nm_match_mutual_u8.hip, and the all-pairs vote scan in nm_link_propose.hip): the operand fragments of a 128-byte row (bytes - 128 as signed i8), the integer row norm
// |row - 128|^2, the norm of a row that does not exist, the alignment test of the entries, the tile stream of their hot
// kernels, and the plain integer distance of two rows that their host twins use.
// A fragment is one lane's share of a row for the four k steps of a 32 x 32 x 128 product: lane (r = lane & 31, h = lane >>
// 5) holds bytes 32 t + 16 h .. + 15 of row r in step t. The accumulator holds the B operand's row on its column (lane & 31)
// and the A operand's rows (e & 3) + 8 (e >> 2) + 4 (lane >> 5) in its 16 registers e (tools/micro/mfma_i8_model.hip).
// The tile stream: a wave owns QW = 64 items (queries, or compacted claims) as QG = 2 groups of 32, lane r of group g standing
// for item first + 32 g + r (last_real keeps a lane past the end on the last item; such a lane stores nothing), and holds
// their fragments Frag qf[QG] in 32 registers as the B operand. for_tiles streams the other side's rows in tiles of 32 as the
// A operand straight from global memory, the next tile and its norms requested before this one is used; per tile the kernel's
// body takes tile_product(cf, qf[g]) (a.b of 32 x 32 rows over the 4 k steps) and decodes a register with acc_row. What a
// kernel makes of the 16 accumulators (an ordered list of the best few, a threshold test) is its own. The ratio test's pieces
// (the top-2 fold of a tile's keys, the last step emit_u8 and their constants) are here for the matcher and the vote scan.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace nmu8 {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int DIM = 128;
constexpr int TILE = 32;                    // rows of the A operand per MFMA tile
constexpr int TB = 256;                     // four waves
constexpr int QG = 2;                       // item groups of 32 per wave
constexpr int QW = 32 * QG;                 // items per wave
constexpr int PAD_NORM = 1 << 25;           // norm of a streamed row that does not exist: d >= 2^25 - 2^22 > 2^23
constexpr int KEY_INF = 0x7fffffff;
static_assert(DIM * 255 * 255 < (1 << 23) && ((PAD_NORM + (1 << 23)) >> 27) == 0, "keys (d << 4 | e) stay positive ints");
constexpr int NO_SECOND = 1 << 24;          // a min2 at or above this is "no second candidate"
constexpr float MIN2_INIT = 2139095040.0f;  // match.cu:91, the int 0x7f800000 converted
constexpr int LIST_INF = KEY_INF >> 4;      // an unused list entry: above every padded row's distance, and what KEY_INF decodes to
constexpr int NO_ROW = KEY_INF;             // the index of an entry that names no row: behind every row at an equal distance
static_assert(LIST_INF > PAD_NORM + (1 << 23), "an unused list entry sorts behind the padded rows");
static_assert(PAD_NORM - (1 << 22) >= NO_SECOND && LIST_INF >= NO_SECOND,
              "a padded row and an unused entry both read as no second candidate");

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

/* Row c of n, or the last real one */
__device__ __forceinline__ int last_real(int c, int n) { return c < n ? c : n - 1; }

/* body(t, cf, cn) for the tiles t0 <= t < t1 of `rows` (n_rows real ones, rows past them repeat the last) and their `norms` */
template <class Body>
__device__ __forceinline__ void for_tiles(const unsigned char *__restrict__ rows, const int *__restrict__ norms, int n_rows,
                                          int t0, int t1, int r, int h, Body body)
{
    auto cand_row = [&](int t) { return rows + (size_t)last_real(t * TILE + r, n_rows) * DIM; };
    Frag cf = load_frag(cand_row(t0), h);
    Norm16 cn = load_norms(norms, t0 * TILE, h);
    for (int t = t0; t < t1; ++t) {
        const int tn = t + 1 < t1 ? t + 1 : t;                       // the last tile asks for itself
        const Frag nf = load_frag(cand_row(tn), h);
        const Norm16 nn = load_norms(norms, tn * TILE, h);
        body(t, cf, cn);
        cf = nf; cn = nn;
    }
}

/* a.b of the tile's 32 rows (cf, A operand) with the wave group's 32 items (qf, B operand): four k steps from zero */
__device__ __forceinline__ i32x16 tile_product(const Frag &cf, const Frag &qf)
{
    i32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(cf.s[s], qf.s[s], acc, 0, 0, 0);
    return acc;
}

/* The streamed row that register e of tile t's accumulator holds in lane half h */
__device__ __forceinline__ int acc_row(int t, int e, int h) { return t * TILE + (e & 3) + 8 * (e >> 2) + 4 * h; }

// The top-2 fold, for an output that reads (ld[0], lj[0], ld[1]) only: the tile's two smallest keys in one min / max pass
// (which finds the smallest again; the kernel's own is then dead code), merged under ONE vote; lj[1] is not kept (it stays
// NO_ROW, so the merge of the halves never puts it in front of a real row). fold_list<2> gives the same three values: 5.6 %
// faster on 16 pairs of 12k rows but 1.1 % slower on one pair of 4k rows, where a scan is few tiles.
__device__ __forceinline__ void fold_top2(int (&ld)[2], int (&lj)[2], const int (&key)[16], int t, int h)
{
    int g1 = KEY_INF, g2 = KEY_INF;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        g2 = min(g2, max(g1, key[e]));
        g1 = min(g1, key[e]);
    }
    const int d1 = g1 >> 4;
    if (__any(d1 < ld[1])) {
        if (d1 < ld[0]) {
            ld[1] = min(ld[0], g2 >> 4);
            ld[0] = d1;
            lj[0] = acc_row(t, g1 & 15, h);
        } else {
            ld[1] = min(ld[1], d1);
        }
    }
}

// The reference's last step on exact integer distances (every one of them is also an exact float): m1 at the lowest index
// idx, m2 = the smallest of the others or anything >= NO_SECOND. The scan's min2 starts at MIN2_INIT and is overwritten at
// every replacement of the minimum, so the start value survives only while the minimum sits at candidate 0; every real
// distance is below it, so it shows only for nB == 1.
__host__ __device__ __forceinline__ void emit_u8(int m1, int idx, int m2, float ambiguity, int *__restrict__ out)
{
    const float f1 = (float)m1;
    const float f2 = m2 >= NO_SECOND ? MIN2_INIT : (float)m2;
    if (f2 > 0.0f) {
        const float q = f1 / f2;
        *out = (q < ambiguity) ? idx : -1;
    }
}

/* Host twins: the exact squared distance of two rows, a plain sum of DIM integer squares */
inline int row_distance(const unsigned char *a, const unsigned char *b)
{
    int d = 0;
    for (int q = 0; q < DIM; ++q) {
        const int t = (int)a[q] - (int)b[q];
        d += t * t;
    }
    return d;
}

/* The matcher's host twin for one pair (nm_match_u8.hip): result[i], i < nA, as nm_sift_match_u8_host leaves it */
void match_pair_host(const unsigned char *A, int nA, const unsigned char *B, int nB, float ambiguity, int *result);

inline bool aligned16(int n, const unsigned char *const *t)
{
    for (int k = 0; k < n; ++k)
        if (reinterpret_cast<uintptr_t>(t[k]) & 15u) return false;
    return true;
}

/* What both device entries ask of their pointers: 16-byte reads of every row, 16-byte parts of the workspace */
inline bool operands_aligned(int n, const unsigned char *const *A, const unsigned char *const *B, const void *workspace)
{
    return aligned16(n, A) && aligned16(n, B) && !(reinterpret_cast<uintptr_t>(workspace) & 15u);
}

}  // namespace nmu8
