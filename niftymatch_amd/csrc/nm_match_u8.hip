// nm_match_u8.hip -- batched brute-force matching of unsigned-char descriptors on the gfx950 i8 matrix pipe (no reference
// counterpart: the reference matches fp32 rows only, kernels/match.cu). The squared distance of two u8 rows is an integer
// <= 128 * 255^2 = 8 323 200 < 2^23, computed EXACTLY in i32, so there is no error bound, no second pass and no fallback.
// ONE scan, TWO outputs. Both entries are the same two launches per call whatever n is, on the caller's stream, no allocation,
// no synchronisation, no host read:
//   1. norms (grid ceil(rows / 256) x 2 x n): one lane per row, |row - 128|^2 as an int into the workspace. Rows of B at and
//      beyond nB (up to the next multiple of 32) get PAD_NORM, which puts their distances above every real one.
//   2. match_scan_u8_kernel<L, Out> (grid ceil(capA / 256) x n), on the tile stream of nm_match_u8_dev.hpp: a wave owns 64
//      queries and keeps their fragments as the B operand of v_mfma_i32_32x32x32_i8; it streams the candidates (a tile is
//      4 KB, one 16-byte read per lane and k step). d = |a|^2 + |b|^2 - 2 a.b. Per query group a lane keeps the L = 1, 2, 4
//      or 8 best (d, j) of its lane half in registers, ascending. Per tile the lane's smallest key (d << 4 | e) is found with
//      min; while the wave votes that some lane's smallest beats that lane's list tail, every lane inserts its smallest (no
//      change where it does not beat the tail) and takes its next key above the one just taken: at most L rounds, because a
//      lane's own L insertions of ascending keys make up its whole list. Ascending e is ascending candidate index inside a
//      lane, tiles ascend, and insertion is strict in d, so equal distances stay in index order; the two lane halves (same
//      query, disjoint candidates) are merged at the end by (d, j), and half 0 hands the merged list to Out:
//        ListOut  (nm_sift_match_knn_u8_batch_dev; L = the next of 1, 2, 4, 8 at or above the runtime k) stores the first k
//                 entries; slots at and beyond min(k, nB) are stored as -1 / 0x7fffffff whatever the list holds there
//                 (padded rows, or its start value).
//        RatioOut (nm_sift_match_u8_batch_dev; L = 2) takes the reference's last step (match.cu:88-116) on (min1, index,
//                 min2) = the list of two: min2 starts at 2139095040.0f, a row with min2 == 0 is left unwritten, result =
//                 min1 / min2 < ambiguity ? index : -1 with an fp32 divide. The result is what the reference's scan makes of
//                 the same distances as floats. It never reads the second index, so its per-tile step is the lighter
//                 fold_top2 (the tile's two smallest keys in one min / max pass, one vote) in place of the rounds above;
//                 prologue, tile stream, merge and store are the shared ones.
// No LDS, no atomics. The lane -> (row, k) map of the i8 operands is checked by tools/micro/mfma_i8_model.hip. The operand
// fragments, the row norm, PAD_NORM, the tile stream and the host's row distance are nm_match_u8_dev.hpp, shared with the
// mutual filter (nm_match_mutual_u8.hip); fold_top2, emit_u8 and their constants are there too, shared with the link votes
// (nm_link_propose.hip), whose host twin calls the matcher's through nmu8::match_pair_host. The host twins are one sorted
// insertion on (d, j); the matcher's is its k = 2.
#include "nm_common.hpp"
#include "nm_match_u8_dev.hpp"
#include "nm_pair_batch.hpp"
#include "../../include/nm_abi.h"

#include <cstdint>

namespace {

using namespace nmu8;

constexpr int QB = QW * TB / 64;            // queries per workgroup
constexpr int KNN_NONE = KEY_INF;           // the distance of a slot without a candidate (its index is -1)
static_assert(KNN_NONE >= NO_SECOND, "an empty slot reads as no second candidate");
static_assert(NM_MATCH_KNN_U8_MAX_BATCH == NM_MATCH_U8_MAX_BATCH, "the k-NN entry shares the matcher's rows and norms launch");

struct PairRows {                           // the rows of both entries: 4 x 64 pointers, 2 KB of kernel arguments
    const unsigned char *A[NM_MATCH_U8_MAX_BATCH];
    const int *d_nA[NM_MATCH_U8_MAX_BATCH];
    const unsigned char *B[NM_MATCH_U8_MAX_BATCH];
    const int *d_nB[NM_MATCH_U8_MAX_BATCH];
    void fill(int n, const unsigned char *const *a, const int *const *nA, const unsigned char *const *b, const int *const *nB)
    {
        nmp::fill_slots(A, a, 0, n); nmp::fill_slots(d_nA, nA, 0, n); nmp::fill_slots(B, b, 0, n); nmp::fill_slots(d_nB, nB, 0, n);
    }
};

__host__ __device__ inline size_t rows_a(int capA) { return ((size_t)capA + QB - 1) / QB * QB; }
__host__ __device__ inline size_t rows_b(int capB) { return ((size_t)capB + TILE - 1) / TILE * TILE; }
// pair k's norms: rows_a(capA) ints of A, then rows_b(capB) ints of B
__host__ __device__ inline int *norms_of(void *ws, int k, int capA, int capB)
{
    return static_cast<int *>(ws) + (size_t)k * (rows_a(capA) + rows_b(capB));
}

// ---- what half 0 stores for query qi of pair p from its merged ascending list (ld, lj) ----
struct ListOut {                            // the first k entries; with PairRows 6 x 64 pointers, 3 KB of kernel arguments
    int *index[NM_MATCH_KNN_U8_MAX_BATCH];
    int *distance[NM_MATCH_KNN_U8_MAX_BATCH];    // all null: indices only
    int k;
    static constexpr bool TOP2_FOLD = false;
    template <int L> __device__ __forceinline__ void store(int p, int qi, const int (&ld)[L], const int (&lj)[L], int nB) const
    {
        const int m = min(k, nB);
        int *__restrict__ oi = index[p] + (size_t)qi * k;
        int *__restrict__ dd = distance[p] ? distance[p] + (size_t)qi * k : nullptr;
#pragma unroll
        for (int s = 0; s < L; ++s)
            if (s < k) {
                oi[s] = s < m ? lj[s] : -1;
                if (dd) dd[s] = s < m ? ld[s] : KNN_NONE;
            }
    }
};
static_assert(sizeof(PairRows) + sizeof(ListOut) + 64 < 4096, "k-NN kernel arguments exceed 4 KB");

struct RatioOut {                           // the ratio test on the list of two; with PairRows 5 x 64 pointers, 2.5 KB
    int *result[NM_MATCH_U8_MAX_BATCH];
    float ambiguity;
    static constexpr bool TOP2_FOLD = true; // reads (ld[0], lj[0], ld[1]) only
    // ld[1] is a real distance, a padded row's or LIST_INF; the last two are >= NO_SECOND (asserted above)
    __device__ __forceinline__ void store(int p, int qi, const int (&ld)[2], const int (&lj)[2], int) const
    {
        emit_u8(ld[0], lj[0], ld[1], ambiguity, result[p] + qi);
    }
};
static_assert(sizeof(PairRows) + sizeof(RatioOut) + 64 < 4096, "match kernel arguments exceed 4 KB");

__global__ __launch_bounds__(TB) void match_u8_norms_kernel(const PairRows a, int capA, int capB, void *__restrict__ ws)
{
    const int k = blockIdx.z, side = blockIdx.y;
    const size_t row = (size_t)blockIdx.x * TB + threadIdx.x;
    int *__restrict__ na = norms_of(ws, k, capA, capB);
    if (side == 0) {
        const int nA = nmp::clip(*a.d_nA[k], capA);
        if (row < rows_a(capA)) na[row] = row < (size_t)nA ? row_norm(a.A[k] + row * DIM) : 0;
    } else {
        const int nB = nmp::clip(*a.d_nB[k], capB);
        if (row < rows_b(capB)) na[rows_a(capA) + row] = row < (size_t)nB ? row_norm(a.B[k] + row * DIM) : PAD_NORM;
    }
}

// (d, j) goes into the ascending list (ld, lj) in front of the first entry it is `before`, the last entry dropping out; no
// change when it is before none.
template <int L, class Before>
__device__ __forceinline__ void list_insert(int (&ld)[L], int (&lj)[L], int d, int j, Before before)
{
#pragma unroll
    for (int s = L - 1; s > 0; --s) {
        const bool up = before(d, j, ld[s - 1], lj[s - 1]), here = before(d, j, ld[s], lj[s]);
        ld[s] = up ? ld[s - 1] : (here ? d : ld[s]);
        lj[s] = up ? lj[s - 1] : (here ? j : lj[s]);
    }
    const bool here = before(d, j, ld[0], lj[0]);
    ld[0] = here ? d : ld[0];
    lj[0] = here ? j : lj[0];
}

// ---- what a lane makes of a tile's 16 keys (d << 4 | e, ascending e = ascending row inside the lane half) ----
// The list fold, from the smallest key g1: the voted rounds of the header. Insertion is strict in d alone: the lane half
// meets its candidates in ascending index, so an equal distance belongs behind.
template <int L>
__device__ __forceinline__ void fold_list(int (&ld)[L], int (&lj)[L], const int (&key)[16], int g1, int t, int h)
{
    const auto nearer = [](int d, int, int ds, int) { return d < ds; };
    for (int round = 0; round < L && __any((g1 >> 4) < ld[L - 1]); ++round) {
        list_insert<L>(ld, lj, g1 >> 4, acc_row(t, g1 & 15, h), nearer);
        if (L > 1) {                                                 // the smallest key above g1: keys at or below it wrap high
            const unsigned above = (unsigned)g1 + 1u;
            unsigned off = 0xffffffffu;
#pragma unroll
            for (int e = 0; e < 16; ++e) off = min(off, (unsigned)key[e] - above);
            g1 = (int)(above + off);
        }
    }
}

template <int L, class Out>
__global__ __launch_bounds__(TB) void match_scan_u8_kernel(const PairRows a, const Out out, int capA, int capB,
                                                           void *__restrict__ ws)
{
    static_assert(L >= 1 && L <= NM_MATCH_KNN_U8_MAX_K && L < 16, "a tile's 16 keys outlast L rounds");
    const int k = blockIdx.y, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int nA = nmp::clip(*a.d_nA[k], capA), nB = nmp::clip(*a.d_nB[k], capB);
    if (nA <= 0 || nB <= 0) return;                                  // a pair without rows is a no-op
    const int q0 = blockIdx.x * QB + (threadIdx.x >> 6) * QW;
    if (q0 >= nA) return;                                            // uniform over the wave; no barrier follows
    const unsigned char *__restrict__ Ad = a.A[k];
    const int *__restrict__ na = norms_of(ws, k, capA, capB);

    Frag qf[QG];
    int nq[QG], ld[QG][L], lj[QG][L];
#pragma unroll
    for (int g = 0; g < QG; ++g) {
        const int qrow = last_real(q0 + 32 * g + r, nA);             // a lane past nA repeats the last row and writes nothing
        qf[g] = load_frag(Ad + (size_t)qrow * DIM, h);
        nq[g] = na[qrow];
#pragma unroll
        for (int s = 0; s < L; ++s) { ld[g][s] = LIST_INF; lj[g][s] = NO_ROW; }
    }

    for_tiles(a.B[k], na + rows_a(capA), nB, 0, (nB + TILE - 1) / TILE, r, h, [&](int t, const Frag cf, const Norm16 cn) {
#pragma unroll
        for (int g = 0; g < QG; ++g) {
            const i32x16 acc = tile_product(cf, qf[g]);
            int key[16], g1 = KEY_INF;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                key[e] = ((nq[g] + cn.g[e >> 2][e & 3] - 2 * acc[e]) << 4) | e;
                g1 = min(g1, key[e]);
            }
            if constexpr (Out::TOP2_FOLD) fold_top2(ld[g], lj[g], key, t, h);
            else fold_list<L>(ld[g], lj[g], key, g1, t, h);
        }
    });

    const auto before = [](int d, int j, int ds, int js) { return d < ds || (d == ds && j < js); };
#pragma unroll
    for (int g = 0; g < QG; ++g) {
        int od[L], oj[L];
#pragma unroll
        for (int s = 0; s < L; ++s) { od[s] = __shfl_xor(ld[g][s], 32); oj[s] = __shfl_xor(lj[g][s], 32); }
#pragma unroll
        for (int s = 0; s < L; ++s) list_insert<L>(ld[g], lj[g], od[s], oj[s], before);
        const int qi = q0 + 32 * g + r;
        if (h == 0 && qi < nA) out.store(k, qi, ld[g], lj[g], nB);
    }
}

// ---- the host twin: exact integer distances, sorted insertion on (d, j) into a list of k, then the fill rule for the slots
// without a candidate ----
void host_knn_pair(const unsigned char *A, int nA, const unsigned char *B, int nB, int k, int *index, int *distance)
{
    if (nA <= 0 || nB <= 0) return;
    for (int i = 0; i < nA; ++i) {
        int ld[NM_MATCH_KNN_U8_MAX_K], lj[NM_MATCH_KNN_U8_MAX_K], held = 0;
        for (int j = 0; j < nB; ++j) {
            const int d = row_distance(A + (size_t)i * DIM, B + (size_t)j * DIM);
            const auto before = [&](int s) { return d < ld[s] || (d == ld[s] && j < lj[s]); };
            if (held == k && !before(k - 1)) continue;
            int s = held < k ? held++ : k - 1;
            for (; s > 0 && before(s - 1); --s) { ld[s] = ld[s - 1]; lj[s] = lj[s - 1]; }
            ld[s] = d; lj[s] = j;
        }
        for (int s = 0; s < k; ++s) {
            index[(size_t)i * k + s] = s < held ? lj[s] : -1;
            if (distance) distance[(size_t)i * k + s] = s < held ? ld[s] : KNN_NONE;
        }
    }
}

// The matcher's host twin: a row's list of two, the same last step (KNN_NONE in slot 1 is "no second candidate")
void host_match_pair(const unsigned char *A, int nA, const unsigned char *B, int nB, float ambiguity, int *result)
{
    if (nA <= 0 || nB <= 0) return;
    for (int i = 0; i < nA; ++i) {
        int lj[2], ld[2];
        host_knn_pair(A + (size_t)i * DIM, 1, B, nB, 2, lj, ld);
        emit_u8(ld[0], lj[0], ld[1], ambiguity, result + i);
    }
}

bool rows_ok(int n, const unsigned char *const *A, const int *const *nA, int capA, const unsigned char *const *B,
             const int *const *nB, int capB)
{
    return nmp::range_ok(n, capA) && nmp::cap_ok(capB) && nmp::tables_ok(n, {A, nA, B, nB}, {}, {});
}

bool u8_args_ok(int n, const unsigned char *const *A, const int *const *nA, int capA, const unsigned char *const *B,
                const int *const *nB, int capB, int *const *result)
{
    return rows_ok(n, A, nA, capA, B, nB, capB) && nmp::tables_ok(n, {result}, {}, {});
}

bool knn_args_ok(int n, const unsigned char *const *A, const int *const *nA, int capA, const unsigned char *const *B,
                 const int *const *nB, int capB, int k, int *const *index, int *const *distance)
{
    return k >= 1 && k <= NM_MATCH_KNN_U8_MAX_K && rows_ok(n, A, nA, capA, B, nB, capB) &&
           nmp::tables_ok(n, {index}, {distance}, {});
}

void launch_norms(const PairRows &rows, int n, int capA, int capB, void *workspace, hipStream_t stream)
{
    const size_t most = rows_a(capA) > rows_b(capB) ? rows_a(capA) : rows_b(capB);
    hipLaunchKernelGGL(match_u8_norms_kernel, dim3((unsigned)((most + TB - 1) / TB), 2, n), dim3(TB), 0, stream, rows, capA,
                       capB, workspace);
}

template <int L, class Out>
void launch_scan(const PairRows &rows, const Out &out, int n, int capA, int capB, void *workspace, hipStream_t stream)
{
    hipLaunchKernelGGL((match_scan_u8_kernel<L, Out>), dim3(nm_divup(capA, QB), n), dim3(TB), 0, stream, rows, out, capA, capB,
                       workspace);
}

}  // namespace

void nmu8::match_pair_host(const unsigned char *A, int nA, const unsigned char *B, int nB, float ambiguity, int *result)
{
    host_match_pair(A, nA, B, nB, ambiguity, result);
}

extern "C" size_t nm_sift_match_u8_workspace_bytes(int n, int capA, int capB)
{
    if (!nmp::range_ok(n, capA) || !nmp::cap_ok(capB)) return 0;
    return (size_t)n * (rows_a(capA) + rows_b(capB)) * sizeof(int);
}

extern "C" int nm_sift_match_u8_batch_dev(int n, const unsigned char *const *A, const int *const *d_nA, int capA,
                                          const unsigned char *const *B, const int *const *d_nB, int capB,
                                          int *const *result, float ambiguity, void *workspace, void *stream)
{
    if (!u8_args_ok(n, A, d_nA, capA, B, d_nB, capB, result) || !workspace || !operands_aligned(n, A, B, workspace))
        return (int)hipErrorInvalidValue;
    PairRows rows;
    RatioOut out;
    rows.fill(n, A, d_nA, B, d_nB);
    nmp::fill_slots(out.result, result, 0, n);
    out.ambiguity = ambiguity;
    launch_norms(rows, n, capA, capB, workspace, nm_stream(stream));
    NM_LAUNCH_CHECK();
    launch_scan<2>(rows, out, n, capA, capB, workspace, nm_stream(stream));
    NM_LAUNCH_CHECK();
    return 0;
}

extern "C" int nm_sift_match_u8_host(int n, const unsigned char *const *A, const int *const *nA, int capA,
                                     const unsigned char *const *B, const int *const *nB, int capB, int *const *result,
                                     float ambiguity)
{
    if (!u8_args_ok(n, A, nA, capA, B, nB, capB, result)) return (int)hipErrorInvalidValue;
    for (int k = 0; k < n; ++k)
        host_match_pair(A[k], nmp::clip(*nA[k], capA), B[k], nmp::clip(*nB[k], capB), ambiguity, result[k]);
    return 0;
}

extern "C" size_t nm_sift_match_knn_u8_workspace_bytes(int n, int capA, int capB)
{
    return nm_sift_match_u8_workspace_bytes(n, capA, capB);          // the matcher's norms, the matcher's layout
}

extern "C" int nm_sift_match_knn_u8_batch_dev(int n, const unsigned char *const *A, const int *const *d_nA, int capA,
                                              const unsigned char *const *B, const int *const *d_nB, int capB, int k,
                                              int *const *index, int *const *distance, void *workspace, void *stream)
{
    if (!knn_args_ok(n, A, d_nA, capA, B, d_nB, capB, k, index, distance) || !workspace ||
        !operands_aligned(n, A, B, workspace))
        return (int)hipErrorInvalidValue;
    PairRows rows;
    ListOut out;
    rows.fill(n, A, d_nA, B, d_nB);
    nmp::fill_slots(out.index, index, 0, n); nmp::fill_slots(out.distance, distance, 0, n);
    out.k = k;
    launch_norms(rows, n, capA, capB, workspace, nm_stream(stream));
    NM_LAUNCH_CHECK();
    if (k == 1) launch_scan<1>(rows, out, n, capA, capB, workspace, nm_stream(stream));
    else if (k == 2) launch_scan<2>(rows, out, n, capA, capB, workspace, nm_stream(stream));
    else if (k <= 4) launch_scan<4>(rows, out, n, capA, capB, workspace, nm_stream(stream));
    else launch_scan<8>(rows, out, n, capA, capB, workspace, nm_stream(stream));
    NM_LAUNCH_CHECK();
    return 0;
}

extern "C" int nm_sift_match_knn_u8_host(int n, const unsigned char *const *A, const int *const *nA, int capA,
                                         const unsigned char *const *B, const int *const *nB, int capB, int k,
                                         int *const *index, int *const *distance)
{
    if (!knn_args_ok(n, A, nA, capA, B, nB, capB, k, index, distance)) return (int)hipErrorInvalidValue;
    for (int p = 0; p < n; ++p)
        host_knn_pair(A[p], nmp::clip(*nA[p], capA), B[p], nmp::clip(*nB[p], capB), k, index[p],
                      distance ? distance[p] : nullptr);
    return 0;
}
