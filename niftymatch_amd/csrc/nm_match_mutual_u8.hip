// nm_match_mutual_u8.hip -- batched mutual-nearest-neighbour filtering of a match list over unsigned-char descriptors on the
// gfx950 i8 matrix pipe (no reference counterpart: the reference matches fp32 rows in one direction only). The fp32 filter
// (nm_match_mutual.hip) walks exact fma chains on the vector ALU; here every squared distance is an integer <= 128 * 255^2 =
// 8 323 200 < 2^23, exact in i32, so the column minimum comes straight from v_mfma_i32_32x32x32_i8 with no error bound, no
// second pass and no fallback.
// THREE launches per call whatever n is, on the caller's stream, no allocation, no synchronisation, no host read:
//   1. claims (grid ceil(capA / 256) x n): one lane per row of A. The lane writes its row's norm |row - 128|^2 into the
//      workspace (A is the streamed side of the scan: rows at and beyond nA, up to the next multiple of 32, get PAD_NORM,
//      which puts their distances above every real one). A workgroup counts the claims below its first row from the match
//      list itself (integers, so the ordered position of a claim needs no word from another workgroup), computes tau =
//      d(i, j) of its claiming rows (one direct 128-byte integer sum per lane) and the norm of the claimed column, compacts
//      (i, j, tau, |B[j] - 128|^2) into the workspace by ordered ballot, and writes the provisional result (j or -1) and the
//      forward distance of all its rows. Workgroup 0 of a pair writes the pair's claim count m_k.
//   2. scan (grid ceil(capA / 256) x SPLIT x n, the hot path): a wave owns 64 consecutive compacted claims as two groups of
//      32 and keeps the four k-step fragments of their columns B[j] (bytes - 128 as signed i8) in 32 registers as the B
//      operand; it streams the rows of A in tiles of 32 as the A operand straight from global memory (the next tile is
//      requested before this one is multiplied). d = |a|^2 + |b|^2 - 2 a.b. Per tile a lane takes the minimum of its 16 keys
//      (d << 4 | e): the smallest distance and, among equals, the lowest row (ascending e is ascending row inside a lane).
//      That one key decides whether the tile holds a row that beats the claim (beats_u8): only when the wave votes that
//      some standing claim has d <= tau is the row index formed at all. A beaten claim leaves the vote. A pair's tiles are
//      cut into SPLIT ranges, one per workgroup; a workgroup that finds a claim beaten stores -1 over its provisional
//      result: several may store the same -1, nothing else is ever stored there, so the outcome does not depend on order.
//   3. counts (grid n): count[k] = entries >= 0 of result[k], integer sums (nm_pair_batch.hip).
// No LDS in the scan, no atomics. The fragments, the row norm and PAD_NORM are nm_match_u8_dev.hpp, shared with the matcher.
#include "nm_common.hpp"
#include "nm_match_u8_dev.hpp"
#include "nm_pair_batch.hpp"
#include "../../include/nm_abi.h"

namespace {

using namespace nmu8;
using nmp::clip;

constexpr int TB = 256;                     // rows (claims kernel) or claims (scan kernel) per workgroup: four waves
constexpr int QG = 2;                       // claim groups of 32 per wave
constexpr int QW = 32 * QG;                 // claims per wave
constexpr int SPLIT = 8;                    // tile ranges of a pair in the scan kernel, one workgroup each
constexpr int HEADER = 256;                 // workspace: int m[64]
static_assert(NM_MATCH_MUTUAL_U8_MAX_BATCH == 64 && NM_MATCH_MUTUAL_U8_MAX_BATCH * sizeof(int) <= HEADER, "workspace header");
static_assert(QW * (TB / 64) == TB, "a scan workgroup takes TB claims");

struct ClArgs {                             // 7 x 64 pointers: 3.5 KB of the 4 KB of kernel arguments
    const unsigned char *A[NM_MATCH_MUTUAL_U8_MAX_BATCH];
    const int *d_nA[NM_MATCH_MUTUAL_U8_MAX_BATCH];
    const unsigned char *B[NM_MATCH_MUTUAL_U8_MAX_BATCH];
    const int *d_nB[NM_MATCH_MUTUAL_U8_MAX_BATCH];
    const int *matches[NM_MATCH_MUTUAL_U8_MAX_BATCH];
    int *result[NM_MATCH_MUTUAL_U8_MAX_BATCH];
    float *fwd[NM_MATCH_MUTUAL_U8_MAX_BATCH];   // all NULL without a forward_distance table
};
static_assert(sizeof(ClArgs) + 64 < 4096, "claims kernel arguments exceed 4 KB");

struct ScArgs {
    const unsigned char *A[NM_MATCH_MUTUAL_U8_MAX_BATCH];
    const int *d_nA[NM_MATCH_MUTUAL_U8_MAX_BATCH];
    const unsigned char *B[NM_MATCH_MUTUAL_U8_MAX_BATCH];
    int *result[NM_MATCH_MUTUAL_U8_MAX_BATCH];
};

__host__ __device__ inline size_t norm_rows(int capA) { return ((size_t)capA + TILE - 1) / TILE * TILE; }
__host__ __device__ inline size_t claim_rows(int capA) { return ((size_t)capA + QW - 1) / QW * QW; }
__host__ __device__ inline size_t pair_ints(int capA) { return norm_rows(capA) + 4 * claim_rows(capA); }
// pair k's share: norm_rows(capA) norms of A, then the compacted claims: rows i, columns j, distances tau, column norms,
// claim_rows(capA) ints each. Every part starts on a multiple of 16 bytes.
__host__ __device__ inline int *norms_of(void *ws, int k, int capA)
{
    return reinterpret_cast<int *>(static_cast<char *>(ws) + HEADER) + (size_t)k * pair_ints(capA);
}
__host__ __device__ inline int *claims_of(void *ws, int k, int capA) { return norms_of(ws, k, capA) + norm_rows(capA); }

/* Row i claims column j = matches[i]: any value outside [0, nB) is no claim */
__host__ __device__ __forceinline__ bool is_claim(int j, int nB) { return j >= 0 && j < nB; }

/* Row ip at distance d takes the column from row i at distance tau: strictly nearer, or as near and earlier in the scan.
 * The keep rule of both entries: a claim is kept exactly when no row of A beats it. */
__host__ __device__ __forceinline__ bool beats_u8(int d, int ip, int tau, int i) { return d < tau || (d == tau && ip < i); }

/* d(i, j) of two rows and |b - 128|^2 of the second, 16 bytes at a time */
__device__ __forceinline__ void tau_and_norm(const unsigned char *__restrict__ a, const unsigned char *__restrict__ b, int &tau,
                                             int &nb)
{
    int s = 0, n = 0;
#pragma unroll
    for (int q = 0; q < DIM / 16; ++q) {
        const uint4 ua = reinterpret_cast<const uint4 *>(a)[q], ub = reinterpret_cast<const uint4 *>(b)[q];
        const unsigned wa[4] = {ua.x, ua.y, ua.z, ua.w}, wb[4] = {ub.x, ub.y, ub.z, ub.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int x = (int)((wa[e] >> (8 * c)) & 255u), y = (int)((wb[e] >> (8 * c)) & 255u);
                s += (x - y) * (x - y);
                n += (y - 128) * (y - 128);
            }
    }
    tau = s;
    nb = n;
}

__global__ __launch_bounds__(TB) void match_mutual_u8_claims_kernel(const ClArgs a, int capA, int capB, void *__restrict__ ws)
{
    __shared__ int s_cnt[2][TB / 64];
    const int k = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * TB, i = row0 + tid;
    const int nA = clip(*a.d_nA[k], capA), nB = clip(*a.d_nB[k], capB);
    const int *__restrict__ mt = a.matches[k];
    int *__restrict__ res = a.result[k];
    float *__restrict__ fwd = a.fwd[k];
    int *__restrict__ na = norms_of(ws, k, capA);
    if ((size_t)i < norm_rows(capA)) na[i] = i < nA ? row_norm(a.A[k] + (size_t)i * DIM) : PAD_NORM;
    if (row0 >= nA) {                                                // uniform over the workgroup: rows without a claim
        if (i < capA) {
            res[i] = -1;
            if (fwd) fwd[i] = __builtin_inff();
        }
        if (blockIdx.x == 0 && tid == 0) static_cast<int *>(ws)[k] = 0;   // nA == 0
        return;
    }
    // claims below this workgroup's first row, and (workgroup 0) in the whole pair: integer counts of the list itself
    const int upto = blockIdx.x == 0 ? nA : row0;
    int below = 0;
    for (int r = tid; r < upto; r += TB) below += is_claim(mt[r], nB) ? 1 : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) below += __shfl_xor(below, d);
    int j = -1;
    bool claim = false;
    if (i < nA) {
        j = mt[i];
        claim = is_claim(j, nB);
    }
    const unsigned long long bal = __ballot(claim);
    if (lane == 0) { s_cnt[0][wave] = below; s_cnt[1][wave] = __popcll(bal); }
    __syncthreads();
    int all_below = 0, before = 0;
#pragma unroll
    for (int w = 0; w < TB / 64; ++w) {
        all_below += s_cnt[0][w];
        before += w < wave ? s_cnt[1][w] : 0;
    }
    if (blockIdx.x == 0) {
        if (tid == 0) static_cast<int *>(ws)[k] = all_below;         // m_k
        all_below = 0;                                               // workgroup 0 has nothing below it
    }
    int tau = 0;
    if (claim) {
        int nb;
        tau_and_norm(a.A[k] + (size_t)i * DIM, a.B[k] + (size_t)j * DIM, tau, nb);
        const size_t cr = claim_rows(capA);
        int *__restrict__ ci = claims_of(ws, k, capA);
        const int pos = all_below + before + __popcll(bal & ((1ull << lane) - 1ull));   // < nA <= capA
        ci[pos] = i;
        ci[cr + pos] = j;
        ci[2 * cr + pos] = tau;
        ci[3 * cr + pos] = nb;
    }
    if (i < capA) {
        res[i] = claim ? j : -1;
        if (fwd) fwd[i] = claim ? (float)tau : __builtin_inff();     // tau < 2^23: an exact float
    }
}

// waves_per_eu: 126 registers instead of 114 + 16, which is the fourth wave per SIMD; no scratch either way
__global__ __launch_bounds__(TB) __attribute__((amdgpu_waves_per_eu(4, 4))) void match_mutual_u8_scan_kernel(const ScArgs a, int capA, void *__restrict__ ws)
{
    const int k = blockIdx.z, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int m = static_cast<const int *>(ws)[k];
    const int c0 = blockIdx.x * TB + (threadIdx.x >> 6) * QW;
    if (c0 >= m) return;                                             // uniform over the wave; no barrier follows
    const int nA = clip(*a.d_nA[k], capA);                           // m > 0: nA > 0 and nB > 0
    const int tiles = (nA + TILE - 1) / TILE, per = (tiles + SPLIT - 1) / SPLIT;
    const int t0 = blockIdx.y * per, t1 = t0 + per < tiles ? t0 + per : tiles;
    if (t0 >= t1) return;
    const size_t cr = claim_rows(capA);
    const int *__restrict__ na = norms_of(ws, k, capA);
    const int *__restrict__ ci = claims_of(ws, k, capA);
    const unsigned char *__restrict__ Ad = a.A[k];
    const unsigned char *__restrict__ Bd = a.B[k];

    Frag qf[QG];
    int row[QG], tau[QG], nq[QG];
    bool standing[QG];                                               // a claim that exists and no row has beaten yet
#pragma unroll
    for (int g = 0; g < QG; ++g) {
        const int c = c0 + 32 * g + r, cc = c < m ? c : m - 1;       // a lane past m repeats the last claim and stores nothing
        standing[g] = c < m;
        row[g] = ci[cc];
        tau[g] = ci[2 * cr + cc];
        nq[g] = ci[3 * cr + cc];
        qf[g] = load_frag(Bd + (size_t)ci[cr + cc] * DIM, h);
    }
    bool beaten[QG] = {false, false};

    auto cand_row = [&](int t) { const int c = t * TILE + r; return Ad + (size_t)(c < nA ? c : nA - 1) * DIM; };
    Frag cf = load_frag(cand_row(t0), h);
    Norm16 cn = load_norms(na, t0 * TILE, h);
    for (int t = t0; t < t1; ++t) {
        const int tn = t + 1 < t1 ? t + 1 : t;                       // the last tile asks for itself
        const Frag nf = load_frag(cand_row(tn), h);
        const Norm16 nn = load_norms(na, tn * TILE, h);
        int ck[16];                                                  // (|a|^2 << 4) | e, shared by both groups
#pragma unroll
        for (int e = 0; e < 16; ++e) ck[e] = cn.g[e >> 2][e & 3] * 16 + e;
#pragma unroll
        for (int g = 0; g < QG; ++g) {
            i32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(cf.s[s], qf[g].s[s], acc, 0, 0, 0);
            int key = KEY_INF;                                       // ((|a|^2 - 2 a.b) << 4) | e: |acc| <= 2^21, no overflow
#pragma unroll
            for (int e = 0; e < 16; ++e) key = min(key, ck[e] - acc[e] * 32);
            const int d1 = nq[g] + (key >> 4);
            if (__any(standing[g] && d1 <= tau[g])) {
                const int e1 = key & 15, ip = t * TILE + (e1 & 3) + 8 * (e1 >> 2) + 4 * h;
                if (standing[g] && beats_u8(d1, ip, tau[g], row[g])) { beaten[g] = true; standing[g] = false; }
            }
        }
        cf = nf; cn = nn;
    }
#pragma unroll
    for (int g = 0; g < QG; ++g)
        if (beaten[g]) a.result[k][row[g]] = -1;                     // plain store; every writer stores -1
}

// ---- the host twin: a plain triple loop over int distances, the same two predicates ----
void host_mutual_u8_pair(const unsigned char *A, int nA, int capA, const unsigned char *B, int nB, const int *matches,
                         int *result, int *count, float *fwd)
{
    int kept = 0;
    for (int i = 0; i < capA; ++i) {
        int out = -1;
        float f = __builtin_inff();
        const int j = i < nA ? matches[i] : -1;
        if (i < nA && is_claim(j, nB)) {
            const unsigned char *bj = B + (size_t)j * DIM;
            int tau = 0;
            for (int q = 0; q < DIM; ++q) {
                const int t = (int)A[(size_t)i * DIM + q] - (int)bj[q];
                tau += t * t;
            }
            bool beaten = false;
            for (int ip = 0; ip < nA && !beaten; ++ip) {
                int d = 0;
                for (int q0 = 0; q0 < DIM && d <= tau; q0 += 16)     // a partial sum above tau cannot come back: no result changes
                    for (int q = q0; q < q0 + 16; ++q) {
                        const int t = (int)A[(size_t)ip * DIM + q] - (int)bj[q];
                        d += t * t;
                    }
                beaten = beats_u8(d, ip, tau, i);
            }
            if (!beaten) out = j;
            f = (float)tau;
        }
        result[i] = out;
        kept += out >= 0 ? 1 : 0;
        if (fwd) fwd[i] = f;
    }
    *count = kept;
}

bool mu8_args_ok(int n, const unsigned char *const *A, const int *const *nA, int capA, const unsigned char *const *B,
                 const int *const *nB, int capB, const int *const *matches, int *const *result, const int *count,
                 float *const *fwd)
{
    return nmp::range_ok(n, capA) && nmp::cap_ok(capB) && nmp::tables_ok(n, {A, nA, B, nB, matches, result}, {fwd}, {count});
}

}  // namespace

extern "C" size_t nm_sift_match_mutual_u8_workspace_bytes(int n, int capA, int capB)
{
    if (!nmp::range_ok(n, capA) || !nmp::cap_ok(capB)) return 0;
    return HEADER + (size_t)n * pair_ints(capA) * sizeof(int);
}

extern "C" int nm_sift_match_mutual_u8_batch_dev(int n, const unsigned char *const *A, const int *const *d_nA, int capA,
                                                 const unsigned char *const *B, const int *const *d_nB, int capB,
                                                 const int *const *matches, int *const *result, int *count,
                                                 float *const *forward_distance, void *workspace, void *stream)
{
    if (!mu8_args_ok(n, A, d_nA, capA, B, d_nB, capB, matches, result, count, forward_distance) || !workspace ||
        !aligned16(n, A) || !aligned16(n, B) || (reinterpret_cast<uintptr_t>(workspace) & 15u))
        return (int)hipErrorInvalidValue;
    ClArgs c;
    ScArgs s;
    nmp::fill_slots(c.A, A, 0, n); nmp::fill_slots(c.d_nA, d_nA, 0, n); nmp::fill_slots(c.B, B, 0, n);
    nmp::fill_slots(c.d_nB, d_nB, 0, n); nmp::fill_slots(c.matches, matches, 0, n); nmp::fill_slots(c.result, result, 0, n);
    nmp::fill_slots(c.fwd, forward_distance, 0, n);
    nmp::fill_slots(s.A, A, 0, n); nmp::fill_slots(s.d_nA, d_nA, 0, n); nmp::fill_slots(s.B, B, 0, n);
    nmp::fill_slots(s.result, result, 0, n);
    const int blocks = nm_divup(capA, TB);
    hipLaunchKernelGGL(match_mutual_u8_claims_kernel, dim3(blocks, n), dim3(TB), 0, nm_stream(stream), c, capA, capB, workspace);
    NM_LAUNCH_CHECK();
    hipLaunchKernelGGL(match_mutual_u8_scan_kernel, dim3(blocks, SPLIT, n), dim3(TB), 0, nm_stream(stream), s, capA, workspace);
    NM_LAUNCH_CHECK();
    return nmp::launch_pair_count(n, result, capA, count, nm_stream(stream));
}

extern "C" int nm_sift_match_mutual_u8_host(int n, const unsigned char *const *A, const int *const *nA, int capA,
                                            const unsigned char *const *B, const int *const *nB, int capB,
                                            const int *const *matches, int *const *result, int *count,
                                            float *const *forward_distance)
{
    if (!mu8_args_ok(n, A, nA, capA, B, nB, capB, matches, result, count, forward_distance)) return (int)hipErrorInvalidValue;
    for (int k = 0; k < n; ++k)
        host_mutual_u8_pair(A[k], clip(*nA[k], capA), capA, B[k], clip(*nB[k], capB), matches[k], result[k], count + k,
                            forward_distance ? forward_distance[k] : nullptr);
    return 0;
}
