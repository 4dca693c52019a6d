// nm_match_mutual_u8.hip -- batched mutual-nearest-neighbour filtering of a match list over unsigned-char descriptors on the
// gfx950 i8 matrix pipe (no reference counterpart: the reference matches fp32 rows in one direction only). The fp32 filter
// (nm_match_mutual.hip) walks exact fma chains on the vector ALU; here every squared distance is an integer <= 128 * 255^2 =
// 8 323 200 < 2^23, exact in i32, so the column minimum comes straight from v_mfma_i32_32x32x32_i8 with no error bound, no
// second pass and no fallback.
// The three launches of a call (claims, scan, counts), the claims stage and the entries' skeleton are
// nm_match_claims_dev.hpp, shared with the fp32 filter. This file's own:
//   the Metric: the claims lane also writes its row's norm |row - 128|^2 into the workspace (A is the streamed side of the
//      scan: rows from nA up to the next multiple of 32 get PAD_NORM, which puts their distances above every real one); tau
//      is one direct 128-byte integer sum per lane, taken together with the norm of the claimed column, which is kept as a
//      fourth claim array: (i, j, tau, |B[j] - 128|^2).
//   the scan (the hot path), on the tile stream of nm_match_u8_dev.hpp: a wave's items are 64 consecutive compacted claims
//      (the fragments of their columns B[j]); the rows of A are streamed. d = |a|^2 + |b|^2 - 2 a.b. Per tile a lane takes
//      the minimum of its 16 keys (d << 4 | e): the smallest distance and, among equals, the lowest row (ascending e is
//      ascending row inside a lane). That one key decides whether the tile holds a row that beats the claim (nmp::beats):
//      only when the wave votes that some standing claim has d <= tau is the row index formed at all. A beaten claim leaves
//      the vote. No LDS, no atomics.
#include "nm_common.hpp"
#include "nm_match_claims_dev.hpp"
#include "nm_match_u8_dev.hpp"
#include "../../include/nm_abi.h"

namespace {

using namespace nmu8;
using nmc::SPLIT;
using nmp::beats;
using nmp::clip;
using nmp::is_claim;

static_assert(TB == nmc::TB && QW * (TB / 64) == TB, "a scan workgroup takes TB claims");

/* d(i, j) of two rows and |b - 128|^2 of the second, 16 bytes at a time */
struct U8Tau { int d, nb; };

__device__ __forceinline__ U8Tau tau_and_norm(const unsigned char *__restrict__ a, const unsigned char *__restrict__ b)
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
    return {s, n};
}

struct U8Metric {
    using Elem = unsigned char;
    using Tau = U8Tau;
    static constexpr int DIM = nmu8::DIM;
    static constexpr int HEADER = 256;      // workspace: int m[64]
    static_assert(nmp::MAX_BATCH * sizeof(int) <= HEADER, "workspace header");
    __host__ __device__ static size_t norm_rows(int capA) { return ((size_t)capA + TILE - 1) / TILE * TILE; }
    __host__ __device__ static size_t claim_rows(int capA) { return ((size_t)capA + QW - 1) / QW * QW; }
    __host__ __device__ static size_t pair_ints(int capA) { return norm_rows(capA) + 4 * claim_rows(capA); }
    // pair k's share: norm_rows(capA) norms of A, then the compacted claims: rows i, columns j, distances tau, column norms,
    // claim_rows(capA) ints each. Every part starts on a multiple of 16 bytes.
    __host__ __device__ static int *norms_of(void *ws, int k, int capA)
    {
        return reinterpret_cast<int *>(static_cast<char *>(ws) + HEADER) + (size_t)k * pair_ints(capA);
    }
    __host__ __device__ static int *claims_of(void *ws, int k, int capA) { return norms_of(ws, k, capA) + norm_rows(capA); }
    __device__ static U8Tau tau_of(const unsigned char *a, const unsigned char *b) { return tau_and_norm(a, b); }
    __device__ static void store_claim(int *t, size_t cr, int pos, U8Tau tau) { t[pos] = tau.d; t[cr + pos] = tau.nb; }
    __device__ static bool yields(U8Tau) { return true; }
    __device__ static float forward(U8Tau tau) { return (float)tau.d; }   // tau < 2^23: an exact float
    __device__ static void row_side(void *ws, int k, int capA, const unsigned char *A, int i, int nA)
    {
        if ((size_t)i < norm_rows(capA)) norms_of(ws, k, capA)[i] = i < nA ? row_norm(A + (size_t)i * DIM) : PAD_NORM;
    }
    static bool operands_ok(int n, const unsigned char *const *A, const unsigned char *const *B, const void *ws)
    {
        return operands_aligned(n, A, B, ws);
    }
};

__global__ __launch_bounds__(TB) void match_mutual_u8_claims_kernel(const nmc::ClaimTables<unsigned char> a, int capA, int capB,
                                                                    void *__restrict__ ws)
{
    nmc::match_claims<U8Metric>(a, capA, capB, ws);
}

// waves_per_eu: 126 registers instead of 114 + 16, which is the fourth wave per SIMD; no scratch either way
__global__ __launch_bounds__(TB) __attribute__((amdgpu_waves_per_eu(4, 4))) void match_mutual_u8_scan_kernel(const nmc::ScanTables<unsigned char> a, int capA, void *__restrict__ ws)
{
    const int k = blockIdx.z, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int m = static_cast<const int *>(ws)[k];
    const int c0 = blockIdx.x * TB + (threadIdx.x >> 6) * QW;
    if (c0 >= m) return;                                             // uniform over the wave; no barrier follows
    const int nA = clip(*a.d_nA[k], capA);                           // m > 0: nA > 0 and nB > 0
    const int tiles = (nA + TILE - 1) / TILE, per = (tiles + SPLIT - 1) / SPLIT;
    const int t0 = blockIdx.y * per, t1 = t0 + per < tiles ? t0 + per : tiles;
    if (t0 >= t1) return;
    const size_t cr = U8Metric::claim_rows(capA);
    const int *__restrict__ ci = U8Metric::claims_of(ws, k, capA);
    const unsigned char *__restrict__ Bd = a.B[k];

    Frag qf[QG];
    int row[QG], tau[QG], nq[QG];
    bool standing[QG];                                               // a claim that exists and no row has beaten yet
#pragma unroll
    for (int g = 0; g < QG; ++g) {
        const int c = c0 + 32 * g + r, cc = last_real(c, m);         // a lane past m repeats the last claim and stores nothing
        standing[g] = c < m;
        row[g] = ci[cc];
        tau[g] = ci[2 * cr + cc];
        nq[g] = ci[3 * cr + cc];
        qf[g] = load_frag(Bd + (size_t)ci[cr + cc] * DIM, h);
    }
    bool beaten[QG] = {false, false};

    for_tiles(a.A[k], U8Metric::norms_of(ws, k, capA), nA, t0, t1, r, h, [&](int t, const Frag cf, const Norm16 cn) {
        int ck[16];                                                  // (|a|^2 << 4) | e, shared by both groups
#pragma unroll
        for (int e = 0; e < 16; ++e) ck[e] = cn.g[e >> 2][e & 3] * 16 + e;
#pragma unroll
        for (int g = 0; g < QG; ++g) {
            const i32x16 acc = tile_product(cf, qf[g]);
            int key = KEY_INF;                                       // ((|a|^2 - 2 a.b) << 4) | e: |acc| <= 2^21, no overflow
#pragma unroll
            for (int e = 0; e < 16; ++e) key = min(key, ck[e] - acc[e] * 32);
            const int d1 = nq[g] + (key >> 4);
            if (__any(standing[g] && d1 <= tau[g])) {
                if (standing[g] && beats(d1, acc_row(t, key & 15, h), tau[g], row[g])) { beaten[g] = true; standing[g] = false; }
            }
        }
    });
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
            const int tau = row_distance(A + (size_t)i * DIM, bj);
            bool beaten = false;
            for (int ip = 0; ip < nA && !beaten; ++ip) {
                int d = 0;
                for (int q0 = 0; q0 < DIM && d <= tau; q0 += 16)     // a partial sum above tau cannot come back: no result changes
                    for (int q = q0; q < q0 + 16; ++q) {
                        const int t = (int)A[(size_t)ip * DIM + q] - (int)bj[q];
                        d += t * t;
                    }
                beaten = beats(d, ip, tau, i);
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

}  // namespace

extern "C" size_t nm_sift_match_mutual_u8_workspace_bytes(int n, int capA, int capB)
{
    if (!nmp::range_ok(n, capA) || !nmp::cap_ok(capB)) return 0;
    return U8Metric::HEADER + (size_t)n * U8Metric::pair_ints(capA) * sizeof(int);
}

extern "C" int nm_sift_match_mutual_u8_batch_dev(int n, const unsigned char *const *A, const int *const *d_nA, int capA,
                                                 const unsigned char *const *B, const int *const *d_nB, int capB,
                                                 const int *const *matches, int *const *result, int *count,
                                                 float *const *forward_distance, void *workspace, void *stream)
{
    return nmc::launch_mutual<U8Metric>(match_mutual_u8_claims_kernel, match_mutual_u8_scan_kernel, n, A, d_nA, capA, B, d_nB,
                                        capB, matches, result, count, forward_distance, workspace, stream);
}

extern "C" int nm_sift_match_mutual_u8_host(int n, const unsigned char *const *A, const int *const *nA, int capA,
                                            const unsigned char *const *B, const int *const *nB, int capB,
                                            const int *const *matches, int *const *result, int *count,
                                            float *const *forward_distance)
{
    return nmc::host_mutual(host_mutual_u8_pair, n, A, nA, capA, B, nB, capB, matches, result, count, forward_distance);
}
