// nm_match_mutual.hip -- batched mutual-nearest-neighbour filtering of a match list for gfx950 (no reference counterpart: the
// reference's matcher, kernels/match.cu, tests one direction only and a client cross-checks with a second, swapped call).
// THREE launches per call whatever n is, on the caller's stream, no allocation, no synchronisation, no host read:
//   1. claims (grid ceil(capA / 256) x n): one lane per row of A. A workgroup counts the claims below its first row from the
//      match list itself (integers, so the ordered position of a claim needs no word from another workgroup), computes tau
//      = d(i, j) of its claiming rows (one full chain per lane), compacts (i, j, tau) into the workspace by ordered ballot,
//      and writes the provisional result (j, or -1 for no claim and for a NaN tau) and the forward distance of all its rows.
//      Workgroup 0 of a pair writes the pair's claim count m_k.
//   2. scan (grid ceil(capA / 256) x SPLIT x n, the hot path): one lane per claim, its column B[j] in 128 registers. The
//      rows of A are the same for every lane of a wave: they are read through a const __restrict__ pointer at wave-uniform
//      addresses (scalar loads of 16 dwords; no LDS), NMM_CHUNK dimensions at a time; chunk 0 of the next row is requested
//      while chunk 0 of this row is computed, a later chunk only once the vote has asked for it (hipcc sinks an earlier
//      request below the vote's branch anyway). After each chunk the wave votes; when no lane has acc <= tau the row is
//      abandoned. A row that runs to the end is judged by nmm::beats. A pair's rows are cut into SPLIT
//      ranges, one per workgroup; a workgroup that finds a claim beaten stores -1 over its provisional result: several
//      workgroups may store the same -1, nothing else is ever stored there, so the outcome does not depend on order.
//   3. counts (grid n): count[k] = entries >= 0 of result[k], integer sums.
// The chain of a distance is sequential in q and stays on one lane. No atomics (the NMM_STATS scratch build adds two
// counters). The arithmetic is nm_match_mutual_math.hpp, shared with the host twin below: both agree bit for bit.
#include "nm_common.hpp"
#include "nm_match_mutual_math.hpp"
#include "nm_pair_batch.hpp"
#include "../../include/nm_abi.h"

namespace {

using namespace nmm;

constexpr int TB = 256;                    // rows (claims kernel) or claims (scan kernel) per workgroup
constexpr int SPLIT = 8;                   // row ranges of a pair in the scan kernel, one workgroup each
constexpr int HEADER = 512;                // workspace: int m[64], then the two NMM_STATS counters at byte 256
static_assert(NM_MATCH_MUTUAL_MAX_BATCH == 64 && NM_MATCH_MUTUAL_MAX_BATCH * sizeof(int) <= 256, "workspace header");

struct ClArgs {                            // 7 x 64 pointers: 3.5 KB of the 4 KB of kernel arguments
    const float *A[NM_MATCH_MUTUAL_MAX_BATCH];
    const int *d_nA[NM_MATCH_MUTUAL_MAX_BATCH];
    const float *B[NM_MATCH_MUTUAL_MAX_BATCH];
    const int *d_nB[NM_MATCH_MUTUAL_MAX_BATCH];
    const int *matches[NM_MATCH_MUTUAL_MAX_BATCH];
    int *result[NM_MATCH_MUTUAL_MAX_BATCH];
    float *fwd[NM_MATCH_MUTUAL_MAX_BATCH];  // all NULL without a forward_distance table
};
static_assert(sizeof(ClArgs) + 64 < 4096, "claims kernel arguments exceed 4 KB");

struct ScArgs {
    const float *A[NM_MATCH_MUTUAL_MAX_BATCH];
    const int *d_nA[NM_MATCH_MUTUAL_MAX_BATCH];
    const float *B[NM_MATCH_MUTUAL_MAX_BATCH];
    int *result[NM_MATCH_MUTUAL_MAX_BATCH];
};

__host__ __device__ inline size_t cap_rows(int capA) { return ((size_t)capA + 63) / 64 * 64; }

// pair k's compacted claims: rows i, columns j, distances tau, cap_rows(capA) entries each
__host__ __device__ inline int *claims_of(void *ws, int k, int capA)
{
    return reinterpret_cast<int *>(static_cast<char *>(ws) + HEADER) + (size_t)k * 3 * cap_rows(capA);
}

__global__ __launch_bounds__(TB) void match_mutual_claims_kernel(const ClArgs a, int capA, int capB, void *__restrict__ ws)
{
    __shared__ int s_cnt[2][TB / 64];
    const int k = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * TB, i = row0 + tid;
    const int nA = clip(*a.d_nA[k], capA), nB = clip(*a.d_nB[k], capB);
    const int *__restrict__ mt = a.matches[k];
    int *__restrict__ res = a.result[k];
    float *__restrict__ fwd = a.fwd[k];
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
    float tau = __builtin_inff();
    if (claim) {
        tau = nmg::distance128(a.A[k] + (size_t)i * 128, a.B[k] + (size_t)j * 128);
        const size_t cr = cap_rows(capA);
        int *__restrict__ ci = claims_of(ws, k, capA);
        const int pos = all_below + before + __popcll(bal & ((1ull << lane) - 1ull));   // < nA <= capA
        ci[pos] = i;
        ci[cr + pos] = j;
        reinterpret_cast<float *>(ci + 2 * cr)[pos] = tau;
    }
    if (i < capA) {
        res[i] = (claim && tau == tau) ? j : -1;
        if (fwd) fwd[i] = tau;
    }
}

struct __attribute__((aligned(4))) Row16 { float v[NMM_CHUNK]; };

__global__ __launch_bounds__(TB) void match_mutual_scan_kernel(const ScArgs a, int capA, void *__restrict__ ws)
{
    const int k = blockIdx.z, tid = threadIdx.x;
    const int m = static_cast<const int *>(ws)[k];
    const int c0 = blockIdx.x * TB;
    if (c0 >= m) return;                                             // uniform: claim tiles beyond the pair's claims
    const int nA = clip(*a.d_nA[k], capA);
    const int per = (nA + SPLIT - 1) / SPLIT, r0 = blockIdx.y * per, r1 = r0 + per < nA ? r0 + per : nA;
    if (r0 >= r1) return;
    if (c0 + (tid & ~63) >= m) return;                               // uniform over the wave: no barrier follows
    const size_t cr = cap_rows(capA);
    const int *__restrict__ ci = claims_of(ws, k, capA);
    const float *__restrict__ Ad = a.A[k];
    const float *__restrict__ Bd = a.B[k];
    const int c = c0 + tid;
    const bool active = c < m;
    int i = 0;
    float tau = __builtin_nanf("");                                  // an idle lane and a NaN claim never keep a row alive
    float b[128];
    if (active) {
        i = ci[c];
        tau = reinterpret_cast<const float *>(ci + 2 * cr)[c];
        const nmg::Quad *__restrict__ src = reinterpret_cast<const nmg::Quad *>(Bd + (size_t)ci[cr + c] * 128);
#pragma unroll
        for (int q = 0; q < 32; ++q) {
            const nmg::Quad u = src[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) b[4 * q + e] = u.v[e];
        }
    } else {
#pragma unroll
        for (int q = 0; q < 128; ++q) b[q] = 0.f;
    }
    float tv = tau;                                                  // tau while the claim stands, NaN once it is beaten
    bool beaten = false;
#ifdef NMM_STATS
    const unsigned long long lanes = __popcll(__ballot(active));
    unsigned long long st_pairs = 0ull, st_chunks = 0ull;
#endif
    auto load = [&](int r, int ch) { return *reinterpret_cast<const Row16 *>(Ad + (size_t)r * 128 + ch * NMM_CHUNK); };
    Row16 cur = load(r0, 0);
    for (int r = r0; r < r1; ++r) {
        const Row16 nxt = load(r + 1 < r1 ? r + 1 : r, 0);           // the last row asks for itself: inside the pair's rows
        Row16 x = cur;
        float acc = 0.f;
        bool full = true;
#pragma unroll
        for (int ch = 0; ch < NMM_CHUNKS; ++ch) {
            acc = chunk(acc, x.v, b + ch * NMM_CHUNK);
#ifdef NMM_STATS
            st_chunks += lanes;
#endif
            if (ch + 1 < NMM_CHUNKS) {
                if (__ballot(alive(acc, tv)) == 0ull) { full = false; break; }   // uniform over the wave
                x = load(r, ch + 1);
            }
        }
#ifdef NMM_STATS
        st_pairs += lanes;
#endif
        if (full && beats(acc, r, tau, i)) { beaten = true; tv = __builtin_nanf(""); }
        cur = nxt;
    }
    if (active && !keep(tau, beaten) && tau == tau) a.result[k][i] = -1;   // plain store; every writer stores -1
#ifdef NMM_STATS
    if ((tid & 63) == 0) {
        unsigned long long *st = reinterpret_cast<unsigned long long *>(static_cast<char *>(ws) + 256);
        atomicAdd(st, st_pairs);
        atomicAdd(st + 1, st_chunks);
    }
#endif
}

// ---- the host twin: the same functions, claims and rival rows walked serially ----
void host_mutual_pair(const float *A, int nA, int capA, const float *B, int nB, const int *matches, int *result, int *count,
                      float *fwd)
{
    int kept = 0;
    for (int i = 0; i < capA; ++i) {
        int out = -1;
        float tau = __builtin_inff();
        const int j = i < nA ? matches[i] : -1;
        if (i < nA && is_claim(j, nB)) {
            const float *bj = B + (size_t)j * 128;
            tau = nmg::distance128(A + (size_t)i * 128, bj);
            bool beaten = false;
            if (tau == tau)
                for (int ip = 0; ip < nA && !beaten; ++ip) beaten = rival_beats(A + (size_t)ip * 128, bj, ip, tau, i, nullptr);
            if (keep(tau, beaten)) out = j;
        }
        result[i] = out;
        kept += out >= 0 ? 1 : 0;
        if (fwd) fwd[i] = tau;
    }
    *count = kept;
}

bool mu_args_ok(int n, const float *const *A, const int *const *nA, int capA, const float *const *B, const int *const *nB,
                int capB, const int *const *matches, int *const *result, const int *count, float *const *fwd)
{
    return nmp::range_ok(n, capA) && nmp::cap_ok(capB) && nmp::tables_ok(n, {A, nA, B, nB, matches, result}, {fwd}, {count});
}

}  // namespace

extern "C" size_t nm_sift_match_mutual_workspace_bytes(int n, int capA)
{
    if (!nmp::range_ok(n, capA)) return 0;
    return HEADER + (size_t)n * 3 * cap_rows(capA) * sizeof(int);
}

extern "C" int nm_sift_match_mutual_batch_dev_f32(int n, const float *const *A, const int *const *d_nA, int capA,
                                                  const float *const *B, const int *const *d_nB, int capB,
                                                  const int *const *matches, int *const *result, int *count,
                                                  float *const *forward_distance, void *workspace, void *stream)
{
    if (!mu_args_ok(n, A, d_nA, capA, B, d_nB, capB, matches, result, count, forward_distance) || !workspace)
        return (int)hipErrorInvalidValue;
    ClArgs c;
    ScArgs s;
    nmp::fill_slots(c.A, A, 0, n); nmp::fill_slots(c.d_nA, d_nA, 0, n); nmp::fill_slots(c.B, B, 0, n);
    nmp::fill_slots(c.d_nB, d_nB, 0, n); nmp::fill_slots(c.matches, matches, 0, n); nmp::fill_slots(c.result, result, 0, n);
    nmp::fill_slots(c.fwd, forward_distance, 0, n);
    nmp::fill_slots(s.A, A, 0, n); nmp::fill_slots(s.d_nA, d_nA, 0, n); nmp::fill_slots(s.B, B, 0, n);
    nmp::fill_slots(s.result, result, 0, n);
    const int tiles = nm_divup(capA, TB);
    hipLaunchKernelGGL(match_mutual_claims_kernel, dim3(tiles, n), dim3(TB), 0, nm_stream(stream), c, capA, capB, workspace);
    NM_LAUNCH_CHECK();
    hipLaunchKernelGGL(match_mutual_scan_kernel, dim3(tiles, SPLIT, n), dim3(TB), 0, nm_stream(stream), s, capA, workspace);
    NM_LAUNCH_CHECK();
    return nmp::launch_pair_count(n, result, capA, count, nm_stream(stream));
}

extern "C" int nm_sift_match_mutual_host_f32(int n, const float *const *A, const int *const *nA, int capA,
                                             const float *const *B, const int *const *nB, int capB,
                                             const int *const *matches, int *const *result, int *count,
                                             float *const *forward_distance)
{
    if (!mu_args_ok(n, A, nA, capA, B, nB, capB, matches, result, count, forward_distance)) return (int)hipErrorInvalidValue;
    for (int k = 0; k < n; ++k)
        host_mutual_pair(A[k], clip(*nA[k], capA), capA, B[k], clip(*nB[k], capB), matches[k], result[k], count + k,
                         forward_distance ? forward_distance[k] : nullptr);
    return 0;
}
