// nm_match_mutual.hip -- batched mutual-nearest-neighbour filtering of a match list for gfx950 (no reference counterpart: the
// reference's matcher, kernels/match.cu, tests one direction only and a client cross-checks with a second, swapped call).
// The three launches of a call (claims, scan, counts), the claims stage and the entries' skeleton are
// nm_match_claims_dev.hpp, shared with the u8 filter (nm_match_mutual_u8.hip). This file's own:
//   the Metric: tau = nmg::distance128 (one full chain per lane), kept as a float in the third claim array; a NaN tau yields
//      -1 at once and never reaches a verdict in the scan.
//   the scan (the hot path): one lane per claim, its column B[j] in 128 registers. The rows of A are the same for every
//      lane of a wave: they are read through a const __restrict__ pointer at wave-uniform addresses (scalar loads of 16
//      dwords; no LDS), NMM_CHUNK dimensions at a time; chunk 0 of the next row is requested while chunk 0 of this row is
//      computed, a later chunk only once the vote has asked for it (hipcc sinks an earlier request below the vote's branch
//      anyway). After each chunk the wave votes; when no lane has acc <= tau the row is abandoned. A row that runs to the
//      end is judged by nmp::beats.
// The chain of a distance is sequential in q and stays on one lane. No atomics (the NMM_STATS scratch build adds two
// counters). The arithmetic is nm_match_mutual_math.hpp, shared with the host twin below: both agree bit for bit.
#include "nm_common.hpp"
#include "nm_match_claims_dev.hpp"
#include "nm_match_mutual_math.hpp"
#include "../../include/nm_abi.h"

namespace {

using namespace nmm;
using nmc::SPLIT;
using nmc::TB;

struct F32Metric {
    using Elem = float;
    using Tau = float;
    static constexpr int DIM = 128;
    static constexpr int HEADER = 512;     // workspace: int m[64], then the two NMM_STATS counters at byte 256
    static_assert(nmp::MAX_BATCH * sizeof(int) <= 256, "workspace header");
    __host__ __device__ static size_t claim_rows(int capA) { return ((size_t)capA + 63) / 64 * 64; }
    // pair k's compacted claims: rows i, columns j, distances tau, claim_rows(capA) entries each
    __host__ __device__ static int *claims_of(void *ws, int k, int capA)
    {
        return reinterpret_cast<int *>(static_cast<char *>(ws) + HEADER) + (size_t)k * 3 * claim_rows(capA);
    }
    __device__ static float tau_of(const float *a, const float *b) { return nmg::distance128(a, b); }
    __device__ static void store_claim(int *t, size_t, int pos, float tau) { reinterpret_cast<float *>(t)[pos] = tau; }
    __device__ static bool yields(float tau) { return tau == tau; }
    __device__ static float forward(float tau) { return tau; }
    __device__ static void row_side(void *, int, int, const float *, int, int) {}
    static bool operands_ok(int, const float *const *, const float *const *, const void *) { return true; }
};

__global__ __launch_bounds__(TB) void match_mutual_claims_kernel(const nmc::ClaimTables<float> a, int capA, int capB,
                                                                 void *__restrict__ ws)
{
    nmc::match_claims<F32Metric>(a, capA, capB, ws);
}

struct __attribute__((aligned(4))) Row16 { float v[NMM_CHUNK]; };

__global__ __launch_bounds__(TB) void match_mutual_scan_kernel(const nmc::ScanTables<float> a, int capA, void *__restrict__ ws)
{
    const int k = blockIdx.z, tid = threadIdx.x;
    const int m = static_cast<const int *>(ws)[k];
    const int c0 = blockIdx.x * TB;
    if (c0 >= m) return;                                             // uniform: claim tiles beyond the pair's claims
    const int nA = clip(*a.d_nA[k], capA);
    const int per = (nA + SPLIT - 1) / SPLIT, r0 = blockIdx.y * per, r1 = r0 + per < nA ? r0 + per : nA;
    if (r0 >= r1) return;
    if (c0 + (tid & ~63) >= m) return;                               // uniform over the wave: no barrier follows
    const size_t cr = F32Metric::claim_rows(capA);
    const int *__restrict__ ci = F32Metric::claims_of(ws, k, capA);
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

}  // namespace

extern "C" size_t nm_sift_match_mutual_workspace_bytes(int n, int capA)
{
    if (!nmp::range_ok(n, capA)) return 0;
    return F32Metric::HEADER + (size_t)n * 3 * F32Metric::claim_rows(capA) * sizeof(int);
}

extern "C" int nm_sift_match_mutual_batch_dev_f32(int n, const float *const *A, const int *const *d_nA, int capA,
                                                  const float *const *B, const int *const *d_nB, int capB,
                                                  const int *const *matches, int *const *result, int *count,
                                                  float *const *forward_distance, void *workspace, void *stream)
{
    return nmc::launch_mutual<F32Metric>(match_mutual_claims_kernel, match_mutual_scan_kernel, n, A, d_nA, capA, B, d_nB, capB,
                                         matches, result, count, forward_distance, workspace, stream);
}

extern "C" int nm_sift_match_mutual_host_f32(int n, const float *const *A, const int *const *nA, int capA,
                                             const float *const *B, const int *const *nB, int capB,
                                             const int *const *matches, int *const *result, int *count,
                                             float *const *forward_distance)
{
    return nmc::host_mutual(host_mutual_pair, n, A, nA, capA, B, nB, capB, matches, result, count, forward_distance);
}
