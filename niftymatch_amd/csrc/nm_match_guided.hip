// nm_match_guided.hip -- batched homography-guided matching for gfx950 (no reference counterpart: the reference's matcher is
// blind, kernels/match.cu, and nothing returns to the descriptors once a model is known).
// THREE launches per call whatever n is, on the caller's stream, no allocation, no synchronisation, no workspace: the pair
// slots 0-31 and 32-63 (ten pointer tables of 32 entries are 2.5 KB of the 4 KB of kernel arguments; the launch of a half
// without pairs is one workgroup that returns at once), then the counts.
// One lane per source row. The row is projected once (two IEEE divides); the candidates' coordinates stream through LDS in
// tiles of TILE and are read by broadcast, CHUNK gate tests (5 fp32 operations each) between two looks at the outcome. A
// hit is not followed at once: the lane notes the candidate in a list of NMG_LIST entries in LDS, and when a list of the
// wave is full (and at the end) the wave computes the noted 128-D distances side by side, each lane walking its own list in
// ascending candidate order through the reference's scan. The chain of a distance is sequential in k and stays on one lane.
// No atomics: a pair's outputs depend on that pair's inputs alone.
// The arithmetic is nm_match_guided_math.hpp, shared with the host twin below: both agree bit for bit.
#include <cmath>

#include "nm_common.hpp"
#include "nm_match_guided_math.hpp"
#include "nm_pair_batch.hpp"
#include "../../include/nm_abi.h"

#ifndef NMG_LIST
#define NMG_LIST 4                         // noted hits per lane between two distance rounds; 1 = follow every hit at once
#endif

namespace {

using namespace nmg;

constexpr int TB = 256;                    // source rows per workgroup
constexpr int TILE = 1024;                 // candidates per LDS tile (8 KB)
constexpr int CHUNK = 8;                   // gate tests between two looks at the outcome
constexpr int SLOTS = 32;                  // pairs per launch
static_assert(NM_MATCH_GUIDED_MAX_BATCH == 2 * SLOTS, "header and kernel disagree");
static_assert(TILE % CHUNK == 0 && TB % 64 == 0 && NMG_LIST >= 1, "tile geometry");

struct GdArgs {                            // 10 x 32 pointers: 2.5 KB of the 4 KB of kernel arguments
    const float *A[SLOTS];
    const float *ax[SLOTS];
    const float *ay[SLOTS];
    const int *d_nA[SLOTS];
    const float *B[SLOTS];
    const float *bx[SLOTS];
    const float *by[SLOTS];
    const int *d_nB[SLOTS];
    int *result[SLOTS];
    float *best[SLOTS];                    // all NULL without a best_distance table
};
static_assert(sizeof(GdArgs) + 96 < 4096, "guided-match kernel arguments exceed 4 KB");

__global__ __launch_bounds__(TB) void match_guided_kernel(const GdArgs a, int first, int n, int capA, int capB,
                                                          const float *__restrict__ H, const int *__restrict__ status_in,
                                                          float radius2, float ambiguity, float max_distance)
{
    __shared__ float tx[TILE], ty[TILE];                             // apart: packed fp32 operations take pairs as they lie
    __shared__ int list[NMG_LIST][TB];
    const int s = blockIdx.y, k = first + s;
    if (k >= n) return;                                              // the idle half of a small batch
    const int tid = threadIdx.x, row0 = blockIdx.x * TB, i = row0 + tid;
    int *__restrict__ res = a.result[s];
    float *__restrict__ best = a.best[s];
    float Hk[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) Hk[q] = H[k * 9 + q];
    const int nA = clip(*a.d_nA[s], capA), nB = clip(*a.d_nB[s], capB);
    const bool usable = (!status_in || status_in[k] == 1) && finite9(Hk);
    if (!usable || row0 >= nA || nB == 0) {                          // uniform over the workgroup
        if (i < capA) {
            res[i] = -1;
            if (best) best[i] = __builtin_inff();
        }
        return;
    }
    const float *__restrict__ bx = a.bx[s], *__restrict__ by = a.by[s];
    const float *__restrict__ Ad = a.A[s], *__restrict__ Bd = a.B[s];
    bool valid = i < nA;
    float px = __builtin_nanf(""), py = px;                          // NaN passes no gate: the lane only keeps the barriers
    if (valid) {
        const float x = a.ax[s][i];
        valid = x >= 0.f;                                            // RANSAC's valid-row rule
        if (valid) project(Hk, x, a.ay[s][i], px, py);
    }
    Scan sc;
    scan_init(sc);
    int cnt = 0;
    // the noted candidates of the wave's lanes, list entry by list entry: converged 128-D chains
    auto flush = [&]() {
        for (int c = 0; c < NMG_LIST; ++c) {
            if (__ballot(cnt > c) == 0ull) break;
            if (cnt > c) {
                const int j = list[c][tid];
                scan_step(sc, j, distance128(Ad + (size_t)i * 128, Bd + (size_t)j * 128));
            }
        }
        cnt = 0;
    };
    for (int t0 = 0; t0 < nB; t0 += TILE) {
        __syncthreads();
        for (int q = tid; q < TILE; q += TB) {
            const int j = t0 + q;
            tx[q] = j < nB ? bx[j] : __builtin_nanf("");
            ty[q] = j < nB ? by[j] : __builtin_nanf("");
        }
        __syncthreads();
        const int left = nB - t0, m = left < TILE ? (left + CHUNK - 1) / CHUNK * CHUNK : TILE;
        for (int q = 0; q < m; q += CHUNK) {
            unsigned long long hits = 0ull;                          // lanes of the wave with a hit in this chunk
#pragma unroll
            for (int u = 0; u < CHUNK; ++u) hits |= __ballot(gate(px, py, tx[q + u], ty[q + u], radius2));
            if (hits != 0ull) {                                      // uniform over the wave, and rare
                for (int u = 0; u < CHUNK; ++u) {
                    if (gate(px, py, tx[q + u], ty[q + u], radius2)) { list[cnt][tid] = t0 + q + u; ++cnt; }
                    if (__ballot(cnt == NMG_LIST) != 0ull) flush();
                }
            }
        }
    }
    if (__ballot(cnt > 0) != 0ull) flush();
    if (i < capA) {
        res[i] = valid ? decide(sc, ambiguity, max_distance) : -1;
        if (best) best[i] = sc.min1;                                 // +inf without a candidate
    }
}

// ---- the host twin: the same functions, rows and candidates walked serially ----
void host_guided_pair(const float *A, const float *ax, const float *ay, int nA, int capA, const float *B, const float *bx,
                      const float *by, int nB, const float *H, int status_in, float radius2, float ambiguity,
                      float max_distance, int *result, int *count, float *best)
{
    const bool usable = status_in == 1 && finite9(H);
    int c = 0;
    for (int i = 0; i < capA; ++i) {
        Scan sc;
        scan_init(sc);
        const bool valid = usable && i < nA && ax[i] >= 0.f;
        if (valid) {
            float px, py;
            project(H, ax[i], ay[i], px, py);
            for (int j = 0; j < nB; ++j)
                if (gate(px, py, bx[j], by[j], radius2)) scan_step(sc, j, distance128(A + (size_t)i * 128, B + (size_t)j * 128));
        }
        result[i] = valid ? decide(sc, ambiguity, max_distance) : -1;
        c += result[i] >= 0 ? 1 : 0;
        if (best) best[i] = sc.min1;
    }
    *count = c;
}

bool gd_args_ok(int n, const float *const *A, const float *const *ax, const float *const *ay, const int *const *nA, int capA,
                const float *const *B, const float *const *bx, const float *const *by, const int *const *nB, int capB,
                const float *H, float radius2, float ambiguity, float max_distance, int *const *result, const int *count,
                float *const *best)
{
    if (!std::isfinite(radius2) || !std::isfinite(ambiguity) || std::isnan(max_distance)) return false;
    return nmp::range_ok(n, capA) && nmp::cap_ok(capB) &&
           nmp::tables_ok(n, {A, ax, ay, nA, B, bx, by, nB, result}, {best}, {H, count});
}

}  // namespace

extern "C" int nm_sift_match_guided_batch_dev_f32(int n, const float *const *A, const float *const *ax,
                                                  const float *const *ay, const int *const *d_nA, int capA,
                                                  const float *const *B, const float *const *bx, const float *const *by,
                                                  const int *const *d_nB, int capB, const float *H, const int *status_in,
                                                  float radius2, float ambiguity, float max_distance, int *const *result,
                                                  int *count, float *const *best_distance, void *stream)
{
    if (!gd_args_ok(n, A, ax, ay, d_nA, capA, B, bx, by, d_nB, capB, H, radius2, ambiguity, max_distance, result, count,
                    best_distance))
        return (int)hipErrorInvalidValue;
    for (int first = 0; first < nmp::MAX_BATCH; first += SLOTS) {
        GdArgs a;
        nmp::fill_slots(a.A, A, first, n); nmp::fill_slots(a.ax, ax, first, n); nmp::fill_slots(a.ay, ay, first, n);
        nmp::fill_slots(a.d_nA, d_nA, first, n);
        nmp::fill_slots(a.B, B, first, n); nmp::fill_slots(a.bx, bx, first, n); nmp::fill_slots(a.by, by, first, n);
        nmp::fill_slots(a.d_nB, d_nB, first, n);
        nmp::fill_slots(a.result, result, first, n);
        nmp::fill_slots(a.best, best_distance, first, n);
        const int pairs = n - first < 0 ? 0 : (n - first > SLOTS ? SLOTS : n - first);
        const dim3 grid = pairs ? dim3(nm_divup(capA, TB), pairs) : dim3(1, 1);
        hipLaunchKernelGGL(match_guided_kernel, grid, dim3(TB), 0, nm_stream(stream), a, first, n, capA, capB, H, status_in,
                           radius2, ambiguity, max_distance);
        NM_LAUNCH_CHECK();
    }
    return nmp::launch_pair_count(n, result, capA, count, nm_stream(stream));
}

extern "C" int nm_sift_match_guided_host_f32(int n, const float *const *A, const float *const *ax, const float *const *ay,
                                             const int *const *nA, int capA, const float *const *B, const float *const *bx,
                                             const float *const *by, const int *const *nB, int capB, const float *H,
                                             const int *status_in, float radius2, float ambiguity, float max_distance,
                                             int *const *result, int *count, float *const *best_distance)
{
    if (!gd_args_ok(n, A, ax, ay, nA, capA, B, bx, by, nB, capB, H, radius2, ambiguity, max_distance, result, count,
                    best_distance))
        return (int)hipErrorInvalidValue;
    for (int k = 0; k < n; ++k)
        host_guided_pair(A[k], ax[k], ay[k], clip(*nA[k], capA), capA, B[k], bx[k], by[k], clip(*nB[k], capB), H + 9 * k,
                         status_in ? status_in[k] : 1, radius2, ambiguity, max_distance, result[k], count + k,
                         best_distance ? best_distance[k] : nullptr);
    return 0;
}
