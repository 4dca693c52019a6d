// nm_match_guided.hip -- batched homography-guided matching for gfx950, of fp32 rows (nm_sift_match_guided_batch_dev_f32)
// and of unsigned-char rows (nm_sift_match_guided_u8_batch_dev, the guided stage of the byte pipeline: finish -> u8 match
// -> mutual u8 -> RANSAC -> refit -> this -> refit). No reference counterpart: the reference's matcher is blind,
// kernels/match.cu, and nothing returns to the descriptors once a model is known.
// THREE launches per call whatever n is, on the caller's stream, no allocation, no synchronisation, no workspace: the pair
// slots 0-31 and 32-63 (ten pointer tables of 32 entries are 2.5 KB of the 4 KB of kernel arguments; the launch of a half
// without pairs is one workgroup that returns at once), then the counts.
// ONE kernel, host twin, argument check and launcher for both element types, over a row policy (nmg::RowsF32,
// nmg8::RowsU8): what a lane keeps of its own row, and the distance of a noted candidate. fp32: the row's address, and the
// reference's 128-D chain, sequential in k on one lane. u8: the row's 128 bytes, loaded ONCE into 32 registers (no copy
// of them is ever made: the flush is forced inline), and |a|^2; a candidate is eight 16-byte loads and, per dword, one
// v_dot4_u32_u8 for a.b and one for |b|^2; d = |a|^2 + |b|^2 - 2 a.b is an exact integer and (float)d the value of the
// fp32 chain on float copies of the bytes.
// One lane per source row. The row is projected once (two IEEE divides); the candidates' coordinates stream through LDS in
// tiles of TILE and are read by broadcast, CHUNK gate tests (5 fp32 operations each) between two looks at the outcome. A
// hit is not followed at once: the lane notes the candidate in a list of NMG_LIST entries in LDS, and when a list of the
// wave is full (and at the end) the wave computes the noted distances side by side, each lane walking its own list in
// ascending candidate order through the reference's scan. No atomics: a pair's outputs depend on that pair's inputs alone.
// The arithmetic is nm_match_guided_math.hpp (projection, gate, scan, fp32 rows) and nm_match_guided_u8_math.hpp (u8
// rows), shared with the host twin below: device and host agree bit for bit, and the u8 entry with the fp32 one on float
// copies of the bytes.
#include <cmath>

#include "nm_common.hpp"
#include "nm_match_guided_math.hpp"
#include "nm_match_guided_u8_math.hpp"
#include "nm_match_u8_dev.hpp"
#include "nm_pair_batch.hpp"
#include "../../include/nm_abi.h"

#ifndef NMG_LIST
#define NMG_LIST 4                         // noted hits per lane between two distance rounds; 1 = follow every hit at once
#endif

namespace {

using namespace nmg;
using nmg8::RowsU8;

constexpr int TB = 256;                    // source rows per workgroup
constexpr int TILE = 1024;                 // candidates per LDS tile (8 KB)
constexpr int CHUNK = 8;                   // gate tests between two looks at the outcome
constexpr int SLOTS = 32;                  // pairs per launch
static_assert(NM_MATCH_GUIDED_MAX_BATCH == 2 * SLOTS, "header and kernel disagree");
static_assert(NM_MATCH_GUIDED_U8_MAX_BATCH == 2 * SLOTS && NM_MATCH_GUIDED_U8_MAX_BATCH == nmp::MAX_BATCH,
              "header, kernel and pair-batch convention disagree");
static_assert(TILE % CHUNK == 0 && TB % 64 == 0 && NMG_LIST >= 1, "tile geometry");

template <class Rows> struct GdArgs {      // 10 x 32 pointers: 2.5 KB of the 4 KB of kernel arguments
    const typename Rows::Elem *A[SLOTS];
    const float *ax[SLOTS];
    const float *ay[SLOTS];
    const int *d_nA[SLOTS];
    const typename Rows::Elem *B[SLOTS];
    const float *bx[SLOTS];
    const float *by[SLOTS];
    const int *d_nB[SLOTS];
    int *result[SLOTS];
    float *best[SLOTS];                    // all NULL without a best_distance table
};
static_assert(sizeof(GdArgs<RowsF32>) + 96 < 4096 && sizeof(GdArgs<RowsU8>) == sizeof(GdArgs<RowsF32>),
              "guided-match kernel arguments exceed 4 KB");

// The noted candidates of the wave's lanes, list entry by list entry: every lane with an entry c takes the step of its own
// scan. `own` stays where it is (forced inline: a u8 row is 32 registers).
template <class Rows>
__device__ __forceinline__ void flush(Scan &sc, int &cnt, const int (*list)[TB], int tid, const typename Rows::Own &own,
                                      const typename Rows::Elem *Bd)
{
    for (int c = 0; c < NMG_LIST; ++c) {
        if (__ballot(cnt > c) == 0ull) break;
        if (cnt > c) {
            const int j = list[c][tid];
            scan_step(sc, j, Rows::distance(own, Bd, j));
        }
    }
    cnt = 0;
}

template <class Rows>
__global__ __launch_bounds__(TB) void match_guided_kernel(const GdArgs<Rows> a, int first, int n, int capA, int capB,
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
    const typename Rows::Elem *__restrict__ Bd = a.B[s];
    bool valid = i < nA;
    float px = __builtin_nanf(""), py = px;                          // NaN passes no gate: the lane only keeps the barriers
    if (valid) {
        const float x = a.ax[s][i];
        valid = x >= 0.f;                                            // RANSAC's valid-row rule
        if (valid) project(Hk, x, a.ay[s][i], px, py);
    }
    typename Rows::Own own;
    Rows::own(own, a.A[s], i, valid);
    Scan sc;
    scan_init(sc);
    int cnt = 0;
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
                    if (__ballot(cnt == NMG_LIST) != 0ull) flush<Rows>(sc, cnt, list, tid, own, Bd);
                }
            }
        }
    }
    if (__ballot(cnt > 0) != 0ull) flush<Rows>(sc, cnt, list, tid, own, Bd);
    if (i < capA) {
        res[i] = valid ? decide(sc, ambiguity, max_distance) : -1;
        if (best) best[i] = sc.min1;                                 // +inf without a candidate
    }
}

// ---- the host twin: the same functions, rows and candidates walked serially ----
template <class Rows>
void host_guided_pair(const typename Rows::Elem *A, const float *ax, const float *ay, int nA, int capA,
                      const typename Rows::Elem *B, const float *bx, const float *by, int nB, const float *H, int status_in,
                      float radius2, float ambiguity, float max_distance, int *result, int *count, float *best)
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
            typename Rows::Own own;
            Rows::own(own, A, i, true);
            for (int j = 0; j < nB; ++j)
                if (gate(px, py, bx[j], by[j], radius2)) scan_step(sc, j, Rows::distance(own, B, j));
        }
        result[i] = valid ? decide(sc, ambiguity, max_distance) : -1;
        c += result[i] >= 0 ? 1 : 0;
        if (best) best[i] = sc.min1;
    }
    *count = c;
}

template <class Elem>
bool gd_args_ok(int n, const Elem *const *A, const float *const *ax, const float *const *ay, const int *const *nA, int capA,
                const Elem *const *B, const float *const *bx, const float *const *by, const int *const *nB, int capB,
                const float *H, float radius2, float ambiguity, float max_distance, int *const *result, const int *count,
                float *const *best)
{
    if (!std::isfinite(radius2) || !std::isfinite(ambiguity) || std::isnan(max_distance)) return false;
    return nmp::range_ok(n, capA) && nmp::cap_ok(capB) &&
           nmp::tables_ok(n, {A, ax, ay, nA, B, bx, by, nB, result}, {best}, {H, count});
}

// The two halves of the slots, then the counts
template <class Rows>
int launch_guided(int n, const typename Rows::Elem *const *A, const float *const *ax, const float *const *ay,
                  const int *const *d_nA, int capA, const typename Rows::Elem *const *B, const float *const *bx,
                  const float *const *by, const int *const *d_nB, int capB, const float *H, const int *status_in,
                  float radius2, float ambiguity, float max_distance, int *const *result, int *count,
                  float *const *best_distance, hipStream_t stream)
{
    for (int first = 0; first < nmp::MAX_BATCH; first += SLOTS) {
        GdArgs<Rows> a;
        nmp::fill_slots(a.A, A, first, n); nmp::fill_slots(a.ax, ax, first, n); nmp::fill_slots(a.ay, ay, first, n);
        nmp::fill_slots(a.d_nA, d_nA, first, n);
        nmp::fill_slots(a.B, B, first, n); nmp::fill_slots(a.bx, bx, first, n); nmp::fill_slots(a.by, by, first, n);
        nmp::fill_slots(a.d_nB, d_nB, first, n);
        nmp::fill_slots(a.result, result, first, n);
        nmp::fill_slots(a.best, best_distance, first, n);
        const int pairs = n - first < 0 ? 0 : (n - first > SLOTS ? SLOTS : n - first);
        const dim3 grid = pairs ? dim3(nm_divup(capA, TB), pairs) : dim3(1, 1);
        hipLaunchKernelGGL(match_guided_kernel<Rows>, grid, dim3(TB), 0, stream, a, first, n, capA, capB, H, status_in,
                           radius2, ambiguity, max_distance);
        NM_LAUNCH_CHECK();
    }
    return nmp::launch_pair_count(n, result, capA, count, stream);
}

template <class Rows>
int host_guided(int n, const typename Rows::Elem *const *A, const float *const *ax, const float *const *ay,
                const int *const *nA, int capA, const typename Rows::Elem *const *B, const float *const *bx,
                const float *const *by, const int *const *nB, int capB, const float *H, const int *status_in, float radius2,
                float ambiguity, float max_distance, int *const *result, int *count, float *const *best_distance)
{
    for (int k = 0; k < n; ++k)
        host_guided_pair<Rows>(A[k], ax[k], ay[k], clip(*nA[k], capA), capA, B[k], bx[k], by[k], clip(*nB[k], capB),
                               H + 9 * k, status_in ? status_in[k] : 1, radius2, ambiguity, max_distance, result[k],
                               count + k, best_distance ? best_distance[k] : nullptr);
    return 0;
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
    return launch_guided<RowsF32>(n, A, ax, ay, d_nA, capA, B, bx, by, d_nB, capB, H, status_in, radius2, ambiguity,
                                  max_distance, result, count, best_distance, nm_stream(stream));
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
    return host_guided<RowsF32>(n, A, ax, ay, nA, capA, B, bx, by, nB, capB, H, status_in, radius2, ambiguity, max_distance,
                                result, count, best_distance);
}

extern "C" int nm_sift_match_guided_u8_batch_dev(int n, const unsigned char *const *A, const float *const *ax,
                                                 const float *const *ay, const int *const *d_nA, int capA,
                                                 const unsigned char *const *B, const float *const *bx,
                                                 const float *const *by, const int *const *d_nB, int capB, const float *H,
                                                 const int *status_in, float radius2, float ambiguity, float max_distance,
                                                 int *const *result, int *count, float *const *best_distance, void *stream)
{
    if (!gd_args_ok(n, A, ax, ay, d_nA, capA, B, bx, by, d_nB, capB, H, radius2, ambiguity, max_distance, result, count,
                    best_distance) ||
        !nmu8::aligned16(n, A) || !nmu8::aligned16(n, B))            // 16-byte reads of every row
        return (int)hipErrorInvalidValue;
    return launch_guided<RowsU8>(n, A, ax, ay, d_nA, capA, B, bx, by, d_nB, capB, H, status_in, radius2, ambiguity,
                                 max_distance, result, count, best_distance, nm_stream(stream));
}

extern "C" int nm_sift_match_guided_u8_host(int n, const unsigned char *const *A, const float *const *ax,
                                            const float *const *ay, const int *const *nA, int capA,
                                            const unsigned char *const *B, const float *const *bx, const float *const *by,
                                            const int *const *nB, int capB, const float *H, const int *status_in,
                                            float radius2, float ambiguity, float max_distance, int *const *result,
                                            int *count, float *const *best_distance)
{
    if (!gd_args_ok(n, A, ax, ay, nA, capA, B, bx, by, nB, capB, H, radius2, ambiguity, max_distance, result, count,
                    best_distance))                                  // no alignment rule on the host
        return (int)hipErrorInvalidValue;
    return host_guided<RowsU8>(n, A, ax, ay, nA, capA, B, bx, by, nB, capB, H, status_in, radius2, ambiguity, max_distance,
                               result, count, best_distance);
}
