// nm_match_guided_u8.hip -- batched homography-guided matching of unsigned-char descriptors for gfx950: the guided stage of
// the byte pipeline (finish -> u8 match -> mutual u8 -> RANSAC -> refit -> this -> refit), no reference counterpart.
// THREE launches per call whatever n is, on the caller's stream, no allocation, no synchronisation, no workspace: the pair
// slots 0-31 and 32-63, then the counts -- the launch shape of nm_match_guided.hip, whose gate loop this kernel repeats
// (folding the two kernels is left for later; the fp32 kernel is untouched).
// One lane per source row. The row is projected once; a valid lane then loads its own 128 bytes ONCE into 32 registers and
// forms |a|^2 with v_dot4_u32_u8. The candidates' coordinates stream through LDS in tiles of TILE, CHUNK gate tests between
// two looks at the outcome; a hit is noted in the lane's list of NMG8_LIST entries in LDS, and when a list of the wave is
// full (and at the end) the wave computes the noted distances side by side: a candidate is eight 16-byte loads and, per
// dword, one dot4 for a.b and one for |b|^2; d = |a|^2 + |b|^2 - 2 a.b is an exact integer and (float)d goes through the
// reference's scan in ascending candidate order. No atomics: a pair's outputs depend on that pair's inputs alone.
// The arithmetic is nm_match_guided_math.hpp (projection, gate, scan) and nm_match_guided_u8_math.hpp (distance), shared
// with the host twin below: both agree bit for bit, and with the fp32 entry on float copies of the bytes.
#include <cmath>

#include "nm_common.hpp"
#include "nm_match_guided_math.hpp"
#include "nm_match_guided_u8_math.hpp"
#include "nm_match_u8_dev.hpp"
#include "nm_pair_batch.hpp"
#include "../../include/nm_abi.h"

#ifndef NMG8_LIST
#define NMG8_LIST 4                        // noted hits per lane between two distance rounds
#endif

namespace {

using namespace nmg;

constexpr int TB = 256;                    // source rows per workgroup
constexpr int TILE = 1024;                 // candidates per LDS tile (8 KB)
constexpr int CHUNK = 8;                   // gate tests between two looks at the outcome
constexpr int SLOTS = 32;                  // pairs per launch
static_assert(NM_MATCH_GUIDED_U8_MAX_BATCH == 2 * SLOTS && NM_MATCH_GUIDED_U8_MAX_BATCH == nmp::MAX_BATCH,
              "header, kernel and pair-batch convention disagree");
static_assert(TILE % CHUNK == 0 && TB % 64 == 0 && NMG8_LIST >= 1, "tile geometry");

struct Gd8Args {                           // 10 x 32 pointers: 2.5 KB of the 4 KB of kernel arguments
    const unsigned char *A[SLOTS];
    const float *ax[SLOTS];
    const float *ay[SLOTS];
    const int *d_nA[SLOTS];
    const unsigned char *B[SLOTS];
    const float *bx[SLOTS];
    const float *by[SLOTS];
    const int *d_nB[SLOTS];
    int *result[SLOTS];
    float *best[SLOTS];                    // all NULL without a best_distance table
};
static_assert(sizeof(Gd8Args) + 96 < 4096, "guided-match kernel arguments exceed 4 KB");

// The noted candidates of the wave's lanes, list entry by list entry: every lane with an entry c reads its candidate's row
// and takes the step of its own scan. `row` / `aa` stay in registers (forced inline: no copy of the row is ever made).
__device__ __forceinline__ void flush(Scan &sc, int &cnt, const int (*list)[TB], int tid, const nmg8::Row &row, unsigned aa,
                                      const unsigned char *__restrict__ Bd)
{
    for (int c = 0; c < NMG8_LIST; ++c) {
        if (__ballot(cnt > c) == 0ull) break;
        if (cnt > c) {
            const int j = list[c][tid];
            nmg8::Row b;
            nmg8::load_row(b, Bd + (size_t)j * nmg8::DIM);
            scan_step(sc, j, (float)nmg8::distance(row, aa, b));
        }
    }
    cnt = 0;
}

__global__ __launch_bounds__(TB) void match_guided_u8_kernel(const Gd8Args a, int first, int n, int capA, int capB,
                                                             const float *__restrict__ H, const int *__restrict__ status_in,
                                                             float radius2, float ambiguity, float max_distance)
{
    __shared__ float tx[TILE], ty[TILE];                             // apart: packed fp32 operations take pairs as they lie
    __shared__ int list[NMG8_LIST][TB];
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
    const unsigned char *__restrict__ Bd = a.B[s];
    bool valid = i < nA;
    float px = __builtin_nanf(""), py = px;                          // NaN passes no gate: the lane only keeps the barriers
    if (valid) {
        const float x = a.ax[s][i];
        valid = x >= 0.f;                                            // RANSAC's valid-row rule
        if (valid) project(Hk, x, a.ay[s][i], px, py);
    }
    nmg8::Row row = {};                                              // the lane's own row, read once (rows beyond nA: never)
    if (valid) nmg8::load_row(row, a.A[s] + (size_t)i * nmg8::DIM);
    const unsigned aa = nmg8::norm2(row);
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
                    if (__ballot(cnt == NMG8_LIST) != 0ull) flush(sc, cnt, list, tid, row, aa, Bd);
                }
            }
        }
    }
    if (__ballot(cnt > 0) != 0ull) flush(sc, cnt, list, tid, row, aa, Bd);
    if (i < capA) {
        res[i] = valid ? decide(sc, ambiguity, max_distance) : -1;
        if (best) best[i] = sc.min1;                                 // +inf without a candidate
    }
}

// ---- the host twin: the same functions, rows and candidates walked serially ----
void host_guided_u8_pair(const unsigned char *A, const float *ax, const float *ay, int nA, int capA, const unsigned char *B,
                         const float *bx, const float *by, int nB, const float *H, int status_in, float radius2,
                         float ambiguity, float max_distance, int *result, int *count, float *best)
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
            nmg8::Row row, b;
            nmg8::load_row(row, A + (size_t)i * nmg8::DIM);
            const unsigned aa = nmg8::norm2(row);
            for (int j = 0; j < nB; ++j)
                if (gate(px, py, bx[j], by[j], radius2)) {
                    nmg8::load_row(b, B + (size_t)j * nmg8::DIM);
                    scan_step(sc, j, (float)nmg8::distance(row, aa, b));
                }
        }
        result[i] = valid ? decide(sc, ambiguity, max_distance) : -1;
        c += result[i] >= 0 ? 1 : 0;
        if (best) best[i] = sc.min1;
    }
    *count = c;
}

bool gd8_args_ok(int n, const unsigned char *const *A, const float *const *ax, const float *const *ay, const int *const *nA,
                 int capA, const unsigned char *const *B, const float *const *bx, const float *const *by,
                 const int *const *nB, int capB, const float *H, float radius2, float ambiguity, float max_distance,
                 int *const *result, const int *count, float *const *best)
{
    if (!std::isfinite(radius2) || !std::isfinite(ambiguity) || std::isnan(max_distance)) return false;
    return nmp::range_ok(n, capA) && nmp::cap_ok(capB) &&
           nmp::tables_ok(n, {A, ax, ay, nA, B, bx, by, nB, result}, {best}, {H, count});
}

}  // namespace

extern "C" int nm_sift_match_guided_u8_batch_dev(int n, const unsigned char *const *A, const float *const *ax,
                                                 const float *const *ay, const int *const *d_nA, int capA,
                                                 const unsigned char *const *B, const float *const *bx,
                                                 const float *const *by, const int *const *d_nB, int capB, const float *H,
                                                 const int *status_in, float radius2, float ambiguity, float max_distance,
                                                 int *const *result, int *count, float *const *best_distance, void *stream)
{
    if (!gd8_args_ok(n, A, ax, ay, d_nA, capA, B, bx, by, d_nB, capB, H, radius2, ambiguity, max_distance, result, count,
                     best_distance) ||
        !nmu8::aligned16(n, A) || !nmu8::aligned16(n, B))            // 16-byte reads of every row
        return (int)hipErrorInvalidValue;
    for (int first = 0; first < nmp::MAX_BATCH; first += SLOTS) {
        Gd8Args a;
        nmp::fill_slots(a.A, A, first, n); nmp::fill_slots(a.ax, ax, first, n); nmp::fill_slots(a.ay, ay, first, n);
        nmp::fill_slots(a.d_nA, d_nA, first, n);
        nmp::fill_slots(a.B, B, first, n); nmp::fill_slots(a.bx, bx, first, n); nmp::fill_slots(a.by, by, first, n);
        nmp::fill_slots(a.d_nB, d_nB, first, n);
        nmp::fill_slots(a.result, result, first, n);
        nmp::fill_slots(a.best, best_distance, first, n);
        const int pairs = n - first < 0 ? 0 : (n - first > SLOTS ? SLOTS : n - first);
        const dim3 grid = pairs ? dim3(nm_divup(capA, TB), pairs) : dim3(1, 1);
        hipLaunchKernelGGL(match_guided_u8_kernel, grid, dim3(TB), 0, nm_stream(stream), a, first, n, capA, capB, H,
                           status_in, radius2, ambiguity, max_distance);
        NM_LAUNCH_CHECK();
    }
    return nmp::launch_pair_count(n, result, capA, count, nm_stream(stream));
}

extern "C" int nm_sift_match_guided_u8_host(int n, const unsigned char *const *A, const float *const *ax,
                                            const float *const *ay, const int *const *nA, int capA,
                                            const unsigned char *const *B, const float *const *bx, const float *const *by,
                                            const int *const *nB, int capB, const float *H, const int *status_in,
                                            float radius2, float ambiguity, float max_distance, int *const *result,
                                            int *count, float *const *best_distance)
{
    if (!gd8_args_ok(n, A, ax, ay, nA, capA, B, bx, by, nB, capB, H, radius2, ambiguity, max_distance, result, count,
                     best_distance))
        return (int)hipErrorInvalidValue;
    for (int k = 0; k < n; ++k)
        host_guided_u8_pair(A[k], ax[k], ay[k], clip(*nA[k], capA), capA, B[k], bx[k], by[k], clip(*nB[k], capB), H + 9 * k,
                            status_in ? status_in[k] : 1, radius2, ambiguity, max_distance, result[k], count + k,
                            best_distance ? best_distance[k] : nullptr);
    return 0;
}
