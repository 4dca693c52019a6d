// nm_match_claims_dev.hpp -- what the two mutual filters (nm_match_mutual.hip, fp32; nm_match_mutual_u8.hip, u8) share: the
// kernel-argument tables, the claims stage and the skeleton of their entries. THREE launches per call whatever n is, on the
// caller's stream, no allocation, no synchronisation, no host read:
//   1. claims (grid ceil(capA / TB) x n, match_claims below): one lane per row of A. A workgroup counts the claims below its
//      first row from the match list itself (integers, so the ordered position of a claim needs no word from another
//      workgroup), computes tau = d(i, j) of its claiming rows, compacts (i, j, tau, ...) into the workspace by ordered
//      ballot, and writes the provisional result (j, or -1) and the forward distance of all its rows. Workgroup 0 of a pair
//      writes the pair's claim count m_k into the workspace header, where the scan reads it.
//   2. scan (grid ceil(capA / TB) x SPLIT x n, the filter's own): one lane per compacted claim against the rows of A, cut
//      into SPLIT ranges, one per workgroup. A workgroup that finds a claim beaten stores -1 over its provisional result:
//      several may store the same -1, nothing else is ever stored there, so the outcome does not depend on order.
//   3. counts (grid n, nm_pair_batch.hip): count[k] = entries >= 0 of result[k], integer sums.
// A filter supplies its scan kernel, its per-pair host twin and a Metric: Elem and DIM (a descriptor row), Tau (what
// tau_of(a_row, b_row) returns), the workspace layout claim_rows(capA) / claims_of(ws, k, capA) (pair k's claim arrays of
// claim_rows ints each: rows i, columns j, then what store_claim(third_array, cr, pos, tau) keeps), yields(tau) (false: the
// result is -1 at once), forward(tau) (the float of the forward-distance output), row_side(ws, k, capA, A, i, nA) (a per-row
// side output, every lane, may be empty) and operands_ok(n, A, B, ws) (host: what the device entry asks beyond args_ok).
#pragma once
#include "nm_common.hpp"
#include "nm_pair_batch.hpp"

namespace nmc {

using nmp::clip;
using nmp::fill_slots;
using nmp::is_claim;

constexpr int TB = 256;                     // rows (claims kernel) or claims (scan kernel) per workgroup
constexpr int SPLIT = 8;                    // ranges of a pair's rows in the scan kernel, one workgroup each

template <class T> struct ClaimTables {     // 7 x 64 pointers: 3.5 KB of the 4 KB of kernel arguments
    const T *A[nmp::MAX_BATCH];
    const int *d_nA[nmp::MAX_BATCH];
    const T *B[nmp::MAX_BATCH];
    const int *d_nB[nmp::MAX_BATCH];
    const int *matches[nmp::MAX_BATCH];
    int *result[nmp::MAX_BATCH];
    float *fwd[nmp::MAX_BATCH];             // all NULL without a forward_distance table
    void fill(int n, const T *const *a, const int *const *nA, const T *const *b, const int *const *nB, const int *const *mt,
              int *const *res, float *const *forward)
    {
        fill_slots(A, a, 0, n); fill_slots(d_nA, nA, 0, n); fill_slots(B, b, 0, n); fill_slots(d_nB, nB, 0, n);
        fill_slots(matches, mt, 0, n); fill_slots(result, res, 0, n); fill_slots(fwd, forward, 0, n);
    }
};
static_assert(sizeof(ClaimTables<float>) + 64 < 4096, "claims kernel arguments exceed 4 KB");

template <class T> struct ScanTables {
    const T *A[nmp::MAX_BATCH];
    const int *d_nA[nmp::MAX_BATCH];
    const T *B[nmp::MAX_BATCH];
    int *result[nmp::MAX_BATCH];
    void fill(int n, const T *const *a, const int *const *nA, const T *const *b, int *const *res)
    {
        fill_slots(A, a, 0, n); fill_slots(d_nA, nA, 0, n); fill_slots(B, b, 0, n); fill_slots(result, res, 0, n);
    }
};

// The claims stage; a filter's claims kernel is this body under the filter's kernel name. m_k is int k of the workspace.
template <class Metric>
__device__ __forceinline__ void match_claims(const ClaimTables<typename Metric::Elem> &a, int capA, int capB,
                                             void *__restrict__ ws)
{
    __shared__ int s_below[TB / 64], s_cnt[TB / 64];
    const int k = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * TB, i = row0 + tid;
    const int nA = clip(*a.d_nA[k], capA), nB = clip(*a.d_nB[k], capB);
    const int *__restrict__ mt = a.matches[k];
    int *__restrict__ res = a.result[k];
    float *__restrict__ fwd = a.fwd[k];
    Metric::row_side(ws, k, capA, a.A[k], i, nA);
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
    below = nmw::wave_sum(below);
    int j = -1;
    bool claim = false;
    if (i < nA) {
        j = mt[i];
        claim = is_claim(j, nB);
    }
    if (lane == 0) s_below[wave] = below;                            // read behind block_rank's barrier
    int claims;
    const int rank = nmw::block_rank<TB / 64>(claim, s_cnt, claims);
    int all_below = 0;
#pragma unroll
    for (int w = 0; w < TB / 64; ++w) all_below += s_below[w];
    if (blockIdx.x == 0) {
        if (tid == 0) static_cast<int *>(ws)[k] = all_below;         // m_k
        all_below = 0;                                               // workgroup 0 has nothing below it
    }
    typename Metric::Tau tau{};
    if (claim) {
        tau = Metric::tau_of(a.A[k] + (size_t)i * Metric::DIM, a.B[k] + (size_t)j * Metric::DIM);
        const size_t cr = Metric::claim_rows(capA);
        int *__restrict__ ci = Metric::claims_of(ws, k, capA);
        const int pos = all_below + rank;                            // < nA <= capA
        ci[pos] = i;
        ci[cr + pos] = j;
        Metric::store_claim(ci + 2 * cr, cr, pos, tau);
    }
    if (i < capA) {
        res[i] = (claim && Metric::yields(tau)) ? j : -1;
        if (fwd) fwd[i] = claim ? Metric::forward(tau) : __builtin_inff();
    }
}

template <class T>
bool args_ok(int n, const T *const *A, const int *const *nA, int capA, const T *const *B, const int *const *nB, int capB,
             const int *const *matches, int *const *result, const int *count, float *const *fwd)
{
    return nmp::range_ok(n, capA) && nmp::cap_ok(capB) && nmp::tables_ok(n, {A, nA, B, nB, matches, result}, {fwd}, {count});
}

// The device entry of a filter: the checks, the tables, claims, scan, counts.
template <class Metric, class T = typename Metric::Elem>
int launch_mutual(void (*claims)(ClaimTables<T>, int, int, void *), void (*scan)(ScanTables<T>, int, void *), int n,
                  const T *const *A, const int *const *d_nA, int capA, const T *const *B, const int *const *d_nB, int capB,
                  const int *const *matches, int *const *result, int *count, float *const *forward_distance, void *workspace,
                  void *stream)
{
    if (!args_ok(n, A, d_nA, capA, B, d_nB, capB, matches, result, count, forward_distance) || !workspace ||
        !Metric::operands_ok(n, A, B, workspace))
        return (int)hipErrorInvalidValue;
    ClaimTables<T> c;
    ScanTables<T> s;
    c.fill(n, A, d_nA, B, d_nB, matches, result, forward_distance);
    s.fill(n, A, d_nA, B, result);
    const int blocks = nm_divup(capA, TB);
    hipLaunchKernelGGL(claims, dim3(blocks, n), dim3(TB), 0, nm_stream(stream), c, capA, capB, workspace);
    NM_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan, dim3(blocks, SPLIT, n), dim3(TB), 0, nm_stream(stream), s, capA, workspace);
    NM_LAUNCH_CHECK();
    return nmp::launch_pair_count(n, result, capA, count, nm_stream(stream));
}

// The host entry of a filter: the same checks, then the filter's per-pair twin, pair by pair.
template <class T, class Pair>
int host_mutual(Pair pair, int n, const T *const *A, const int *const *nA, int capA, const T *const *B, const int *const *nB,
                int capB, const int *const *matches, int *const *result, int *count, float *const *forward_distance)
{
    if (!args_ok(n, A, nA, capA, B, nB, capB, matches, result, count, forward_distance)) return (int)hipErrorInvalidValue;
    for (int k = 0; k < n; ++k)
        pair(A[k], clip(*nA[k], capA), capA, B[k], clip(*nB[k], capB), matches[k], result[k], count + k,
             forward_distance ? forward_distance[k] : nullptr);
    return 0;
}

}  // namespace nmc
