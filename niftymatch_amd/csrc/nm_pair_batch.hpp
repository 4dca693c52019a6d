// nm_pair_batch.hpp -- the convention of the per-pair stages behind the blind matcher (nm_ransac_batch.hip,
// nm_ransac_refit.hip, nm_match_guided.hip, nm_match_mutual.hip, nm_match_mutual_u8.hip), stated once. A call takes n <= MAX_BATCH pairs. A pair is
// a row of host tables of device pointers; the tables travel to the kernels as [MAX_BATCH] pointer arrays inside the kernel
// arguments, unused slots null. Sizes are device ints clipped to a capacity below CAP_LIMIT. A bad argument is refused
// with hipErrorInvalidValue before anything is launched and before any device pointer is dereferenced; a host twin runs
// the same check. What is particular to a stage (model, iterations, rounds, finite thresholds) stays with the stage.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <initializer_list>

#include "../../include/nm_abi.h"

namespace nmp {

constexpr int MAX_BATCH = 64;               // pairs per call
constexpr int CAP_LIMIT = 1 << 22;          // capacities (rows per pair) lie in [1, CAP_LIMIT)
static_assert(NM_RANSAC_MAX_BATCH == MAX_BATCH && NM_MATCH_GUIDED_MAX_BATCH == MAX_BATCH &&
              NM_MATCH_MUTUAL_MAX_BATCH == MAX_BATCH && NM_MATCH_MUTUAL_U8_MAX_BATCH == MAX_BATCH &&
              NM_MATCH_U8_MAX_BATCH == MAX_BATCH && NM_DESC_FINISH_MAX_BATCH == MAX_BATCH &&
              NM_SELECT_MAX_BATCH == MAX_BATCH && NM_MATCH_KNN_U8_MAX_BATCH == MAX_BATCH,
              "public header and pair-batch convention disagree");

/* A device size as the kernels (and the host twins) use it */
__host__ __device__ __forceinline__ int clip(int v, int cap) { return v < 0 ? 0 : (v > cap ? cap : v); }

/* The two predicates of the mutual filters (fp32 and u8, device and host twins). Row i claims column j = matches[i]: any
 * value outside [0, nB) is no claim. Rival row ip at distance d takes the column from row i at distance tau: strictly
 * nearer, or as near and earlier in the scan. A claim is kept exactly when no row of A beats it. */
__host__ __device__ __forceinline__ bool is_claim(int j, int nB) { return j >= 0 && j < nB; }
template <class D> __host__ __device__ __forceinline__ bool beats(D d, int ip, D tau, int i)
{
    return d < tau || (d == tau && ip < i);
}

__host__ __device__ __forceinline__ bool finite9(const float H[9])
{
    bool ok = true;
    for (int q = 0; q < 9; ++q) ok = ok && __builtin_isfinite(H[q]);
    return ok;
}

inline bool cap_ok(int cap) { return cap >= 1 && cap < CAP_LIMIT; }
inline bool range_ok(int n, int capA) { return n >= 1 && n <= MAX_BATCH && cap_ok(capA); }

// A host table of pointers of any type, looked at only for null slots (memcpy: no pointer type is punned).
struct Table {
    const void *base;
    template <class T> Table(T *const *t) : base(t) {}
    bool slot_set(int k) const
    {
        const void *p;
        std::memcpy(&p, static_cast<const char *>(base) + (size_t)k * sizeof p, sizeof p);
        return p != nullptr;
    }
    bool slots_set(int n) const
    {
        for (int k = 0; k < n; ++k)
            if (!slot_set(k)) return false;
        return true;
    }
};

// Required tables: present, every used slot set. Optional tables: absent, or every used slot set. Plain pointers: set.
// Reads host memory only; call it after range_ok.
inline bool tables_ok(int n, std::initializer_list<Table> required, std::initializer_list<Table> optional,
                      std::initializer_list<const void *> pointers)
{
    for (const void *p : pointers)
        if (!p) return false;
    for (const Table &t : required)
        if (!t.base || !t.slots_set(n)) return false;
    for (const Table &t : optional)
        if (t.base && !t.slots_set(n)) return false;
    return true;
}

// dst[s] = src[first + s] for the pairs first + s < n, null for the rest (and for all of an absent optional table)
template <int N, class D, class S> inline void fill_slots(D *(&dst)[N], S *const *src, int first, int n)
{
    for (int s = 0; s < N; ++s) dst[s] = (src && first + s < n) ? src[first + s] : nullptr;
}

// fill_slots for a table the kernel reads through another pointer type (BGRA bytes as uchar4)
template <int N, class D, class S> inline void fill_slots_as(D *(&dst)[N], S *const *src, int first, int n)
{
    for (int s = 0; s < N; ++s) dst[s] = (src && first + s < n) ? reinterpret_cast<D *>(src[first + s]) : nullptr;
}

struct PointTables {                        // the point pairs of RANSAC and refit: 6 x 64 pointers, 3 KB of kernel arguments
    const float *sx[MAX_BATCH];
    const float *sy[MAX_BATCH];
    const float *dx[MAX_BATCH];
    const float *dy[MAX_BATCH];
    const int *matches[MAX_BATCH];
    const int *d_nA[MAX_BATCH];
    void fill(int n, const float *const *src_x, const float *const *src_y, const float *const *dst_x,
              const float *const *dst_y, const int *const *mt, const int *const *nA)
    {
        fill_slots(sx, src_x, 0, n); fill_slots(sy, src_y, 0, n); fill_slots(dx, dst_x, 0, n); fill_slots(dy, dst_y, 0, n);
        fill_slots(matches, mt, 0, n); fill_slots(d_nA, nA, 0, n);
    }
};

// count[k] = entries >= 0 among the capA results of pair k, k < n (nm_pair_batch.hip): one launch, grid n, on `stream`
int launch_pair_count(int n, int *const *result, int capA, int *count, hipStream_t stream);

// p[0 .. words) = 0 (nm_pair_batch.hip): one launch of one workgroup on `stream`. A kernel and not hipMemsetAsync: a captured
// memset node replayed correctly once and left other values from the second replay on ("Median composite")
hipError_t launch_zero_u64(unsigned long long *p, size_t words, hipStream_t stream);

}  // namespace nmp
