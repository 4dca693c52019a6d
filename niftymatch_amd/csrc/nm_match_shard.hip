// nm_match_shard.hip -- candidate shards over several GPUs: the neutral triple, the merges and the RCCL all-gather entry.
#include <dlfcn.h>

#include "nm_match_select.hpp"
#include "../../include/nm_abi.h"

namespace nm_match {
namespace {

// Multi-GPU merge: shard-major triples, ascending shard order, strict < so the lowest global index wins ties.
__global__ __launch_bounds__(256) void match_merge_kernel(const float *__restrict__ min1, const int *__restrict__ idx1,
                                                         const float *__restrict__ min2, int n_shards, int nA,
                                                         float ambiguity, int *__restrict__ result)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nA) return;
    float m1 = __builtin_inff(), m2 = __builtin_inff(); int idx = -1;             // the neutral (empty shard) triple
    for (int g = 0; g < n_shards; ++g) {
        const float a1 = min1[(size_t)g * nA + i], a2 = min2[(size_t)g * nA + i];
        const int ai = idx1[(size_t)g * nA + i];
        // a NaN minimum can only come from the shard holding global candidate 0 (every shard before it is empty): it is
        // the scan's min_1_distance for good (match.cu:90,96)
        if (a1 != a1) { m1 = a1; idx = 0; m2 = a2; }
        else if (a1 < m1) { m2 = (m1 < a2) ? m1 : a2; m1 = a1; idx = ai; }
        else if (a1 < m2) m2 = a1;
    }
    emit_match(i, m1, idx, m2, 0, ambiguity, result, nullptr, nullptr, nullptr);     // clamps iff the minimum sits at 0
}

// An empty candidate shard (world > nB, or uneven tiny sets): the neutral triple, so that the merge ignores the shard.
__global__ __launch_bounds__(256) void shard_neutral_kernel(float *__restrict__ min1, int *__restrict__ idx1,
                                                           float *__restrict__ min2, int nA)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nA) return;
    min1[i] = __builtin_inff(); idx1[i] = -1; min2[i] = __builtin_inff();
}

// The same merge on the buffer an all-gather of per-rank (min1[nA], idx1[nA], min2[nA]) blocks produces: element c of row i
// of rank g sits at packed[(g * 3 + c) * nA + i].
__global__ __launch_bounds__(256) void match_merge_packed_kernel(const int *__restrict__ packed, int n_shards, int nA,
                                                                float ambiguity, int *__restrict__ result)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nA) return;
    float m1 = __builtin_inff(), m2 = __builtin_inff(); int idx = -1;
    for (int g = 0; g < n_shards; ++g) {
        const int *p = packed + (size_t)g * 3 * nA;
        const float a1 = __int_as_float(p[i]), a2 = __int_as_float(p[2 * (size_t)nA + i]);
        const int ai = p[(size_t)nA + i];
        if (a1 != a1) { m1 = a1; idx = 0; m2 = a2; }
        else if (a1 < m1) { m2 = (m1 < a2) ? m1 : a2; m1 = a1; idx = ai; }
        else if (a1 < m2) m2 = a1;
    }
    emit_match(i, m1, idx, m2, 0, ambiguity, result, nullptr, nullptr, nullptr);
}

}  // namespace

void launch_shard_neutral(float *min1, int *idx1, float *min2, int nA, hipStream_t st)
{
    hipLaunchKernelGGL(shard_neutral_kernel, dim3(nm_divup(nA, 256)), dim3(256), 0, st, min1, idx1, min2, nA);
}

}  // namespace nm_match
using namespace nm_match;

extern "C" {

// ---- native multi-GPU entry: shard -> ONE ncclAllGather of 12 B per row per rank -> merge ----
// RCCL is resolved at run time from the process (the caller created the communicator, so its RCCL is loaded already;
// torch ships its own copy): libnm_hip.so has no link-time dependency on librccl.
typedef int (*NmAllGatherFn)(const void *, void *, size_t, int, void *, hipStream_t);
static NmAllGatherFn nm_resolve_allgather()
{
    static NmAllGatherFn fn = [] {
        void *sym = dlsym(RTLD_DEFAULT, "ncclAllGather");
        if (!sym) {
            void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
            if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
            if (h) sym = dlsym(h, "ncclAllGather");
        }
        return reinterpret_cast<NmAllGatherFn>(sym);
    }();
    return fn;
}

int nm_sift_match_merge_packed_f32(const int *packed, int n_shards, int nA, int *result, float ambiguity, void *stream)
{
    if (nA <= 0 || n_shards <= 0) return 0;
    if (!packed || !result) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(match_merge_packed_kernel, dim3(nm_divup(nA, 256)), dim3(256), 0, nm_stream(stream), packed, n_shards,
                       nA, ambiguity, result);
    NM_LAUNCH_CHECK();
    return 0;
}

size_t nm_sift_match_allgather_workspace_bytes(int nA, int nB_shard, int n_ranks)
{
    if (nA < 0) nA = 0;
    if (n_ranks < 1) n_ranks = 1;
    return pair_workspace_bytes(nA, nB_shard) + align256((size_t)3 * nA * 4) + align256((size_t)n_ranks * 3 * nA * 4);
}

int nm_sift_match_allgather_f32(const float *A, int nA, const float *B_shard, int nB_shard, int index_offset, int n_ranks,
                                int *result, float ambiguity, void *workspace, void *nccl_comm, void *stream)
{
    if (nA <= 0) return 0;
    if (!A || !result || !workspace || n_ranks < 1 || (n_ranks > 1 && !nccl_comm)) return (int)hipErrorInvalidValue;
    hipStream_t st = nm_stream(stream);
    char *base = static_cast<char *>(workspace) + pair_workspace_bytes(nA, nB_shard);
    int *mine = reinterpret_cast<int *>(base);
    int *gathered = reinterpret_cast<int *>(base + align256((size_t)3 * nA * 4));
    int rc = nm_sift_match_shard_f32(A, nA, B_shard, nB_shard, index_offset, reinterpret_cast<float *>(mine), mine + nA,
                                     reinterpret_cast<float *>(mine + 2 * (size_t)nA), workspace, stream);
    if (rc) return rc;
    const int *merged_from = mine;
    if (n_ranks > 1) {
        const NmAllGatherFn allgather = nm_resolve_allgather();
        if (!allgather) return (int)hipErrorNotSupported;                 // no RCCL in this process
        const int nrc = allgather(mine, gathered, (size_t)3 * nA, /* ncclInt32 */ 2, nccl_comm, st);
        if (nrc != 0) return (int)hipErrorUnknown;
        merged_from = gathered;
    }
    return nm_sift_match_merge_packed_f32(merged_from, n_ranks, nA, result, ambiguity, stream);
}

int nm_sift_match_merge_f32(const float *min1, const int *idx1, const float *min2, int n_shards, int nA, int *result,
                            float ambiguity, void *stream)
{
    if (nA <= 0 || n_shards <= 0) return 0;
    hipLaunchKernelGGL(match_merge_kernel, dim3(nm_divup(nA, 256)), dim3(256), 0, nm_stream(stream), min1, idx1, min2,
                       n_shards, nA, ambiguity, result);
    NM_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
