// nm_pair_batch.hip -- the kernels the batched stages share (nm_pair_batch.hpp): the counts of guided and mutual matching, and
// the zeroing of the 64-bit sums and counts that median, frame weights and exposure sums add into.
#include "nm_common.hpp"
#include "nm_pair_batch.hpp"

namespace {

constexpr int TB = 256;

struct CtArgs {
    const int *result[nmp::MAX_BATCH];
};

// count[k] = entries >= 0 among the capA results of pair k: integer sums, one workgroup per pair
__global__ __launch_bounds__(TB) void pair_count_kernel(const CtArgs a, int capA, int *__restrict__ count)
{
    __shared__ int part[TB / 64];
    const int k = blockIdx.x, tid = threadIdx.x;
    const int *__restrict__ res = a.result[k];
    int c = 0;
    for (int i = tid; i < capA; i += TB) c += res[i] >= 0 ? 1 : 0;
    c = nmw::wave_sum(c);
    if ((tid & 63) == 0) part[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int w = 0; w < TB / 64; ++w) t += part[w];
        count[k] = t;
    }
}

// one workgroup, a stride loop: the callers zero at most a few thousand words
__global__ __launch_bounds__(TB) void zero_u64_kernel(unsigned long long *__restrict__ p, size_t words)
{
    for (size_t i = threadIdx.x; i < words; i += TB) p[i] = 0;
}

}  // namespace

int nmp::launch_pair_count(int n, int *const *result, int capA, int *count, hipStream_t stream)
{
    CtArgs c;
    fill_slots(c.result, result, 0, n);
    hipLaunchKernelGGL(pair_count_kernel, dim3(n), dim3(TB), 0, stream, c, capA, count);
    NM_LAUNCH_CHECK();
    return 0;
}

hipError_t nmp::launch_zero_u64(unsigned long long *p, size_t words, hipStream_t stream)
{
    hipLaunchKernelGGL(zero_u64_kernel, dim3(1), dim3(TB), 0, stream, p, words);
    return hipGetLastError();
}
