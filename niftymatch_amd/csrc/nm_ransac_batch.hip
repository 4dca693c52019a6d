// nm_ransac_batch.hip -- batched RANSAC of up to NM_RANSAC_MAX_BATCH frame pairs with device-side sampling, for gfx950
// (no reference counterpart: the reference fits one pair per call and draws the samples on the host, ransac.cu:523-694).
// Three launches per call whatever n is, all on the caller's stream, no allocation, no synchronisation:
//   1. prep      (grid n): reads the pair's DEVICE size, gathers the valid rows of align_points' semantics (matched and
//                src_x >= 0, ascending) into contiguous float4 (sx, sy, dx, dy) by ordered ballot compaction, writes m_k
//                and resets the pair's selection key;
//   2. fit+count (grid ceil(iterations / 256) x n): ONE LANE PER HYPOTHESIS draws its sample with the stateless
//                counter-based sampler below, fits in registers (nm_ransac_math.hpp, unchanged), then the workgroup
//                streams the pair's compacted points through LDS; every lane tests every point (broadcast reads, no
//                cross-lane reduction). The workgroup's first maximum goes to ONE 64-bit atomicMax on
//                (count << 32) | (0xFFFFFFFF - t): order-independent, and the largest key is the first maximum;
//   3. finalize  (grid n): decodes the key, copies the winning hypothesis.
// Fit and inlier test are the operation sequences of nm_ransac_f32, so results equal that entry (and the oracle) bit for
// bit when it is given the same sample list.
#include <cmath>

#include "nm_common.hpp"
#include "nm_pair_batch.hpp"
#include "nm_ransac_math.hpp"
#include "../../include/nm_abi.h"

namespace {

constexpr int RB_PREP_THREADS = 1024;
constexpr int RB_FIT_THREADS = 256;        // hypotheses per workgroup
constexpr int RB_TILE = 1024;              // float4 points per LDS tile (16 KB)

struct RbHeader {                          // per pair, at the front of the workspace
    unsigned long long key;
    int m;
    int pad;
};

// SplitMix64 (Steele, Lea, Flood 2014) on the counter (seed << 32 | index), then Lemire's multiply-shift reduction to
// [0, m). Fully specified so that a client (or numpy) reproduces every draw.
__host__ __device__ __forceinline__ unsigned int rb_sample(unsigned int seed, unsigned int index, unsigned int m)
{
    unsigned long long z = (((unsigned long long)seed << 32) | index) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (unsigned int)(((z >> 32) * (unsigned long long)m) >> 32);
}

constexpr int rb_min_points(int model) { return model == 2 ? 4 : 2; }     // ransac_impl's minima

struct RbLayout {
    size_t hdr, pts, hyp, total;
};

inline size_t rb_align(size_t b) { return (b + 255) & ~(size_t)255; }

inline RbLayout rb_layout(int n, int capA, int iterations)
{
    RbLayout L;
    L.hdr = 0;
    L.pts = rb_align((size_t)n * sizeof(RbHeader));
    L.hyp = L.pts + rb_align((size_t)n * capA * sizeof(float4));
    L.total = L.hyp + rb_align((size_t)n * iterations * 9 * sizeof(float));
    return L;
}

static_assert(sizeof(nmp::PointTables) + 64 < 4096, "prep kernel arguments exceed 4 KB");

__global__ __launch_bounds__(RB_PREP_THREADS) void ransac_batch_prep_kernel(const nmp::PointTables a, int capA,
                                                                            RbHeader *__restrict__ hdr,
                                                                            float4 *__restrict__ pts)
{
    __shared__ int s_cnt[RB_PREP_THREADS / 64];
    const int k = blockIdx.x, tid = threadIdx.x;
    const int nA = nmp::clip(*a.d_nA[k], capA);
    const float *__restrict__ sx = a.sx[k];
    const float *__restrict__ sy = a.sy[k];
    const float *__restrict__ dx = a.dx[k];
    const float *__restrict__ dy = a.dy[k];
    const int *__restrict__ mt = a.matches[k];
    float4 *__restrict__ out = pts + (size_t)k * capA;
    int base = 0;
    for (int i0 = 0; i0 < nA; i0 += RB_PREP_THREADS) {
        const int i = i0 + tid;
        bool valid = false;
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < nA) {
            const int j = mt[i];
            const float x = sx[i];
            if (j >= 0 && x >= 0.f) {
                valid = true;
                p = make_float4(x, sy[i], dx[j], dy[j]);
            }
        }
        int total;
        const int rank = nmw::block_rank<RB_PREP_THREADS / 64>(valid, s_cnt, total);
        if (valid) out[base + rank] = p;
        base += total;
        __syncthreads();                                   // s_cnt is rewritten by the next chunk
    }
    if (tid == 0) {
        hdr[k].m = base;
        hdr[k].key = 0ull;
    }
}

struct RbSeeds {
    unsigned int seed[NM_RANSAC_MAX_BATCH];
};

template <int MODEL>
__global__ __launch_bounds__(RB_FIT_THREADS) void ransac_batch_fit_count_kernel(const RbSeeds seeds, int capA,
                                                                                int iterations, float thr,
                                                                                RbHeader *__restrict__ hdr,
                                                                                const float4 *__restrict__ pts,
                                                                                float *__restrict__ hyp,
                                                                                float *__restrict__ homographies,
                                                                                int *__restrict__ inliers)
{
    constexpr int NS = nmr_samples(MODEL);
    __shared__ float4 s_pts[RB_TILE];
    __shared__ unsigned long long s_key[RB_FIT_THREADS / 64];
    const int k = blockIdx.y, tid = threadIdx.x;
    const int t = blockIdx.x * RB_FIT_THREADS + tid;
    const bool active = t < iterations;
    const int m = hdr[k].m;
    const size_t row = (size_t)k * iterations + t;
    if (m < rb_min_points(MODEL)) {                        // uniform over the workgroup: no fit, zero optional rows
        if (active) {
            if (homographies)
#pragma unroll
                for (int q = 0; q < 9; ++q) homographies[row * 9 + q] = 0.f;
            if (inliers) inliers[row] = 0;
        }
        return;
    }
    const float4 *__restrict__ P = pts + (size_t)k * capA;
    float H[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) H[q] = 0.f;
    bool dup = false;
    if (active) {
        int ri[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) ri[s] = (int)rb_sample(seeds.seed[k], (unsigned int)(t * NS + s), (unsigned int)m);
        dup = nmr_fit_sampled<MODEL>(ri, [&](int i) { return P[i]; }, H);
#pragma unroll
        for (int q = 0; q < 9; ++q) hyp[row * 9 + q] = H[q];
        if (homographies)
#pragma unroll
            for (int q = 0; q < 9; ++q) homographies[row * 9 + q] = H[q];
    }
    const bool counting = active && !dup;                  // a repeated index counts 0, as nm_ransac_f32
    int cnt = 0;
    for (int p0 = 0; p0 < m; p0 += RB_TILE) {
        const int len = min(RB_TILE, m - p0);
        for (int q = tid; q < len; q += RB_FIT_THREADS) s_pts[q] = P[p0 + q];
        __syncthreads();
        if (counting) {
#pragma unroll 4
            for (int q = 0; q < len; ++q) {
                const float4 v = s_pts[q];
                cnt += nmr_is_inlier(H, v.x, v.y, v.z, v.w, thr) ? 1 : 0;
            }
        }
        __syncthreads();
    }
    if (active && inliers) inliers[row] = cnt;
    unsigned long long key = active ? (((unsigned long long)cnt << 32) | (0xFFFFFFFFu - (unsigned int)t)) : 0ull;
    key = nmw::wave_max(key);
    if ((tid & 63) == 0) s_key[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
        unsigned long long best = s_key[0];
#pragma unroll
        for (int w = 1; w < RB_FIT_THREADS / 64; ++w) best = s_key[w] > best ? s_key[w] : best;
        atomicMax(&hdr[k].key, best);
    }
}

__global__ __launch_bounds__(64) void ransac_batch_finalize_kernel(int model, int iterations,
                                                                   const RbHeader *__restrict__ hdr,
                                                                   const float *__restrict__ hyp,
                                                                   float *__restrict__ H_best, int *__restrict__ best_inliers,
                                                                   int *__restrict__ position, int *__restrict__ status)
{
    const int k = blockIdx.x, tid = threadIdx.x;
    if (hdr[k].m < rb_min_points(model)) {                // too few valid rows: no hypothesis was fitted
        if (tid < 9) H_best[k * 9 + tid] = 0.f;
        if (tid == 0) { best_inliers[k] = 0; position[k] = -1; status[k] = 0; }
        return;
    }
    const unsigned long long key = hdr[k].key;         // >= 1 atomicMax landed: hypothesis 0 always exists
    const int t = (int)(0xFFFFFFFFu - (unsigned int)key);
    if (tid < 9) H_best[k * 9 + tid] = hyp[((size_t)k * iterations + t) * 9 + tid];
    if (tid == 0) { best_inliers[k] = (int)(key >> 32); position[k] = t; status[k] = 1; }
}

}  // namespace

extern "C" size_t nm_ransac_batch_dev_workspace_bytes(int n, int capA, int iterations)
{
    if (!nmp::range_ok(n, capA) || iterations < 1 || iterations > NM_RANSAC_MAX_ITERATIONS) return 0;
    return rb_layout(n, capA, iterations).total;
}

extern "C" int nm_ransac_batch_sample(unsigned int seed, int hypothesis, int sample, int samples, int m)
{
    if (!(samples == 1 || samples == 2 || samples == 4) || hypothesis < 0 || hypothesis >= NM_RANSAC_MAX_ITERATIONS ||
        sample < 0 || sample >= samples || m < 1)
        return -1;
    return (int)rb_sample(seed, (unsigned int)(hypothesis * samples + sample), (unsigned int)m);
}

extern "C" int nm_ransac_batch_dev_f32(int model, int n, const float *const *src_x, const float *const *src_y,
                                       const int *const *d_nA, int capA, const float *const *dst_x,
                                       const float *const *dst_y, const int *const *matches, int iterations,
                                       float inlier_threshold, const unsigned int *seeds, float *H_best,
                                       int *best_inliers, int *position, int *status, float *homographies,
                                       int *inliers, void *workspace, void *stream)
{
    if (model < 0 || model > 2 || iterations < 1 || iterations > NM_RANSAC_MAX_ITERATIONS || !std::isfinite(inlier_threshold))
        return (int)hipErrorInvalidValue;
    if (!nmp::range_ok(n, capA) ||
        !nmp::tables_ok(n, {src_x, src_y, d_nA, dst_x, dst_y, matches}, {},
                        {seeds, H_best, best_inliers, position, status, workspace}))
        return (int)hipErrorInvalidValue;
    nmp::PointTables a;
    a.fill(n, src_x, src_y, dst_x, dst_y, matches, d_nA);
    RbSeeds sd;
    for (int k = 0; k < nmp::MAX_BATCH; ++k) sd.seed[k] = k < n ? seeds[k] : 0;
    const RbLayout L = rb_layout(n, capA, iterations);
    char *ws = static_cast<char *>(workspace);
    RbHeader *hdr = reinterpret_cast<RbHeader *>(ws + L.hdr);
    float4 *pts = reinterpret_cast<float4 *>(ws + L.pts);
    float *hyp = reinterpret_cast<float *>(ws + L.hyp);
    hipStream_t st = nm_stream(stream);
    hipLaunchKernelGGL(ransac_batch_prep_kernel, dim3(n), dim3(RB_PREP_THREADS), 0, st, a, capA, hdr, pts);
    NM_LAUNCH_CHECK();
    const dim3 grid(nm_divup(iterations, RB_FIT_THREADS), n);
    if (model == 0)
        hipLaunchKernelGGL(ransac_batch_fit_count_kernel<0>, grid, dim3(RB_FIT_THREADS), 0, st, sd, capA, iterations,
                           inlier_threshold, hdr, pts, hyp, homographies, inliers);
    else if (model == 1)
        hipLaunchKernelGGL(ransac_batch_fit_count_kernel<1>, grid, dim3(RB_FIT_THREADS), 0, st, sd, capA, iterations,
                           inlier_threshold, hdr, pts, hyp, homographies, inliers);
    else
        hipLaunchKernelGGL(ransac_batch_fit_count_kernel<2>, grid, dim3(RB_FIT_THREADS), 0, st, sd, capA, iterations,
                           inlier_threshold, hdr, pts, hyp, homographies, inliers);
    NM_LAUNCH_CHECK();
    hipLaunchKernelGGL(ransac_batch_finalize_kernel, dim3(n), dim3(64), 0, st, model, iterations, hdr, hyp, H_best,
                       best_inliers, position, status);
    NM_LAUNCH_CHECK();
    return 0;
}
