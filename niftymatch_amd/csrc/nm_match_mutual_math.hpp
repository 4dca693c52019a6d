// nm_match_mutual_math.hpp -- mutual-nearest-neighbour filtering of a match list (nm_sift_match_mutual_batch_dev_f32 and its
// host twin), for gfx950. No reference counterpart: the reference's matcher (kernels/match.cu) tests one direction only; a
// client that wants a cross-check calls it a second time with the sets swapped. Everything here is __host__ __device__ and
// is the ONLY arithmetic of both entries, so host and device agree bit for bit: the claim test and the verdict (nm_pair_batch.hpp), the 128-D distance of
// nm_bf_distance_f32 (acc = fma(t, t, acc), t = a_q - b_q, q ascending) cut into chunks of NMM_CHUNK dimensions with the
// test that abandons a rival row, and the keep rule. The chain never decreases (t * t >= 0, rounding is monotone, a NaN stays
// a NaN), so a rival whose partial sum is no longer <= tau cannot end below or at tau: abandoning it changes no result.
// All fp32, fma explicit (-ffp-contract=off). tau itself is nmg::distance128 (nm_match_guided_math.hpp), the same chain.
#pragma once
#include <hip/hip_runtime.h>

#include "nm_match_guided_math.hpp"
#include "nm_pair_batch.hpp"

namespace nmm {

constexpr int NMM_CHUNK = 16;                       // dimensions between two looks at the partial sum
constexpr int NMM_CHUNKS = 128 / NMM_CHUNK;

using nmp::beats;                                   // the verdict on a rival that ran to the end
using nmp::clip;
using nmp::is_claim;

/* The next NMM_CHUNK links of the chain: a and b point at dimension q0 of the rival row and of the claimed column */
__host__ __device__ __forceinline__ float chunk(float acc, const float *a, const float *b)
{
#pragma unroll
    for (int q = 0; q < NMM_CHUNK; ++q) {
        const float t = a[q] - b[q];
        acc = __builtin_fmaf(t, t, acc);
    }
    return acc;
}

/* A rival with this partial sum can still beat or tie tau. False for a NaN on either side: NaN rivals and NaN claims drop out. */
__host__ __device__ __forceinline__ bool alive(float acc, float tau) { return acc <= tau; }

/* The keep rule: tau is a number and no rival beat it */
__host__ __device__ __forceinline__ bool keep(float tau, bool beaten) { return tau == tau && !beaten; }

/* One rival against one claim, serially: the early exit and the verdict. `walked` counts chunks (statistics only). */
__host__ __device__ __forceinline__ bool rival_beats(const float *a, const float *b, int ip, float tau, int i, int *walked)
{
    float acc = 0.f;
    for (int c = 0; c < NMM_CHUNKS; ++c) {
        acc = chunk(acc, a + c * NMM_CHUNK, b + c * NMM_CHUNK);
        if (walked) ++*walked;
        if (!alive(acc, tau)) return false;
    }
    return beats(acc, ip, tau, i);
}

}  // namespace nmm
