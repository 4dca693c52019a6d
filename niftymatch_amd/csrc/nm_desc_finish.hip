// nm_desc_finish.hip -- batched descriptor finish for gfx950 (no reference counterpart: the reference's descriptors leave
// kernels/descriptor.cu raw, its normalize_histogram is never called). One launch for 1..64 frames, the frame
// a grid dimension: a wave takes one row of 128 floats, lane l elements (2 l, 2 l + 1) (one 512-byte coalesced read), runs
// nmdf::finish (nm_desc_finish_math.hpp) and writes the fp32 row (8 bytes per lane) and / or the u8 row (2 bytes per lane).
// The row count is the device int the frame driver wrote, clipped to the capacity; rows at or beyond it are not touched.
// No LDS, no atomics, no allocation, no synchronisation. Bandwidth-bound: 512 B in, 128 .. 640 B out per row.
#include "nm_common.hpp"
#include "nm_desc_finish_math.hpp"
#include "nm_pair_batch.hpp"
#include "../../include/nm_abi.h"

namespace {

constexpr int TB = 256;                     // four waves = four rows per workgroup
constexpr int ROWS = TB / 64;

struct FinishArgs {                         // 4 x 64 pointers: 2 KB of kernel arguments
    const float *desc[NM_DESC_FINISH_MAX_BATCH];
    const int *d_num[NM_DESC_FINISH_MAX_BATCH];
    float *out_f32[NM_DESC_FINISH_MAX_BATCH];
    unsigned char *out_u8[NM_DESC_FINISH_MAX_BATCH];
};
static_assert(sizeof(FinishArgs) + 64 < 4096, "finish kernel arguments exceed 4 KB");

struct __attribute__((aligned(2))) U8x2 { unsigned char v[2]; };

__global__ __launch_bounds__(TB) void desc_finish_kernel(const FinishArgs a, int capacity, int mode)
{
    const int k = blockIdx.y, lane = threadIdx.x & 63;
    const int row = blockIdx.x * ROWS + (threadIdx.x >> 6);
    const int count = nmp::clip(*a.d_num[k], capacity);
    if (row >= count) return;                                        // uniform over the wave
    const size_t at = (size_t)row * nmdf::DIM + 2 * lane;
    const float2 v = *reinterpret_cast<const float2 *>(a.desc[k] + at);   // read before any write: out_f32 may be desc
    nmdf::LaneRow r;
    r.a[0] = v.x; r.b[0] = v.y;
    const bool ok = nmdf::finish(r, mode);                           // uniform: every lane holds the same sums
    const float x = ok ? r.a[0] : 0.0f, y = ok ? r.b[0] : 0.0f;
    if (a.out_f32[k]) *reinterpret_cast<float2 *>(a.out_f32[k] + at) = make_float2(x, y);
    if (a.out_u8[k]) {
        U8x2 q;
        q.v[0] = nmdf::quantise(x); q.v[1] = nmdf::quantise(y);
        *reinterpret_cast<U8x2 *>(a.out_u8[k] + at) = q;
    }
}

bool finish_args_ok(int n, const float *const *desc, const int *const *num, int capacity, float *const *out_f32,
                    unsigned char *const *out_u8, int mode)
{
    if (!nmp::range_ok(n, capacity) || (mode != NM_DESC_L2 && mode != NM_DESC_ROOT)) return false;
    if (!out_f32 && !out_u8) return false;
    return nmp::tables_ok(n, {desc, num}, {out_f32, out_u8}, {});
}

}  // namespace

extern "C" int nm_sift_desc_finish_batch_dev(int n, const float *const *desc, const int *const *d_num_items, int capacity,
                                             float *const *out_f32, unsigned char *const *out_u8, int mode, void *stream)
{
    if (!finish_args_ok(n, desc, d_num_items, capacity, out_f32, out_u8, mode)) return (int)hipErrorInvalidValue;
    FinishArgs a;
    nmp::fill_slots(a.desc, desc, 0, n); nmp::fill_slots(a.d_num, d_num_items, 0, n);
    nmp::fill_slots(a.out_f32, out_f32, 0, n); nmp::fill_slots(a.out_u8, out_u8, 0, n);
    hipLaunchKernelGGL(desc_finish_kernel, dim3(nm_divup(capacity, ROWS), n), dim3(TB), 0, nm_stream(stream), a, capacity, mode);
    NM_LAUNCH_CHECK();
    return 0;
}

extern "C" int nm_sift_desc_finish_host(int n, const float *const *desc, const int *const *num_items, int capacity,
                                        float *const *out_f32, unsigned char *const *out_u8, int mode)
{
    if (!finish_args_ok(n, desc, num_items, capacity, out_f32, out_u8, mode)) return (int)hipErrorInvalidValue;
    for (int k = 0; k < n; ++k) {
        const int count = nmp::clip(*num_items[k], capacity);
        for (int row = 0; row < count; ++row) {
            const float *src = desc[k] + (size_t)row * nmdf::DIM;
            nmdf::HostRow r;
            for (int l = 0; l < nmdf::PAIRS; ++l) { r.a[l] = src[2 * l]; r.b[l] = src[2 * l + 1]; }
            const bool ok = nmdf::finish(r, mode);
            for (int l = 0; l < nmdf::PAIRS; ++l) {
                const float x = ok ? r.a[l] : 0.0f, y = ok ? r.b[l] : 0.0f;
                const size_t at = (size_t)row * nmdf::DIM + 2 * l;
                if (out_f32) { out_f32[k][at] = x; out_f32[k][at + 1] = y; }
                if (out_u8) { out_u8[k][at] = nmdf::quantise(x); out_u8[k][at + 1] = nmdf::quantise(y); }
            }
        }
    }
    return 0;
}
