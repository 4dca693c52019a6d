// nm_ingest.hip -- batched frame ingest for gfx950: up to NM_INGEST_MAX_BATCH BGRA frames of one camera undistorted
// through one shared map (resample_2D<uchar4>, kernels/resample.cu) and turned into the fp32 gray planes SIFT reads
// (cuda_grayscale, kernels/bgra_2_gray.cu), in ONE launch. No reference counterpart: the reference's client undistorts
// and converts each frame with its own launches.
//   One lane per output pixel p (grid x), frames split over grid y only when the geometry is small. The map and the
// sampler's per-pixel work are per pixel, not per frame: a lane loads (u, v) once, runs tex_setup (border test, 1/256
// weights) and the tap addressing once (nm_warp_math.hpp), then walks its frames IG_UNROLL at a time: the
// 4 x IG_UNROLL uchar4 taps are issued before any of them is used (gathers that hit L2: neighbouring lanes touch
// neighbouring texels), then each frame's filter, uchar4 rounding and gray (nm_gray.hpp) run from registers and write
// one uchar4 and one float. Per call the map is read once, each frame's texels about once, each output written once.
#include "nm_gray.hpp"
#include "nm_pair_batch.hpp"
#include "nm_warp_math.hpp"

namespace {

using namespace nmw;
using nmg::gray_of;

constexpr int IG_THREADS = 256;
constexpr int IG_UNROLL = 4;                    // frames whose taps are in flight together
constexpr int IG_FILL_BLOCKS_PER_CU = 8;        // below this many pixel workgroups per CU, frames split over grid y

struct IgArgs {                                 // 3 x 64 pointers: 1.5 KB of the 4 KB of kernel arguments
    const uchar4 *frames[NM_INGEST_MAX_BATCH];
    float *gray[NM_INGEST_MAX_BATCH];
    uchar4 *undistorted[NM_INGEST_MAX_BATCH];
};
static_assert(sizeof(IgArgs) + 64 < 4096, "ingest kernel arguments exceed 4 KB");

// MAP: sample through (map_x, map_y); else the identity (gray of the frame itself). UNDIST: write the uchar4 result.
template <bool MAP, bool UNDIST>
__global__ __launch_bounds__(IG_THREADS) void frame_ingest_kernel(const IgArgs a, int n, int per_group, size_t P,
                                                                  int fw, int fh, const float *__restrict__ map_x,
                                                                  const float *__restrict__ map_y)
{
    const size_t p = (size_t)blockIdx.x * IG_THREADS + threadIdx.x;
    if (p >= P) return;
    const int k0 = blockIdx.y * per_group;
    const int k1 = k0 + per_group < n ? k0 + per_group : n;
    if (!MAP) {
        for (int k = k0; k < k1; k += IG_UNROLL) {
            uchar4 px[IG_UNROLL];
#pragma unroll
            for (int f = 0; f < IG_UNROLL; ++f)
                if (k + f < k1) px[f] = a.frames[k + f][p];
#pragma unroll
            for (int f = 0; f < IG_UNROLL; ++f)
                if (k + f < k1) a.gray[k + f][p] = gray_of(px[f]);
        }
        return;
    }
    const Tex t{nullptr, fw, fh, NM_TEX_U8X4N};
    int i, j;
    float w[4];
    if (!tex_setup(t, map_x[p] + 0.5f, map_y[p] + 0.5f, i, j, w)) {
        // outside the sampler's support: every tap out of frame and zero weights give the +0 samples tex2d_u8x4 returns
        i = j = -2;
        w[0] = w[1] = w[2] = w[3] = 0.f;
    }
    size_t off[4];
    bool in[4];
    tex_taps_u8x4(t, i, j, off, in);
    for (int k = k0; k < k1; k += IG_UNROLL) {
        uchar4 px[IG_UNROLL][4];
#pragma unroll
        for (int f = 0; f < IG_UNROLL; ++f)
            if (k + f < k1) tex_fetch_u8x4(a.frames[k + f], off, in, px[f]);
#pragma unroll
        for (int f = 0; f < IG_UNROLL; ++f) {
            if (k + f >= k1) continue;
            float s[4];
            tex_filter_u8x4(px[f], w, s);
            const uchar4 r = u8x4_of(s);
            if (UNDIST) a.undistorted[k + f][p] = r;
            a.gray[k + f][p] = gray_of(r);
        }
    }
}

template <bool MAP, bool UNDIST>
void launch(const IgArgs &a, int n, int cols, int rows, int fw, int fh, const float *map_x, const float *map_y,
            hipStream_t st)
{
    const size_t P = (size_t)cols * rows;
    const size_t blocks = (P + IG_THREADS - 1) / IG_THREADS;
    // Split the frames over grid y only while the pixel grid alone cannot fill the chip; a group keeps whole unrolled
    // steps. The split changes which lane computes a frame's pixel, never what it computes.
    const size_t fill = (size_t)nm_cu_count() * IG_FILL_BLOCKS_PER_CU;
    const int max_groups = (n + IG_UNROLL - 1) / IG_UNROLL;
    int groups = blocks >= fill ? 1 : (int)((fill + blocks - 1) / blocks);
    groups = groups < max_groups ? groups : max_groups;
    int per_group = (n + groups - 1) / groups;
    per_group = (per_group + IG_UNROLL - 1) / IG_UNROLL * IG_UNROLL;
    groups = (n + per_group - 1) / per_group;
    hipLaunchKernelGGL((frame_ingest_kernel<MAP, UNDIST>), dim3((unsigned)blocks, groups), dim3(IG_THREADS), 0, st, a,
                       n, per_group, P, fw, fh, map_x, map_y);
}

}  // namespace

extern "C" {

int nm_frame_ingest_batch_f32(int n, const unsigned char *const *frames, int fw, int fh, const float *map_x,
                              const float *map_y, int cols, int rows, float *const *gray,
                              unsigned char *const *undistorted, void *stream)
{
    if (n < 1 || n > NM_INGEST_MAX_BATCH || !nm_size_ok(fw) || !nm_size_ok(fh) || !nm_size_ok(cols) || !nm_size_ok(rows))
        return (int)hipErrorInvalidValue;
    if (!nmp::tables_ok(n, {frames, gray}, {undistorted}, {}) || (!map_x) != (!map_y)) return (int)hipErrorInvalidValue;
    const bool map = map_x != nullptr;
    if (!map && (undistorted || cols != fw || rows != fh)) return (int)hipErrorInvalidValue;
    IgArgs a;
    nmp::fill_slots_as(a.frames, frames, 0, n); nmp::fill_slots(a.gray, gray, 0, n);
    nmp::fill_slots_as(a.undistorted, undistorted, 0, n);
    const hipStream_t st = nm_stream(stream);
    if (!map) launch<false, false>(a, n, cols, rows, fw, fh, nullptr, nullptr, st);
    else if (undistorted) launch<true, true>(a, n, cols, rows, fw, fh, map_x, map_y, st);
    else launch<true, false>(a, n, cols, rows, fw, fh, map_x, map_y, st);
    NM_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
