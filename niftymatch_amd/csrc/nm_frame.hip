// nm_frame.hip -- library-level entry points: device helpers, host-side tap generation, and the per-frame driver
// that runs the reference's implied client loop (orchestration order of sift/siftfunctions.cu:42-181)
// as one allocation-free, sync-free launch sequence on a stream.
#include <atomic>
#include <cmath>

#include "nm_arena.hpp"
#include "nm_describe.hpp"
#include "nm_frame_plan.hpp"
#include "nm_keypoint.hpp"

namespace {

__global__ __launch_bounds__(256) void fill_u32_kernel(unsigned int *__restrict__ p, size_t n, unsigned int v)
{
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * 256;
    for (; i < n; i += stride) p[i] = v;
}

}  // namespace

thread_local NmProfSite nm_prof_sites[NM_PROF_SITES] = {};

static_assert(NM_FRAME_TAIL_MAX_FRAMES == NM_TAIL_MAX_FRAMES && NM_FRAME_MAX_OCTAVES == 20, "nm_frame_plan.hpp follows nm_tail.hpp / the arena");

// Issue order of the per-octave path (calls of more frames than the octave tail serves). 0: levels 1-5 of every octave on the
// caller's stream, detection beside the next octave's levels. 1 (skewed): only levels 1-3 -- all that the next octave's level 0
// needs -- stay on the caller's stream; levels 4-5 go to the side stream in front of the octave's detection, so the chain
// reaches the small octaves while the large launches of octaves 0-2 still run. Same launches, same results in either order.
// Order 1 is off: measured, a 64-frame call takes 7 904 us against 7 799 (profiles/r07_a_skew_alternation.txt) -- the side stream
// becomes one serial chain, and the plain order's pairing of octave o's detection with octave o + 1's levels is lost (DESIGN.md
// section 9).
// 2 (cross): order 1 with levels 4-5 on a THIRD stream (the helper set's description stream, idle on this path), which keeps the
// plain order's pairing: per octave o, levels 1-3 of octave o + 1 on the caller's stream, levels 4-5 of octave o on the third,
// detection of octave o - 1 on the side stream.
// The order of a call is nm_frame_resolve's (nm_frame_plan.hpp): what nm_sift_set_frame_skew selected; else NM_FRAME_SKEW where
// the environment names one (read once); else the cross order for calls of at least NM_FRAME_CROSS_MIN_FRAMES frames (a compile-
// time value, NM_FRAME_CROSS_MIN_FRAMES in the environment overrides it, read once; 0 = never) and order 0 below that.
// The three streams of a call are the caller's and the two of the helper set that nm_helper_set_acquire (nm_arena.hip) keeps for
// that caller stream.
// The schedule of every order is nm_frame_plan's (nm_frame_plan.hpp); what the orders rely on -- which stream touches which
// planes and which event orders them -- is checked on that plan by tests/test_frame_plan.py.
static std::atomic<int> g_frame_skew{-1};          // -1: the default

extern "C" {

int nm_sift_set_frame_skew(int mode)
{
    const int prev = g_frame_skew.exchange((mode >= 0 && mode <= 2) ? mode : -1);
    return prev < 0 ? nm_frame_switches().order : prev;
}

const char *nm_version(void) { return "niftymatch_amd 0.1.0 gfx950"; }
int nm_device_count(int *count) { return (int)hipGetDeviceCount(count); }
int nm_set_device(int device) { return (int)hipSetDevice(device); }
const char *nm_error_string(int status) { return hipGetErrorString((hipError_t)status); }

int nm_profile_events(int site, void *start_event, void *stop_event)
{
    if (site < 0 || site >= NM_PROF_SITES) return (int)hipErrorInvalidValue;
    nm_prof_sites[site].start = static_cast<hipEvent_t>(start_event);
    nm_prof_sites[site].stop = static_cast<hipEvent_t>(stop_event);
    nm_prof_sites[site].list = nullptr; nm_prof_sites[site].n = nm_prof_sites[site].next = 0;
    return 0;
}

int nm_profile_event_pairs(int site, void *const *events, int npairs)
{
    if (site < 0 || site >= NM_PROF_SITES || npairs < 0) return (int)hipErrorInvalidValue;
    nm_prof_sites[site].start = nm_prof_sites[site].stop = nullptr;
    nm_prof_sites[site].list = npairs ? events : nullptr;
    nm_prof_sites[site].n = npairs; nm_prof_sites[site].next = 0;
    return 0;
}

int nm_fill_u32(void *dst, size_t count, unsigned int pattern, void *stream)
{
    if (count == 0) return 0;
    size_t blocks = (count + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(fill_u32_kernel, dim3((unsigned)blocks), dim3(256), 0, nm_stream(stream),
                       static_cast<unsigned int *>(dst), count, pattern);
    NM_LAUNCH_CHECK();
    return 0;
}

// sift/pyramidata.cu:105-123: radius = ceil(4 sigma); w_j = (float)exp(-0.5 ((j-r)/sigma)^2) with a double exp on the
// host; normalised by the float running sum.
int nm_create_kernel_for_sigma(float sigma, float *taps)
{
    const int radius = (int)(std::ceil(sigma * 4));
    const int length = 2 * radius + 1;
    float sum = 0.f;
    for (int j = 0; j < length; ++j) {
        float u = ((float)j - radius) / sigma;
        u = (float)std::exp(-0.5 * (u * u));
        if (taps) taps[j] = u;
        sum += u;
    }
    if (taps)
        for (int j = 0; j < length; ++j) taps[j] = taps[j] / sum;
    return radius;
}

}  // extern "C"

// ---- the launches behind the plan's ops -------------------------------------------------------------------------------

static int base_blur(nm_sift_arena *const *as, int n, const float *const *gray, hipStream_t st)
{
    NmConvBatch base{};
    base.n = n;
    for (int f = 0; f < n; ++f) { base.result[f] = as[f]->lev[0][0]; base.image[f] = gray[f]; }
    return nm_launch_convolve_batch(base, as[0]->width, as[0]->height, as[0]->taps_base, as[0]->base_radius, st);
}

// Levels i_first .. i_last of octave o (ow x oh), one launch each. write_dog = false (frame driver): the DoG planes are not
// materialised -- detection forms them from the levels -- which takes 20 of the chain's 64 written bytes per pixel away (level 5
// has to be stored instead, store_top: + 4). The orders 1 and 2 issue levels 1-3 and 4-5 on different streams; the octave-0
// profile site then begins in front of level 1 on the one and ends behind level 5 on the other.
struct NmLevels { int o, ow, oh, i_first, i_last; bool store_top, write_dog, write_grad, decimate; };
static int octave_levels(nm_sift_arena *const *as, int n, const NmLevels &l, hipStream_t st)
{
    const int o = l.o;
    if (o == 0 && l.i_first == 1) nm_prof_begin(NM_PROF_PYRAMID_O0, st);
    const size_t plane = (size_t)l.ow * l.oh;
    int rc = 0;
    for (int i = l.i_first; i <= l.i_last && !rc; ++i) {
        // the launch that blurs level i-1 into level i also emits DoG i-1 and, for i-1 in 1..3, the gradient plane
        // i-2 of level i-1 (compute_gradients: level l from octave[l+1], sift/siftfunctions.cu:53-63)
        NmConvBatch b{};
        b.n = n;
        for (int f = 0; f < n; ++f) {
            nm_sift_arena *a = as[f];
            b.result[f] = (i < 5 || l.store_top) ? a->lev[o][i] : nullptr;     // level 5 is only read through DoG 4
            b.image[f] = a->lev[o][i - 1];
            b.dog[f] = l.write_dog ? a->dog[o][i - 1] : nullptr;
            b.grad[f] = (l.write_grad && i >= 2 && i <= 4) ? a->grad[o] + 2 * (size_t)(i - 2) * plane : nullptr;
            // level 3 decimated IS the next octave's level 0 (pyramidata / downsample.cu)
            b.down[f] = (l.decimate && i == 3) ? a->lev[o + 1][0] : nullptr;
        }
        rc = nm_launch_convolve_batch(b, l.ow, l.oh, as[0]->taps[i - 1], as[0]->radii[i - 1], st);
    }
    if (o == 0 && l.i_last == 5) nm_prof_end(NM_PROF_PYRAMID_O0, st);
    return rc;
}

// Detection, scan and ordered gather of octave o for all frames of the call.
static int detect_octave(nm_sift_arena *const *as, int n, int o, bool dogs, float *const *kp, int *const *d_num_items,
                         hipStream_t st)
{
    const SiftParams &P = as[0]->params;
    const int ow = as[0]->width >> o, oh = as[0]->height >> o;
    const int nseg = nm_divup(ow, NM_DET_SEG_W);
    const int n_blocks = oh * nseg;
    NmDetectArgs d{};
    NmScanArgs s{};
    NmGatherArgs g{};
    d.n = s.n = g.n = n;
    d.ow = ow; d.oh = oh; d.peak = P._peak_threshold; d.edge = P._edge_threshold; d.xper = (float)std::pow(2.0, o);
    d.sigma0 = P._sigma_0; d.num_dogs = P._num_dog_levels; d.stage_stride = as[0]->stage_stride;
    d.n_blocks = n_blocks; d.nseg = nseg;
    d.from_levels = dogs ? 0 : 1;
    d.plane_stride = as[0]->plane_stride[o];
    d.mask_w = as[0]->width; d.mask_h = as[0]->height;
    s.n_blocks = n_blocks; s.octave = o;
    g.stage_stride = as[0]->stage_stride; g.n_blocks = n_blocks; g.octave = o;
    s.capacity = as[0]->capacity; g.capacity = as[0]->capacity;
    for (int f = 0; f < n; ++f) {
        nm_sift_arena *a = as[f];
        d.plane0[f] = dogs ? a->dog[o][0] : a->lev[o][0];
        d.staging[f] = a->staging; d.counts[f] = a->counts;
        d.masks[f] = a->mask; d.any_mask |= a->mask ? 1 : 0;
        s.counts[f] = a->counts; s.offsets[f] = a->offsets; s.book[f] = a->book;
        s.d_num_items[f] = d_num_items ? d_num_items[f] : nullptr;
        g.staging[f] = a->staging; g.counts[f] = a->counts; g.offsets[f] = a->offsets; g.book[f] = a->book;
        g.kpts[f] = kp[f];
    }
    return nm_launch_detect_octave(d, s, g, st);
}

// The path a call of n frames on these arenas takes (n_arenas of them are looked at): THE decision, for the driver and for
// nm_sift_arena_launches_per_call.
static NmFrameConfig resolve_call(const nm_sift_arena *const *as, int n_arenas, int n)
{
    NmArenaTail tails[NM_MAX_BATCH];
    for (int f = 0; f < n_arenas; ++f) tails[f] = NmArenaTail{as[f]->tail_ok, as[f]->tail.T, as[f]->tail.n_oct};
    const NmFrameSwitches &sw = nm_frame_switches();
    return nm_frame_resolve(as[0]->params._num_octaves, tails, n_arenas, n, sw, g_frame_skew.load(std::memory_order_relaxed));
}

extern "C" {

// Kernel launches one nm_sift_detect_describe[_batch] call of n frames on this arena issues (HOST function): those of the
// call's plan. Base blur, five Gaussian launches + detect / scan / gather per octave, orientation + descriptors (twice where the
// description is split); with the octave tail (calls of up to NM_FRAME_TAIL_MAX_BATCH = 2 frames) the octaves >= T are two
// launches and the description runs in two parts.
int nm_sift_arena_launches_per_call(const nm_sift_arena *a, int n)
{
    if (!a || n <= 0) return 0;
    NmFrameOp ops[NM_FRAME_PLAN_MAX_OPS];
    return nm_frame_plan_launches(ops, nm_frame_plan(resolve_call(&a, 1, n), ops));
}

// HOST function (no device access): the plan of a call with this resolved configuration, six ints per op.
int nm_sift_frame_plan(int num_octaves, int first_tail, int split, int write_dog, int order, int *ops, int max_ops)
{
    NmFrameOp plan[NM_FRAME_PLAN_MAX_OPS];
    const int n = nm_frame_plan(NmFrameConfig{num_octaves, first_tail, split, write_dog ? 1 : 0, order}, plan);
    for (int k = 0; ops && k < n && k < max_ops; ++k) {
        const int v[6] = {plan[k].kind, plan[k].stream, plan[k].octave, plan[k].lo, plan[k].hi, plan[k].event};
        for (int j = 0; j < 6; ++j) ops[6 * k + j] = v[j];
    }
    return n;
}

// HOST function (no device access): nm_frame_resolve for a call of n frames on arenas of num_octaves octaves whose octave-tail
// plan starts at tail_first (0: they have none). cfg: num_octaves, first_tail, split, write_dog, order -- nm_sift_frame_plan's
// arguments.
int nm_sift_frame_resolve(int num_octaves, int tail_first, int n, int selected_order, int split, int cross_min_frames, int cfg[5])
{
    if (!cfg || num_octaves < 1 || num_octaves > NM_FRAME_MAX_OCTAVES || n < 1 || tail_first < 0) return (int)hipErrorInvalidValue;
    NmFrameSwitches sw = nm_frame_switches();
    if (split >= 0) sw.split = split;
    if (cross_min_frames >= 0) sw.cross_min_frames = cross_min_frames;
    const bool tail = tail_first > 0 && tail_first < num_octaves;
    const NmArenaTail t{tail, tail_first, tail ? num_octaves - tail_first : 0};
    const NmFrameConfig c = nm_frame_resolve(num_octaves, &t, 1, n, sw, selected_order);
    cfg[0] = c.num_octaves; cfg[1] = c.first_tail; cfg[2] = c.split; cfg[3] = c.dogs; cfg[4] = c.order;
    return 0;
}

int nm_sift_frame_cross_min_frames(void) { return nm_frame_switches().cross_min_frames; }

int nm_sift_octave_pyramid(nm_sift_arena *a, int ow, int oh, void *stream)
{
    if (!a || ow <= 0 || oh <= 0 || (size_t)ow * oh > a->npix) return (int)hipErrorInvalidValue;
    return octave_levels(&a, 1, NmLevels{0, ow, oh, 1, 5, true, true, true, false}, nm_stream(stream));
}

// Frame driver for n <= NM_MAX_BATCH equally sized frames: EVERY launch covers all frames of the call (the frame index is
// a grid dimension), so a call of 4 frames issues the same ~60 launches as a call of one, each 4x fatter. The
// scale-space chain (base blur, decimations, 5 fused Gaussian launches per octave) runs on the caller's stream; extrema +
// ordered compaction of octave o run on the side stream as soon as that octave's DoG planes exist, i.e.
// concurrently with the pyramid of octave o+1; orientation + descriptors follow on the side stream, which the caller's
// stream joins at the end. The helper streams and events are the set nm_helper_set_acquire keeps for the caller's stream, taken
// before the first operation is enqueued. Capture-safe (events only; a capture takes a set made beforehand). The call resolves
// its path, plans it (nm_frame_plan.hpp), fills the per-call arguments and walks the plan.
//
// Paths other than the plain one:
// NM_FRAME_SPLIT_DESCRIBE=2 (experiment, off by default): octaves 0 and 1 hold ~98 % of a frame's keypoints; their
// orientation + descriptor pass then starts as soon as octave 1 has been detected, on a stream of its own, beside the
// pyramids and detections of the small octaves, and the few keypoints of the small octaves are described at the end
// (output slots are octave-major: the passes write [oct_base[0], oct_base[2]) and [oct_base[2], num_items)). Measured
// (MI355X, round 3): throughput unchanged (2 260 vs 2 250 frame-pairs/s), a captured graph replays in the same 445 us per
// frame (this runtime executes a graph's branches one after the other), and eager single-frame calls, which are bound
// by the HOST's ~55 launches on the slower boxes, got 40 us slower (545 vs 507 us): two more launches and four more
// event operations. Not the default.
// Octave tail (nm_tail.hip): every arena of the call planned it for this geometry (same width / height => same plan).
// It is the LATENCY path: a call of one or two frames is a chain of dependent launches that no other frame's work fills
// (a 1080p frame: 22 launches instead of 55); in calls of many frames every per-octave launch is shared by all of them
// and runs at a better efficiency than the tail's LDS-fused tiles (halo recomputed per tile), so those keep them
// (16 frames per call, MI355X: 160 vs 171 us per frame). NM_FRAME_TAIL_MAX_BATCH moves the threshold.
int nm_sift_detect_describe_batch(nm_sift_arena *const *as, int n, const float *const *gray, float *const *desc,
                                  float *const *x, float *const *y, float *const *kpts, float *const *orients,
                                  int *const *d_num_items, void *stream)
{
    if (!as || n <= 0 || n > NM_MAX_BATCH || !gray || !desc || !x || !y) return (int)hipErrorInvalidValue;
    for (int f = 0; f < n; ++f) {
        if (!as[f] || !gray[f] || !desc[f] || !x[f] || !y[f]) return (int)hipErrorInvalidValue;
        if (as[f]->width != as[0]->width || as[f]->height != as[0]->height || as[f]->capacity != as[0]->capacity)
            return (int)hipErrorInvalidValue;
        // one set of thresholds per call (they are launch arguments); masks are per frame
        if (as[f]->params._peak_threshold != as[0]->params._peak_threshold ||
            as[f]->params._edge_threshold != as[0]->params._edge_threshold)
            return (int)hipErrorInvalidValue;
        for (int g = 0; g < f; ++g)
            if (as[g] == as[f]) return (int)hipErrorInvalidValue;
    }
    int cur = -1;
    NM_RETURN_IF(hipGetDevice(&cur));
    for (int f = 0; f < n; ++f)
        if (as[f]->device != cur) return (int)hipErrorInvalidDevice;     // arenas live on the device they were created on

    const NmFrameConfig cfg = resolve_call(as, n, n);
    NmFrameOp ops[NM_FRAME_PLAN_MAX_OPS];
    const int n_ops = nm_frame_plan(cfg, ops);
    if (n_ops <= 0) return (int)hipErrorInvalidValue;

    const SiftParams &P = as[0]->params;
    const int W = as[0]->width, H = as[0]->height;
    const bool dogs = cfg.dogs != 0;
    NmDescribeArgs da{};
    float *kp[NM_MAX_BATCH];
    da.n = n; da.num_octaves = P._num_octaves; da.num_dogs = P._num_dog_levels;
    for (int o = 0; o < 20; ++o) da.grad_off[o] = as[0]->grad_off[o];      // same geometry => same offsets in every arena
    for (int o = 0; o < P._num_octaves; ++o) { da.geom[o].ow = W >> o; da.geom[o].oh = H >> o; da.geom[o].xper = (float)std::pow(2.0, o); }
    for (int f = 0; f < n; ++f) {
        nm_sift_arena *a = as[f];
        kp[f] = (kpts && kpts[f]) ? kpts[f] : a->kpts;
        da.book[f] = a->book; da.kpts[f] = kp[f]; da.grad0[f] = a->grad[0];
        da.orients[f] = (orients && orients[f]) ? orients[f] : a->orients;
        da.desc[f] = desc[f]; da.x[f] = x[f]; da.y[f] = y[f];
    }
    NmTailArgs tail_args{};
    if (cfg.first_tail < cfg.num_octaves) {
        tail_args = as[0]->tail;
        tail_args.n = n;
        for (int f = 0; f < n; ++f) {
            tail_args.fr[f] = as[f]->tail_frame; tail_args.kpts[f] = kp[f];
            tail_args.d_num_items[f] = d_num_items ? d_num_items[f] : nullptr;
            tail_args.masks[f] = as[f]->mask; tail_args.any_mask |= as[f]->mask ? 1 : 0;
        }
        tail_args.mask_w = W; tail_args.mask_h = H;
        tail_args.peak = P._peak_threshold; tail_args.edge = P._edge_threshold; tail_args.sigma0 = P._sigma_0;
        tail_args.num_dogs = P._num_dog_levels; tail_args.capacity = as[0]->capacity;
        tail_args.state = as[0]->tail_state;
    }

    // every detection / description launch covers all frames of the call: ONE helper set serves it, the caller stream's
    NmHelperSet *hs = nullptr;
    {
        const int e = nm_helper_set_acquire(as[0], nm_stream(stream), &hs);
        if (e) return e;
    }
    const hipStream_t streams[3] = {nm_stream(stream), hs->side, hs->desc};
    auto event = [&](const NmFrameOp &p) {
        return p.event == NM_FE_PYR ? hs->ev_pyr[p.octave] : p.event == NM_FE_TOP ? hs->ev_top[p.octave]
               : p.event == NM_FE_DET ? hs->ev_det : p.event == NM_FE_DESC ? hs->ev_desc : hs->ev_join;
    };
    auto issue = [&](const NmFrameOp &p) -> int {
        const hipStream_t st = streams[p.stream];
        const int o = p.octave;
        switch (p.kind) {
        case NM_FO_BASE_BLUR: return base_blur(as, n, gray, st);
        case NM_FO_LEVELS:
            return octave_levels(as, n, NmLevels{o, W >> o, H >> o, p.lo, p.hi, !dogs, dogs, true, o + 1 < cfg.num_octaves}, st);
        case NM_FO_DETECT: return detect_octave(as, n, o, dogs, kp, d_num_items, st);
        case NM_FO_TAIL: return nm_launch_tail(tail_args, st);
        case NM_FO_TAIL_SCAN: return nm_launch_tail_scan(tail_args, st);
        case NM_FO_DESCRIBE: da.o_begin = p.lo; da.o_end = p.hi; return nm_launch_frame_describe(da, st);
        case NM_FO_RECORD: return (int)hipEventRecord(event(p), st);
        case NM_FO_WAIT: return (int)hipStreamWaitEvent(st, event(p), 0);
        default: return (int)hipErrorInvalidValue;
        }
    };
    // A helper stream is forked once a wait has been issued on it. After an error nothing more is launched, but every forked
    // stream is still joined (the plan's last ops): a stream capture would otherwise be left with an unjoined fork, and the next
    // call on this stream could overtake helper-stream work still in flight.
    bool forked[3] = {false, false, false};
    int rc = 0;
    for (int k = 0; k < n_ops; ++k) {
        const NmFrameOp &p = ops[k];
        if (p.kind == NM_FO_JOIN) {
            if (!forked[p.stream]) continue;
            const hipError_t e1 = hipEventRecord(event(p), streams[p.stream]);
            const hipError_t e2 = (e1 == hipSuccess) ? hipStreamWaitEvent(streams[NM_FS_CALLER], event(p), 0) : e1;
            if (!rc && e2 != hipSuccess) rc = (int)e2;
        } else if (!rc) {
            rc = issue(p);
            if (!rc && p.kind == NM_FO_WAIT) forked[p.stream] = p.stream != NM_FS_CALLER;
        }
    }
    return rc;
}

// The scale-space chain of nm_sift_detect_describe_batch alone (base blur, then per octave the five fused Gaussian + DoG +
// gradient launches with the decimation in the level-3 epilogue), exactly the launches the frame driver issues on the
// caller's stream, without detection / description: what bench.py times for the whole-pyramid roofline.
int nm_sift_scale_space_batch_ex(nm_sift_arena *const *as, int n, const float *const *gray, int write_dog, void *stream)
{
    if (!as || n <= 0 || n > NM_MAX_BATCH || !gray) return (int)hipErrorInvalidValue;
    int cur = -1;
    NM_RETURN_IF(hipGetDevice(&cur));
    for (int f = 0; f < n; ++f) {
        if (!as[f] || !gray[f] || as[f]->device != cur) return (int)hipErrorInvalidValue;
        if (as[f]->width != as[0]->width || as[f]->height != as[0]->height) return (int)hipErrorInvalidValue;
    }
    hipStream_t st = nm_stream(stream);
    const int num_octaves = as[0]->params._num_octaves;
    const int W = as[0]->width, H = as[0]->height;
    int rc = base_blur(as, n, gray, st);
    // write_dog bit 0: materialise the DoG planes; bit 1: leave the gradient planes out (measurement of the plain
    // Gaussian + DoG chain, the 108 B per octave-pixel of SURVEY.md 8(d), without the fused 36 B of gradients)
    const bool dogs = (write_dog & 1) != 0, grads = (write_dog & 2) == 0;
    for (int o = 0; !rc && o < num_octaves; ++o)
        rc = octave_levels(as, n, NmLevels{o, W >> o, H >> o, 1, 5, !dogs, dogs, grads, o + 1 < num_octaves}, st);
    return rc;
}

int nm_sift_scale_space_batch(nm_sift_arena *const *as, int n, const float *const *gray, void *stream)
{
    return nm_sift_scale_space_batch_ex(as, n, gray, 1, stream);
}

int nm_sift_detect_describe(nm_sift_arena *a, const float *gray, float *desc, float *x, float *y, float *kpts,
                            float *orients, int *d_num_items, void *stream)
{
    return nm_sift_detect_describe_batch(&a, 1, &gray, &desc, &x, &y, &kpts, &orients, &d_num_items, stream);
}

}  // extern "C"
