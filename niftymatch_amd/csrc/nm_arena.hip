// nm_arena.hip -- the frame driver's arena: creation (every buffer and the octave-tail plan of one geometry), destruction, the
// accessors and the thresholds / mask setters, and the octave tail's diagnostics; and the per-device pool of helper sets (the
// helper streams and events of a call). The driver that runs a call on arenas is nm_frame.hip.
#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "nm_arena.hpp"
#include "nm_frame_plan.hpp"

// ---- helper sets ---------------------------------------------------------------------------------------------------------
// A process used to hold two helper streams per arena (about 130 with the 64 arenas of a many-frame call) of which a call
// only ever used the first arena's pair; which hardware queue those two shared with the caller's stream was then a matter of
// where among all the others they had been created. Now a process holds two helper streams per caller stream in use, created
// in the order in which the caller streams issue their first call.
// (Round 5, measured: HIP stream priorities for the two helper streams -- the device offers 0 and -1 -- change nothing when one
// of them is raised (headline 2 934-3 058 against 2 953-3 047) and cost 17 % when both are (2 479-2 498).)
namespace {

void helper_set_destroy(NmHelperSet *s)
{
    if (s->side) { (void)hipStreamSynchronize(s->side); (void)hipStreamDestroy(s->side); }
    if (s->desc) { (void)hipStreamSynchronize(s->desc); (void)hipStreamDestroy(s->desc); }
    for (int o = 0; o < 20; ++o) {
        if (s->ev_pyr[o]) (void)hipEventDestroy(s->ev_pyr[o]);
        if (s->ev_top[o]) (void)hipEventDestroy(s->ev_top[o]);
    }
    if (s->ev_join) (void)hipEventDestroy(s->ev_join);
    if (s->ev_det) (void)hipEventDestroy(s->ev_det);
    if (s->ev_desc) (void)hipEventDestroy(s->ev_desc);
    *s = NmHelperSet{};
}

// On the current device. A set is geometry-free: it holds the events of all 20 octaves a plan can name.
int helper_set_create(NmHelperSet *s)
{
    *s = NmHelperSet{};
    int rc = 0;
    for (int o = 0; !rc && o < 20; ++o) rc = (int)hipEventCreateWithFlags(&s->ev_pyr[o], hipEventDisableTiming);
    for (int o = 0; !rc && o < 20; ++o) rc = (int)hipEventCreateWithFlags(&s->ev_top[o], hipEventDisableTiming);
    if (!rc) rc = (int)hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming);
    if (!rc) rc = (int)hipEventCreateWithFlags(&s->ev_det, hipEventDisableTiming);
    if (!rc) rc = (int)hipEventCreateWithFlags(&s->ev_desc, hipEventDisableTiming);
    if (!rc) rc = (int)hipStreamCreateWithFlags(&s->side, hipStreamNonBlocking);
    if (!rc) rc = (int)hipStreamCreateWithFlags(&s->desc, hipStreamNonBlocking);
    if (rc) helper_set_destroy(s);
    return rc;
}

// sets[0, assigned) serve the caller streams key[.]; sets[assigned, created) are spares. A stream capture must not create
// streams, so whenever the pool is touched outside a capture it makes sure that ONE spare stands ready: a capture on a caller
// stream that has not issued a call yet then takes the spare. The sets live until the process ends: they are never destroyed
// (a static destructor would run after the HIP runtime has begun to shut down), which leaks at most NM_HELPER_POOL_SETS sets
// per device, once.
struct HelperPool {
    NmHelperSet sets[NM_HELPER_POOL_SETS];
    hipStream_t key[NM_HELPER_POOL_SETS];
    int assigned, created;
};
HelperPool g_pool[NM_HELPER_POOL_DEVICES] = {};
std::mutex g_pool_mutex;

void pool_reserve(HelperPool &p, int want)          // g_pool_mutex held, not capturing; failures leave the pool as it is
{
    want = std::min(want, NM_HELPER_POOL_SETS);
    while (p.created < want && helper_set_create(&p.sets[p.created]) == 0) ++p.created;
}

bool capturing(hipStream_t st)
{
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &status) != hipSuccess) {
        (void)hipGetLastError();                    // e.g. the legacy stream while another stream captures: create nothing
        return true;
    }
    return status != hipStreamCaptureStatusNone;
}

}  // namespace

int nm_helper_set_acquire(nm_sift_arena *a0, hipStream_t caller, NmHelperSet **out)
{
    std::lock_guard<std::mutex> lock(g_pool_mutex);
    if (a0->device >= 0 && a0->device < NM_HELPER_POOL_DEVICES) {
        HelperPool &p = g_pool[a0->device];
        for (int i = 0; i < p.assigned; ++i)
            if (p.key[i] == caller) { *out = &p.sets[i]; return 0; }
        const bool cap = capturing(caller);
        if (!cap) pool_reserve(p, p.assigned + 1);
        if (p.assigned < p.created) {
            p.key[p.assigned] = caller;
            *out = &p.sets[p.assigned++];
            if (!cap) pool_reserve(p, p.assigned + 1);
            return 0;
        }
    }
    // the pool is full (or has nothing ready for a capture): the first arena's own set, made when first needed
    if (!a0->own) {
        NmHelperSet *s = new (std::nothrow) NmHelperSet();
        if (!s) return (int)hipErrorOutOfMemory;
        const int rc = helper_set_create(s);
        if (rc) { delete s; return rc; }
        a0->own = s;
    }
    *out = a0->own;
    return 0;
}

extern "C" {

int nm_sift_arena_create(int width, int height, int capacity, nm_sift_arena **out)
{
    if (!out || width <= 0 || height <= 0 || capacity <= 0) return (int)hipErrorInvalidValue;
    nm_sift_arena *a = new (std::nothrow) nm_sift_arena();
    if (!a) return (int)hipErrorOutOfMemory;
    a->width = width; a->height = height; a->capacity = capacity;
    a->own = nullptr;
    a->mask = nullptr;
    a->device = -1;
    (void)hipGetDevice(&a->device);
    a->params = SiftParams(width, height);
    a->npix = (size_t)width * height;
    a->bytes = 0;
    const SiftParams &P = a->params;
    if (P._num_octaves > 20 || (int)P._sigmas.size() > 8) { delete a; return (int)hipErrorInvalidValue; }
    int rc = 0;
    auto upload = [&](float sigma, float **dev, int *radius) -> int {
        *radius = nm_create_kernel_for_sigma(sigma, nullptr);
        std::vector<float> h(2 * *radius + 1);
        nm_create_kernel_for_sigma(sigma, h.data());
        int e = a->alloc(dev, h.size());
        if (e) return e;
        return (int)hipMemcpy(*dev, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice);
    };
    rc = upload(P._base_smooth, &a->taps_base, &a->base_radius);
    for (size_t i = 0; !rc && i < P._sigmas.size(); ++i) rc = upload(P._sigmas[i], &a->taps[i], &a->radii[i]);
    // an octave's six levels (and its five DoG planes) are ONE block, plane p at p * plane_stride[o]: the detection launches then
    // take one pointer per frame (NmDetectArgs). The stride is the plane rounded up to 4 floats: every plane 16-byte aligned.
    for (int o = 0; !rc && o < P._num_octaves; ++o) {
        const size_t plane = (size_t)(width >> o) * (height >> o);
        a->plane_stride[o] = (plane + 3) & ~(size_t)3;
        float *blk = nullptr;
        rc = a->alloc(&blk, 6 * a->plane_stride[o]);
        for (int i = 0; i < 6; ++i) a->lev[o][i] = blk + i * a->plane_stride[o];
        if (!rc) rc = a->alloc(&blk, 5 * a->plane_stride[o]);
        for (int i = 0; i < 5; ++i) a->dog[o][i] = blk + i * a->plane_stride[o];
    }
    {   // the gradient planes of all octaves: one block (NmDescribeArgs takes one pointer per frame and the offsets)
        size_t total = 0;
        for (int o = 0; o < 20; ++o) a->grad_off[o] = 0;
        for (int o = 0; o < P._num_octaves; ++o) {
            a->grad_off[o] = total;
            total += (6 * (size_t)(width >> o) * (height >> o) + 3) & ~(size_t)3;
        }
        float *blk = nullptr;
        if (!rc) rc = a->alloc(&blk, total);
        for (int o = 0; o < P._num_octaves; ++o) a->grad[o] = blk + a->grad_off[o];
    }
    // No streams and no events here: a call takes its helper set from the device's pool (nm_helper_set_acquire). An arena is
    // never created inside a stream capture, so this is where the pool's spare set is made for a process whose FIRST call is
    // captured.
    if (a->device >= 0 && a->device < NM_HELPER_POOL_DEVICES) {
        std::lock_guard<std::mutex> lock(g_pool_mutex);
        pool_reserve(g_pool[a->device], g_pool[a->device].assigned + 1);
    }
    a->max_blocks = height * nm_divup(width, NM_DET_SEG_W);
    a->stage_stride = (size_t)a->max_blocks * 256;
    if (!rc) rc = a->alloc(&a->staging, 3 * a->stage_stride * 4);
    if (!rc) rc = a->alloc(&a->counts, (size_t)3 * a->max_blocks);
    if (!rc) rc = a->alloc(&a->offsets, (size_t)3 * a->max_blocks);
    if (!rc) rc = a->alloc(&a->book, 1);
    if (!rc) rc = a->alloc(&a->kpts, (size_t)4 * capacity);
    if (!rc) rc = a->alloc(&a->orients, (size_t)2 * capacity);
    if (!rc) rc = (int)hipMemset(a->book, 0, sizeof(NmFrameBook));
    // octave tail: first octave T = 2 (NM_FRAME_TAIL=0 switches it off, 1..3 choose T): octaves 0 and 1 are real streaming
    // work for the whole chip and keep their per-octave launches
    a->tail_ok = false; a->tail_frame = NmTailFrame{}; a->tail_state = nullptr;
    for (int o = 0; o < 20; ++o) { a->stg[o] = nullptr; a->stg_stride[o] = 0; a->cnt[o] = nullptr; }
    {
        const char *e = getenv("NM_FRAME_TAIL");
        const int T = e ? atoi(e) : 2;
        int radii[5] = {0, 0, 0, 0, 0};
        for (size_t i = 0; i < P._sigmas.size() && i < 5; ++i) radii[i] = a->radii[i];
        if (!rc && T >= 1 && T <= 3 && P._sigmas.size() == 5 && P._num_dog_levels == 3 && !nm_frame_switches().dogs &&
            nm_tail_plan(a->tail, width, height, P._num_octaves, T, radii)) {
            NmTailFrame &h = a->tail_frame;
            for (int o = T; !rc && o < P._num_octaves; ++o) {
                const int j = o - T;
                for (int i = 0; i < 6; ++i) h.lev[j][i] = a->lev[o][i];
                h.grad[j] = a->grad[o];
                const size_t units = (size_t)(height >> o) * nm_divup(width >> o, NM_DET_SEG_W);
                a->stg_stride[o] = units * 256;
                rc = a->alloc(&a->stg[o], 3 * a->stg_stride[o] * 4);
                if (!rc) rc = a->alloc(&a->cnt[o], 3 * units);
                h.staging[j] = a->stg[o]; h.stage_stride[j] = a->stg_stride[o]; h.counts[j] = a->cnt[o];
            }
            h.book = a->book;
            if (!rc) rc = a->alloc(&a->tail_state, NM_TAIL_STATE_INTS);
            if (!rc) rc = (int)hipMemset(a->tail_state, 0, NM_TAIL_STATE_INTS * sizeof(int));
            for (int i = 0; i < 5; ++i) a->tail.taps[i] = a->taps[i];
            a->tail.trace = nullptr;
            const char *tr = getenv("NM_TAIL_TRACE");          // diagnostic: per-item timestamps of the tail launch
            if (!rc && tr && tr[0] == '1') {
                rc = a->alloc(&a->tail.trace, (size_t)16 * NM_TAIL_MAX_FRAMES * a->tail.items_per_frame);
                if (!rc) rc = (int)hipMemset(a->tail.trace, 0, (size_t)128 * NM_TAIL_MAX_FRAMES * a->tail.items_per_frame);
            }
            a->tail_ok = !rc;
        }
    }
    if (!rc) rc = (int)hipDeviceSynchronize();
    if (rc) { nm_sift_arena_destroy(a); return rc; }
    *out = a;
    return 0;
}

void nm_sift_arena_destroy(nm_sift_arena *a)
{
    if (!a) return;
    // The pool's sets stay: later calls on other arenas use them. Only a set of this arena's own (calls beyond the pool's cap
    // that had this arena first) goes, behind the work still on its streams.
    if (a->own) { helper_set_destroy(a->own); delete a->own; }
    // (hipFree waits for the device's streams, the pooled helper streams among them, before it releases a buffer)
    for (void *p : a->allocs) (void)hipFree(p);
    delete a;
}

size_t nm_sift_arena_bytes(const nm_sift_arena *a) { return a ? a->bytes : 0; }

// Diagnostic: the per-item record of the arena's last octave-tail launch (NM_TAIL_TRACE=1 when the arena was created; the
// arena must have been the FIRST of its call). Synchronises the device. out: 4 words per item -- kind | slot << 8 | frame
// << 16 | index << 24 | workgroup << 48, then the 100 MHz clock when the ticket was drawn, when its inputs were ready, when it
// was done. Returns the number of items per frame (0: no trace), *n_segments / segments (5 ints each: kind, slot, items per
// frame, first item, octave) describe the plan.
int nm_sift_arena_tail_trace(const nm_sift_arena *a, unsigned long long *out, int max_items, int *segments, int max_segments)
{
    if (!a || !a->tail_ok) return 0;
    for (int i = 0; segments && i < a->tail.n_seg && i < max_segments; ++i) {
        const NmTailSeg &g = a->tail.seg[i];
        int *r = segments + 5 * i;
        r[0] = g.kind; r[1] = g.slot; r[2] = g.per_frame; r[3] = g.first_per_frame; r[4] = a->tail.oct[g.slot].o;
    }
    // the trace buffer holds NM_TAIL_MAX_FRAMES * items_per_frame records of 128 bytes: never copy past it
    max_items = std::min(max_items, NM_TAIL_MAX_FRAMES * a->tail.items_per_frame);
    if (out && a->tail.trace && max_items > 0) {
        // layout of the launch's record: 4 words per item for all n_frames * items_per_frame items, then 12 phase stamps per item
        // (conv items only); max_items must be that product, out holds 16 words per item
        if (hipDeviceSynchronize() != hipSuccess) return -1;
        if (hipMemcpy(out, a->tail.trace, (size_t)max_items * 128, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    }
    return a->tail.items_per_frame;
}
int nm_sift_arena_tail_segments(const nm_sift_arena *a) { return (a && a->tail_ok) ? a->tail.n_seg : 0; }

// Status of the last octave-tail launch that used this arena's state words (the FIRST arena of a call of <= 2 frames lends
// them): 0 = complete, 1 = a wait inside the launch hit its spin limit and the octaves >= T of that call's frames were dropped
// (their d_num_items read -1). Synchronises `stream`. An arena without a tail plan reports 0.
int nm_sift_arena_tail_status(const nm_sift_arena *a, int *status, void *stream)
{
    if (!a || !status) return (int)hipErrorInvalidValue;
    *status = 0;
    if (!a->tail_ok) return 0;
    NM_RETURN_IF(hipStreamSynchronize(nm_stream(stream)));
    NM_RETURN_IF(hipMemcpy(status, a->tail_state + 3, sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

// TEST HOOK: sets the sticky error word of the arena's tail state, as a timed-out wait would, so that the NEXT tail launch on
// it drains without working (tests/test_gpu_tail.py: the call must report failure and the call after it must be correct).
int nm_sift_arena_tail_inject_error(nm_sift_arena *a)
{
    if (!a || !a->tail_ok) return (int)hipErrorInvalidValue;
    const int one = 1;
    NM_RETURN_IF(hipDeviceSynchronize());
    NM_RETURN_IF(hipMemcpy(a->tail_state + 2, &one, sizeof(int), hipMemcpyHostToDevice));
    return 0;
}

// HOST function (no device access): the octave-tail plan of a width x height frame with first tail octave T -- what
// nm_sift_arena_create makes for the arena. segments: 8 ints each (kind, slot, items per frame, first item, octave, whole
// plane?, octave width, octave height); info: items per frame, LDS bytes of the tail launch, LDS bytes of the scan launch,
// tail octaves. Returns the number of segments, 0 when the geometry takes the per-octave launches.
int nm_sift_tail_plan(int width, int height, int T, int *segments, int max_segments, int info[4])
{
    if (width <= 0 || height <= 0) return 0;
    const SiftParams P(width, height);
    NmTailArgs a{};
    int radii[5] = {0, 0, 0, 0, 0};
    if (P._sigmas.size() != 5) return 0;
    for (int i = 0; i < 5; ++i) radii[i] = nm_create_kernel_for_sigma(P._sigmas[i], nullptr);
    if (!nm_tail_plan(a, width, height, P._num_octaves, T, radii)) return 0;
    for (int i = 0; segments && i < a.n_seg && i < max_segments; ++i) {
        const NmTailSeg &g = a.seg[i];
        const NmTailOct &oc = a.oct[g.slot];
        int *r = segments + 8 * i;
        r[0] = g.kind; r[1] = g.slot; r[2] = g.per_frame; r[3] = g.first_per_frame; r[4] = oc.o; r[5] = oc.whole; r[6] = oc.ow; r[7] = oc.oh;
    }
    if (info) { info[0] = a.items_per_frame; info[1] = a.lds_bytes; info[2] = a.scan_lds_bytes; info[3] = a.n_oct; }
    return a.n_seg;
}

// The reference's run-time knobs on the frame driver: SiftParams::_peak_threshold / _edge_threshold are public fields read
// per compute_keypoints call (sift/siftparams.h:97-98, siftfunctions.cu:123-125); compute_keypoints_with_mask
// (siftfunctions.cu:65-98) restricts detection to where the full-resolution mask's bilinear fetch is >= 1 (keypoint.cu:214).
int nm_sift_arena_set_params(nm_sift_arena *a, float peak_threshold, float edge_threshold)
{
    if (!a || !(edge_threshold > 0.f) || peak_threshold != peak_threshold) return (int)hipErrorInvalidValue;
    a->params._peak_threshold = peak_threshold;
    a->params._edge_threshold = edge_threshold;
    return 0;
}

int nm_sift_arena_get_params(const nm_sift_arena *a, float *peak_threshold, float *edge_threshold)
{
    if (!a) return (int)hipErrorInvalidValue;
    if (peak_threshold) *peak_threshold = a->params._peak_threshold;
    if (edge_threshold) *edge_threshold = a->params._edge_threshold;
    return 0;
}

int nm_sift_arena_set_mask(nm_sift_arena *a, const float *mask, int mask_width, int mask_height)
{
    if (!a || (mask && (mask_width != a->width || mask_height != a->height))) return (int)hipErrorInvalidValue;
    a->mask = mask;
    return 0;
}
float *nm_sift_arena_level(nm_sift_arena *a, int l) { return (a && l >= 0 && l < 6) ? a->lev[0][l] : nullptr; }
float *nm_sift_arena_dog(nm_sift_arena *a, int d) { return (a && d >= 0 && d < 5) ? a->dog[0][d] : nullptr; }
float *nm_sift_arena_grad(nm_sift_arena *a) { return a ? a->grad[0] : nullptr; }

}  // extern "C"
