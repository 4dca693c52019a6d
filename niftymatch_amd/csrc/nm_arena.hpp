// nm_arena.hpp -- the frame driver's arena (internal, not C ABI): every buffer one frame's detect / describe call needs,
// allocated once by nm_sift_arena_create (nm_arena.hip) and used by the driver (nm_frame.hip), and the helper sets -- the two
// helper streams and the events of a call's plan --, which belong to the CALLER's stream, not to an arena.
#pragma once
#include <vector>

#include "../../include/nm_abi.h"
#include "../nm/siftparams.h"
#include "nm_common.hpp"
#include "nm_tail.hpp"

// The helper streams and events one call's plan (nm_frame_plan.hpp) names. Every launch of a call covers all its frames, so a
// call needs ONE set whatever its size.
struct NmHelperSet {
    hipStream_t side;          // detection / compaction stream forked off the caller's stream
    hipStream_t desc;          // orientation + descriptors of the large octaves, beside the small octaves' pyramids / detection;
                               // in the cross issue order levels 4-5 of every octave instead
    hipEvent_t ev_pyr[20], ev_join, ev_det, ev_desc;
    hipEvent_t ev_top[20];     // cross issue order: behind level 5 of octave o on the desc stream
};
// Sets the pool keeps per device: one per caller stream that has issued a call, plus one spare (see nm_helper_set_acquire).
// bench.py's --streams / --host-threads run 1..8 caller streams and its latency probe two more; the GPU tests use at most four
// at a time. Caller streams beyond the cap take the first arena's own set.
constexpr int NM_HELPER_POOL_SETS = 16;
constexpr int NM_HELPER_POOL_DEVICES = 16;

struct nm_sift_arena;
// The set a call on `caller` with first arena a0 uses. Calls on one caller stream share a set: the stream orders them, and
// every plan ends with the joins of its helper streams. Calls on different caller streams get different sets.
int nm_helper_set_acquire(nm_sift_arena *a0, hipStream_t caller, NmHelperSet **out);

struct nm_sift_arena {
    int width, height, capacity;
    int device;                // the HIP device every buffer belongs to
    SiftParams params;
    size_t npix;
    size_t bytes;
    std::vector<void *> allocs;
    float *taps_base; int base_radius;
    float *taps[8]; int radii[8];
    float *lev[20][6];         // Gaussian levels PER OCTAVE (the single-octave API call uses lev[0]): the frame driver's detection
                               // reads them (DoG = difference of consecutive levels, formed in the detection kernel) while the next
                               // octave's pyramid is being computed, so the octaves cannot share planes
    float *dog[20][5];         // DoG planes PER OCTAVE: detection of octave o overlaps the pyramid of octave o+1
    NmHelperSet *own;          // NULL until a call with this arena first finds the pool full (or empty while capturing)
    float *grad[20];           // per octave: 3 float2 planes
    size_t grad_off[20];       // grad[o] = grad[0] + grad_off[o]: the gradient planes of all octaves are one block
    size_t plane_stride[20];   // floats between consecutive levels / DoG planes of an octave (one block per octave)
    float *staging; size_t stage_stride;
    int *counts, *offsets; int max_blocks;
    NmFrameBook *book;
    float *kpts, *orients;     // internal lists used when the caller passes NULL
    const float *mask;         // nm_sift_arena_set_mask: caller-owned full-resolution plane (width x height) or NULL
    // octave tail (nm_tail.hip): the octaves >= tail.T of a call run as ONE persistent launch. Their detection stages into
    // per-octave lists (an octave's gather may run after the next octave's detection), the launch finds a frame's planes in a
    // device-resident table, and the FIRST arena of a call lends its state words (zero between launches).
    float *stg[20]; size_t stg_stride[20]; int *cnt[20];
    NmTailFrame tail_frame;      // this arena's planes of the tail octaves (copied into the launch's arguments)
    int *tail_state;
    NmTailArgs tail;           // the plan for this geometry (per-call fields are filled by the driver)
    bool tail_ok;

    template <typename T>
    int alloc(T **p, size_t n)
    {
        void *q = nullptr;
        const size_t b = n * sizeof(T);
        hipError_t e = hipMalloc(&q, b ? b : 4);
        if (e != hipSuccess) return (int)e;
        allocs.push_back(q);
        bytes += b;
        *p = static_cast<T *>(q);
        return 0;
    }
};
