// nm_frame_plan.hpp -- the schedule of one nm_sift_detect_describe_batch call as DATA: which launches, on which of the call's
// three streams, behind which events. HOST ONLY (no HIP types: any C++17 compiler takes it). nm_frame_resolve decides the path
// of a call once -- the driver and nm_sift_arena_launches_per_call both ask it --, nm_frame_plan writes the ops in issue order
// and the driver (nm_frame.hip) walks them. That the schedule is free of hazards, capturable and joined on every error path
// is checked on the plan, for every configuration, without a GPU: tests/test_frame_plan.py.
#pragma once
#include <cstdlib>

constexpr int NM_FRAME_MAX_OCTAVES = 20;
constexpr int NM_FRAME_TAIL_MAX_FRAMES = 2;        // frames one octave-tail launch serves (= NM_TAIL_MAX_FRAMES, nm_tail.hpp)

enum NmFrameStream { NM_FS_CALLER = 0,             // the caller's stream: base blur, the levels, the tail
                     NM_FS_SIDE = 1,               // the helper set's side stream: detection, the description
                     NM_FS_DESC = 2 };             // its description stream: early description (split), levels 4-5 (cross order)
enum NmFrameEvent { NM_FE_NONE = -1,
                    NM_FE_PYR = 0,                 // ev_pyr[octave]: behind the octave's last level on the caller's stream
                    NM_FE_TOP = 1,                 // ev_top[octave]: behind level 5 on the description stream (cross order)
                    NM_FE_DET = 2, NM_FE_DESC = 3, NM_FE_JOIN = 4 };
enum NmFrameOpKind {
    NM_FO_BASE_BLUR = 0,                           // 1 launch: gray -> level 0 of octave 0
    NM_FO_LEVELS = 1,                              // levels lo..hi of `octave`, one launch each
    NM_FO_DETECT = 2,                              // 3 launches: detect, scan, gather of `octave`
    NM_FO_TAIL = 3,                                // 1 launch: levels, gradients, detection of the octaves >= first_tail
    NM_FO_TAIL_SCAN = 4,                           // 1 launch: their book-keeping scans + gathers
    NM_FO_DESCRIBE = 5,                            // 2 launches: orientations + descriptors of the octaves [lo, hi)
    NM_FO_RECORD = 6, NM_FO_WAIT = 7,              // `event` on `stream`
    NM_FO_JOIN = 8                                 // record `event` on the helper `stream`, the caller's stream waits for it
};

struct NmFrameOp { int kind, stream, octave, lo, hi, event; };     // six ints: nm_sift_frame_plan hands them out as they are

// A call's resolved path. first_tail == num_octaves: no octave tail. split: the octaves < split are described early (0: one
// description pass). order: 0 plain, 1 skewed, 2 cross (nm_sift_set_frame_skew).
struct NmFrameConfig { int num_octaves, first_tail, split, dogs, order; };

// widest plan: the cross order's seven ops per octave; base blur, one early description (record, wait, describe), the final
// one (wait, tail scan, describe) and two joins around them
constexpr int NM_FRAME_PLAN_MAX_OPS = 1 + 7 * NM_FRAME_MAX_OCTAVES + 3 + 3 + 2;

// The switches of the frame driver, each read from the environment ONCE per process, here.
struct NmFrameSwitches {
    bool dogs;                 // NM_FRAME_DOG=1: materialise the DoG planes (detection then reads them); no octave tail
    int split;                 // NM_FRAME_SPLIT_DESCRIBE=k: describe the octaves < k early, on a stream of their own
    int tail_max_batch;        // NM_FRAME_TAIL_MAX_BATCH (2): calls of more frames take the per-octave launches
    int order;                 // NM_FRAME_SKEW (0): the issue order where nm_sift_set_frame_skew has not set one
    bool order_env;            // NM_FRAME_SKEW is set: it then holds for calls of every size
    int cross_min_frames;      // NM_FRAME_CROSS_MIN_FRAMES: calls of at least so many frames default to the cross order; 0: never
};
#ifndef NM_FRAME_SKEW_DEFAULT
#define NM_FRAME_SKEW_DEFAULT 0
#endif
// Frames per call from which the cross order (2) is the default. 0 = never: measured on MI355X with the three streams on three
// hardware queues, the cross order is 1-47 us per call SLOWER than order 0 for calls of 64, 32, 16 and 4 frames
// (profiles/r12_a_cross_order_alternation.txt, r12_a_call_timeline_cross.txt).
#ifndef NM_FRAME_CROSS_MIN_FRAMES
#define NM_FRAME_CROSS_MIN_FRAMES 0
#endif
inline const NmFrameSwitches &nm_frame_switches()
{
    static const NmFrameSwitches s = [] {
        NmFrameSwitches v;
        const char *e = getenv("NM_FRAME_DOG");
        v.dogs = e && e[0] == '1';
        e = getenv("NM_FRAME_SPLIT_DESCRIBE");
        v.split = e ? atoi(e) : 0;
        e = getenv("NM_FRAME_TAIL_MAX_BATCH");
        v.tail_max_batch = e ? atoi(e) : 2;
        e = getenv("NM_FRAME_SKEW");
        const int m = e ? atoi(e) : NM_FRAME_SKEW_DEFAULT;
        v.order = (m >= 0 && m <= 2) ? m : NM_FRAME_SKEW_DEFAULT;
        v.order_env = e != nullptr && m >= 0 && m <= 2;
        e = getenv("NM_FRAME_CROSS_MIN_FRAMES");
        v.cross_min_frames = e ? atoi(e) : NM_FRAME_CROSS_MIN_FRAMES;
        if (v.cross_min_frames < 0) v.cross_min_frames = 0;
        return v;
    }();
    return s;
}

struct NmArenaTail { bool ok; int T, n_oct; };     // an arena's octave-tail plan (made when the arena was created)

// THE path decision of a call of n frames on arenas with these tail plans (n_arenas of them: all of the call's for the
// driver, one for nm_sift_arena_launches_per_call). selected: the order nm_sift_set_frame_skew set, -1 for the default -- which
// is NM_FRAME_SKEW where the environment names one, else the cross order for calls of at least sw.cross_min_frames frames and
// sw.order below that.
inline NmFrameConfig nm_frame_resolve(int num_octaves, const NmArenaTail *tails, int n_arenas, int n, const NmFrameSwitches &sw,
                                      int selected)
{
    const int order = (selected >= 0 && selected <= 2) ? selected
                      : (!sw.order_env && sw.cross_min_frames > 0 && n >= sw.cross_min_frames) ? 2 : sw.order;
    NmFrameConfig c;
    c.num_octaves = num_octaves;
    c.dogs = sw.dogs ? 1 : 0;
    c.split = (sw.split > 0 && sw.split < num_octaves) ? sw.split : 0;
    // The octave tail is the LATENCY path (calls of one or two frames). The first arena's plan is paired with every arena's
    // own plane table: the plans must be the same plan -- T comes from NM_FRAME_TAIL at arena creation, so arenas of one
    // geometry CAN differ -- or the call takes the per-octave launches.
    bool tail = !c.dogs && !c.split && n <= sw.tail_max_batch && n <= NM_FRAME_TAIL_MAX_FRAMES;
    for (int f = 0; f < n_arenas; ++f)
        tail = tail && tails[f].ok && tails[f].T == tails[0].T && tails[f].n_oct == tails[0].n_oct;
    c.first_tail = tail ? tails[0].T : num_octaves;
    // With the tail, the octaves < T are described as soon as octave T - 1 has been detected, beside the tail launch.
    if (tail) c.split = c.first_tail;
    // the skewed and cross orders are for the per-octave path with one description pass (the description stream is then free
    // to carry the cross order's levels 4-5)
    c.order = (tail || c.split) ? 0 : order;
    return c;
}

// Writes the call's ops into ops[NM_FRAME_PLAN_MAX_OPS] in issue order; the JOIN ops (description stream, then side stream)
// come last. Returns their number, 0 for a configuration nm_frame_resolve does not produce.
inline int nm_frame_plan(const NmFrameConfig &c, NmFrameOp *ops)
{
    const int O = c.num_octaves, T = c.first_tail;
    if (O < 1 || O > NM_FRAME_MAX_OCTAVES || T < 1 || T > O || c.order < 0 || c.order > 2) return 0;
    const bool tail = T < O;
    if (tail ? (c.split != T || c.dogs) : (c.split < 0 || c.split >= O)) return 0;
    if (c.split && c.order) return 0;
    int k = 0;
    bool forked[3] = {false, false, false};
    auto put = [&](int kind, int stream, int octave, int lo, int hi, int event) {
        ops[k++] = NmFrameOp{kind, stream, octave, lo, hi, event};
        if (kind == NM_FO_WAIT) forked[stream] = true;
    };
    put(NM_FO_BASE_BLUR, NM_FS_CALLER, 0, 0, 0, NM_FE_NONE);
    for (int o = 0; o < T; ++o) {
        // orders 1 and 2: the caller's stream carries levels 1-3 only (level 3's launch decimates into the next octave's
        // level 0; nothing of octave o + 1 reads levels 4-5), ev_pyr[o] then stands behind level 3
        put(NM_FO_LEVELS, NM_FS_CALLER, o, 1, c.order ? 3 : 5, NM_FE_NONE);
        put(NM_FO_RECORD, NM_FS_CALLER, o, 0, 0, NM_FE_PYR);
        // The tail launch goes to the CALLER's stream, straight behind the pyramid of octave T - 1 whose decimated level 3 seeds
        // it -- issued BEFORE this octave's detection launches so that the host does not hold it back -- and runs beside the
        // detection of the octaves < T on the side stream.
        if (tail && o + 1 == T) put(NM_FO_TAIL, NM_FS_CALLER, T, 0, 0, NM_FE_NONE);
        if (c.order == 2) {
            put(NM_FO_WAIT, NM_FS_DESC, o, 0, 0, NM_FE_PYR);
            put(NM_FO_LEVELS, NM_FS_DESC, o, 4, 5, NM_FE_NONE);
            put(NM_FO_RECORD, NM_FS_DESC, o, 0, 0, NM_FE_TOP);
            put(NM_FO_WAIT, NM_FS_SIDE, o, 0, 0, NM_FE_TOP);
        } else {
            put(NM_FO_WAIT, NM_FS_SIDE, o, 0, 0, NM_FE_PYR);
        }
        if (c.order == 1) put(NM_FO_LEVELS, NM_FS_SIDE, o, 4, 5, NM_FE_NONE);
        put(NM_FO_DETECT, NM_FS_SIDE, o, 0, 0, NM_FE_NONE);
        // (Describing the octaves below T - 1 even earlier, on the description stream beside octave T - 1's pyramid and
        // detection, was measured: 435 instead of 282 us per frame -- the descriptor kernel fills every CU's wave slots and
        // the tail launch's 1 024-thread workgroups, issued at the same time, wait for whole CUs: 158 instead of 98 us.)
        if (c.split && o + 1 == c.split) {
            put(NM_FO_RECORD, NM_FS_SIDE, 0, 0, 0, NM_FE_DET);
            if (tail) {
                // with the tail the side stream has nothing left to detect: the octaves < T are described right there (one
                // stream hand-over less on the path base blur -> ... -> descriptors), beside the tail on the caller's
                put(NM_FO_DESCRIBE, NM_FS_SIDE, 0, 0, c.split, NM_FE_NONE);
            } else {
                put(NM_FO_WAIT, NM_FS_DESC, 0, 0, 0, NM_FE_DET);
                put(NM_FO_DESCRIBE, NM_FS_DESC, 0, 0, c.split, NM_FE_NONE);
            }
        }
    }
    if (tail) {
        // The tail's book-keeping scans + gathers continue octave T - 1's book (ev_det: recorded on the side stream behind that
        // octave's detection, long reached by now) and stay on the CALLER's stream, straight behind the tail launch -- an event
        // hand-over to another stream costs ~10 us at the end of the chain -- as does the description of the tail octaves' few
        // keypoints.
        put(NM_FO_WAIT, NM_FS_CALLER, 0, 0, 0, NM_FE_DET);
        put(NM_FO_TAIL_SCAN, NM_FS_CALLER, T, 0, 0, NM_FE_NONE);
        put(NM_FO_DESCRIBE, NM_FS_CALLER, 0, c.split, O, NM_FE_NONE);
    } else {
        put(NM_FO_DESCRIBE, NM_FS_SIDE, 0, c.split, O, NM_FE_NONE);
    }
    // Both helper streams join the CALLER's stream directly. Joining the description stream into the side stream it was forked
    // from -- an equivalent DAG -- makes this ROCm's stream capture segfault (tools/capture_shapes.py: fork s2 -> s3, join
    // s3 -> s2 -> s1 crashes, s3 -> s1 and s2 -> s1 works).
    if (forked[NM_FS_DESC]) put(NM_FO_JOIN, NM_FS_DESC, 0, 0, 0, NM_FE_DESC);
    if (forked[NM_FS_SIDE]) put(NM_FO_JOIN, NM_FS_SIDE, 0, 0, 0, NM_FE_JOIN);
    return k;
}
static_assert(NM_FRAME_PLAN_MAX_OPS >= 1 + 7 * 20 + 3 + 3 + 2, "the plan of 20 octaves in the cross order must fit");

// Kernel launches of a plan (what nm_sift_arena_launches_per_call reports).
inline int nm_frame_plan_launches(const NmFrameOp *ops, int n_ops)
{
    int n = 0;
    for (int k = 0; k < n_ops; ++k) {
        const NmFrameOp &p = ops[k];
        n += p.kind == NM_FO_LEVELS ? p.hi - p.lo + 1 : p.kind == NM_FO_DETECT ? 3 : p.kind == NM_FO_DESCRIBE ? 2
             : (p.kind == NM_FO_BASE_BLUR || p.kind == NM_FO_TAIL || p.kind == NM_FO_TAIL_SCAN) ? 1 : 0;
    }
    return n;
}
