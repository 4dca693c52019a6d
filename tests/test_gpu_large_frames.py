"""GPU parity of detect/describe beyond 1080p, on structured content and at the capacity edges, bit for bit against the oracle.

Every other frame test stops at 1920 x 1080 and nearly all use blurred noise, which leaves a handful of keypoints in the deep
octaves. Here: 3840 x 2160 (7 octaves; the octave tail, csrc/nm_tail.hip, covers octaves 2..6 from a 960 x 540 plane),
7680 x 4320 (8 octaves, ~200 k keypoints, the largest staging offsets; the tail from octave 3 on request), a width that is not
a multiple of 4 at a large size, and long thin frames; contents: blurred noise, helpers.blob_field (keypoints in every octave),
helpers.step_field (exact ties, zero gradients, dense level 0). Paths: one- and two-frame calls take the tail, calls of 3 or more
frames the per-octave launches. Each oracle result is computed once per module."""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers as H
from test_gpu_stages import _eq, _t
from test_gpu_tail import _arena

pytestmark = pytest.mark.gpu

W4K, H4K = 3840, 2160
W8K, H8K = 7680, 4320
CAP4K, CAP8K = 65536, 262144


@functools.lru_cache(maxsize=None)
def _frame(kind, w, h):
    if kind == "noise":
        return H.blurred_frame(0, w, h)
    if kind == "noise_1e-4":
        return (H.blurred_frame(0, w, h) * np.float32(1e-4)).astype(np.float32)
    return (H.blob_field if kind == "blobs" else H.step_field)(0, w, h)


@functools.lru_cache(maxsize=None)
def _ref(kind, w, h, cap):
    import oracle_lib as O
    return O.sift_detect_describe(_frame(kind, w, h), cap)


def _tail_planned(nm, w, h):
    return nm.lib().nm_sift_tail_plan(w, h, 2, None, 0, None) > 0


def _out(a):
    """(n, [kpts, orients, x, y, desc] as uint32 views) of an arena; the tail's status word must read 0 after every call (a
    wait that hits its spin limit drops the octaves >= T without any other sign)."""
    assert a.tail_status() == 0, "octave-tail launch timed out"
    n = int(a.num_items.item())
    return n, [t[:n].cpu().numpy().view(np.uint32).copy() for t in (a.kpts, a.orients, a.x, a.y, a.desc)]


def _same_as_oracle(out, ref, what):
    n, (kpts, ori, x, y, desc) = out
    assert n == ref["n"], (what, n, ref["n"])
    for got, key in ((kpts, "kpts"), (ori, "orient"), (x, "x"), (y, "y"), (desc, "desc")):
        _eq(got, ref[key].view(np.uint32), "%s: %s" % (what, key))


def _same(o0, o1, what):
    assert o0[0] == o1[0], (what, o0[0], o1[0])
    for k, (a, b) in enumerate(zip(o0[1], o1[1])):
        _eq(a, b, "%s: output %d" % (what, k))


def _single(nm, cuda, kind, w, h, cap, tail=None):
    a = _arena(nm, cuda, w, h, tail, cap)
    try:
        segs = nm.lib().nm_sift_arena_tail_segments(a._h)
        if tail is None:
            assert (segs > 0) == _tail_planned(nm, w, h), (w, h)
        else:
            assert (segs > 0) == (tail > 0), (w, h, tail)
        a.detect_describe(_t(_frame(kind, w, h), cuda))
        return _out(a)
    finally:
        a.close()


# ---- single-frame driver -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["noise", "blobs", "steps"])
def test_4k_single_frame_tail_against_oracle_and_per_octave(nm, oracle, cuda, kind):
    """3840 x 2160, one-frame call: octaves 0-1 per octave, 2-6 in the tail (first tail plane 960 x 540); against the oracle
    and against an NM_FRAME_TAIL=0 arena (per-octave launches for every octave), bit for bit."""
    assert _tail_planned(nm, W4K, H4K)
    ref = _ref(kind, W4K, H4K, CAP4K)
    assert ref["n"] < CAP4K and ref["counts"].shape[0] == 7
    got = _single(nm, cuda, kind, W4K, H4K, CAP4K)
    _same_as_oracle(got, ref, "4K %s, tail" % kind)
    _same(got, _single(nm, cuda, kind, W4K, H4K, CAP4K, tail=0), "4K %s, tail against per-octave launches" % kind)


def test_8k_noise_single_frame_per_octave_and_tail_from_octave_3(nm, oracle, cuda):
    """7680 x 4320 blurred noise, capacity 262144: 8 octaves, ~200 k keypoints; the level-0 detection staging is ~1.65 GB, the
    closest any byte offset comes to 2^31. The host plan refuses a tail from octave 2 here (the tail's scan would need more than
    60 KB of LDS), so a default arena takes the per-octave launches for all 8 octaves; an NM_FRAME_TAIL=3 arena runs octaves
    3..7 in the tail (first tail plane 960 x 540). Both against the oracle, bit for bit."""
    assert not _tail_planned(nm, W8K, H8K) and nm.lib().nm_sift_tail_plan(W8K, H8K, 3, None, 0, None) > 0
    ref = _ref("noise", W8K, H8K, CAP8K)
    assert ref["counts"].shape[0] == 8 and 150000 < ref["n"] < CAP8K
    got = _single(nm, cuda, "noise", W8K, H8K, CAP8K)
    _same_as_oracle(got, ref, "8K noise, per-octave launches")
    _same(_single(nm, cuda, "noise", W8K, H8K, CAP8K, tail=3), got, "8K noise, tail from octave 3 against per-octave launches")


@pytest.mark.parametrize("kind,wh,cap", [("noise", (2047, 1531), 32768), ("blobs", (4096, 130), 16384),
                                         ("blobs", (129, 2000), 16384)],
                         ids=["noise-2047x1531-generic-width", "blobs-4096x130", "blobs-129x2000"])
def test_odd_large_geometries_single_frame(nm, oracle, cuda, kind, wh, cap):
    """A width that is not a multiple of 4 (the generic, unpacked kernels) at 3 Mpixel, and long thin frames whose octaves
    shrink to a few rows or columns; the tail wherever the host plan takes it (test_tail_plan.py)."""
    w, h = wh
    ref = _ref(kind, w, h, cap)
    assert 0 < ref["n"] < cap
    _same_as_oracle(_single(nm, cuda, kind, w, h, cap), ref, "%s %dx%d" % (kind, w, h))


# ---- batched calls -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", [("blobs", "noise_1e-4"), ("noise", "blobs", "steps", "noise_1e-4")],
                         ids=["2-frames-tail", "4-frames-per-octave"])
def test_4k_batch_mixed_content_with_tall_and_default_detection_groups(nm, oracle, cuda, kinds):
    """detect_describe_batch at 3840 x 2160: two frames share one tail launch; four frames take the per-octave launches over
    all 7 octaves. Every frame against the oracle, once with 20-row detection groups forced and once with the default choice --
    the same bits both times."""
    n = len(kinds)
    outs = {}
    for tall_min in (1, -1):
        prev = nm.set_detect_tall_min(tall_min)
        arenas = []
        try:
            arenas = [nm.SiftArena(W4K, H4K, CAP4K, device=cuda) for _ in range(n)]
            if n <= 2:
                assert nm.lib().nm_sift_arena_tail_segments(arenas[0]._h) > 0
            assert nm.lib().nm_sift_arena_launches_per_call(arenas[0]._h, n) != nm.lib().nm_sift_arena_launches_per_call(
                arenas[0]._h, 4 if n <= 2 else 2)
            nm.detect_describe_batch(arenas, [_t(_frame(k, W4K, H4K), cuda) for k in kinds])
            outs[tall_min] = [_out(a) for a in arenas]
        finally:
            nm.set_detect_tall_min(prev)
            for a in arenas:
                a.close()
    nm.set_detect_tall_min(-1)
    for i, k in enumerate(kinds):
        _same(outs[1][i], outs[-1][i], "4K batch of %d, frame %d (%s): 20-row against default groups" % (n, i, k))
        _same_as_oracle(outs[-1][i], _ref(k, W4K, H4K, CAP4K), "4K batch of %d, frame %d (%s)" % (n, i, k))


# ---- capacity edges (siftfunctions.cu:165-169) --------------------------------------------------------------------------
def _caps():
    full = _ref("steps", W4K, H4K, CAP4K)
    cnt = full["counts"]
    per_oct = cnt.sum(1)
    assert cnt[0][0] > 5000 and cnt[3][0] > 2
    in_tail = int(per_oct[:3].sum() + cnt[3][0] // 2)          # inside level 0 of octave 3, a tail octave
    return {"oct0-level0": 5000, "tail-oct3": in_tail, "full": full["n"], "full-minus-1": full["n"] - 1}


@pytest.mark.parametrize("where", ["oct0-level0", "tail-oct3", "full", "full-minus-1"])
def test_4k_steps_capacity_edges(nm, oracle, cuda, where):
    """3840 x 2160 step field, one-frame call (tail), capacity cut inside level 0 of octave 0, inside a tail octave, at exactly
    the full count and one below it: the oracle's clipped result, which is a prefix of the unclipped one."""
    cap = _caps()[where]
    full = _ref("steps", W4K, H4K, CAP4K)
    ref = _ref("steps", W4K, H4K, cap)
    assert ref["n"] == cap
    for key in ("kpts", "orient", "x", "y", "desc"):
        _eq(ref[key], full[key][:cap], "oracle prefix property, %s, capacity %d" % (key, cap))
    _same_as_oracle(_single(nm, cuda, "steps", W4K, H4K, cap), ref, "4K steps, capacity %d (%s)" % (cap, where))


# ---- the C++ API client loop at 4K ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["blobs", "steps"])
def test_4k_cpp_api_client_loop(nm, oracle, cuda, kind):
    """The reference-style per-octave client (SiftParams / PyramidData / SiftData + compute_*) at 3840 x 2160."""
    frame = _frame(kind, W4K, H4K)
    ref = _ref(kind, W4K, H4K, CAP4K)
    desc = np.zeros((CAP4K, 128), np.float32)
    x = np.zeros(CAP4K, np.float32)
    y = np.zeros(CAP4K, np.float32)
    n = nm.lib().nm_client_detect_describe(frame.ctypes.data, W4K, H4K, CAP4K, desc.ctypes.data, x.ctypes.data, y.ctypes.data)
    assert n == ref["n"] and n > 2000
    _eq(desc[:n], ref["desc"], "C++ API descriptors, 4K %s" % kind)
    _eq(x[:n], ref["x"], "x")
    _eq(y[:n], ref["y"], "y")


@pytest.mark.parametrize("kind", ["blobs", "steps"])
def test_4k_lazy_counts_show_the_reference_observable_state(nm, oracle, cuda, kind):
    """nm_client_lazy_counts at 3840 x 2160 (7 octaves): the sizes a curious client reads are the oracle's accepted counts and
    the running item count their clipped running sum; the looking, the never-looking and the eager client agree."""
    f = np.ascontiguousarray(_frame(kind, W4K, H4K))
    cap = CAP4K
    ref = _ref(kind, W4K, H4K, cap)
    n_oct = ref["counts"].shape[0]
    watch = (C.c_int * (4 * n_oct))()
    pending = C.c_int(0)
    n = nm.lib().nm_client_lazy_counts(f.ctypes.data, W4K, H4K, cap, watch, n_oct, C.byref(pending))
    assert n == ref["n"]
    assert pending.value >= 4 * n_oct, "the lazy path was not taken"
    run = 0
    for o in range(n_oct):
        cnt = [int(c) for c in ref["counts"][o]]
        for l in range(3):
            assert watch[4 * o + l] == cnt[l], (o, l)
        run = min(cap, run + sum(cnt))
        assert watch[4 * o + 3] == run, o
