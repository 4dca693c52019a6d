"""The helper streams and events of a detect/describe call belong to the CALLER's stream (the per-device pool of
niftymatch_amd/csrc/nm_arena.hip), not to the call's first arena: calls on one stream share a set and are ordered by that stream
and by the joins every plan ends with, calls on different streams get different sets, no set dies with an arena, and a call that
is captured takes a set made beforehand. None of it may change a result: everything a call leaves behind must equal, bit for
bit, what a plain-order call followed by a device synchronisation leaves, and the oracle's keypoints and descriptors."""
import numpy as np
import pytest

import helpers as H
from test_gpu_frame_cross import _fetch, _poison, _same, _snapshot, _wipe
from test_gpu_stages import _t

pytestmark = pytest.mark.gpu

CAP = 4096
GEOMETRIES = [(256, 192), (135, 67)]        # three octaves; odd extents, where every decimation drops a column and a row
CALLS = [3, 1]                              # per-octave launches; the octave tail where the geometry has one

_cache = {}


def _inputs(oracle, cuda, w, h):
    """Eight frames of the geometry on the device and the oracle's results for them: computed once, never changed."""
    if (w, h) not in _cache:
        host = [H.blurred_frame(700 + i, w, h) for i in range(8)]
        _cache[(w, h)] = ([_t(f, cuda) for f in host], [oracle.sift_detect_describe(f, CAP) for f in host])
    return _cache[(w, h)]


def _call(nm, arenas, frames):
    """A call on the current stream behind a poisoning of the planes it writes (the padding behind an odd-sized gradient plane
    is never written: poisoned, it compares equal between arenas)."""
    _poison(nm, arenas)
    nm.detect_describe_batch(arenas, frames)


def _plain(nm, arenas, frames):
    """What a call in order 0 on the default stream leaves, the device synchronised before and after."""
    import torch
    torch.cuda.synchronize()
    nm.set_frame_skew(0)
    try:
        _wipe(arenas)
        _call(nm, arenas, frames)
        return _fetch(_snapshot(nm, arenas))
    finally:
        nm.set_frame_skew(-1)


def _against_oracle(res, refs, what):
    for f, (r, ref) in enumerate(zip(res, refs)):
        assert r[0] == ref["n"], "%s: frame %d has %d keypoints, the oracle %d" % (what, f, r[0], ref["n"])
        assert np.array_equal(r[1], np.ascontiguousarray(ref["kpts"]).view(np.uint32)), "%s: keypoints of frame %d against the oracle" % (what, f)
        assert np.array_equal(r[3], np.ascontiguousarray(ref["desc"]).view(np.uint32)), "%s: descriptors of frame %d against the oracle" % (what, f)


@pytest.mark.parametrize("n", CALLS)
@pytest.mark.parametrize("w,h", GEOMETRIES)
def test_calls_back_to_back_and_on_two_streams(nm, oracle, cuda, w, h, n):
    import torch
    frames, refs = _inputs(oracle, cuda, w, h)
    fa, fb = frames[:n], frames[n:2 * n]
    xs = [nm.SiftArena(w, h, CAP) for _ in range(n)]
    ys = [nm.SiftArena(w, h, CAP) for _ in range(n)]
    want_a, want_b = _plain(nm, xs, fa), _plain(nm, xs, fb)
    _against_oracle(want_a, refs[:n], "plain call, frames a")
    _against_oracle(want_b, refs[n:2 * n], "plain call, frames b")
    assert sum(r[0] for r in want_a) > 0 and any(a[0] != b[0] for a, b in zip(want_a, want_b))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    _wipe(xs); _wipe(ys)
    torch.cuda.synchronize()
    # two calls on one stream with nothing but device copies between them: the second call's base blur overwrites planes the
    # first call's helper streams read
    with torch.cuda.stream(s1):
        _call(nm, xs, fa)
        first = _snapshot(nm, xs)
        _call(nm, xs, fb)
        second = _snapshot(nm, xs)
        nm.detect_describe_batch(xs, fa)
        nm.detect_describe_batch(xs, fb)
        third = _snapshot(nm, xs)
    _same(_fetch(first), want_a, "first call on the stream")
    _same(_fetch(second), want_b, "second call on the stream")
    _same(_fetch(third), want_b, "second call straight behind the first")
    # two calls on two caller streams, in flight together, twice (the second round reuses each stream's set)
    _wipe(xs); _wipe(ys)
    torch.cuda.synchronize()
    for rep in range(2):
        with torch.cuda.stream(s1):
            _call(nm, xs, fa)
            on1 = _snapshot(nm, xs)
        with torch.cuda.stream(s2):
            _call(nm, ys, fb)
            on2 = _snapshot(nm, ys)
    _same(_fetch(on1), want_a, "call on the first of two streams")
    _same(_fetch(on2), want_b, "call on the second of two streams")


@pytest.mark.parametrize("n", CALLS)
@pytest.mark.parametrize("w,h", GEOMETRIES)
def test_no_helper_stream_dies_with_an_arena(nm, oracle, cuda, w, h, n):
    import torch
    frames, refs = _inputs(oracle, cuda, w, h)
    arenas = [nm.SiftArena(w, h, CAP) for _ in range(8)]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        nm.detect_describe_batch(arenas[:n], frames[:n])         # arenas[0] is the first arena of the stream's first call
        arenas[0].close()
        groups = [list(range(k, k + n)) for k in range(1, 8 - n + 1, n)]
        assert len(groups) >= 2
        snaps = []
        for g in groups:
            _wipe([arenas[i] for i in g])
            nm.detect_describe_batch([arenas[i] for i in g], [frames[i] for i in g])
            snaps.append(_snapshot(nm, [arenas[i] for i in g]))
    for g, snap in zip(groups, snaps):
        _against_oracle(_fetch(snap), [refs[i] for i in g], "call on the arenas %r after the first arena was destroyed" % g)
    for a in arenas[1:]:
        a.close()
    # and once more on new arenas, after every arena the stream's set has served is gone
    fresh = [nm.SiftArena(w, h, CAP) for _ in range(n)]
    with torch.cuda.stream(s):
        nm.detect_describe_batch(fresh, frames[:n])
        snap = _snapshot(nm, fresh)
    _against_oracle(_fetch(snap), refs[:n], "call on new arenas")


@pytest.mark.parametrize("w,h", GEOMETRIES)
def test_captured_four_frame_call_equals_the_eager_calls(nm, oracle, cuda, w, h):
    """The capture runs on a stream that has not issued a call: its set is one the pool made beforehand."""
    import torch
    n = 4
    frames, refs = _inputs(oracle, cuda, w, h)
    arenas = [nm.SiftArena(w, h, CAP) for _ in range(n)]
    want = {"a": _plain(nm, arenas, frames[:n]), "b": _plain(nm, arenas, frames[n:2 * n])}
    _against_oracle(want["a"], refs[:n], "eager 4-frame call")
    assert any(a[0] != b[0] for a, b in zip(want["a"], want["b"]))
    d = [f.clone() for f in frames[:n]]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        nm.detect_describe_batch(arenas, d)
    for key, src in (("a", frames[:n]), ("b", frames[n:2 * n]), ("b", frames[n:2 * n])):
        for x, f in zip(d, src):
            x.copy_(f)
        _wipe(arenas)
        g.replay()
        torch.cuda.synchronize()
        _same(_fetch(_snapshot(nm, arenas)), want[key], "captured 4-frame call replayed on the frames %s" % key)
    # the stream the capture ran on goes on to issue eager calls
    _wipe(arenas)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        _call(nm, arenas, frames[:n])
        snap = _snapshot(nm, arenas)
    _same(_fetch(snap), want["a"], "eager call on the stream of the capture")


@pytest.mark.parametrize("w,h", GEOMETRIES)
def test_orders_0_and_2_give_the_same_three_frame_call(nm, oracle, cuda, w, h):
    import torch
    n = 3
    frames, refs = _inputs(oracle, cuda, w, h)
    arenas = [nm.SiftArena(w, h, CAP) for _ in range(n)]
    want = _plain(nm, arenas, frames[:n])
    _against_oracle(want, refs[:n], "order 0")
    s = torch.cuda.Stream()
    try:
        for order in (2, 0, 2):
            nm.set_frame_skew(order)
            _wipe(arenas)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                _call(nm, arenas, frames[:n])
                snap = _snapshot(nm, arenas)
            _same(_fetch(snap), want, "order %d through nm_sift_set_frame_skew" % order)
    finally:
        nm.set_frame_skew(-1)
