"""The cross issue order of a many-frame detect/describe call (nm_sift_set_frame_skew(2), csrc/nm_frame.hip) puts levels 4-5 of every
octave on a third stream, beside the next octave's levels 1-3 on the caller's stream and the previous octave's detection on the
side stream. It changes where launches are issued and nothing else, so everything a call leaves behind -- counts, keypoints,
orientations, descriptors, octave 0's six levels and the gradient planes of all octaves -- must equal the plain order's bit for
bit: eagerly, call after call on the same arenas without a host synchronisation, and through a captured graph."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

W, H, CAP = 256, 192, 4096       # three octaves (levels 4-5 of octave 0 and 1 run beside another octave's levels), tail-capable


def _frames(nm, dev, seeds, w, h):
    """Noise frames with the Gaussian pre-blur of the synthetic workload, made on the device (any width: nm.convolve)."""
    import torch
    from niftymatch_amd import synth
    taps, r = nm.create_kernel_for_sigma(synth.preblur_sigma(w, h))
    taps_d = torch.from_numpy(taps).to(dev)
    out = [nm.convolve(synth.noise_frame_torch(s, w, h, dev), taps_d, r) for s in seeds]
    torch.cuda.synchronize()
    return out


def _octaves(nm, arena):
    return (nm.lib().nm_sift_arena_launches_per_call(arena._h, 64) - 3) // 8      # 64 frames: 1 + 8 per octave + 2


_hip = None


def _copy_async(dst, src_ptr, count):
    """count floats of arena memory into the tensor dst, on the current stream (no host synchronisation)."""
    import torch
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so")
        _hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    assert _hip.hipMemcpyAsync(dst.data_ptr(), src_ptr, count * 4, 3, torch.cuda.current_stream().cuda_stream) == 0


def _snapshot(nm, arenas):
    """Device copies of everything the arenas hold after a call, enqueued on the current stream behind that call."""
    import torch
    snap = []
    for a in arenas:
        w, h = a.width, a.height
        n_grad = sum((6 * (w >> o) * (h >> o) + 3) & ~3 for o in range(_octaves(nm, a)))
        planes = torch.empty(6 * w * h + n_grad, dtype=torch.float32, device=a.device)
        for l in range(6):
            _copy_async(planes[l * w * h:], a.level_ptr(l), w * h)
        _copy_async(planes[6 * w * h:], a.grad_ptr(), n_grad)
        snap.append((a.num_items.clone(), a.kpts.clone(), a.orients.clone(), a.desc.clone(), a.x.clone(), a.y.clone(), planes))
    return snap


NAMES = ("keypoints", "orientations", "descriptors", "x", "y", "levels and gradient planes")


def _fetch(snap):
    import torch
    torch.cuda.synchronize()
    out = []
    for s in snap:
        n = int(s[0].item())
        # compared as bit patterns: equal means equal bits (a NaN equals itself, +0 does not equal -0)
        out.append((n,) + tuple(t[:n].cpu().numpy().view(np.uint32) for t in s[1:6]) + (s[6].cpu().numpy().view(np.uint32),))
    return out


def _same(got, want, what):
    assert len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], "%s: frame %d has %d keypoints, the plain order %d" % (what, f, g[0], w[0])
        for name, x, y in zip(NAMES, g[1:], w[1:]):
            assert np.array_equal(x, y), "%s: %s of frame %d differ" % (what, name, f)


def _wipe(arenas):
    for a in arenas:
        a.desc.zero_(); a.kpts.zero_(); a.orients.zero_(); a.x.zero_(); a.y.zero_(); a.num_items.zero_()


def _poison(nm, arenas):
    """Octave 0's levels and every gradient plane set to 1e7 on the current stream: what a call leaves there it has written."""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    for a in arenas:
        w, h = a.width, a.height
        n_grad = sum((6 * (w >> o) * (h >> o) + 3) & ~3 for o in range(_octaves(nm, a)))
        for l in range(6):
            assert nm.lib().nm_fill_u32(a.level_ptr(l), w * h, 0x4b189680, st) == 0
        assert nm.lib().nm_fill_u32(a.grad_ptr(), n_grad, 0x4b189680, st) == 0


def _run(nm, arenas, frames, order):
    nm.set_frame_skew(order)
    _wipe(arenas)
    _poison(nm, arenas)
    nm.detect_describe_batch(arenas, frames)
    return _fetch(_snapshot(nm, arenas))


def _per_octave_launches(nm, arenas):
    n = len(arenas)
    launches = nm.lib().nm_sift_arena_launches_per_call(arenas[0]._h, n)
    assert launches == 1 + 8 * _octaves(nm, arenas[0]) + 2, "the call must take the per-octave launches"
    return launches


@pytest.mark.gpu
@pytest.mark.parametrize("n,w,h", [(3, W, H),           # one frame more than the octave tail serves; three octaves
                                   (4, 135, 67),        # odd extents: decimation drops a column and a row
                                   (4, 60, 33)])        # levels 4-5 of the last octave are a few hundred pixels
def test_cross_order_equals_the_plain_order(nm, cuda, n, w, h):
    frames = _frames(nm, cuda, range(900, 900 + n), w, h)
    arenas = [nm.SiftArena(w, h, CAP) for _ in range(n)]
    _per_octave_launches(nm, arenas)
    try:
        plain = _run(nm, arenas, frames, 0)
        cross = _run(nm, arenas, frames, 2)
    finally:
        nm.set_frame_skew(-1)
    # (a 60 x 33 noise frame holds 0-2 keypoints: there the levels and gradient planes carry the comparison)
    assert (sum(r[0] for r in plain) > 0 or w < 100) and all(r[0] < CAP for r in plain)
    _same(cross, plain, "%d frames %d x %d, cross order" % (n, w, h))


@pytest.mark.gpu
def test_two_calls_back_to_back_on_the_same_arenas(nm, cuda):
    """The second call's base blur and levels overwrite planes that the first call's third-stream and side-stream launches read:
    nothing but the joins at the end of the first call orders them."""
    n = 3
    first = _frames(nm, cuda, range(910, 910 + n), W, H)
    other = _frames(nm, cuda, range(920, 920 + n), W, H)
    arenas = [nm.SiftArena(W, H, CAP) for _ in range(n)]
    _per_octave_launches(nm, arenas)
    res = {}
    try:
        for order in (0, 2):
            nm.set_frame_skew(order)
            _wipe(arenas)
            nm.detect_describe_batch(arenas, first)
            s1 = _snapshot(nm, arenas)                   # device copies on the same stream: the host does not wait
            nm.detect_describe_batch(arenas, other)
            s2 = _snapshot(nm, arenas)
            nm.detect_describe_batch(arenas, first)      # and with nothing at all between two calls
            nm.detect_describe_batch(arenas, other)
            s3 = _snapshot(nm, arenas)
            res[order] = [_fetch(s) for s in (s1, s2, s3)]
    finally:
        nm.set_frame_skew(-1)
    assert any(a[0] != b[0] for a, b in zip(res[0][0], res[0][1])), "the two sets of frames must differ in their results"
    for k, what in enumerate(("first call", "second call", "second call straight behind the first")):
        _same(res[2][k], res[0][k], what)
    _same(res[0][2], res[0][1], "plain order, second call straight behind the first")


@pytest.mark.gpu
def test_the_switch_holds_no_state(nm, cuda):
    n = 3
    frames = _frames(nm, cuda, range(930, 930 + n), W, H)
    arenas = [nm.SiftArena(W, H, CAP) for _ in range(n)]
    _per_octave_launches(nm, arenas)
    try:
        want = _run(nm, arenas, frames, 0)
        for step, order in enumerate((2, 1, 2)):
            _same(_run(nm, arenas, frames, order), want, "step %d of 0 -> 2 -> 1 -> 2 (order %d)" % (step + 1, order))
    finally:
        nm.set_frame_skew(-1)
    assert sum(r[0] for r in want) > 0


@pytest.mark.gpu
def test_cross_call_replays_from_a_graph_on_other_frames(nm, cuda):
    import torch
    n = 4
    first = _frames(nm, cuda, range(940, 940 + n), W, H)
    other = _frames(nm, cuda, range(950, 950 + n), W, H)
    arenas = [nm.SiftArena(W, H, CAP) for _ in range(n)]
    _per_octave_launches(nm, arenas)
    d = [f.clone() for f in first]
    s = torch.cuda.Stream()
    try:
        want = {}
        nm.set_frame_skew(0)
        for key, src in (("first", first), ("other", other)):
            _wipe(arenas)
            torch.cuda.synchronize()                 # the wipe ran on the default stream
            with torch.cuda.stream(s):
                nm.detect_describe_batch(arenas, src)
            torch.cuda.synchronize()
            want[key] = _fetch(_snapshot(nm, arenas))
        assert any(a[0] != b[0] for a, b in zip(want["first"], want["other"]))
        nm.set_frame_skew(2)
        with torch.cuda.stream(s):
            nm.detect_describe_batch(arenas, d)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            nm.detect_describe_batch(arenas, d)
        nm.set_frame_skew(0)                         # the order is part of the captured graph, not of the replay
        for key, src in (("first", first), ("other", other), ("first", first)):
            for x, f in zip(d, src):
                x.copy_(f)
            _wipe(arenas)
            g.replay()
            torch.cuda.synchronize()
            _same(_fetch(_snapshot(nm, arenas)), want[key], "graph of the cross order replayed on the %s frames" % key)
    finally:
        nm.set_frame_skew(-1)


@pytest.mark.gpu
def test_launch_count_does_not_depend_on_the_order(nm, cuda):
    arena = nm.SiftArena(W, H, CAP)
    try:
        for n in (1, 3, 64):
            counts = []
            for order in (0, 1, 2):
                nm.set_frame_skew(order)
                counts.append(nm.lib().nm_sift_arena_launches_per_call(arena._h, n))
            assert counts[0] > 0 and counts[0] == counts[1] == counts[2], (n, counts)
    finally:
        nm.set_frame_skew(-1)


@pytest.mark.gpu
def test_a_tail_call_ignores_the_order(nm, cuda):
    n = 2
    frames = _frames(nm, cuda, range(960, 960 + n), W, H)
    arenas = [nm.SiftArena(W, H, CAP) for _ in range(n)]
    assert nm.lib().nm_sift_arena_launches_per_call(arenas[0]._h, n) != 1 + 8 * _octaves(nm, arenas[0]) + 2, \
        "a 2-frame call of this size must take the octave tail"
    try:
        plain = _run(nm, arenas, frames, 0)
        cross = _run(nm, arenas, frames, 2)
    finally:
        nm.set_frame_skew(-1)
    assert sum(r[0] for r in plain) > 0
    _same(cross, plain, "2-frame call (octave tail), cross order selected")


_SPLIT_CHILD = r"""
import hashlib, json, sys
sys.path[:0] = [%r, %r]
import torch
import niftymatch_amd as nm
import test_gpu_frame_cross as T
dev = torch.device("cuda:0")
frames = T._frames(nm, dev, range(970, 973), T.W, T.H)
arenas = [nm.SiftArena(T.W, T.H, T.CAP) for _ in frames]
out = {}
for order in (0, 2):
    res = T._run(nm, arenas, frames, order)
    h = hashlib.sha256()
    for r in res:
        h.update(str(r[0]).encode())
        for x in r[1:]:
            h.update(x.tobytes())
    out[str(order)] = [h.hexdigest(), sum(r[0] for r in res)]
nm.set_frame_skew(-1)
print(json.dumps(out))
"""


def _digest(res):
    import hashlib
    h = hashlib.sha256()
    for r in res:
        h.update(str(r[0]).encode())
        for x in r[1:]:
            h.update(x.tobytes())
    return [h.hexdigest(), sum(r[0] for r in res)]


@pytest.mark.gpu
def test_a_split_describe_call_ignores_the_order(nm, cuda):
    """NM_FRAME_SPLIT_DESCRIBE is read once per process, so the split-describe calls run in a child: with the cross order selected
    they give what they give in order 0, which is what this process's plain call gives on the same frames."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, NM_FRAME_SPLIT_DESCRIBE="2")
    env.pop("NM_FRAME_SKEW", None)
    r = subprocess.run([sys.executable, "-c", _SPLIT_CHILD % (here, os.path.dirname(here))], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    child = json.loads(r.stdout.strip().splitlines()[-1])
    frames = _frames(nm, cuda, range(970, 973), W, H)
    arenas = [nm.SiftArena(W, H, CAP) for _ in frames]
    try:
        plain = _digest(_run(nm, arenas, frames, 0))
    finally:
        nm.set_frame_skew(-1)
    assert plain[1] > 0
    assert child["0"] == plain, "split-describe call in order 0 against the plain call"
    assert child["2"] == plain, "split-describe call with the cross order selected against the plain call"
