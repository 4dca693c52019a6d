"""The issue order of a many-frame detect/describe call (nm_sift_set_frame_skew, csrc/nm_frame.hip) changes WHERE the launches
of the per-octave path are issued -- levels 4-5 of an octave beside the next octaves' levels 1-3 -- and nothing else: the same
launches, so counts, keypoints, orientations and descriptors must be identical, bit for bit, in every order; eagerly and
through a captured graph."""
import numpy as np
import pytest

ORDERS = (0, 1)


def _frames(nm, dev, seeds, w, h):
    """Noise frames with the Gaussian pre-blur of the synthetic workload, made on the device (any width: nm.convolve)."""
    import torch
    from niftymatch_amd import synth
    taps, r = nm.create_kernel_for_sigma(synth.preblur_sigma(w, h))
    taps_d = torch.from_numpy(taps).to(dev)
    out = [nm.convolve(synth.noise_frame_torch(s, w, h, dev), taps_d, r) for s in seeds]
    torch.cuda.synchronize()
    return out


def _wipe(arenas):
    for a in arenas:
        a.desc.zero_(); a.kpts.zero_(); a.orients.zero_(); a.x.zero_(); a.y.zero_(); a.num_items.zero_()


def _results(arenas):
    import torch
    torch.cuda.synchronize()
    out = []
    for a in arenas:
        n = int(a.num_items.item())
        out.append((n, a.kpts[:n].cpu().numpy(), a.orients[:n].cpu().numpy(), a.desc[:n].cpu().numpy(),
                    a.x[:n].cpu().numpy(), a.y[:n].cpu().numpy()))
    return out


def _same(got, want, what):
    assert len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], "%s: frame %d has %d keypoints, the plain order %d" % (what, f, g[0], w[0])
        for name, x, y in zip(("keypoints", "orientations", "descriptors", "x", "y"), g[1:], w[1:]):
            assert np.array_equal(x, y), "%s: %s of frame %d differ" % (what, name, f)


def _compare_orders(nm, cuda, n, w, h, cap, seed0):
    frames = _frames(nm, cuda, range(seed0, seed0 + n), w, h)
    arenas = [nm.SiftArena(w, h, cap) for _ in range(n)]
    launches = nm.lib().nm_sift_arena_launches_per_call(arenas[0]._h, n)
    assert launches > 3 and (launches - 3) % 8 == 0, "the call must take the per-octave launches (1 + 8 per octave + 2)"
    res = {}
    try:
        for order in ORDERS + (0,):                  # the plain order once more at the end: the switch goes both ways
            nm.set_frame_skew(order)
            assert nm.lib().nm_sift_arena_launches_per_call(arenas[0]._h, n) == launches
            for rep in range(2):                     # back to back: the second call's chain runs into the first one's joins
                _wipe(arenas)
                nm.detect_describe_batch(arenas, frames)
            got = _results(arenas)
            if order in res:
                _same(got, res[order], "order %d, second visit" % order)
            res[order] = got
    finally:
        nm.set_frame_skew(-1)
    assert sum(r[0] for r in res[0]) > 0
    assert all(0 < r[0] < cap for r in res[0]), "the lists must neither be empty nor cut at the capacity"
    for order in ORDERS[1:]:
        _same(res[order], res[0], "%d frames %d x %d, order %d" % (n, w, h, order))
    return res[0]


@pytest.mark.gpu
def test_orders_agree_on_a_64_frame_1080p_call(nm, cuda):
    res = _compare_orders(nm, cuda, 64, 1920, 1080, 16384, 0)
    assert min(r[0] for r in res) > 4000


@pytest.mark.gpu
@pytest.mark.parametrize("n,w,h", [(3, 640, 480),        # one frame more than the octave tail serves
                                   (5, 1000, 562),       # width a multiple of 4, not of 16; height of neither
                                   (4, 333, 251)])       # odd width: the launches go frame by frame, decimation on its own
def test_orders_agree_above_the_tail_limit_and_on_odd_geometry(nm, cuda, n, w, h):
    _compare_orders(nm, cuda, n, w, h, 8192, 500)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS[1:])
def test_skewed_32_frame_call_replays_from_a_graph_on_other_frames(nm, cuda, order):
    import torch
    w, h, cap, n = 320, 240, 4096, 32
    first = _frames(nm, cuda, range(700, 700 + n), w, h)
    other = _frames(nm, cuda, range(800, 800 + n), w, h)
    arenas = [nm.SiftArena(w, h, cap) for _ in range(n)]
    d = [f.clone() for f in first]
    s = torch.cuda.Stream()
    try:
        want = {}
        nm.set_frame_skew(0)
        for key, src in (("first", first), ("other", other)):
            _wipe(arenas)
            with torch.cuda.stream(s):
                nm.detect_describe_batch(arenas, src)
            want[key] = _results(arenas)
        assert any(a[0] != b[0] for a, b in zip(want["first"], want["other"]))
        nm.set_frame_skew(order)
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
            _same(_results(arenas), want[key], "graph of order %d replayed on the %s frames" % (order, key))
    finally:
        nm.set_frame_skew(-1)


def test_setter_returns_the_previous_order_and_restores_the_default(nm):
    default = nm.set_frame_skew(-1)
    assert default in ORDERS
    try:
        assert nm.set_frame_skew(1) == default
        assert nm.set_frame_skew(0) == 1
        assert nm.set_frame_skew(7) == 0             # out of range: the default again
        assert nm.set_frame_skew(-1) == default
    finally:
        nm.set_frame_skew(-1)
