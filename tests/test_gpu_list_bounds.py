"""The level lists of the device-sized orientation / descriptor entries hold `max_pts` entries each, and a level count above that
is clipped (nm_abi.h; nm_detect_orientations_levels_dev, nm_compute_sift_descriptors_levels_dev). The C++ layer sizes
_orientations[l] for the strict-extremum bound nm_keypoint_bound(w, h) (test_content_strength.py pins the bound); only a client
that fills the public _key_pts itself can exceed it. Before the clip the kernels wrote orientations past the list and the
descriptor kernel read them back from there.

The ABI test allocates every list as max_pts rows PLUS a guard at least as large as the overflow, prefilled with a sentinel: a
kernel without the clip writes only into the test's own allocation and fails an assertion. The C++ test writes into memory the
library owns, where no guard can help, so it first runs the guarded case and goes on only when that passed."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
from test_gpu_stages import _eq, _t

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD          # a quiet-NaN bit pattern no kernel produces


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


class _MappedWords:
    """n ints of mapped pinned host memory (hipHostMallocMapped), what the C++ layer passes as h_counts / h_items."""

    def __init__(self, n):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
        self.hip.hipHostGetDevicePointer.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint]
        self.hip.hipHostFree.argtypes = [C.c_void_p]
        self.host = C.c_void_p()
        assert self.hip.hipHostMalloc(C.byref(self.host), 4 * n, 0x2) == 0      # hipHostMallocMapped
        self.dev = C.c_void_p()
        assert self.hip.hipHostGetDevicePointer(C.byref(self.dev), self.host, 0) == 0
        self.words = (C.c_int * n).from_address(self.host.value)
        for i in range(n):
            self.words[i] = -1

    def close(self):
        self.hip.hipHostFree(self.host)


def _octave0(oracle, w, h, seed):
    p = oracle.sift_params(w, h)
    base = oracle.convolve(H.blurred_frame(seed, w, h), *oracle.create_kernel_for_sigma(p.base_smooth))[0]
    _, dogs, grad = oracle.octave_pyramid(base, w, h)
    return p, dogs, grad


def _sentinel(cuda, shape):
    import torch
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=cuda).view(torch.float32)


def _untouched(t, what):
    bits = t.cpu().numpy().view(np.uint32)
    assert (bits == SENTINEL).all(), "%s: %d of %d guard words overwritten" % (what, (bits != SENTINEL).sum(), bits.size)


def _overflowing_levels(nm, oracle, cuda, base, capacity):
    """Device counts [400, 250, 350] with max_pts = 300 (levels 0 and 2 overflow) on a 96 x 64 octave; hand-made keypoints at
    interior pixels in raster order. base: the running item count in a device word (None: host_base = 0)."""
    import torch
    w, h, max_pts = 96, 64, 300
    counts = [400, 250, 350]
    sigmas = [2.0, 2.6, 3.3]
    p, dogs, grad = _octave0(oracle, w, h, 21)
    yy, xx = np.mgrid[6: h - 6, 6: w - 6]
    lists = []
    for l, c in enumerate(counts):
        pix = np.stack([xx.ravel(), yy.ravel()], 1)[17 * l: 17 * l + c].astype(np.float32)
        lists.append(np.concatenate([pix, np.full((c, 1), sigmas[l], np.float32), np.full((c, 1), l, np.float32)], 1))
    tk = [_t(k, cuda) for k in lists]
    tg = _t(grad, cuda)
    ori = [_sentinel(cuda, (max_pts + max(c - max_pts, 0) + 16, 2)) for c in counts]
    d_counts = torch.tensor(counts, dtype=torch.int32, device=cuda)
    rows = capacity + 64
    desc, xs, ys = _sentinel(cuda, (rows, 128)), _sentinel(cuda, (rows,)), _sentinel(cuda, (rows,))
    d_base = None if base is None else torch.tensor([base], dtype=torch.int32, device=cuda)
    d_items = torch.full((1,), -5, dtype=torch.int32, device=cuda)
    words = _MappedWords(4)
    try:
        assert nm.lib().nm_detect_orientations_levels_dev(_ptrs(tk), d_counts.data_ptr(), max_pts, tg.data_ptr(), w, h, 1.5, 1.0,
                                                          _ptrs(ori), words.dev.value, None) == 0
        assert nm.lib().nm_compute_sift_descriptors_levels_dev(
            _ptrs(tk), _ptrs(ori), d_counts.data_ptr(), max_pts, None if d_base is None else d_base.data_ptr(), 0, capacity,
            d_items.data_ptr(), words.dev.value + 12, tg.data_ptr(), w, h, 3, 1.0, desc.data_ptr(), xs.data_ptr(),
            ys.data_ptr(), None) == 0
        torch.cuda.synchronize()
        h_counts, h_items = [words.words[i] for i in range(3)], words.words[3]
    finally:
        words.close()
    kept = [min(c, max_pts) for c in counts]
    for l in range(3):
        _untouched(ori[l][kept[l]:], "orientation list %d beyond its %d entries" % (l, kept[l]))
    ref_ori = [oracle.detect_orientations(lists[l][: kept[l]], grad, w, h, 1.5, 1.0) for l in range(3)]
    for l in range(3):
        _eq(ori[l][: kept[l]], ref_ori[l], "orientations of level %d, first %d keypoints" % (l, kept[l]))
    first = 0 if base is None else base
    run, want = first, []
    for l in range(3):                                    # max_pts per level, then the capacity across levels
        n = max(0, min(kept[l], capacity - run))
        want.append(oracle.compute_sift_descriptors(lists[l][:n], ref_ori[l][:n], grad, w, h, 3, 1.0))
        run += n
    assert int(d_items.item()) == run and h_items == run, (int(d_items.item()), h_items, run)
    assert h_counts == kept, h_counts
    _untouched(desc[:first], "descriptor slots before the running count")
    _untouched(desc[run:], "descriptor slots at and after the clipped count")
    _untouched(xs[run:], "x slots after the clipped count")
    _eq(desc[first:run], np.concatenate([d for d, _, _ in want]), "descriptors, clipped at max_pts and capacity")
    _eq(xs[first:run], np.concatenate([x for _, x, _ in want]), "x")
    _eq(ys[first:run], np.concatenate([y for _, _, y in want]), "y")
    return run


@pytest.mark.parametrize("base,capacity", [(None, 4096), (7, 657), (0, 520)],
                         ids=["host-base-no-capacity-cut", "device-base-cut-in-level-2", "device-base-cut-in-level-1"])
def test_level_counts_above_max_pts_are_clipped(nm, oracle, cuda, base, capacity):
    """d_counts [400, 250, 350], max_pts 300: each list keeps its first 300 entries, whose orientations are the oracle's for
    the list prefix; the descriptors follow max_pts per level and then the capacity; *d_items_out, h_items and h_counts report
    what was written. Nothing past max_pts (or the capacity) is touched."""
    run = _overflowing_levels(nm, oracle, cuda, base, capacity)
    assert run == min(capacity, (base or 0) + 300 + 250 + 300)


def test_cpp_api_hand_filled_key_pts_are_clipped_on_the_lazy_path(nm, oracle, cuda):
    """A client fills _key_pts[0] of a 128 x 96 octave with one keypoint per pixel (12 288 against nm_keypoint_bound = 6 144)
    after compute_keypoints; compute_orientations / compute_descriptors on the lazy path keep the first 6 144 (the last in
    raster order are dropped), levels 1 and 2 as detected. Sizes, item count and descriptors against
    the oracle. Runs only after the guarded ABI case has shown that this library clips."""
    _overflowing_levels(nm, oracle, cuda, 7, 657)
    w, h, cap, sigma = 128, 96, 16384, 2.0
    frame = np.ascontiguousarray(H.blurred_frame(9, w, h))
    bound = 2 * ((w + 1) // 2) * ((h + 1) // 2)
    sizes = (C.c_int * 4)()
    desc = np.zeros((cap, 128), np.float32)
    x, y = np.zeros(cap, np.float32), np.zeros(cap, np.float32)
    lazy = nm.lib().nm_client_dense_level_keypoints(frame.ctypes.data, w, h, cap, sigma, sizes, desc.ctypes.data,
                                                    x.ctypes.data, y.ctypes.data)
    assert lazy == 1, "compute_descriptors did not take the lazy path (%d)" % lazy
    p, dogs, grad = _octave0(oracle, w, h, 9)
    yy, xx = np.mgrid[0:h, 0:w]
    dense0 = np.stack([xx.ravel(), yy.ravel(), np.full(w * h, sigma), np.zeros(w * h)], 1).astype(np.float32)
    detected = [oracle.compact_keypoints(oracle.find_keypoints(dogs[l + 1], dogs[l], dogs[l + 2], p.peak_threshold,
                                                               p.edge_threshold, 1.0, p.sigma_0, 3, l)) for l in (1, 2)]
    lists = [dense0[:bound]] + detected
    assert len(lists[1]) > 0 and len(lists[2]) > 0
    assert list(sizes) == [bound, len(lists[1]), len(lists[2]), bound + len(lists[1]) + len(lists[2])]
    want = []
    for k in lists:
        o = oracle.detect_orientations(k, grad, w, h, 1.5, 1.0)
        want.append(oracle.compute_sift_descriptors(k, o, grad, w, h, 3, 1.0))
    n = sizes[3]
    _eq(desc[:n], np.concatenate([d for d, _, _ in want]), "descriptors of the clipped hand-filled level and the detected ones")
    _eq(x[:n], np.concatenate([v for _, v, _ in want]), "x")
    _eq(y[:n], np.concatenate([v for _, _, v in want]), "y")
