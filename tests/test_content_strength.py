"""The structured test content of helpers.blob_field / helpers.step_field is strong enough for what the large-frame GPU tests
(test_gpu_large_frames.py) rely on, and the bound the level lists are sized for (nm_keypoint_bound, nm/pyramidata.h) holds.
Oracle only: these fail if a generator is later weakened into content the GPU comparisons would pass trivially."""
import functools

import numpy as np
import pytest

import helpers as H

W4K, H4K = 3840, 2160


@functools.lru_cache(maxsize=None)
def _ref(kind, seed, w, h, cap=1 << 20):
    import oracle_lib as O
    f = (H.blob_field if kind == "blob" else H.step_field)(seed, w, h)
    return O.sift_detect_describe(f, cap)


@functools.lru_cache(maxsize=None)
def _octave0(kind, seed, w, h):
    """The oracle's octave 0 of the frame: 5 DoG planes and the 3 gradient planes."""
    import oracle_lib as O
    f = (H.blob_field if kind == "blob" else H.step_field)(seed, w, h)
    p = O.sift_params(w, h)
    base = O.convolve(f, *O.create_kernel_for_sigma(p.base_smooth))[0]
    _, dogs, grad = O.octave_pyramid(base, w, h)
    return p, dogs, grad


def test_generators_are_deterministic_quantised_and_in_range():
    for fn in (H.blob_field, H.step_field):
        a, b, c = fn(3, 301, 207), fn(3, 301, 207), fn(4, 301, 207)
        assert a.dtype == np.float32 and a.shape == (207, 301)
        assert np.array_equal(a, b) and not np.array_equal(a, c)
        assert a.min() >= 0 and a.max() <= 255 and np.array_equal(a, np.rint(a))
    blobs, steps = H.blob_field(0, 640, 480), H.step_field(0, 640, 480)
    assert (blobs == 0).any() and (blobs == 255).any(), "no blob saturates: the clipped flats are gone"
    assert len(np.unique(blobs)) > 100
    assert set(np.unique(steps).tolist()) == {0.0, 255.0}


@pytest.mark.parametrize("seed", [0, 1])
def test_blob_field_reaches_the_deep_octaves(oracle, seed):
    """Blurred noise at 4K leaves [.., 91, 17, 2, 0] keypoints in octaves 3..6; the tail's octaves need real work. Measured:
    octaves 2..5 hold 375 / 291 / 138 / 50 (seed 0) and 401 / 268 / 131 / 55 (seed 1)."""
    per_oct = _ref("blob", seed, W4K, H4K)["counts"].sum(1)
    assert len(per_oct) == 7
    for o in (2, 3, 4, 5):
        assert per_oct[o] >= 25, (o, per_oct.tolist())


@pytest.mark.parametrize("seed", [0, 1])
def test_step_field_fills_level_zero(oracle, seed):
    """The capacity cuts of the GPU tests inside level 0 of octave 0 (5000) need more than 5000 keypoints there (measured
    5839 / 5862), and keypoints in every octave up to the tail's last ones."""
    r = _ref("step", seed, W4K, H4K)
    assert r["counts"][0][0] > 5000, r["counts"][0].tolist()
    assert r["n"] > 10000
    assert (r["counts"].sum(1)[:6] > 10).all(), r["counts"].sum(1).tolist()


def _neighbour_extremes(cur, dn, up):
    c = cur[1:-1, 1:-1]
    nb = [pl[1 + dy: pl.shape[0] - 1 + dy, 1 + dx: pl.shape[1] - 1 + dx] for pl in (cur, dn, up) for dy in (-1, 0, 1)
          for dx in (-1, 0, 1) if not (pl is cur and dy == 0 and dx == 0)]
    return c, np.maximum.reduce(nb), np.minimum.reduce(nb)


def test_step_field_has_exact_ties_in_the_dog_planes(oracle):
    """DoG pixels (not 0: not a flat) that EQUAL the largest or the smallest of their 26 neighbours: a >= comparison would
    take them, only the strict one (keypoint.cu:195-196) rejects them."""
    _, dogs, _ = _octave0("step", 0, W4K, H4K)
    ties = 0
    for l in range(3):
        c, hi, lo = _neighbour_extremes(dogs[l + 1], dogs[l], dogs[l + 2])
        ties += int((((c == hi) | (c == lo)) & (c != 0)).sum())
    assert ties >= 1000, ties


def test_step_field_keypoints_see_exactly_zero_gradients(oracle):
    """Orientation windows (orientation.cu:29-30: radius min(max(floor(4.5 sigma), 1), 10), clipped at the plane) that hold
    gradients of magnitude exactly 0: the flats of the 0/255 frame. Their votes are exact zeros in the histogram bins."""
    p, dogs, grad = _octave0("step", 0, W4K, H4K)
    kp = oracle.compact_keypoints(oracle.find_keypoints(dogs[1], dogs[0], dogs[2], p.peak_threshold, p.edge_threshold, 1.0,
                                                        p.sigma_0, 3, 0))
    assert len(kp) > 5000
    hits = 0
    for x, y, s, lev in kp[::7]:
        xi, yi = int(float(x) + 0.5), int(float(y) + 0.5)
        r = min(max(int(np.floor(3 * 1.5 * s)), 1), 10)
        win = grad[int(lev), max(0, yi - r): yi + r + 1, max(0, xi - r): xi + r + 1, 0]
        hits += bool((win == 0).any())
    assert hits >= 50, hits


# ---- the bound of the level lists ------------------------------------------------------------------------------------
def _lattice(w, h, pattern, hi=9.0, lo=-9.0):
    """The middle DoG plane: a 2 x 2 tile of 'H' (positive), 'L' (negative) and '0' repeated over the plane."""
    val = {"H": hi, "L": lo, "0": 0.0}
    tile = np.array([[val[pattern[0]], val[pattern[1]]], [val[pattern[2]], val[pattern[3]]]], np.float32)
    return np.tile(tile, ((h + 1) // 2, (w + 1) // 2))[:h, :w].copy()


@pytest.mark.parametrize("w,h", [(9, 7), (10, 8), (64, 48), (101, 77), (128, 96), (255, 130)])
def test_keypoints_per_level_never_exceed_the_list_bound(oracle, w, h):
    """A keypoint is a strict extremum of its 26 neighbours, so two touching pixels are never both maxima (or both minima)
    and a level holds at most 2 ceil(w/2) ceil(h/2) keypoints -- what PyramidData sizes _orientations[l] for and what the
    lazy path clips at. Adversarial planes: H / L / 0 lattices in the middle plane (H and L on the two diagonals of the 2 x 2
    tile make every H a strict maximum and every L a strict minimum), flat neighbours, and random three-valued planes."""
    p = oracle.sift_params(1920, 1080)
    bound = 2 * ((w + 1) // 2) * ((h + 1) // 2)
    flat = np.zeros((h, w), np.float32)
    rng = np.random.default_rng(w * 1000 + h)
    planes = [_lattice(w, h, pat) for pat in ("H00L", "L00H", "0HL0", "0LH0", "HL0H", "H0H0", "HHLL")]
    planes += [rng.choice(np.array([9.0, -9.0, 0.0], np.float32), (h, w)) for _ in range(4)]
    best = 0
    for cur in planes:
        for level in range(3):
            n = len(oracle.compact_keypoints(oracle.find_keypoints(cur, flat, flat, p.peak_threshold, p.edge_threshold, 1.0,
                                                                   p.sigma_0, 3, level)))
            assert n <= bound, (w, h, n, bound)
            best = max(best, n)
    if min(w, h) >= 64:
        assert best >= 0.9 * bound, (w, h, best, bound)
    assert best > 0
