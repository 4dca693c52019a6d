"""The scene of the loop-closure tests, in numpy float64: K views of one texture whose centres go once round a closed
path, their true view -> scene maps, the true pairwise maps and the true overlap of any two views.

The path is a racetrack: views 0 .. 4 go right along an upper row, views 5 .. 9 come back left along a lower row that is
shifted by half a step, so view 9 ends below and to the left of view 0. A view overlaps its successor, and each view of the
lower row overlaps the two views of the upper row it sits between; every other pair shares next to nothing. That makes the
overlaps two-sided (tests/test_loop_closure_ref.py): high pairs at 0.35 and above, low pairs at 0.10 and below, none between.
"""
import numpy as np

F64 = np.float64
K, VW, VH = 10, 480, 360
STEP_X, STEP_Y = 270, 150                      # the step along a row and the distance of the rows, scene pixels
ORIGIN_X, ORIGIN_Y = 200, 40                   # view 0's pixel (0, 0) in the scene: the mosaic's offset
SCENE_W, SCENE_H = 1800, 600
HIGH, LOW = 0.35, 0.10


def centres():
    """the views' centres in the scene: the upper row rightwards, the lower row leftwards, half a step to the left"""
    c0 = np.array([ORIGIN_X + VW / 2, ORIGIN_Y + VH / 2], F64)
    upper = [c0 + [STEP_X * k, 0] for k in range(5)]
    lower = [c0 + [STEP_X * (4 - k) - STEP_X / 2, STEP_Y] for k in range(5)]
    return np.array(upper + lower)


def view_maps():
    """A_k (K, 3, 3): view-k pixel -> scene pixel. A small roll about the view's centre and a mild perspective term for
    k > 0; A_0 is a pure translation by whole pixels, so the mosaic's frame-0 coordinates are scene - (ORIGIN_X, ORIGIN_Y)."""
    out = []
    for k, (cx, cy) in enumerate(centres()):
        a = 2 * np.pi * k / K
        th = 0.03 * np.sin(a + 0.4 * k) if k else 0.0
        P = np.array([[1, 0, 0], [0, 1, 0], [2e-5 * np.sin(a), -1.5e-5 * np.cos(a), 1]], F64) if k else np.eye(3)
        R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]], F64)
        A = np.array([[1, 0, cx], [0, 1, cy], [0, 0, 1]], F64) @ R @ P @ np.array([[1, 0, -VW / 2], [0, 1, -VH / 2], [0, 0, 1]], F64)
        out.append(A / A[2, 2])
    return np.stack(out)


def pair_map(a, b, maps=None):
    """the true map of view-a pixels to view-b pixels, scaled to [2, 2] = 1"""
    A = view_maps() if maps is None else maps
    H = np.linalg.inv(A[b]) @ A[a]
    return H / H[2, 2]


def apply(H, p):
    q = np.c_[p, np.ones(len(p))] @ np.asarray(H, F64).reshape(3, 3).T
    return q[:, :2] / q[:, 2:]


def _clip(poly, normal, offset):
    """Sutherland-Hodgman against one half plane normal . p <= offset"""
    out = []
    for i in range(len(poly)):
        p, q = poly[i], poly[(i + 1) % len(poly)]
        dp, dq = normal @ p - offset, normal @ q - offset
        if dp <= 0:
            out.append(p)
        if (dp < 0 < dq) or (dq < 0 < dp):
            out.append(p + (q - p) * (dp / (dp - dq)))
    return out


def overlap(a, b, maps=None):
    """The share of frame a that the true map takes into frame b: frame b's rectangle warped into frame a (a homography
    with positive denominators keeps its sides straight), clipped against frame a's rectangle as a polygon, by area."""
    poly = list(apply(pair_map(b, a, maps), np.array([[0, 0], [VW, 0], [VW, VH], [0, VH]], F64)))
    for normal, offset in (([-1, 0], 0), ([1, 0], VW), ([0, -1], 0), ([0, 1], VH)):
        poly = _clip(poly, np.array(normal, F64), float(offset))
        if len(poly) < 3:
            return 0.0
    p = np.array(poly)
    area = 0.5 * abs(np.dot(p[:, 0], np.roll(p[:, 1], -1)) - np.dot(p[:, 1], np.roll(p[:, 0], -1)))
    return float(area / (VW * VH))


def overlaps(maps=None):
    """{(a, b): overlap(a, b)} for every ordered pair a != b"""
    A = view_maps() if maps is None else maps
    return {(a, b): overlap(a, b, A) for a in range(K) for b in range(K) if a != b}


def pair_overlap(a, b, ov=None):
    """an unordered pair's overlap: the smaller of the two directions"""
    ov = overlaps() if ov is None else ov
    return min(ov[(a, b)], ov[(b, a)])


def high_pairs(ov=None):
    """the unordered pairs (a < b) on the high side, in (a, b) order"""
    ov = overlaps() if ov is None else ov
    return [(a, b) for a in range(K) for b in range(a + 1, K) if pair_overlap(a, b, ov) >= HIGH]


def low_pairs(ov=None):
    ov = overlaps() if ov is None else ov
    return [(a, b) for a in range(K) for b in range(a + 1, K) if max(ov[(a, b)], ov[(b, a)]) <= LOW]


def scene(seed):
    """the texture as BGRA uint8 (SCENE_H, SCENE_W, 4), built as tests/test_gpu_mosaic.py builds its scene"""
    import helpers
    g = np.clip(helpers.blurred_frame(seed, SCENE_W, SCENE_H, sigma=2.0) * 1.4, 0, 255).astype(np.uint8)
    return np.stack([g, np.roll(g, 3, 1), np.roll(g, 5, 0), np.full_like(g, 255)], -1)
