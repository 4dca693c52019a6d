"""The corner detector's definition (include/nm_abi.h, "Corner detection") in numpy integers and float64, written from the
header text and independent of the C++ code. Every fp64 step is a single operation (numpy fuses nothing), so the model is
expected to EQUAL the host twin: coordinates, the scores' bits, counts, totals and score planes. Also the shared cases of
tests/test_klt_corners_host.py and tests/test_gpu_klt_corners.py."""
import numpy as np

import klt_ref as K

F32 = np.float32


def levels(gray, mask=None):
    """(q int64 with 0 where a pixel holds no level, valid bool)"""
    g = np.asarray(gray, F32)
    with np.errstate(invalid="ignore"):
        valid = (g >= 0) & (g <= 255)
        q = np.where(valid, np.rint(np.where(valid, g, 0) * F32(16)), 0).astype(np.int64)
    if mask is not None:
        valid &= np.asarray(mask) != 0
    return np.where(valid, q, 0), valid


def _box(a, lo, hi):
    """sum of a over offsets lo .. hi on both axes (zero outside), int64"""
    h, w = a.shape
    p = max(-lo, hi) + 1
    c = np.zeros((h + 2 * p + 1, w + 2 * p + 1), np.int64)
    c[p + 1:p + 1 + h, p + 1:p + 1 + w] = a
    c = c.cumsum(0).cumsum(1)
    y, x = np.mgrid[0:h, 0:w]
    y0, y1, x0, x1 = y + p + lo, y + p + hi + 1, x + p + lo, x + p + hi + 1
    return c[y1, x1] - c[y0, x1] - c[y1, x0] + c[y0, x0]


def sums(gray, r, mask=None):
    """(has_window, Gxx, Gxy, Gyy) planes; the sums are meaningful where has_window"""
    q, valid = levels(gray, mask)
    h, w = q.shape
    inside = np.zeros((h, w), bool)
    inside[r + 1:h - r - 2, r + 1:w - r - 2] = True
    has = inside & (_box((~valid).astype(np.int64), -(r + 1), r + 2) == 0)
    gx, gy = np.zeros_like(q), np.zeros_like(q)
    gx[:, 1:-1] = q[:, 2:] - q[:, :-2]
    gy[1:-1, :] = q[2:, :] - q[:-2, :]
    return has, _box(gx * gx, -r, r), _box(gx * gy, -r, r), _box(gy * gy, -r, r)


def score_plane(gray, r, min_eig, mask=None):
    has, Gxx, Gxy, Gyy = sums(gray, r, mask)
    a, b, c = Gxx.astype(np.float64), Gxy.astype(np.float64), Gyy.astype(np.float64)
    with np.errstate(all="ignore"):
        t1, t2 = a * c, b * b
        det = t1 - t2
        s, dd = a + c, a - c
        root = np.sqrt(dd * dd + 4.0 * t2)
        lam = (s - root) / 2.0
        eig = lam / float(1024 * (2 * r + 1) ** 2)
        scored = has & np.isfinite(det) & (det > 0.0) & ~(eig < float(F32(min_eig)))
        return np.where(scored, eig, -1.0).astype(F32)


def held_pixels(held, fw, fh):
    """the pixels of the tried held rows, (m, 2) int64; held = (xs, ys, nH, cap_held) or None"""
    if held is None:
        return np.zeros((0, 2), np.int64)
    xs, ys, nH, cap_held = held
    n = min(max(int(nH), 0), cap_held)
    hx, hy = np.asarray(xs, F32)[:n], np.asarray(ys, F32)[:n]
    with np.errstate(invalid="ignore"):
        tried = (hx >= 0) & np.isfinite(hx) & np.isfinite(hy)
    lim = 2.0 ** 40                                   # further than any frame reaches; keeps the conversion defined
    tried &= (np.abs(np.where(tried, hx, 0)) < lim) & (np.abs(np.where(tried, hy, 0)) < lim)
    return np.c_[np.rint(hx[tried]), np.rint(hy[tried])].astype(np.int64)


def corners(gray, r=7, nms=8, min_eig=1.0, cap=4096, mask=None, held=None):
    """dict(x, y, score: the first `cap` corners in raster order, count, total, plane)"""
    plane = score_plane(gray, r, min_eig, mask)
    h, w = plane.shape
    pad = np.full((h + 2 * nms, w + 2 * nms), F32(-1))
    pad[nms:nms + h, nms:nms + w] = plane
    wins = plane >= 0
    for v in range(-nms, nms + 1):
        for u in range(-nms, nms + 1):
            if (u, v) == (0, 0):
                continue
            other = pad[nms + v:nms + v + h, nms + u:nms + u + w]
            first = v < 0 or (v == 0 and u < 0)       # the other pixel comes first in raster order
            wins &= ~((other > plane) | ((other == plane) & first))
    ys, xs = np.nonzero(wins)
    keep = np.ones(len(xs), bool)
    for px, py in held_pixels(held, w, h):
        keep &= ~((np.abs(xs - px) <= nms) & (np.abs(ys - py) <= nms))
    xs, ys = xs[keep], ys[keep]
    total = len(xs)
    n = min(total, cap)
    return dict(x=xs[:n].astype(F32), y=ys[:n].astype(F32), score=plane[ys[:n], xs[:n]], count=n, total=total, plane=plane)


# ---- shared cases ----
def noise(seed, w, h):
    return K.textured(seed, w, h, 0.0, 255.0)


def checker(w, h, square):
    y, x = np.mgrid[0:h, 0:w]
    return (255.0 * (((x // square) + (y // square)) & 1)).astype(F32)


def bright_square(w, h):
    g = np.full((h, w), 40.0, F32)
    g[h // 2 - 8:h // 2 + 8, w // 2 - 10:w // 2 + 10] = 200.0
    return g


def holes(w, h):
    m = np.ones((h, w), np.uint8)
    m[h // 3:h // 3 + 3, w // 4:w // 4 + 5] = 0
    m[2 * h // 3, 2 * w // 3] = 0
    m[0:2, :] = 0
    return m


def _case(name, grays, **kw):
    c = dict(name=name, grays=grays, r=7, nms=8, min_eig=0.25, cap=512, mask=None, held=None)
    c.update(kw)
    return c


def cases():
    out = []
    special = noise(3, 130, 70)
    special[20, 31] = np.nan
    special[44, 90] = 255.5
    for w, h, g in ((97, 61, noise(1, 97, 61)), (64, 64, noise(2, 64, 64)), (130, 70, special)):
        for r in (1, 3, 7):
            for nms in (1, 8, 16):
                out.append(_case("noise%dx%d_r%d_nms%d" % (w, h, r, nms), [g], r=r, nms=nms, cap=4096))
    for r in (1, 3, 7):
        s = 2 * r + 4
        out.append(_case("one_window_r%d" % r, [noise(5, s, s)], r=r, min_eig=0.0))
        out.append(_case("no_window_r%d" % r, [noise(5, s - 1, s - 1)], r=r, min_eig=0.0))
    out.append(_case("no_window_33x17", [noise(6, 33, 17)], min_eig=0.0))
    out.append(_case("flat", [np.full((40, 50), 128.0, F32)], r=3, min_eig=0.0))
    out.append(_case("checker2_r7", [checker(64, 48, 2)], cap=4096))
    out.append(_case("checker1_r3", [checker(47, 33, 1)], r=3, nms=1, min_eig=0.0, cap=4096))
    out.append(_case("square", [bright_square(80, 60)], r=3, nms=8, min_eig=1.0))
    base = noise(1, 97, 61)
    out.append(_case("mask_holes", [base], r=3, mask=holes(97, 61)))
    out.append(_case("min_eig_0", [base], r=3, min_eig=0.0))
    out.append(_case("min_eig_above_all", [base], r=3, min_eig=1e9))
    out.append(_case("cap_below_total", [base], r=3, nms=1, cap=5))
    # held points round the corners the frame has without them
    free = corners(base, 3, 8, 0.25)
    assert free["total"] >= 4
    cx, cy = free["x"], free["y"]
    nan, inf = float("nan"), float("inf")
    pts = [(cx[0], cy[0]), (cx[1] + 8, cy[1] - 8), (cx[2] + 9, cy[2]), (cx[3] + 0.4, cy[3] - 9), (0, 30), (96, 5), (100, 30), (50, -3),
           (50, 64), (104.6, 30), (112.49, 20), (113, 20), (-1, 30), (-0.25, 12), (nan, 30), (30, nan), (inf, 30), (30, -inf), (3e9, 30),
           (cx[-1], cy[-1])]
    hx, hy = np.array([p[0] for p in pts], F32), np.array([p[1] for p in pts], F32)
    for nH in (0, 1, len(pts), len(pts) + 7, -3):
        out.append(_case("held_nH%d" % nH, [base], r=3, held=[(hx, hy, nH)]))
    out.append(_case("held_short_cap", [base], r=3, held=[(hx[:4], hy[:4], 9)]))
    frames = [base, noise(7, 97, 61), checker(97, 61, 3)]
    out.append(_case("three_frames", frames, r=3, held=[(hx, hy, len(pts)), (hx, hy, 2), (hx, hy, 0)]))
    out.append(_case("sixty_four_repeated", [frames[k % 3] for k in range(64)], r=3, nms=8))
    return out


def model_case(c):
    """the model's result per frame of a case"""
    res = []
    for k, g in enumerate(c["grays"]):
        held = None
        if c["held"] is not None:
            hx, hy, nH = c["held"][k]
            held = (hx, hy, nH, len(hx))
        res.append(corners(g, c["r"], c["nms"], c["min_eig"], c["cap"], c["mask"], held))
    return res


def assert_equal(got, want, k, what):
    """frame k of a result dict of (n, ...) arrays against the model's frame result, exactly"""
    n = want["count"]
    assert int(got["count"][k]) == n and int(got["total"][k]) == want["total"], (what, k, int(got["count"][k]), n, want["total"])
    for key in ("x", "y", "score"):
        a = np.asarray(got[key][k])[:n]
        assert np.array_equal(a.view(np.uint32), want[key].view(np.uint32)), (what, k, key)
    if got.get("score_plane") is not None:
        assert np.array_equal(np.asarray(got["score_plane"][k]).view(np.uint32), want["plane"].view(np.uint32)), (what, k, "plane")
