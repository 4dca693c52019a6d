"""Inputs for the corner detector's edges that its feature tests do not reach, each with the assertion, made on the numpy
model of tests/klt_corners_ref.py and never on the code under test, that the input reaches what it is built for: frames
whose flag words take the emit kernel through 2 to 32 scan trips and caps placed at the trip boundaries (A), Gxy beyond
32 bits signed of both signs at corners (B), exactly equal isolated maxima within nms of each other on either side of
the tile seams (C), lone pixels without a level at the 88-bit word's split, the seams and the plane's edges (D), and held
points in bulk (E). Shared by tests/test_klt_corners_edges_host.py and tests/test_gpu_klt_corners_edges.py."""
import functools

import numpy as np

import klt_corners_ref as R
import klt_ref as K

F32 = np.float32
TX, TY = 64, 16                                                       # a tile of the response and suppression passes
TRIP = 1024                                                           # flag words per trip of the emit kernel


def case(name, grays, **kw):
    c = R._case(name, grays, cap=1 << 16)
    c.update(kw)
    return c


def words(fw, fh):
    """flag words of a frame: one for 64 pixels of a pixel row"""
    return fh * ((fw + TX - 1) // TX)


def trips(fw, fh):
    return (words(fw, fh) + TRIP - 1) // TRIP


def word_of(x, y, fw):
    return np.asarray(y).astype(np.int64) * ((fw + TX - 1) // TX) + np.asarray(x).astype(np.int64) // TX


def apart(x, y):
    """the smallest Chebyshev distance between two of the points"""
    x, y = np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64)
    best = 1 << 30
    for i in range(len(x) - 1):
        best = min(best, int(np.maximum(np.abs(x[i + 1:] - x[i]), np.abs(y[i + 1:] - y[i])).min()))
    return best


# ---- A. scan trips --------------------------------------------------------------------------------------------------------------
# name: (fw, fh, nms, words, trips, trips that hold corners, the least total); r = 3
TRIP_FRAMES = {
    "trips_64x1025": (64, 1025, 8, 1025, 2, 1, 8),                       # the second trip holds one word
    "trips_64x2100": (64, 2100, 2, 2100, 3, 3, 512),                     # the parity buffer is reused
    "trips_130x800": (130, 800, 4, 2400, 3, 3, 256),                     # trip boundaries inside a pixel row
    "trips_18x32767": (18, 32767, 1, 32767, 32, 32, 2048),                # one word a row, the tallest frame
    "trips_32767x18": (32767, 18, 16, 9216, 9, 5, 256),                  # 512 words a row, the widest mark pitch
}


@functools.lru_cache(maxsize=None)
def trip_gray(name):
    fw, fh = TRIP_FRAMES[name][:2]
    g = R.noise(31 + fw % 7 + fh % 11, fw, fh)
    return g


@functools.lru_cache(maxsize=None)
def trip_model(name):
    """the model's result on a trip frame, every corner kept"""
    return R.corners(trip_gray(name), 3, TRIP_FRAMES[name][2], 0.25, 1 << 22)


def trip_case(name, **kw):
    return case(name, [trip_gray(name)], r=3, nms=TRIP_FRAMES[name][2], **kw)


def assert_trip_frame(name):
    fw, fh, nms, want_words, want_trips, want_live, least = TRIP_FRAMES[name]
    assert words(fw, fh) == want_words and trips(fw, fh) == want_trips >= 2
    m = trip_model(name)
    w = word_of(m["x"], m["y"], fw)
    assert m["total"] >= least and (np.diff(w) >= 0).all()
    per_trip = np.bincount(w // TRIP, minlength=want_trips)
    wpr, r, live = want_words // fh, 3, 0
    for t in range(want_trips):                                       # every trip that holds a row with windows (rows r + 1 ..
        y0, y1 = t * TRIP // wpr, min(((t + 1) * TRIP - 1) // wpr, fh - 1)     # fh - r - 3) adds corners to the running base
        if y1 >= r + 1 and y0 <= fh - r - 3:
            assert per_trip[t] >= 1, (name, t)
            live += 1
    assert live == want_live and (live >= 2 or want_trips == 2)       # two or more: a trip starts from a base that is not 0


def trip_caps(name):
    """the caps at and round the trip boundaries: (caps, c1, c2, total); c1 (c2) corners lie in the first 1024 (2048) words"""
    fw = TRIP_FRAMES[name][0]
    m = trip_model(name)
    w = word_of(m["x"], m["y"], fw)
    c1, c2, total = int((w < TRIP).sum()), int((w < 2 * TRIP).sum()), m["total"]
    assert c1 >= 2 and c2 - c1 >= 1 and total > c2 + 1
    if name == "trips_130x800":
        wpr = 3
        assert 1023 // wpr == 1024 // wpr and 2047 // wpr == 2048 // wpr   # both boundaries fall inside a pixel row
    caps = [1, c1 - 1, c1, c1 + 1, c2, total - 1, total, total + 1]
    return caps, c1, c2, total


def back_to_back_case():
    """three different multi-trip frames of one shape with totals that differ: one workgroup emits them in sequence"""
    g = trip_gray("trips_130x800")
    grays = [g, np.ascontiguousarray(g[::-1, ::-1]) * F32(0.5), R.noise(77, 130, 800)]
    c = case("back_to_back", grays, r=3, nms=4)
    totals = [m["total"] for m in R.model_case(c)]
    assert len(set(totals)) == 3 and min(totals) >= 3, totals
    return c


# ---- B. Gxy beyond 32 bits signed ------------------------------------------------------------------------------------------------
def stripes(s, w, h, seed, share):
    """diagonal 0 / 255 stripes of period 4 along x + s y, a seeded `share` of the pixels replaced by uniform integers"""
    y, x = np.mgrid[0:h, 0:w]
    g = (255.0 * (((x + s * y) % 4) < 2)).astype(F32)
    rng = np.random.RandomState(seed)
    hit = rng.uniform(size=(h, w)) < share
    g[hit] = rng.randint(0, 256, size=int(hit.sum())).astype(F32)
    return g


def plane_of_sums(has, Gxx, Gxy, Gyy, r, min_eig):
    """klt_corners_ref.score_plane's fp64 steps on given sums"""
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


def wrapped_to_int32(G):
    return ((G + 2 ** 31) % 2 ** 32) - 2 ** 31


def gxy_case(h=70, w=130):
    grays = [stripes(+1, w, h, 5, 0.05), stripes(-1, w, h, 6, 0.10)]
    return case("gxy33_%dx%d" % (w, h), grays, r=7, nms=8)


def assert_gxy_case(c):
    for g, sign, m in zip(c["grays"], (+1, -1), R.model_case(c)):
        has, Gxx, Gxy, Gyy = R.sums(g, c["r"])
        true = plane_of_sums(has, Gxx, Gxy, Gyy, c["r"], c["min_eig"])
        assert np.array_equal(true.view(np.uint32), m["plane"].view(np.uint32))
        at = Gxy[m["y"].astype(int), m["x"].astype(int)]
        assert m["total"] >= 3 and (sign * at > 2 ** 31).any(), (sign, at)     # at corners, not only at scored pixels
        assert (sign * Gxy[has] > 0).all() and np.abs(Gxy).max() <= 3745440000
        wrapped = plane_of_sums(has, Gxx, wrapped_to_int32(Gxy), Gyy, c["r"], c["min_eig"])
        assert not np.array_equal(wrapped, true)
        assert (wrapped[m["y"].astype(int), m["x"].astype(int)] != m["score"]).any()
        as_unsigned = plane_of_sums(has, Gxx, Gxy % 2 ** 32, Gyy, c["r"], c["min_eig"])
        assert sign > 0 or not np.array_equal(as_unsigned, true)


# ---- C. exact ties ----------------------------------------------------------------------------------------------------------------
def mirror_tiling(seed, bw=32, bh=16, nx=6, ny=4):
    """blocks of bw x bh noise, flipped in x in every other column of blocks and in y in every other row of blocks: the
    mirror axes lie between pixels k bw - 1 and k bw, and between rows k bh - 1 and k bh"""
    b = R.noise(seed, bw, bh)
    row = np.concatenate([b if i % 2 == 0 else b[:, ::-1] for i in range(nx)], axis=1)
    return np.ascontiguousarray(np.concatenate([row if j % 2 == 0 else row[::-1] for j in range(ny)], axis=0))


def half_turn_strips(seed, width=20, count=9, first=14, bh=16, bands=2, tail=6):
    """Bands of 2 bh rows; in a band, side by side from column `first`, `count` strips [B ; B turned by 180 degrees] of
    `width` columns, a different B per strip: a faint texture with one patch of 3 x 3 random levels three rows above the
    seam, two columns right of the strip's centre in every other strip and three left of it in the rest. The patch and its
    image are the strip's strongest points, exactly equal and about five pixels apart, the earlier row's further right (or
    left). The strip from column 54 has its centre on the seam at x = 64; every band's centre is a seam of 16 rows."""
    fw = first + width * count + tail
    g = K.textured(seed, fw, 2 * bh * bands, 100.0, 110.0).copy()
    rng = np.random.RandomState(seed)
    for band in range(bands):
        for k in range(count):
            b = K.textured(seed + 1 + band * count + k, width, bh, 100.0, 110.0).copy()
            cx = width // 2 + 2 if (k + band) % 2 == 0 else width // 2 - 3
            b[bh - 4:bh - 1, cx - 1:cx + 2] = rng.randint(0, 256, size=(3, 3))
            x, y = first + width * k, 2 * bh * band
            g[y:y + bh, x:x + width] = b
            g[y + bh:y + 2 * bh, x:x + width] = b[::-1, ::-1]
    return np.ascontiguousarray(g.astype(F32))


def nms_wins(plane, nms, last=False):
    """klt_corners_ref.corners' suppression on a score plane; last: of equal scores the LAST in raster order wins"""
    h, w = plane.shape
    pad = np.full((h + 2 * nms, w + 2 * nms), F32(-1))
    pad[nms:nms + h, nms:nms + w] = plane
    wins = plane >= 0
    for v in range(-nms, nms + 1):
        for u in range(-nms, nms + 1):
            if (u, v) == (0, 0):
                continue
            other = pad[nms + v:nms + v + h, nms + u:nms + u + w]
            first = v < 0 or (v == 0 and u < 0)
            wins &= ~((other > plane) | ((other == plane) & (first != last)))
    return wins


def ties(plane, nms):
    """Of the scored pixels that are a window maximum by value: dict of lists of (winner x, y, loser x, y), a loser being such
    a pixel with an equal pixel that comes earlier in its window and a winner the corner that is equal to it, by where the
    winner lies from the loser: "same_row", "earlier_row" (any column) and "earlier_row_right" (a subset of the latter)"""
    h, w = plane.shape
    pad = np.full((h + 2 * nms, w + 2 * nms), F32(-1))
    pad[nms:nms + h, nms:nms + w] = plane
    top = plane >= 0
    for v in range(-nms, nms + 1):
        for u in range(-nms, nms + 1):
            top &= ~(pad[nms + v:nms + v + h, nms + u:nms + u + w] > plane)
    corner = nms_wins(plane, nms)
    out = dict(same_row=[], earlier_row=[], earlier_row_right=[])
    for y, x in zip(*np.nonzero(top & ~corner)):
        for v in range(-nms, 1):
            for u in range(-nms, nms + 1):
                yy, xx = y + v, x + u
                if (v == 0 and u >= 0) or yy < 0 or xx < 0 or xx >= w or plane[yy, xx] != plane[y, x] or not corner[yy, xx]:
                    continue
                pair = (int(xx), int(yy), int(x), int(y))
                if v == 0:
                    out["same_row"].append(pair)
                else:
                    out["earlier_row"].append(pair)
                    if u > 0:
                        out["earlier_row_right"].append(pair)
    return out


def tie_cases():
    """(case, the kinds of loser it is for, whether a pair must straddle a (seam of 64 columns, seam of 16 rows))"""
    both = ("same_row", "earlier_row")
    tiling, off_seam, strips = mirror_tiling(40), mirror_tiling(43, 48, 16, 4, 4), half_turn_strips(1)
    assert tiling.shape == off_seam.shape == (64, 192) and strips.shape == (64, 200)
    return [(case("tiling_r3_nms8", [tiling], r=3, nms=8), both, (True, True)),
            (case("tiling_r3_nms16", [tiling], r=3, nms=16), both, (True, True)),
            (case("tiling_r1_nms4", [tiling], r=1, nms=4), both, (True, True)),
            (case("tiling_axes_off_the_seam_r1_nms4", [off_seam], r=1, nms=4), both, (False, True)),   # axes at x = 48, 96, 144
            (case("half_turn_r1_nms8", [strips], r=1, nms=8), ("earlier_row", "earlier_row_right"), (True, True)),
            (case("half_turn_r3_nms8", [strips], r=3, nms=8), ("earlier_row", "earlier_row_right"), (True, True))]


def assert_tie_case(c, kinds, straddle):
    nms = c["nms"]
    m = R.model_case(c)[0]
    plane = m["plane"]
    first = nms_wins(plane, nms)
    ys, xs = np.nonzero(first)
    assert np.array_equal(xs.astype(F32), m["x"]) and np.array_equal(ys.astype(F32), m["y"])     # the variant is the model's rule
    assert not np.array_equal(nms_wins(plane, nms, last=True), first)
    t = ties(plane, nms)
    for kind in kinds:
        assert len(set(p[2:] for p in t[kind])) >= 3, (c["name"], kind, len(t[kind]))
    pairs = t["earlier_row_right"] if "earlier_row_right" in kinds else [p for kind in kinds for p in t[kind]]
    assert len(set(p[:2] for p in pairs)) >= 3                        # tie winners
    assert not straddle[0] or any(p[0] // TX != p[2] // TX for p in pairs), c["name"]
    assert not straddle[1] or any(p[1] // TY != p[3] // TY for p in pairs), c["name"]
    return t


# ---- D. the window's footprint --------------------------------------------------------------------------------------------------
FOOT_W, FOOT_H = 200, 50
FOOT_COLS = (0, 1, 51, 52, 53, 63, 64, 65, 115, 116, 117, 198, 199)
FOOT_ROWS = (0, 15, 16, 17, 49)
BAD_VALUES = (float("nan"), -1.0, 255.5)


def foot_groups(r):
    """the 65 positions in groups whose members lie further than 2 r + 4 apart in at least one axis, greedily"""
    groups = []
    for by in FOOT_ROWS:
        for bx in FOOT_COLS:
            for grp in groups:
                if all(abs(bx - ox) > 2 * r + 4 or abs(by - oy) > 2 * r + 4 for ox, oy in grp):
                    grp.append((bx, by))
                    break
            else:
                groups.append([(bx, by)])
    assert sum(len(grp) for grp in groups) == len(FOOT_COLS) * len(FOOT_ROWS)
    return groups


@functools.lru_cache(maxsize=None)
def foot_clean():
    g = R.noise(21, FOOT_W, FOOT_H)
    return g


def foot_cases(r):
    """(a case of one frame per group with bad VALUES at the group's positions, the kinds taking turns; cases of one frame
    each with the mask byte 0 there instead), min_eig 0 so that only the window decides; and the groups"""
    groups = foot_groups(r)
    grays, masked = [], []
    for i, grp in enumerate(groups):
        g, m = foot_clean().copy(), np.ones((FOOT_H, FOOT_W), np.uint8)
        for j, (bx, by) in enumerate(grp):
            g[by, bx] = BAD_VALUES[(i + j) % 3]
            m[by, bx] = 0
        grays.append(g)
        masked.append(case("foot_mask_r%d_%d" % (r, i), [foot_clean(), foot_clean()[::-1].copy()], r=r, nms=4, min_eig=0.0, mask=m))
    return case("foot_r%d" % r, grays, r=r, nms=4, min_eig=0.0), masked, groups


def assert_footprint(plane, clean_plane, grp, r):
    """the pixels unscored against the clean frame are exactly those with x - bx and y - by in [-(r + 2), r + 1]"""
    y, x = np.mgrid[0:FOOT_H, 0:FOOT_W]
    foot = np.zeros((FOOT_H, FOOT_W), bool)
    for bx, by in grp:
        foot |= (x - bx >= -(r + 2)) & (x - bx <= r + 1) & (y - by >= -(r + 2)) & (y - by <= r + 1)
    was = clean_plane >= 0
    assert np.array_equal((plane < 0) & was, foot & was)
    assert np.array_equal(plane[~foot].view(np.uint32), clean_plane[~foot].view(np.uint32))
    return foot, was


# ---- E. held points in bulk -----------------------------------------------------------------------------------------------------
def bulk_held_case():
    """the 130 x 800 frame three times, held: all its own corners, every other one, none"""
    name = "trips_130x800"
    m = trip_model(name)
    total, nms = m["total"], TRIP_FRAMES[name][2]
    assert 3 * total > 256 and total > 256                            # more than one workgroup's worth of held rows per launch
    assert apart(m["x"], m["y"]) > nms                                # what makes "exactly the other half" true
    hx, hy = m["x"].copy(), m["y"].copy()
    half = (total + 1) // 2
    ex, ey = np.full(total, F32(-7)), np.full(total, F32(3))          # rows at and beyond the count are never tried
    ex[:half], ey[:half] = hx[0::2], hy[0::2]
    g = trip_gray(name)
    c = case("bulk_held", [g, g, g], r=3, nms=nms, held=[(hx, hy, total), (ex, ey, half), (hx, hy, 0)])
    want = [(hx[:0], hy[:0]), (hx[1::2], hy[1::2]), (hx, hy)]
    return c, want


def assert_bulk_held(x, y, count, total, want):
    """the three properties, on any result (the model's, the host twin's, the device's)"""
    for k, (wx, wy) in enumerate(want):
        n = len(wx)
        assert int(count[k]) == n == int(total[k]), (k, int(count[k]), int(total[k]), n)
        assert np.array_equal(np.asarray(x[k])[:n], wx) and np.array_equal(np.asarray(y[k])[:n], wy), k


def wide_held_case():
    """the 32767 x 18 frame with held points: every third of its own corners, and rows beyond the right and the bottom
    edge, where the widest mark plane's border takes them"""
    name = "trips_32767x18"
    m = trip_model(name)
    hx = np.concatenate([m["x"][0::3], np.array([32767 + 15, 32767 + 16, 32766, 0, 20000], F32)])
    hy = np.concatenate([m["y"][0::3], np.array([9, 9, 18 + 15, -16, 18 + 16], F32)])
    c = trip_case(name, held=[(hx, hy, len(hx))])
    left = R.model_case(c)[0]["total"]
    assert 0 < left < m["total"] - len(m["x"][0::3]) + 1 and len(hx) > 256
    return c


def cut(m, cap):
    """the model's result `m` (every corner kept) as it is under a cap"""
    n = min(m["total"], cap)
    return dict(x=m["x"][:n], y=m["y"][:n], score=m["score"][:n], count=n, total=m["total"], plane=m["plane"])


def mask_case(w, h):
    """three different frames under one mask: 128 x 40 takes the 16-byte loads where the planes allow, 130 x 70 never"""
    grays = [R.noise(9, w, h), R.noise(10, w, h), np.ascontiguousarray(R.noise(9, w, h)[::-1])]
    return case("mask_n3_%dx%d" % (w, h), grays, r=3, nms=4, mask=R.holes(w, h))
