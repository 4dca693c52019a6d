"""The host twin of the corner detector (nm_klt_corners_host_f32) against the Python model of tests/klt_corners_ref.py,
exactly: coordinates, the scores' bits, counts, totals and score planes; every refusal of the two entries (the device entry
refuses before any launch or device access, so it is called here with pointers that are never dereferenced); and three
properties that are asserted, not only compared: the sums are the tracker's, the tracker calls no corner FLAT or BORDER,
and corners keep their distance from each other and from held points. Last, the benefit: corners against the lattice as
the tracker's points on the accuracy cases of tests/test_klt_host.py."""
import ctypes as C

import numpy as np
import pytest

import klt_corners_ref as R
import klt_ref as K

F32 = np.float32
CASES = R.cases()
MODEL = {}


def model(c):
    if c["name"] not in MODEL:
        MODEL[c["name"]] = R.model_case(c)
    return MODEL[c["name"]]


def host_case(nm, c, want_plane=True):
    held = None
    if c["held"] is not None:
        held = ([h[0] for h in c["held"]], [h[1] for h in c["held"]], [h[2] for h in c["held"]])
    return nm.klt_corners_host(c["grays"], radius=c["r"], nms=c["nms"], min_eig=c["min_eig"], cap=c["cap"], mask=c["mask"],
                               held=held, want_score_plane=want_plane, fill=-7)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_host_twin_equals_the_model(nm, c):
    got = host_case(nm, c)
    for k, want in enumerate(model(c)):
        R.assert_equal(got, want, k, c["name"])
        assert (got["x"][k][want["count"]:] == -7).all()            # rows at and beyond the count are not written


def test_the_cases_reach_what_they_are_meant_to(nm):
    by = {c["name"]: model(c) for c in CASES}
    for r in (1, 3, 7):
        one = by["one_window_r%d" % r][0]
        assert (one["plane"] >= 0).sum() <= 1 and R.sums(R.noise(5, 2 * r + 4, 2 * r + 4), r)[0].sum() == 1
        assert by["no_window_r%d" % r][0]["total"] == 0
    assert by["no_window_33x17"][0]["total"] == 0 and by["flat"][0]["total"] == 0 and by["min_eig_above_all"][0]["total"] == 0
    assert all(by["noise%dx%d_r%d_nms8" % (w, h, r)][0]["total"] >= 3 for w, h in ((97, 61), (64, 64), (130, 70)) for r in (1, 3, 7))
    has, Gxx, Gxy, Gyy = R.sums(R.checker(64, 48, 2), 7)
    assert has.any() and (Gxx[has] == 3745440000).all() and (Gyy[has] == 3745440000).all() and 3745440000 > 2 ** 31
    chk = by["checker2_r7"][0]
    scores = chk["plane"][chk["plane"] >= 0]
    assert scores.size == has.sum() and len(set(scores.tolist())) == 1    # equal scores: the raster tie rule decides alone,
    assert chk["total"] == 1 and (chk["x"][0], chk["y"][0]) == (8, 8)      # and only the first scored pixel beats every neighbour
    assert by["checker1_r3"][0]["total"] == 0                              # gx = gy = 0 everywhere: flat
    sq = by["square"][0]
    g = R.bright_square(80, 60)
    ends = {(80 // 2 - 10, 60 // 2 - 8), (80 // 2 + 9, 60 // 2 - 8), (80 // 2 - 10, 60 // 2 + 7), (80 // 2 + 9, 60 // 2 + 7)}
    assert sq["total"] == 4 and g[30, 40] == 200.0
    assert all(min(max(abs(x - ex), abs(y - ey)) for ex, ey in ends) <= 2 for x, y in zip(sq["x"], sq["y"]))
    assert by["mask_holes"][0]["total"] != by["noise97x61_r3_nms8"][0]["total"] or \
        not np.array_equal(by["mask_holes"][0]["plane"], by["noise97x61_r3_nms8"][0]["plane"])
    cut = by["cap_below_total"][0]
    assert cut["count"] == 5 < cut["total"]
    full = R.corners(R.noise(1, 97, 61), 3, 1, 0.25, 4096)
    assert np.array_equal(cut["x"], full["x"][:5]) and np.array_equal(cut["y"], full["y"][:5])      # the first in raster order
    free, held = by["noise97x61_r3_nms8"][0], by["held_nH20"][0]
    pairs = lambda m: set(zip(m["x"].tolist(), m["y"].tolist()))
    cx, cy = free["x"], free["y"]
    gone = pairs(free) - pairs(held)
    assert {(cx[0], cy[0]), (cx[1], cy[1]), (cx[-1], cy[-1])} <= gone       # on a corner, nms away, the last row
    assert (cx[2], cy[2]) in pairs(held) and (cx[3], cy[3]) in pairs(held)     # nms + 1 away
    assert pairs(held) <= pairs(free)                                          # held points make no new corner
    assert pairs(by["held_nH0"][0]) == pairs(free) == pairs(by["held_nH-3"][0])
    assert pairs(by["held_nH1"][0]) == pairs(free) - {(cx[0], cy[0])}
    assert pairs(by["held_nH27"][0]) == pairs(held)                            # above cap_held: clipped
    assert pairs(by["held_short_cap"][0]) == pairs(free) - {(cx[0], cy[0]), (cx[1], cy[1])}


@pytest.mark.parametrize("name", ["noise97x61_r3_nms8", "noise64x64_r7_nms1", "noise130x70_r1_nms16", "checker2_r7"])
def test_sums_of_every_corner_are_the_trackers(nm, name):
    """nm_klt_sums_host at level 0 gives the sums from which the model's score follows bit for bit"""
    c = next(c for c in CASES if c["name"] == name)
    g = c["grays"][0]
    h, w = g.shape
    want = model(c)[0]
    pyr, _ = nm.gray_pyramid_host([g], levels=1)
    assert want["count"] > 0
    for x, y, s in zip(want["x"], want["y"], want["score"]):
        (Gxx, Gxy, Gyy, _, _, _), flags = nm.klt_sums_host(pyr[0], pyr[0], w, h, 1, 0, c["r"], float(x), float(y), 0.0, 0.0)
        assert flags == 0
        det = K.gate(Gxx, Gxy, Gyy, c["r"], float(F32(c["min_eig"])))
        assert det is not None
        a, b, cc = float(Gxx), float(Gxy), float(Gyy)
        dd = a - cc
        lam = ((a + cc) - np.sqrt(dd * dd + 4.0 * (b * b))) / 2.0
        assert F32(lam / float(1024 * (2 * c["r"] + 1) ** 2)).view(np.uint32) == F32(s).view(np.uint32)


@pytest.mark.parametrize("name", ["noise97x61_r3_nms8", "noise64x64_r7_nms1", "noise130x70_r1_nms16", "noise130x70_r7_nms8",
                                  "checker2_r7", "mask_holes", "square", "min_eig_0", "one_window_r3"])
def test_tracker_calls_no_corner_flat_or_border(nm, name):
    c = next(c for c in CASES if c["name"] == name)
    g = c["grays"][0]
    h, w = g.shape
    got = host_case(nm, c)
    n = int(got["count"][0])
    mask = None if c["mask"] is None else c["mask"].astype(F32)
    pyr, mp = nm.gray_pyramid_host([g], levels=1, mask=mask)
    if n == 0:
        assert name == "one_window_r3"
        return
    t = nm.klt_track_host([pyr[0]], [pyr[0]], w, h, [got["x"][0][:n]], [got["y"][0][:n]], [n], levels=1, radius=c["r"],
                          min_eig=c["min_eig"], mask_pyr=mp)
    assert not np.isin(t.reason[0], (K.FLAT, K.BORDER)).any(), t.reason[0]
    assert (t.reason[0] == 0).all()                                  # a frame against itself: every corner is tracked


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_corners_keep_their_distance(nm, c):
    got = host_case(nm, c, want_plane=False)
    for k, g in enumerate(c["grays"]):
        n = int(got["count"][k])
        x, y = got["x"][k][:n].astype(np.int64), got["y"][k][:n].astype(np.int64)
        d = np.maximum(np.abs(x[:, None] - x[None, :]), np.abs(y[:, None] - y[None, :]))
        d[np.arange(n), np.arange(n)] = 1 << 30
        assert n == 0 or d.min() > c["nms"]
        if c["held"] is not None:
            hx, hy, nH = c["held"][k]
            for px, py in R.held_pixels((hx, hy, nH, len(hx)), g.shape[1], g.shape[0]):
                assert n == 0 or np.maximum(np.abs(x - px), np.abs(y - py)).min() > c["nms"]


def test_frames_do_not_depend_on_n_or_slot(nm):
    c = next(c for c in CASES if c["name"] == "sixty_four_repeated")
    got = host_case(nm, c, want_plane=False)
    one = [host_case(nm, dict(c, grays=[g]), want_plane=False) for g in c["grays"][:3]]
    for k in range(64):
        n = int(one[k % 3]["count"][0])
        assert int(got["count"][k]) == n and int(got["total"][k]) == int(one[k % 3]["total"][0])
        for key in ("x", "y", "score"):
            assert np.array_equal(got[key][k][:n], one[k % 3][key][0][:n])


def refusals(nm):
    """(entry, arguments, change) of every refused call of the two entries"""
    good = np.zeros(16, np.int64).ctypes.data                       # never dereferenced
    tab = lambda n=64: (C.c_void_p * 64)(*([good] * n))
    hole = (C.c_void_p * 64)(*([good] * 2 + [None] + [good] * 61))
    inf, nan = float("inf"), float("nan")
    base = dict(n=3, gray=tab(), fw=97, fh=61, mask=None, held_x=None, held_y=None, d_held=None, cap_held=0, radius=7, nms=8,
                min_eig=1.0, cap=100, x=tab(), y=tab(), score=tab(), d_count=good, d_total=None, score_plane=None)
    held = dict(held_x=tab(), held_y=tab(), d_held=tab(), cap_held=10)
    bad = [dict(n=0), dict(n=65), dict(fw=0), dict(fh=0), dict(fw=32768), dict(fh=32768), dict(radius=0), dict(radius=8), dict(nms=0),
           dict(nms=17), dict(min_eig=-1.0), dict(min_eig=nan), dict(min_eig=inf), dict(cap=0), dict(cap=1 << 22), dict(d_count=None),
           dict(score_plane=hole), dict(held_x=tab()), dict(held_y=tab()), dict(d_held=tab()), dict(held, held_x=None),
           dict(held, held_y=None), dict(held, d_held=None), dict(held, cap_held=0), dict(held, cap_held=1 << 22),
           dict(held, held_x=hole), dict(held, held_y=hole), dict(held, d_held=hole)]
    for name in ("gray", "x", "y", "score"):
        bad += [{name: None}, {name: hole}]
    L = nm.lib()
    for change in bad:
        args = list(dict(base, **change).values())
        yield L.nm_klt_corners_batch_dev_f32, args + [good, None], change
        yield L.nm_klt_corners_host_f32, args, change
    yield L.nm_klt_corners_batch_dev_f32, list(base.values()) + [None, None], "workspace"


def test_every_refusal(nm):
    count = 0
    for fn, args, change in refusals(nm):
        assert fn(*args) == 1, change                               # hipErrorInvalidValue
        count += 1
    assert count == 2 * (28 + 8) + 1
    assert nm.klt_corners_workspace_bytes(0, 97, 61) == 0 and nm.klt_corners_workspace_bytes(65, 97, 61) == 0
    assert nm.klt_corners_workspace_bytes(1, 0, 61) == 0 and nm.klt_corners_workspace_bytes(1, 97, 32768) == 0
    assert nm.klt_corners_workspace_bytes(2, 97, 61) > 2 * 97 * 61 * 4
    assert nm.klt_corners_set_grid_cap(5) == 0 and nm.klt_corners_set_grid_cap(0) == 5
    g = R.noise(1, 97, 61)
    for kw in (dict(radius=0), dict(nms=17), dict(min_eig=-1.0), dict(cap=0), dict(held=([g[0]], [g[0]])), dict(mask=np.ones((3, 3), np.uint8))):
        with pytest.raises(nm.NmError):
            nm.klt_corners_host([g], **kw)


# ---- the benefit: corners + selection against the lattice as the tracker's points (DESIGN.md section 7 has the figures) ----
def benefit(nm, which):
    """(lattice figures, corner figures): share tracked over the points whose windows lie inside both frames under the true
    map, median error, refit corner error; 192 points each"""
    A, B, true, H = K.accuracy_case(which)
    pyr, _ = nm.gray_pyramid_host([A, B], levels=K.ACC["levels"])
    c = nm.klt_corners_host([A], radius=K.ACC["radius"], nms=3, min_eig=1.0, cap=8192)
    n = int(c["count"][0])
    s = nm.sift_select_host([n], [c["x"][0]], [c["y"][0]], K.AW, K.AH, scores=[c["score"][0]], gx=16, gy=12, keep=192)
    m = int(s["count"][0])
    out = []
    for xs, ys in (nm.klt_grid_points(K.AW, K.AH, K.ASTEP), (s["x"][0][:m].copy(), s["y"][0][:m].copy())):
        cnt = len(xs)

        def refit(dst, ok):
            dx, dy = np.where(ok, dst[:, 0], -1).astype(F32), np.where(ok, dst[:, 1], -1).astype(F32)
            mt = np.where(ok, np.arange(cnt), -1).astype(np.int32)
            Hf, _, st, _ = nm.ransac_refit_host(2, [xs], [ys], [cnt], [dx], [dy], [mt], true.astype(F32).reshape(1, 9), rounds=2,
                                                threshold=4.0)
            assert st[0] == 1
            return Hf[0]

        got = nm.klt_track_host([pyr[0]], [pyr[1]], K.AW, K.AH, [xs], [ys], [cnt], H=H, **K.ACC)
        dst = np.c_[got.dst_xs[0], got.dst_ys[0]].astype(np.float64)
        dst[got.matches[0] < 0] = np.nan
        fig = K.accuracy_figures(dst, true, xs, ys, refit)
        inside = K.inside_both(true, xs, ys, K.ACC["radius"])
        fig["points"], fig["inside"] = cnt, int(inside.sum())
        fig["inside_share"] = float(np.isfinite(dst[inside, 0]).mean())
        out.append(fig)
    return out


@pytest.mark.parametrize("which", ["a", "b"])
def test_benefit_figures_on_the_accuracy_cases(nm, which):
    """Measured here, lattice | corners + selection (16 x 12 grid, keep 192; nms 3, the largest that leaves 192 corners on both
    frames; min_eig 1; levels 4, radius 7, fb_max 1, max_residual 6), 192 points each:
      (a) translation, no start: share of all points 0.46875 | 0.48438; of the points whose windows lie inside both frames
          0.64286 (of 140) | 0.57407 (of 162); median 0.01914 | 0.02000 px; refit corner error 0.02756 | 0.08796 px
      (b) roll + perspective:   share 0.56771 | 0.69792; inside 0.93966 (of 116) | 0.97101 (of 138); median 0.06038 | 0.05522 px;
          refit corner error 0.03124 | 0.03097 px
    The corners do NOT track the larger inside share in both cases, so no ordering is asserted. The reason, from the reason
    codes: neither set loses a single row to FLAT on this scene; what (a) loses inside the frames is RESIDUAL (50 lattice rows,
    63 corner rows), the mean absolute difference above 6 gray values after a 9.4 px move without a start map, and that mean
    grows with the window's contrast, which is what the detector selects for. Asserted: the lattice's shares are the
    yardstick's, and the selection delivers 192 points."""
    lattice, corner = benefit(nm, which)
    print(which, "lattice", lattice, "corners", corner)
    assert abs(lattice["share"] - dict(a=0.46875, b=0.56771)[which]) < 1e-5
    assert corner["points"] == lattice["points"] == 192
