"""The host twins of the gray pyramid and the KLT tracker (nm_gray_pyramid_host_f32, nm_klt_track_host_f32, nm_klt_sums_host)
against the Python model of tests/klt_ref.py, exactly: planes bit for bit, sums word for word, tracks, reasons and counts;
every refusal of the entries (the device entries refuse before any launch or device access, so they are called here with
pointers that are never dereferenced); the fixed-point property; and the accuracy of the stage against a float64
Lucas-Kanade run on views of the loop-closure scene.

A mask cannot cut a window at level 0 and leave the levels above whole (a level's bytes are the erosion of the level below),
so "level 0 only" is the one-level call; with three levels the same hole cuts every level."""
import ctypes as C

import numpy as np
import pytest

import klt_ref as K

F32 = np.float32
CASES = K.cases()


def host_case(nm, c):
    h, w = c["A"].shape
    kw = c["kw"]
    pyr, mp = nm.gray_pyramid_host([c["A"], c["B"]], levels=kw.get("levels", 4), mask=c.get("mask"))
    st = c.get("status")
    xs, ys = K.padded(c)
    return nm.klt_track_host([pyr[0]], [pyr[1]], w, h, [xs], [ys], [c["nA"]], mask_pyr=mp, H=c.get("H"),
                             status=None if st is None else [st], capA=c["capA"], **kw)


@pytest.mark.parametrize("fw,fh,levels", [(97, 61, 4), (64, 64, 4), (97, 61, 1), (33, 2, 1), (5, 7, 2), (130, 70, 6)])
def test_pyramid_planes_equal_the_model(nm, fw, fh, levels):
    g = K.textured(fw * 131 + fh, fw, fh, 0.0, 255.0)
    g[fh // 2, fw // 3] = np.nan
    mask = (K.textured(7, fw, fh, 0.0, 1.0) > 0.25).astype(F32)
    pyr, mp = nm.gray_pyramid_host([g, g[::-1].copy()], levels=levels, mask=mask)
    off = K.offsets(fw, fh, levels)
    assert nm.gray_pyramid_floats(fw, fh, levels) == off[-1] == pyr[0].size == mp.size
    assert [nm.gray_pyramid_offset(fw, fh, l) for l in range(levels + 1)] == off
    assert K.sizes(fw, fh, levels)[1:] == [((fw + (1 << l) - 1) >> l, (fh + (1 << l) - 1) >> l) for l in range(1, levels)]
    for got, src in ((pyr[0], g), (pyr[1], g[::-1])):
        assert np.array_equal(got.view(np.uint32), K.block(K.pyramid(src, levels), F32).view(np.uint32))
    assert np.array_equal(mp, K.block(K.mask_pyramid(mask, levels), np.uint8))
    assert np.array_equal(nm.gray_pyramid_level(pyr[0], fw, fh, 0).view(np.uint32), g.view(np.uint32))


def test_sums_equal_the_model_word_for_word(nm):
    A, B = K.textured(1, 97, 61), K.textured(3, 97, 61)
    levels = 3
    mask = np.ones((61, 97), F32)
    mask[10, 12] = 0
    pyr, mp = nm.gray_pyramid_host([A, B], levels=levels, mask=mask)
    mq = K.mask_pyramid(mask, levels)
    some = 0
    for use_mask in (False, True):
        QA, QB = (K.quantise(K.pyramid(g, levels), mq if use_mask else None) for g in (A, B))
        for r in (1, 3, 7):
            for level in range(levels):
                w, h = K.sizes(97, 61, levels)[level]
                for px, py, dx, dy in ((48.0, 30.0, 0.0, 0.0), (48.5, 30.25, 1.75, -2.5), (40 + 1 / 512, 33 - 1 / 512, -0.3, 0.7),
                                       (14.0, 12.0, 0.5, 0.5), (3.0, 3.0, 0.0, 0.0), (96.0, 60.0, 0.0, 0.0)):
                    s = 1.0 / (1 << level)
                    sums, flags = nm.klt_sums_host(pyr[0], pyr[1], 97, 61, levels, level, r, px, py, dx, dy,
                                                   mask_pyr=mp if use_mask else None)
                    tpl = K.template(QA[level], w, h, F32(px * s), F32(py * s), r)
                    assert (flags & 1) == (tpl is None), (r, level, px, py)
                    if tpl is None:
                        continue
                    assert sums[:3] == tpl[3:6]
                    m = K.mismatch(QB[level], w, h, F32(px * s + dx), F32(py * s + dy), r, tpl)
                    assert bool(flags & 2) == (m is None)
                    if m is not None:
                        assert sums[3:] == m
                        some += 1
    assert some > 40


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_tracks_reasons_and_counts_equal_the_model(nm, c):
    got = host_case(nm, c)
    dst_x, dst_y, matches, count, reason, resid, fb = K.model_case(c)
    assert np.array_equal(got.reason[0], reason), (got.reason[0], reason)
    assert np.array_equal(got.matches[0], matches) and int(got.count[0]) == count
    for g, want in ((got.dst_xs[0], dst_x), (got.dst_ys[0], dst_y), (got.residual[0], resid), (got.fb_error[0], fb)):
        assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), (g, want)


def test_the_cases_reach_every_reason_and_every_gate(nm):
    seen = set()
    for c in CASES:
        seen |= set(host_case(nm, c).reason[0].tolist())
    assert seen == set(range(8)), seen


@pytest.mark.parametrize("levels,shift", [(1, (3, -2)), (1, (0, 0)), (3, (8, -4)), (4, (16, 8))])
def test_whole_pixel_shift_with_an_exact_start_is_a_fixed_point(nm, levels, shift):
    """B(x + s) = A(x) for a whole s that is a multiple of 2^(levels-1), and the start map is that shift: every evaluation
    has e = 0 at every tap (the windows on A and B share their fractional part), so each level ends after one step of zero,
    d stays put and the residual is 0. Points at fractional positions whose sum with s is exact in fp32."""
    fw, fh = 160, 128
    A = K.textured(5, fw, fh)
    B = K.shifted(A, *shift)
    xs = np.array([60, 60.5, 70 + 1 / 512, 80.25, 90 + 255 / 256, 64 + 1 / 256], F32)
    ys = np.array([50, 50.5, 60 - 1 / 512, 64.75, 70 + 1 / 256, 58 + 127 / 256], F32)
    H = np.array([1, 0, shift[0], 0, 1, shift[1], 0, 0, 1], F32)
    pyr, _ = nm.gray_pyramid_host([A, B], levels=levels)
    for r in (3, 7):
        got = nm.klt_track_host([pyr[0]], [pyr[1]], fw, fh, [xs], [ys], [len(xs)], levels=levels, radius=r, iterations=10, H=H,
                                fb_max=0.5)
        assert got.reason[0].tolist() == [0] * len(xs)
        assert np.array_equal(got.dst_xs[0], xs + F32(shift[0])) and np.array_equal(got.dst_ys[0], ys + F32(shift[1]))
        assert not got.residual[0].any() and not got.fb_error[0].any()
        for x, y in zip(xs, ys):
            for level in range(levels):
                s = 1.0 / (1 << level)
                sums, flags = nm.klt_sums_host(pyr[0], pyr[1], fw, fh, levels, level, r, x, y, shift[0] * s, shift[1] * s)
                if flags & 1:                                   # the window does not fit this level's plane: a skipped level
                    assert level > 0 and 2 * (r + 2) + 1 > min(K.sizes(fw, fh, levels)[level]) - 2 * 3
                    continue
                assert flags == 0 and sums[3:] == (0, 0, 0) and sums[0] > 0


def test_pairs_are_independent_and_outputs_hold_nothing_old(nm):
    cs = [c for c in CASES if c["A"].shape == (61, 97) and c["kw"] == dict(levels=3, radius=3, iterations=4) and "H" not in c]
    cap = max(c["capA"] for c in cs)
    pad = lambda v: np.r_[v, np.zeros(max(0, cap - len(v)), F32)][:max(cap, len(v))]
    pyrs = [nm.gray_pyramid_host([c["A"], c["B"]], levels=3)[0] for c in cs]
    got = nm.klt_track_host([p[0] for p in pyrs], [p[1] for p in pyrs], 97, 61, [pad(c["xs"]) for c in cs],
                            [pad(c["ys"]) for c in cs], [min(c["nA"], c["capA"]) for c in cs], capA=cap, levels=3, radius=3, iterations=4)
    for k, c in enumerate(cs):
        want = K.model_case(c)
        m = c["capA"]
        assert np.array_equal(got.reason[k][:m], want[4]) and (got.reason[k][m:] == K.ABSENT).all()
        assert np.array_equal(got.dst_xs[k][:m], want[0]) and int(got.count[k]) == want[3]


def _refusals(nm):
    """(entry, arguments) of every refused call: one table over every argument of the four entries"""
    good = np.zeros(16, np.int64).ctypes.data                       # never dereferenced
    tab = lambda n=64: (C.c_void_p * 64)(*([good] * n))
    hole = (C.c_void_p * 64)(*([good] * 2 + [None] + [good] * 61))
    inf, nan = float("inf"), float("nan")
    pyr = dict(n=3, gray=tab(), fw=97, fh=61, levels=4, pyr=tab(), mask=None, mask_pyr=None)
    bad_pyr = [dict(n=0), dict(n=65), dict(fw=0), dict(fh=32768), dict(levels=0), dict(levels=7), dict(fw=8, levels=4),
               dict(fh=9, levels=5), dict(gray=None), dict(pyr=None), dict(gray=hole), dict(pyr=hole), dict(mask=good),
               dict(mask_pyr=good)]
    trk = dict(n=3, pyrA=tab(), pyrB=tab(), fw=97, fh=61, levels=4, mask_pyr=None, src_x=tab(), src_y=tab(), d_nA=tab(), capA=100,
               H_in=None, status_in=None, radius=7, iterations=10, eps=2.0 ** -6, max_step=16.0, min_eig=0.0, max_residual=0.0,
               fb_max=0.0, dst_x=tab(), dst_y=tab(), matches=tab(), count=good, reason=None, residual=None, fb_error=None)
    bad_trk = [dict(n=0), dict(n=65), dict(fw=0), dict(fh=0), dict(fw=32768), dict(levels=0), dict(levels=7), dict(fw=8), dict(capA=0),
               dict(capA=1 << 22), dict(radius=0), dict(radius=8), dict(iterations=0), dict(iterations=17), dict(eps=0.0),
               dict(eps=-1.0), dict(eps=nan), dict(eps=inf), dict(max_step=0.0), dict(max_step=inf), dict(max_step=nan),
               dict(min_eig=-1.0), dict(min_eig=nan), dict(max_residual=-0.5), dict(max_residual=inf), dict(fb_max=-1.0),
               dict(fb_max=nan), dict(status_in=good), dict(count=None)]
    for name in ("pyrA", "pyrB", "src_x", "src_y", "d_nA", "dst_x", "dst_y", "matches"):
        bad_trk += [{name: None}, {name: hole}]
    for name in ("reason", "residual", "fb_error"):
        bad_trk.append({name: hole})
    L = nm.lib()
    for base, bad, entries in ((pyr, bad_pyr, ((L.nm_gray_pyramid_batch_f32, True), (L.nm_gray_pyramid_host_f32, False))),
                               (trk, bad_trk, ((L.nm_klt_track_batch_dev_f32, True), (L.nm_klt_track_host_f32, False)))):
        for change in bad:
            args = dict(base, **change)
            for fn, stream in entries:
                yield fn, list(args.values()) + ([None] if stream else []), change


def test_every_refusal(nm):
    count = 0
    for fn, args, change in _refusals(nm):
        assert fn(*args) == 1, change                               # hipErrorInvalidValue
        count += 1
    assert count == 2 * (14 + 29 + 16 + 3)
    assert nm.gray_pyramid_floats(8, 97, 4) == 0 and nm.gray_pyramid_floats(97, 61, 7) == 0 and nm.gray_pyramid_floats(16, 16, 4) > 0
    L = nm.lib()
    good = np.zeros(64, np.float32).ctypes.data
    out, fl = np.zeros(6, np.int64).ctypes.data, np.zeros(1, np.int32).ctypes.data
    for args in ((None, good, None, 16, 16, 2, 0, 3, 8., 8., 0., 0., out, fl), (good, good, None, 16, 16, 2, 2, 3, 8., 8., 0., 0., out, fl),
                 (good, good, None, 16, 16, 2, 0, 8, 8., 8., 0., 0., out, fl), (good, good, None, 16, 16, 2, 0, 3, 8., 8., 0., 0., None, fl),
                 (good, good, None, 16, 16, 5, 0, 3, 8., 8., 0., 0., out, fl)):
        assert L.nm_klt_sums_host(*args) == 1
    with pytest.raises(nm.NmError):
        nm.klt_grid_points(64, 64, 0)
    assert nm.klt_set_grid_cap(5) == 0 and nm.klt_set_grid_cap(0) == 5


def test_grid_points(nm):
    xs, ys = nm.klt_grid_points(20, 9, 4)
    assert xs.dtype == F32 and xs.tolist() == [2, 6, 10, 14, 18] * 2 and ys.tolist() == [2] * 5 + [6] * 5
    mask = np.ones((9, 20), F32)
    mask[2, 6] = 0.5
    xs, ys = nm.klt_grid_points(20, 9, 4, mask)
    assert len(xs) == 9 and (6, 2) not in set(zip(xs.tolist(), ys.tolist()))


# ---- accuracy against the float64 Lucas-Kanade yardstick (DESIGN.md section 7 has the measured figures and the margin) ----
MARGIN_PX = 1.0 / 256.0 + 1.0 / 96.0     # the weight phase of two windows (1/512 px each) + levels of 1/16 gray (below 1/96 px)
MARGIN_ROWS = 2             # rows whose gate value lies within the same quantisation of its threshold


def accuracy(nm, which):
    xs, ys = nm.klt_grid_points(K.AW, K.AH, K.ASTEP)
    n = len(xs)
    A, B, true, H = K.accuracy_case(which)

    def refit(dst, ok):
        dx, dy = np.where(ok, dst[:, 0], -1).astype(F32), np.where(ok, dst[:, 1], -1).astype(F32)
        m = np.where(ok, np.arange(n), -1).astype(np.int32)
        Hf, _, st, _ = nm.ransac_refit_host(2, [xs], [ys], [n], [dx], [dy], [m], true.astype(F32).reshape(1, 9), rounds=2, threshold=4.0)
        assert st[0] == 1
        return Hf[0]

    ref = K.lk_float64(K.Params(K.AW, K.AH, **K.ACC), A, B, xs, ys, H)
    pyr, _ = nm.gray_pyramid_host([A, B], levels=K.ACC["levels"])
    got = nm.klt_track_host([pyr[0]], [pyr[1]], K.AW, K.AH, [xs], [ys], [n], H=H, **K.ACC)
    dst = np.c_[got.dst_xs[0], got.dst_ys[0]].astype(np.float64)
    dst[got.matches[0] < 0] = np.nan
    inside = K.inside_both(true, xs, ys, K.ACC["radius"])
    return (K.accuracy_figures(ref, true, xs, ys, refit), K.accuracy_figures(dst, true, xs, ys, refit),
            float(np.isfinite(ref[inside, 0]).mean()), n)


@pytest.mark.parametrize("which", ["a", "b"])
def test_accuracy_against_the_float64_tracker(nm, which):
    """Measured here (float64 yardstick | stage), 192 grid points of step 16 on 256 x 192 views of scene seed 90, levels 4, radius
    7, fb_max 1, max_residual 6: (a) translation (9.4, -6.7), no start: share 0.46875 | 0.46875, median 0.01877 | 0.01914 px,
    p95 0.04697 | 0.04611 px, refit corner error 0.02769 | 0.02756 px; the yardstick tracks 0.643 of the 140 points whose
    window lies inside both frames. (b) roll + perspective, start map 8 px off at the corners: share 0.56771 | 0.56771, median
    0.06063 | 0.06038, p95 0.11393 | 0.11296, corner 0.03130 | 0.03124."""
    ref, got, inside_share, n = accuracy(nm, which)
    print(which, "float64", ref, "stage", got, "yardstick share of inside points", inside_share)
    if which == "a":
        assert inside_share >= 0.5                                  # fixed in advance: else another scene seed
    assert abs(got["share"] - ref["share"]) * n <= MARGIN_ROWS
    for key in ("median", "p95", "corner"):
        assert got[key] <= ref[key] + MARGIN_PX, key
