"""The inlier refit through its host twin (nm_ransac_refit_host_f32: the device entry's functions, compiled for the host)
against a float64 restatement (tests/ransac_refit_ref.py) on the 84 scenes of ransac_ref.sweep. No GPU.

H_in is the first-maximum winner of the CPU oracle's RANSAC on the sweep's sample lists (threshold 4.0).

One-round accuracy: the yardstick e_round is the corner displacement of the float64 reference map rounded to float32; the
limit is 4 x its maximum over the seven motions of a model and frame size. Figures when recorded, in pixels (max over the
motions; the product column is the corner distance between the product's rounds = 1 map and the float64 fit on the same rows):

    model        frame        e_round max   limit (4 x)   product max   scenes compared
    translation  640x480      2.93e-05      1.17e-04      4.42e-07      1
    translation  1920x1080    4.62e-05      1.85e-04      4.62e-05      3
    translation  3840x2160    2.25e-04      9.01e-04      2.04e-05      3
    translation  7680x4320    1.69e-04      6.76e-04      4.04e-05      3
    similarity   640x480      6.39e-05      2.55e-04      6.39e-05      7
    similarity   1920x1080    2.42e-04      9.69e-04      2.42e-04      6
    similarity   3840x2160    5.13e-04      2.05e-03      5.13e-04      7
    similarity   7680x4320    1.05e-03      4.21e-03      1.05e-03      7
    homography   640x480      1.26e-04      5.04e-04      1.26e-04      7
    homography   1920x1080    3.13e-04      1.25e-03      3.13e-04      7
    homography   3840x2160    3.66e-04      1.47e-03      3.66e-04      7
    homography   7680x4320    8.83e-04      3.53e-03      8.83e-04      7

(the product's worst case equals e_round's: its map is the float64 fit rounded once. A translation's first round is accepted
on few scenes: the mean seldom keeps every inlier of a winner that was chosen for its count.)

What the refit is for (rounds = 3, corner distance to the scene's true map, sums over a model's 28 scenes):

    model        sum before   float64 after / before   product after / before   worst single scene, float64 / product
    translation  3.62 px      0.791                    0.791                    1.000 / 1.000
    similarity   13.7 px      0.205                    0.205                    1.000 / 1.000
    homography   48.3 px      0.133                    0.133                    0.307 / 0.307
"""
import numpy as np
import pytest

import ransac_ref as R
import ransac_refit_ref as F

MODELS = [0, 1, 2]
NAMES = {0: "translation", 1: "similarity", 2: "homography"}
THR = R.SWEEP_THR
_cache = {}


def _pts(sc):
    return sc["sx"], sc["sy"], sc["dx"], sc["dy"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def scenes(oracle, model, W, Hh):
    """[(motion, scene, H_in float32 (9,), oracle's best count)] of one model and frame size, computed once."""
    key = (model, W, Hh)
    if key not in _cache:
        out = []
        for motion, sc, rl in R.sweep(model, W, Hh):
            pos, Hb, Ha, inl = oracle.ransac(model, *_pts(sc), rl, THR)
            assert int(pos) == int(np.argmax(inl))
            out.append((motion, sc, np.asarray(Hb, np.float32).copy(), int(inl[int(pos)])))
        _cache[key] = out
    return _cache[key]


def refit(nm, model, pts, H, rounds, thr=THR, matches=None, nA=None, status=None, capA=None):
    """One pair through the host twin; returns a dict of its outputs."""
    sx, sy, dx, dy = pts
    m = np.arange(len(sx), dtype=np.int32) if matches is None else np.asarray(matches, np.int32)
    nA = len(sx) if nA is None else nA
    Ho, cnt, st, done, mask, rms = nm.ransac_refit_host(model, [sx], [sy], [nA], [dx], [dy], [m], np.asarray(H, np.float32),
                                                        status=status, rounds=rounds, threshold=thr, capA=capA,
                                                        want_mask=True, want_rms=True)
    return dict(H=Ho[0], count=int(cnt[0]), status=int(st[0]), done=int(done[0]), mask=mask[0], rms=float(rms[0]))


@pytest.mark.parametrize("W,Hh", R.FRAMES)
@pytest.mark.parametrize("model", MODELS)
def test_rounds_0_is_the_count_and_mask_of_the_input_map(nm, oracle, model, W, Hh):
    for motion, sc, Hin, best in scenes(oracle, model, W, Hh):
        pts = _pts(sc)
        r = refit(nm, model, pts, Hin, 0)
        replay = F.valid_rows(sc["sx"]) & F.is_inlier32(Hin, *pts, THR)
        lo, hi, _, _ = R.inlier_bracket64(Hin.reshape(1, 9), *pts, THR)
        print("%s %dx%d %-11s count %d  replay %d  oracle %d  bracket [%d, %d]" % (NAMES[model], W, Hh, motion, r["count"],
                                                                                   replay.sum(), best, lo[0], hi[0]))
        assert r["status"] == 1 and r["done"] == 0
        assert r["count"] == int(replay.sum()) == best, motion
        assert lo[0] <= r["count"] <= hi[0], motion
        assert np.array_equal(r["mask"], replay.astype(np.uint8)), motion
        assert int(r["mask"].sum()) == r["count"]
        assert np.array_equal(_bits(r["H"]), _bits(Hin)), motion
        d2 = F.d2_64(Hin.astype(np.float64), *pts)[replay]
        assert abs(r["rms"] - np.sqrt(d2.mean())) <= 1e-6 * max(1.0, np.sqrt(d2.mean())), motion


def test_rounds_0_mask_outside_the_valid_rows(nm, oracle):
    """Bytes are 0 for unmatched rows, for rows of -1 (align_points' convention) and beyond nA, and all capA bytes are written."""
    for model in MODELS:
        sc = R.scene(model, 1920, 1080, 600, 0.3, 0.5, 17 + model, "mild", unmatched=(3, 77, 400))
        pts = _pts(sc)
        m = np.arange(600, dtype=np.int32)
        m[[5, 9, 333]] = -1
        Hin = sc["M"].astype(np.float32).reshape(9)
        nA = 450
        r = refit(nm, model, pts, Hin, 0, matches=m, nA=nA)
        valid = F.valid_rows(sc["sx"], m, nA)
        want = valid & F.is_inlier32(Hin, *pts, THR)
        assert r["mask"].shape == (600,) and np.array_equal(r["mask"], want.astype(np.uint8))
        assert not r["mask"][[3, 77, 400, 5, 9, 333]].any() and not r["mask"][nA:].any() and r["count"] == want.sum() > 100
        for bad_nA, rows in ((-5, 0), (10 ** 6, 600)):                  # the size is clamped to [0, capA]
            r = refit(nm, model, pts, Hin, 0, matches=m, nA=bad_nA)
            assert r["count"] == (F.valid_rows(sc["sx"], m, rows) & F.is_inlier32(Hin, *pts, THR)).sum()


@pytest.mark.parametrize("W,Hh", R.FRAMES)
@pytest.mark.parametrize("model", MODELS)
def test_one_round_against_float64(nm, oracle, model, W, Hh):
    e_round, got, compared = [], [], 0
    for motion, sc, Hin, _ in scenes(oracle, model, W, Hh):
        pts = _pts(sc)
        S = refit(nm, model, pts, Hin, 0)["mask"].astype(bool)
        H64 = F.fit64(model, *(a[S] for a in pts))
        e_round.append(F.rounding_error(H64, W, Hh))
        r = refit(nm, model, pts, Hin, 1)
        if r["done"] == 1:
            got.append((motion, F.corner_error(r["H"], H64, W, Hh)))
            compared += 1
    limit = 4.0 * max(e_round)
    for motion, e in got:
        print("%s %dx%d %-11s product vs float64 fit %.3g px (limit %.3g, e_round max %.3g)" % (NAMES[model], W, Hh, motion, e,
                                                                                               limit, max(e_round)))
    print("%s %dx%d: e_round max %.3g  limit %.3g  product max %.3g over %d scenes" % (
        NAMES[model], W, Hh, max(e_round), limit, max(e for _, e in got), compared))
    # the translation's mean seldom keeps every inlier of a winner that was chosen for its count: its first round is
    # accepted on few scenes; the other two models gain inliers almost everywhere
    assert compared >= (1 if model == 0 else 5), "too few scenes accepted their first round: %d" % compared
    for motion, e in got:
        assert e <= limit, (motion, e, limit)


@pytest.mark.parametrize("W,Hh", R.FRAMES)
@pytest.mark.parametrize("model", MODELS)
def test_round_rule(nm, oracle, model, W, Hh):
    for motion, sc, Hin, _ in scenes(oracle, model, W, Hh):
        pts = _pts(sc)
        base = refit(nm, model, pts, Hin, 0)
        prev = base
        for rounds in range(1, 5):
            r = refit(nm, model, pts, Hin, rounds)
            assert r["status"] == 1 and r["done"] <= rounds and r["count"] >= base["count"], (motion, rounds)
            assert r["count"] >= prev["count"] and r["done"] >= prev["done"], (motion, rounds)
            assert int(r["mask"].sum()) == r["count"]
            if r["done"] == 0:
                assert np.array_equal(_bits(r["H"]), _bits(Hin)), (motion, rounds)
            prev = r
        # 1 + 3 rounds in two calls = 4 rounds in one
        first = refit(nm, model, pts, Hin, 1)
        second = refit(nm, model, pts, first["H"], 3)
        for k in ("count", "rms"):
            assert second[k] == prev[k], (motion, k)
        assert np.array_equal(_bits(second["H"]), _bits(prev["H"])) and np.array_equal(second["mask"], prev["mask"]), motion
        assert first["done"] + second["done"] == prev["done"], motion


@pytest.mark.parametrize("model", MODELS)
def test_the_refit_brings_the_map_closer_to_the_truth(nm, oracle, model):
    before, ref, got = [], [], []
    for W, Hh in R.FRAMES:
        for motion, sc, Hin, _ in scenes(oracle, model, W, Hh):
            pts = _pts(sc)
            H64, _, _ = F.refit64(model, *pts, Hin, THR, 3)
            r = refit(nm, model, pts, Hin, 3)
            before.append(F.corner_error(Hin, sc["M"], W, Hh))
            ref.append(F.corner_error(H64, sc["M"], W, Hh))
            got.append(F.corner_error(r["H"], sc["M"], W, Hh))
            print("%s %dx%d %-11s before %.3g  float64 %.3g  product %.3g px  (rounds %d, count %d)" % (
                NAMES[model], W, Hh, motion, before[-1], ref[-1], got[-1], r["done"], r["count"]))
    before, ref, got = np.array(before), np.array(ref), np.array(got)
    factor = 1.0 if model == 0 else 0.5
    print("%s: sum before %.4g px; after / before: float64 %.3f, product %.3f; worst scene: float64 %.3f, product %.3f" % (
        NAMES[model], before.sum(), ref.sum() / before.sum(), got.sum() / before.sum(), (ref / before).max(), (got / before).max()))
    for name, after in (("the float64 restatement", ref), ("the product", got)):
        assert np.isfinite(after).all(), name
        assert after.sum() <= factor * before.sum(), (name, after.sum(), before.sum())
        if model == 2:
            assert (after <= 0.5 * before).all(), (name, float((after / before).max()))


@pytest.mark.parametrize("model", MODELS)
def test_degenerate_inputs(nm, model):
    sc = R.scene(model, 1920, 1080, 400, 0.3, 0.5, 99 + model, "mild")
    pts = _pts(sc)
    Hin = sc["M"].astype(np.float32).reshape(9)
    good = refit(nm, model, pts, Hin, 2)
    assert good["status"] == 1 and good["count"] > 200 and np.isfinite(good["H"]).all()

    def assert_zero(r, what):
        assert r["status"] == 0 and r["count"] == 0 and r["done"] == 0 and r["rms"] == 0.0, what
        assert not r["H"].any() and not r["mask"].any(), what

    assert_zero(refit(nm, model, pts, Hin, 2, status=np.array([0], np.int32)), "status_in = 0")
    assert_zero(refit(nm, model, pts, Hin, 2, status=np.array([2], np.int32)), "status_in = 2")
    for q in range(9):
        for v in (np.nan, np.inf, -np.inf):
            Hb = Hin.copy()
            Hb[q] = v
            assert_zero(refit(nm, model, pts, Hb, 2), "H_in[%d] = %r" % (q, v))

    def assert_unchanged(r, what, count=None):
        assert r["status"] == 1 and r["done"] == 0 and np.array_equal(_bits(r["H"]), _bits(Hin)), what
        assert int(r["mask"].sum()) == r["count"], what
        if count is not None:
            assert r["count"] == count and (count > 0 or r["rms"] == 0.0), what

    # zero valid rows: nA = 0, nothing matched, every row -1
    assert_unchanged(refit(nm, model, pts, Hin, 3, nA=0), "nA = 0", 0)
    assert_unchanged(refit(nm, model, pts, Hin, 3, matches=np.full(400, -1, np.int32)), "no matches", 0)
    neg = tuple(np.full(400, -1, np.float32) for _ in range(4))
    assert_unchanged(refit(nm, model, neg, Hin, 3), "all rows -1", 0)
    # fewer inliers than the model's minimum
    if model > 0:
        keep = np.flatnonzero(F.is_inlier32(Hin, *pts, THR))[:F.MIN_INLIERS[model] - 1]
        m = np.full(400, -1, np.int32)
        m[keep] = keep
        assert_unchanged(refit(nm, model, pts, Hin, 3, matches=m), "below the minimum", len(keep))
    # thresholds: <= 0 counts nothing, FLT_MAX counts every valid row with a finite distance
    for thr in (0.0, -1.0):
        assert_unchanged(refit(nm, model, pts, Hin, 3, thr=thr), "thr = %r" % thr, 0)
    r = refit(nm, model, pts, Hin, 2, thr=R.FLT_MAX)
    assert r["status"] == 1 and np.isfinite(r["H"]).all() and r["count"] == 400 and int(r["mask"].sum()) == 400
    # all inlier sources on one line (homography: the null space is not unique): finite or rejected
    t = np.linspace(0, 1, 300)
    lx, ly = (100 + 1500 * t).astype(np.float32), (50 + 900 * t).astype(np.float32)
    ldx, ldy = R.apply64(sc["M"], lx, ly)
    r = refit(nm, model, (lx, ly, ldx.astype(np.float32), ldy.astype(np.float32)), Hin, 4)
    assert r["status"] == 1 and np.isfinite(r["H"]).all() and r["count"] >= 290 and int(r["mask"].sum()) == r["count"]
    # every source and destination identical: no scale to normalise by
    one = tuple(np.full(50, v, np.float32) for v in (512, 256)) + tuple(
        np.full(50, np.float32(v)) for v in R.apply64(sc["M"], 512.0, 256.0))
    r = refit(nm, model, one, Hin, 4)
    assert r["status"] == 1 and np.isfinite(r["H"]).all() and r["count"] == 50
    if model > 0:
        assert r["done"] == 0 and np.array_equal(_bits(r["H"]), _bits(Hin))


@pytest.mark.parametrize("model", MODELS)
def test_catalogue_rows_with_non_finite_coordinates(nm, oracle, model):
    """ransac_ref.catalogue's point lists (coincident, collinear, horizon rows, NaN / +-inf coordinates, thr 0 / FLT_MAX / -1):
    the result is a usable finite map whose count never falls, and a non-finite coordinate changes nothing else."""
    cases, _ = R.catalogue(model)
    clean = None
    for name, pts, rl, thr, base in cases:
        pos, Hb, Ha, inl = oracle.ransac(model, *pts, rl, 4.0)
        Hin = np.asarray(Hb, np.float32)
        r0 = refit(nm, model, pts, Hin, 0, thr=thr)
        r = refit(nm, model, pts, Hin, 3, thr=thr)
        replay = F.valid_rows(pts[0]) & F.is_inlier32(Hin, *pts, thr)
        assert r0["count"] == replay.sum() and np.array_equal(r0["mask"], replay.astype(np.uint8)), name
        assert r["status"] == 1 and np.isfinite(r["H"]).all() and r["count"] >= r0["count"], name
        assert int(r["mask"].sum()) == r["count"] and np.isfinite(r["rms"]), name
        if name == "all together":
            clean = r
        if "[" in name:                                     # the spare row is an outlier of every map
            assert np.array_equal(_bits(r["H"]), _bits(clean["H"])) and r["count"] == clean["count"], name
            assert not r["mask"][226], name


def test_refusals(nm):
    import ctypes as C
    lib = nm.lib()
    n = 2
    sx = np.zeros(8, np.float32)
    mt = np.zeros(8, np.int32)
    nA = np.array([8], np.int32)
    H = np.tile(np.eye(3, dtype=np.float32).reshape(9), (n, 1))
    Ho = np.full((n, 9), 7, np.float32)
    cnt, st, done = (np.full(n, 7, np.int32) for _ in range(3))
    tab = lambda a, k=n: (C.c_void_p * 64)(*([a.ctypes.data] * k))
    p = lambda a: a.ctypes.data

    def call(fn, model=2, n_=n, capA=8, thr=4.0, rounds=2, **kw):
        a = dict(src_x=tab(sx), src_y=tab(sx), nA=tab(nA), dst_x=tab(sx), dst_y=tab(sx), matches=tab(mt), H_in=p(H),
                 H_out=p(Ho), count=p(cnt), status=p(st), done=p(done))
        a.update(kw)
        args = [model, n_, a["src_x"], a["src_y"], a["nA"], capA, a["dst_x"], a["dst_y"], a["matches"], a["H_in"], None, thr,
                rounds, a["H_out"], a["count"], a["status"], a["done"], None, None]
        return fn(*(args + ([None] if fn is lib.nm_ransac_refit_batch_dev_f32 else [])))

    assert call(lib.nm_ransac_refit_host_f32) == 0 and (st == 1).all()
    Ho[:], cnt[:], st[:], done[:] = 7, 7, 7, 7
    bad = [dict(model=-1), dict(model=3), dict(n_=0), dict(n_=65), dict(rounds=-1), dict(rounds=5), dict(capA=0),
           dict(capA=1 << 22), dict(thr=float("nan")), dict(thr=float("inf")), dict(thr=float("-inf"))]
    bad += [dict([(k, None)]) for k in ("src_x", "src_y", "nA", "dst_x", "dst_y", "matches", "H_in", "H_out", "count", "status", "done")]
    bad += [dict([(k, tab(sx if k != "matches" else mt, 1))]) for k in ("src_x", "src_y", "nA", "dst_x", "dst_y", "matches")]
    for fn in (lib.nm_ransac_refit_host_f32, lib.nm_ransac_refit_batch_dev_f32):       # both refuse before touching memory
        for kw in bad:
            assert call(fn, **kw) != 0, (fn.__name__, kw)
    assert (Ho == 7).all() and (cnt == 7).all() and (st == 7).all() and (done == 7).all()
    assert "nm_ransac_refit_batch_dev_f32" in nm.ABI_SYMBOLS and "nm_ransac_refit_host_f32" in nm.ABI_SYMBOLS


def test_wrapper_checks(nm):
    sx = np.zeros(8, np.float32)
    mt = np.arange(8, dtype=np.int32)
    H = np.eye(3, dtype=np.float32).reshape(1, 9)
    ok = lambda **kw: nm.ransac_refit_host(kw.pop("model", 2), [sx], [sx], [8], [sx], [sx], [kw.pop("mt", mt)],
                                           kw.pop("H", H), **kw)
    assert len(ok()) == 4 and len(ok(want_mask=True)) == 5 and len(ok(want_mask=True, want_rms=True)) == 6
    assert ok(want_mask=True)[4].shape == (1, 8) and ok(capA=5, want_mask=True)[4].shape == (1, 5)
    for kw in (dict(model=3), dict(rounds=5), dict(rounds=-1), dict(rounds=1.5), dict(threshold=float("nan")),
               dict(threshold=float("inf")), dict(capA=9), dict(capA=0), dict(H=np.zeros(8, np.float32)),
               dict(status=np.zeros(2, np.int32)), dict(mt=np.full(8, 8, np.int32))):
        with pytest.raises(nm.NmError):
            ok(**kw)
    with pytest.raises(nm.NmError):
        nm.ransac_refit_host(2, [sx, sx], [sx], [8], [sx], [sx], [mt], H)
    with pytest.raises(nm.NmError):
        nm.ransac_refit_host(2, [sx] * 65, [sx] * 65, [8] * 65, [sx] * 65, [sx] * 65, [mt] * 65, np.zeros((65, 9), np.float32))
    with pytest.raises(nm.NmError):                          # the device wrapper wants device tensors
        import torch
        t = torch.zeros(8)
        nm.ransac_refit_batch_dev(2, [t], [t], [torch.zeros(1, dtype=torch.int32)], [t], [t],
                                  [torch.zeros(8, dtype=torch.int32)], torch.zeros(9))
