"""Homography-guided matching through its host twin (nm_sift_match_guided_host_f32: the device entry's functions, compiled
for the host) against the independent restatement tests/guided_ref.py. No GPU. Both sequences are fully specified in
float32, so equality is exact: no tolerance, no excluded rows.

The real links are views 0-3 of tests/test_gpu_mosaic.py (seed 90, 640 x 480) made with the CPU oracle alone (warp, gray,
detect + describe), with the true pairwise map rounded to float32, radius^2 9, ambiguity 0.8, no distance cap. Figures when
recorded (matches within 1.5 px of the truth):

    link   keypoints A / B   ratio matches (true)   guided matches (true)   guided true / ratio true
    0->1   2528 / 2629       1760 (1603)            2029 (2009)             1.25
    1->2   2629 / 2618       1773 (1609)            2032 (2015)             1.25
    2->3   2618 / 2643       1701 (1543)            1969 (1950)             1.26
"""
import ctypes as C

import numpy as np
import pytest

import guided_ref as G
import ransac_refit_ref as F

R2, AMB = 9.0, 0.8
_links = None


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def real_links(oracle):
    """[(A, B, H float32 (9,), H64)] for links 0->1, 1->2, 2->3; A / B are the oracle's detect-describe results."""
    global _links
    if _links is None:
        import test_gpu_mosaic as M
        scene = M._scene(90)
        maps = M._view_maps()[:4]
        feats = []
        for Ak in maps:
            view, _, _ = oracle.resample_perspective(scene, M.VW, M.VH, np.linalg.inv(Ak).astype(np.float32), inverse=True)
            feats.append(oracle.sift_detect_describe(oracle.grayscale(view), M.CAP))
        _links = []
        for k in range(3):
            Ht = np.linalg.inv(maps[k + 1]) @ maps[k]
            Ht /= Ht[2, 2]
            _links.append((feats[k], feats[k + 1], Ht.astype(np.float32).reshape(9), Ht))
    return _links


def pair_of(fa, fb, H, **kw):
    p = dict(A=fa["desc"], ax=fa["x"], ay=fa["y"], nA=fa["n"], B=fb["desc"], bx=fb["x"], by=fb["y"], nB=fb["n"], H=H, status=1)
    p.update(kw)
    return p


def random_pair(seed, rows_a, rows_b, nA=None, nB=None, side=60.0, status=1, H=None, negative=()):
    """Descriptors of small integers (exact ties), candidates planted as copies of query rows and of each other (min1 = 0,
    min2 = 0), coordinates crowded into side x side pixels so that a gate of a few pixels holds several candidates."""
    rng = np.random.default_rng(seed)
    B = rng.integers(0, 4, (rows_b, 128)).astype(np.float32)
    A = rng.integers(0, 4, (rows_a, 128)).astype(np.float32)
    bx, by = (rng.uniform(0, side, rows_b).astype(np.float32) for _ in range(2))
    ax, ay = (rng.uniform(0, side, rows_a).astype(np.float32) for _ in range(2))
    m = min(rows_a, rows_b)
    for i in range(0, m, 3):                                  # query i sits on candidate i: a true match, often distance 0
        ax[i], ay[i] = bx[i] + np.float32(0.25), by[i] - np.float32(0.5)
        if i % 2 == 0:
            A[i] = B[i]
    for j in range(0, rows_b - 1, 7):                         # twin candidates side by side: min2 == 0 or exact ties
        B[j + 1] = B[j]
        bx[j + 1], by[j + 1] = bx[j] + np.float32(0.5), by[j]
    for i in negative:
        ax[i] = -1.0
    H = np.eye(3, dtype=np.float32).reshape(9) if H is None else np.asarray(H, np.float32).reshape(9)
    return dict(A=A, ax=ax, ay=ay, nA=rows_a if nA is None else nA, B=B, bx=bx, by=by, nB=rows_b if nB is None else nB, H=H,
                status=status)


def host(nm, pairs, radius2=R2, ambiguity=AMB, max_distance=np.inf, capA=None, capB=None):
    k = lambda key: [p[key] for p in pairs]
    return nm.sift_match_guided_host(k("A"), k("ax"), k("ay"), k("nA"), k("B"), k("bx"), k("by"), k("nB"),
                                     np.stack(k("H")), status=np.array(k("status"), np.int32), radius2=radius2,
                                     ambiguity=ambiguity, max_distance=max_distance, capA=capA, capB=capB, want_distance=True)


def assert_equals_restatement(nm, pairs, what, **kw):
    res, cnt, best = host(nm, pairs, **kw)
    kw.setdefault("capB", min(len(p["bx"]) for p in pairs))               # the capacities the wrapper chose
    for k, p in enumerate(pairs):
        want, wcount, wbest = G.guided(p["A"], p["ax"], p["ay"], p["nA"], p["B"], p["bx"], p["by"], p["nB"], p["H"], p["status"],
                                       kw.get("radius2", R2), kw.get("ambiguity", AMB), kw.get("max_distance", np.inf),
                                       capA=res.shape[1], capB=kw.get("capB"))
        diff = np.flatnonzero(res[k] != want)
        assert not len(diff), (what, k, diff[:5], res[k][diff[:5]], want[diff[:5]])
        assert cnt[k] == wcount == (res[k] >= 0).sum(), (what, k)
        assert np.array_equal(_bits(best[k]), _bits(wbest)), (what, k)
    return res, cnt, best


def test_real_links_equal_the_restatement_and_precondition(nm, oracle):
    links = real_links(oracle)
    pairs = [pair_of(fa, fb, H) for fa, fb, H, _ in links]
    assert_equals_restatement(nm, pairs, "real links in one call, clipped to the smallest set")
    for k, (fa, fb, H, H64) in enumerate(links):
        res, cnt, best = (v[0] for v in assert_equals_restatement(nm, [pairs[k]], "real link %d" % k))
        ratio, _, _ = oracle.sift_matches(fa["desc"], fb["desc"], AMB, want_distance=False)
        p = H64 @ np.stack([fa["x"].astype(np.float64), fa["y"].astype(np.float64), np.ones(fa["n"])])
        px, py = p[0] / p[2], p[1] / p[2]

        def true_rows(m):
            rows = np.flatnonzero(m >= 0)
            ok = np.hypot(fb["x"][m[rows]] - px[rows], fb["y"][m[rows]] - py[rows]) < 1.5
            return rows[ok]

        want, _, _ = G.guided(fa["desc"], fa["x"], fa["y"], fa["n"], fb["desc"], fb["x"], fb["y"], fb["n"], H, 1, R2, AMB)
        rt, gt = true_rows(ratio), true_rows(want)
        print("link %d->%d: keypoints %d / %d, ratio matches %d (%d true), guided %d (%d true), %.3f x" % (
            k, k + 1, fa["n"], fb["n"], (ratio >= 0).sum(), len(rt), (want >= 0).sum(), len(gt), len(gt) / len(rt)))
        # the precondition, on the restatement alone: the inputs are worth a guided pass
        assert len(gt) >= 1.15 * len(rt), (k, len(gt), len(rt))
        assert np.array_equal(want[rt], ratio[rt]), "a true ratio match changed its index"
        # every guided match lies inside the gate
        rows = np.flatnonzero(res >= 0)
        assert F.is_inlier32(H, fa["x"][rows], fa["y"][rows], fb["x"][res[rows]], fb["y"][res[rows]], R2).all()
        assert cnt > (ratio >= 0).sum()


def test_a_distance_cap_only_removes_matches(nm, oracle):
    fa, fb, H, _ = real_links(oracle)[0]
    free, _, best = assert_equals_restatement(nm, [pair_of(fa, fb, H)], "no cap")
    cap = float(np.median(best[0][free[0] >= 0]))
    capped, cnt, _ = assert_equals_restatement(nm, [pair_of(fa, fb, H)], "cap", max_distance=cap)
    kept = capped[0] >= 0
    assert 0 < cnt[0] < (free[0] >= 0).sum() and np.array_equal(capped[0][kept], free[0][kept])
    assert (best[0][kept] < cap).all() and (best[0][(free[0] >= 0) & ~kept] >= cap).all()


def test_planted_duplicates_ties_and_degenerate_pairs(nm):
    z0 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 0], np.float32)                 # z = 0 for every row: nothing passes
    zrow = np.array([1, 0, 0, 0, 1, 0, -1.0 / 16, 0, 1], np.float32)       # z = 0 exactly on the line ax = 16
    pairs = [random_pair(1, 300, 280), random_pair(2, 257, 1030, negative=(0, 5, 256)),
             random_pair(3, 64, 120), random_pair(4, 200, 200, status=0), random_pair(5, 200, 200, status=2),
             random_pair(6, 200, 150, nA=0), random_pair(7, 150, 200, nB=0), random_pair(8, 120, 130, nA=10 ** 6, nB=10 ** 6),
             random_pair(9, 120, 130, nA=-4, nB=-1), random_pair(10, 90, 77, nA=31, nB=50), random_pair(11, 100, 100, H=z0),
             random_pair(12, 100, 100, H=zrow)]
    pairs[11]["ax"][:20] = 16.0
    nanH = random_pair(13, 100, 100)
    nanH["H"][3] = np.nan
    pairs.append(nanH)
    capA, capB = min(len(p["ax"]) for p in pairs), min(len(p["bx"]) for p in pairs)
    for p in pairs:                                                      # the wrappers take one capacity per call
        for key in ("A", "ax", "ay"):
            p[key] = p[key][:capA]
        for key in ("B", "bx", "by"):
            p[key] = p[key][:capB]
    res, cnt, best = assert_equals_restatement(nm, pairs, "capacity %d x %d" % (capA, capB), radius2=6.0)
    assert cnt[3] == cnt[4] == cnt[5] == cnt[6] == cnt[10] == cnt[12] == 0 and np.isinf(best[3]).all()
    assert (res[8] == -1).all() and (res[9][31:] == -1).all()
    # at full size, pair by pair, with two radii and a tight ratio; the planted cases do occur
    seen = dict(min2_zero=0, tie=0, min1_zero=0)
    for seed, (ra, rb) in enumerate([(300, 280), (257, 1030), (513, 700), (64, 9)]):
        p = random_pair(20 + seed, ra, rb, negative=(1, 2))
        for r2, amb in ((6.0, 0.8), (30.0, 0.95), (0.5, 0.8), (1e9, 0.8)):
            res, cnt, best = assert_equals_restatement(nm, [p], "seed %d r2 %g" % (seed, r2), radius2=r2, ambiguity=amb)
            assert (res[0][[1, 2]] == -1).all() and np.isinf(best[0][[1, 2]]).all()
            seen["min1_zero"] += int((best[0] == 0).sum())
            seen["min2_zero"] += int(((best[0] == 0) & (res[0] < 0)).sum())
        D = G.O.bf_distance(G.O.transpose(p["A"]), p["B"]).T
        seen["tie"] += int((np.sort(D, axis=1)[:, 0] == np.sort(D, axis=1)[:, 1]).sum())
    assert all(v > 0 for v in seen.values()), seen
    # a radius that admits nothing
    for r2 in (0.0, -1.0):
        res, cnt, _ = assert_equals_restatement(nm, [random_pair(1, 300, 280)], "r2 %g" % r2, radius2=r2)
        assert cnt[0] == 0


def test_a_gate_that_passes_everything_is_the_blind_matcher(nm, oracle):
    eye = np.eye(3, dtype=np.float32).reshape(9)
    for seed, (ra, rb) in enumerate([(300, 280), (90, 513), (64, 1)]):
        p = random_pair(40 + seed, ra, rb)
        for amb in (0.8, 0.95):
            res, cnt, best = host(nm, [p], radius2=1e12, ambiguity=amb)
            want, _, (m1, ix, m2) = oracle.sift_matches(p["A"], p["B"], amb, want_distance=False)
            assert np.array_equal(res[0], want) and np.array_equal(_bits(best[0]), _bits(m1)), (seed, amb)
            assert cnt[0] == (want >= 0).sum()
    fa, fb, _, _ = real_links(oracle)[0]
    sub = lambda f, n: dict(desc=f["desc"][:n], x=f["x"][:n], y=f["y"][:n], n=n)
    res, cnt, _ = host(nm, [pair_of(sub(fa, 700), sub(fb, 650), eye)], radius2=1e12)
    want, _, _ = oracle.sift_matches(fa["desc"][:700], fb["desc"][:650], AMB, want_distance=False)
    assert np.array_equal(res[0], want) and cnt[0] > 50


def test_every_guided_match_is_an_inlier_of_the_map(nm, oracle):
    """ransac_refit_host(rounds = 0, threshold = radius2, matches = guided) counts exactly the guided matches."""
    links = real_links(oracle)
    pairs = [pair_of(fa, fb, H) for fa, fb, H, _ in links] + [random_pair(60, 300, 280), random_pair(61, 200, 200, status=0)]
    for p in pairs:
        res, cnt, _ = host(nm, [p], radius2=R2 if len(p["ax"]) > 1000 else 6.0)
        r2 = R2 if len(p["ax"]) > 1000 else 6.0
        Ho, rc, st, done = nm.ransac_refit_host(2, [p["ax"]], [p["ay"]], [p["nA"]], [p["bx"]], [p["by"]], [res[0]],
                                                p["H"], status=np.array([p["status"]], np.int32), rounds=0, threshold=r2)
        assert rc[0] == cnt[0] and (cnt[0] > 20 or p["status"] != 1)


def test_refusals(nm):
    lib = nm.lib()
    n = 2
    d = np.zeros((8, 128), np.float32)
    x = np.zeros(8, np.float32)
    cnt8 = np.array([8], np.int32)
    H = np.tile(np.eye(3, dtype=np.float32).reshape(9), (n, 1))
    res = np.full((n, 8), 7, np.int32)
    best = np.full((n, 8), 7, np.float32)
    count = np.full(n, 7, np.int32)
    tab = lambda a, k=n: (C.c_void_p * 64)(*([a.ctypes.data] * k))
    rows = lambda a, k=n: (C.c_void_p * 64)(*[a[i].ctypes.data for i in range(k)])
    p = lambda a: a.ctypes.data

    def call(fn, n_=n, capA=8, capB=8, r2=4.0, amb=0.8, maxd=float("inf"), **kw):
        a = dict(A=tab(d), ax=tab(x), ay=tab(x), nA=tab(cnt8), B=tab(d), bx=tab(x), by=tab(x), nB=tab(cnt8), H=p(H),
                 result=rows(res), count=p(count), best=rows(best))
        a.update(kw)
        args = [n_, a["A"], a["ax"], a["ay"], a["nA"], capA, a["B"], a["bx"], a["by"], a["nB"], capB, a["H"], None, r2, amb,
                maxd, a["result"], a["count"], a["best"]]
        return fn(*(args + ([None] if fn is lib.nm_sift_match_guided_batch_dev_f32 else [])))

    assert call(lib.nm_sift_match_guided_host_f32) == 0 and (res == -1).all() and (count == 0).all() and (best == 0).all()
    assert call(lib.nm_sift_match_guided_host_f32, best=None, maxd=float("-inf")) == 0
    res[:], count[:], best[:] = 7, 7, 7
    nan, inf = float("nan"), float("inf")
    bad = [dict(n_=0), dict(n_=-1), dict(n_=65), dict(capA=0), dict(capA=1 << 22), dict(capB=0), dict(capB=1 << 22),
           dict(r2=nan), dict(r2=inf), dict(r2=-inf), dict(amb=nan), dict(amb=inf), dict(amb=-inf), dict(maxd=nan)]
    bad += [dict([(k, None)]) for k in ("A", "ax", "ay", "nA", "B", "bx", "by", "nB", "H", "result", "count")]
    bad += [dict([(k, tab(d if k in "AB" else cnt8 if k in ("nA", "nB") else x, 1))]) for k in
            ("A", "ax", "ay", "nA", "B", "bx", "by", "nB")]
    bad += [dict(result=rows(res, 1)), dict(best=rows(best, 1))]
    for fn in (lib.nm_sift_match_guided_host_f32, lib.nm_sift_match_guided_batch_dev_f32):   # both refuse before touching memory
        for kw in bad:
            assert call(fn, **kw) != 0, (fn.__name__, kw)
    assert (res == 7).all() and (count == 7).all() and (best == 7).all()
    assert "nm_sift_match_guided_batch_dev_f32" in nm.ABI_SYMBOLS and "nm_sift_match_guided_host_f32" in nm.ABI_SYMBOLS


def test_wrapper_checks_and_the_batch_limit(nm):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = int(re.search(r"#define NM_MATCH_GUIDED_MAX_BATCH (\d+)", open(os.path.join(root, "include", "nm_abi.h")).read()).group(1))
    src = open(os.path.join(root, "niftymatch_amd", "csrc", "nm_match_guided.hip")).read()
    slots = int(re.search(r"constexpr int SLOTS = (\d+);", src).group(1))
    assert "static_assert(NM_MATCH_GUIDED_MAX_BATCH == 2 * SLOTS" in src
    assert hdr == 2 * slots == nm.MATCH_GUIDED_MAX_BATCH == 64
    d = np.zeros((8, 128), np.float32)
    x = np.zeros(8, np.float32)
    H = np.eye(3, dtype=np.float32).reshape(1, 9)

    def ok(**kw):
        a = dict(As=[d], axs=[x], ays=[x], nAs=[8], Bs=[d], bxs=[x], bys=[x], nBs=[8], H=H)
        a.update(kw)
        return nm.sift_match_guided_host(a.pop("As"), a.pop("axs"), a.pop("ays"), a.pop("nAs"), a.pop("Bs"), a.pop("bxs"),
                                         a.pop("bys"), a.pop("nBs"), a.pop("H"), **a)

    r = ok()
    assert len(r) == 2 and r[0].shape == (1, 8) and r[0].dtype == np.int32 and len(ok(want_distance=True)) == 3
    assert ok(capA=5)[0].shape == (1, 5)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(radius2=nan), dict(radius2=inf), dict(ambiguity=nan), dict(ambiguity=-inf), dict(max_distance=nan),
               dict(capA=9), dict(capA=0), dict(capB=9), dict(capB=0), dict(H=np.zeros(8, np.float32)),
               dict(status=np.zeros(2, np.int32)), dict(As=[np.zeros((8, 64), np.float32)]), dict(axs=[x, x]),
               dict(bxs=[np.zeros(4, np.float32)], capB=8)):
        with pytest.raises(nm.NmError):
            ok(**kw)
    with pytest.raises(nm.NmError):
        ok(As=[d] * 65, axs=[x] * 65, ays=[x] * 65, nAs=[8] * 65, Bs=[d] * 65, bxs=[x] * 65, bys=[x] * 65, nBs=[8] * 65,
           H=np.zeros((65, 9), np.float32))
    with pytest.raises(nm.NmError):                          # the device wrapper wants device tensors
        import torch
        t, td = torch.zeros(8), torch.zeros(8, 128)
        one = torch.zeros(1, dtype=torch.int32)
        nm.sift_match_guided_batch_dev([td], [t], [t], [one], [td], [t], [t], [one], torch.zeros(9))
