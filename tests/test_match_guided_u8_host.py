"""Homography-guided matching of unsigned-char descriptors through its host twin (nm_sift_match_guided_u8_host: the device
entry's functions, compiled for the host) against the independent restatement tests/guided_u8_ref.py, against the fp32 host
twin on float copies of the same bytes and against the u8 matcher. No GPU. Distances are exact integers and every other step
is fully specified in float32, so equality is exact: array_equal on results and counts and on the uint32 views of the best
distances, no tolerance, no excluded rows.

The real links are those of tests/test_match_guided_host.py (views 0-3 of tests/test_gpu_mosaic.py, seed 90, 640 x 480, CPU
oracle alone), their descriptors finished to u8 with desc_finish_host (L2), the true pairwise map rounded to float32,
radius^2 9, ambiguity 0.8, no distance cap; blind = sift_match_u8_host on the same bytes. Figures when recorded (matches
within 1.5 px of the truth; the fp32 figures of the same links are 1.25 / 1.25 / 1.26):

    link   keypoints A / B   blind u8 matches (true)   guided u8 matches (true)   guided true / blind true
    0->1   2528 / 2629       1760 (1631)               2029 (2013)                1.23
    1->2   2629 / 2618       1758 (1635)               2030 (2015)                1.23
    2->3   2618 / 2643       1711 (1573)               1972 (1951)                1.24
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import guided_u8_ref as G8
from test_match_guided_host import real_links

R2, AMB = 9.0, 0.8
EYE = np.eye(3, dtype=np.float32).reshape(9)
SIZES = [(1, 1), (5, 9), (70, 37), (300, 1030)]
_links8 = None


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def byte_pair(seed, rows_a, rows_b, top, nA=None, nB=None, side=60.0, status=1, H=None, negative=()):
    """test_match_guided_host.random_pair on bytes 0 .. top: candidates planted as copies of query rows and of each other
    (min1 = 0, min2 = 0, exact ties), coordinates crowded into side x side pixels so that a gate of a few pixels holds
    several candidates, ax = -1 on the rows `negative`."""
    rng = np.random.default_rng(seed)
    B = rng.integers(0, top + 1, (rows_b, 128)).astype(np.uint8)
    A = rng.integers(0, top + 1, (rows_a, 128)).astype(np.uint8)
    bx, by = (rng.uniform(0, side, rows_b).astype(np.float32) for _ in range(2))
    ax, ay = (rng.uniform(0, side, rows_a).astype(np.float32) for _ in range(2))
    for i in range(0, min(rows_a, rows_b), 3):                # query i sits on candidate i: a true match, often distance 0
        ax[i], ay[i] = bx[i] + np.float32(0.25), by[i] - np.float32(0.5)
        if i % 2 == 0:
            A[i] = B[i]
    for j in range(0, rows_b - 1, 7):                         # twin candidates side by side: min2 == 0 or exact ties
        B[j + 1] = B[j]
        bx[j + 1], by[j + 1] = bx[j] + np.float32(0.5), by[j]
    for i in negative:
        ax[i] = -1.0
    H = EYE.copy() if H is None else np.asarray(H, np.float32).reshape(9)
    return dict(A=A, ax=ax, ay=ay, nA=rows_a if nA is None else nA, B=B, bx=bx, by=by, nB=rows_b if nB is None else nB, H=H,
                status=status)


def _call(fn, pairs, floats, radius2=R2, ambiguity=AMB, max_distance=np.inf, capA=None, capB=None):
    k = lambda key: [p[key] for p in pairs]
    d = (lambda key: [p[key].astype(np.float32) for p in pairs]) if floats else k
    return fn(d("A"), k("ax"), k("ay"), k("nA"), d("B"), k("bx"), k("by"), k("nB"), np.stack(k("H")),
              status=np.array(k("status"), np.int32), radius2=radius2, ambiguity=ambiguity, max_distance=max_distance,
              capA=capA, capB=capB, want_distance=True)


def host8(nm, pairs, **kw):
    return _call(nm.sift_match_guided_u8_host, pairs, False, **kw)


def host32(nm, pairs, **kw):
    """The fp32 host twin on float copies of the bytes."""
    return _call(nm.sift_match_guided_host, pairs, True, **kw)


def assert_equals_restatement(nm, pairs, what, fp32=True, **kw):
    """The u8 host twin against guided_u8_ref pair by pair and, with fp32, against the fp32 host twin on float copies."""
    res, cnt, best = host8(nm, pairs, **kw)
    capB = kw.get("capB") or min(len(p["bx"]) for p in pairs)              # the capacities the wrapper chose
    for k, p in enumerate(pairs):
        want, wcount, wbest = G8.guided(p["A"], p["ax"], p["ay"], p["nA"], p["B"], p["bx"], p["by"], p["nB"], p["H"],
                                        p["status"], kw.get("radius2", R2), kw.get("ambiguity", AMB),
                                        kw.get("max_distance", np.inf), capA=res.shape[1], capB=capB)
        assert np.array_equal(res[k], want), (what, k, np.flatnonzero(res[k] != want)[:5])
        assert cnt[k] == wcount == (res[k] >= 0).sum(), (what, k)
        assert np.array_equal(_bits(best[k]), _bits(wbest)), (what, k)
    if fp32:
        r32, c32, b32 = host32(nm, pairs, **kw)
        assert np.array_equal(res, r32) and np.array_equal(cnt, c32) and np.array_equal(_bits(best), _bits(b32)), (what, "fp32")
    return res, cnt, best


@pytest.mark.parametrize("top", [3, 255])
def test_host_twin_equals_the_restatement_and_the_fp32_twin(nm, top):
    seen = dict(min1_zero=0, min2_zero=0, tie=0, matched=0)
    for s, (ra, rb) in enumerate(SIZES):
        p = byte_pair(100 * top + s, ra, rb, top, negative=(1, 2) if ra > 2 else ())
        for r2, amb, maxd in ((6.0, 0.8, np.inf), (30.0, 0.95, np.inf), (0.5, 0.8, np.inf), (1e9, 0.8, np.inf),
                              (30.0, 0.95, 150.0 if top == 3 else 4e5)):
            if r2 == 1e9 and ra * rb > 10000:
                continue                                              # the restatement's scan is a Python loop
            res, cnt, best = assert_equals_restatement(nm, [p], "top %d %dx%d r2 %g" % (top, ra, rb, r2), radius2=r2,
                                                       ambiguity=amb, max_distance=maxd)
            if ra > 2:
                assert (res[0][[1, 2]] == -1).all() and np.isinf(best[0][[1, 2]]).all()
            seen["min1_zero"] += int((best[0] == 0).sum())
            seen["min2_zero"] += int(((best[0] == 0) & (res[0] < 0)).sum())
            seen["matched"] += int(cnt[0])
        if ra * rb <= 70 * 37:
            D = np.sort(G8.distances(p["A"], p["B"]), axis=1)
            seen["tie"] += int((D[:, 0] == D[:, 1]).sum()) if rb > 1 else 0
    assert all(v > 0 for v in seen.values()), seen
    # several pairs in one call, clipped to the smallest capacity; a radius that admits nothing
    pairs = [byte_pair(7 * top + s, ra, rb, top) for s, (ra, rb) in enumerate([(70, 37), (90, 200), (75, 40)])]
    capA, capB = 70, 37
    for p in pairs:
        for key, cap in (("A", capA), ("ax", capA), ("ay", capA), ("B", capB), ("bx", capB), ("by", capB)):
            p[key] = p[key][:cap]
        p["nA"], p["nB"] = min(p["nA"], capA), min(p["nB"], capB)
    assert_equals_restatement(nm, pairs, "three pairs", radius2=20.0)
    for r2 in (0.0, -1.0):
        _, cnt, _ = assert_equals_restatement(nm, pairs[:1], "r2 %g" % r2, radius2=r2)
        assert cnt[0] == 0


D_MAX = 128 * 255 * 255
# (byte of the query row, bytes of the candidates it sees in ascending j, result as a local index or -1 at ambiguity 0.8)
EXTREME_ROWS = ((255, (0,), 0), (255, (0, 0), -1), (255, (255,), 0), (0, (0, 0), -1), (0, (255,), 0), (255, (0, 255), 1),
                (255, (255, 0), 0), (0, (255, 0, 255), 1), (255, (0, 254), 1), (7, (7, 7, 7), -1), (0, (255, 255, 255, 255, 255), -1))


def extreme_pair():
    """Rows of one byte value against candidates of one byte value, each row alone on a point 100 px from the next with its
    candidates on that point: d is 0, 128, or 128 * 255^2 = 8 323 200, the largest value there is."""
    A = np.zeros((len(EXTREME_ROWS), 128), np.uint8)
    ax = 100.0 * np.arange(len(EXTREME_ROWS), dtype=np.float32)
    ay = np.full(len(EXTREME_ROWS), 50.0, np.float32)
    B, bx, by, first = [], [], [], []
    for i, (a, bs, _) in enumerate(EXTREME_ROWS):
        A[i] = a
        first.append(len(B))
        for b in bs:
            B.append(np.full(128, b, np.uint8))
            bx.append(ax[i] + 1.0)
            by.append(ay[i])
    p = dict(A=A, ax=ax, ay=ay, nA=len(A), B=np.stack(B), bx=np.array(bx, np.float32), by=np.array(by, np.float32), nB=len(B),
             H=EYE.copy(), status=1)
    want = np.array([f + loc if loc >= 0 else -1 for f, (_, _, loc) in zip(first, EXTREME_ROWS)], np.int32)
    best = np.array([min(128 * (a - b) ** 2 for b in bs) for a, bs, _ in EXTREME_ROWS], np.float32)
    return p, want, best


def test_extremes_the_largest_distance_is_exact(nm):
    p, want, wbest = extreme_pair()
    res, cnt, best = assert_equals_restatement(nm, [p], "extremes")
    assert np.array_equal(res[0], want) and np.array_equal(_bits(best[0]), _bits(wbest)) and cnt[0] == (want >= 0).sum()
    assert best[0][0] == best[0][1] == D_MAX == 8323200 and best[0][2] == 0 and best[0][8] == 128
    # the same rows under a gate that passes everything: every distance of the table meets every scan
    res, cnt, best = assert_equals_restatement(nm, [p], "extremes, open gate", radius2=1e30)
    assert set(np.unique(best[0]).tolist()) == {0.0}


@pytest.mark.parametrize("top", [3, 255])
def test_a_gate_that_passes_everything_is_the_u8_matcher(nm, top):
    for s, (ra, rb) in enumerate([(300, 280), (90, 513), (64, 1), (1, 1), (5, 9)]):
        p = byte_pair(40 + s + top, ra, rb, top)
        for amb in (0.8, 0.95):
            res, cnt, best = host8(nm, [p], radius2=1e30, ambiguity=amb)
            want = nm.sift_match_u8_host([p["A"]], [ra], [p["B"]], [rb], ambiguity=amb, prior=-1)
            assert np.array_equal(res, want) and cnt[0] == (want >= 0).sum(), (top, s, amb)
            assert np.array_equal(_bits(best[0]), _bits(G8.distances(p["A"], p["B"]).min(axis=1)))
            r32, c32, b32 = host32(nm, [p], radius2=1e30, ambiguity=amb)
            assert np.array_equal(res, r32) and np.array_equal(cnt, c32) and np.array_equal(_bits(best), _bits(b32))
    assert cnt[0] > 0


def unusable_pairs(top, rows_a=100, rows_b=110):
    """One usable pair and every kind that is not, or that has rows without candidates; all of rows_a x rows_b rows."""
    z0 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 0], np.float32)                 # z = 0 for every row: nothing passes
    zrow = np.array([1, 0, 0, 0, 1, 0, -1.0 / 16, 0, 1], np.float32)       # z = 0 exactly on the line ax = 16
    mk = lambda seed, **kw: byte_pair(seed + top, rows_a, rows_b, top, **kw)
    pairs = [mk(1, negative=(0, 5)), mk(2, status=0), mk(3, status=2), mk(4, status=-1), mk(5, nA=0), mk(6, nB=0),
             mk(7, nA=10 ** 6, nB=10 ** 6), mk(8, nA=-4, nB=-1), mk(9, nA=31, nB=50), mk(10, H=z0), mk(11, H=zrow)]
    pairs[10]["ax"][:20] = 16.0
    for q, bad in ((3, np.nan), (8, np.inf), (0, -np.inf)):
        p = mk(12 + q)
        p["H"][q] = bad
        pairs.append(p)
    return pairs


@pytest.mark.parametrize("top", [3, 255])
def test_unusable_pairs_and_rows_without_candidates(nm, top):
    pairs = unusable_pairs(top)
    res, cnt, best = assert_equals_restatement(nm, pairs, "unusable kinds", radius2=6.0)
    assert cnt[0] > 0 and cnt[6] > 0 and cnt[8] > 0
    for k in (1, 2, 3, 4, 5, 7, 9, 11, 12, 13):
        assert cnt[k] == 0 and (res[k] == -1).all() and np.isposinf(best[k]).all(), k
    assert (res[8][31:] == -1).all() and np.isposinf(best[8][31:]).all() and res[8].max() < 50
    assert (res[10][:20] == -1).all() and np.isposinf(best[10][:20]).all()
    assert (res[0][[0, 5]] == -1).all() and np.isposinf(best[0][[0, 5]]).all()


def test_refusals(nm):
    lib = nm.lib()
    n = 2
    d = np.zeros((8, 128), np.uint8)
    x = np.zeros(8, np.float32)
    cnt8 = np.array([8], np.int32)
    H = np.tile(EYE, (n, 1))
    res = np.full((n, 8), 7, np.int32)
    best = np.full((n, 8), 7, np.float32)
    count = np.full(n, 7, np.int32)
    tab = lambda a, k=n: (C.c_void_p * 64)(*([a.ctypes.data] * k))
    rows = lambda a, k=n: (C.c_void_p * 64)(*[a[i].ctypes.data for i in range(k)])
    p = lambda a: a.ctypes.data
    dev, hst = lib.nm_sift_match_guided_u8_batch_dev, lib.nm_sift_match_guided_u8_host

    def call(fn, n_=n, capA=8, capB=8, r2=4.0, amb=0.8, maxd=float("inf"), **kw):
        a = dict(A=tab(d), ax=tab(x), ay=tab(x), nA=tab(cnt8), B=tab(d), bx=tab(x), by=tab(x), nB=tab(cnt8), H=p(H),
                 result=rows(res), count=p(count), best=rows(best))
        a.update(kw)
        args = [n_, a["A"], a["ax"], a["ay"], a["nA"], capA, a["B"], a["bx"], a["by"], a["nB"], capB, a["H"], None, r2, amb,
                maxd, a["result"], a["count"], a["best"]]
        return fn(*(args + ([None] if fn is dev else [])))

    assert d.ctypes.data % 16 == 0
    assert call(hst) == 0 and (res == -1).all() and (count == 0).all() and (best == 0).all()     # d = 0 twice: min2 == 0
    assert call(hst, best=None, maxd=float("-inf")) == 0
    res[:], count[:], best[:] = 7, 7, 7
    nan, inf = float("nan"), float("inf")
    bad = [dict(n_=0), dict(n_=-1), dict(n_=65), dict(capA=0), dict(capA=1 << 22), dict(capB=0), dict(capB=1 << 22),
           dict(r2=nan), dict(r2=inf), dict(r2=-inf), dict(amb=nan), dict(amb=inf), dict(amb=-inf), dict(maxd=nan)]
    bad += [dict([(k, None)]) for k in ("A", "ax", "ay", "nA", "B", "bx", "by", "nB", "H", "result", "count")]
    bad += [dict([(k, tab(d if k in "AB" else cnt8 if k in ("nA", "nB") else x, 1))]) for k in
            ("A", "ax", "ay", "nA", "B", "bx", "by", "nB")]
    bad += [dict(result=rows(res, 1)), dict(best=rows(best, 1))]
    for fn in (hst, dev):                                      # both refuse before touching memory
        for kw in bad:
            assert call(fn, **kw) != 0, (fn.__name__, kw)
    # alignment: the device entry refuses a descriptor pointer off a 16-byte boundary before anything is launched; the
    # host twin has no such rule and computes what it computes on an aligned copy
    keep = []

    def shifted(values, shift):
        buf = np.zeros(8 * 128 + 32, np.uint8)
        keep.append(buf)
        off = (-buf.ctypes.data) % 16 + shift
        m = buf[off:off + 8 * 128].reshape(8, 128)
        m[:] = values
        assert m.ctypes.data % 16 == shift
        return m

    for shift in (1, 4, 8):
        for key in ("A", "B"):
            assert call(dev, **{key: tab(shifted(d, shift))}) != 0, (key, shift)
    assert (res == 7).all() and (count == 7).all() and (best == 7).all()
    q = byte_pair(5, 8, 8, 255)
    want = host8(nm, [q, q], radius2=1e9)
    assert call(hst, A=tab(shifted(q["A"], 1)), ax=tab(q["ax"]), ay=tab(q["ay"]), B=tab(shifted(q["B"], 3)), bx=tab(q["bx"]),
                by=tab(q["by"]), r2=1e9) == 0
    assert np.array_equal(res, want[0]) and np.array_equal(count, want[1]) and np.array_equal(_bits(best), _bits(want[2]))
    assert count[0] > 0
    assert "nm_sift_match_guided_u8_batch_dev" in nm.ABI_SYMBOLS and "nm_sift_match_guided_u8_host" in nm.ABI_SYMBOLS


def test_wrapper_checks_and_the_batch_limit(nm):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = int(re.search(r"#define NM_MATCH_GUIDED_U8_MAX_BATCH (\d+)", open(os.path.join(root, "include", "nm_abi.h")).read()).group(1))
    src = open(os.path.join(root, "niftymatch_amd", "csrc", "nm_match_guided.hip")).read()
    slots = int(re.search(r"constexpr int SLOTS = (\d+);", src).group(1))
    assert "static_assert(NM_MATCH_GUIDED_U8_MAX_BATCH == 2 * SLOTS" in src
    assert hdr == 2 * slots == nm.MATCH_GUIDED_U8_MAX_BATCH == 64
    d = np.zeros((8, 128), np.uint8)
    x = np.zeros(8, np.float32)
    H = EYE.reshape(1, 9)

    def ok(**kw):
        a = dict(As=[d], axs=[x], ays=[x], nAs=[8], Bs=[d], bxs=[x], bys=[x], nBs=[8], H=H)
        a.update(kw)
        return nm.sift_match_guided_u8_host(a.pop("As"), a.pop("axs"), a.pop("ays"), a.pop("nAs"), a.pop("Bs"), a.pop("bxs"),
                                            a.pop("bys"), a.pop("nBs"), a.pop("H"), **a)

    r = ok()
    assert len(r) == 2 and r[0].shape == (1, 8) and r[0].dtype == np.int32 and r[1].shape == (1,)
    r = ok(want_distance=True)
    assert len(r) == 3 and r[2].shape == (1, 8) and r[2].dtype == np.float32
    assert ok(capA=5)[0].shape == (1, 5)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(radius2=nan), dict(radius2=inf), dict(ambiguity=nan), dict(ambiguity=-inf), dict(max_distance=nan),
               dict(capA=9), dict(capA=0), dict(capB=9), dict(capB=0), dict(H=np.zeros(8, np.float32)),
               dict(status=np.zeros(2, np.int32)), dict(As=[np.zeros((8, 64), np.uint8)]), dict(Bs=[np.zeros(8 * 128, np.uint8)]),
               dict(As=[np.zeros((8, 128), np.float32)]), dict(Bs=[np.zeros((8, 128), np.int8)]),
               dict(As=[np.zeros((8, 128), np.int32)]), dict(axs=[x, x]), dict(bxs=[np.zeros(4, np.float32)], capB=8)):
        with pytest.raises(nm.NmError):
            ok(**kw)
    with pytest.raises(nm.NmError):
        ok(As=[d] * 65, axs=[x] * 65, ays=[x] * 65, nAs=[8] * 65, Bs=[d] * 65, bxs=[x] * 65, bys=[x] * 65, nBs=[8] * 65,
           H=np.zeros((65, 9), np.float32))
    import torch
    t, one = torch.zeros(8), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(nm.NmError):                          # the device wrapper wants device tensors
        td = torch.zeros(8, 128, dtype=torch.uint8)
        nm.sift_match_guided_u8_batch_dev([td], [t], [t], [one], [td], [t], [t], [one], torch.zeros(9))


def real_links_u8(nm, oracle):
    """real_links with the descriptors finished to u8: [(fa, fb, H float32 (9,), H64)], fa / fb with desc uint8."""
    global _links8
    if _links8 is None:
        done = {}

        def finished(f):
            if id(f) not in done:
                _, u8 = nm.desc_finish_host([f["desc"]], [f["n"]], want_f32=False)
                done[id(f)] = dict(desc=u8[0][:f["n"]].copy(), x=f["x"], y=f["y"], n=f["n"])
            return done[id(f)]

        _links8 = [(finished(fa), finished(fb), H, H64) for fa, fb, H, H64 in real_links(oracle)]
    return _links8


def test_real_links_equal_the_restatement_and_keep_more_true_matches_than_the_blind_matcher(nm, oracle):
    for k, (fa, fb, H, H64) in enumerate(real_links_u8(nm, oracle)):
        p = dict(A=fa["desc"], ax=fa["x"], ay=fa["y"], nA=fa["n"], B=fb["desc"], bx=fb["x"], by=fb["y"], nB=fb["n"], H=H, status=1)
        res, cnt, best = (v[0] for v in assert_equals_restatement(nm, [p], "real link %d" % k))
        blind = nm.sift_match_u8_host([fa["desc"]], [fa["n"]], [fb["desc"]], [fb["n"]], ambiguity=AMB, prior=-1)[0]
        q = H64 @ np.stack([fa["x"].astype(np.float64), fa["y"].astype(np.float64), np.ones(fa["n"])])
        px, py = q[0] / q[2], q[1] / q[2]

        def true_rows(m):
            rows = np.flatnonzero(m >= 0)
            return rows[np.hypot(fb["x"][m[rows]] - px[rows], fb["y"][m[rows]] - py[rows]) < 1.5]

        bt, gt = true_rows(blind), true_rows(res)
        print("link %d->%d: keypoints %d / %d, blind u8 matches %d (%d true), guided u8 %d (%d true), %.3f x" % (
            k, k + 1, fa["n"], fb["n"], (blind >= 0).sum(), len(bt), cnt, len(gt), len(gt) / len(bt)))
        assert len(bt) > 1000 and len(gt) >= len(bt), (k, len(gt), len(bt))
