"""The mutual filter for u8 descriptors through its host twin (nm_sift_match_mutual_u8_host) against the independent
restatement tests/mutual_u8_ref.py, against the fp32 filter's host twin on float copies of the same bytes (bit for bit, the
forward distances included) and against the swapped u8 match. No GPU. Everything is integer, so equality is exact: no
tolerance, no excluded rows. The cases are the GPU test's (tests/test_gpu_match_mutual_u8.py), plus the refusals.
"""
import ctypes as C

import numpy as np
import pytest

import mutual_u8_ref as M


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def host(nm, cases, capA=None, capB=None):
    k = lambda key: [c[key] for c in cases]
    return nm.sift_match_mutual_u8_host(k("A"), k("nA"), k("B"), k("nB"), k("m"), capA=capA, capB=capB, want_distance=True)


def host_f32(nm, cases, capA=None, capB=None):
    k = lambda key: [c[key] for c in cases]
    f = lambda key: [c[key].astype(np.float32) for c in cases]
    return nm.sift_match_mutual_host(f("A"), k("nA"), f("B"), k("nB"), k("m"), capA=capA, capB=capB, want_distance=True)


def assert_one_to_one(res, case):
    nA = min(max(case["nA"], 0), len(res))
    kept = res[res >= 0]
    assert len(np.unique(kept)) == len(kept), (case["what"], "two rows keep one column")
    assert (res[nA:] == -1).all(), (case["what"], "a row beyond nA")
    rows = np.flatnonzero(res >= 0)
    assert np.array_equal(res[rows], case["m"][rows]), (case["what"], "a kept row changed its column")


def assert_cases(nm, cases, capA=None, capB=None):
    """The host twin of one call against the restatement and against the fp32 twin on float copies."""
    res, cnt, fwd = host(nm, cases, capA, capB)
    fres, fcnt, ffwd = host_f32(nm, cases, capA, capB)
    for k, c in enumerate(cases):
        want, wcount, wfwd = M.expected(c, capA=res.shape[1], capB=capB)
        diff = np.flatnonzero(res[k] != want)
        assert not len(diff), (c["what"], "restatement", diff[:5], res[k][diff[:5]], want[diff[:5]])
        assert cnt[k] == wcount == (res[k] >= 0).sum(), c["what"]
        assert np.array_equal(_bits(fwd[k]), _bits(wfwd)), c["what"]
        assert np.array_equal(res[k], fres[k]) and cnt[k] == fcnt[k], (c["what"], "fp32 filter on float copies")
        assert np.array_equal(_bits(fwd[k]), _bits(ffwd[k])), (c["what"], "fp32 forward distances")
        assert_one_to_one(res[k], c)
    return res, cnt, fwd


@pytest.mark.parametrize("family", ["size_cases", "claim_count_cases", "duplicate_cases", "shared_column_case", "extremes_case",
                                    "clip_cases"])
def test_host_twin_equals_restatement_and_fp32_filter(nm, family):
    cases = getattr(M, family)()
    kept = 0
    for c in cases:
        res, cnt, fwd = assert_cases(nm, [c])
        kept += int(cnt[0])
        no_claim = np.ones(len(res[0]), bool)
        nA, nB = min(max(c["nA"], 0), len(res[0])), min(max(c["nB"], 0), len(c["B"]))
        no_claim[:nA] = (c["m"][:nA] < 0) | (c["m"][:nA] >= nB)
        assert np.isposinf(fwd[0][no_claim]).all() and np.isfinite(fwd[0][~no_claim]).all(), c["what"]
    assert kept == M.kept_removed(cases)[0]


@pytest.mark.parametrize("n", [1, 3, 16, 64])
def test_ragged_batches(nm, n):
    cases, capA, capB = M.ragged_batch(n)
    res, cnt, fwd = assert_cases(nm, cases, capA, capB)
    empty = [i for i, c in enumerate(cases) if c["nA"] <= 0 or c["nB"] <= 0]
    assert len(empty) == 1 and (res[empty[0]] == -1).all() and cnt[empty[0]] == 0 and np.isposinf(fwd[empty[0]]).all()
    alone = host(nm, [cases[-1]], capA, capB)
    assert np.array_equal(alone[0][0], res[-1]) and alone[1][0] == cnt[-1]     # a pair's outputs do not depend on the batch
    assert np.array_equal(_bits(alone[2][0]), _bits(fwd[-1]))


def test_equals_the_swapped_u8_match(nm):
    """On the lists sift_match_u8_host wrote, kept(i) <=> rev[m[i]] == i, rev being the swapped u8 match under an ambiguity
    above 1 (the ratio of the nearest to the second nearest is at most 1, so only the nearest decides). The one exception:
    the swapped call leaves a column's entry unwritten when its second-smallest distance is 0 (two rows of A equal the
    column; a one-row A has the matcher's start value as second distance and is written). Those claims are compared against
    the restatement instead; they are counted and must be a small minority."""
    c = M.random_case(61, 600, 500, pad=0)
    A, B = c["A"].copy(), c["B"].copy()
    for t in range(6):                                           # two rows of A on one column: min2 == 0 in the swapped call
        A[40 * t + 7] = A[40 * t + 19] = B[11 * t]
    m = nm.sift_match_u8_host([A], [600], [B], [500], ambiguity=0.8, prior=-1)[0]
    rev = nm.sift_match_u8_host([B], [500], [A], [600], ambiguity=1.5, prior=-9)[0]
    res, cnt = nm.sift_match_mutual_u8_host([A], [600], [B], [500], [m])
    want, wcount, _ = M.mutual(A, 600, B, 500, m)
    assert np.array_equal(res[0], want) and cnt[0] == wcount
    claims = np.flatnonzero(m >= 0)
    unwritten = claims[rev[m[claims]] == -9]
    decided = claims[rev[m[claims]] != -9]
    print("600 x 500: %d claims, %d kept, %d on columns the swapped call leaves unwritten" % (len(claims), wcount, len(unwritten)))
    assert len(claims) > 100 and 1 <= len(unwritten) <= len(claims) // 10
    assert np.array_equal(res[0][decided] >= 0, rev[m[decided]] == decided)
    assert 0 < wcount < len(claims)


def test_refusals(nm):
    lib = nm.lib()
    n = 2
    d = np.zeros((8, 128), np.uint8)
    cnt8 = np.array([8], np.int32)
    mt = np.arange(8, dtype=np.int32)
    res = np.full((n, 8), 7, np.int32)
    fwd = np.full((n, 8), 7, np.float32)
    count = np.full(n, 7, np.int32)
    ws = np.full(4096, 7, np.int32)
    assert d.ctypes.data % 16 == 0 and ws.ctypes.data % 16 == 0
    tab = lambda a, k=n: (C.c_void_p * 64)(*([a.ctypes.data] * k))
    rows = lambda a, k=n: (C.c_void_p * 64)(*[a[i].ctypes.data for i in range(k)])
    p = lambda a: a.ctypes.data
    dev, hst = lib.nm_sift_match_mutual_u8_batch_dev, lib.nm_sift_match_mutual_u8_host

    def call(fn, n_=n, capA=8, capB=8, **kw):
        a = dict(A=tab(d), nA=tab(cnt8), B=tab(d), nB=tab(cnt8), m=tab(mt), result=rows(res), count=p(count), fwd=rows(fwd),
                 ws=p(ws))
        a.update(kw)
        args = [n_, a["A"], a["nA"], capA, a["B"], a["nB"], capB, a["m"], a["result"], a["count"], a["fwd"]]
        return fn(*(args + ([a["ws"], None] if fn is dev else [])))

    assert call(hst) == 0
    assert (res == np.array([0] + [-1] * 7)).all() and (count == 1).all() and (fwd == 0).all()
    assert call(hst, fwd=None) == 0
    res[:], count[:], fwd[:] = 7, 7, 7
    bad = [dict(n_=0), dict(n_=-1), dict(n_=65), dict(capA=0), dict(capA=1 << 22), dict(capB=0), dict(capB=1 << 22)]
    bad += [dict([(k, None)]) for k in ("A", "nA", "B", "nB", "m", "result", "count")]
    bad += [dict([(k, tab(d if k in "AB" else mt if k == "m" else cnt8, 1))]) for k in ("A", "nA", "B", "nB", "m")]
    bad += [dict(result=rows(res, 1)), dict(fwd=rows(fwd, 1))]
    for fn in (hst, dev):                                      # both refuse before touching memory
        for kw in bad:
            assert call(fn, **kw) != 0, (fn.__name__, kw)
    assert call(dev, ws=None) != 0
    odd = np.zeros(8 * 128 + 32, np.uint8)
    off = (-odd.ctypes.data) % 16 + 1                          # a descriptor pointer that is not 16-byte aligned
    for key in ("A", "B"):
        assert call(dev, **{key: (C.c_void_p * 64)(*([odd.ctypes.data + off] * n))}) != 0
    assert call(dev, ws=p(ws) + 4) != 0                        # a workspace that is not 16-byte aligned
    assert (res == 7).all() and (count == 7).all() and (fwd == 7).all() and (ws == 7).all()
    for name in ("nm_sift_match_mutual_u8_batch_dev", "nm_sift_match_mutual_u8_host", "nm_sift_match_mutual_u8_workspace_bytes"):
        assert name in nm.ABI_SYMBOLS
    wsb = lib.nm_sift_match_mutual_u8_workspace_bytes
    assert wsb(1, 1, 1) > 0 and wsb(64, (1 << 22) - 1, 16384) > wsb(16, 16384, 16384) > wsb(1, 16384, 16384) >= 5 * 4 * 16384
    assert wsb(16, 16384, 16384) % 16 == 0
    assert wsb(0, 8, 8) == wsb(65, 8, 8) == wsb(1, 0, 8) == wsb(1, 8, 0) == wsb(1, 1 << 22, 8) == wsb(1, 8, 1 << 22) == 0


def test_wrapper_checks_and_the_batch_limit(nm):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = int(re.search(r"#define NM_MATCH_MUTUAL_U8_MAX_BATCH (\d+)", open(os.path.join(root, "include", "nm_abi.h")).read()).group(1))
    assert hdr == nm.MATCH_MUTUAL_U8_MAX_BATCH == 64
    d = np.zeros((8, 128), np.uint8)
    mt = np.arange(8, dtype=np.int32)

    def ok(**kw):
        a = dict(As=[d], nAs=[8], Bs=[d], nBs=[8], matches=[mt])
        a.update(kw)
        return nm.sift_match_mutual_u8_host(a.pop("As"), a.pop("nAs"), a.pop("Bs"), a.pop("nBs"), a.pop("matches"), **a)

    r = ok()
    assert len(r) == 2 and r[0].shape == (1, 8) and r[0].dtype == np.int32 and len(ok(want_distance=True)) == 3
    assert ok(capA=5)[0].shape == (1, 5)
    for kw in (dict(capA=9), dict(capA=0), dict(capB=9), dict(capB=0), dict(As=[np.zeros((8, 64), np.uint8)]),
               dict(nAs=[8, 8]), dict(matches=[mt, mt]), dict(matches=[mt[:4]], capA=8), dict(matches=[np.zeros((8, 2), np.int32)]),
               dict(As=[], nAs=[], Bs=[], nBs=[], matches=[])):
        with pytest.raises(nm.NmError):
            ok(**kw)
    with pytest.raises(nm.NmError):
        ok(As=[d] * 65, nAs=[8] * 65, Bs=[d] * 65, nBs=[8] * 65, matches=[mt] * 65)
    assert ok(As=[d] * 64, nAs=[8] * 64, Bs=[d] * 64, nBs=[8] * 64, matches=[mt] * 64)[0].shape == (64, 8)
    import torch
    td, one, tm = torch.zeros(8, 128, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)
    with pytest.raises(nm.NmError):                          # the device wrapper wants device tensors
        nm.sift_match_mutual_u8_batch_dev([td], [one], [td], [one], [tm])
    with pytest.raises(nm.NmError):
        nm.sift_match_mutual_u8_batch_dev([td], [one], [td], [one], [tm, tm])
    with pytest.raises(nm.NmError):
        nm.MatchMutualU8Workspace(65, 8, 8, device="cpu")
