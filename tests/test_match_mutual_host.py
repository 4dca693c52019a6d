"""Mutual-nearest-neighbour filtering through its host twin (nm_sift_match_mutual_host_f32: the device entry's functions,
compiled for the host) against the independent restatement tests/mutual_ref.py and against the swapped blind match of the
CPU oracle. No GPU. Every sequence is fully specified in float32, so equality is exact: no tolerance, no excluded rows.
"""
import ctypes as C

import numpy as np
import pytest

import mutual_ref as M

AMB = 0.8
NEVER = 3.0e38                                   # an ambiguity the ratio test never rejects (min1 / min2 < NEVER)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def random_pair(oracle, seed, rows_a, rows_b, nA=None, nB=None):
    """Descriptors of small integers (exact ties and zero distances occur), copies planted across and inside the sets. The
    match list is the oracle's ratio-test result, salted with values that are no claim (-1, -7, nB, nB + 3) and with rows
    forced onto a column another row already claims."""
    rng = np.random.default_rng(seed)
    A = rng.integers(0, 4, (rows_a, 128)).astype(np.float32)
    B = rng.integers(0, 4, (rows_b, 128)).astype(np.float32)
    for i in range(0, min(rows_a, rows_b), 3):                # row i sits on column i: distance 0
        A[i] = B[i]
    for i in range(1, rows_a - 1, 5):                         # twin rows of A: exact ties on whatever column they claim
        A[i + 1] = A[i]
    for i in range(2, min(rows_a, rows_b), 11):               # near copies: a clear nearest neighbour that is not 0
        A[i] = B[i]
        A[i, :3] += 1
    m, _, _ = oracle.sift_matches(A, B, AMB, want_distance=False)
    m = m.astype(np.int32)
    claimed = np.flatnonzero(m >= 0)
    for t, i in enumerate(range(5, rows_a, 7)):
        m[i] = (-1, -7, rows_b if nB is None else nB, (rows_b if nB is None else nB) + 3)[t % 4]
    if len(claimed):
        for t, i in enumerate(range(3, rows_a, 4)):           # several rows claim one column
            m[i] = m[claimed[t % len(claimed)]]
    return dict(A=A, B=B, m=m, nA=rows_a if nA is None else nA, nB=rows_b if nB is None else nB)


def trap_pair(rows_a=40):
    """The early-exit traps, one column of B each (the columns are 10 apart in every dimension, so a trap's rows are far from
    every other column). Logical rows 0 .. 39 are spread over rows_a rows in order; the others are far from everything.
    Returns the pair and {row: kept?} as the semantics decide it."""
    assert rows_a >= 40
    at = lambda t: t * (rows_a // 40)
    B = np.repeat(np.arange(12, dtype=np.float32)[:, None] * 10, 128, axis=1)
    A = np.full((rows_a, 128), 500.0, np.float32)
    m = np.full(rows_a, -1, np.int32)
    expect = {}
    ones = np.ones(128, np.float32)
    quarter = np.full(128, 0.25, np.float32)
    quarter[127] = 1.0                                        # tau = 127 / 16 + 1
    four = np.zeros(128, np.float32)
    four[:4] = 1.0                                            # tau = 4
    half16 = np.zeros(128, np.float32)
    half16[:16] = 0.5                                         # partial sum 4 after the first chunk of 16, exactly

    def put(t, j, pattern, claims, kept=None, **change):
        row = B[j] + pattern
        for q, v in change.items():
            row[int(q[1:])] = B[j, 0] + v if np.isfinite(v) else v
        A[at(t)] = row
        if claims:
            m[at(t)] = j
            expect[at(t)] = kept

    put(2, 0, ones, False)                                    # a twin at a lower index: the exact tie goes to the lower one
    put(4, 0, ones, True, kept=False)
    put(5, 1, ones, True, kept=True)                          # a twin at a higher index
    put(9, 1, ones, False)
    put(6, 2, ones, True, kept=True)                          # both twins claim: one-to-one
    put(7, 2, ones, True, kept=False)
    put(10, 3, quarter, True, kept=False)                     # a rival that differs in q = 127 alone, just smaller
    put(11, 3, quarter, False, q127=1.0 - 2.0 ** -10)
    put(12, 4, quarter, True, kept=True)                      # ... just larger, at a lower index
    put(3, 4, quarter, False, q127=1.0 + 2.0 ** -10)
    put(13, 5, quarter, True, kept=False)                     # a rival that differs in q = 0 alone, smaller
    put(14, 5, quarter, False, q0=0.0)
    put(15, 6, quarter, True, kept=True)                      # ... larger, at a lower index
    put(1, 6, quarter, False, q0=0.5)
    put(16, 7, four, True, kept=True)                         # partial sum == tau at the chunk boundary, then it grows
    put(0, 7, half16, False, q16=1.0)
    put(17, 8, four, True, kept=False)                        # ... and stays: a tie with a lower index
    put(8, 8, half16, False)
    put(18, 9, ones, True, kept=True)                         # NaN and inf inside rivals that would otherwise win
    put(19, 9, np.zeros(128, np.float32), False, q120=np.nan)
    put(20, 9, np.zeros(128, np.float32), False, q100=np.inf)
    put(21, 9, np.zeros(128, np.float32), False, q5=np.nan)
    put(22, 10, ones, True, kept=False, q64=np.nan)           # NaN inside the claiming row: the claim is dropped
    put(23, 11, ones, True, kept=False, q3=np.inf)            # tau = +inf: every finite rival is nearer
    return dict(A=A, B=B, m=m, nA=rows_a, nB=12), expect


def host(nm, pairs, capA=None, capB=None):
    k = lambda key: [p[key] for p in pairs]
    return nm.sift_match_mutual_host(k("A"), k("nA"), k("B"), k("nB"), k("m"), capA=capA, capB=capB, want_distance=True)


def assert_equals_restatement(nm, pairs, what, capA=None, capB=None):
    res, cnt, fwd = host(nm, pairs, capA=capA, capB=capB)
    for k, p in enumerate(pairs):
        want, wcount, wfwd = M.mutual(p["A"], p["nA"], p["B"], p["nB"], p["m"], capA=res.shape[1],
                                      capB=min(len(q["B"]) for q in pairs) if capB is None else capB)
        diff = np.flatnonzero(res[k] != want)
        assert not len(diff), (what, k, diff[:5], res[k][diff[:5]], want[diff[:5]])
        assert cnt[k] == wcount == (res[k] >= 0).sum(), (what, k)
        assert np.array_equal(_bits(fwd[k]), _bits(wfwd)), (what, k)
        assert_one_to_one(res[k], p, what)
    return res, cnt, fwd


def assert_one_to_one(res, p, what=""):
    nA = min(max(p["nA"], 0), len(res))
    kept = res[res >= 0]
    assert len(np.unique(kept)) == len(kept), (what, "two rows keep one column")
    assert (res[nA:] == -1).all(), (what, "a row beyond nA")
    rows = np.flatnonzero(res >= 0)
    assert np.array_equal(res[rows], p["m"][rows]), (what, "a kept row changed its column")


@pytest.mark.parametrize("shape", [(1, 1), (1, 5), (5, 1), (63, 65), (300, 257), (1000, 700)])
def test_host_twin_equals_the_restatement(nm, oracle, shape):
    p = random_pair(oracle, 100 + shape[0], *shape)
    res, cnt, fwd = assert_equals_restatement(nm, [p], "shape %r" % (shape,))
    claims = int(((p["m"] >= 0) & (p["m"] < p["nB"])).sum())
    assert claims >= 1 and (shape[0] < 60 or 0 < cnt[0] < claims), (claims, cnt)   # the filter kept some and removed some
    assert np.isinf(fwd[0][(p["m"] < 0) | (p["m"] >= p["nB"])]).all()


def test_early_exit_traps(nm):
    for rows_a in (40, 1100):
        p, expect = trap_pair(rows_a)
        res, cnt, fwd = assert_equals_restatement(nm, [p], "traps over %d rows" % rows_a)
        got = {i: bool(res[0][i] >= 0) for i in expect}
        assert got == expect, {i: (got[i], expect[i]) for i in expect if got[i] != expect[i]}
        at = lambda t: t * (rows_a // 40)
        assert np.isnan(fwd[0][at(22)]) and np.isposinf(fwd[0][at(23)]) and fwd[0][at(16)] == 4.0


def test_size_handling(nm, oracle):
    p = random_pair(oracle, 7, 120, 130)
    full, _, _ = assert_equals_restatement(nm, [p], "full")
    assert (full[0] >= 0).sum() > 10
    assert_equals_restatement(nm, [dict(p, nA=10 ** 6, nB=10 ** 6)], "sizes above the capacities are clipped")
    clipped, _, _ = assert_equals_restatement(nm, [dict(p, nA=500)], "nA above capA", capA=100)
    assert clipped.shape == (1, 100)
    for kw in (dict(nA=0), dict(nA=-4), dict(nB=0), dict(nB=-1), dict(nA=0, nB=0)):
        res, cnt, fwd = assert_equals_restatement(nm, [dict(p, **kw)], repr(kw))
        assert (res == -1).all() and cnt[0] == 0 and np.isinf(fwd).all()
    part, _, _ = assert_equals_restatement(nm, [dict(p, nA=31, nB=50)], "partial sizes")
    assert (part[0][31:] == -1).all()
    # several pairs in one call, each as alone
    pairs = [random_pair(oracle, 8, 120, 130), dict(p, nA=31, nB=50), random_pair(oracle, 9, 200, 140, nA=150)]
    res, cnt, _ = assert_equals_restatement(nm, pairs, "three pairs", capA=120, capB=130)
    assert np.array_equal(res[1], part[0])


def _assert_cross_check(oracle, nm, A, B, forward_ambiguity, what):
    m, _, _ = oracle.sift_matches(A, B, forward_ambiguity, want_distance=False)
    rev, _, _ = oracle.sift_matches(B, A, NEVER, want_distance=False)
    claimed = np.flatnonzero(m >= 0)
    assert len(claimed) > 20, (what, len(claimed))
    assert (rev[m[claimed]] >= 0).all(), (what, "the swapped match left a claimed column out")
    res, cnt, _ = nm.sift_match_mutual_host([A], [len(A)], [B], [len(B)], [m], want_distance=True)
    want = np.where((m >= 0) & (rev[np.maximum(m, 0)] == np.arange(len(A))), m, -1)
    assert np.array_equal(res[0], want), (what, np.flatnonzero(res[0] != want)[:8])
    assert cnt[0] == (want >= 0).sum()
    assert_one_to_one(res[0], dict(nA=len(A), m=m), what)
    return int(len(claimed)), int(cnt[0])


def test_equals_the_swapped_blind_match(nm, oracle):
    """Float descriptors without exact ties or zero distances: kept(i) <=> rev[matches[i]] == i, rev being the oracle's match
    of B against A under a ratio test that never rejects; no claimed column is left out of the comparison."""
    rng = np.random.default_rng(5)
    A = rng.uniform(0, 255, (400, 128)).astype(np.float32)
    B = rng.uniform(0, 255, (380, 128)).astype(np.float32)
    B[:150] = A[100:250] + rng.normal(0, 20, (150, 128)).astype(np.float32)      # true matches the ratio test accepts
    B[150:200] = A[100:150] + rng.normal(0, 25, (50, 128)).astype(np.float32)    # a second column for 50 of those rows
    for amb in (AMB, NEVER):                                                     # NEVER: every row claims its nearest column
        claims, kept = _assert_cross_check(oracle, nm, A, B, amb, "uniform rows, ambiguity %g" % amb)
        print("uniform 400 x 380, forward ambiguity %g: %d claims, %d kept" % (amb, claims, kept))
        assert kept < claims or amb == AMB
    from test_match_guided_host import real_links
    fa, fb, _, _ = real_links(oracle)[0]
    claims, kept = _assert_cross_check(oracle, nm, fa["desc"][:fa["n"]], fb["desc"][:fb["n"]], AMB, "SIFT descriptors")
    print("SIFT views 0 -> 1: %d x %d rows, %d ratio matches, %d mutual" % (fa["n"], fb["n"], claims, kept))
    assert 0 < kept <= claims


def test_refusals(nm):
    lib = nm.lib()
    n = 2
    d = np.zeros((8, 128), np.float32)
    cnt8 = np.array([8], np.int32)
    mt = np.arange(8, dtype=np.int32)
    res = np.full((n, 8), 7, np.int32)
    fwd = np.full((n, 8), 7, np.float32)
    count = np.full(n, 7, np.int32)
    ws = np.full(64, 7, np.int32)
    tab = lambda a, k=n: (C.c_void_p * 64)(*([a.ctypes.data] * k))
    rows = lambda a, k=n: (C.c_void_p * 64)(*[a[i].ctypes.data for i in range(k)])
    p = lambda a: a.ctypes.data

    def call(fn, n_=n, capA=8, capB=8, **kw):
        a = dict(A=tab(d), nA=tab(cnt8), B=tab(d), nB=tab(cnt8), m=tab(mt), result=rows(res), count=p(count), fwd=rows(fwd),
                 ws=p(ws))
        a.update(kw)
        args = [n_, a["A"], a["nA"], capA, a["B"], a["nB"], capB, a["m"], a["result"], a["count"], a["fwd"]]
        return fn(*(args + ([a["ws"], None] if fn is lib.nm_sift_match_mutual_batch_dev_f32 else [])))

    assert call(lib.nm_sift_match_mutual_host_f32) == 0
    assert (res == np.array([0] + [-1] * 7)).all() and (count == 1).all() and (fwd == 0).all()
    assert call(lib.nm_sift_match_mutual_host_f32, fwd=None) == 0
    res[:], count[:], fwd[:] = 7, 7, 7
    bad = [dict(n_=0), dict(n_=-1), dict(n_=65), dict(capA=0), dict(capA=1 << 22), dict(capB=0), dict(capB=1 << 22)]
    bad += [dict([(k, None)]) for k in ("A", "nA", "B", "nB", "m", "result", "count")]
    bad += [dict([(k, tab(d if k in "AB" else mt if k == "m" else cnt8, 1))]) for k in ("A", "nA", "B", "nB", "m")]
    bad += [dict(result=rows(res, 1)), dict(fwd=rows(fwd, 1))]
    for fn in (lib.nm_sift_match_mutual_host_f32, lib.nm_sift_match_mutual_batch_dev_f32):   # both refuse before touching memory
        for kw in bad:
            assert call(fn, **kw) != 0, (fn.__name__, kw)
    assert call(lib.nm_sift_match_mutual_batch_dev_f32, ws=None) != 0
    assert (res == 7).all() and (count == 7).all() and (fwd == 7).all() and (ws == 7).all()
    for name in ("nm_sift_match_mutual_batch_dev_f32", "nm_sift_match_mutual_host_f32", "nm_sift_match_mutual_workspace_bytes"):
        assert name in nm.ABI_SYMBOLS
    wsb = lib.nm_sift_match_mutual_workspace_bytes
    assert wsb(1, 1) > 0 and wsb(64, (1 << 22) - 1) > wsb(16, 16384) > wsb(1, 16384) >= 3 * 4 * 16384
    assert wsb(0, 8) == wsb(65, 8) == wsb(1, 0) == wsb(1, 1 << 22) == 0


def test_wrapper_checks_and_the_batch_limit(nm):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = int(re.search(r"#define NM_MATCH_MUTUAL_MAX_BATCH (\d+)", open(os.path.join(root, "include", "nm_abi.h")).read()).group(1))
    assert hdr == nm.MATCH_MUTUAL_MAX_BATCH == 64
    d = np.zeros((8, 128), np.float32)
    mt = np.arange(8, dtype=np.int32)

    def ok(**kw):
        a = dict(As=[d], nAs=[8], Bs=[d], nBs=[8], matches=[mt])
        a.update(kw)
        return nm.sift_match_mutual_host(a.pop("As"), a.pop("nAs"), a.pop("Bs"), a.pop("nBs"), a.pop("matches"), **a)

    r = ok()
    assert len(r) == 2 and r[0].shape == (1, 8) and r[0].dtype == np.int32 and len(ok(want_distance=True)) == 3
    assert ok(capA=5)[0].shape == (1, 5)
    for kw in (dict(capA=9), dict(capA=0), dict(capB=9), dict(capB=0), dict(As=[np.zeros((8, 64), np.float32)]),
               dict(nAs=[8, 8]), dict(matches=[mt, mt]), dict(matches=[mt[:4]], capA=8), dict(matches=[np.zeros((8, 2), np.int32)]),
               dict(As=[], nAs=[], Bs=[], nBs=[], matches=[])):
        with pytest.raises(nm.NmError):
            ok(**kw)
    with pytest.raises(nm.NmError):
        ok(As=[d] * 65, nAs=[8] * 65, Bs=[d] * 65, nBs=[8] * 65, matches=[mt] * 65)
    assert ok(As=[d] * 64, nAs=[8] * 64, Bs=[d] * 64, nBs=[8] * 64, matches=[mt] * 64)[0].shape == (64, 8)
    import torch
    td, one, tm = torch.zeros(8, 128), torch.zeros(1, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)
    with pytest.raises(nm.NmError):                          # the device wrapper wants device tensors
        nm.sift_match_mutual_batch_dev([td], [one], [td], [one], [tm])
    with pytest.raises(nm.NmError):
        nm.sift_match_mutual_batch_dev([td], [one], [td], [one], [tm, tm])
    with pytest.raises(nm.NmError):
        nm.MatchMutualWorkspace(65, 8, device="cpu")
