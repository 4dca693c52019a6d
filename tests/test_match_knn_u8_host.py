"""The u8 k-nearest-neighbour entry through its host twin (nm_sift_match_knn_u8_host) against the numpy restatement
(tests/knn_u8_ref.py), array_equal, on the u8 matcher's cases and ragged batches at k = 1, 2, 3, 5, 8, with and without
distances; the refusals; and, from the k = 2 lists, the u8 matcher's own result through its last step. No GPU.
"""
import ctypes as C

import numpy as np
import pytest

import knn_u8_ref as K
import match_u8_ref as M


def _host(nm, cases, k, capA, capB, want_distance=True):
    col = lambda key: [c[key] for c in cases]
    return nm.sift_match_knn_u8_host(col("A"), col("nA"), col("B"), col("nB"), k, capA=capA, capB=capB,
                                     want_distance=want_distance, prior=K.PRIOR)


def _assert_cases(nm, cases, k, capA, capB):
    idx, dist = _host(nm, cases, k, capA, capB)
    only, none = _host(nm, cases, k, capA, capB, want_distance=False)
    assert none is None and idx.dtype == dist.dtype == np.int32 and idx.shape == dist.shape == (len(cases), capA, k)
    for p, c in enumerate(cases):
        wi, wd = K.expected(c, k, capA, capB)
        assert np.array_equal(idx[p], wi), (c["what"], k, "index")
        assert np.array_equal(dist[p], wd), (c["what"], k, "distance")
        assert np.array_equal(only[p], wi), (c["what"], k, "index alone")
    return idx, dist


@pytest.mark.parametrize("k", K.KS)
def test_cases_equal_restatement(nm, k):
    for c in M.all_cases():
        _assert_cases(nm, [c], k, len(c["A"]), len(c["B"]))


@pytest.mark.parametrize("n", [1, 3, 64])
def test_ragged_batches(nm, n):
    cases, capA, capB = M.ragged_batch(n)
    for k in K.KS:
        idx, dist = _assert_cases(nm, cases, k, capA, capB)
    empty = [p for p, c in enumerate(cases) if c["nA"] <= 0 or c["nB"] <= 0]
    assert len(empty) == 1 and (idx[empty[0]] == K.PRIOR[0]).all() and (dist[empty[0]] == K.PRIOR[1]).all()
    alone = _host(nm, cases[:1], K.KS[-1], capA, capB)
    assert np.array_equal(alone[0][0], idx[0]) and np.array_equal(alone[1][0], dist[0])


def test_ties_and_the_largest_distance(nm):
    for c in K.tie_cases():
        idx, _ = _assert_cases(nm, [c], 8, 40, 70)
        first = 0 if "70" in c["what"] else 28
        assert (idx[0] == np.arange(first, first + 8)).all(), c["what"]
    for c in K.extreme_cases():
        _, dist = _assert_cases(nm, [c], 8, 40, 70)
    assert dist[0, :, 7].max() == 128 * 255 * 255 and dist.min() == 0


@pytest.mark.parametrize("amb", [0.8, 1.0, 1.5])
def test_k2_lists_reproduce_the_matcher(nm, amb):
    for c in M.all_cases():
        capA = len(c["A"])
        idx, dist = _host(nm, [c], 2, capA, len(c["B"]))
        prior = np.full(capA, c["prior"], np.int32)
        got = K.matcher_last_step(idx[0], dist[0], c["nB"], amb, prior)
        want = nm.sift_match_u8_host([c["A"]], [c["nA"]], [c["B"]], [c["nB"]], ambiguity=amb, prior=c["prior"])[0]
        assert np.array_equal(got, want), (c["what"], amb)


def test_refusals(nm):
    lib = nm.lib()
    n, k = 2, 3
    d = np.zeros((8, 128), np.uint8)
    cnt8 = np.array([8], np.int32)
    idx, dist = np.full((n, 8, k), 7, np.int32), np.full((n, 8, k), 7, np.int32)
    ws = np.full(4096, 7, np.int32)
    tab = lambda a, m=n: (C.c_void_p * 64)(*([a.ctypes.data] * m))
    rows = lambda a, m=n: (C.c_void_p * 64)(*[a[i].ctypes.data for i in range(m)])

    def call(fn, n_=n, capA=8, capB=8, k_=k, **kw):
        a = dict(A=tab(d), nA=tab(cnt8), B=tab(d), nB=tab(cnt8), index=rows(idx), distance=rows(dist), ws=ws.ctypes.data)
        a.update(kw)
        args = [n_, a["A"], a["nA"], capA, a["B"], a["nB"], capB, k_, a["index"], a["distance"]]
        return fn(*(args + ([a["ws"], None] if fn is lib.nm_sift_match_knn_u8_batch_dev else [])))

    bad = [dict(k_=0), dict(k_=9), dict(k_=-1), dict(n_=0), dict(n_=65), dict(capA=0), dict(capA=1 << 22), dict(capB=0),
           dict(capB=1 << 22)]
    bad += [dict([(key, None)]) for key in ("A", "nA", "B", "nB", "index")]
    bad += [dict([(key, tab(d if key in "AB" else cnt8, 1))]) for key in ("A", "nA", "B", "nB")]
    bad += [dict(index=rows(idx, 1)), dict(distance=rows(dist, 1))]
    for fn in (lib.nm_sift_match_knn_u8_host, lib.nm_sift_match_knn_u8_batch_dev):   # both refuse before touching memory
        for kw in bad:
            assert call(fn, **kw) != 0, (fn.__name__, kw)
    assert call(lib.nm_sift_match_knn_u8_batch_dev, ws=None) != 0
    odd = np.zeros(8 * 128 + 16, np.uint8)
    off = (-odd.ctypes.data) % 16 + 1                          # a descriptor pointer that is not 16-byte aligned
    assert call(lib.nm_sift_match_knn_u8_batch_dev, A=(C.c_void_p * 64)(*([odd.ctypes.data + off] * n))) != 0
    assert (idx == 7).all() and (dist == 7).all() and (ws == 7).all()
    assert call(lib.nm_sift_match_knn_u8_host, distance=None) == 0               # indices only
    assert (idx == np.arange(k)).all() and (dist == 7).all()   # identical rows: the k lowest indices
    assert call(lib.nm_sift_match_knn_u8_host) == 0
    assert (dist == 0).all()
    for name in ("nm_sift_match_knn_u8_batch_dev", "nm_sift_match_knn_u8_host", "nm_sift_match_knn_u8_workspace_bytes"):
        assert name in nm.ABI_SYMBOLS
    wsb = lib.nm_sift_match_knn_u8_workspace_bytes
    assert wsb(16, 16384, 16384) == lib.nm_sift_match_u8_workspace_bytes(16, 16384, 16384) > 0
    assert wsb(0, 8, 8) == wsb(65, 8, 8) == wsb(1, 0, 8) == wsb(1, 8, 0) == wsb(1, 1 << 22, 8) == wsb(1, 8, 1 << 22) == 0


def test_wrapper_checks(nm):
    d = np.zeros((8, 128), np.uint8)

    def ok(k=2, **kw):
        a = dict(As=[d], nAs=[8], Bs=[d], nBs=[8])
        a.update(kw)
        return nm.sift_match_knn_u8_host(a.pop("As"), a.pop("nAs"), a.pop("Bs"), a.pop("nBs"), k, **a)

    idx, dist = ok()
    assert idx.shape == dist.shape == (1, 8, 2) and ok(capA=5)[0].shape == (1, 5, 2) and ok(want_distance=False)[1] is None
    assert nm.MATCH_KNN_U8_MAX_BATCH == 64 and nm.MATCH_KNN_U8_MAX_K == 8
    idx, dist = ok(k=8, nAs=[3], nBs=[2])                      # default prior: the values of an empty slot
    assert (idx[0, :3, :2] == [0, 1]).all() and (idx[0, :3, 2:] == -1).all() and (idx[0, 3:] == -1).all()
    assert (dist[0, :3, :2] == 0).all() and (dist[0, :3, 2:] == 0x7fffffff).all() and (dist[0, 3:] == 0x7fffffff).all()
    for kw in (dict(k=0), dict(k=9), dict(k=2.0), dict(capA=9), dict(capB=0), dict(As=[np.zeros((8, 64), np.uint8)]),
               dict(nAs=[8, 8]), dict(As=[], nAs=[], Bs=[], nBs=[]), dict(As=[d] * 65, nAs=[8] * 65, Bs=[d] * 65, nBs=[8] * 65)):
        with pytest.raises(nm.NmError):
            ok(**kw)
    import torch
    td, one = torch.zeros(8, 128, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(nm.NmError):                            # the device wrapper wants device tensors
        nm.sift_match_knn_u8_batch_dev([td], [one], [td], [one], 2)
    with pytest.raises(nm.NmError):
        nm.MatchKnnU8Workspace(65, 8, 8, device="cpu")
