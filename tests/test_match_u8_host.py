"""The u8 matcher through its host twin (nm_sift_match_u8_host) against two references, bit for bit: the exact int64
distance matrix put through the reference's scan (tests/match_u8_ref.py), and the CPU oracle's fp32 matcher on float
copies of the same bytes. No GPU. The cases are the GPU test's (tests/test_gpu_match_u8.py), plus the refusals.
"""
import ctypes as C

import numpy as np
import pytest

import match_u8_ref as M


def oracle_on_float_copies(oracle, case, capA, capB):
    nA, nB = min(max(case["nA"], 0), capA), min(max(case["nB"], 0), capB)
    res = np.full(capA, case["prior"], np.int32)
    if nA > 0 and nB > 0:
        res[:nA], _, _ = oracle.sift_matches(case["A"][:nA].astype(np.float32), case["B"][:nB].astype(np.float32), case["amb"],
                                             want_distance=False, prior=res[:nA])
    return res


def assert_case(nm, oracle, case):
    got = nm.sift_match_u8_host([case["A"]], [case["nA"]], [case["B"]], [case["nB"]], ambiguity=case["amb"], prior=case["prior"])[0]
    capA, capB = len(case["A"]), len(case["B"])
    want = M.expected_clipped(case, capA, capB)
    diff = np.flatnonzero(got != want)
    assert not len(diff), (case["what"], "restatement", diff[:5], got[diff[:5]], want[diff[:5]])
    ref = oracle_on_float_copies(oracle, case, capA, capB)
    diff = np.flatnonzero(got != ref)
    assert not len(diff), (case["what"], "oracle on float copies", diff[:5], got[diff[:5]], ref[diff[:5]])
    return got


def test_mixed_sizes(nm, oracle):
    matched = 0
    for case in M.mixed_size_cases():
        got = assert_case(nm, oracle, case)
        matched += int((got >= 0).sum())
    assert matched > 150                                       # the ratio test accepted rows, not only rejected them


def test_extremes_duplicates_and_single_candidates(nm, oracle):
    for case in M.extremes_case() + M.duplicate_cases() + M.single_candidate_cases():
        assert_case(nm, oracle, case)
    D = M.distances(*[M.extremes_case()[0][k] for k in ("A", "B")])
    assert D.max() == 128 * 255 * 255 and D.min() == 0


@pytest.mark.parametrize("n", [1, 3, 16, 64])
def test_ragged_batches(nm, oracle, n):
    cases, capA, capB = M.ragged_batch(n)
    k = lambda key: [c[key] for c in cases]
    assert len({c["amb"] for c in cases}) <= 2
    for amb in sorted({c["amb"] for c in cases}):               # one ambiguity per call
        got = nm.sift_match_u8_host(k("A"), k("nA"), k("B"), k("nB"), ambiguity=amb, capA=capA, capB=capB, prior=-7)
        for i, c in enumerate(cases):
            cc = dict(c, amb=amb)
            assert np.array_equal(got[i], M.expected_clipped(cc, capA, capB)), c["what"]
            assert np.array_equal(got[i], oracle_on_float_copies(oracle, cc, capA, capB)), c["what"]
    empty = [i for i, c in enumerate(cases) if c["nA"] <= 0 or c["nB"] <= 0]
    assert len(empty) == 1 and (got[empty[0]] == -7).all()
    alone = nm.sift_match_u8_host([cases[0]["A"]], [cases[0]["nA"]], [cases[0]["B"]], [cases[0]["nB"]], ambiguity=amb,
                                  capA=capA, capB=capB, prior=-7)
    assert np.array_equal(alone[0], got[0])                     # a pair's result does not depend on the batch


@pytest.mark.parametrize("amb", [0.8, 1.0])
def test_host_matcher_is_the_ratio_rule_on_the_host_k2_lists(nm, amb):
    """The host matcher is the host k-NN twin at k = 2 followed by the last step: its result equals that step restated in
    numpy on the host k = 2 lists, alone and as a 3-pair batch with the empty pair, and the restatement of the matcher."""
    import knn_u8_ref as K
    cases, capA, capB = M.shared_scan_cases()
    for batch in [[c] for c in cases] + [cases[1:]]:
        col = lambda key: [c[key] for c in batch]
        got = nm.sift_match_u8_host(col("A"), col("nA"), col("B"), col("nB"), ambiguity=amb, capA=capA, capB=capB, prior=-7)
        idx, dist = nm.sift_match_knn_u8_host(col("A"), col("nA"), col("B"), col("nB"), 2, capA=capA, capB=capB, prior=K.PRIOR)
        for p, c in enumerate(batch):
            assert np.array_equal(got[p], K.matcher_from_lists(c, idx[p], dist[p], amb, capA, capB)), c["what"]
            assert np.array_equal(got[p], M.expected_clipped(dict(c, amb=amb), capA, capB)), c["what"]
            assert (got[p][max(c["nA"], 0):] == -7).all(), "a row beyond nA was written"
    # the batch (identical, empty, ties): min2 == 0 kept, min2 == min1 rejected, nothing for the empty pair, ties by index
    assert (got[0][:32] == -7).all() and (got[0][32:65] == -1).all()
    assert (got[1] == -7).all() and tuple(idx[2][10]) == (1, 5) and tuple(idx[2][11]) == (0, 32)


def finished_real_pair(oracle, nm, rows=4096):
    """Two views of one synthetic scene, detected and described by the CPU oracle, finished by the host twin: (A, B) uint8."""
    import helpers as H
    out = []
    for shift in (0, 7):
        g = np.roll(H.blurred_frame(31, 1280, 960, sigma=1.6), shift, 1).astype(np.float32)
        f = oracle.sift_detect_describe(g, 16384)
        assert f["n"] >= rows, f["n"]
        _, u = nm.desc_finish_host([f["desc"][:rows]], [rows], want_f32=False)
        out.append(u[0])
    return out


def test_finished_real_descriptors_4096(nm, oracle):
    A, B = finished_real_pair(oracle, nm)
    case = dict(A=A, B=B, nA=4096, nB=4096, amb=0.8, prior=-1, what="4096 x 4096 finished descriptors")
    got = assert_case(nm, oracle, case)
    print("4096 x 4096 finished descriptors: %d matches" % (got >= 0).sum())
    assert (got >= 0).sum() > 400


def test_refusals(nm):
    lib = nm.lib()
    n = 2
    d = np.zeros((8, 128), np.uint8)
    cnt8 = np.array([8], np.int32)
    res = np.full((n, 8), 7, np.int32)
    ws = np.full(4096, 7, np.int32)
    tab = lambda a, k=n: (C.c_void_p * 64)(*([a.ctypes.data] * k))
    rows = lambda a, k=n: (C.c_void_p * 64)(*[a[i].ctypes.data for i in range(k)])

    def call(fn, n_=n, capA=8, capB=8, **kw):
        a = dict(A=tab(d), nA=tab(cnt8), B=tab(d), nB=tab(cnt8), result=rows(res), ws=ws.ctypes.data)
        a.update(kw)
        args = [n_, a["A"], a["nA"], capA, a["B"], a["nB"], capB, a["result"], 0.8]
        return fn(*(args + ([a["ws"], None] if fn is lib.nm_sift_match_u8_batch_dev else [])))

    assert call(lib.nm_sift_match_u8_host) == 0
    assert (res == 7).all()                                    # identical rows: min2 == 0, every entry kept
    bad = [dict(n_=0), dict(n_=-1), dict(n_=65), dict(capA=0), dict(capA=1 << 22), dict(capB=0), dict(capB=1 << 22)]
    bad += [dict([(k, None)]) for k in ("A", "nA", "B", "nB", "result")]
    bad += [dict([(k, tab(d if k in "AB" else cnt8, 1))]) for k in ("A", "nA", "B", "nB")]
    bad += [dict(result=rows(res, 1))]
    for fn in (lib.nm_sift_match_u8_host, lib.nm_sift_match_u8_batch_dev):       # both refuse before touching memory
        for kw in bad:
            assert call(fn, **kw) != 0, (fn.__name__, kw)
    assert call(lib.nm_sift_match_u8_batch_dev, ws=None) != 0
    odd = np.zeros(8 * 128 + 16, np.uint8)
    off = (-odd.ctypes.data) % 16 + 1                          # a descriptor pointer that is not 16-byte aligned
    assert call(lib.nm_sift_match_u8_batch_dev, A=(C.c_void_p * 64)(*([odd.ctypes.data + off] * n))) != 0
    assert (res == 7).all() and (ws == 7).all()
    for name in ("nm_sift_match_u8_batch_dev", "nm_sift_match_u8_host", "nm_sift_match_u8_workspace_bytes"):
        assert name in nm.ABI_SYMBOLS
    wsb = lib.nm_sift_match_u8_workspace_bytes
    assert wsb(1, 1, 1) > 0 and wsb(64, (1 << 22) - 1, 16384) > wsb(16, 16384, 16384) > wsb(1, 16384, 16384) >= 2 * 4 * 16384
    assert wsb(0, 8, 8) == wsb(65, 8, 8) == wsb(1, 0, 8) == wsb(1, 8, 0) == wsb(1, 1 << 22, 8) == wsb(1, 8, 1 << 22) == 0


def test_wrapper_checks(nm):
    d = np.zeros((8, 128), np.uint8)

    def ok(**kw):
        a = dict(As=[d], nAs=[8], Bs=[d], nBs=[8])
        a.update(kw)
        return nm.sift_match_u8_host(a.pop("As"), a.pop("nAs"), a.pop("Bs"), a.pop("nBs"), **a)

    assert ok().shape == (1, 8) and ok().dtype == np.int32 and ok(capA=5).shape == (1, 5) and nm.MATCH_U8_MAX_BATCH == 64
    for kw in (dict(capA=9), dict(capA=0), dict(capB=9), dict(capB=0), dict(As=[np.zeros((8, 64), np.uint8)]), dict(nAs=[8, 8]),
               dict(As=[], nAs=[], Bs=[], nBs=[]), dict(As=[d] * 65, nAs=[8] * 65, Bs=[d] * 65, nBs=[8] * 65)):
        with pytest.raises(nm.NmError):
            ok(**kw)
    import torch
    td, one = torch.zeros(8, 128, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(nm.NmError):                            # the device wrapper wants device tensors
        nm.sift_match_u8_batch_dev([td], [one], [td], [one])
    with pytest.raises(nm.NmError):
        nm.MatchU8Workspace(65, 8, 8, device="cpu")
