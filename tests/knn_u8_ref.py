"""An independent restatement of the u8 k-nearest-neighbour entry (nm_sift_match_knn_u8_*), shared by its host and GPU
tests.

Written from the header's words, not from csrc/nm_match_u8.hip: the exact int64 distance matrix of match_u8_ref, a STABLE
argsort of every row (ascending distance, equal distances in ascending index: the order (d, j)), its first k columns, then
the fill rule for nB < k and a pre-filled prior for the rows at and beyond nA. Everything is exact: array_equal, no
tolerance, no excluded rows.
"""
import numpy as np

import match_u8_ref as M

NO_INDEX, NO_DISTANCE = -1, 0x7fffffff
PRIOR = (-7, -9)                            # what the tests pre-fill index and distance with
KS = (1, 2, 3, 5, 8)


def knn(D, k):
    """(index, distance), rows x k int32, of the distance matrix D (rows x nB, nB >= 1)."""
    rows, nB = D.shape
    m = min(k, nB)
    order = np.argsort(D, axis=1, kind="stable")[:, :m]
    idx = np.full((rows, k), NO_INDEX, np.int32)
    dist = np.full((rows, k), NO_DISTANCE, np.int32)
    idx[:, :m] = order
    dist[:, :m] = np.take_along_axis(D, order, axis=1)
    return idx, dist


def expected(case, k, capA, capB=None, prior=PRIOR):
    """What the entry leaves in (capA, k) outputs pre-filled with `prior`; sizes clipped to the capacities."""
    capB = len(case["B"]) if capB is None else capB
    nA, nB = min(max(case["nA"], 0), capA), min(max(case["nB"], 0), capB)
    idx = np.full((capA, k), prior[0], np.int32)
    dist = np.full((capA, k), prior[1], np.int32)
    if nA > 0 and nB > 0:
        idx[:nA], dist[:nA] = knn(M.distances(case["A"][:nA], case["B"][:nB]), k)
    return idx, dist


def matcher_last_step(idx, dist, nB, ambiguity, prior):
    """The u8 matcher's last step on the first two columns of a k >= 2 list: min2 = 2139095040.0f when nB == 1, a row with
    min2 == 0 keeps its prior, result = min1 / min2 < ambiguity ? first index : -1 with an fp32 divide."""
    res = np.array(prior, np.int32).copy()
    min1 = dist[:, 0].astype(np.float32)
    min2 = np.full(len(idx), M.MIN2_INIT, np.float32) if nB == 1 else dist[:, 1].astype(np.float32)
    live = min2 > 0
    with np.errstate(all="ignore"):
        ratio = (min1 / np.where(live, min2, np.float32(1))).astype(np.float32)
    res[live] = np.where(ratio[live] < np.float32(ambiguity), idx[live, 0], -1)
    return res


def matcher_from_lists(case, idx, dist, ambiguity, capA, capB):
    """matcher_last_step on the rows below nA of a pair's (capA, k >= 2) lists; a result pre-filled with case['prior']."""
    nA, nB = min(max(case["nA"], 0), capA), min(max(case["nB"], 0), capB)
    res = np.full(capA, case["prior"], np.int32)
    if nA > 0 and nB > 0:
        res[:nA] = matcher_last_step(idx[:nA], dist[:nA], nB, ambiguity, res[:nA])
    return res


def extreme_cases():
    """match_u8_ref.extremes_case() as it is (70 candidates: the eight nearest of a row never include its farthest), then
    the same rows with nB = 8, where a k = 8 list holds every candidate and ends on 128 * 255^2 for the rows of all 0 and
    all 255."""
    c = M.extremes_case()[0]
    few = dict(c, nB=8, what="extremes, 8 candidates")
    assert M.distances(c["A"], c["B"][:8]).max() == 128 * 255 * 255
    return c, few


def tie_cases():
    """70 candidate rows and 40 queries. (a) every candidate identical: the eight nearest of every query are 0 .. 7, which
    span both lane halves (rows 0-3 | 4-7 of a tile). (b) identical rows at 28 .. 35 only, the others distinct and farther:
    the eight span the tile boundary 31 | 32."""
    rng = np.random.default_rng(21)
    same = rng.integers(60, 200, 128)
    A = same[None, :] + rng.integers(-9, 10, (40, 128))
    Ba = np.tile(same, (70, 1))
    Bb = same[None, :] + rng.integers(40, 56, (70, 128)) * rng.choice((-1, 1), (70, 128))
    Bb[28:36] = same
    a, b = M._case(A, Ba, what="70 identical candidates"), M._case(A, Bb, what="identical candidates at 28..35")
    Db = M.distances(A, Bb)
    far = np.delete(Db, np.s_[28:36], axis=1)
    assert (far.min(1) > Db[:, 28]).all() and (Db[:, 28:36] == Db[:, 28:29]).all() and len(np.unique(Bb, axis=0)) == 63
    return a, b
