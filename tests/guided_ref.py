"""An independent restatement of homography-guided matching (nm_sift_match_guided_*), for the tests.

Built from parts that exist apart from the product's code (csrc/nm_match_guided_math.hpp): the gate is
ransac_refit_ref.is_inlier32 (the numpy float32 replay of nmr_is_inlier), the distances come from the CPU oracle's
compute_brute_force_distance (oracle_lib.bf_distance) and the scan is get_sift_matches' written out in numpy float32. Every
step is fully specified in float32, so the product must equal this exactly: no tolerance, no excluded rows.
"""
import numpy as np

import oracle_lib as O
import ransac_refit_ref as F

MIN2_INIT = np.float32(2139095040.0)
INF = np.float32(np.inf)


def gate_matrix(H, ax, ay, bx, by, radius2):
    """(len(ax), len(bx)) bool: candidate j passes for row i. Vectorised over j with is_inlier32, row by row."""
    ax, ay, bx, by = (np.asarray(a, np.float32) for a in (ax, ay, bx, by))
    out = np.zeros((len(ax), len(bx)), bool)
    for i in range(len(ax)):
        out[i] = F.is_inlier32(H, np.full(len(bx), ax[i], np.float32), np.full(len(bx), ay[i], np.float32), bx, by, radius2)
    return out


def scan(dist, ambiguity, max_distance):
    """get_sift_matches over one row's gated distances in ascending candidate order; returns (local index or -1, min1)."""
    if len(dist) == 0:
        return -1, INF
    min1, min2, idx = np.float32(dist[0]), MIN2_INIT, 0
    for j in range(1, len(dist)):
        cur = np.float32(dist[j])
        if cur < min1:
            min2, idx, min1 = min1, j, cur
        elif cur < min2:
            min2 = cur
    if not min2 > 0:
        return -1, min1
    with np.errstate(all="ignore"):
        ok = np.float32(min1) / np.float32(min2) < np.float32(ambiguity) and min1 < np.float32(max_distance)
    return (idx if ok else -1), min1


def guided(A, ax, ay, nA, B, bx, by, nB, H, status=1, radius2=9.0, ambiguity=0.8, max_distance=np.inf, capA=None, capB=None):
    """One pair. Returns (result (capA,) int32, count, best (capA,) float32)."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    capA = len(A) if capA is None else capA
    capB = len(B) if capB is None else capB
    nA, nB = min(max(int(nA), 0), capA), min(max(int(nB), 0), capB)
    H = np.asarray(H, np.float32).reshape(9)
    result = np.full(capA, -1, np.int32)
    best = np.full(capA, INF, np.float32)
    if status != 1 or not np.isfinite(H).all() or nA == 0 or nB == 0:
        return result, 0, best
    ax, ay = np.asarray(ax, np.float32)[:nA], np.asarray(ay, np.float32)[:nA]
    bx, by = np.asarray(bx, np.float32)[:nB], np.asarray(by, np.float32)[:nB]
    for r0 in range(0, nA, 256):                                      # blocks of rows keep the distance matrices small
        G = gate_matrix(H, ax[r0:r0 + 256], ay[r0:r0 + 256], bx, by, radius2) & F.valid_rows(ax[r0:r0 + 256])[:, None]
        rows = np.flatnonzero(G.any(axis=1))
        if not len(rows):
            continue
        cols = np.flatnonzero(G[rows].any(axis=0))
        D = O.bf_distance(O.transpose(A[r0 + rows]), B[cols]).T       # (rows, cols), the oracle's fma chain
        for r, i in enumerate(rows):
            js = np.flatnonzero(G[i][cols])
            loc, best[r0 + i] = scan(D[r, js], ambiguity, max_distance)
            if loc >= 0:
                result[r0 + i] = cols[js[loc]]
    return result, int((result >= 0).sum()), best
