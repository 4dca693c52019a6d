"""An independent restatement of mutual-nearest-neighbour filtering (nm_sift_match_mutual_*), for the tests.

Written from the entry's stated semantics, not from csrc/nm_match_mutual_math.hpp: the distances of a claimed column to every
row of A come from the CPU oracle's compute_brute_force_distance (oracle_lib.bf_distance, the reference's fma chain, no early
exit), and the column's first minimum is numpy.argmin over the rows whose distance is a number. Every step is fully specified
in float32, so the product must equal this exactly: no tolerance, no excluded rows.
"""
import numpy as np

import oracle_lib as O

INF = np.float32(np.inf)


def column_distances(A, B, cols):
    """(len(cols), len(A)) float32: d(i, j) for every row i of A and the listed columns j of B."""
    if len(cols) == 0 or len(A) == 0:
        return np.zeros((len(cols), len(A)), np.float32)
    At = O.transpose(np.ascontiguousarray(A, np.float32))
    out = np.empty((len(cols), len(A)), np.float32)
    for c0 in range(0, len(cols), 512):                              # blocks of columns keep the matrices small
        out[c0:c0 + 512] = O.bf_distance(At, np.ascontiguousarray(B[cols[c0:c0 + 512]], np.float32))
    return out


def first_minimum(col):
    """Index of the first minimum among the entries that are numbers (ascending scan, strict <); -1 when none is."""
    ok = np.flatnonzero(~np.isnan(col))
    return int(ok[np.argmin(col[ok])]) if len(ok) else -1


def mutual(A, nA, B, nB, matches, capA=None, capB=None):
    """One pair. Returns (result (capA,) int32, count, forward (capA,) float32)."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    matches = np.asarray(matches, np.int32)
    capA = min(len(A), len(matches)) if capA is None else capA
    capB = len(B) if capB is None else capB
    nA, nB = min(max(int(nA), 0), capA), min(max(int(nB), 0), capB)
    result = np.full(capA, -1, np.int32)
    forward = np.full(capA, INF, np.float32)
    m = matches[:nA]
    rows = np.flatnonzero((m >= 0) & (m < nB))
    if len(rows) == 0:
        return result, 0, forward
    cols = np.unique(m[rows])
    D = column_distances(A[:nA], B, cols)
    best = {int(j): first_minimum(D[c]) for c, j in enumerate(cols)}
    where = {int(j): c for c, j in enumerate(cols)}
    for i in rows:
        j = int(m[i])
        forward[i] = D[where[j], i]
        if best[j] == i:
            result[i] = j
    return result, int((result >= 0).sum()), forward
