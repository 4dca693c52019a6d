"""An independent restatement of homography-guided matching over unsigned-char descriptors (nm_sift_match_guided_u8_*), for
the tests.

Built from parts that exist apart from the product's code (csrc/nm_match_guided_u8_math.hpp): the gate is
guided_ref.gate_matrix (ransac_refit_ref.is_inlier32, the numpy float32 replay of nmr_is_inlier) with
ransac_refit_ref.valid_rows, the distances are int64 numpy sums of squared byte differences cast to float32 (exact: at most
128 * 255^2 < 2^23), and the scan is guided_ref.scan. Every step is fully specified, so the product must equal this
exactly: no tolerance, no excluded rows.
"""
import numpy as np

import guided_ref as G
import ransac_refit_ref as F

D_MAX = 128 * 255 * 255


def distances(A, B):
    """(len(A), len(B)) float32: the exact integer squared distances of uint8 rows."""
    A, B = np.asarray(A), np.asarray(B)
    assert A.dtype == np.uint8 and B.dtype == np.uint8
    t = A.astype(np.int64)[:, None, :] - B.astype(np.int64)[None, :, :]
    D = (t * t).sum(-1)
    assert D.min(initial=0) >= 0 and D.max(initial=0) <= D_MAX
    return D.astype(np.float32)


def guided(A, ax, ay, nA, B, bx, by, nB, H, status=1, radius2=9.0, ambiguity=0.8, max_distance=np.inf, capA=None, capB=None):
    """One pair. Returns (result (capA,) int32, count, best (capA,) float32)."""
    A, B = np.asarray(A), np.asarray(B)
    capA = len(A) if capA is None else capA
    capB = len(B) if capB is None else capB
    nA, nB = min(max(int(nA), 0), capA), min(max(int(nB), 0), capB)
    H = np.asarray(H, np.float32).reshape(9)
    result = np.full(capA, -1, np.int32)
    best = np.full(capA, G.INF, np.float32)
    if status != 1 or not np.isfinite(H).all() or nA == 0 or nB == 0:
        return result, 0, best
    ax, ay = np.asarray(ax, np.float32)[:nA], np.asarray(ay, np.float32)[:nA]
    bx, by = np.asarray(bx, np.float32)[:nB], np.asarray(by, np.float32)[:nB]
    for r0 in range(0, nA, 256):                                      # blocks of rows keep the distance tensors small
        gate = G.gate_matrix(H, ax[r0:r0 + 256], ay[r0:r0 + 256], bx, by, radius2) & F.valid_rows(ax[r0:r0 + 256])[:, None]
        for i in np.flatnonzero(gate.any(axis=1)):
            js = np.flatnonzero(gate[i])
            loc, best[r0 + i] = G.scan(distances(A[r0 + i:r0 + i + 1], B[js])[0], ambiguity, max_distance)
            if loc >= 0:
                result[r0 + i] = js[loc]
    return result, int((result >= 0).sum()), best
