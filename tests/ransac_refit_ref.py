"""A plain float64 restatement of the inlier refit (nm_ransac_refit_*), written from the definitions (numpy only).

Nothing here follows the product's operation sequence (csrc/nm_ransac_refit_math.hpp): the translation is the mean of
dst - src, the similarity the closed-form complex least squares on centred points, the homography the textbook normalised
DLT over all rows (two equations per row, Hartley normalisation, numpy.linalg.svd of the 2N x 9 design matrix,
denormalisation by 3x3 products). `is_inlier32` alone replays the product's float32 inlier test, operation by operation.
"""
import numpy as np

import ransac_ref as R

MIN_INLIERS = {0: 1, 1: 2, 2: 4}


# ------------------------------------------------------------------------------------ the float32 inlier test, replayed
def _fma32(a, b, c):
    """fmaf(a, b, c) for float32 arrays: the product of two float32 is exact in float64; the sum is rounded to odd in
    float64 (TwoSum tells whether it was exact), which makes the final rounding to float32 the single rounding of fmaf."""
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        c = c.astype(np.float64)
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def is_inlier32(H, sx, sy, dx, dy, thr):
    """nmr_is_inlier's sequence (csrc/nm_ransac_math.hpp) in numpy float32; H: 9 float32 values. Validity is not tested here."""
    H = np.asarray(H, np.float32).reshape(9)
    sx, sy, dx, dy = (np.asarray(a, np.float32) for a in (sx, sy, dx, dy))
    h = lambda i: np.full(sx.shape, H[i], np.float32)
    with np.errstate(all="ignore"):
        x = _fma32(h(0), sx, h(1) * sy) + h(2)
        y = _fma32(h(3), sx, h(4) * sy) + h(5)
        z = _fma32(h(6), sx, h(7) * sy) + h(8)
        x = x / z
        y = y / z
        ex, ey = dx - x, dy - y
        return _fma32(ex, ex, ey * ey) < np.float32(thr)


def valid_rows(sx, matches=None, nA=None):
    """RANSAC's valid rows: below nA, matched, src_x >= 0."""
    sx = np.asarray(sx, np.float32)
    ok = sx >= np.float32(0)
    if matches is not None:
        ok &= np.asarray(matches)[:len(sx)] >= 0
    if nA is not None:
        ok &= np.arange(len(sx)) < nA
    return ok


# ---------------------------------------------------------------------------------------------------------- the fits
def _hartley(x, y):
    cx, cy = x.mean(), y.mean()
    s = np.sqrt(2.0) / np.sqrt((x - cx) ** 2 + (y - cy) ** 2).mean()
    T = np.array([[s, 0, -s * cx], [0, s, -s * cy], [0, 0, 1.0]])
    return T


def fit64(model, sx, sy, dx, dy):
    """The least-squares map of `model` through ALL the given correspondences, float64, 3 x 3 with H[2, 2] = 1."""
    sx, sy, dx, dy = (np.asarray(a, np.float64) for a in (sx, sy, dx, dy))
    H = np.eye(3)
    with np.errstate(all="ignore"):
        if model == 0:
            H[0, 2], H[1, 2] = (dx - sx).mean(), (dy - sy).mean()
            return H
        if model == 1:
            s, d = sx + 1j * sy, dx + 1j * dy
            sc, dc = s - s.mean(), d - d.mean()
            a = (np.conj(sc) * dc).sum() / (np.abs(sc) ** 2).sum()
            t = d.mean() - a * s.mean()
            return np.array([[a.real, -a.imag, t.real], [a.imag, a.real, t.imag], [0, 0, 1.0]])
        Ts, Td = _hartley(sx, sy), _hartley(dx, dy)
        if not (np.isfinite(Ts).all() and np.isfinite(Td).all()):
            return np.full((3, 3), np.nan)
        ax, ay = Ts[0, 0] * sx + Ts[0, 2], Ts[1, 1] * sy + Ts[1, 2]
        bx, by = Td[0, 0] * dx + Td[0, 2], Td[1, 1] * dy + Td[1, 2]
        n = len(sx)
        A = np.zeros((2 * n, 9))
        A[0::2, 3], A[0::2, 4], A[0::2, 5] = -ax, -ay, -1
        A[0::2, 6], A[0::2, 7], A[0::2, 8] = by * ax, by * ay, by
        A[1::2, 0], A[1::2, 1], A[1::2, 2] = ax, ay, 1
        A[1::2, 6], A[1::2, 7], A[1::2, 8] = -bx * ax, -bx * ay, -bx
        _, _, Vh = np.linalg.svd(A, full_matrices=False) if 2 * n >= 9 else np.linalg.svd(A, full_matrices=True)
        Hn = Vh[-1].reshape(3, 3)
        M = np.linalg.inv(Td) @ Hn @ Ts
        return M / M[2, 2]


def d2_64(H, sx, sy, dx, dy):
    """Squared reprojection distance in float64."""
    px, py = R.apply64(np.asarray(H, np.float64).reshape(3, 3), sx, sy)
    return (np.asarray(dx, np.float64) - px) ** 2 + (np.asarray(dy, np.float64) - py) ** 2


def refit64(model, sx, sy, dx, dy, H_in, thr, rounds, valid=None):
    """The round rule in float64: S = rows with d2 < thr under the current map; fit all of S; accept when the fit is finite and
    keeps at least as many inliers. Returns (H (3, 3) float64, count, rounds_done)."""
    valid = valid_rows(sx) if valid is None else valid
    H = np.asarray(H_in, np.float64).reshape(3, 3)
    with np.errstate(all="ignore"):
        S = valid & (d2_64(H, sx, sy, dx, dy) < thr)
        done = 0
        for _ in range(rounds):
            if S.sum() < MIN_INLIERS[model]:
                break
            Hn = fit64(model, sx[S], sy[S], dx[S], dy[S])
            if not np.isfinite(Hn).all():
                break
            Sn = valid & (d2_64(Hn, sx, sy, dx, dy) < thr)
            if Sn.sum() < S.sum():
                break
            H, S, done = Hn, Sn, done + 1
    return H, int(S.sum()), done


def rounding_error(H64, W, Hh):
    """Corner displacement, in pixels, of the float64 map rounded to float32: what no float32-output fit can avoid."""
    return float(R.corner_distance64(np.asarray(H64, np.float64).astype(np.float32).reshape(1, 9).astype(np.float64),
                                     np.asarray(H64, np.float64).reshape(1, 3, 3), W, Hh)[0])


def corner_error(H, M, W, Hh):
    return float(R.corner_distance64(np.asarray(H, np.float64).reshape(1, 9), np.asarray(M, np.float64).reshape(1, 3, 3), W, Hh)[0])
