"""The link verification (include/nm_abi.h, "Batched link verification") restated in numpy, apart from the C++ functions.

verify_int   the written semantics: fp32 projection with exact fused multiply-adds, the sampler's 1/256 weights as
             integers, 1/16 levels, Python-int sums, the finalize in float64 with exact fused multiply-adds (Fractions),
             the corner geometry in float32 / float64.
model_f64    a second, UNQUANTISED model: the map, true bilinear weights and all sums in float64, no levels.
"""
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
UNUSABLE, FEW_INLIERS, BAD_GEOMETRY, LOW_OVERLAP, LOW_NCC = 1, 2, 4, 8, 16


def fma32(a, b, c):
    """round32(a * b + c) of float32 arrays, exactly. The product of two float32 is exact in float64; the sum is rounded to
    ODD in float64 (TwoSum gives the exact error), and 53 >= 24 + 2 bits make the second rounding to float32 innocuous."""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        even = (np.atleast_1d(s).view(np.int64).reshape(np.shape(s)) & 1) == 0
        fix = even & (e != 0) & np.isfinite(s)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def fma64(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def project32(m, x, y):
    """project_den / project of csrc/nm_warp_math.hpp on float32 arrays: (den, xp, yp)"""
    m = np.asarray(m, F32).reshape(9)
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    with np.errstate(all="ignore"):
        a = fma32(m[0], x, m[1] * y) + m[2]
        b = fma32(m[3], x, m[4] * y) + m[5]
        s = fma32(m[6], x, m[7] * y) + m[8]
        return s, a / s, b / s


def lattice(fw, fh, stride):
    u, v = np.arange(fw // stride), np.arange(fh // stride)
    x, y = np.meshgrid(stride * u + stride // 2, stride * v + stride // 2)
    return x.reshape(-1).astype(np.int64), y.reshape(-1).astype(np.int64)


def levels(v):
    """(has a level, the level) of float32 values"""
    v = np.asarray(v, F32)
    with np.errstate(all="ignore"):
        ok = (v >= 0) & (v <= 255)
        q = np.where(ok, np.rint(v * F32(16)), 0).astype(np.int64)
    return ok, q


def sums_int(A, B, H, mask=None, stride=4):
    """The seven sums (Python ints): L, N, sum qa, sum qb, sum qa^2, sum qb^2, sum qa qb."""
    A, B = np.asarray(A, F32), np.asarray(B, F32)
    fh, fw = A.shape
    seen = np.ones((fh, fw), bool) if mask is None else (np.asarray(mask, F32) > 0.5)
    x, y = lattice(fw, fh, stride)
    if x.size == 0:
        return [0] * 7
    okA, qa = levels(A[y, x])
    inL = seen[y, x] & okA
    den, xp, yp = project32(H, x.astype(F32), y.astype(F32))
    with np.errstate(all="ignore"):
        ok = inL & np.isfinite(den) & (den > 0)
        xb, yb = (xp + F32(0.5)) - F32(0.5), (yp + F32(0.5)) - F32(0.5)
        ok &= (xb >= -1) & (xb < F32(fw)) & (yb >= -1) & (yb < F32(fh))          # a NaN fails
        xb, yb = np.where(ok, xb, F32(0)), np.where(ok, yb, F32(0))
        fi, fj = np.floor(xb), np.floor(yb)
        a = np.floor((xb - fi) * F32(256) + F32(0.5)).astype(np.int64)
        b = np.floor((yb - fj) * F32(256) + F32(0.5)).astype(np.int64)
    i, j = fi.astype(np.int64), fj.astype(np.int64)
    ok &= (i >= 0) & (i + 1 < fw) & (j >= 0) & (j + 1 < fh)
    i, j = np.where(ok, i, 0), np.where(ok, j, 0)
    acc = np.full(x.shape, 32768, np.int64)
    weights = ((256 - a) * (256 - b), a * (256 - b), (256 - a) * b, a * b)
    assert all(int(v) == 65536 for v in sum(weights))
    for t, w in enumerate(weights):
        ii, jj = np.where(ok, i + (t & 1), 0), np.where(ok, j + (t >> 1), 0)   # a rejected pixel reads (0, 0): a frame of
        okB, qt = levels(B[jj, ii])                                             # one column or row has no (1, .) or (., 1)
        ok &= okB & seen[jj, ii]
        acc += w * qt
    qb = acc >> 16
    qa, qb = qa[ok].tolist(), qb[ok].tolist()
    return [int(inL.sum()), len(qa), sum(qa), sum(qb), sum(v * v for v in qa), sum(v * v for v in qb),
            sum(v * w for v, w in zip(qa, qb))]


def finalize(s):
    """The eight stats from the seven sums, in float64 in the written sequence."""
    L, N, Sa, Sb, Saa, Sbb, Sab = (float(v) for v in s)
    cov, va, vb = fma64(N, Sab, -(Sa * Sb)), fma64(N, Saa, -(Sa * Sa)), fma64(N, Sbb, -(Sb * Sb))
    overlap = N / L if s[0] else 0.0
    ncc = cov / math.sqrt(va * vb) if s[1] >= 2 and va > 0 and vb > 0 else 0.0
    gain = cov / va if s[1] >= 1 and va > 0 else 0.0
    unit = 16.0 * N
    bias = fma64(-gain, Sa, Sb) / unit if s[1] else 0.0
    return np.array([N, L, overlap, ncc, gain, bias, Sa / unit if s[1] else 0.0, Sb / unit if s[1] else 0.0], np.float64)


def geometry_ok(H, fw, fh, max_area_ratio):
    den, xp, yp = project32(H, np.array([0, fw, fw, 0], F32), np.array([0, 0, fh, fh], F32))
    if not (np.isfinite(den).all() and (den > 0).all()):
        return False
    if not (np.isfinite(xp).all() and np.isfinite(yp).all()):
        return False           # the C++ turns or the area are then infinite or NaN, and fail as well
    x, y = [float(v) for v in xp], [float(v) for v in yp]
    ex = [x[(c + 1) % 4] - x[c] for c in range(4)]
    ey = [y[(c + 1) % 4] - y[c] for c in range(4)]
    S, ok = 0.0, True
    for c in range(4):
        d = (c + 1) % 4
        ok = ok and fma64(ex[c], ey[d], -(ey[c] * ex[d])) > 0
        S = S + fma64(x[c], y[d], -(x[d] * y[c]))
    r = (0.5 * S) / (float(fw) * float(fh))
    return bool(ok and 1.0 / float(F32(max_area_ratio)) <= r <= float(F32(max_area_ratio)))


def verify_int(A, B, H, mask=None, stride=4, status_in=1, inliers=None, min_inliers=16, max_area_ratio=4.0,
               min_overlap=0.5, min_ncc=0.5):
    """One pair: (status_out, reason, stats[8], sums[7])."""
    H = np.asarray(H, F32).reshape(9)
    fh, fw = np.shape(A)
    if status_in != 1 or not np.isfinite(H).all():
        return 0, UNUSABLE, np.zeros(8), [0] * 7
    s = sums_int(A, B, H, mask, stride)
    stats = finalize(s)
    why = (LOW_OVERLAP if stats[2] < float(F32(min_overlap)) else 0) | (LOW_NCC if stats[3] < float(F32(min_ncc)) else 0)
    if inliers is not None and inliers < min_inliers:
        why |= FEW_INLIERS
    if not geometry_ok(H, fw, fh, max_area_ratio):
        why |= BAD_GEOMETRY
    return int(why == 0), why, stats, s


def model_f64(A, B, H, mask=None, stride=4):
    """The unquantised model of one pair: dict(N, L, overlap, ncc, gain, bias). The same lattice and the same rules of
    what counts, but the map, the bilinear weights (true fractions, not 1/256 steps), the gray values (no levels) and the
    sums are float64."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    H = np.asarray(H, np.float64).reshape(9)
    fh, fw = A.shape
    seen = np.ones((fh, fw), bool) if mask is None else (np.asarray(mask) > 0.5)
    x, y = lattice(fw, fh, stride)
    out = dict(N=0, L=0, overlap=0.0, ncc=0.0, gain=0.0, bias=0.0)
    if x.size == 0:
        return out
    a = A[y, x]
    with np.errstate(all="ignore"):
        inL = seen[y, x] & (a >= 0) & (a <= 255)
        den = H[6] * x + H[7] * y + H[8]
        xp, yp = (H[0] * x + H[1] * y + H[2]) / den, (H[3] * x + H[4] * y + H[5]) / den
        ok = inL & np.isfinite(den) & (den > 0) & np.isfinite(xp) & np.isfinite(yp)
        ok &= (xp >= 0) & (xp < fw - 1) & (yp >= 0) & (yp < fh - 1)
    xp, yp = np.where(ok, xp, 0.0), np.where(ok, yp, 0.0)
    i, j = np.floor(xp).astype(np.int64), np.floor(yp).astype(np.int64)
    fx, fy = xp - i, yp - j
    b = np.zeros(x.shape)
    for t, w in enumerate(((1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy)):
        ii, jj = i + (t & 1), j + (t >> 1)
        tap = B[jj, ii]
        with np.errstate(all="ignore"):
            ok &= seen[jj, ii] & (tap >= 0) & (tap <= 255)
        b += w * np.where(np.isfinite(tap), tap, 0.0)
    out["L"], out["N"] = int(inL.sum()), int(ok.sum())
    out["overlap"] = out["N"] / out["L"] if out["L"] else 0.0
    if out["N"] >= 2:
        a, b = a[ok], b[ok]
        da, db = a - a.mean(), b - b.mean()
        va, vb, cov = float(da @ da), float(db @ db), float(da @ db)
        if va > 0 and vb > 0:
            out["ncc"] = cov / math.sqrt(va * vb)
        if va > 0:
            out["gain"] = cov / va
            out["bias"] = float(b.mean() - out["gain"] * a.mean())
    return out
