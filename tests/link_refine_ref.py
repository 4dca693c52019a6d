"""The direct link refinement (include/nm_abi.h, "Batched direct (photometric) refinement") restated in numpy, apart from
the C++ functions.

sums_ref     the 67 sums of one walk: the verification's integer levels and sample (restated in link_verify_ref.py), the
             Jacobian in float64 with every product and sum rounded on its own, added in the WRITTEN ORDER: virtual
             workgroup, wave, lane, then the butterfly, the waves and the rows.
refine_ref   the whole call for one pair: walks, Cholesky solve, step and stop rule, with exact fused multiply-adds from
             Fractions where the header writes fma.
model_f64    a second, UNQUANTISED model of the same algorithm: true bilinear weights, gray values instead of levels,
             plain float64 sums, numpy.linalg.solve.
"""
import math
from fractions import Fraction

import numpy as np

import link_verify_ref as V

F32 = np.float32
TRANSLATION, AFFINE, HOMOGRAPHY = 0, 1, 2
END_ITERATIONS, END_CONVERGED, END_UNUSABLE, END_FEW_PIXELS, END_SINGULAR, END_STEP = range(6)
GAIN_SCALE, BIAS_SCALE, CONVERGED_STEP = 4.0, 8192.0, 2.0 ** -7
SUMS, S_JTR, S_RR, S_L = 67, 55, 65, 66
COLUMNS = {TRANSLATION: [2, 5, 8, 9], AFFINE: [0, 1, 2, 3, 4, 5, 8, 9], HOMOGRAPHY: list(range(10))}


def fma(a, b, c):
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def e_of(i, j):
    return 10 * i - i * (i - 1) // 2 + (j - i)


def pixels_int(A, B, H, mask, stride):
    """Per lattice pixel (row-major over the lattice): x, y, in L, in the verification's N, qa, qb."""
    A, B = np.asarray(A, F32), np.asarray(B, F32)
    fh, fw = A.shape
    seen = np.ones((fh, fw), bool) if mask is None else (np.asarray(mask, F32) > 0.5)
    x, y = V.lattice(fw, fh, stride)
    okA, qa = V.levels(A[y, x])
    inL = seen[y, x] & okA
    den, xp, yp = V.project32(H, x.astype(F32), y.astype(F32))
    with np.errstate(all="ignore"):
        ok = inL & np.isfinite(den) & (den > 0)
        xb, yb = (xp + F32(0.5)) - F32(0.5), (yp + F32(0.5)) - F32(0.5)
        ok &= (xb >= -1) & (xb < F32(fw)) & (yb >= -1) & (yb < F32(fh))
        xb, yb = np.where(ok, xb, F32(0)), np.where(ok, yb, F32(0))
        fi, fj = np.floor(xb), np.floor(yb)
        a = np.floor((xb - fi) * F32(256) + F32(0.5)).astype(np.int64)
        b = np.floor((yb - fj) * F32(256) + F32(0.5)).astype(np.int64)
    i, j = fi.astype(np.int64), fj.astype(np.int64)
    ok &= (i >= 0) & (i + 1 < fw) & (j >= 0) & (j + 1 < fh)
    i, j = np.where(ok, i, 0), np.where(ok, j, 0)
    acc = np.full(x.shape, 32768, np.int64)
    for t, w in enumerate(((256 - a) * (256 - b), a * (256 - b), (256 - a) * b, a * b)):
        ii, jj = np.where(ok, i + (t & 1), 0), np.where(ok, j + (t >> 1), 0)   # a rejected pixel reads (0, 0): a frame of
        okB, qt = V.levels(B[jj, ii])                                           # one column or row has no (1, .) or (., 1)
        ok &= okB & seen[jj, ii]
        acc += w * qt
    return x, y, inL, ok, qa, acc >> 16, seen


def sums_ref(A, B, H, mask=None, stride=4):
    """The 67 sums of one walk under the fp32 map H, float64, in the written summation order."""
    A = np.asarray(A, F32)
    fh, fw = A.shape
    lw, lh = fw // stride, fh // stride
    tot = np.zeros(SUMS)
    if lw == 0 or lh == 0:
        return tot
    x, y, inL, inN, qa, qb, seen = pixels_int(A, B, H, mask, stride)
    q = {}
    for name, dx, dy in (("w", -1, 0), ("e", 1, 0), ("n", 0, -1), ("s", 0, 1)):
        xx, yy = x + dx, y + dy
        inside = (xx >= 0) & (xx < fw) & (yy >= 0) & (yy < fh)
        xx, yy = np.where(inside, xx, 0), np.where(inside, yy, 0)
        ok, lev = V.levels(A[yy, xx])
        inN = inN & inside & ok & seen[yy, xx]
        q[name] = lev
    h, cx, cy = 0.5 * max(fw, fh), 0.5 * (fw - 1), 0.5 * (fh - 1)
    X, Y = (x.astype(np.float64) - cx) / h, (y.astype(np.float64) - cy) / h
    gX = h * (0.5 * (q["e"] - q["w"]).astype(np.float64))
    gY = h * (0.5 * (q["s"] - q["n"]).astype(np.float64))
    d = gX * X + gY * Y
    J = [gX * X, gX * Y, gX, gY * X, gY * Y, gY, -(X * d), -(Y * d), GAIN_SCALE * qa.astype(np.float64),
         np.full(x.shape, BIAS_SCALE)]
    r = (qb - qa).astype(np.float64)
    terms = np.zeros((x.size, SUMS))
    for i in range(10):
        for j in range(i, 10):
            terms[:, e_of(i, j)] = J[i] * J[j]
        terms[:, S_JTR + i] = J[i] * r
    terms[:, S_RR] = r * r
    terms[~inN] = 0.0                      # a running sum that starts at +0 is never -0: adding +0 leaves it as it is
    terms[:, S_L] = inL.astype(np.float64)
    # the written order: who adds a pixel, and when
    u, v = np.meshgrid(np.arange(lw), np.arange(lh))
    u, v = u.reshape(-1), v.reshape(-1)
    tiles_x = -(-lw // 64)
    tiles = tiles_x * -(-lh // 32)
    t = (v // 32) * tiles_x + u // 64
    g, lane, wave = t % 256, u % 64, (v % 32) % 4
    when = (t // 256) * 8 + (v % 32) // 4
    parts = min(tiles, 256)
    acc = np.zeros((parts, 4, 64, SUMS))
    for step in np.unique(when):
        sel = when == step
        acc[g[sel], wave[sel], lane[sel]] = acc[g[sel], wave[sel], lane[sel]] + terms[sel]
    for dd in (32, 16, 8, 4, 2, 1):
        acc[:, :, :dd] = acc[:, :, :dd] + acc[:, :, dd:2 * dd]
    rows = np.zeros((parts, SUMS))
    for w in range(4):
        rows = rows + acc[:, w, 0]
    for p in range(parts):
        tot = tot + rows[p]
    return tot


def solve_ref(tot, model):
    """(ok, p[8], alpha, beta): the Cholesky solve in the written order."""
    idx = COLUMNS[model]
    m = len(idx)
    Lm = [[0.0] * m for _ in range(m)]
    for j in range(m):
        d = float(tot[e_of(idx[j], idx[j])])
        for k in range(j):
            d = fma(-Lm[j][k], Lm[j][k], d)
        if not (d > 0 and math.isfinite(d)):
            return False, None, 0.0, 0.0
        Lm[j][j] = math.sqrt(d)
        for i in range(j + 1, m):
            t = float(tot[e_of(idx[j], idx[i])])
            for k in range(j):
                t = fma(-Lm[i][k], Lm[j][k], t)
            Lm[i][j] = t / Lm[j][j]
    yv, xv = [0.0] * m, [0.0] * m
    for i in range(m):
        t = float(tot[S_JTR + idx[i]])
        for k in range(i):
            t = fma(-Lm[i][k], yv[k], t)
        yv[i] = t / Lm[i][i]
    for i in range(m - 1, -1, -1):
        t = yv[i]
        for k in range(i + 1, m):
            t = fma(-Lm[k][i], xv[k], t)
        xv[i] = t / Lm[i][i]
    p = [0.0] * 8
    for i, c in enumerate(idx):
        if c < 8:
            p[c] = xv[i]
    return all(math.isfinite(v) for v in xv), p, xv[m - 2], xv[m - 1]


def mul3(P, Q):
    return [fma(P[3 * r + 2], Q[6 + c], fma(P[3 * r + 1], Q[3 + c], P[3 * r] * Q[c])) for r in range(3) for c in range(3)]


def adjugate3(t):
    return [fma(t[4], t[8], -(t[7] * t[5])), fma(t[2], t[7], -(t[1] * t[8])), fma(t[1], t[5], -(t[2] * t[4])),
            fma(t[5], t[6], -(t[3] * t[8])), fma(t[0], t[8], -(t[2] * t[6])), fma(t[3], t[2], -(t[0] * t[5])),
            fma(t[3], t[7], -(t[6] * t[4])), fma(t[6], t[1], -(t[0] * t[7])), fma(t[0], t[4], -(t[3] * t[1]))]


def step_map(p, fw, fh):
    h, cx, cy = 0.5 * max(fw, fh), 0.5 * (fw - 1), 0.5 * (fh - 1)
    W = [1.0 + p[0], p[1], p[2], p[3], 1.0 + p[4], p[5], p[6], p[7], 1.0]
    T = [1.0 / h, 0.0, -(cx / h), 0.0, 1.0 / h, -(cy / h), 0.0, 0.0, 1.0]
    Ti = [h, 0.0, cx, 0.0, h, cy, 0.0, 0.0, 1.0]
    return mul3(Ti, mul3(W, T))


def corner_step(M, fw, fh):
    size, ok = 0.0, True
    for x, y in ((0.0, 0.0), (float(fw), 0.0), (float(fw), float(fh)), (0.0, float(fh))):
        den = fma(M[6], x, fma(M[7], y, M[8]))
        if not den > 0:
            return math.inf
        dx = fma(M[0], x, fma(M[1], y, M[2])) / den - x
        dy = fma(M[3], x, fma(M[4], y, M[5])) / den - y
        dist = math.sqrt(fma(dx, dx, dy * dy))
        ok = ok and math.isfinite(dist)
        size = max(size, dist)
    return size if ok else math.inf


def refine_ref(A, B, H_in, mask=None, status_in=1, model=HOMOGRAPHY, stride=4, iterations=4, min_pixels=64, max_step=16.0):
    """One pair: (H_out float32[9], status_out, stats[9])."""
    H_in = np.asarray(H_in, F32).reshape(9)
    fh, fw = np.shape(A)
    stats = np.zeros(9)
    if status_in != 1 or not np.isfinite(H_in).all():
        stats[8] = END_UNUSABLE
        return H_in.copy(), 0, stats
    H = [float(v) for v in H_in]
    Hf, applied, rms_first = H_in.copy(), 0, 0.0
    for it in range(iterations):
        tot = sums_ref(A, B, Hf, mask, stride)
        N = float(tot[54]) / (BIAS_SCALE * BIAS_SCALE)
        rms = math.sqrt(float(tot[S_RR]) / N) / 16.0 if N > 0 else 0.0
        if it == 0:
            rms_first = rms
        stats[:] = 0.0
        stats[:4] = N, tot[S_L], rms_first, rms
        end = -1
        if not N >= min_pixels:
            end = END_FEW_PIXELS
        else:
            ok, p, alpha, beta = solve_ref(tot, model)
            if not ok:
                end = END_SINGULAR
            else:
                stats[4], stats[5] = fma(GAIN_SCALE, alpha, 1.0), (BIAS_SCALE * beta) / 16.0
                M = step_map(p, fw, fh)
                size = corner_step(M, fw, fh)
                stats[7] = size
                Hn = mul3(H, adjugate3(M))
                with np.errstate(all="ignore"):
                    Hn = [float(v) for v in np.array(Hn) / Hn[8]]
                    Hn32 = np.array(Hn, np.float64).astype(F32)
                if not (size <= float(F32(max_step)) and np.isfinite(Hn32).all()):
                    end = END_STEP
                else:
                    H, Hf, applied = Hn, Hn32, applied + 1
                    if size < CONVERGED_STEP:
                        end = END_CONVERGED
        if end < 0 and it == iterations - 1:
            end = END_ITERATIONS
        if end >= 0:
            break
    stats[6], stats[8] = applied, end
    return (Hf if applied else H_in).copy(), int(applied > 0), stats


def model_f64(A, B, H, mask=None, model=HOMOGRAPHY, stride=4, iterations=4):
    """The unquantised model: the refined map as float64 (3, 3). Gray values, true bilinear weights, float64 throughout."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    H = np.asarray(H, np.float64).reshape(3, 3).copy()
    fh, fw = A.shape
    seen = np.ones((fh, fw), bool) if mask is None else (np.asarray(mask) > 0.5)
    x, y = V.lattice(fw, fh, stride)
    keep = (x >= 1) & (x + 1 < fw) & (y >= 1) & (y + 1 < fh)
    x, y = x[keep], y[keep]
    good = lambda img, yy, xx: seen[yy, xx] & (img[yy, xx] >= 0) & (img[yy, xx] <= 255)
    with np.errstate(all="ignore"):
        keep = good(A, y, x) & good(A, y, x - 1) & good(A, y, x + 1) & good(A, y - 1, x) & good(A, y + 1, x)
    x, y = x[keep], y[keep]
    h, cx, cy = 0.5 * max(fw, fh), 0.5 * (fw - 1), 0.5 * (fh - 1)
    X, Y = (x - cx) / h, (y - cy) / h
    gX, gY = h * 0.5 * (A[y, x + 1] - A[y, x - 1]), h * 0.5 * (A[y + 1, x] - A[y - 1, x])
    d = gX * X + gY * Y
    a = A[y, x]
    J = np.stack([gX * X, gX * Y, gX, gY * X, gY * Y, gY, -X * d, -Y * d, a, np.ones_like(a)], 1)[:, COLUMNS[model]]
    T = np.array([[1 / h, 0, -cx / h], [0, 1 / h, -cy / h], [0, 0, 1]])
    for _ in range(iterations):
        den = H[2, 0] * x + H[2, 1] * y + H[2, 2]
        xp, yp = (H[0, 0] * x + H[0, 1] * y + H[0, 2]) / den, (H[1, 0] * x + H[1, 1] * y + H[1, 2]) / den
        ok = (den > 0) & (xp >= 0) & (xp < fw - 1) & (yp >= 0) & (yp < fh - 1)
        i, j = np.floor(np.where(ok, xp, 0)).astype(int), np.floor(np.where(ok, yp, 0)).astype(int)
        fx, fy = xp - i, yp - j
        b = np.zeros(x.shape)
        for t, w in enumerate(((1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy)):
            ii, jj = i + (t & 1), j + (t >> 1)
            with np.errstate(all="ignore"):
                ok &= good(B, jj, ii)
            b += w * np.where(np.isfinite(B[jj, ii]), B[jj, ii], 0.0)
        Jk, rk = J[ok], (b - a)[ok]
        sol = np.linalg.solve(Jk.T @ Jk, Jk.T @ rk)
        p = np.zeros(8)
        p[[c for c in COLUMNS[model] if c < 8]] = sol[:-2]
        W = np.array([[1 + p[0], p[1], p[2]], [p[3], 1 + p[4], p[5]], [p[6], p[7], 1]])
        H = H @ np.linalg.inv(np.linalg.inv(T) @ W @ T)
        H = H / H[2, 2]
    return H


def corner_error(H, H_true, fw, fh):
    """The largest distance between the images of the four frame corners under the two maps, in pixels."""
    c = np.array([[0, 0, 1], [fw, 0, 1], [fw, fh, 1], [0, fh, 1]], np.float64).T
    p, q = np.asarray(H, np.float64).reshape(3, 3) @ c, np.asarray(H_true, np.float64).reshape(3, 3) @ c
    return float(np.max(np.hypot(p[0] / p[2] - q[0] / q[2], p[1] / p[2] - q[1] / q[2])))
