"""The gray pyramid and the pyramidal KLT tracker of include/nm_abi.h ("Gray pyramid and point tracking") in Python integers,
numpy float32 where the text says fp32 and Python floats (IEEE binary64, one operation per step) where it says fp64; written
from the header text. Every fp64 step is a single operation without contraction, so the model is expected to EQUAL the host
twin, not to approximate it. `lk_float64` is the yardstick of the accuracy tests: the same descent with continuous bilinear
weights, unquantised values and float64 sums. The module also holds the frames and point sets the host and GPU tests share.
"""
import math

import numpy as np

F32 = np.float32
OK, ABSENT, START, BORDER, FLAT, STEP, RESIDUAL, FB = range(8)


# ---- geometry ----
def sizes(fw, fh, levels):
    out = [(fw, fh)]
    for _ in range(levels - 1):
        w, h = out[-1]
        out.append(((w + 1) >> 1, (h + 1) >> 1))
    return out


def offsets(fw, fh, levels):
    """offsets of levels 0 .. levels (the last one is the block's size)"""
    off = [0]
    for w, h in sizes(fw, fh, levels):
        off.append(off[-1] + ((w * h + 3) // 4) * 4)
    return off


def _binom(a, axis):
    """(1 4 6 4 1) / 16 at the even positions along `axis`, indices clamped, in float32 operations as the header orders them"""
    n = a.shape[axis]
    c = 2 * np.arange((n + 1) >> 1)
    s = lambda t: np.take(a, np.clip(c + t, 0, n - 1), axis=axis)
    return (((s(-2) + s(2)) + F32(4) * (s(-1) + s(1))) + F32(6) * s(0)) * F32(0.0625)


def pyramid(gray, levels):
    planes = [np.asarray(gray, F32)]
    for _ in range(levels - 1):
        planes.append(_binom(_binom(planes[-1], 1), 0))
    return planes


def mask_pyramid(mask, levels):
    planes = [(np.asarray(mask, F32) > F32(0.5)).astype(np.uint8)]
    for _ in range(levels - 1):
        m = planes[-1]
        h, w = m.shape
        ys, xs = 2 * np.arange((h + 1) >> 1), 2 * np.arange((w + 1) >> 1)
        out = np.ones((len(ys), len(xs)), np.uint8)
        for v in range(-2, 3):
            for u in range(-2, 3):
                out &= m[np.clip(ys + v, 0, h - 1)][:, np.clip(xs + u, 0, w - 1)]
        planes.append(out)
    return planes


def block(planes, dtype):
    h, w = planes[0].shape
    off = offsets(w, h, len(planes))
    out = np.zeros(off[-1], dtype)
    for p, o in zip(planes, off):
        out[o:o + p.size] = p.reshape(-1)
    return out


# ---- the integer tracker ----
def quantise(planes, mask_planes=None):
    """per level: the levels as int64 and which pixels hold one (and are seen)"""
    out = []
    for l, p in enumerate(planes):
        with np.errstate(invalid="ignore"):
            ok = (p >= F32(0)) & (p <= F32(255))
            q = np.where(ok, np.rint(np.where(ok, p, F32(0)) * F32(16)), 0).astype(np.int64)
        if mask_planes is not None:
            ok = ok & (mask_planes[l] == 1)
        out.append((q, ok))
    return out


def window(w, h, cx, cy, R):
    """(i0, j0, weights) of a window, or None when it is outside; cx, cy are float32"""
    if not (cx >= 0 and cx < F32(w) and cy >= 0 and cy < F32(h)):
        return None
    fi, fj = np.floor(cx), np.floor(cy)
    ax = int(np.floor((cx - fi) * F32(256) + F32(0.5)))
    ay = int(np.floor((cy - fj) * F32(256) + F32(0.5)))
    i0, j0 = int(fi), int(fj)
    if not (i0 - R >= 0 and i0 + R + 1 < w and j0 - R >= 0 and j0 + R + 1 < h):
        return None
    return i0, j0, ((256 - ax) * (256 - ay), ax * (256 - ay), (256 - ax) * ay, ax * ay)


def samples(level, win, R):
    """the (2R+1)^2 samples of a window and which of them are valid"""
    q, ok = level
    i0, j0, (w00, w10, w01, w11) = win
    sl = (slice(j0 - R, j0 + R + 2), slice(i0 - R, i0 + R + 2))
    P, V = q[sl], ok[sl]
    S = (w00 * P[:-1, :-1] + w10 * P[:-1, 1:] + w01 * P[1:, :-1] + w11 * P[1:, 1:] + 32768) >> 16
    return S, V[:-1, :-1] & V[:-1, 1:] & V[1:, :-1] & V[1:, 1:]


def template(level, w, h, cx, cy, r):
    """(T, gx, gy, Gxx, Gxy, Gyy) or None; the four corner samples of the (2r+3)^2 window enter no difference and are not
    looked at"""
    win = window(w, h, cx, cy, r + 1)
    if win is None:
        return None
    S, V = samples(level, win, r + 1)
    V = V.copy()
    V[0, 0] = V[0, -1] = V[-1, 0] = V[-1, -1] = True
    if not V.all():
        return None
    T, gx, gy = S[1:-1, 1:-1], S[1:-1, 2:] - S[1:-1, :-2], S[2:, 1:-1] - S[:-2, 1:-1]
    return T, gx, gy, int((gx * gx).sum()), int((gx * gy).sum()), int((gy * gy).sum())


def mismatch(level, w, h, cx, cy, r, tpl):
    """(bx, by, sum |e|) or None"""
    win = window(w, h, cx, cy, r)
    if win is None:
        return None
    S, V = samples(level, win, r)
    if not V.all():
        return None
    e = S - tpl[0]
    return int((e * tpl[1]).sum()), int((e * tpl[2]).sum()), int(np.abs(e).sum())


def gate(Gxx, Gxy, Gyy, r, min_eig):
    """det, or None for a flat window"""
    a, b, c = float(Gxx), float(Gxy), float(Gyy)
    t2 = b * b
    det = a * c - t2
    if not (math.isfinite(det) and det > 0.0):
        return None
    dd = a - c
    lam = ((a + c) - math.sqrt(dd * dd + 4.0 * t2)) / 2.0
    return None if lam / float(1024 * (2 * r + 1) ** 2) < min_eig else det


def lk_step(Gxx, Gxy, Gyy, bx, by, det):
    a, b, c, x, y = float(Gxx), float(Gxy), float(Gyy), float(bx), float(by)
    with np.errstate(all="ignore"):
        sx = float(np.float64(2.0 * (c * x - b * y)) / np.float64(det))
        sy = float(np.float64(2.0 * (a * y - b * x)) / np.float64(det))
    return sx, sy


class Params:
    def __init__(self, fw, fh, levels=4, radius=7, iterations=10, eps=2.0 ** -6, max_step=16.0, min_eig=0.0, max_residual=0.0,
                 fb_max=0.0):
        self.fw, self.fh, self.levels, self.r, self.iterations = fw, fh, levels, radius, iterations
        self.eps, self.max_step, self.min_eig, self.max_residual, self.fb_max = (float(F32(v)) for v in (
            eps, max_step, min_eig, max_residual, fb_max))


def track(q, A, B, px, py, dx, dy, tpl_fn=template, mis_fn=mismatch, unit=16):
    """one track: (reason, dx, dy, residual); A, B are per-level planes as tpl_fn / mis_fn take them"""
    down = 1.0 / float(1 << (q.levels - 1))
    dx, dy = dx * down, dy * down
    szs = sizes(q.fw, q.fh, q.levels)
    tpl = None
    for l in range(q.levels - 1, -1, -1):
        w, h = szs[l]
        s = 1.0 / float(1 << l)
        plx, ply, ex, ey = px * s, py * s, dx, dy
        fail = 0
        tpl = tpl_fn(A[l], w, h, _c(plx, tpl_fn), _c(ply, tpl_fn), q.r)
        det = None
        if tpl is None:
            fail = BORDER
        else:
            det = gate(tpl[3], tpl[4], tpl[5], q.r, q.min_eig)
            if det is None:
                fail = FLAT
        it = 0
        while not fail:
            m = mis_fn(B[l], w, h, _c(plx + dx, tpl_fn), _c(ply + dy, tpl_fn), q.r, tpl)
            if m is None:
                fail = BORDER
                break
            sx, sy = lk_step(tpl[3], tpl[4], tpl[5], m[0], m[1], det)
            big = max(abs(sx), abs(sy))
            if not (math.isfinite(sx) and math.isfinite(sy)) or big > q.max_step:
                fail = STEP
                break
            dx, dy = dx - sx, dy - sy
            it += 1
            if big < q.eps or it >= q.iterations:
                break
        if fail:
            if l > 0:
                dx, dy = ex, ey
            else:
                return fail, dx, dy, -1.0
        if l > 0:
            dx, dy = dx * 2.0, dy * 2.0
    m = mis_fn(B[0], q.fw, q.fh, _c(px + dx, tpl_fn), _c(py + dy, tpl_fn), q.r, tpl)
    if m is None:
        return BORDER, dx, dy, -1.0
    resid = float(m[2]) / float(unit * (2 * q.r + 1) ** 2)
    if q.max_residual > 0.0 and resid > q.max_residual:
        return RESIDUAL, dx, dy, resid
    return OK, dx, dy, resid


def _c(v, tpl_fn):
    """a window centre: rounded to fp32 once for the integer tracker, left alone for the float64 yardstick"""
    return F32(v) if tpl_fn is template else v


def project(H, x, y):
    """project and project_den of csrc/nm_warp_math.hpp in float32: fmaf(m0, x, m1 y) + m2, one division per coordinate"""
    H = [F32(v) for v in np.asarray(H).reshape(-1)]
    fma = lambda a, b, c: F32(np.float64(a) * np.float64(b) + np.float64(c))      # exact product, one rounding
    with np.errstate(all="ignore"):
        a = fma(H[0], x, H[1] * y) + H[2]
        b = fma(H[3], x, H[4] * y) + H[5]
        s = fma(H[6], x, H[7] * y) + H[8]
        return a / s, b / s, s


def track_row(q, A, B, sx, sy, H=None, **kw):
    """(dst_x, dst_y, reason, residual, fb_error) of one row, as float32 / int"""
    sx, sy = F32(sx), F32(sy)
    none = (F32(-1), F32(-1))
    if not (sx >= 0 and np.isfinite(sx) and np.isfinite(sy)):
        return none + (ABSENT, F32(-1), F32(-1))
    dx = dy = 0.0
    if H is not None:
        xp, yp, den = project(H, sx, sy)
        if not (np.isfinite(den) and den > 0 and np.isfinite(xp) and np.isfinite(yp)):
            return none + (START, F32(-1), F32(-1))
        dx, dy = float(xp) - float(sx), float(yp) - float(sy)
    px, py = float(sx), float(sy)
    reason, dx, dy, resid = track(q, A, B, px, py, dx, dy, **kw)
    if reason:
        return none + (reason, F32(resid), F32(-1))
    qx, qy = F32(px + dx), F32(py + dy)
    fb = F32(-1)
    if q.fb_max > 0.0:
        r2, bx, by, _ = track(q, B, A, float(qx), float(qy), -dx, -dy, **kw)
        if r2:
            return none + (FB, F32(resid), fb)
        rx, ry = F32(float(qx) + bx), F32(float(qy) + by)
        err = max(abs(float(rx) - float(sx)), abs(float(ry) - float(sy)))
        fb = F32(err)
        if err > q.fb_max:
            return none + (FB, F32(resid), fb)
    return qx, qy, OK, F32(resid), fb


def track_pair(q, grayA, grayB, xs, ys, nA, capA, mask=None, H=None):
    """the tracker's outputs for one pair from the gray planes: dst_x, dst_y, matches, count, reason, residual, fb_error"""
    mp = None if mask is None else mask_pyramid(mask, q.levels)
    A, B = quantise(pyramid(grayA, q.levels), mp), quantise(pyramid(grayB, q.levels), mp)
    dst_x, dst_y, resid, fb = (np.full(capA, -1, F32) for _ in range(4))
    matches, reason = np.full(capA, -1, np.int32), np.full(capA, ABSENT, np.uint8)
    for i in range(min(max(int(nA), 0), capA)):
        dst_x[i], dst_y[i], reason[i], resid[i], fb[i] = track_row(q, A, B, xs[i], ys[i], H)
        if reason[i] == OK:
            matches[i] = i
    return dst_x, dst_y, matches, int((matches >= 0).sum()), reason, resid, fb


def usable(H, status):
    return H is not None and (status is None or status == 1) and bool(np.isfinite(np.asarray(H, F32)).all())


# ---- the float64 yardstick: continuous bilinear weights, no level quantisation, float64 sums ----
def pyramid64(gray, levels):
    """the same binomial pyramid in float64, scaled to the tracker's unit (16 per gray value)"""
    planes = [np.asarray(gray, np.float64) * 16.0]
    for _ in range(levels - 1):
        a = planes[-1]
        for axis in (1, 0):
            n = a.shape[axis]
            c = 2 * np.arange((n + 1) >> 1)
            s = lambda t: np.take(a, np.clip(c + t, 0, n - 1), axis=axis)
            a = (s(-2) + s(2) + 4.0 * (s(-1) + s(1)) + 6.0 * s(0)) / 16.0
        planes.append(a)
    return planes


def _samples64(p, w, h, cx, cy, R):
    if not (0 <= cx < w and 0 <= cy < h):
        return None
    i0, j0 = int(math.floor(cx)), int(math.floor(cy))
    if not (i0 - R >= 0 and i0 + R + 1 < w and j0 - R >= 0 and j0 + R + 1 < h):
        return None
    a, b = cx - i0, cy - j0
    P = p[j0 - R:j0 + R + 2, i0 - R:i0 + R + 2]
    return (1 - a) * (1 - b) * P[:-1, :-1] + a * (1 - b) * P[:-1, 1:] + (1 - a) * b * P[1:, :-1] + a * b * P[1:, 1:]


def _template64(p, w, h, cx, cy, r):
    S = _samples64(p, w, h, cx, cy, r + 1)
    if S is None:
        return None
    T, gx, gy = S[1:-1, 1:-1], S[1:-1, 2:] - S[1:-1, :-2], S[2:, 1:-1] - S[:-2, 1:-1]
    return T, gx, gy, float((gx * gx).sum()), float((gx * gy).sum()), float((gy * gy).sum())


def _mismatch64(p, w, h, cx, cy, r, tpl):
    S = _samples64(p, w, h, cx, cy, r)
    if S is None:
        return None
    e = S - tpl[0]
    return float((e * tpl[1]).sum()), float((e * tpl[2]).sum()), float(np.abs(e).sum())


def lk_float64(q, grayA, grayB, xs, ys, H=None):
    """dst (len, 2) float64 with NaN rows where the float64 tracker loses the point; the same gates as the stage"""
    A, B = pyramid64(grayA, q.levels), pyramid64(grayB, q.levels)
    out = np.full((len(xs), 2), np.nan)
    for i, (x, y) in enumerate(zip(xs, ys)):
        r = track_row(q, A, B, x, y, H, tpl_fn=_template64, mis_fn=_mismatch64)
        if r[2] == OK:
            out[i] = float(r[0]), float(r[1])
    return out


# ---- shared cases ----
def textured(seed, w, h, lo=20.0, hi=230.0):
    """a smooth random texture in [lo, hi]: sums of a few random sinusoids, float32"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    g = np.zeros((h, w))
    for _ in range(12):
        fx, fy, ph = rng.uniform(-0.35, 0.35), rng.uniform(-0.35, 0.35), rng.uniform(0, 2 * np.pi)
        g += rng.uniform(0.3, 1.0) * np.sin(fx * x + fy * y + ph)
    g = (g - g.min()) / (g.max() - g.min())
    return (lo + (hi - lo) * g).astype(F32)


def shifted(gray, dx, dy):
    """B with B(x + dx, y + dy) = A(x, y) for whole dx, dy; what enters at the edges repeats the edge"""
    h, w = gray.shape
    ys, xs = np.clip(np.arange(h) - dy, 0, h - 1), np.clip(np.arange(w) - dx, 0, w - 1)
    return np.ascontiguousarray(gray[ys][:, xs])


def edge_points(w, h, r):
    """points on the border, r + 1 from it, and at half-pixel and 1/512-pixel fractions; and two src_x < 0 rows"""
    m = r + 2
    pts = [(0, 0), (w - 1, h - 1), (m, m), (m - 1, m), (w - 1 - m, h - 1 - m), (w - m, h - 1 - m), (w / 2, h / 2),
           (w / 2 + 0.5, h / 2 + 0.5), (w / 2 + 1 / 512, h / 2 - 1 / 512), (w / 2 + 255 / 512, h / 2 + 511 / 512), (-1, 5), (-0.5, 7),
           (w / 3 + 0.25, h / 3 + 0.75), (2 * w / 3, h / 4), (w / 4 + 0.125, 3 * h / 4), (m + 0.5, h / 2), (w - 1 - m - 0.5, h / 2),
           (float("nan"), 4), (5, float("inf"))]
    a = np.array(pts, np.float64)
    return a[:, 0].astype(F32), a[:, 1].astype(F32)


def grid_points(w, h, count, r):
    """`count` points spread over the frame's inside, at quarter-pixel fractions"""
    k = np.arange(count)
    xs = (r + 3) + (k * 7.25) % (w - 2 * r - 7)
    ys = (r + 3) + (k * 3.5) % (h - 2 * r - 7)
    return xs.astype(F32), ys.astype(F32)


def cases():
    """The shared cases: dicts of name, A, B (gray planes), xs, ys, nA, capA, mask, H, status and the Params keywords. The
    host test runs the model on each; the GPU test compares device and host twin on the same."""
    out = []
    A97, A64 = textured(1, 97, 61), textured(2, 64, 64)
    B97, B64 = textured(1, 97 + 8, 61 + 8)[3:3 + 61, 5:5 + 97].copy(), shifted(A64, 2, -1)
    for r in (1, 3, 7):
        for levels in (1, 3, 4):
            for (A, B) in ((A97, B97), (A64, B64)):
                h, w = A.shape
                xs, ys = edge_points(w, h, r)
                out.append(dict(name="edges %dx%d r%d L%d" % (w, h, r, levels), A=A, B=B, xs=xs, ys=ys, nA=len(xs), capA=len(xs) + 3,
                                kw=dict(levels=levels, radius=r, iterations=5, fb_max=(1.0 if r == 3 else 0.0),
                                        max_residual=(12.0 if levels == 3 else 0.0), min_eig=(0.05 if r == 1 else 0.0))))
    xs, ys = grid_points(97, 61, 8, 3)
    flat = np.full((61, 97), 77.25, F32)
    out.append(dict(name="flat", A=flat, B=flat, xs=xs, ys=ys, nA=8, capA=8, kw=dict(levels=3, radius=3)))
    out.append(dict(name="steps beyond max_step", A=A97, B=B97, xs=xs, ys=ys, nA=8, capA=8, kw=dict(levels=1, radius=3, max_step=0.05)))
    out.append(dict(name="min_eig above the texture", A=A97, B=B97, xs=xs, ys=ys, nA=8, capA=8, kw=dict(levels=2, radius=3, min_eig=1e4)))
    odd = A97.copy()
    odd[30, 40], odd[20, 60] = np.nan, 255.5
    out.append(dict(name="nan and 255.5", A=odd, B=B97, xs=np.r_[xs, F32(41.5), F32(59)], ys=np.r_[ys, F32(29.5), F32(21)], nA=10,
                    capA=10, kw=dict(levels=3, radius=3)))
    out.append(dict(name="nan in B", A=A97, B=odd, xs=np.r_[xs, F32(41.5), F32(59)], ys=np.r_[ys, F32(29.5), F32(21)], nA=10,
                    capA=10, kw=dict(levels=1, radius=3, fb_max=2.0)))
    # a mask hole next to (48, 30): inside the level-0 window; and one 22 px away: outside the level-0 window of radius 3
    # (+- 5 px) and inside level 2's reach (+- 5 level-2 pixels = +- 20 px, plus what the byte pyramid erodes)
    near, far = np.ones((61, 97), F32), np.ones((61, 97), F32)
    near[31, 50], far[30, 70] = 0.0, 0.5
    p = (np.array([48, 20], F32), np.array([30, 40], F32))
    out.append(dict(name="mask cuts level 0, one level", A=A97, B=B97, xs=p[0], ys=p[1], nA=2, capA=2, mask=near,
                    kw=dict(levels=1, radius=3)))
    out.append(dict(name="mask cuts level 0, three levels", A=A97, B=B97, xs=p[0], ys=p[1], nA=2, capA=2, mask=near,
                    kw=dict(levels=3, radius=3)))
    out.append(dict(name="mask cuts level 2 only", A=A97, B=B97, xs=p[0], ys=p[1], nA=2, capA=2, mask=far,
                    kw=dict(levels=3, radius=3)))
    gx, gy = grid_points(97, 61, 130, 3)
    for nA, capA in ((0, 4), (1, 5), (63, 70), (64, 70), (65, 70), (130, 131), (500, 40)):
        out.append(dict(name="rows nA %d capA %d" % (nA, capA), A=A97, B=B97, xs=gx, ys=gy, nA=nA, capA=capA,
                        kw=dict(levels=3, radius=3, iterations=4)))
    Hs = {"shift": [1, 0, 2.5, 0, 1, 2.25, 0, 0, 1], "den <= 0": [1, 0, 0, 0, 1, 0, -0.03, 0, 1], "nan": [1, 0, 0, 0, np.nan, 0, 0, 0, 1],
          "far": [1, 0, 4000, 0, 1, 0, 0, 0, 1]}
    for name, H in Hs.items():
        for status in (None, 1, 0):
            out.append(dict(name="H %s status %r" % (name, status), A=A97, B=B97, xs=gx[:12], ys=gy[:12], nA=12, capA=12,
                            H=np.array(H, F32), status=status, kw=dict(levels=3, radius=3, iterations=4)))
    return out


def model_case(c):
    q = Params(c["A"].shape[1], c["A"].shape[0], **c["kw"])
    H = c.get("H") if usable(c.get("H"), c.get("status")) else None
    return track_pair(q, c["A"], c["B"], c["xs"], c["ys"], c["nA"], c["capA"], c.get("mask"), H)


def padded(c):
    """the case's coordinate arrays grown to capA rows (what lies beyond nA is never read: garbage)"""
    grow = lambda v: np.r_[np.asarray(v, F32), np.full(max(0, c["capA"] - len(v)), 7.0, F32)]
    return grow(c["xs"]), grow(c["ys"])


# ---- the accuracy cases: views of the loop-closure scene, 256 x 192 ----
AW, AH, ASTEP = 256, 192, 16
ACC = dict(levels=4, radius=7, iterations=10, eps=2.0 ** -6, max_step=16.0, fb_max=1.0, max_residual=6.0)


def _render(gray, M, w=AW, h=AH):
    """the view whose pixel p shows scene point M p, bilinear in float64, as float32"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    q = np.stack([x, y, np.ones_like(x)], -1) @ np.asarray(M, np.float64).T
    u, v = q[..., 0] / q[..., 2], q[..., 1] / q[..., 2]
    i, j = np.floor(u).astype(int), np.floor(v).astype(int)
    a, b = u - i, v - j
    g = gray.astype(np.float64)
    return ((1 - a) * (1 - b) * g[j, i] + a * (1 - b) * g[j, i + 1] + (1 - a) * b * g[j + 1, i] + a * b * g[j + 1, i + 1]).astype(F32)


def _homography(src, dst):
    """the map through four point pairs (direct linear solve)"""
    rows, rhs = [], []
    for (x, y), (u, v) in zip(src, dst):
        rows += [[x, y, 1, 0, 0, 0, -u * x, -u * y], [0, 0, 0, x, y, 1, -v * x, -v * y]]
        rhs += [u, v]
    return np.append(np.linalg.solve(np.array(rows, np.float64), np.array(rhs, np.float64)), 1.0).reshape(3, 3)


def accuracy_case(which, seed=90):
    """(grayA, grayB, true map A -> B as float64 3 x 3, H_in float32 (9,) or None). (a): a pure translation of
    (9.4, -6.7) px, no start map. (b): two views with a roll and a perspective term as loop_closure_ref.view_maps builds
    them, 30 x 18 px apart, and the true map with its corners moved by 8 px as the start."""
    import loop_closure_ref as LC
    gray = LC.scene(seed)[..., 1]
    shift = lambda tx, ty: np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float64)
    if which == "a":
        Ma, Mb = shift(600, 200), shift(600 + 9.4, 200 - 6.7)
    else:
        def view(cx, cy, th, px, py):
            R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
            P = np.array([[1, 0, 0], [0, 1, 0], [px, py, 1]], np.float64)
            return shift(cx, cy) @ R @ P @ shift(-AW / 2, -AH / 2)
        Ma, Mb = view(700, 300, 0.0, 0.0, 0.0), view(730, 318, 0.03, 2e-5, -1.5e-5)
    true = np.linalg.inv(Mb) @ Ma
    true /= true[2, 2]
    H = None
    if which == "b":
        corners = np.array([[0, 0], [AW, 0], [AW, AH], [0, AH]], np.float64)
        q = np.c_[corners, np.ones(4)] @ true.T
        moved = q[:, :2] / q[:, 2:] + np.array([[8, -6], [-7, 8], [6, 7], [-8, -5]], np.float64)
        H = _homography(corners, moved).astype(F32).reshape(-1)
    return _render(gray, Ma), _render(gray, Mb), true, H


def accuracy_figures(dst, true, xs, ys, refit):
    """share tracked, median and 95th percentile distance from the truth, corner error of refit(dst) -> 3 x 3 map"""
    p = np.c_[xs, ys].astype(np.float64)
    q = np.c_[p, np.ones(len(p))] @ true.T
    want = q[:, :2] / q[:, 2:]
    ok = np.isfinite(dst[:, 0]) & (dst[:, 0] >= 0)
    d = np.hypot(*(dst[ok] - want[ok]).T)
    Hfit = refit(dst, ok)
    c = np.array([[0, 0, 1], [AW, 0, 1], [AW, AH, 1], [0, AH, 1]], np.float64)
    a, b = c @ np.asarray(Hfit, np.float64).reshape(3, 3).T, c @ true.T
    corner = np.hypot(*(a[:, :2] / a[:, 2:] - b[:, :2] / b[:, 2:]).T).max()
    return dict(share=float(ok.mean()), median=float(np.median(d)), p95=float(np.percentile(d, 95)), corner=float(corner))


def inside_both(true, xs, ys, r):
    """grid points whose window of radius r + 2 lies inside both frames under the true map"""
    q = np.c_[xs, ys, np.ones(len(xs))].astype(np.float64) @ true.T
    u, v = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
    m = r + 2
    ok = lambda x, y: (x >= m) & (x <= AW - 1 - m) & (y >= m) & (y <= AH - 1 - m)
    return ok(np.asarray(xs, np.float64), np.asarray(ys, np.float64)) & ok(u, v)
