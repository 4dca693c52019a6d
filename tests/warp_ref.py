"""Float64 model of the texture-sampled warps, the blend and the frame ingest. TEST INFRASTRUCTURE ONLY.

Written from the reference's definition of each operation (kernels/resample.cu, kernels/undistort.cu,
utils/cudatex2D.cu, kernels/bgra_2_gray.cu, kernels/cast.cu) and CUDA's documented linear filter

    tex(X, Y) = (1-a)(1-b) T[i,j] + a(1-b) T[i+1,j] + (1-a) b T[i,j+1] + a b T[i+1,j+1],
    i = floor(X - 0.5), a = frac(X - 0.5), likewise j, b; a texel outside the texture reads 0 (border addressing),

NOT from the product's sampler nor from the CPU oracle: this file imports neither. Everything is numpy float64 (or exact
integers / fractions): no fixed-point weights, no single-precision step, no prescribed summation order. What the product
and the oracle may differ from this model by is bounded in tests/test_warp_float64.py, not here.

Conventions shared with the reference: every kernel samples at (coordinate + 0.5); a BGRA texture has channels B, G, R, A
in that order; 8-bit texels are read as c / 255.
"""
from fractions import Fraction

import numpy as np

K_U8 = 255.9999            # resample_2D / transform_and_blend: unsigned char(value * 255.9999f)
K_MASK = 255.999           # resample_mask_2D
_PAD = 2                   # zero border kept around a texture: cells i-1 .. i+1 of a supported point index texels -2 .. w+1


class Texture:
    """A w x h texture with border addressing. data: 2-D float (F32), 2-D uint8 (U8N) or (h, w, 4) uint8 (U8X4N).
    lx / ly: for the cell (i, j) (texels i..i+1, j..j+1) the largest |difference| of horizontally / vertically adjacent
    texels within the 3 x 3 block of CELLS around it, that is texels i-1..i+2, j-1..j+2, border texels counted as 0, the
    largest over the channels; in texel units (c / 255 for 8-bit). A point that moves by less than one texel stays
    inside that block, and the bilinear interpolant's slope inside a cell is at most the cell's largest difference, so
    |S(p) - S(q)| <= lx |px - qx| + ly |py - qy| for |p - q| < 1 per axis, p in cell (i, j)."""

    def __init__(self, data):
        a = np.asarray(data)
        self.u8 = a.dtype == np.uint8
        assert (self.u8 and a.ndim in (2, 3)) or (a.dtype.kind == "f" and a.ndim == 2), "unsupported texture"
        self.h, self.w = a.shape[:2]
        self.nch = 1 if a.ndim == 2 else a.shape[2]
        p = np.zeros((self.h + 2 * _PAD, self.w + 2 * _PAD, self.nch), np.uint8 if self.u8 else np.float64)
        p[_PAD:-_PAD, _PAD:-_PAD] = a.reshape(self.h, self.w, self.nch)
        self.pad = p
        s = p.astype(np.int16) if self.u8 else p
        dx = np.abs(s[:, 1:] - s[:, :-1]).max(axis=2)           # (H, W-1): texel I -> I+1
        dy = np.abs(s[1:, :] - s[:-1, :]).max(axis=2)           # (H-1, W)
        del s
        H, W = p.shape[:2]
        # cell (J, I) in padded indices; lx: diffs I-1..I+1 on rows J-1..J+2; ly: diffs J-1..J+1 on columns I-1..I+2
        self.lx = self._window_max(dx, H, W, cols=(-1, 0, 1), rows=(-1, 0, 1, 2))
        self.ly = self._window_max(dy, H, W, cols=(-1, 0, 1, 2), rows=(-1, 0, 1))
        self.max_abs = float(np.abs(p).max()) / (255.0 if self.u8 else 1.0)

    @staticmethod
    def _window_max(d, H, W, cols, rows):
        big = np.zeros((H + 4, W + 4), d.dtype)
        big[2:2 + d.shape[0], 2:2 + d.shape[1]] = d
        acc = None
        for c in cols:
            v = big[:, 2 + c:2 + c + W]
            acc = v.copy() if acc is None else np.maximum(acc, v)
        out = None
        for r in rows:
            v = acc[2 + r:2 + r + H]
            out = v.copy() if out is None else np.maximum(out, v)
        return out

    def texels(self, J, I):
        v = self.pad[J, I]
        return v / 255.0 if self.u8 else v


def sample(tex, x, y):
    """The exact bilinear sample at coordinates (x, y), i.e. at the point (x + 0.5, y + 0.5). Returns S (N, channels),
    Lx (N,), Ly (N,) and `inside` (N,), the support of the filter: a point with X - 0.5 < -1 or >= w (or not finite) can
    touch no texel and reads 0."""
    x = np.asarray(x, np.float64).reshape(-1)
    y = np.asarray(y, np.float64).reshape(-1)
    X, Y = x + 0.5, y + 0.5
    xb, yb = X - 0.5, Y - 0.5
    with np.errstate(invalid="ignore"):
        inside = (xb >= -1.0) & (xb < tex.w) & (yb >= -1.0) & (yb < tex.h)
    xb = np.where(inside, xb, 0.0)
    yb = np.where(inside, yb, 0.0)
    fi, fj = np.floor(xb), np.floor(yb)
    a, b = (xb - fi)[:, None], (yb - fj)[:, None]
    I, J = fi.astype(np.int64) + _PAD, fj.astype(np.int64) + _PAD
    S = np.zeros((x.size, tex.nch))
    S += (1.0 - a) * (1.0 - b) * tex.texels(J, I)
    S += a * (1.0 - b) * tex.texels(J, I + 1)
    S += (1.0 - a) * b * tex.texels(J + 1, I)
    S += a * b * tex.texels(J + 1, I + 1)
    S[~inside] = 0.0
    unit = 255.0 if tex.u8 else 1.0
    Lx = tex.lx[J, I] / unit
    Ly = tex.ly[J, I] / unit
    return S, Lx, Ly, inside


def sample_nearest(tex, x, y):
    """MUTANT support: nearest texel instead of the bilinear filter."""
    x = np.asarray(x, np.float64).reshape(-1)
    y = np.asarray(y, np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        inside = (x >= -1.0) & (x < tex.w) & (y >= -1.0) & (y < tex.h)
    I = np.floor(np.where(inside, x, 0.0) + 0.5).astype(np.int64) + _PAD
    J = np.floor(np.where(inside, y, 0.0) + 0.5).astype(np.int64) + _PAD
    S = np.array(tex.texels(J, I), np.float64)
    S[~inside] = 0.0
    return S


# ---- geometry ------------------------------------------------------------------------------------------------------
def matrix64(mat3x3):
    """The caller's single-precision matrix, taken as float64 (exact)."""
    return np.asarray(mat3x3, np.float32).astype(np.float64).reshape(3, 3)


def true_inverse(mat3x3):
    return np.linalg.inv(matrix64(mat3x3))


def project(m, x, y):
    """x' = (m0 x + m1 y + m2) / (m6 x + m7 y + m8), y' likewise (apply_perspective)."""
    m = np.asarray(m, np.float64).reshape(9)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    s = m[6] * x + m[7] * y + m[8]
    return (m[0] * x + m[1] * y + m[2]) / s, (m[3] * x + m[4] * y + m[5]) / s


def undistort(x, y, cam, dist):
    """The radial model in closed form: x' = (x - cx) / fx, r2 = x'^2 + y'^2, u = x' (1 + k1 r2 + k2 r2^2 + k3 r2^3) fx + cx."""
    fx, fy, cx, cy = [float(np.float32(c)) for c in cam]
    k1, k2, k3 = [float(np.float32(k)) for k in dist]
    xn = (np.asarray(x, np.float64) - cx) / fx
    yn = (np.asarray(y, np.float64) - cy) / fy
    r2 = xn * xn + yn * yn
    poly = 1.0 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    return xn * poly * fx + cx, yn * poly * fy + cy


# ---- gray ----------------------------------------------------------------------------------------------------------
def gray_table():
    """0.07 B + 0.72 G + 0.21 R is the rational n / 100, n = 7 B + 72 G + 21 R in 0 .. 25500. Returns, for every n, the
    correctly rounded single-precision value of n / 100 (as its bit pattern, uint32) and the distance from n / 100 to the
    nearest rounding tie (the midpoint of two adjacent single-precision numbers), relative to n / 100 (inf for n = 0),
    both from exact rational arithmetic."""
    bits = np.zeros(25501, np.uint32)
    tie_rel = np.full(25501, np.inf)
    for n in range(1, 25501):
        q = Fraction(n, 100)
        e = 0
        while Fraction(2) ** (e + 1) <= q:
            e += 1
        while Fraction(2) ** e > q:
            e -= 1
        ulp = Fraction(2) ** (e - 23)
        k = q / ulp                                   # in [2^23, 2^24)
        lo = k.numerator // k.denominator
        frac = k - lo
        if frac > Fraction(1, 2) or (frac == Fraction(1, 2) and lo % 2 == 1):
            lo += 1
        mant = Fraction(lo) * ulp                     # exact value of the rounded result
        m, ee = lo, e
        if m == 1 << 24:
            m, ee = 1 << 23, e + 1
        bits[n] = ((ee + 127) << 23) | (m - (1 << 23))
        assert abs(mant - q) <= ulp / 2
        tie_rel[n] = float(abs(frac - Fraction(1, 2)) * ulp / q)
    return bits, tie_rel


def gray_index(bgra):
    b = np.asarray(bgra)
    return 7 * b[..., 0].astype(np.int64) + 72 * b[..., 1].astype(np.int64) + 21 * b[..., 2].astype(np.int64)


# ---- unsigned char outputs -------------------------------------------------------------------------------------------
def u8_interval(S, e, k=K_U8):
    """The integer interval of trunc(v * k) for v in [S - e, S + e] (values stay in [0, 256): truncation = floor, and a
    negative lower end, which the non-negative product value cannot reach, is 0)."""
    lo = np.floor(np.maximum(S - e, 0.0) * k)
    hi = np.floor(np.maximum(S + e, 0.0) * k)
    return np.minimum(lo, 255.0), np.minimum(hi, 255.0)


# ---- the blend recurrence, as intervals ----------------------------------------------------------------------------
class BlendState:
    """Canvas colour (3 channels) and weight per pixel as intervals [lo, hi], plus `known`: False once a decision on the
    pixel could not be made within the bounds (its later values are not checked), and `touched`."""

    def __init__(self, canvas, canvas_wts):
        c = np.asarray(canvas)[..., :3].astype(np.float64)
        w = np.asarray(canvas_wts, np.float64)
        self.c_lo, self.c_hi = c.copy(), c.copy()
        self.w_lo, self.w_hi = w.copy(), w.copy()
        self.alpha = np.asarray(canvas)[..., 3].astype(np.int64)
        self.known = np.ones(w.shape, bool)


def blend_step(st, idx, contributes, undecided, r_lo, r_hi, n_lo, n_hi, slack):
    """One frame into the canvas pixels idx = (py, px) (1-D index arrays, each canvas pixel at most once).
    transform_and_blend: if canvas_wts == 0 the pixel takes trunc(r * 255.9999) and the frame's weight (first touch), else
    trunc((r * nwt * 255.9999 + cur * cwt) / (cwt + nwt)) and cwt + nwt; alpha 255. contributes: the frame passes the
    cutoff and the mask test; undecided: one of those tests lies within its bound. r_* (N, 3) and n_* (N,) bound the
    frame's colour and weight samples. slack: relative allowance for the single-precision evaluation of the mean and of
    the weight sum. The mean is monotone in r and cur, and monotone in each weight for fixed colours, so its range over the
    weight intervals is attained at their corners (weights positive)."""
    py, px = idx
    known = st.known[py, px] & ~undecided
    st.known[py, px] = known
    sel = contributes & known
    py, px = py[sel], px[sel]
    r_lo, r_hi, n_lo, n_hi = r_lo[sel], r_hi[sel], n_lo[sel], n_hi[sel]
    cw_lo, cw_hi = st.w_lo[py, px], st.w_hi[py, px]
    first = cw_hi == 0.0
    # a canvas weight interval that contains 0 without being 0, or a non-positive frame weight: decision unknown
    bad = ((cw_lo <= 0.0) & ~first) | (n_lo <= 0.0)
    st.known[py[bad], px[bad]] = False
    ok = ~bad
    py, px, first = py[ok], px[ok], first[ok]
    r_lo, r_hi, n_lo, n_hi, cw_lo, cw_hi = r_lo[ok], r_hi[ok], n_lo[ok], n_hi[ok], cw_lo[ok], cw_hi[ok]
    cur_lo, cur_hi = st.c_lo[py, px], st.c_hi[py, px]
    f_lo = np.minimum(np.floor(np.maximum(r_lo, 0.0) * K_U8), 255.0)
    f_hi = np.minimum(np.floor(np.maximum(r_hi, 0.0) * K_U8), 255.0)
    m_lo, m_hi = None, None
    with np.errstate(invalid="ignore", divide="ignore"):
        for nw in (n_lo, n_hi):
            for cw in (cw_lo, cw_hi):
                s = (cw + nw)[:, None]
                lo = (np.maximum(r_lo, 0.0) * nw[:, None] * K_U8 + cur_lo * cw[:, None]) / s
                hi = (r_hi * nw[:, None] * K_U8 + cur_hi * cw[:, None]) / s
                m_lo = lo if m_lo is None else np.minimum(m_lo, lo)
                m_hi = hi if m_hi is None else np.maximum(m_hi, hi)
    m_lo = np.minimum(np.floor(np.maximum(m_lo * (1.0 - slack), 0.0)), 255.0)
    m_hi = np.minimum(np.floor(m_hi * (1.0 + slack)), 255.0)
    f = first[:, None]
    st.c_lo[py, px] = np.where(f, f_lo, m_lo)
    st.c_hi[py, px] = np.where(f, f_hi, m_hi)
    st.w_lo[py, px] = np.where(first, n_lo, (cw_lo + n_lo) * (1.0 - slack))
    st.w_hi[py, px] = np.where(first, n_hi, (cw_hi + n_hi) * (1.0 + slack))
    st.alpha[py, px] = 255
