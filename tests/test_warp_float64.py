"""The warp family (undistortion map, texture resampling, perspective warp, blend, gray) against the float64 model of
tests/warp_ref.py, on the CPU: the oracle (oracle/nmo_warp.h) goes through the model, which validates the model and the
bounds before a GPU is involved. tests/test_gpu_warp_float64.py imports the cases, bounds and checks below and sends the
device kernels through them.

BOUNDS (u = 2^-24, the single-precision unit roundoff; none of these is fitted to an output)

Sampler. The product rounds the filter weights a, b to 1/256. With such weights its sample is the EXACT bilinear
interpolant evaluated at a point moved by at most 1/512 per axis (a weight of 256/256 lands on the next texel, where the
interpolant is continuous). The interpolant moves by at most Lx per texel in x and Ly in y (warp_ref.Texture), so

    |got - S(x, y)| <= Lx (1/512 + dx) + Ly (1/512 + dy) + eps                                     (1)

  dx, dy: the coordinate error reaching the sampler. A kernel that is handed its coordinates x in single precision (a
      caller's map, or its own x_pos / y_pos outputs) forms fl(x + 0.5) and then subtracts 0.5: two roundings of relative
      size u on a magnitude of at most |x| + 1, dx = 2 u (|x| + 1) (coord_delta). The blend never shows its
      coordinates; there dx is in addition the forward error of the projection (project_error, below).
  eps: 8-bit texels are c / 255 rounded (u), the four weights are exact products of two 9-bit numbers, each weight times
      texel rounds once (u), three sums round once each on partial sums no larger than the largest texel M: every term
      carries at most 5 roundings, eps = 6 u M covers (1 + u)^5 - 1.
  The result times 255.9999f rounds once more and the constant itself is rounded (relative 4.2e-8 < u):
      e' = e + 3 u (|S| + e); a float output lies within 255.9999 e' of 255.9999 S, an unsigned char output in
      [trunc((S - e') 255.9999), trunc((S + e') 255.9999)].

Projection x' = (m0 x + m1 y + m2) / (m6 x + m7 y + m8) (project_error). x, y are integers, exact. A three-term dot product
evaluated in single precision in any order, with or without fused multiply-adds, has |error| <= 3 u T (1 + 2^-10),
T = |m0 x| + |m1 y| + |m2| (each term passes through at most 3 roundings). With E_m the entry-wise error of the matrix in
use (0 for a caller's matrix), E_a = 3 u T_a + E_m0 |x| + E_m1 |y| + E_m2 and likewise E_s for the denominator s;
    |fl(a^/s^) - a/s| <= (E_a + |a/s| E_s) / (|s| - E_s) + u |a/s|,   taken times (1 + 2^-10) for the second-order terms.

Inverse (inverse_error): adjugate over determinant in single precision against numpy.linalg.inv of the same matrix in
float64. A cofactor ab - cd carries |error| <= 2 u (|ab| + |cd|) = E_c; the determinant sum_k t_k c_k carries
E_det = sum |t_k| E_ck + 3 u sum |t_k c_k|; 1 / det carries the relative error E_det / (|det| - E_det) + u; an entry
cofactor / det therefore (E_c + |c| (E_det / (|det| - E_det) + 2 u)) / |det|, times (1 + 2^-10).

Undistortion map (undistort_error): a = (x - cx) / fx is two roundings, |da| <= 2 u |a|; r2 = a^2 + b^2 has relative error
<= 6 u (4 u from the squares' inputs, one rounding per product, one for the sum; all terms positive), r2^2 <= 13 u,
r2^3 <= 20 u; the polynomial adds one rounding per term and per sum, E_p = 6 u |k1| r2 + 13 u |k2| r2^2 + 20 u |k3| r2^3
+ 3 u (1 + |k1| r2 + |k2| r2^2 + |k3| r2^3); the output a p fx + cx: fx (|a| E_p + 4 u |a p|) + u |result|, times
(1 + 2^-10).

Blend (run_blend): r, the mask sample and the weight sample obey (1) with dx = coord_delta + project_error. The
recurrence is carried as intervals (warp_ref.blend_step); the single-precision evaluation of the mean (two products, one
fused multiply-add, one sum, one division: 5 roundings per term) and of cwt + nwt (1) is allowed a relative 6 u.

Exclusions. A pixel whose decision lies within its bound of a threshold (the sampler's support edge, the blend's
x_p >= fw / y_p >= fh cutoff, mask <= 0.5, canvas_wts == 0, resample_mask's lower limit) is not value-checked but
counted; the excluded share of every case is asserted <= 2 %.

MEASURED median interval widths in grey levels, oracle on the CPU (a report of how tight the derived bounds are, not what
is asserted): see MEDIAN_WIDTHS at the end of this docstring; the smooth-field cases must stay <= 2 levels, which the
test asserts.

MEDIAN_WIDTHS (hi - lo of the unsigned char interval; float outputs: 2 * 255.9999 e'):
    perspective 1920x1080 noise similarity inv coords     0.003   (excluded 0.0000 %)
    perspective 1920x1080 noise similarity inv            2.000   (excluded 0.0000 %)
    perspective 1920x1080 step perspective fwd coords     0.001   (excluded 0.0000 %)
    perspective 1920x1080 step perspective fwd            0.000   (excluded 0.0001 %)
    perspective 3840x2160 smooth scale0.5 inv coords      0.002   (excluded 0.0000 %)
    perspective 3840x2160 smooth scale0.5 inv             0.000   (excluded 0.0001 %)
    perspective 3840x2160 noise scale2 fwd coords         0.002   (excluded 0.0000 %)
    perspective 3840x2160 noise scale2 fwd                2.000   (excluded 0.0000 %)
    perspective 7680x4320 smooth perspective inv coords   0.016   (excluded 0.0000 %)
    perspective 7680x4320 smooth perspective inv          0.000   (excluded 0.0000 %)
    perspective 7680x4320 noise similarity fwd coords     0.004   (excluded 0.0000 %)
    perspective 7680x4320 noise similarity fwd            2.000   (excluded 0.0001 %)
    perspective 2047x1531 step scale0.5 fwd coords        0.001   (excluded 0.0000 %)
    perspective 2047x1531 step scale0.5 fwd               0.000   (excluded 0.0001 %)
    perspective 2047x1531 smooth scale2 inv coords        0.011   (excluded 0.0000 %)
    perspective 2047x1531 smooth scale2 inv               0.000   (excluded 0.0001 %)
    radial 1920x1080 map                                  0.001   (excluded 0.0000 %)
    radial 1920x1080 u8x4 map                             2.000   (excluded 0.0000 %)
    radial 1920x1080 f32                                  0.008   (excluded 0.0000 %)
    radial 1920x1080 mask                                 0.000   (excluded 0.3044 %)
    radial 1920x1080 mask disc                            0.000   (excluded 0.0011 %)
    radial 2047x1531 map                                  0.001   (excluded 0.0000 %)
    radial 2047x1531 u8x4 map                             2.000   (excluded 0.0001 %)
    radial 2047x1531 f32                                  0.008   (excluded 0.0001 %)
    radial 2047x1531 mask                                 0.000   (excluded 0.2340 %)
    radial 2047x1531 mask disc                            0.000   (excluded 0.0016 %)
    radial 3840x2160 map                                  0.001   (excluded 0.0000 %)
    radial 3840x2160 u8x4 map                             2.000   (excluded 0.0000 %)
    radial 3840x2160 f32                                  0.008   (excluded 0.0000 %)
    radial 3840x2160 mask                                 0.000   (excluded 0.2019 %)
    radial 3840x2160 mask disc                            0.000   (excluded 0.0007 %)
    radial 7680x4320 map                                  0.002   (excluded 0.0000 %)
    radial 7680x4320 u8x4 map                             0.000   (excluded 0.0001 %)
    radial 7680x4320 f32                                  1.712   (excluded 0.0001 %)
    blend one_4k_f32                                      2.000   (excluded 0.0011 %)
    blend three_odd_u8                                    1.000   (excluded 0.0024 %)
    blend seventeen_1080p_f32                             0.000   (excluded 0.0126 %)
    ("coords" / "map" rows: pixels, not grey levels; the smooth-field rows are all <= 2)
"""
import numpy as np
import pytest

import warp_ref as R

U = 2.0 ** -24
SECOND = 1.0 + 2.0 ** -10
CHUNK = 1 << 21
MAX_EXCLUDED = 0.02


# ---- bounds ----------------------------------------------------------------------------------------------------------
def coord_delta(x):
    return 2.0 * U * (np.abs(x) + 1.0)


def sample_error(Lx, Ly, x, y, M, dx=0.0, dy=0.0):
    return Lx * (1.0 / 512 + coord_delta(x) + dx) + Ly * (1.0 / 512 + coord_delta(y) + dy) + 6.0 * U * M


def scaled_error(S, e):
    return e + 3.0 * U * (np.abs(S) + e)


def project_error(m, x, y, Em=None):
    m = np.asarray(m, np.float64).reshape(9)
    Em = np.zeros(9) if Em is None else np.asarray(Em, np.float64).reshape(9)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    ax, ay = np.abs(x), np.abs(y)

    def dot_err(k):
        return 3.0 * U * (np.abs(m[k]) * ax + np.abs(m[k + 1]) * ay + np.abs(m[k + 2])) * SECOND + \
            Em[k] * ax + Em[k + 1] * ay + Em[k + 2]
    Ea, Eb, Es = dot_err(0), dot_err(3), dot_err(6)
    s = m[6] * x + m[7] * y + m[8]
    xp, yp = R.project(m, x, y)
    den = np.maximum(np.abs(s) - Es, 1e-300)
    return ((Ea + np.abs(xp) * Es) / den + U * np.abs(xp)) * SECOND, ((Eb + np.abs(yp) * Es) / den + U * np.abs(yp)) * SECOND


_COF = [(4, 8, 7, 5), (2, 7, 1, 8), (1, 5, 2, 4), (5, 6, 3, 8), (0, 8, 2, 6), (3, 2, 0, 5), (3, 7, 6, 4), (6, 1, 0, 7),
        (0, 4, 3, 1)]             # entry k of the adjugate = t[a] t[b] - t[c] t[d]


def inverse_error(mat):
    t = R.matrix64(mat).reshape(9)
    cof = np.array([t[a] * t[b] - t[c] * t[d] for a, b, c, d in _COF])
    Ec = np.array([2.0 * U * (abs(t[a] * t[b]) + abs(t[c] * t[d])) for a, b, c, d in _COF])
    # det by the first row: t0 C0 - t1 C1' + t2 C2' with the cofactors (4,8,7,5), (3,8,5,6), (3,7,4,6)
    row = [(4, 8, 7, 5), (3, 8, 5, 6), (3, 7, 4, 6)]
    c3 = np.array([t[a] * t[b] - t[c] * t[d] for a, b, c, d in row])
    e3 = np.array([2.0 * U * (abs(t[a] * t[b]) + abs(t[c] * t[d])) for a, b, c, d in row])
    det = t[0] * c3[0] - t[1] * c3[1] + t[2] * c3[2]
    Edet = (np.abs(t[:3]) * e3).sum() + 3.0 * U * (np.abs(t[:3] * c3)).sum()
    assert abs(det) > 4 * Edet, "matrix too close to singular for a bound"
    rel = Edet / (abs(det) - Edet) + 2.0 * U
    return (Ec + np.abs(cof) * rel) / abs(det) * SECOND


def undistort_error(x, y, cam, dist):
    fx, fy, cx, cy = [float(np.float32(c)) for c in cam]
    k1, k2, k3 = [abs(float(np.float32(k))) for k in dist]
    a = (np.asarray(x, np.float64) - cx) / fx
    b = (np.asarray(y, np.float64) - cy) / fy
    r2 = a * a + b * b
    t1, t2, t3 = k1 * r2, k2 * r2 ** 2, k3 * r2 ** 3
    Ep = U * (6 * t1 + 13 * t2 + 20 * t3 + 3 * (1 + t1 + t2 + t3))
    u, v = R.undistort(x, y, cam, dist)
    p = np.abs((u - cx) / fx) / np.maximum(np.abs(a), 1e-300)
    p = np.where(a == 0, np.abs((v - cy) / fy) / np.maximum(np.abs(b), 1e-300), p)
    eu = (fx * (np.abs(a) * Ep + 4 * U * np.abs(a) * p) + U * np.abs(u)) * SECOND
    ev = (fy * (np.abs(b) * Ep + 4 * U * np.abs(b) * p) + U * np.abs(v)) * SECOND
    return eu, ev


# ---- inputs ----------------------------------------------------------------------------------------------------------
def content(kind, w, h, seed):
    """A BGRA uint8 frame: 'noise', 'smooth' (low-frequency sinusoids, about one grey level per texel at most) or 'step'
    (constant 64 x 64 blocks)."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if kind == "step":
        blocks = rng.integers(0, 256, (h // 64 + 1, w // 64 + 1, 4), dtype=np.uint8)
        return np.ascontiguousarray(np.repeat(np.repeat(blocks, 64, axis=0), 64, axis=1)[:h, :w])
    assert kind == "smooth"
    x = np.arange(w)[None, :, None] / 640.0
    y = np.arange(h)[:, None, None] / 640.0
    ph = rng.uniform(0, 6.28, (1, 1, 4))
    fx_, fy_ = rng.uniform(1.5, 3.0, (1, 1, 4)), rng.uniform(1.5, 3.0, (1, 1, 4))
    return (127.5 + 100.0 * np.sin(fx_ * x + ph) * np.cos(fy_ * y - ph)).astype(np.uint8)


def plane(kind, w, h, seed, dtype):
    """Scalar planes for masks, weights and textures. 'disc': 1 inside a disc, 0 outside; 'half': a half-plane; 'feather':
    positive weights falling toward the frame edge; 'smooth': one smooth channel in [0, 1]; 'step'/'noise' likewise."""
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "disc":
        v = (((xx - 0.48 * w) / (0.47 * w)) ** 2 + ((yy - 0.52 * h) / (0.46 * h)) ** 2 < 1.0).astype(np.float64)
    elif kind == "half":
        v = (xx * 0.8 + yy * 0.6 > 0.12 * (w + h)).astype(np.float64)
    elif kind == "feather":
        v = np.minimum(np.minimum(xx, w - 1 - xx), np.minimum(yy, h - 1 - yy)) / (0.25 * min(w, h))
        v = np.minimum(v, 1.0) * 0.95 + 0.04
    else:
        v = content(kind, w, h, seed)[..., 1] / 255.0
    return np.round(v * 255).astype(np.uint8) if dtype == np.uint8 else v.astype(np.float32)


def grid_map(kind, fw, fh, cols, rows):
    """The map from the output grid into the frame, float32 3 x 3."""
    sx = fw / cols
    if kind == "similarity":
        a, s = 0.05, 1.12 * sx
        G = [[s * np.cos(a), -s * np.sin(a), -0.07 * fw], [s * np.sin(a), s * np.cos(a), -0.09 * fh], [0, 0, 1]]
    elif kind == "perspective":                       # the denominator runs from 1 to 1.25 / 0.85 across the grid
        G = [[1.2 * sx, 0.03, -0.06 * fw], [-0.02, 1.15 * sx, -0.05 * fh], [0.25 / cols, -0.15 / rows, 1]]
    elif kind == "scale0.5":
        G = [[0.5, 1e-3, 3.25], [-1e-3, 0.5, -2.5], [0, 0, 1]]
    else:
        assert kind == "scale2"
        G = [[2.0, 1e-3, -40.25], [-1e-3, 2.0, -30.5], [0, 0, 1]]
    return np.array(G, np.float32)


# (frame w, h, content, map kind, inverse, cols, rows). Every frame size, content, map kind and direction of the issue
# occurs, each map kind in both directions, output grids smaller and larger than the frame; the full cross product (192
# cases) would run for an hour in numpy, so the two large sizes carry the extremes of content (noise, smooth).
PERSPECTIVE_CASES = [
    (1920, 1080, "noise", "similarity", True, 1920, 1080),
    (1920, 1080, "step", "perspective", False, 1280, 720),
    (3840, 2160, "smooth", "scale0.5", True, 2400, 1350),
    (3840, 2160, "noise", "scale2", False, 1920, 1080),
    (7680, 4320, "smooth", "perspective", True, 7680, 4320),
    (7680, 4320, "noise", "similarity", False, 3840, 2160),
    (2047, 1531, "step", "scale0.5", False, 2500, 1800),
    (2047, 1531, "smooth", "scale2", True, 1100, 800),
]


def perspective_inputs(case):
    fw, fh, kind, mk, inverse, cols, rows = case
    frame = content(kind, fw, fh, 100 + fw % 97)
    G = grid_map(mk, fw, fh, cols, rows)
    mat = np.linalg.inv(G.astype(np.float64)).astype(np.float32) if inverse else G
    return frame, mat


# (w, h, (k1, k2, k3)): pincushion, strong enough that the map leaves the frame on all four sides
RADIAL_CASES = [(1920, 1080, (0.30, 0.08, -0.02)), (2047, 1531, (0.22, -0.05, 0.03)), (3840, 2160, (0.30, 0.08, -0.02)),
                (7680, 4320, (0.35, 0.10, -0.03))]


def radial_inputs(w, h, k):
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    cam = np.array([0.9 * w, 0.95 * w, w / 2 - 3.5, h / 2 + 1.25], np.float32)
    return np.ascontiguousarray(x), np.ascontiguousarray(y), cam, np.array(k, np.float32)


def blend_case(name):
    """name -> dict(canvas, cwts, frames=[(frame, mask, wts, mat, tx, ty, nw, nh)])."""
    rng = np.random.default_rng(7)
    if name == "one_4k_f32":
        fw, fh, cw, ch, n = 3840, 2160, 4200, 2400, 1
        kinds, mk, wk, dt = ["noise"], "disc", "feather", np.float32
        nw, nh = fw + 20, fh + 10
    elif name == "three_odd_u8":
        fw, fh, cw, ch, n = 2047, 1531, 2600, 1900, 3
        kinds, mk, wk, dt = ["smooth", "step", "noise"], "half", "feather", np.uint8
        nw, nh = fw + 20, fh + 10
    elif name == "seventeen_1080p_f32":
        fw, fh, cw, ch, n = 1920, 1080, 2200, 1300, 17
        kinds, mk, wk, dt = ["smooth"] * 15 + ["noise", "step"], "disc", "feather", np.float32
        nw, nh = 1300, 740
    elif name == "sixtyfour_small_u8":               # the batched entry's largest batch (GPU file)
        fw, fh, cw, ch, n = 640, 360, 1100, 700, 64
        kinds, mk, wk, dt = ["smooth", "noise"] * 32, "disc", "feather", np.uint8
        nw, nh = 660, 370
    else:
        raise KeyError(name)
    canvas = np.zeros((ch, cw, 4), np.uint8)
    cwts = np.zeros((ch, cw), np.float32)
    if name != "one_4k_f32":                         # a partly filled, patterned canvas
        yy, xx = np.mgrid[0:ch, 0:cw]
        filled = ((xx // 97 + yy // 61) % 3 == 0) & (xx < 0.6 * cw)
        pat = content("step", cw, ch, 5)
        pat[..., 3] = 255
        canvas[filled] = pat[filled]
        cwts[filled] = (0.25 + 0.5 * ((xx // 97) % 2))[filled]
    frames = []
    mask = plane(mk, fw, fh, 1, dt)
    wts = plane(wk, fw, fh, 2, dt)
    for k in range(n):
        a = rng.uniform(-0.04, 0.04)
        s = (fw / nw) * rng.uniform(1.0, 1.08)
        M = np.array([[s * np.cos(a), -s * np.sin(a), rng.uniform(-0.02, 0.01) * fw],
                      [s * np.sin(a), s * np.cos(a), rng.uniform(-0.02, 0.01) * fh],
                      [rng.uniform(-1e-5, 1e-5), rng.uniform(-1e-5, 1e-5), 1.0]], np.float32)
        tx = int(rng.integers(-40, max(cw - nw + 40, 1)))
        ty = int(rng.integers(-30, max(ch - nh + 30, 1)))
        frames.append((content(kinds[k], fw, fh, 300 + k), mask, wts, M, tx, ty, nw, nh))
    return dict(canvas=canvas, cwts=cwts, frames=frames)


# ---- checks ----------------------------------------------------------------------------------------------------------
class Stats:
    def __init__(self, name):
        self.name, self.n, self.excluded, self.bad, self.widths, self.first_bad = name, 0, 0, 0, [], None

    def add(self, ok, checked, width=None, excluded=0):
        self.n += int(checked.sum()) + int(excluded)
        self.excluded += int(excluded)
        bad = checked & ~ok
        if bad.any() and self.first_bad is None:
            self.first_bad = int(np.flatnonzero(bad)[0])
        self.bad += int(bad.sum())
        if width is not None and checked.any():
            self.widths.append(np.asarray(width)[checked][::17].astype(np.float32))

    @property
    def share(self):
        return self.excluded / max(self.n, 1)

    @property
    def median_width(self):
        return float(np.median(np.concatenate(self.widths))) if self.widths else 0.0

    def require(self):
        assert self.bad == 0, "%s: %d of %d outside the interval (first chunk-local index %s), excluded %.4f %%" % (
            self.name, self.bad, self.n, self.first_bad, 100 * self.share)
        assert self.share <= MAX_EXCLUDED, "%s: excluded share %.4f %% > 2 %%" % (self.name, 100 * self.share)
        return self


def _near_support(tex, x, y, dx, dy):
    with np.errstate(invalid="ignore"):
        near = (np.abs(x + 1.0) <= dx) | (np.abs(x - tex.w) <= dx) | (np.abs(y + 1.0) <= dy) | (np.abs(y - tex.h) <= dy)
    return near


def model_sample(tex, x, y, dx=0.0, dy=0.0):
    """S, e (per pixel, shared by the channels) and `excluded` (support decision within the bound)."""
    x, y = np.asarray(x, np.float64).reshape(-1), np.asarray(y, np.float64).reshape(-1)
    S, Lx, Ly, inside = R.sample(tex, x, y)
    ddx, ddy = coord_delta(x) + dx, coord_delta(y) + dy
    e = sample_error(Lx, Ly, x, y, tex.max_abs, dx, dy)
    e = np.where(inside, e, 0.0)
    with np.errstate(invalid="ignore"):
        excluded = _near_support(tex, x, y, ddx, ddy) & np.isfinite(x) & np.isfinite(y)
    return S, e, excluded


def check_u8_samples(name, got, tex, x, y, stats=None):
    """got: unsigned char (N, channels) = trunc(sample * 255.9999) at the single-precision coordinates x, y."""
    st = stats or Stats(name)
    got = np.asarray(got).reshape(-1, tex.nch)
    x, y = np.asarray(x).reshape(-1), np.asarray(y).reshape(-1)
    for o in range(0, x.size, CHUNK):
        sl = slice(o, o + CHUNK)
        S, e, exc = model_sample(tex, x[sl], y[sl])
        lo, hi = R.u8_interval(S, scaled_error(S, e[:, None]))
        g = got[sl].astype(np.float64)
        ok = ((g >= lo) & (g <= hi)).all(axis=1)
        st.add(ok, ~exc, (hi - lo).max(axis=1), exc.sum())
    return st


def check_f32_samples(name, got, tex, x, y, stats=None):
    """got: float = sample * 255.9999f (resample_undistort)."""
    st = stats or Stats(name)
    got = np.asarray(got, np.float64).reshape(-1)
    x, y = np.asarray(x).reshape(-1), np.asarray(y).reshape(-1)
    for o in range(0, x.size, CHUNK):
        sl = slice(o, o + CHUNK)
        S, e, exc = model_sample(tex, x[sl], y[sl])
        S = S[:, 0]
        ee = scaled_error(S, e) * R.K_U8
        ok = np.abs(got[sl] - S * R.K_U8) <= ee
        st.add(ok, ~exc, 2 * ee, exc.sum())
    return st


def check_mask_samples(name, got, tex, x, y, limit, stats=None):
    """got: unsigned char = 0 where sample <= limit else trunc(sample * 255.999f) (resample_mask)."""
    st = stats or Stats(name)
    got = np.asarray(got).reshape(-1).astype(np.float64)
    x, y = np.asarray(x).reshape(-1), np.asarray(y).reshape(-1)
    lim = float(np.float32(limit))
    for o in range(0, x.size, CHUNK):
        sl = slice(o, o + CHUNK)
        S, e, exc = model_sample(tex, x[sl], y[sl])
        S = S[:, 0]
        exc = exc | (np.abs(S - lim) <= e)
        lo, hi = R.u8_interval(S, scaled_error(S, e), R.K_MASK)
        below = S <= lim
        ok = np.where(below, got[sl] == 0, (got[sl] >= lo) & (got[sl] <= hi))
        st.add(ok, ~exc, np.where(below, 0.0, hi - lo), exc.sum())
    return st


def check_coords(name, gx, gy, mx, my, ex, ey):
    st = Stats(name)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(np.asarray(gx, np.float64) - mx) <= ex) & (np.abs(np.asarray(gy, np.float64) - my) <= ey)
    st.add(ok.reshape(-1), np.ones(ok.size, bool), (2 * np.maximum(ex, ey)).reshape(-1))
    return st


def perspective_coords(mat, inverse, cols, rows):
    """Model coordinates and their bound for resample_perspective's x_pos / y_pos."""
    x, y = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    m = R.true_inverse(mat) if inverse else R.matrix64(mat)
    Em = inverse_error(mat) if inverse else None
    mx, my = R.project(m, x, y)
    ex, ey = project_error(m, x, y, Em)
    return mx, my, ex, ey


def run_blend(case, point=False, ignore_weights=False, reverse=False, strict_mask=False, strict_cutoff=False, on_frame=None):
    """The blend of `case` through the model. Returns the final warp_ref.BlendState and `covered`, the canvas pixels inside
    some frame's grid. point=True collapses every bound to 0 (a point model, the base of the mutants); the other flags are
    the mutants: every weight taken as 1, frames in reverse order, mask < 0.5 for <= 0.5, x_p > fw for >= fw."""
    st = R.BlendState(case["canvas"], case["cwts"])
    ch, cw = case["cwts"].shape
    covered = np.zeros((ch, cw), bool)
    frames = case["frames"][::-1] if reverse else case["frames"]
    texs = {}
    for k, (frame, mask, wts, mat, tx, ty, nw, nh) in enumerate(frames):
        for a in (frame, mask, wts):
            if id(a) not in texs:
                texs[id(a)] = R.Texture(a)
        tf, tm, tw = texs[id(frame)], texs[id(mask)], texs[id(wts)]
        x0, x1, y0, y1 = max(0, -tx), min(nw, cw - tx), max(0, -ty), min(nh, ch - ty)
        if x0 >= x1 or y0 >= y1:
            continue
        covered[y0 + ty:y1 + ty, x0 + tx:x1 + tx] = True
        rows_per = max(1, CHUNK // (x1 - x0))
        m = R.matrix64(mat)
        for r0 in range(y0, y1, rows_per):
            gx, gy = np.meshgrid(np.arange(x0, x1, dtype=np.float64), np.arange(r0, min(r0 + rows_per, y1), dtype=np.float64))
            gx, gy = gx.reshape(-1), gy.reshape(-1)
            xp, yp = R.project(m, gx, gy)
            dx, dy = (0.0, 0.0) if point else project_error(m, gx, gy)
            z = 0.0 if point else 1.0
            cut = ((xp > tf.w) | (yp > tf.h)) if strict_cutoff else ((xp >= tf.w) | (yp >= tf.h))
            und = ((np.abs(xp - tf.w) <= dx) | (np.abs(yp - tf.h) <= dy)) & (not point)
            Sm, em, xm = model_sample(tm, xp, yp, dx, dy)
            Sm, em = Sm[:, 0], em * z
            inmask = (Sm >= 0.5) if strict_mask else (Sm > 0.5)
            und = und | ((np.abs(Sm - 0.5) <= em) & (not point)) | (xm & ~cut & (not point))
            Sw, ew, xw = model_sample(tw, xp, yp, dx, dy)
            Sw, ew = Sw[:, 0], ew * z
            Sr, er, xr = model_sample(tf, xp, yp, dx, dy)
            er = (er * z)[:, None]
            if ignore_weights:
                Sw, ew = np.ones_like(Sw), 0.0 * ew
            contributes = ~cut & inmask
            und = und | ((xw | xr) & contributes & (not point))
            idx = (gy.astype(np.int64) + ty, gx.astype(np.int64) + tx)
            R.blend_step(st, idx, contributes, und, Sr[:, :3] - er, Sr[:, :3] + er, Sw - ew, Sw + ew,
                         0.0 if point else 6.0 * U)
        if on_frame is not None:
            on_frame(k, st, covered)
    return st, covered


def check_blend(name, canvas, cwts, st, covered, initial):
    """The product's canvas / weights against the model state."""
    s = Stats(name)
    c = np.asarray(canvas)[..., :3].astype(np.float64)
    w = np.asarray(cwts, np.float64)
    ok = ((c >= st.c_lo) & (c <= st.c_hi)).all(axis=2) & (w >= st.w_lo) & (w <= st.w_hi) & \
        (np.asarray(canvas)[..., 3] == st.alpha)
    s.add(ok[covered], st.known[covered], (st.c_hi - st.c_lo).max(axis=2)[covered], 0)
    s.excluded = int((~st.known[covered]).sum())
    s.n = int(covered.sum())
    same = (np.asarray(canvas) == initial[0]).all(axis=2) & (np.asarray(cwts) == initial[1])
    assert same[~covered].all(), name + ": a pixel outside every frame's grid changed"
    return s


# ---- the CPU run: the oracle through the model -----------------------------------------------------------------------------
WIDTHS = {}


def _record(st):
    WIDTHS[st.name] = st.median_width
    print("%-58s n=%-10d excluded=%.4f%% median width=%.3f" % (st.name, st.n, 100 * st.share, st.median_width))
    return st


def oracle_u8x4(oracle, frame, u, v):
    return np.stack([oracle.resample_undistort(np.ascontiguousarray(frame[..., c]), u, v).astype(np.uint8)
                     for c in range(4)], axis=-1)


@pytest.mark.parametrize("case", PERSPECTIVE_CASES, ids=lambda c: "%dx%d-%s-%s-%s-%dx%d" % (
    c[0], c[1], c[2], c[3], "inv" if c[4] else "fwd", c[5], c[6]))
def test_oracle_perspective_against_model(oracle, case):
    fw, fh, kind, mk, inverse, cols, rows = case
    frame, mat = perspective_inputs(case)
    out, xp, yp = oracle.resample_perspective(frame, cols, rows, mat, inverse)
    name = "perspective %dx%d %s %s %s" % (fw, fh, kind, mk, "inv" if inverse else "fwd")
    _record(check_coords(name + " coords", xp, yp, *perspective_coords(mat, inverse, cols, rows))).require()
    st = _record(check_u8_samples(name, out, R.Texture(frame), xp, yp)).require()
    assert (out != 0).mean() > 0.3, "the case must sample the frame"
    if kind == "smooth":
        assert st.median_width <= 2.0, "bound too loose to be a test: %.2f levels" % st.median_width


@pytest.mark.parametrize("case", RADIAL_CASES, ids=lambda c: "%dx%d" % (c[0], c[1]))
def test_oracle_radial_maps_against_model(oracle, case):
    w, h, k = case
    x, y, cam, dist = radial_inputs(w, h, k)
    u, v = oracle.undistort_map(x, y, cam, dist)
    mu, mv = R.undistort(x, y, cam, dist)
    eu, ev = undistort_error(x, y, cam, dist)
    name = "radial %dx%d" % (w, h)
    _record(check_coords(name + " map", u, v, mu, mv, eu, ev)).require()
    assert u.min() < -1 and v.min() < -1 and u.max() > w and v.max() > h, "the map must leave the frame on all four sides"
    big = w >= 7680
    frame = content("smooth" if big else "noise", w, h, 41)
    st = _record(check_u8_samples(name + " u8x4 map", oracle_u8x4(oracle, frame, u, v), R.Texture(frame), u, v)).require()
    if big:
        assert st.median_width <= 2.0
    tf = plane("noise" if big else "smooth", w, h, 42, np.float32)
    st = _record(check_f32_samples(name + " f32", oracle.resample_undistort(tf, u, v), R.Texture(tf), u, v)).require()
    if not big:
        assert st.median_width <= 2.0
        tu = plane("step", w, h, 43, np.uint8)
        _record(check_mask_samples(name + " mask", oracle.resample_mask(tu, u, v, 0.4), R.Texture(tu), u, v, 0.4)).require()
        td = plane("disc", w, h, 44, np.float32)
        _record(check_mask_samples(name + " mask disc", oracle.resample_mask(td, u, v, 0.5), R.Texture(td), u, v, 0.5)).require()


@pytest.mark.parametrize("name", ["one_4k_f32", "three_odd_u8", "seventeen_1080p_f32"])
def test_oracle_blend_against_model(oracle, name):
    case = blend_case(name)
    canvas, cwts = case["canvas"], case["cwts"]
    steps = []
    for (frame, mask, wts, mat, tx, ty, nw, nh) in case["frames"]:
        canvas, cwts = oracle.transform_blend(canvas, cwts, frame, nw, nh, mat, tx, ty, mask, wts)
        steps.append((canvas, cwts))

    def on_frame(k, st, covered):
        check_blend("blend %s frame %d" % (name, k), steps[k][0], steps[k][1], st, covered,
                    (case["canvas"], case["cwts"])).require()
    st, covered = run_blend(case, on_frame=on_frame)
    s = _record(check_blend("blend " + name, canvas, cwts, st, covered, (case["canvas"], case["cwts"]))).require()
    assert (cwts > 0).mean() > 0.3
    if name == "seventeen_1080p_f32":
        assert s.median_width <= 2.0


def exact_subset_inputs():
    """F32 texture of 8-bit dyadic values, coordinates on and beside the 1/256 lattice, away from the border."""
    rng = np.random.default_rng(3)
    w, h = 2000, 1500
    tex = (rng.integers(0, 256, (h, w)) / 256.0).astype(np.float32)
    n = 1 << 18
    i = rng.integers(2, w - 3, n).astype(np.float64)
    j = rng.integers(2, h - 3, n).astype(np.float64)
    fr = np.array([0, 1, 128, 255], np.float64)
    fx_, fy_ = rng.choice(fr, n), rng.choice(fr, n)
    fx_[n // 2:], fy_[n // 2:] = rng.integers(0, 256, n - n // 2), rng.integers(0, 256, n - n // 2)
    x, y = i + fx_ / 256.0, j + fy_ / 256.0               # lattice points
    # half-way points (2k+1)/512, approached from both sides by 2^-12: the weight must round to the nearer lattice point
    k = rng.integers(0, 255, n).astype(np.float64)
    side = rng.choice([-1.0, 1.0], n)
    xh = i + (2 * k + 1) / 512.0 + side * 2.0 ** -12
    xh_lattice = i + (k + (side > 0)) / 256.0
    xs = np.concatenate([x, xh]).astype(np.float32)
    ys = np.concatenate([y, y]).astype(np.float32)
    assert (xs.astype(np.float64) == np.concatenate([x, xh])).all() and (ys.astype(np.float64) == np.concatenate([y, y])).all()
    return tex, xs.reshape(512, -1), ys.reshape(512, -1), np.concatenate([x, xh_lattice]), np.concatenate([y, y])


def exact_subset_expected(tex, lx, ly):
    S = R.sample(R.Texture(tex), lx, ly)[0][:, 0]
    return (S * float(np.float32(255.9999))).astype(np.float32)          # the exact product, rounded once


def test_oracle_exact_subset_is_bit_exact(oracle):
    tex, xs, ys, lx, ly = exact_subset_inputs()
    got = oracle.resample_undistort(tex, xs, ys)
    np.testing.assert_array_equal(got.reshape(-1).view(np.uint32), exact_subset_expected(tex, lx, ly).view(np.uint32))


def gray_triples():
    v = np.arange(1 << 24, dtype=np.uint32)
    bgra = np.empty((4096, 4096, 4), np.uint8)
    bgra[..., 0], bgra[..., 1], bgra[..., 2] = (v & 255).reshape(4096, 4096), ((v >> 8) & 255).reshape(4096, 4096), \
        (v >> 16).reshape(4096, 4096)
    bgra[..., 3] = (v * 2654435761 >> 24).astype(np.uint8).reshape(4096, 4096)      # alpha must not matter
    return bgra


def check_gray(got, bgra):
    """All triples against the correctly rounded n / 100. The product evaluates 0.07 B + 0.72 G + 0.21 R in double (three
    rounded constants, three roundings: relative error <= 6 * 2^-53) and narrows; where n / 100 lies within 8 * 2^-53
    (relative) of a single-precision tie, the narrowing may go either way: those triples are counted and allowed 1 ulp."""
    bits, tie_rel = R.gray_table()
    n = R.gray_index(bgra)
    want = bits[n]
    near = tie_rel[n] <= 8 * 2.0 ** -53
    g = np.asarray(got, np.float32).view(np.uint32).reshape(n.shape)
    diff = np.abs(g.astype(np.int64) - want.astype(np.int64))
    assert (diff[~near] == 0).all(), "gray: %d triples differ from the correctly rounded n/100" % int((diff[~near] != 0).sum())
    assert (diff[near] <= 1).all()
    return int(near.sum())


def test_oracle_gray_all_triples(oracle):
    bgra = gray_triples()
    near = check_gray(oracle.grayscale(bgra), bgra)
    print("gray: %d of 2^24 triples within the double-precision error of a tie" % near)


# ---- the checks bite ---------------------------------------------------------------------------------------------------
def test_checks_reject_mutants(oracle):
    """Mutants of the MODEL's output, fed to the checks as if they were the product's output. Each is rejected on the
    named case."""
    rejected = {}
    case = PERSPECTIVE_CASES[0]                        # 1920x1080 noise, similarity, inverse
    fw, fh, kind, mk, inverse, cols, rows = case
    frame, mat = perspective_inputs(case)
    tex = R.Texture(frame)
    mx, my, ex, ey = perspective_coords(mat, inverse, cols, rows)
    xs, ys = mx.astype(np.float32), my.astype(np.float32)
    x64, y64 = xs.astype(np.float64).reshape(-1), ys.astype(np.float64).reshape(-1)

    def as_u8(S):
        return np.minimum(np.floor(S * R.K_U8), 255).astype(np.uint8)
    base = as_u8(R.sample(tex, x64, y64)[0])
    assert check_u8_samples("unmutated model", base, tex, xs, ys).bad == 0
    cname = "perspective 1920x1080 noise similarity inv"
    rejected["half-texel shift"] = (cname, check_u8_samples("m", as_u8(R.sample(tex, x64 - 0.5, y64 - 0.5)[0]), tex, xs, ys).bad)
    fl = np.floor(x64)
    rejected["a and 1-a swapped"] = (cname, check_u8_samples("m", as_u8(R.sample(tex, fl + (1.0 - (x64 - fl)) % 1.0, y64)[0]),
                                                             tex, xs, ys).bad)
    rejected["nearest neighbour"] = (cname, check_u8_samples("m", as_u8(R.sample_nearest(tex, x64, y64)), tex, xs, ys).bad)
    rejected["B and R swapped"] = (cname, check_u8_samples("m", base[:, [2, 1, 0, 3]], tex, xs, ys).bad)
    x, y = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    tx_, ty_ = R.project(R.true_inverse(mat).T, x, y)
    rejected["matrix transposed"] = (cname + " coords", check_coords("m", tx_, ty_, mx, my, ex, ey).bad)
    fx_, fy_ = R.project(R.matrix64(mat), x, y)
    rejected["forward map used for inverse"] = (cname + " coords", check_coords("m", fx_, fy_, mx, my, ex, ey).bad)
    # gray with B and R swapped
    bgra = gray_triples()[::16, ::16]
    bits, _ = R.gray_table()
    with pytest.raises(AssertionError):
        check_gray(bits[R.gray_index(bgra[..., [2, 1, 0, 3]])].view(np.float32), bgra)
    # blend mutants on the three-frame case
    bc = blend_case("three_odd_u8")
    st, covered = run_blend(bc)
    initial = (bc["canvas"], bc["cwts"])

    def as_canvas(p):
        c = np.concatenate([p.c_lo, p.alpha[..., None]], axis=2).astype(np.uint8)
        return c, p.w_lo
    p, _ = run_blend(bc, point=True)
    assert check_blend("unmutated point model", *as_canvas(p), st, covered, initial).bad == 0
    for label, kw in (("blend ignoring the weights", dict(ignore_weights=True)), ("frames blended in reverse order", dict(reverse=True))):
        p, _ = run_blend(bc, point=True, **kw)
        c, w = as_canvas(p)
        if kw.get("ignore_weights"):                  # judge the colours alone: the mutant's weights are not the point
            w = np.clip(w, st.w_lo, st.w_hi)
        rejected[label] = ("blend three_odd_u8", check_blend("m", c, w, st, covered, initial).bad)
    # cutoffs at an exact edge: identity map, mask exactly 0.5 on half the frame
    fw2, fh2 = 64, 48
    f2 = content("noise", fw2, fh2, 9)
    m2 = np.ones((fh2, fw2), np.float32)
    m2[:, 20:40] = 0.5
    ec = dict(canvas=np.zeros((60, 80, 4), np.uint8), cwts=np.zeros((60, 80), np.float32),
              frames=[(f2, m2, np.full((fh2, fw2), 0.5, np.float32), np.eye(3, dtype=np.float32), 3, 2, fw2 + 8, fh2 + 8)])
    oc, ow = oracle.transform_blend(ec["canvas"], ec["cwts"], *[ec["frames"][0][k] for k in (0, 6, 7, 3, 4, 5, 1, 2)])
    est, ecov = run_blend(ec, point=True)              # exact inputs: the point model decides every pixel
    assert check_blend("exact edge", oc, ow, est, ecov, (ec["canvas"], ec["cwts"])).bad == 0
    assert (ow[2:50, 23:43] == 0).all(), "mask == 0.5 contributes nothing"
    p, _ = run_blend(ec, point=True, strict_mask=True)
    rejected["cutoff: mask < 0.5 for <= 0.5 at mask == 0.5"] = ("exact edge", check_blend("m", *as_canvas(p), est, ecov,
                                                                                       (ec["canvas"], ec["cwts"])).bad)
    # x_p > fw for x_p >= fw: the grid is 8 wider than the frame, so x_p == fw IS reached; the mutant then samples at
    # X - 0.5 = fw, outside the filter's support, reads mask 0 and drops the pixel all the same. The cutoff duplicates
    # the border rule: this mutant has no observable effect through any entry, which is asserted, not assumed.
    p, _ = run_blend(ec, point=True, strict_cutoff=True)
    c, w = as_canvas(p)
    assert check_blend("m", c, w, est, ecov, (ec["canvas"], ec["cwts"])).bad == 0
    for label, (where, bad) in rejected.items():
        print("mutant %-48s rejected on %-50s (%d pixels)" % (label, where, bad))
        assert bad > 0, "mutant not rejected: " + label
