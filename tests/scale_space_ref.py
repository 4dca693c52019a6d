"""Binary64 model of the scale space, extrema and refinement stages, numpy only.

Written from the semantics of the reference -- sift/siftparams.h:30-51, sift/pyramidata.cu:105-123, kernels/convolution.cu,
kernels/downsample.cu, kernels/cudamath.cu:26-54, kernels/cudamath.h:82-87, kernels/keypoint.cu:19-251, utils/cudatex2D.cu:15-19 --
and from nothing else: no oracle, no ctypes, no product header. Inputs are the float32 arrays (and float32 scalars) a stage
receives; every operation on them is binary64. Beside each value a function returns a rounding bound for a binary32 evaluation
of the same expressions under the fp spec of DESIGN.md section 2, and the margin of every discrete decision. `mutant=` switches
in one wrong line at a time (MUTANTS; tests/test_scale_space_float64.py shows that each is caught); None is the model.

Notation: u = 2^-24, gamma(k) = k u / (1 - k u), fl() one binary32 rounding, RN32 the correctly rounded value, TINY = 2^-149 (one
subnormal ulp: the absolute floor of a rounding whose result may be subnormal). First-order terms carry SLACK = 1.01.

PARAMETERS (sift_params64)
  Real-number values: octaves = max(1, floor(log2(2 min(w, h) / 32))), k = 2^(1/3), sigma_0 = 1.6 k,
  sigma_d_0 = sigma_0 sqrt(1 - 1 / k^2), base_smooth = sqrt((sigma_0 / k)^2 - 0.5^2), sigmas[i] = sigma_d_0 k^i, i = 0..4 (the
  INCREMENTAL blur from level i to i + 1: sqrt(s_{i+1}^2 - s_i^2) with s_i = sigma_0 k^(i-1)). Relative bounds from the operation
  count of siftparams.h:39-50: k is one float pow (2u); sigma_0 = fl(1.6f k): u (1.6f) + 2u + u = 4u; sigma_d_0: fl(k k) 5u, the
  difference 1 - 1 / kk = 0.37 amplifies it by 0.63 / 0.37 to 8.5u, the root halves it, times sigma_0 (4u) and one rounding: 10u;
  base_smooth: sa = fl(sigma_0 / k) 7u, fl(sa sa) 15u, the difference 2.56 - 0.25 amplifies by 1.11 (+u): 17.6u, the root halves
  (+u): 10u; sigmas[i]: 10u + 2u i + u. PARAM_REL holds them.
TAPS (taps64): r = ceil(4 sigma) (4 sigma is exact in binary32: no margin); v_j = exp(-q_j / 2), q_j = fl(fl((j - r) / sigma)^2):
  q carries 3u relative, so v_j carries q_j 1.5u + u (the cast); the float sum of n = 2r + 1 positive terms gamma(n - 1) S + sum e_v;
  t_j = fl(v_j / S): e_t = t_j (e_v / v_j + e_S / S + u) -- a few u of the tap at the centre, some 15 u at q = 16 where the tap is
  3e-4 of the centre. When sigma itself carries a relative error eps (the chain), d t_j / t_j = (q_j - <q>) eps is added.
CONVOLUTION (convolve64): zero padded, row pass into buf, column pass of buf (convolution.cu:16-159: out[x] = sum_k in[x + k]
  t[r - k]). For any summation order of the n = 2r + 1 products, fused or not: |buf - buf64| <= gamma(n) sum |t_k| |x_k|; for the
  result the same with buf in place of x, plus sum |t_k| e_row. Input and tap errors (e_x, e_t; the chain) enter as
  sum |t_k| e_x + sum e_t (|x_k| + e_x).
DECIMATION, SUBTRACTION (downsample64, subtract64): a copy / one IEEE subtraction of float32 operands: RN32 of the model value IS
  the answer; compared with array_equal.
GRADIENT (gradient64): dx = fl(nx - px), g = 0.5 sqrtf(fma(dx, dx, fl(dy dy))): the squares carry 2u + u, the fma one more, the
  root halves and adds one: |g - g64| <= 3.5u g + TINY (domain: dx^2, dy^2 not subnormal or zero). The ring is (0, 0); g == 0 <=> dx = dy = 0.
  angle = mod_2pi_f((float)(atan2f(dy, dx) + 2 pi)): with a = atan2: u (the roundings of dy, dx move a by at most u 2 |dx dy| / r^2),
  2.5 ulp(a) <= 5u |a| (atan2f, tests/test_oracle_math.py), u |a + 2 pi| (the cast); a wrap subtracts (float)(2 pi), which is
  2.9u off 2 pi, and rounds once more: + 2.9u + u |theta|. theta lies in (0, 2 pi]: a = 0 gives (float)(2 pi). A pixel with
  0 < |a| <= max(16u, twice its angle bound) is fragile (its float sum a + 2 pi may round to (float)(2 pi) and not wrap, or its
  a may have the other sign) and is left out of the angle comparison.
  With an input error e (the chain): e_dx = e(x+1) + e(x-1) + u |dx|, e_g = (e_dx + e_dy) / 2 + 3.5u g, and the angle gains
  (|dx| e_dy + |dy| e_dx) / (r (r - e_r)); a pixel with r <= 4 (e_dx + e_dy) is fragile.
EXTREMA (extrema64): strict against all 26 neighbours, gate c >= fl(0.8f peak) for maxima / c <= for minima (both at equality),
  the 1-pixel frame skipped, mask = bilinear border fetch of the full-resolution plane at ((x + 0.5) xper, (y + 0.5) xper) >= 1
  (exact for xper a power of two and the masks used). Comparisons of the given floats: the candidate set is exact.
REFINEMENT (refine64): g = (fx, fy, fs), H from the 3 x 3 x 3 neighbourhood, d = -H^-1 g by np.linalg.solve.
  Formation: fx = 0.5 fl(a - b): u |fx|; fxx = fl(fl(a + b) - 2c): u |a + b| + u |fxx|; fxy = 0.25 fl(fl(fl(a + b) - c) - d):
  0.25 u (|a + b| + |a + b - c| + |a + b - c - d|); each + TINY. These are e_g and e_H.
  The bound on d is the CONDITION-NUMBER FORM. The reference eliminates with partial pivoting (largest leading element first,
  the larger of the two remaining second), for which the computed d solves (H + dH) d = -(g + dg) with |dH| <= e_H +
  gamma(9) |L||U| and |L||U| <= n rho max|H| = 12 max|H| elementwise (n = 3, growth rho <= 4; Higham, Accuracy and Stability,
  Thm 9.4 with 9.3). With E = e_H + 12 gamma(9) max|H| and rho_E = || |H^-1| E ||_inf < 1 (else the candidate is fragile):
      |delta d| <= |H^-1| (E |d| + e_g) / (1 - rho_E)                                      (Higham Thm 7.4)
  which holds for ANY pivot order a binary32 evaluation may choose, so no row-swap decision enters.
  v = c + 0.5 g.d: e_v = 0.5 (|g| . e_d + e_g . |d|) + 0.5 gamma(3) sum |g_i d_i| + u |v|.
  score = tr^2 / det, tr = fxx + fyy, det = fxx fyy - fxy^2: e_tr = e_fxx + e_fyy + u |tr|, e_det = |fyy| e_fxx + |fxx| e_fyy +
  2 |fxy| e_fxy + u (|fxx fyy| + fxy^2 + |det|) + TINY; relative e_s = 2 e_tr / |tr| + e_det / (|det| - e_det) + 2u. Compared with
  (e + 1)^2 / e (2u relative). A negative determinant gives a negative score and is ACCEPTED; |det| <= e_det is fragile.
  Pivots: every pivot of ANY partial-pivoting order is at least |det H| / (4 max|H|)^2 in magnitude; where that exceeds
  1e-10 (all ordinary content) the three tests pass whatever the order. Otherwise the pivots are taken in the reference's order
  (elimination in binary64) with a running error bound (z = x / y: (e_x + |z| e_y) / (|y| - e_y) + u |z|; fma(-a, b, c):
  |a| e_b + |b| e_a + e_a e_b + e_c + u |result|), and a row choice within its bound makes the candidate fragile.
  Outputs: X = (x + dx) xper: (e_dx + u |x + dx|) xper + u |X|, Y alike; S = sigma_0 2^((level + ds) / num_dogs) xper: relative
  ln 2 (e_ds + u |level + ds|) / num_dogs + 2u; w = level.
  FRAGILE: a pivot next to 1e-10, |v| next to peak, the score next to its threshold, an offset next to 1 -- margin / bound <= 1.
  Fragile candidates are left out of the VALUE comparison only (a fragile candidate must still be either the sentinel or a row
  of its level); their number is reported.
CHAIN (octave64): levels 1..5 from level 0 in binary64 without intermediate rounding, the model's own sigmas (relative error
  PARAM_REL in the taps); level error e_l propagated through convolve64, DoG error e_{l+1} + e_l + u |d|, gradient as above.

MEASURED ON THE MODEL (tests/test_scale_space_float64.py and tests/test_gpu_scale_space_float64.py print them)
  worst deviation / bound, CPU (the oracle) | GPU (every kernel family of the stage):
    parameters 0.16 | sigmas as the product's taps see them: taps 0.42          taps 0.42 | 0.42
    convolution, row pass 0.38 | 0.38 (packed 320x200), 0.38 / 0.35 / 0.11 (tile 201x83, misaligned 68x35, 3x2)
    convolution, result   0.22 | 0.22, 0.21 / 0.16 / 0.05
    decimation, subtraction: array_equal on both sides
    gradient magnitude 0.50 | 0.50     angle 0.72 | 0.74 (single and batch launch, ramp, flats, step field)
    chain (fused octave; the bound carries the taps' 16 eps_sigma term, hence the small ratios):
      levels 0.068 | 0.068 (octave_pyramid), 0.077 (scale_space_batch, level 0 included)    DoG 0.067 | 0.067, 0.031
      gradient magnitude 0.023 | 0.023, 0.010     angle 0.052 | 0.052, 0.024
    keypoints (x, y, sigma) 0.38 | detection forms 0.13-0.34 over the twelve shapes, wide exponent 0.058, saddle 0.29, ties 0.30
    whole frame 0.34 | frame driver 0.37 (320x200), 0.32 (250x131), 5-row and tall unit groups alike; octave tail 0.44 (640x480)
  fragile share per case (cap 5 %): 0 on every detection case (dense planes at the twelve shapes, 320x200 octave, peak, offset,
    steps, saddle, masked xper 1 and 2, wide exponent); whole frames: 320x200 0.31 %, 250x131 0; gradient pixels next to the
    wrap: 0 on float32 inputs, at most 3 pixels of a 320x200 plane in the chain.
  Note: with DoG planes asked for, nm_sift_scale_space_batch does not store level 5 (it is only read through DoG 4).
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
SLACK = 1.01
TWO_PI = 2.0 * np.pi
F2PI = float(np.float32(TWO_PI))
PIVOT_MIN = 1e-10

PARAM_REL = dict(sigma_k=2 * U, sigma_0=4 * U, sigma_d_0=10 * U, base_smooth=10 * U,
                 sigmas=[(11 + 2 * i) * U for i in range(5)])

MUTANTS = ("sigma_absolute", "radius_round", "taps_unnormalised", "border_replicate", "decimate_odd", "dog_sign", "grad_no_half",
           "angle_half_open", "extremum_ge", "no_sign_gate", "gate_at_peak", "edge_abs_det", "offset_half", "updn_fs", "updn_fxs",
           "updn_fys", "sigma_no_div", "sigma_no_xper", "v_no_half", "mask_no_half")


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


def ratio(dev, bound):
    """max of |dev| / bound; a zero bound demands a zero deviation (ratio 0 then, inf otherwise)."""
    dev, bound = np.abs(np.asarray(dev, np.float64)), np.broadcast_to(np.asarray(bound, np.float64), np.shape(dev))
    if dev.size == 0:
        return 0.0
    out = np.where(dev == 0, 0.0, np.inf)
    np.divide(dev, bound, out=out, where=bound > 0)
    return float(np.max(out))


def _margin(margin, bound):
    """margin / bound per element; inf where the bound is 0 and the margin is not."""
    margin, bound = np.abs(np.asarray(margin, np.float64)), np.asarray(bound, np.float64)
    out = np.where(margin > 0, np.inf, 0.0) * np.ones(np.broadcast(margin, bound).shape)
    np.divide(margin, bound, out=out, where=bound > 0)
    return out


# ---- parameters and taps --------------------------------------------------------------------------------------------------------
def sift_params64(width, height, mutant=None):
    """siftparams.h:30-51 in real numbers. Returns a dict; PARAM_REL holds the relative bounds of the float fields."""
    nd = 3
    no = int(np.floor(np.log2(min(width, height) * 2.0 / 32.0)))
    k = 2.0 ** (1.0 / nd)
    s0 = 1.6 * k
    sd0 = s0 * np.sqrt(1.0 - 1.0 / (k * k))
    sa, sb = s0 / k, 0.5
    lo, hi = -1, nd + 1
    if mutant == "sigma_absolute":
        sig = [s0 * k ** i for i in range(lo + 1, hi + 1)]
    else:
        sig = [sd0 * k ** i for i in range(lo + 1, hi + 1)]
    return dict(num_octaves=max(no, 1), num_dog_levels=nd, level_min=lo, level_max=hi, sigma_k=k, sigma_0=s0, sigma_d_0=sd0,
                sigma_n=sb, base_smooth=float(np.sqrt(sa * sa - sb * sb)), sigmas=sig, peak_threshold=0.0, edge_threshold=10.0)


def taps64(sigma, mutant=None, eps_sigma=0.0):
    """pyramidata.cu:105-123 for a float32 sigma. Returns (taps (2r+1,), bound (2r+1,), r)."""
    sigma = float(np.float32(sigma))
    a = 4.0 * sigma
    r = int(np.rint(a)) if mutant == "radius_round" else int(np.ceil(a))
    j = np.arange(2 * r + 1, dtype=np.float64) - r
    q = (j / sigma) ** 2
    v = np.exp(-0.5 * q)
    e_v = v * (1.5 * U * q + U) + TINY
    n = len(v)
    S = v.sum()
    e_S = gamma(n - 1) * S + e_v.sum()
    t = v if mutant == "taps_unnormalised" else v / S
    qbar = float((q * v).sum() / S)
    e_t = SLACK * t * (e_v / v + e_S / S + U + np.abs(q - qbar) * eps_sigma) + TINY
    return t, e_t, r


# ---- convolution ----------------------------------------------------------------------------------------------------------------
def _corr_axis(x, t, r, axis, mode):
    """out[i] = sum_k x[i + k] t[r - k], k = -r..r, along `axis`; outside the plane 0 ("zero") or the edge value ("edge")."""
    pad = [(0, 0), (0, 0)]
    pad[axis] = (r, r)
    xp = np.pad(x, pad, mode="constant" if mode == "zero" else "edge")
    n = x.shape[axis]
    out = np.zeros_like(x)
    for k in range(-r, r + 1):
        sl = [slice(None), slice(None)]
        sl[axis] = slice(r + k, r + k + n)
        out += xp[tuple(sl)] * t[r - k]
    return out


def convolve64(image, taps, r, e_taps=None, e_image=None, mutant=None):
    """convolution.cu:16-159. image float32 (h, w) (or float64 with e_image: the chain). Returns dict(buf, out, e_buf, e_out)."""
    x = np.asarray(image).astype(np.float64)
    t = np.asarray(taps, np.float64)
    at = np.abs(t)
    et = np.zeros_like(t) if e_taps is None else np.asarray(e_taps, np.float64)
    ex = np.zeros_like(x) if e_image is None else np.asarray(e_image, np.float64)
    mode = "edge" if mutant == "border_replicate" else "zero"
    n = 2 * r + 1
    g = float(gamma(n))
    buf = _corr_axis(x, t, r, 1, mode)
    ax = np.abs(x) + ex
    e_buf = SLACK * (g * _corr_axis(ax, at + et, r, 1, "zero") + _corr_axis(ax, et, r, 1, "zero") + _corr_axis(ex, at, r, 1, "zero")) + TINY
    out = _corr_axis(buf, t, r, 0, mode)
    ab = np.abs(buf) + e_buf
    e_out = SLACK * (g * _corr_axis(ab, at + et, r, 0, "zero") + _corr_axis(ab, et, r, 0, "zero") + _corr_axis(e_buf, at, r, 0, "zero")) + TINY
    return dict(buf=buf, out=out, e_buf=e_buf, e_out=e_out)


def downsample64(src, rw, rh, mutant=None):
    """downsample.cu:6-17: result(x, y) = source(2x, 2y)."""
    s = np.asarray(src).astype(np.float64)
    o = 1 if mutant == "decimate_odd" else 0
    return s[o::2, o::2][:rh, :rw].copy()


def subtract64(a, b, mutant=None):
    """cudamath.cu:26-35: A - B."""
    a, b = np.asarray(a).astype(np.float64), np.asarray(b).astype(np.float64)
    return b - a if mutant == "dog_sign" else a - b


# ---- gradient -------------------------------------------------------------------------------------------------------------------
def gradient64(src, e_src=None, mutant=None):
    """cudamath.cu:38-54. Returns dict(mag, ang (h, w), e_mag, e_ang, fragile (h, w) bool: the angle is not compared there)."""
    s = np.asarray(src).astype(np.float64)
    h, w = s.shape
    e = np.zeros_like(s) if e_src is None else np.asarray(e_src, np.float64)
    mag, ang = np.zeros((h, w)), np.zeros((h, w))
    e_mag, e_ang = np.zeros((h, w)), np.zeros((h, w))
    fragile = np.zeros((h, w), bool)
    if h < 3 or w < 3:
        return dict(mag=mag, ang=ang, e_mag=e_mag, e_ang=e_ang, fragile=fragile)
    dx, dy = s[1:-1, 2:] - s[1:-1, :-2], s[2:, 1:-1] - s[:-2, 1:-1]
    e_dx = e[1:-1, 2:] + e[1:-1, :-2] + U * np.abs(dx)
    e_dy = e[2:, 1:-1] + e[:-2, 1:-1] + U * np.abs(dy)
    e_in = e_dx + e_dy - U * (np.abs(dx) + np.abs(dy))             # what the input error contributes (0 for float32 inputs)
    r = np.sqrt(dx * dx + dy * dy)
    g = r if mutant == "grad_no_half" else 0.5 * r
    a = np.arctan2(dy, dx)
    th = a + TWO_PI
    wrap = th >= TWO_PI if mutant == "angle_half_open" else th > TWO_PI
    th = np.where(wrap, th - TWO_PI, th)
    th = np.where(g == 0, 0.0, th)
    e_r = e_dx + e_dy
    safe = r > 4.0 * e_in
    den = np.where(safe, r * (r - e_r), 1.0)
    e_a = np.where(safe, (np.abs(dx) * e_dy + np.abs(dy) * e_dx) / np.where(den > 0, den, 1.0), 0.0)   # includes the u of dx, dy
    e_th = SLACK * (e_a + 5 * U * np.abs(a) + U * np.abs(a + TWO_PI) + np.where(wrap, abs(TWO_PI - F2PI) + U * np.abs(th), 0.0))
    frag = ((np.abs(a) <= np.maximum(16 * U, 2 * e_th)) & ~((a == 0) & (e_in == 0))) | (~safe & (e_in > 0))
    c = (slice(1, -1), slice(1, -1))
    mag[c], ang[c] = g, th
    e_mag[c] = SLACK * (0.5 * e_in + 3.5 * U * g) + np.where(r > 0, TINY, 0.0) + np.where(e_in > 0, TINY, 0.0)
    e_ang[c] = np.where(g == 0, 0.0, e_th)
    fragile[c] = frag
    return dict(mag=mag, ang=ang, e_mag=e_mag, e_ang=e_ang, fragile=fragile)


def gradient_outside(model, got):
    """Number of pixels of `got` (h, w, 2) float32 outside the model's bounds (angle: non-fragile pixels only), and the worst
    deviation / bound of magnitude and angle."""
    got = np.asarray(got, np.float64)
    dm, da = np.abs(got[..., 0] - model["mag"]), np.abs(got[..., 1] - model["ang"])
    keep = ~model["fragile"]
    bad = int((~(dm <= model["e_mag"])).sum() + (~(da <= model["e_ang"]) & keep).sum())
    return bad, ratio(dm, model["e_mag"]), ratio(da[keep], model["e_ang"][keep])


# ---- extrema --------------------------------------------------------------------------------------------------------------------
def mask_fetch64(mask, u, v):
    """Bilinear, border-addressed, unnormalised fetch (cudatex2D.cu:15-19) of a float plane at texture coordinates (u, v)."""
    m = np.asarray(mask).astype(np.float64)
    mh, mw = m.shape
    xb, yb = np.asarray(u, np.float64) - 0.5, np.asarray(v, np.float64) - 0.5
    i, j = np.floor(xb).astype(np.int64), np.floor(yb).astype(np.int64)
    a, b = xb - i, yb - j

    def T(ii, jj):
        ok = (ii >= 0) & (ii < mw) & (jj >= 0) & (jj < mh)
        return np.where(ok, m[np.clip(jj, 0, mh - 1), np.clip(ii, 0, mw - 1)], 0.0)
    return (1 - a) * (1 - b) * T(i, j) + a * (1 - b) * T(i + 1, j) + (1 - a) * b * T(i, j + 1) + a * b * T(i + 1, j + 1)


def extrema64(cur, dn, up, peak, xper=1.0, mask=None, mutant=None):
    """keypoint.cu:19-106, 183-224: (ys, xs) of the candidates in raster order. Exact: comparisons of the given floats."""
    P = [np.asarray(p).astype(np.float64) for p in (cur, dn, up)]
    h, w = P[0].shape
    if h < 3 or w < 3:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    c = P[0][1:-1, 1:-1]
    gt, lt = np.ones(c.shape, bool), np.ones(c.shape, bool)
    for pi, p in enumerate(P):
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                if pi == 0 and dx == 1 and dy == 1:
                    continue
                nb = p[dy:dy + h - 2, dx:dx + w - 2]
                if mutant == "extremum_ge":
                    gt &= c >= nb
                    lt &= c <= nb
                else:
                    gt &= c > nb
                    lt &= c < nb
    thr = float(np.float32(np.float32(peak) if mutant == "gate_at_peak" else np.float32(0.8) * np.float32(peak)))
    if mutant == "no_sign_gate":
        cand = gt | lt
    else:
        cand = (lt & (c <= thr)) | (gt & (c >= thr))
    if mask is not None:
        yy, xx = np.mgrid[1:h - 1, 1:w - 1]
        half = 0.0 if mutant == "mask_no_half" else 0.5
        xp = float(np.float32(xper))
        cand &= mask_fetch64(mask, (xx + half) * xp, (yy + half) * xp) >= 1.0
    ys, xs = np.nonzero(cand)
    return ys + 1, xs + 1


# ---- refinement -----------------------------------------------------------------------------------------------------------------
def _reference_pivots(H, eH):
    """The three pivots of keypoint.cu:137-161 in binary64 with a running error bound, and whether a row choice lies within its
    bound. H, eH: (n, 3, 3). Returns (p (n, 3), e_p (n, 3), ambiguous (n,))."""
    n = len(H)
    A, E = H.copy(), eH.copy()
    sg = np.where(np.stack([H[:, 0, 0], H[:, 0, 1], H[:, 0, 2]], 1) > 0, 1.0, -1.0)        # rows made non-negative in column 0
    A = A * sg[:, :, None]
    lead = A[:, :, 0]
    order = np.argmax(np.stack([lead[:, 1], lead[:, 2], lead[:, 0]], 1), 1)                # ties: row 1, else row 2, else row 0
    piv = np.array([1, 2, 0])[order]
    mx = lead.max(1)
    others = np.where(np.arange(3)[None, :] == piv[:, None], -np.inf, lead)
    amb = (mx - others.max(1)) <= (E[:, :, 0].max(1) * 2)
    idx = np.arange(n)
    for k in (1, 2):                                                                       # swap row piv to the front
        m = piv == k
        A[m, 0], A[m, k] = A[m, k].copy(), A[m, 0].copy()
        E[m, 0], E[m, k] = E[m, k].copy(), E[m, 0].copy()
    p1, e1 = A[:, 0, 0], E[:, 0, 0]
    with np.errstate(all="ignore"):
        den = np.abs(p1) - e1
        u01, u02 = A[:, 0, 1] / p1, A[:, 0, 2] / p1
        eu01 = (E[:, 0, 1] + np.abs(u01) * e1) / den + U * np.abs(u01)
        eu02 = (E[:, 0, 2] + np.abs(u02) * e1) / den + U * np.abs(u02)

        def fms(c, ec, a, ea, b, eb):                                                      # fma(-a, b, c)
            res = c - a * b
            return res, np.abs(a) * eb + np.abs(b) * ea + ea * eb + ec + U * np.abs(res) + TINY
        r1y, e1y = fms(A[:, 1, 1], E[:, 1, 1], A[:, 1, 0], E[:, 1, 0], u01, eu01)
        r1z, e1z = fms(A[:, 1, 2], E[:, 1, 2], A[:, 1, 0], E[:, 1, 0], u02, eu02)
        r2y, e2y = fms(A[:, 2, 1], E[:, 2, 1], A[:, 2, 0], E[:, 2, 0], u01, eu01)
        r2z, e2z = fms(A[:, 2, 2], E[:, 2, 2], A[:, 2, 0], E[:, 2, 0], u02, eu02)
        sw = np.abs(r2y) > np.abs(r1y)
        amb |= np.abs(np.abs(r2y) - np.abs(r1y)) <= e1y + e2y
        b1y, f1y, b1z, f1z = np.where(sw, r2y, r1y), np.where(sw, e2y, e1y), np.where(sw, r2z, r1z), np.where(sw, e2z, e1z)
        b2y, f2y, b2z, f2z = np.where(sw, r1y, r2y), np.where(sw, e1y, e2y), np.where(sw, r1z, r2z), np.where(sw, e1z, e2z)
        q = b1z / b1y
        eq = (f1z + np.abs(q) * f1y) / (np.abs(b1y) - f1y) + U * np.abs(q)
        p3, e3 = fms(b2z, f2z, b2y, f2y, q, eq)
    p = np.stack([p1, b1y, p3], 1)
    e = np.stack([e1, f1y, e3], 1)
    bad = ~np.isfinite(p) | ~np.isfinite(e) | (e < 0)
    return np.where(bad, 0.0, p), np.where(bad, np.inf, e), amb


def refine64(cur, dn, up, ys, xs, peak, edge, xper, sigma0, num_dogs, level, mutant=None):
    """keypoint.cu:108-180 on the candidates (ys, xs). Returns a dict of per-candidate arrays: accepted (bool), kp (n, 4) =
    (X, Y, S, level) (valid where accepted), bound (n, 3), fragile (bool), margins {pivot, peak, edge, offset} (margin / bound),
    d (n, 3), e_d (n, 3), ys, xs."""
    ys, xs = np.asarray(ys, np.int64), np.asarray(xs, np.int64)
    n = len(ys)
    P = [np.asarray(p).astype(np.float64) for p in (dn, cur, up)]
    peak, edge, xper, sigma0 = (float(np.float32(v)) for v in (peak, edge, xper, sigma0))
    nb = np.empty((n, 3, 3, 3))
    for s in range(3):
        for j in range(3):
            for i in range(3):
                nb[:, s, j, i] = P[s][ys + j - 1, xs + i - 1]

    def C(dx, dy): return nb[:, 1, 1 + dy, 1 + dx]
    def D(dx, dy): return nb[:, 0, 1 + dy, 1 + dx]
    def Up(dx, dy): return nb[:, 2, 1 + dy, 1 + dx]
    c = C(0, 0)

    def first(a, b):                       # 0.5 fl(a - b)
        v = 0.5 * (a - b)
        return v, U * np.abs(v) + TINY

    def second(a, b):                      # fl(fl(a + b) - 2c)
        v = a + b - 2.0 * c
        return v, U * np.abs(a + b) + U * np.abs(v) + TINY

    def cross(a, b, cc, d):                # 0.25 fl(fl(fl(a + b) - cc) - d)
        v = 0.25 * (a + b - cc - d)
        return v, 0.25 * U * (np.abs(a + b) + np.abs(a + b - cc) + np.abs(a + b - cc - d)) + TINY
    fx, e_fx = first(C(1, 0), C(-1, 0))
    fy, e_fy = first(C(0, 1), C(0, -1))
    fs, e_fs = first(D(0, 0), Up(0, 0)) if mutant == "updn_fs" else first(Up(0, 0), D(0, 0))
    fxx, e_fxx = second(C(1, 0), C(-1, 0))
    fyy, e_fyy = second(C(0, 1), C(0, -1))
    fss, e_fss = second(Up(0, 0), D(0, 0))
    fxy, e_fxy = cross(C(1, 1), C(-1, -1), C(-1, 1), C(1, -1))
    if mutant == "updn_fxs":
        fxs, e_fxs = cross(D(1, 0), Up(-1, 0), D(-1, 0), Up(1, 0))
    else:
        fxs, e_fxs = cross(Up(1, 0), D(-1, 0), Up(-1, 0), D(1, 0))
    if mutant == "updn_fys":
        fys, e_fys = cross(D(0, 1), Up(0, -1), D(0, -1), Up(0, 1))
    else:
        fys, e_fys = cross(Up(0, 1), D(0, -1), Up(0, -1), D(0, 1))
    g = np.stack([fx, fy, fs], 1)
    e_g = np.stack([e_fx, e_fy, e_fs], 1)
    H = np.stack([np.stack([fxx, fxy, fxs], 1), np.stack([fxy, fyy, fys], 1), np.stack([fxs, fys, fss], 1)], 1)
    eH = np.stack([np.stack([e_fxx, e_fxy, e_fxs], 1), np.stack([e_fxy, e_fyy, e_fys], 1), np.stack([e_fxs, e_fys, e_fss], 1)], 1)
    hmax = np.abs(H).reshape(n, 9).max(1) if n else np.zeros(0)
    # d = -H^-1 g on a row-scaled system (the scaling by a power of two is exact and keeps wide-exponent cases inside binary64)
    with np.errstate(all="ignore"):
        scale = np.where(hmax > 0, 2.0 ** -np.floor(np.log2(np.where(hmax > 0, hmax, 1.0))), 1.0)
        Hs = H * scale[:, None, None]
        dets = np.linalg.det(Hs) if n else np.zeros(0)
        regular = np.isfinite(dets) & (np.abs(dets) > 1e-300) & (hmax > 0)
        d = np.zeros((n, 3))
        Hinv = np.zeros((n, 3, 3))
        if regular.any():
            d[regular] = np.linalg.solve(Hs[regular], -(g[regular] * scale[regular, None])[..., None])[..., 0]
            Hinv[regular] = np.abs(np.linalg.inv(Hs[regular])) * scale[regular, None, None]
        E = eH + 12.0 * float(gamma(9)) * hmax[:, None, None]
        rho = (Hinv @ E).sum(2).max(1) if n else np.zeros(0)
        ok = regular & (rho < 1.0)
        e_d = SLACK * (Hinv @ ((E @ np.abs(d)[..., None])[..., 0] + e_g)[..., None])[..., 0] / np.where(ok, 1.0 - rho, 1.0)[:, None]
        e_d = np.where(ok[:, None], e_d, np.inf)
        # pivots
        floor_any = np.abs(dets / scale ** 3) / np.where(hmax > 0, (4.0 * hmax) ** 2, 1.0) * (1.0 - 64 * U)
        p, e_p, amb = _reference_pivots(H, eH) if n else (np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, bool))
        sure = regular & (floor_any > PIVOT_MIN)
        piv_ok = sure | (np.abs(p) >= PIVOT_MIN).all(1)
        m_piv = np.where(sure, np.inf, np.where(amb, 0.0, _margin(np.abs(p) - PIVOT_MIN, e_p).min(1) if n else 0.0))
        # value
        gd = g * d
        half = 1.0 if mutant == "v_no_half" else 0.5
        v = c + half * gd.sum(1)
        e_v = SLACK * (0.5 * ((np.abs(g) * e_d).sum(1) + (e_g * np.abs(d)).sum(1)) + 0.5 * float(gamma(3)) * np.abs(gd).sum(1)) + U * np.abs(v) + TINY
        m_peak = _margin(np.abs(v) - peak, e_v)
        # edge score
        tr = fxx + fyy
        det2 = fxx * fyy - fxy * fxy
        e_tr = e_fxx + e_fyy + U * np.abs(tr)
        e_det = SLACK * (np.abs(fyy) * e_fxx + np.abs(fxx) * e_fyy + 2 * np.abs(fxy) * e_fxy) + U * (np.abs(fxx * fyy) + fxy * fxy + np.abs(det2)) + TINY
        score = tr * tr / (np.abs(det2) if mutant == "edge_abs_det" else det2)
        ethr = (edge + 1.0) * (edge + 1.0) / edge
        det_ok = np.abs(det2) > e_det
        rel_s = SLACK * (2 * e_tr / np.where(tr != 0, np.abs(tr), 1.0) + e_det / np.where(det_ok, np.abs(det2) - e_det, 1.0) + 2 * U)
        e_s = np.abs(score) * rel_s + 2 * U * ethr
        m_edge = np.where(det_ok, _margin(score - ethr, e_s), 0.0)
        edge_ok = score < ethr
        lim = 0.5 if mutant == "offset_half" else 1.0
        m_off = _margin(np.abs(d) - 1.0, e_d).min(1) if n else np.zeros(0)
        off_ok = (np.abs(d) < lim).all(1)
        accepted = piv_ok & regular & (np.abs(v) > peak) & edge_ok & off_ok
        # outputs
        X, Y = (xs + d[:, 0]) * xper, (ys + d[:, 1]) * xper
        bX = SLACK * ((e_d[:, 0] + U * np.abs(xs + d[:, 0])) * xper + U * np.abs(X)) + TINY
        bY = SLACK * ((e_d[:, 1] + U * np.abs(ys + d[:, 1])) * xper + U * np.abs(Y)) + TINY
        lev = level + d[:, 2]
        ex = lev if mutant == "sigma_no_div" else lev / num_dogs
        S = sigma0 * 2.0 ** ex * (1.0 if mutant == "sigma_no_xper" else xper)
        bS = SLACK * S * (np.log(2.0) * (e_d[:, 2] + U * np.abs(lev)) / num_dogs + 2 * U) + TINY
    margins = dict(pivot=m_piv, peak=m_peak, edge=m_edge, offset=m_off)
    fragile = np.stack([margins[k] for k in ("pivot", "peak", "edge", "offset")]).min(0) <= 1.0 if n else np.zeros(0, bool)
    fragile = fragile | ~ok
    kp = np.stack([X, Y, S, np.full(n, float(level))], 1) if n else np.zeros((0, 4))
    return dict(accepted=accepted, kp=kp, bound=np.stack([bX, bY, bS], 1) if n else np.zeros((0, 3)), fragile=fragile,
                margins=margins, d=d, e_d=e_d, ys=ys, xs=xs, v=v, score=score, level=level, xper=xper)


def detect64(cur, dn, up, peak, edge, xper, sigma0, num_dogs, level, mask=None, mutant=None):
    """find_keypoints (keypoint.cu:183-251) on three DoG planes: extrema64 + refine64. The dict of refine64 plus shape."""
    ys, xs = extrema64(cur, dn, up, peak, xper, mask, mutant)
    out = refine64(cur, dn, up, ys, xs, peak, edge, xper, sigma0, num_dogs, level, mutant)
    out["shape"] = np.asarray(cur).shape
    return out


def octave_detect64(dogs, peak, edge, xper, sigma0, num_dogs=3, mask=None, mutant=None):
    """The three detections of one octave: level l searches dogs[l + 1] between dogs[l] and dogs[l + 2]."""
    return [detect64(dogs[l + 1], dogs[l], dogs[l + 2], peak, edge, xper, sigma0, num_dogs, l, mask, mutant) for l in range(num_dogs)]


def frame_list64(octaves):
    """octaves: per octave the list of octave_detect64. An empty level ends its octave (siftfunctions.cu:145,160; an empty level
    whose emptiness hangs on a fragile candidate is reported). Returns the levels' models in output order."""
    out = []
    for levels in octaves:
        for m in levels:
            if not (m["accepted"] | m["fragile"]).any():
                break
            out.append(m)
    return out


# ---- comparison of an implementation's float32 keypoints with the model --------------------------------------------------------
def dense_outside(model, got, sentinel=-1.0):
    """`got`: the dense (h, w, 4) float32 map. Returns (number of wrong pixels, worst deviation / bound over the compared values,
    number of fragile candidates). A pixel that is no candidate, or a non-fragile rejected candidate, must hold the sentinel in
    all four floats; a non-fragile accepted candidate must hold its keypoint within the bounds and its level exactly; a fragile
    candidate must hold the sentinel or a row of its level."""
    got = np.asarray(got, np.float64)
    h, w = model["shape"]
    ys, xs = model["ys"], model["xs"]
    is_cand = np.zeros((h, w), bool)
    is_cand[ys, xs] = True
    bad = int((~is_cand[..., None] & (got != sentinel)).sum())
    row = got[ys, xs]
    fr, acc = model["fragile"], model["accepted"]
    empty = (row == sentinel).all(1)
    bad += int((~fr & ~acc & ~empty).sum())
    dev = np.abs(row[:, :3] - model["kp"][:, :3])
    cmp_ = ~fr & acc
    inside = (dev <= model["bound"]).all(1) & (row[:, 3] == model["level"])
    bad += int((cmp_ & ~inside).sum())
    bad += int((fr & ~empty & (row[:, 3] != model["level"])).sum())
    return bad, ratio(dev[cmp_ & ~empty], model["bound"][cmp_ & ~empty]), int(fr.sum())


def list_outside(models, got):
    """`got`: (m, 4) float32 rows, the raster-ordered lists of `models` (one per level) back to back. Walks both in order: every
    non-fragile accepted candidate must be the next row (within its bounds, level exact); a fragile candidate may take the next
    row when that row lies within a pixel of it at its level. Returns (number of mismatches, worst ratio, fragile count)."""
    got = np.asarray(got, np.float64).reshape(-1, 4)
    p, bad, worst, nfr = 0, 0, 0.0, 0
    for m in models:
        xper = m["xper"]
        for k in range(len(m["ys"])):
            fr, acc = bool(m["fragile"][k]), bool(m["accepted"][k])
            nfr += fr
            if not fr and not acc:
                continue
            row = got[p] if p < len(got) else None
            if fr:
                if row is not None and row[3] == m["level"] and abs(row[0] / xper - m["xs"][k]) < 1 and abs(row[1] / xper - m["ys"][k]) < 1:
                    p += 1
                continue
            if row is None:
                bad += 1
                continue
            dev = np.abs(row[:3] - m["kp"][k, :3])
            if (dev <= m["bound"][k]).all() and row[3] == m["level"]:
                worst = max(worst, ratio(dev, m["bound"][k]))
            else:
                bad += 1
            p += 1
    bad += len(got) - p if p < len(got) else 0
    return bad, worst, nfr


def fragile_share(models):
    n = sum(len(m["ys"]) for m in models)
    return (sum(int(m["fragile"].sum()) for m in models) / n) if n else 0.0


# ---- chain ----------------------------------------------------------------------------------------------------------------------
def octave64(level0, width, height, mutant=None, want_grad=True, e_level0=None):
    """One octave from its level 0 (float32, or binary64 with its error e_level0): levels (6), e_levels, dogs (5), e_dogs, grads
    (3 dicts of gradient64 on levels 1..3)."""
    P = sift_params64(width, height, mutant)
    lv = [np.asarray(level0).astype(np.float64)]
    ev = [np.zeros_like(lv[0]) if e_level0 is None else np.asarray(e_level0, np.float64)]
    for i, s in enumerate(P["sigmas"]):
        t, et, r = taps64(np.float32(s), mutant, eps_sigma=PARAM_REL["sigmas"][i] + U)
        c = convolve64(lv[i], t, r, e_taps=et, e_image=ev[i], mutant=mutant)
        lv.append(c["out"])
        ev.append(c["e_out"])
    dogs = [subtract64(lv[i + 1], lv[i], mutant) for i in range(5)]
    e_dogs = [SLACK * (ev[i + 1] + ev[i] + U * np.abs(dogs[i])) + TINY for i in range(5)]
    grads = [gradient64(lv[l + 1], ev[l + 1], mutant) for l in range(3)] if want_grad else None
    return dict(levels=lv, e_levels=ev, dogs=dogs, e_dogs=e_dogs, grads=grads, params=P)


def frame_octave0_64(gray, mutant=None):
    """Octave 0 of a frame: level 0 is the float32 frame blurred by base_smooth, then octave64 with that level's error."""
    h, w = np.asarray(gray).shape
    P = sift_params64(w, h, mutant)
    t, et, r = taps64(np.float32(P["base_smooth"]), mutant, eps_sigma=PARAM_REL["base_smooth"] + U)
    c = convolve64(gray, t, r, e_taps=et, mutant=mutant)
    return octave64(c["out"], w, h, mutant, e_level0=c["e_out"])


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def wide_exponent_dogs(seed, width=64, height=28):
    """Three DoG planes of isolated spikes on a 4-pixel grid of the middle plane: a spike of magnitude 2^k, k from -40 to 40, sits
    in neighbours of its own sign that are more than 2^29 times smaller (random mantissas, 2^(k-31) .. 2^(k-30); with the spike's
    sign and the zero gaps between the blocks none of them is an extremum itself), so that sums such as
    cxp + cxm - 2c have operands beyond the 29-bit window in which a binary64 difference of floats is exact, the squares fxy^2 of
    the small spikes are subnormal or zero in binary32, and the pivots of the smallest spikes lie below 1e-10. Returns float32
    (cur, dn, up)."""
    rng = np.random.default_rng(seed)
    planes = np.zeros((3, height, width), np.float64)
    ks = np.linspace(-40, 40, ((height - 2) // 4) * ((width - 2) // 4)).round().astype(int)
    rng.shuffle(ks)
    i = 0
    for y in range(2, height - 2, 4):
        for x in range(2, width - 2, 4):
            if i >= len(ks):
                break
            k = int(ks[i])
            i += 1
            sign = rng.choice([-1.0, 1.0])
            planes[:, y - 1:y + 2, x - 1:x + 2] = rng.uniform(1.0, 2.0, (3, 3, 3)) * sign * 2.0 ** (k - 31)
            planes[1, y, x] = rng.uniform(1.0, 2.0) * sign * 2.0 ** k
    p32 = planes.astype(np.float32)
    return p32[1], p32[0], p32[2]


def saddle_dogs(seed, width=64, height=28):
    """Three DoG planes of isolated strict maxima on a sharp diagonal ridge: fxx, fyy < 0 and fxy^2 on either side of fxx fyy, so
    that the in-plane determinant is small and of either sign. Where it is NEGATIVE the reference's score tr^2 / det is negative
    and passes the edge test, while tr^2 / |det| would fail it; where it is positive the score is large and fails. Blocks on a
    4-pixel grid over a zero background (no other pixel of a block is an extremum). Returns float32 (cur, dn, up)."""
    rng = np.random.default_rng(seed)
    planes = np.zeros((3, height, width), np.float64)
    for y in range(2, height - 2, 4):
        for x in range(2, width - 2, 4):
            j = lambda: 1.0 + 0.2 * rng.random()
            b = np.empty((3, 3, 3))
            b[0], b[2] = 10.0 - 5.0 * (1.0 + 0.2 * rng.random((3, 3))), 10.0 - 5.0 * (1.0 + 0.2 * rng.random((3, 3)))
            b[1] = [[10.0 - 0.1 * j(), 10.0 - j(), 10.0 - 4.6 * j()], [10.0 - j(), 10.0, 10.0 - j()], [10.0 - 4.6 * j(), 10.0 - j(), 10.0 - 0.1 * j()]]
            planes[:, y - 1:y + 2, x - 1:x + 2] = b
    p32 = planes.astype(np.float32)
    return p32[1], p32[0], p32[2]
