"""A plain float64 reference of the RANSAC stage's geometry, written from the mathematical definitions (numpy only).

Nothing here follows the product's operation sequence (csrc/nm_ransac_math.hpp) or the CPU oracle's (oracle/nmo_ransac.h):
the translation is a subtraction, the similarity the complex ratio of two correspondences, the homography the textbook DLT
(two equations per point, Hartley normalisation to a mean distance of sqrt(2), numpy.linalg.svd, denormalisation by 3x3
matrix products). `fit_lapack32` is the same text run in float32 (LAPACK's Householder SVD): the working-precision
yardstick from which tests/test_ransac_float64.py takes its limits.

All fitters are batched: coordinates of shape (T, ns) give (T, 3, 3) maps and (T, k) singular values.
"""
import numpy as np

SAMPLES = {0: 1, 1: 2, 2: 4}
U32 = 2.0 ** -24                                           # unit roundoff of float32, round to nearest
ETA32 = 2.0 ** -149                                        # smallest float32 subnormal: absolute error of an underflow
FLT_MAX = float(np.finfo(np.float32).max)
MAX_ITERATIONS = 1 << 20                                   # NM_RANSAC_MAX_ITERATIONS

#: A sample is called well posed when sigma[-2] / sigma[0] of its float64 design matrix is at least this. Reasoning: a
#: null vector computed in float32 is perturbed by about u * sigma[0] / sigma[-2] (Wedin), so 1e-3 keeps the relative
#: error of the map near 1e-4 * (a small constant): the fit still has digits left at 8K coordinates. Below it, only the
#: conditioning-normalised forward error is asserted.
WELL_POSED = 1e-3
#: Below this ratio float32 input data cannot resolve the null space at all (16 u); such samples count as degenerate.
RESOLVABLE = 1e-6
#: A fit's pixel error grows like 1 / z^2 near the fit's own horizon line, whatever computes it. The error limits are
#: therefore asserted for samples whose float64 fit keeps z over the sample's points and the four frame corners within a
#: factor 10 (amplification at most 100); the others (wild maps through outliers) are still held to the inlier bracket.
HORIZON = 0.1


# ------------------------------------------------------------------------------------------------------------ fits
def _as2d(a, dtype):
    a = np.asarray(a, dtype)
    return a[None, :] if a.ndim == 1 else a


def _hartley(x, y, dtype):
    """Similarity T (T, 3, 3) that moves the centroid to 0 and the mean distance from it to sqrt(2), and T's inverse."""
    cx, cy = x.mean(axis=1, dtype=dtype), y.mean(axis=1, dtype=dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.sqrt((x - cx[:, None]) ** 2 + (y - cy[:, None]) ** 2, dtype=dtype).mean(axis=1, dtype=dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (dtype(np.sqrt(2.0)) / d).astype(dtype)
    n = len(s)
    Tm, Ti = np.zeros((n, 3, 3), dtype), np.zeros((n, 3, 3), dtype)
    Tm[:, 0, 0] = Tm[:, 1, 1] = s
    with np.errstate(invalid="ignore", over="ignore"):
        Tm[:, 0, 2], Tm[:, 1, 2] = -s * cx, -s * cy
    Tm[:, 2, 2] = 1
    with np.errstate(divide="ignore", invalid="ignore"):
        Ti[:, 0, 0] = Ti[:, 1, 1] = dtype(1) / s
    Ti[:, 0, 2], Ti[:, 1, 2] = cx, cy
    Ti[:, 2, 2] = 1
    return Tm, Ti


def _apply(M, x, y):
    """Points (T, k) through maps (T, 3, 3): (X / Z, Y / Z) in the maps' precision."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        X = M[:, 0, 0, None] * x + M[:, 0, 1, None] * y + M[:, 0, 2, None]
        Y = M[:, 1, 0, None] * x + M[:, 1, 1, None] * y + M[:, 1, 2, None]
        Z = M[:, 2, 0, None] * x + M[:, 2, 1, None] * y + M[:, 2, 2, None]
        return X / Z, Y / Z


def _fit(model, sx, sy, dx, dy, dtype):
    sx, sy, dx, dy = (_as2d(a, dtype) for a in (sx, sy, dx, dy))
    T, ns = sx.shape
    assert ns == SAMPLES[model] and sy.shape == dx.shape == dy.shape == sx.shape
    H = np.zeros((T, 3, 3), dtype)
    H[:, 2, 2] = 1
    if model == 0:
        H[:, 0, 0] = H[:, 1, 1] = 1
        H[:, 0, 2], H[:, 1, 2] = dx[:, 0] - sx[:, 0], dy[:, 0] - sy[:, 0]
        sigma = np.tile(np.array([1, 1, 0], dtype), (T, 1))            # x' = x + t has the design matrix [I | -t]
        return H, sigma
    if model == 1:
        ctype = np.complex64 if dtype == np.float32 else np.complex128
        s = (sx + 1j * sy).astype(ctype)
        d = (dx + 1j * dy).astype(ctype)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            a = (d[:, 1] - d[:, 0]) / (s[:, 1] - s[:, 0])
            t = d[:, 0] - a * s[:, 0]
        H[:, 0, 0], H[:, 0, 1], H[:, 0, 2] = a.real, -a.imag, t.real
        H[:, 1, 0], H[:, 1, 1], H[:, 1, 2] = a.imag, a.real, t.imag
        # design matrix of the unknowns (Re a, Im a, Re t, Im t, w) on Hartley-normalised points: 4 x 5, one null vector
        Ts, _ = _hartley(sx, sy, dtype)
        Td, _ = _hartley(dx, dy, dtype)
        ax, ay = _apply(Ts, sx, sy)
        bx, by = _apply(Td, dx, dy)
        A = np.zeros((T, 4, 5), dtype)
        A[:, 0::2, 0], A[:, 0::2, 1], A[:, 0::2, 2], A[:, 0::2, 4] = ax, -ay, 1, -bx
        A[:, 1::2, 0], A[:, 1::2, 1], A[:, 1::2, 3], A[:, 1::2, 4] = ay, ax, 1, -by
        sigma = np.full((T, 5), np.nan, dtype)
        ok = np.isfinite(A).all(axis=(1, 2))
        if ok.any():
            sigma[ok, :4] = np.linalg.svd(A[ok], compute_uv=False)
            sigma[ok, 4] = 0
        return H, sigma
    Ts, _ = _hartley(sx, sy, dtype)
    Td, Tdi = _hartley(dx, dy, dtype)
    ax, ay = _apply(Ts, sx, sy)
    bx, by = _apply(Td, dx, dy)
    A = np.zeros((T, 8, 9), dtype)
    A[:, 0::2, 3], A[:, 0::2, 4], A[:, 0::2, 5] = -ax, -ay, -1
    A[:, 0::2, 6], A[:, 0::2, 7], A[:, 0::2, 8] = by * ax, by * ay, by
    A[:, 1::2, 0], A[:, 1::2, 1], A[:, 1::2, 2] = ax, ay, 1
    A[:, 1::2, 6], A[:, 1::2, 7], A[:, 1::2, 8] = -bx * ax, -bx * ay, -bx
    sigma = np.full((T, 9), np.nan, dtype)
    H[:] = np.nan
    ok = np.isfinite(A).all(axis=(1, 2))
    if ok.any():
        _, sv, Vh = np.linalg.svd(A[ok], full_matrices=True)
        sigma[ok, :8] = sv
        sigma[ok, 8] = 0                                               # 8 equations, 9 unknowns: the structural zero
        Hn = Vh[:, 8, :].reshape(-1, 3, 3)
        H[ok] = np.matmul(np.matmul(Tdi[ok], Hn), Ts[ok])
    return H, sigma


def fit64(model, sx, sy, dx, dy):
    """The model through the sample's correspondences in float64. model 0/1/2 = translation/similarity/homography with
    1/2/4 correspondences. Returns (H (T, 3, 3), sigma (T, k)): sigma are the singular values, descending, of the sample's
    float64 design matrix on Hartley-normalised points, closed by the structural zero of the null direction, so
    sigma[-2] / sigma[0] tells a well-posed sample from a degenerate one for every model (a translation's is 1).
    A sample that cannot be normalised (all source or all destination points coincide) gives NaN sigma."""
    return _fit(model, sx, sy, dx, dy, np.float64)


def fit_lapack32(model, sx, sy, dx, dy):
    """fit64's text in float32 working precision (numpy.linalg.svd on a float32 matrix is LAPACK's sgesdd): an independent
    implementation with the product's number format, the yardstick for what float32 rounding alone costs."""
    return _fit(model, sx, sy, dx, dy, np.float32)


def conditioning(sigma):
    """sigma[0] / sigma[-2] per sample (inf for a degenerate one, NaN sigma included)."""
    sigma = np.asarray(sigma, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = sigma[..., 0] / sigma[..., -2]
    return np.where(np.isfinite(k), k, np.inf)


def _maps(H):
    H = np.asarray(H, np.float64)
    if H.shape[-1] == 9:
        H = H.reshape(H.shape[:-1] + (3, 3))
    return H[None] if H.ndim == 2 else H


def backward_error64(H, sample):
    """Largest distance in pixels between H, applied in float64 to the sample's source points, and the sample's destination
    points. H: (T, 9) or (T, 3, 3) of any float type, taken as exact; sample = (sx, sy, dx, dy), each (T, ns). NaN where the
    map or a point is not finite or a sample point maps to infinity."""
    M = _maps(H)
    sx, sy, dx, dy = (_as2d(a, np.float64) for a in sample)
    px, py = _apply(M, sx, sy)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.sqrt((px - dx) ** 2 + (py - dy) ** 2).max(axis=1)
    return np.where(np.isfinite(e), e, np.nan)


def corners(W, Hh):
    return np.array([0.0, W, 0.0, W]), np.array([0.0, 0.0, Hh, Hh])


def corner_distance64(Ha, Hb, W, Hh):
    """Largest distance in pixels between where two sets of maps send the four frame corners, in float64 (NaN if undefined).
    Either side may be a single map."""
    cx, cy = corners(W, Hh)
    A, B = _maps(Ha), _maps(Hb)
    ax, ay = _apply(A, np.tile(cx, (len(A), 1)), np.tile(cy, (len(A), 1)))
    bx, by = _apply(B, np.tile(cx, (len(B), 1)), np.tile(cy, (len(B), 1)))
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.sqrt((ax - bx) ** 2 + (ay - by) ** 2).max(axis=1)
    return np.where(np.isfinite(e), e, np.nan)


# ------------------------------------------------------------------------------------------------- inlier bracket
def _gamma(k):
    return k * U32 / (1.0 - k * U32)


def inlier_bracket64(H, sx, sy, dx, dy, thr):
    """(lo, hi, d2, band) for float32 maps H (T, 9), taken as exact, over float32 point lists: any correct float32 evaluation
    of the product's inlier test counts, per hypothesis, within [lo[t], hi[t]]. d2 (T, n) is the squared reprojection
    distance in float64 and band its error bound. Rows with sx < 0 or NaN sx count in neither (the product's validity rule).

    The test is `d < thr` with d the float32 result of the fixed sequence

        X = fl(fl(fma(H0, sx, fl(H1 * sy))) + H2)       (likewise Y with H3..H5 and Z with H6..H8)
        x = fl(X / Z),  y = fl(Y / Z)
        ex = fl(dx - x),  ey = fl(dy - y)
        d = fl(fma(ex, ex, fl(ey * ey)))

    Each fl() is one IEEE rounding: fl(a) = a (1 + delta) + eta, |delta| <= u = 2^-24, |eta| <= 2^-149 (underflow only).
    With g_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1), hats for computed values:

      * the sum passes H1 sy through 3 roundings, H0 sx through 2, H2 through 1, so
            |X^ - X| <= eX := g_3 (|H0 sx| + |H1 sy| + |H2|) + 3 eta         (same for eY, eZ);
      * X^/Z^ - X/Z = (X^ - X)/Z^ + (X/Z)(Z - Z^)/Z^ and |Z^| >= |Z| - eZ, so, when |Z| > eZ,
            |X^/Z^ - x| <= q := (eX + |x| eZ) / (|Z| - eZ),     and the divide's own rounding adds u (|x| + q) + eta:
            |x^ - x| <= Ex := q + u (|x| + q) + eta;
        when |Z| <= eZ the sign of Z^ is not determined and the point is undecided (band = inf);
      * |ex^ - (dx - x)| <= Dx := Ex + u (|dx - x| + Ex)                       (a subtraction cannot underflow);
      * ex^2 differs from (dx - x)^2 by at most 2 |dx - x| Dx + Dx^2; call the sum of that and its y twin A. The product and
        the fma add two roundings to terms that are all non-negative:
            |d - d2| <= band := A + g_2 (d2 + A) + 2 eta.

    Nothing is measured: the bound follows from the sequence and the format alone. A point counts in lo when
    d2 + band < thr, in hi when d2 - band < thr or when d2 or band is not finite. thr is rounded to float32 first, as the
    kernel receives it."""
    M = _maps(H)
    sx32 = np.asarray(sx, np.float32)
    sx, sy, dx, dy = (np.asarray(a, np.float64)[None, :] for a in (sx, sy, dx, dy))
    thr = float(np.float32(thr))
    valid = sx32 >= np.float32(0)                                      # False for NaN
    h = lambda i, j: M[:, i, j, None]
    g3, g2 = _gamma(3), _gamma(2)
    with np.errstate(all="ignore"):
        X = h(0, 0) * sx + h(0, 1) * sy + h(0, 2)
        Y = h(1, 0) * sx + h(1, 1) * sy + h(1, 2)
        Z = h(2, 0) * sx + h(2, 1) * sy + h(2, 2)
        eX = g3 * (np.abs(h(0, 0) * sx) + np.abs(h(0, 1) * sy) + np.abs(h(0, 2))) + 3 * ETA32
        eY = g3 * (np.abs(h(1, 0) * sx) + np.abs(h(1, 1) * sy) + np.abs(h(1, 2))) + 3 * ETA32
        eZ = g3 * (np.abs(h(2, 0) * sx) + np.abs(h(2, 1) * sy) + np.abs(h(2, 2))) + 3 * ETA32
        x, y = X / Z, Y / Z
        den = np.abs(Z) - eZ
        qx = np.where(den > 0, (eX + np.abs(x) * eZ) / den, np.inf)
        qy = np.where(den > 0, (eY + np.abs(y) * eZ) / den, np.inf)
        Ex = qx + U32 * (np.abs(x) + qx) + ETA32
        Ey = qy + U32 * (np.abs(y) + qy) + ETA32
        rx, ry = dx - x, dy - y
        Dx = Ex + U32 * (np.abs(rx) + Ex)
        Dy = Ey + U32 * (np.abs(ry) + Ey)
        d2 = rx * rx + ry * ry
        A = 2 * np.abs(rx) * Dx + Dx * Dx + 2 * np.abs(ry) * Dy + Dy * Dy
        band = A + g2 * (d2 + A) + 2 * ETA32
        loose = ~np.isfinite(d2) | ~np.isfinite(band)
        in_lo = valid[None, :] & ~loose & (d2 + band < thr)
        in_hi = valid[None, :] & (loose | (d2 - band < thr))
    return in_lo.sum(axis=1), in_hi.sum(axis=1), d2, band


def undecided_share(lo, hi, valid_points):
    """sum(hi - lo) / (hypotheses * valid points): the share of (hypothesis, point) pairs the bracket leaves open."""
    return float(np.sum(hi - lo)) / max(1, len(lo) * int(valid_points))


# --------------------------------------------------------------------------------------------------------- scenes
MOTIONS = ("mild", "perspective", "rot90", "rot180", "scale025", "scale4", "negative")
FRAMES = ((640, 480), (1920, 1080), (3840, 2160), (7680, 4320))


def motion_matrix(model, W, Hh, motion):
    """The true float64 map of a named motion on a W x Hh frame, restricted to what `model` can express: model 0 keeps the
    translation, model 1 the similarity, model 2 everything. Perspective terms scale with 1920 / W so that z stays in
    [0.4, 1.3] over the frame at every size (|h31| = 3e-4, |h32| = 2e-4 at 1080p)."""
    f = W / 1920.0
    cx, cy = W / 2.0, Hh / 2.0

    def about_centre(A, tx, ty):                                       # x' = A (x - c) + c + t
        M = np.eye(3)
        M[:2, :2] = A
        M[:2, 2] = np.array([cx, cy]) - A @ np.array([cx, cy]) + np.array([tx, ty])
        return M

    rot = lambda deg, s=1.0: s * np.array([[np.cos(np.deg2rad(deg)), -np.sin(np.deg2rad(deg))],
                                            [np.sin(np.deg2rad(deg)), np.cos(np.deg2rad(deg))]])
    if motion == "mild":
        M = about_centre(rot(5.0, 1.02), 12.0 * f, -7.0 * f)
        M[2, :2] = [1e-5 / f, -2e-5 / f]
    elif motion == "perspective":
        M = about_centre(rot(3.0, 1.05), 30.5 * f, 11.25 * f)
        M[2, :2] = [-3e-4 / f, 2e-4 / f]
    elif motion == "rot90":
        M = about_centre(rot(90.0), 5.5 * f, -3.25 * f)
    elif motion == "rot180":
        M = about_centre(rot(180.0), -8.0 * f, 6.5 * f)
    elif motion == "scale025":
        M = np.diag([0.25, 0.25, 1.0]); M[:2, 2] = [40.0 * f, 25.0 * f]
    elif motion == "scale4":
        M = np.diag([4.0, 4.0, 1.0]); M[:2, 2] = [-100.0 * f, 60.0 * f]
    elif motion == "negative":
        M = about_centre(rot(-4.0, 0.97), -1.5 * W, -0.7 * Hh)          # most destinations have negative coordinates
    else:
        raise ValueError(motion)
    if model <= 1:
        M[2, :2] = 0
    if model == 0:
        M[:2, :2] = np.eye(2)
    return M


def apply64(M, x, y):
    """One 3x3 map on float64 points."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    Z = M[2, 0] * x + M[2, 1] * y + M[2, 2]
    return (M[0, 0] * x + M[0, 1] * y + M[0, 2]) / Z, (M[1, 0] * x + M[1, 1] * y + M[1, 2]) / Z


def scene(model, W, Hh, n, outlier_share, noise_px, seed, motion, unmatched=()):
    """n correspondences on a W x Hh frame: float32 sources uniform over the frame, destinations = true map applied in
    float64 (+ Gaussian noise of noise_px per axis) rounded once to float32; a share of rows gets a destination uniform
    over the bounding box of the true destinations instead. Rows listed in `unmatched` hold -1 in all four arrays (what
    align_points writes for an unmatched row). A negative destination is valid; only a negative source x is not.
    Returns a dict: sx, sy, dx, dy (float32), M (3x3 float64), inlier (bool mask of rows that follow M), W, H."""
    rng = np.random.default_rng(seed)
    M = motion_matrix(model, W, Hh, motion)
    sx = rng.uniform(0, W, n).astype(np.float32)
    sy = rng.uniform(0, Hh, n).astype(np.float32)
    tx, ty = apply64(M, sx, sy)
    bx, by = apply64(M, *corners(W, Hh))
    if noise_px:
        tx = tx + rng.normal(0, noise_px, n)
        ty = ty + rng.normal(0, noise_px, n)
    dx, dy = tx.astype(np.float32), ty.astype(np.float32)
    inlier = np.ones(n, bool)
    k = int(round(outlier_share * n))
    if k:
        out = rng.choice(n, k, replace=False)
        dx[out] = rng.uniform(bx.min(), bx.max(), k).astype(np.float32)
        dy[out] = rng.uniform(by.min(), by.max(), k).astype(np.float32)
        inlier[out] = False
    for r in unmatched:
        sx[r] = sy[r] = dx[r] = dy[r] = -1
        inlier[r] = False
    return dict(sx=sx, sy=sy, dx=dx, dy=dy, M=M, inlier=inlier, W=W, H=Hh)


def sample_lists(n, iterations, model, seed, rows=None):
    """(iterations, samples) int32 indices, uniform over `rows` (default all n)."""
    rng = np.random.default_rng(seed)
    S = SAMPLES[model]
    if rows is None:
        return rng.integers(0, n, (iterations, S)).astype(np.int32)
    rows = np.asarray(rows)
    return rows[rng.integers(0, len(rows), (iterations, S))].astype(np.int32)


def skipped(rl):
    """Hypotheses whose sample repeats an index (the product skips them: zero map, count 0)."""
    s = np.sort(np.asarray(rl), axis=1)
    return (s[:, 1:] == s[:, :-1]).any(axis=1) if s.shape[1] > 1 else np.zeros(len(s), bool)


def gather(sc, rl):
    """The sample's coordinates: four (iterations, samples) arrays."""
    return tuple(sc[k][rl] for k in ("sx", "sy", "dx", "dy"))


def iterations_for(inlier_share, samples, miss=1e-9):
    """Hypotheses needed so that an all-inlier sample is drawn with probability above 1 - miss (draws with replacement)."""
    p = inlier_share ** samples
    if p >= 1.0:
        return 1
    return int(np.ceil(np.log(miss) / np.log1p(-p)))


def z_spread64(H, sx, sy, W, Hh):
    """min z / max z of the maps' third coordinate over the sample's source points and the four frame corners (0 when the
    signs differ or a value is not finite): how far the map keeps those points from its horizon line."""
    M = _maps(H)
    sx, sy = _as2d(sx, np.float64), _as2d(sy, np.float64)
    cx, cy = corners(W, Hh)
    x = np.concatenate([sx, np.tile(cx, (len(M), 1))], axis=1)
    y = np.concatenate([sy, np.tile(cy, (len(M), 1))], axis=1)
    with np.errstate(all="ignore"):
        Z = M[:, 2, 0, None] * x + M[:, 2, 1, None] * y + M[:, 2, 2, None]
        Z = Z * np.sign(Z[:, :1])
        r = Z.min(axis=1) / Z.max(axis=1)
    return np.where(np.isfinite(r) & (r > 0), r, 0.0)


# ------------------------------------------------------------------------------------- the sweep and its limits
SWEEP_POINTS, SWEEP_HYPOTHESES, SWEEP_THR, SWEEP_NOISE, SWEEP_OUTLIERS = 1500, 400, 4.0, 0.7, 0.4


def sweep(model, W, Hh):
    """One scene and sample list per motion: half the samples drawn from all rows (40 % outliers: wild fits), half from
    the rows that follow the true map. Yields (motion, scene, rand_list)."""
    for mi, motion in enumerate(MOTIONS):
        sc = scene(model, W, Hh, SWEEP_POINTS, SWEEP_OUTLIERS, SWEEP_NOISE, 1000 * model + 10 * mi + W, motion)
        half = SWEEP_HYPOTHESES // 2
        rl = np.concatenate([sample_lists(SWEEP_POINTS, half, model, 77 + mi),
                             sample_lists(SWEEP_POINTS, SWEEP_HYPOTHESES - half, model, 177 + mi,
                                          rows=np.flatnonzero(sc["inlier"]))])
        yield motion, sc, rl


def fit_errors(model, Hyp, sc, rl):
    """(backward error over the well-posed samples, forward corner error / conditioning over the resolvable ones) of the
    hypotheses Hyp (T, 9) against the float64 reference; selection by the float64 side alone. Skipped samples excluded."""
    smp = gather(sc, rl)
    H64, sig = fit64(model, *smp)
    kappa = conditioning(sig)
    keep = ~skipped(rl) & (z_spread64(H64, smp[0], smp[1], sc["W"], sc["H"]) >= HORIZON)
    well = keep & (1.0 / kappa >= WELL_POSED)
    res = keep & (1.0 / kappa >= RESOLVABLE)
    bwd = backward_error64(Hyp, smp)[well]
    fwd = (corner_distance64(Hyp, H64, sc["W"], sc["H"]) / kappa)[res]
    return bwd, fwd


#: Maxima of fit_lapack32 over sweep(model, W, H), in pixels: (backward, forward / conditioning). Measured once with
#: numpy 2 / OpenBLAS; tests/test_ransac_float64.py prints this machine's figures next to them.
LAPACK32_MAX = {
    (0, 640, 480): (6.82e-05, 6.82e-05), (0, 1920, 1080): (2.46e-04, 2.46e-04),
    (0, 3840, 2160): (2.73e-04, 2.73e-04), (0, 7680, 4320): (5.46e-04, 5.46e-04),
    (1, 640, 480): (1.30e-03, 9.60e-04), (1, 1920, 1080): (3.05e-03, 3.46e-03),
    (1, 3840, 2160): (1.04e-02, 1.20e-02), (1, 7680, 4320): (1.09e-02, 1.30e-02),
    (2, 640, 480): (4.65e-04, 1.83e-03), (2, 1920, 1080): (1.32e-03, 4.26e-03),
    (2, 3840, 2160): (2.82e-03, 1.40e-02), (2, 7680, 4320): (5.79e-03, 2.08e-02),
}
LIMIT_FACTOR = 8.0


def limits(model, W, Hh):
    """(backward, forward / conditioning) limits in pixels: 8 x the float32 LAPACK maxima."""
    b, f = LAPACK32_MAX[(model, W, Hh)]
    return LIMIT_FACTOR * b, LIMIT_FACTOR * f


# ------------------------------------------------------------------------- properties of one call, and the catalogue
def bracket_counts(Hyp, pts, thr, chunk_pairs=2_000_000):
    """inlier_bracket64's (lo, hi), computed in slices of hypotheses so that large calls fit in memory."""
    n = max(1, len(pts[0]))
    step = max(1, chunk_pairs // n)
    lo, hi = [], []
    for a in range(0, len(Hyp), step):
        l, h, _, _ = inlier_bracket64(Hyp[a:a + step], *pts, thr)
        lo.append(l); hi.append(h)
    return np.concatenate(lo), np.concatenate(hi)


def check_call(model, pts, rl, thr, result, label="", max_pairs=12_000_000, always=()):
    """Everything a RANSAC call must satisfy whatever its arithmetic, for result = (position, H_best (9,), homographies
    (T, 9), inliers (T,)) as numpy values: a repeated index gives a zero map and count 0; a map with a non-finite entry
    counts 0; a finite map counts within the float64 bracket; position is the first index of the maximum count; H_best is
    homographies[position] bit for bit and is non-finite only when the best count is 0; thr <= 0 leaves every count 0.
    Where hypotheses x points exceeds max_pairs the bracket is evaluated on an even stride of the hypotheses, plus the
    winner and those listed in `always`; every other rule still covers all of them."""
    pos, Hb, Ha, inl = result
    pos, Hb, Ha, inl = int(pos), np.asarray(Hb, np.float32).reshape(9), np.asarray(Ha, np.float32), np.asarray(inl)
    sx, sy, dx, dy = pts
    skip = skipped(rl)
    finite = np.isfinite(Ha).all(axis=1)
    assert not Ha[skip].any() and not inl[skip].any(), label + ": a skipped hypothesis holds a map or a count"
    assert not inl[~finite].any(), label + ": a non-finite hypothesis counts inliers"
    use = finite & ~skip
    if len(inl) * len(sx) > max_pairs:
        pick = np.zeros(len(inl), bool)
        pick[::int(np.ceil(len(inl) * len(sx) / max_pairs))] = True
        pick[[pos] + [int(a) for a in always]] = True
        use &= pick
    if use.any():
        lo, hi = bracket_counts(Ha[use], pts, thr)
        got = inl[use]
        bad = np.flatnonzero((got < lo) | (got > hi))
        assert len(bad) == 0, "%s: %d counts outside the float64 bracket, first: hypothesis %d counts %d, bracket [%d, %d]" % (
            label, len(bad), np.flatnonzero(use)[bad[0]], got[bad[0]], lo[bad[0]], hi[bad[0]])
    assert (inl >= 0).all() and pos == int(np.argmax(inl)), label + ": position %d is not the first maximum %d" % (pos, int(np.argmax(inl)))
    assert np.array_equal(np.ascontiguousarray(Hb).view(np.uint32), np.ascontiguousarray(Ha[pos]).view(np.uint32)), \
        label + ": H_best is not homographies[position]"
    assert np.isfinite(Hb).all() or inl[pos] == 0, label + ": non-finite H_best with a positive count"
    if not float(np.float32(thr)) > 0:
        assert not inl.any() and pos == 0, label + ": thr <= 0 must count nothing"


HORIZON_MAP = np.array([[1.0, 0, 0], [0, 1.0, 0], [-1 / 1500.0, -1 / 1500.0, 1.0]])   # horizon line x + y = 1500


def catalogue(model):
    """Hand-built degenerate inputs: a list of (name, points, rand_list, thr, base), where points = (sx, sy, dx, dy),
    rand_list interleaves the case's hand-built samples with `base` well-posed ones, and base indexes the well-posed
    hypotheses in rand_list. Every case shares the same well-posed samples, and all cases except the non-finite-coordinate
    ones share one point list, so the well-posed hypotheses must come out bit-identical across them.
    No index is out of range; non-finite coordinates sit at rows that no sample touches. The second value is a sample list
    of hypotheses that are all unusable (non-finite fit or repeated index), a non-finite one first; empty for model 0."""
    S = SAMPLES[model]
    sc = scene(model, 1920, 1080, 200, 0.3, 0.0, 4242 + model, "mild")
    good = sample_lists(200, 24, model, 5, rows=np.flatnonzero(sc["inlier"]))
    good = good[~skipped(good)]
    xy = lambda *p: np.array(p, np.float64)
    # extra rows, appended after the scene's 200: (sx, sy, dx, dy)
    extra = [
        (300, 400, 10, 20), (300, 400, 700, 90), (300, 400, 35, 800), (300, 400, 900, 900),       # 200..203 same source
        (100, 50, 640, 360), (900, 70, 640, 360), (80, 700, 640, 360), (1000, 900, 640, 360),     # 204..207 same destination
        (512, 256, 128, 64), (512, 256, 128, 64), (512, 256, 128, 64), (512, 256, 128, 64),       # 208..211 identical rows
        (100, 100, 40, 900), (400, 250, 800, 30), (700, 400, 100, 100), (1300, 700, 900, 1000),   # 212..215 collinear sources
        (250, 900, 333, 444),                                                                     # 216 off that line
    ]
    hs = [(0, 0), (500, 0), (0, 500), (500, 500), (750, 750), (1000, 500), (1000, 1000),          # 217..223: horizon map
          (1500, 1500), (1000, 1500)]                                                             # 224, 225: behind it
    for x, y in hs:
        z = 1 - (x + y) / 1500.0
        extra.append((x, y, x / z, y / z) if z != 0 else (x, y, 5000.0, 5000.0))
    extra.append((1700, 200, 60, 70))                                                             # 226: never sampled
    E = np.array(extra, np.float64)
    with np.errstate(all="ignore"):
        pts = tuple(np.concatenate([sc[k], E[:, i].astype(np.float32)]) for i, k in enumerate(("sx", "sy", "dx", "dy")))
    SPARE = 226
    if model == 2:
        hand = {
            "repeated index": [[5, 9, 5, 11], [7, 7, 7, 7]],
            "coincident sources": [[200, 201, 202, 203], [200, 201, 3, 8]],
            "coincident destinations": [[204, 205, 206, 207], [204, 205, 3, 8]],
            "identical rows": [[208, 209, 210, 211], [208, 209, 3, 8]],
            "three collinear sources": [[212, 213, 214, 216]],
            "four collinear sources": [[212, 213, 214, 215]],
            "point at infinity": [[217, 218, 219, 220]],
            "centroid on the horizon": [[217, 218, 224, 225]],
        }
    elif model == 1:
        hand = {
            "repeated index": [[5, 5]],
            "coincident sources": [[200, 201]],
            "coincident destinations": [[204, 205]],
            "identical rows": [[208, 209]],
        }
    else:
        hand = {"identical rows": [[208], [209]]}

    def interleave(rows):
        rl = [list(g) for g in good]
        for i, r in enumerate(rows):
            rl.insert(min(len(rl), 3 * i + 1), list(r))
        rl = np.array(rl, np.int32)
        base = np.array([i for i, r in enumerate(rl.tolist()) if r in good.tolist() and r not in [list(x) for x in rows]])
        return rl, base

    cases = [("clean", pts, good.copy(), 4.0, np.arange(len(good)))]
    for name, rows in hand.items():
        rl, base = interleave(rows)
        cases.append((name, pts, rl, 4.0, base))
    everything, base = interleave([r for rows in hand.values() for r in rows])
    cases.append(("all together", pts, everything, 4.0, base))
    for ai, an in enumerate(("src_x", "src_y", "dst_x", "dst_y")):
        for v in (np.nan, np.inf, -np.inf):
            q = tuple(a.copy() for a in pts)
            q[ai][SPARE] = v
            cases.append(("%s[%d] = %r" % (an, SPARE, v), q, everything, 4.0, base))
    for thr in (0.0, FLT_MAX, -1.0):
        cases.append(("thr = %r" % thr, pts, everything, thr, base))
    if model == 2:
        dead = [[200, 201, 202, 203], [5, 9, 5, 11], [204, 205, 206, 207], [208, 209, 210, 211], [7, 7, 7, 7]]
    elif model == 1:
        dead = [[200, 201], [5, 5], [204, 205], [208, 209]]
    else:
        dead = []                                                      # one point always gives a translation
    return cases, np.array(dead, np.int32).reshape(len(dead), S)


def assert_recovery(model, sc, rl, thr, result):
    """The two recovery rules for a scene with noise-free inliers. The best count is at least the count the true map itself
    is sure of (its lo bracket, the map rounded to float32): RANSAC must find something at least as good as the answer.
    And H_best sends the frame corners within 2 sqrt(thr) px of the true map: a hypothesis that holds every true inlier
    within the threshold radius sqrt(thr), with inliers spread over the whole frame, cannot leave that radius by more than
    a small factor at the corners; 2 covers the extrapolation. The float64 fit of a clean sample from the same list is
    held to the same rule first, so the rule is known to be attainable before the result is judged by it."""
    pos, Hb, Ha, inl = result
    pts = tuple(sc[k] for k in ("sx", "sy", "dx", "dy"))
    W, Hh, radius = sc["W"], sc["H"], 2.0 * np.sqrt(thr)
    smp = gather(sc, rl)
    H64, sig = fit64(model, *smp)
    clean = np.flatnonzero(sc["inlier"][rl].all(axis=1) & ~skipped(rl) & (1.0 / conditioning(sig) >= 0.05))
    assert len(clean), "no clean well-posed sample in the list"
    ref = corner_distance64(H64[clean[:1]], sc["M"], W, Hh)[0]
    assert ref <= radius, "the float64 reference misses its own rule: %g" % ref
    lo, _, _, _ = inlier_bracket64(sc["M"].astype(np.float32).reshape(1, 9), *pts, thr)
    best = int(np.asarray(inl)[int(pos)])
    got = corner_distance64(np.asarray(Hb, np.float64).reshape(1, 9), sc["M"], W, Hh)[0]
    print("recovery: best count %d (true map is sure of %d), corners off by %.3g px (allowed %.3g, float64 fit %.3g)" % (
        best, lo[0], got, radius, ref))
    assert best >= lo[0], (best, int(lo[0]))
    assert got <= radius, (got, radius)
