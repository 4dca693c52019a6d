"""The mosaic exposure compensation (include/nm_abi.h, "Mosaic exposure compensation") restated in numpy, apart from the C++
functions. TEST INFRASTRUCTURE ONLY. Written from the header's text; it imports the projection and the lattice of
tests/link_verify_ref.py (the header says they are the verification's) and the sampler model of tests/warp_ref.py.

sums_int    the seven sums of one link in exact integer arithmetic (int64 arrays, Python ints for the totals).
solve_f64   the gains as numpy.linalg.solve in float64 on the normal equations of the written cost, no prescribed order;
            also the cost itself, so that a test can see that the solution minimises it.
run_blend   the gained blend as warp_ref's interval recurrence with the multiply inserted.

TOLERANCES
  sums      none: integers.
  gains     gain_bound() below. The cost is sum_l N_l [ (g_a abar - g_b bbar)^2 / sn^2 + ((1 - g_a)^2 + (1 - g_b)^2) / sg^2 ].
            Its Hessian is M = D + E: D diagonal with D_kk = sum of N_l / sg^2 over the usable links of frame k, and E the
            positive semi-definite data term. A link adds x^T E x = (N_l / sn^2) (abar x_a - bbar x_b)^2
            <= 2 (255 / sn)^2 N_l (x_a^2 + x_b^2), the means being bytes. With x = D^(-1/2) y the sum over the links is at
            most 2 (255 sg / sn)^2 |y|^2, so the eigenvalues of D^(-1/2) M D^(-1/2) lie in [1, kappa],
                kappa = 1 + 2 (255 sg / sn)^2         (14.005 for the defaults sn = 10, sg = 0.1),
            whatever the links are: the prior bounds the condition number. A frame with no link has the row (1, 1) and
            changes nothing. The error of a Cholesky (or LU) solve does not depend on a diagonal scaling (van der Sluis), so
            a backward stable solve of n unknowns in float64 (Higham, Accuracy and Stability of Numerical Algorithms, th. 10.4)
            has a relative forward error of at most about 4 n (3 n + 1) u kappa, u = 2^-53. The entries carry at most L + 4
            roundings each (a chain of at most L additions of terms of one sign, one division, two products), (L + 4) u
            relative, amplified by kappa as well. For the two solves together, product and numpy:
                |g_dev - g_ref| <= 2 kappa (4 n (3 n + 1) + L + 4) u max|g|     (6e-10 for n = 64, L = 256, defaults, |g| <= 4)
            and the float32 output adds one rounding, 2^-24 |g|, which dominates. Where the clamp acts the clamped reference
            is compared: the clamp is monotone and does not widen the bound.
  blend     warp_ref's bounds (tests/test_warp_float64.py derives them) with the colour interval [r_lo, r_hi] scaled by the
            gain, a non-negative float32 taken exactly, and widened by the ONE extra single-precision rounding of
            r * g: relative 2^-24 on both ends. Nothing else changes: weights, mask and cutoff are those of the ungained model.
"""
import numpy as np

import link_verify_ref as V
import warp_ref as R

F32 = np.float32
U32 = 2.0 ** -24
PER_CHANNEL, COMMON = 0, 1
END_OK, END_NO_LINK, END_SINGULAR = 0, 1, 2


def sums_int(A, B, H, mask=None, stride=4, lo=5, hi=250, a_only=False, counted=None):
    """The seven sums (Python ints) N, Sa_B, Sa_G, Sa_R, Sb_B, Sb_G, Sb_R of one link: A, B uint8 (fh, fw, 4), H maps A
    pixels to B pixels. a_only is a MUTANT: the range test on frame A's bytes only. counted: a list that receives the bool
    array (lh, lw) of the lattice pixels that count (nothing for a non-finite H or an empty lattice)."""
    A, B = np.asarray(A, np.uint8), np.asarray(B, np.uint8)
    fh, fw = A.shape[:2]
    H = np.asarray(H, F32).reshape(9)
    if not np.isfinite(H).all():
        return [0] * 7
    seen = np.ones((fh, fw), bool) if mask is None else (np.asarray(mask, F32) > 0.5)
    x, y = V.lattice(fw, fh, stride)
    if x.size == 0:
        return [0] * 7
    den, xp, yp = V.project32(H, x.astype(F32), y.astype(F32))
    with np.errstate(all="ignore"):
        ok = seen[y, x] & np.isfinite(den) & (den > 0)
        xb, yb = (xp + F32(0.5)) - F32(0.5), (yp + F32(0.5)) - F32(0.5)
        ok &= (xb >= -1) & (xb < F32(fw)) & (yb >= -1) & (yb < F32(fh))          # a NaN fails
        xb, yb = np.where(ok, xb, F32(0)), np.where(ok, yb, F32(0))
        fi, fj = np.floor(xb), np.floor(yb)
        a = np.floor((xb - fi) * F32(256) + F32(0.5)).astype(np.int64)
        b = np.floor((yb - fj) * F32(256) + F32(0.5)).astype(np.int64)
    i, j = fi.astype(np.int64), fj.astype(np.int64)
    ok &= (i >= 0) & (i + 1 < fw) & (j >= 0) & (j + 1 < fh)
    i, j = np.where(ok, i, 0), np.where(ok, j, 0)
    pa = A[y, x, :3].astype(np.int64)
    ok &= ((pa >= lo) & (pa <= hi)).all(axis=1)
    acc = np.full((x.size, 3), 32768, np.int64)
    weights = ((256 - a) * (256 - b), a * (256 - b), (256 - a) * b, a * b)
    assert all(int(v) == 65536 for v in sum(weights))
    for t, w in enumerate(weights):
        ii, jj = np.where(ok, i + (t & 1), 0), np.where(ok, j + (t >> 1), 0)
        pt = B[jj, ii, :3].astype(np.int64)
        ok &= seen[jj, ii]
        if not a_only:
            ok &= ((pt >= lo) & (pt <= hi)).all(axis=1)
        acc += w[:, None] * pt
    pb = acc >> 16
    if counted is not None:
        counted.append(ok.reshape(fh // stride, fw // stride))
    return [int(ok.sum())] + [int(v) for v in pa[ok].sum(axis=0)] + [int(v) for v in pb[ok].sum(axis=0)]


def link_sums(frames, link_a, link_b, H, link_status=None, **kw):
    """(L, 7) Python-int sums of a link list; zeros for a link whose status is not 1"""
    H = np.asarray(H, F32).reshape(-1, 9)
    return [sums_int(frames[a], frames[b], H[l], **kw) if link_status is None or link_status[l] == 1 else [0] * 7
            for l, (a, b) in enumerate(zip(link_a, link_b))]


def _means(s, c, mode):
    N = float(s[0])
    if mode == COMMON:
        return float(s[1] + s[2] + s[3]) / (3.0 * N), float(s[4] + s[5] + s[6]) / (3.0 * N)
    return float(s[1 + c]) / N, float(s[4 + c]) / N


def cost_f64(g, n, link_a, link_b, sums, usable, c, sigma_n, sigma_g, mode=PER_CHANNEL, swap=False, prior=True):
    cost = 0.0
    for l, (a, b) in enumerate(zip(link_a, link_b)):
        if not usable[l]:
            continue
        abar, bbar = _means(sums[l], c, mode)
        if swap:
            abar, bbar = bbar, abar
        N = float(sums[l][0])
        cost += N * (g[a] * abar - g[b] * bbar) ** 2 / sigma_n ** 2
        if prior:
            cost += N * ((1 - g[a]) ** 2 + (1 - g[b]) ** 2) / sigma_g ** 2
    return cost


def solve_f64(n, link_a, link_b, sums, link_status=None, min_pixels=64, sigma_n=10.0, sigma_g=0.1, g_min=0.25, g_max=4.0,
              mode=PER_CHANNEL, swap=False, prior=True):
    """(gains float64 (n, 3) clamped, unclamped (n, 3), stats dict) by numpy.linalg.solve. swap / prior=False are MUTANTS: the
    a and b means exchanged; the prior left out (least squares of the then singular system)."""
    L = len(link_a)
    usable = [(link_status is None or link_status[l] == 1) and sums[l][0] >= min_pixels for l in range(L)]
    deg = np.zeros(n, int)
    for l in range(L):
        if usable[l]:
            deg[link_a[l]] += 1
            deg[link_b[l]] += 1
    g = np.ones((n, 3))
    stats = dict(links=int(sum(usable)), frames=int((deg > 0).sum()), end=END_OK if any(usable) else END_NO_LINK,
                 cost_unit=[0.0] * 3, cost=[0.0] * 3)
    if not any(usable):
        return g.copy(), g, stats
    for c in range(3):
        sys_c = 0 if mode == COMMON else c
        M, r = np.zeros((n, n)), np.zeros(n)
        for l, (a, b) in enumerate(zip(link_a, link_b)):
            if not usable[l]:
                continue
            abar, bbar = _means(sums[l], sys_c, mode)
            if swap:
                abar, bbar = bbar, abar
            N = float(sums[l][0])
            wn, wg = N / sigma_n ** 2, (N / sigma_g ** 2 if prior else 0.0)
            M[a, a] += wn * abar * abar + wg
            M[b, b] += wn * bbar * bbar + wg
            M[a, b] -= wn * abar * bbar
            M[b, a] -= wn * abar * bbar
            r[a] += wg
            r[b] += wg
        for k in range(n):
            if deg[k] == 0:
                M[k, k], r[k] = 1.0, 1.0
        g[:, c] = np.linalg.solve(M, r) if prior else np.linalg.lstsq(M, r, rcond=None)[0]
        stats["cost_unit"][c] = cost_f64(np.ones(n), n, link_a, link_b, sums, usable, sys_c, sigma_n, sigma_g, mode)
        stats["cost"][c] = cost_f64(g[:, c], n, link_a, link_b, sums, usable, sys_c, sigma_n, sigma_g, mode)
    return np.clip(g, g_min, g_max), g, stats


def kappa(sigma_n, sigma_g):
    return 1.0 + 2.0 * (255.0 * sigma_g / sigma_n) ** 2


def gain_bound(g, n, L, sigma_n=10.0, sigma_g=0.1):
    """the allowance for a float32 product gain against the clamped float64 reference g (see TOLERANCES)"""
    g = np.asarray(g, np.float64)
    return np.abs(g) * U32 + 2.0 * kappa(sigma_n, sigma_g) * (4 * n * (3 * n + 1) + L + 4) * 2.0 ** -53 * np.abs(g).max()


def spread(g, t):
    """per channel max_k(g_k t_k) / min_k(g_k t_k) - 1 of corrected exposures; g, t (n, 3)"""
    e = np.asarray(g, np.float64) * np.asarray(t, np.float64)
    return e.max(axis=0) / e.min(axis=0) - 1.0


def run_blend(case, gains):
    """warp_ref's interval recurrence over tests/test_warp_float64's case, frame k's colour interval multiplied by
    gains[k] (float32, >= 0) and widened by the product's one rounding. Returns (BlendState, covered)."""
    import test_warp_float64 as W
    st = R.BlendState(case["canvas"], case["cwts"])
    ch, cw = case["cwts"].shape
    covered = np.zeros((ch, cw), bool)
    texs = {}
    gains = np.asarray(gains, F32).astype(np.float64).reshape(-1, 3)
    assert (gains >= 0).all()
    for k, (frame, mask, wts, mat, tx, ty, nw, nh) in enumerate(case["frames"]):
        for a in (frame, mask, wts):
            if id(a) not in texs:
                texs[id(a)] = R.Texture(a)
        tf, tm, tw = texs[id(frame)], texs[id(mask)], texs[id(wts)]
        x0, x1, y0, y1 = max(0, -tx), min(nw, cw - tx), max(0, -ty), min(nh, ch - ty)
        if x0 >= x1 or y0 >= y1:
            continue
        covered[y0 + ty:y1 + ty, x0 + tx:x1 + tx] = True
        rows_per = max(1, W.CHUNK // (x1 - x0))
        m = R.matrix64(mat)
        for r0 in range(y0, y1, rows_per):
            gx, gy = np.meshgrid(np.arange(x0, x1, dtype=np.float64), np.arange(r0, min(r0 + rows_per, y1), dtype=np.float64))
            gx, gy = gx.reshape(-1), gy.reshape(-1)
            xp, yp = R.project(m, gx, gy)
            dx, dy = W.project_error(m, gx, gy)
            cut = (xp >= tf.w) | (yp >= tf.h)
            und = (np.abs(xp - tf.w) <= dx) | (np.abs(yp - tf.h) <= dy)
            Sm, em, xm = W.model_sample(tm, xp, yp, dx, dy)
            Sm = Sm[:, 0]
            inmask = Sm > 0.5
            und = und | (np.abs(Sm - 0.5) <= em) | (xm & ~cut)
            Sw, ew, xw = W.model_sample(tw, xp, yp, dx, dy)
            Sw = Sw[:, 0]
            Sr, er, xr = W.model_sample(tf, xp, yp, dx, dy)
            er = er[:, None]
            contributes = ~cut & inmask
            und = und | ((xw | xr) & contributes)
            r_lo = np.maximum(Sr[:, :3] - er, 0.0) * gains[k] * (1.0 - U32)
            r_hi = (Sr[:, :3] + er) * gains[k] * (1.0 + U32)
            idx = (gy.astype(np.int64) + ty, gx.astype(np.int64) + tx)
            R.blend_step(st, idx, contributes, und, r_lo, r_hi, Sw - ew, Sw + ew, 6.0 * W.U)
    return st, covered
