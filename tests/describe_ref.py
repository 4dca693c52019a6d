"""Binary64 model of the orientation and descriptor stages (csrc/nm_describe.hip, rows a9/a10), numpy only.

Written from the semantics of the reference kernels -- kernels/orientation.cu:11-129 (smoothing as the race-free loop of
:181-192 intends it) and kernels/descriptor.cu:32-145, mod_2pi_f of kernels/cudamath.h:82-87 -- and from nothing else: no
oracle, no ctypes, no product header. Inputs are the float32 arrays the kernels receive; every operation on them is binary64.
Beside each value the model returns a rounding bound for a float32 evaluation of the same expressions under the fp spec of
DESIGN.md section 2, and the margin of every discrete decision, so that a test can tell "differs by rounding" from "computes
something else". The `mutant` argument switches in one wrong line at a time (tests/test_describe_float64.py shows that every one
of them is caught); None is the model.

Notation: u = 2^-24 (unit roundoff of binary32), fl() one binary32 rounding, RN32 the correctly rounded value.
Quotients by xper are IEEE divisions, so the product's x is RN32(x64) exactly and e_x = |RN32(x64) - x64| (<= u |x|, and 0 for
xper a power of two) is used as it is; likewise e_y, and eps_s = |RN32(s64) - s64| / s64.

ORIENTATION (per keypoint)
  sigma_w = fl(gf s): relative eps_s + u.  3 sigma_w: one more rounding -- the argument of the floor that gives W carries
  (eps_s + 2u) relative.  2 sigma_w^2 = fl(fl(2 sigma_w) sigma_w): 2 eps_s + 3u relative (the doubling is exact).
  dx = fl((float)(cx + xi) - x): e_dx = e_x + u |dx|.  r2 = fma(dx, dx, fl(dy dy)):
      e_r2 = 2 |dx| e_dx + 2 |dy| e_dy + u dy^2 + u r2.
  exponent q = fl(r2 / 2 sigma_w^2): e_q = e_r2 / (2 sigma_w^2) + q (2 eps_s + 4u).
  weight = expf(q), at most 1.5 ulp = 3u relative (tests/test_oracle_math.py): relative e_q + 3u.  vote = fl(mag weight): + u.
  A vote therefore carries a relative error of (c_o + kappa_s) u with the constant c_o = 4 (expf 3, product 1) and the sample's
  conditioning kappa_s = e_q / u (about 6 q <= 45 when xper is a power of two; it grows with |x| / sigma otherwise).
  A bin of n_i non-negative votes, in ANY order: |h - h64_i| <= gamma(n_i - 1) h64_i + sum_votes (c_o + kappa_s) u vote_s, which is
  the issue's (n_i - 1 + c_o) u h64_i with the conditioning carried per sample.  (gamma(k) = k u / (1 - k u).)
  3-tap mean: fl(fl(hm + h0) + hp) is 2u relative on non-negative terms, fl(. / 3) one more: e <- mean3(e) + 3u h_new per pass;
  the mean does not expand e.
  threshold = fl(0.8 max): e_thr = 0.8 max_i e_i + u thr.
  di = -1/2 N / D, N = fl(hp - hm), D = fl(fl(hp + hm) - 2 h0):  e_N = e_p + e_m + u |N|,  e_D = e_p + e_m + 2 e_0 + u (hp + hm) + u |D|.
  With D + e_D < 0 (else the keypoint is fragile):
      |delta di| <= 1/2 (e_N |D| + |N| e_D) / (|D| (|D| - e_D)) + u |di|      -- the first-order sensitivities in hp, hm, h0, made rigorous
  angle = fl(2 pi (fl(i + di) + 0.5) / 36):  e_th = (2 pi / 36) (delta di + u |i + di|) + u th.

DESCRIPTOR (per keypoint; per sample s, per element e)
  SBP = fl(fl(3 s) + 1e-7): eps_S = eps_s + 2u relative; the floor that gives W has the argument sqrt2 SBP 2.5 + 0.5 with that
  relative error.  sinf / cosf of the orientation: 2u ABSOLUTE (tests/test_oracle_math.py).
  nx = fl((ct0 dx + st0 dy) / SBP), the products and the sum in binary64:
      e_nx = (2u (|dx| + |dy|) + |ct0| e_dx + |st0| e_dy) / SBP + |nx| (eps_S + u),   e_ny alike with ct0, st0 exchanged.
  theta = mod_2pi_f(fl(ang - a0)): e_th = u |ang - a0| + u |theta| per wrap.   nt = fl(8 theta / 2 pi): e_nt = 8 e_th / 2 pi + u nt.
  win = fl(exp(fma(nx, nx, fl(ny ny)) / 8)): relative E_w = (2 |nx| e_nx + 2 |ny| e_ny + u ny^2 + u t) / 8 + u.
  A trilinear factor |1 - db - r|, r = fl(n - (bin + 0.5)): ABSOLUTE error e_n + 2u (it is at most 1).
  wt = fl(fl(fl(fl(win mod) ax) ay) at): four roundings.  |delta wt| <= (E_w + 4u) wt + (win mod) (e_ax + e_ay + e_at), so with
      c_s u = E_w + 4u + (e_nx + 2u) + (e_ny + 2u) + (e_nt + 2u)
  |got_e - d64_e| <= gamma(n_e - 1) d64_e + u sum_{s touches e} c_s (mod win)_s                  (1)
  which is the issue's (n_e - 1) u d64_e + c_d u M_e with c_s <= c_d carried per sample.  The ceiling: a voting sample has
  |nx|, |ny| < 2.5, (|dx| + |dy|) / SBP <= sqrt2 |(nx, ny)| <= 5, so for xper a power of two e_nx <= (10 + 5 + 3 * 2.5) u = 22.5 u,
  E_w <= (4 * 2.5 * 22.5 + 2 * 12.5) u / 8 + u = 32.3 u, e_nt <= (8 * (7.3 + 6.3) / 6.28 + 8) u = 25.4 u:
      c_d = 32.3 + 4 + 24.5 + 24.5 + 27.4 = 113   (asserted as a ceiling of every c_s in the CPU test).
  "Touches": the elements of the sample's eight votes, and -- the hat functions being continuous across a cell border -- the cell
  beyond a border that nx - 0.5 or ny - 0.5 lies within 2^-12 of (a float32 evaluation may put a vote of at most (e_n + 2u) mod win
  there).  The temporal border is not treated that way: a sample whose 8 theta / 2 pi is next to an integer makes its keypoint fragile.
  Every first-order term is multiplied by 1.01 for the second-order ones.

FRAGILE keypoints are left out of the value comparison: the model's margin at a discrete step is within the bound of the quantity
compared there -- x + 0.5, y + 0.5 next to an integer (e_x, e_y); 3 sigma_w next to 2..10 or the descriptor's W argument next to an
integer; r2 next to W^2 + 0.6 for a sample with mag > 0; 36 theta / 2 pi (2u relative) or 8 theta / 2 pi (e_nt) next to an integer for
a sample whose vote is not zero; a bin whose peak test can go either way (h0 > thr, h0 > hm, h0 > hp, none of them false beyond
the bound, not all true beyond it) before two certain peaks have been found, or a peak whose D is within e_D of 0.

MEASURED ON THE MODEL (tests/test_describe_float64.py prints them; case A = 96 x 64, xper 1, 300 keypoints):
  median over descriptors of (largest element bound / largest element): 2.0e-05 = 338 u, where the median of a descriptor's largest
    vote count is 128 and of its largest c_s 78: about (n + 2.7 c_s) u, the mass of an element being some eight times its value
    (the mean trilinear factor). The oracle's and the kernels' worst deviation is 0.16 of the bound.
  median angle bound: 9.2e-06 rad = 154 u (about 25 u of a bin after six means, divided by a |D| of a few per cent of h0, times 2 pi / 36).
    Worst deviation 0.13 of the bound.
  fragile share per case, orientation / descriptor (cap 5 %):
    A 96x64 xper 1: 0 / 0      A 96x64 xper 2: 0.33 % / 0      A 61x45 xper 0.5: 0 / 0      B 200x20: 0 / 0      C: 0 / 0
    frame driver, octave 0 of the 320 x 200 frame (207 keypoints): 0.48 % / 0
"""
import numpy as np

U = 2.0 ** -24
TWO_PI = 2.0 * np.pi
F2PI = float(np.float32(TWO_PI))          # cudamath.h:84-85 wraps by (float)(2 * M_PI)
SLACK = 1.01                              # second-order terms
C_O = 4.0
C_D = 113.0
NEAR = 2.0 ** -12                         # "next to a cell border" for the vote mass

ORIENT_MUTANTS = ("ori_exp_minus", "ori_radius_plus1", "ori_five_passes", "ori_threshold_09", "ori_no_half")
DESC_MUTANTS = ("desc_exp_minus", "desc_st0_negated", "desc_all_chunks", "desc_floor_nx", "desc_no_wrap", "desc_slot1")


def _gamma(k):
    k = np.maximum(np.asarray(k, np.float64), 0.0)
    return k * U / (1.0 - k * U)


def _ratio(margin, bound):
    """margin / bound; inf where the bound is 0 (an exact quantity decides the same way on both sides)."""
    margin, bound = np.asarray(margin, np.float64), np.asarray(bound, np.float64)
    out = np.full(np.broadcast(margin, bound).shape, np.inf)
    np.divide(margin, bound, out=out, where=bound > 0)
    return out


def _min(a):
    a = np.asarray(a)
    return float(a.min()) if a.size else np.inf


def _keypoint(kp, xper):
    """x, y, s in binary64, their exact binary32 rounding errors, the truncated pixel and the margin of that truncation."""
    x, y, s = float(kp[0]) / xper, float(kp[1]) / xper, float(kp[2]) / xper
    ex, ey = abs(float(np.float32(x)) - x), abs(float(np.float32(y)) - y)
    eps_s = abs(float(np.float32(s)) - s) / abs(s) if s != 0 else 0.0
    xi, yi = int(np.trunc(x + 0.5)), int(np.trunc(y + 0.5))          # (int)(x + 0.5): truncation (orientation.cu:23-24)
    m_pix = min(_ratio(abs(x + 0.5 - np.rint(x + 0.5)), ex), _ratio(abs(y + 0.5 - np.rint(y + 0.5)), ey))
    return x, y, s, ex, ey, eps_s, xi, yi, float(m_pix)


def orientations64(kpts, grad, ow, oh, gauss_factor, xper, mutant=None):
    """kernels/orientation.cu:11-129. Returns a dict: angles (n,2) (-1 = unset), bound (n,2), processed (n,), fragile (n,),
    hist / mass (n,36) raw bins (the vote mass of a bin is the bin), nvotes (n,36), hist_bound (n,36), W (n,), peak_ratio (n,2) (a
    reported peak's smoothed height over the maximum), margins {name: (n,)}
    (margin / bound of the keypoint's closest decision of that kind; fragile = some ratio <= 1)."""
    assert mutant is None or mutant in ORIENT_MUTANTS
    kpts = np.asarray(kpts, np.float32).reshape(-1, 4)
    g = np.asarray(grad, np.float32).astype(np.float64)
    gf, xper = float(np.float32(gauss_factor)), float(np.float32(xper))
    n = len(kpts)
    angles, bound, peak_ratio = np.full((n, 2), -1.0), np.zeros((n, 2)), np.full((n, 2), np.inf)
    processed = np.zeros(n, bool)
    hist, nvotes, hist_bound = np.zeros((n, 36)), np.zeros((n, 36), np.int64), np.zeros((n, 36))
    Ws = np.zeros(n, np.int64)
    names = ("pixel", "radius", "r2", "bin", "peak")
    margins = {k: np.full(n, np.inf) for k in names}
    for p in range(n):
        if kpts[p, 3] < 0:                                            # :17
            continue
        processed[p] = True
        x, y, s, ex, ey, eps_s, xi, yi, margins["pixel"][p] = _keypoint(kpts[p], xper)
        sigma = gf * s
        a3 = 3.0 * sigma
        W = int(min(10, max(1, np.floor(a3))))                        # :27-30, 22 x 22 threads
        steps = np.arange(2, 11)
        margins["radius"][p] = _min(_ratio(np.abs(a3 - steps), abs(a3) * (eps_s + 2 * U)))
        if mutant == "ori_radius_plus1":
            W += 1
        Ws[p] = W
        xmin, xmax = max(-W, -xi), min(W, ow - 1 - xi)                # :43-46
        ymin, ymax = max(-W, -yi), min(W, oh - 1 - yi)
        if xmin > xmax or ymin > ymax:
            continue
        cy, cx = np.mgrid[ymin:ymax + 1, xmin:xmax + 1]
        smp = g[int(kpts[p, 3]), yi + cy, xi + cx]
        mag, th = smp[..., 0].ravel(), smp[..., 1].ravel()
        dx, dy = (cx + xi - x).ravel(), (cy + yi - y).ravel()
        r2 = dx * dx + dy * dy
        e_r2 = 2 * np.abs(dx) * (ex + U * np.abs(dx)) + 2 * np.abs(dy) * (ey + U * np.abs(dy)) + U * dy * dy + U * r2
        lim = W * W + 0.6                                             # :55
        live = mag != 0
        margins["r2"][p] = _min(_ratio(np.abs(r2 - lim)[live], SLACK * e_r2[live]))
        v = r2 < lim
        mag, th, r2, e_r2 = mag[v], th[v], r2[v], e_r2[v]
        denom = 2.0 * sigma * sigma
        q = r2 / denom
        e_q = e_r2 / denom + q * (2 * eps_s + 4 * U)
        wgt = np.exp(-q if mutant == "ori_exp_minus" else q)          # :56, the sign is the reference's
        qb = 36.0 * th / TWO_PI                                       # :57
        live = mag != 0
        margins["bin"][p] = _min(_ratio(np.abs(qb - np.rint(qb))[live], SLACK * 2 * U * np.abs(qb[live])))
        b = np.floor(qb).astype(np.int64) % 36
        vote = mag * wgt
        h = np.bincount(b, vote, 36)
        nv = np.bincount(b, None, 36)
        e = SLACK * (_gamma(nv - 1) * h + np.bincount(b, vote * (C_O * U + e_q), 36))
        hist[p], nvotes[p], hist_bound[p] = h, nv, e
        for _ in range(5 if mutant == "ori_five_passes" else 6):      # :181-192
            h = (np.roll(h, 1) + h + np.roll(h, -1)) / 3.0
            e = (np.roll(e, 1) + e + np.roll(e, -1)) / 3.0 + SLACK * 3 * U * h
        thr = (0.9 if mutant == "ori_threshold_09" else 0.8) * h.max()     # :96
        e_thr = 0.8 * e.max() + U * thr
        hm, hp, em, ep = np.roll(h, 1), np.roll(h, -1), np.roll(e, 1), np.roll(e, -1)
        gaps = np.stack([h - thr, h - hm, h - hp])                    # :107
        tol = np.stack([e + e_thr, e + em, e + ep])
        sure_no = ((gaps <= 0) & ((-gaps > tol) | (tol == 0))).any(0)
        sure_yes = ((gaps > 0) & ((gaps > tol) | (tol == 0))).all(0)
        found, worst = 0, np.inf
        for i in range(36):                                           # :117-128, bin order, at most two
            if found == 2:
                break
            if sure_no[i]:
                continue
            if not sure_yes[i]:
                worst = 0.0
                break
            worst = min(worst, _min(_ratio(np.abs(gaps[:, i]), tol[:, i])))
            N, D = hp[i] - hm[i], hp[i] + hm[i] - 2 * h[i]
            e_N = ep[i] + em[i] + U * abs(N)
            e_D = ep[i] + em[i] + 2 * e[i] + U * (hp[i] + hm[i]) + U * abs(D)
            if not D + e_D < 0:
                worst = 0.0
                break
            di = -0.5 * N / D                                         # :108
            e_di = SLACK * 0.5 * (e_N * abs(D) + abs(N) * e_D) / (abs(D) * (abs(D) - e_D)) + U * abs(di)
            half = 0.0 if mutant == "ori_no_half" else 0.5
            ang = TWO_PI * (i + di + half) / 36.0                     # :109
            angles[p, found] = ang
            peak_ratio[p, found] = h[i] / h.max()
            bound[p, found] = SLACK * ((TWO_PI / 36.0) * (e_di + U * abs(i + di)) + U * abs(ang))
            found += 1
        margins["peak"][p] = worst
    fragile = processed & (np.stack([margins[k] for k in names]).min(0) <= 1.0)
    return dict(angles=angles, bound=bound, processed=processed, fragile=fragile, hist=hist, mass=hist, nvotes=nvotes,
                hist_bound=hist_bound, W=Ws, margins=margins, peak_ratio=peak_ratio)


def descriptors64(kpts, orients, grad, ow, oh, num_dogs, xper, mutant=None):
    """kernels/descriptor.cu:32-145. Returns a dict: desc (n,128), bound (n,128), x, y (n,) (:75-77), processed (n,) (:49-50),
    fragile (n,), nvotes (n,128), mass (n,128) (sum of mod win over the samples that touch the element), coef (n,) the largest
    c_s of the keypoint, W, chunks (n,), clipped (n,) (window cut by the plane on both sides of an axis), margins {name: (n,)}."""
    assert mutant is None or mutant in DESC_MUTANTS
    kpts = np.asarray(kpts, np.float32).reshape(-1, 4)
    orients = np.asarray(orients, np.float32).reshape(-1, 2).astype(np.float64)
    g = np.asarray(grad, np.float32).astype(np.float64)
    xper = float(np.float32(xper))
    n = len(kpts)
    desc, bound, mass = np.zeros((n, 128)), np.zeros((n, 128)), np.zeros((n, 128))
    nvotes = np.zeros((n, 128), np.int64)
    xs, ys = np.zeros(n), np.zeros(n)
    processed, clipped = np.zeros(n, bool), np.zeros(n, bool)
    coef = np.zeros(n)
    Ws, chunks = np.zeros(n, np.int64), np.zeros(n, np.int64)
    names = ("pixel", "radius", "bin")
    margins = {k: np.full(n, np.inf) for k in names}
    for p in range(n):
        x, y, s, ex, ey, eps_s, xi, yi, m_pix = _keypoint(kpts[p], xper)
        si = int(np.trunc(kpts[p, 3]))
        if xi < 0 or xi >= ow or yi < 0 or yi >= oh or si < 0 or si >= num_dogs:      # :49-50
            continue
        processed[p] = True
        margins["pixel"][p] = m_pix
        xs[p], ys[p] = kpts[p, 0], kpts[p, 1]                          # :75-77
        SBP = 3.0 * s + 1e-7                                           # :54
        eps_S = eps_s + 2 * U
        A = np.sqrt(2.0) * SBP * 5.0 / 2.0 + 0.5                       # :55
        W = int(np.floor(A))
        margins["radius"][p] = float(_ratio(abs(A - np.rint(A)), SLACK * abs(A) * eps_S))
        xmin, xmax = max(-W, -xi), min(W, ow - 1 - xi)                 # :57-60
        ymin, ymax = max(-W, -yi), min(W, oh - 1 - yi)
        Ws[p] = W
        chunks[p] = int(np.ceil((max(xmax - xmin, ymax - ymin) + 1.0) / 16.0))       # :64-65
        clipped[p] = (xmin > -W and xmax < W) or (ymin > -W and ymax < W)
        cy, cx = np.mgrid[ymin:ymax + 1, xmin:xmax + 1]
        cx, cy = cx.ravel(), cy.ravel()
        if mutant != "desc_all_chunks":                                # :86-87,142-143: cx and cy advance together
            d = (cx - xmin) // 16 == (cy - ymin) // 16
            cx, cy = cx[d], cy[d]
        a0 = orients[p, 1 if mutant == "desc_slot1" else 0]            # :89, -1 is used as -1 rad
        st0, ct0 = np.sin(a0), np.cos(a0)                              # :90-91
        if mutant == "desc_st0_negated":
            st0 = -st0
        smp = g[si, yi + cy, xi + cx]
        mod, ang = smp[:, 0], smp[:, 1]                                # :98-99
        raw = ang - a0
        theta, wraps = raw.copy(), np.zeros(len(raw))
        for _ in range(4):                                             # cudamath.h:84-85
            hi, lo = theta > F2PI, theta < 0.0
            theta = np.where(hi, theta - F2PI, np.where(lo, theta + F2PI, theta))
            wraps += hi | lo
        dx, dy = xi + cx - x, yi + cy - y                              # :102-103
        nx = (ct0 * dx + st0 * dy) / SBP                               # :104-105
        ny = (-st0 * dx + ct0 * dy) / SBP
        nt = 8.0 * theta / TWO_PI                                      # :107
        t2 = nx * nx + ny * ny
        win = np.exp((-t2 if mutant == "desc_exp_minus" else t2) / 8.0)     # :108, wsigma = 2
        binx = np.floor(nx if mutant == "desc_floor_nx" else nx - 0.5)      # :110-112
        biny, bint = np.floor(ny - 0.5), np.floor(nt)
        rbx, rby, rbt = nx - (binx + 0.5), ny - (biny + 0.5), nt - bint     # :113-115
        binx, biny, bint = binx.astype(np.int64), biny.astype(np.int64), bint.astype(np.int64)
        # rounding of one sample (module docstring)
        e_dx, e_dy = ex + U * np.abs(dx), ey + U * np.abs(dy)
        lever = 2 * U * (np.abs(dx) + np.abs(dy))
        e_nx = (lever + abs(ct0) * e_dx + abs(st0) * e_dy) / SBP + np.abs(nx) * (eps_S + U)
        e_ny = (lever + abs(st0) * e_dx + abs(ct0) * e_dy) / SBP + np.abs(ny) * (eps_S + U)
        e_nt = 8.0 * (U * np.abs(raw) + wraps * U * np.abs(theta)) / TWO_PI + U * nt
        E_w = (2 * np.abs(nx) * e_nx + 2 * np.abs(ny) * e_ny + U * ny * ny + U * t2) / 8.0 + U
        c_s = (E_w + 4 * U + e_nx + e_ny + e_nt + 6 * U) / U
        wm = win * mod
        val, cnt, cm, ms = np.zeros(128), np.zeros(128), np.zeros(128), np.zeros(128)
        voting = np.zeros(len(cx), bool)
        for ox in (-1, 0, 1, 2):
            for oy in (-1, 0, 1, 2):
                regular = ox in (0, 1) and oy in (0, 1)
                tx = (rbx < NEAR) if ox == -1 else (rbx > 1 - NEAR) if ox == 2 else np.ones(len(cx), bool)
                ty = (rby < NEAR) if oy == -1 else (rby > 1 - NEAR) if oy == 2 else np.ones(len(cx), bool)
                ok = tx & ty & (binx + ox >= -2) & (binx + ox < 2) & (biny + oy >= -2) & (biny + oy < 2)      # :123-126
                if not ok.any():
                    continue
                for dbt in (0, 1):
                    tb = bint + dbt
                    m = ok & (tb < 8) if mutant == "desc_no_wrap" else ok
                    e = ((binx + ox + 2) * 8 + (biny + oy + 2) * 32 + tb % 8)[m]       # :81,134
                    if regular:
                        wt = (wm * np.abs(1.0 - ox - rbx) * np.abs(1.0 - oy - rby) * np.abs(1.0 - dbt - rbt))[m]   # :128-132
                        val += np.bincount(e, wt, 128)
                        voting |= m & (wm != 0)
                    cnt += np.bincount(e, None, 128)
                    cm += np.bincount(e, (wm * c_s)[m], 128)
                    ms += np.bincount(e, wm[m], 128)
        margins["bin"][p] = _min(_ratio(np.abs(nt - np.rint(nt))[voting], SLACK * e_nt[voting]))
        coef[p] = c_s[voting].max() if voting.any() else 0.0
        desc[p], nvotes[p], mass[p] = val, cnt, ms
        bound[p] = SLACK * (_gamma(cnt - 1) * val + U * cm)
    fragile = processed & (np.stack([margins[k] for k in names]).min(0) <= 1.0)
    return dict(desc=desc, bound=bound, x=xs, y=ys, processed=processed, fragile=fragile, nvotes=nvotes, mass=mass, coef=coef,
                W=Ws, chunks=chunks, clipped=clipped, margins=margins)


# ---- comparison of an implementation's float32 outputs with the model (CPU: the oracle; GPU: every kernel family) ----
def orientations_outside(model, got, unset=-1.0):
    """Per keypoint: True where `got` (n,2) float32 is NOT the model's answer within its bound -- a set slot off by more than the
    bound, or an unset slot that does not hold `unset` (the launchers that write both slots leave -1; nm_detect_orientations writes
    found peaks only, so there it is the caller's fill). Only meaningful on processed, non-fragile rows."""
    got = np.asarray(got, np.float64).reshape(-1, 2)
    a, b = model["angles"], model["bound"]
    is_set = a != -1.0
    bad = np.where(is_set, ~(np.abs(got - a) <= b), got != unset)
    return bad.any(1)


def descriptors_outside(model, got):
    """Per keypoint: True where some element of `got` (n,128) float32 differs from the model by more than bound (1)."""
    got = np.asarray(got, np.float64).reshape(-1, 128)
    return (~(np.abs(got - model["desc"]) <= model["bound"])).any(1)


def compared(model):
    """Rows whose values are compared: processed and not fragile."""
    return model["processed"] & ~model["fragile"]


def tile_rows(arr, length):
    """The first `length` rows of `arr` repeated end to end (the long lists of case D: the model runs once per distinct row)."""
    arr = np.asarray(arr)
    reps = -(-length // len(arr))
    return np.concatenate([arr] * reps)[:length]


# ---- the cases of tests/test_describe_float64.py and tests/test_gpu_describe_float64.py (inputs only; planes come from the caller) ----
def case_a_keypoints(grad, ow, oh, xper, seed, n=300, banded=0.65):
    """n random keypoints over the whole plane (borders and corners included), levels 0..2, s / xper log-uniform in [0.25, 12] with
    every orientation radius 1..10 present; orientations random in [0, 2 pi) in BOTH slots, one row in eight -1.
    On blurred noise only one keypoint in twelve has a reported peak between 0.8 and 0.9 of the maximum, so a wrong threshold would
    show on few of them. The list is therefore drawn by rejection: of 13 n random candidates (the last 10 n with s / xper >= 1.3, radius
    6 and up, where such peaks are twice as frequent), the first `banded` n whose MODEL histogram has such a peak are taken, and the
    rest in the order drawn. Nothing but the model decides what is taken."""
    rng = np.random.default_rng(seed)
    m = 13 * n
    x, y = rng.uniform(0.0, ow - 1.0, m), rng.uniform(0.0, oh - 1.0, m)
    x[:8] = [0.0, 0.3, ow - 1.0, ow - 1.3, 0.2, ow - 1.2, ow / 2.0, 0.45]
    y[:8] = [0.0, oh - 1.0, 0.4, oh - 1.0, oh / 2.0, 0.1, oh - 1.1, oh - 1.45]
    s = np.exp(rng.uniform(np.log(0.25), np.log(12.0), m))
    s[3 * n:] = np.exp(rng.uniform(np.log(1.3), np.log(12.0), m - 3 * n))
    s[8:18] = (np.arange(1, 11) + 0.5) / 4.5                # 3 * 1.5 * s = W + 0.5: every orientation radius 1..10
    lvl = rng.integers(0, 3, m)
    cand = np.stack([x * xper, y * xper, s * xper, lvl], 1).astype(np.float32)
    in_band = (orientations64(cand, grad, ow, oh, 1.5, xper)["peak_ratio"] < 0.9).any(1)
    fixed = np.arange(m) < 18
    want = int(banded * n)
    take_band = in_band & ~fixed & (np.cumsum(in_band & ~fixed) <= want)
    rest = ~fixed & ~take_band
    take_rest = rest & (np.cumsum(rest) <= n - 18 - int(take_band.sum()))
    kp = cand[fixed | take_band | take_rest]
    assert len(kp) == n
    ori = rng.uniform(0.0, TWO_PI, (n, 2)).astype(np.float32)
    ori[rng.random(n) < 0.125] = -1.0
    return kp, ori


def case_b_keypoints(ow, oh, xper, seed):
    """Keypoints at xi in {0, 1, ow-2, ow-1} x yi in {0, oh-1}, four scales each, sub-pixel offsets that keep the pixel."""
    rng = np.random.default_rng(seed)
    rows, ori = [], []
    for xi in (0, 1, ow - 2, ow - 1):
        for yi in (0, oh - 1):
            for s in (0.6, 1.3, 2.9, 7.0):
                fx, fy = rng.uniform(-0.3, 0.3, 2)
                rows.append((max(xi + fx, 0.0) * xper, max(yi + fy, 0.0) * xper, s * xper, float(rng.integers(0, 3))))
                ori.append((rng.uniform(0.0, TWO_PI), rng.uniform(0.0, TWO_PI)))
    return np.asarray(rows, np.float32), np.asarray(ori, np.float32)


def case_c_keypoints(grad, ow, oh, xper, seed, num_dogs=3):
    """Ordinary rows interleaved with rows that must not be processed. Returns (kp_orient, kp_desc, ori): the orientation list
    has w = -1 rows (:17 of orientation.cu); the descriptor list has those, levels at and beyond num_dogs (3.9 truncates to 3) and
    pixels outside the plane on every side (descriptor.cu:49-50) -- and x = -0.4, which truncates to pixel 0 and IS processed."""
    kp, ori = case_a_keypoints(grad, ow, oh, xper, seed, n=48, banded=0.0)
    kp_o, kp_d = kp.copy(), kp.copy()
    for i in (3, 11, 12, 30, 47):
        kp_o[i, 3] = kp_d[i, 3] = -1.0
    for i, w in ((5, float(num_dogs)), (20, num_dogs + 2.0), (21, 3.9)):
        kp_d[i, 3] = w
    for i, (x, y) in ((7, (ow + 3.0, 5.0)), (25, (-2.0, 5.0)), (26, (5.0, oh + 0.0)), (40, (ow - 0.5, 5.0)), (41, (5.0, -1.6))):
        kp_d[i, 0], kp_d[i, 1] = x * xper, y * xper
    kp_d[33, 0] = -0.4 * xper
    return kp_o, kp_d, ori
