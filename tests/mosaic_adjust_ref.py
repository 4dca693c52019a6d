"""References for the global mosaic adjustment (nm_mosaic_adjust_*), in numpy.

sums(): the per-link sums restated from include/nm_abi.h in the written order (512 virtual lanes, the butterfly, the eight
group totals ascending), every product and sum rounded on its own: equal to nm_mosaic_adjust_sums_host_f32 bit for bit.
model_f64(): an independent float64 Levenberg-Marquardt on the same cost, with a dense Jacobian and numpy.linalg.solve; no
virtual lanes, no Cholesky of its own, not written from the library's header.
scene(): the frames, links and noisy matched points the host and GPU tests share.
"""
import numpy as np

F32, F64 = np.float32, np.float64
SUMS, LANES = 153, 512
(END_ITERATIONS, END_CONVERGED, END_UNUSABLE, END_NO_LINK, END_SINGULAR, END_STEP, END_COST_ROSE) = range(7)


def norm(fw, fh):
    return 0.5 * fw, 0.5 * fh, 0.5 * max(fw, fh)


def T_of(fw, fh):
    cx, cy, h = norm(fw, fh)
    return np.array([[1 / h, 0, -cx / h], [0, 1 / h, -cy / h], [0, 0, 1]], F64)


def normalised(G, fw, fh):
    """Gh = T G T^-1 scaled to [8] = 1, for a pixel -> mosaic map G (float64 3 x 3)"""
    T = T_of(fw, fh)
    Gh = T @ np.asarray(G, F64).reshape(3, 3) @ np.linalg.inv(T)
    return (Gh / Gh[2, 2]).reshape(9)


def _has_x(c):
    return (c & 7) < 3 or (c & 7) >= 6


def _has_y(c):
    return (c & 7) >= 3


def sums(src_x, src_y, nA, dst_x, dst_y, matches, fw, fh, Ga, Gb, mask=None, capA=None):
    """(sums float64 (153,), contributing rows) of one link in the library's summation order"""
    capA = len(src_x) if capA is None else capA
    nA = min(max(int(nA), 0), capA)
    cx, cy, h = (F64(v) for v in norm(fw, fh))
    Ga, Gb = np.asarray(Ga, F64).reshape(9), np.asarray(Gb, F64).reshape(9)
    sx, sy = np.asarray(src_x, F32)[:nA], np.asarray(src_y, F32)[:nA]
    mt = np.asarray(matches, np.int32)[:nA]
    ok = (mt >= 0) & (sx >= 0)
    if mask is not None:
        ok &= np.asarray(mask, np.uint8).reshape(-1)[:nA] != 0
    j = np.where(ok, mt, 0)
    dx, dy = np.asarray(dst_x, F32), np.asarray(dst_y, F32)
    with np.errstate(all="ignore"):
        px, py = (sx.astype(F64) - cx) / h, (sy.astype(F64) - cy) / h
        qx = (dx[j].astype(F64) - cx) / h if nA else np.zeros(0)
        qy = (dy[j].astype(F64) - cy) / h if nA else np.zeros(0)
        da = (Ga[6] * px + Ga[7] * py) + Ga[8]
        db = (Gb[6] * qx + Gb[7] * qy) + Gb[8]
        ok &= (da > 0) & np.isfinite(da) & (db > 0) & np.isfinite(db)
        ux, uy = ((Ga[0] * px + Ga[1] * py) + Ga[2]) / da, ((Ga[3] * px + Ga[4] * py) + Ga[5]) / da
        vx, vy = ((Gb[0] * qx + Gb[1] * qy) + Gb[2]) / db, ((Gb[3] * qx + Gb[4] * qy) + Gb[5]) / db
        rx, ry = ux - vx, uy - vy
        z = np.zeros(nA, F64)
        one = np.ones(nA, F64)
        Jx = [px / da, py / da, one / da, z, z, z, (-(ux * px)) / da, (-(ux * py)) / da,
              -(qx / db), -(qy / db), -(one / db), z, z, z, -((-(vx * qx)) / db), -((-(vx * qy)) / db)]
        Jy = [z, z, z, px / da, py / da, one / da, (-(uy * px)) / da, (-(uy * py)) / da,
              z, z, z, -(qx / db), -(qy / db), -(one / db), -((-(vy * qx)) / db), -((-(vy * qy)) / db)]
        terms = []
        for i in range(16):
            for k in range(i, 16):
                x, y = _has_x(i) and _has_x(k), _has_y(i) and _has_y(k)
                if x and y:
                    terms.append(Jx[i] * Jx[k] + Jy[i] * Jy[k])
                elif x or y:
                    terms.append(Jx[i] * Jx[k] if x else Jy[i] * Jy[k])
                else:
                    terms.append(z)
        for i in range(16):
            if _has_x(i) and _has_y(i):
                terms.append(Jx[i] * rx + Jy[i] * ry)
            else:
                terms.append(Jx[i] * rx if _has_x(i) else Jy[i] * ry)
        terms.append(rx * rx + ry * ry)
    Tm = np.where(ok[:, None], np.stack(terms, 1), 0.0) if nA else np.zeros((0, SUMS))
    pad = (-nA) % LANES
    Tm = np.concatenate([Tm, np.zeros((pad, SUMS))]).reshape(-1, LANES, SUMS)
    lane = np.zeros((LANES, SUMS), F64)
    for chunk in Tm:                                     # lane t: rows t, t + 512, .. ascending (a skipped row adds +0)
        lane = lane + chunk
    v = lane.reshape(8, 64, SUMS).copy()
    d = 32
    while d >= 1:
        v[:, :d] = v[:, :d] + v[:, d:2 * d]
        d //= 2
    tot = v[0, 0].copy()
    for w in range(1, 8):
        tot = tot + v[w, 0]
    return tot, int(ok.sum())


# ---- the independent model ----

def _project(G, x, y):
    d = G[6] * x + G[7] * y + G[8]
    return (G[0] * x + G[1] * y + G[2]) / d, (G[3] * x + G[4] * y + G[5]) / d, d


def _block(G, x, y):
    """d pi(G p) / d G[0..7] for points (x, y): two (rows, 8) arrays"""
    u, v, d = _project(G, x, y)
    z, o = np.zeros_like(x), np.ones_like(x)
    return (np.stack([x, y, o, z, z, z, -u * x, -u * y], 1) / d[:, None],
            np.stack([z, z, z, x, y, o, -v * x, -v * y], 1) / d[:, None])


def model_f64(G0, links, fw, fh, anchor=0, rounds=30):
    """Levenberg-Marquardt on sum || pi(G_a p) - pi(G_b q) ||^2 over links = [(a, b, p (rows, 2), q (rows, 2))] in pixels,
    from the maps G0 (n, 3, 3) pixel -> mosaic, the anchor fixed. Works on normalised maps for conditioning only. Returns
    the adjusted maps (n, 3, 3), pixel -> mosaic."""
    n = len(G0)
    T = T_of(fw, fh)
    Ti = np.linalg.inv(T)
    G = np.stack([normalised(g, fw, fh) for g in G0])
    free = [k for k in range(n) if k != anchor]
    col = {k: 8 * i for i, k in enumerate(free)}
    pts = [(a, b, (np.c_[p, np.ones(len(p))] @ T.T)[:, :2], (np.c_[q, np.ones(len(q))] @ T.T)[:, :2]) for a, b, p, q in links]

    def residual(G):
        out = []
        for a, b, p, q in pts:
            ux, uy, _ = _project(G[a], p[:, 0], p[:, 1])
            vx, vy, _ = _project(G[b], q[:, 0], q[:, 1])
            out += [ux - vx, uy - vy]
        return np.concatenate(out)

    lam = 1e-6
    r = residual(G)
    for _ in range(rounds):
        J = np.zeros((r.size, 8 * len(free)))
        at = 0
        for a, b, p, q in pts:
            m = len(p)
            ax, ay = _block(G[a], p[:, 0], p[:, 1])
            bx, by = _block(G[b], q[:, 0], q[:, 1])
            if a != anchor:
                J[at:at + m, col[a]:col[a] + 8] = ax
                J[at + m:at + 2 * m, col[a]:col[a] + 8] = ay
            if b != anchor:
                J[at:at + m, col[b]:col[b] + 8] = -bx
                J[at + m:at + 2 * m, col[b]:col[b] + 8] = -by
            at += 2 * m
        A, g = J.T @ J, J.T @ r
        while True:
            step = np.linalg.solve(A + lam * np.diag(np.diag(A)), g)
            Gn = G.copy()
            for k in free:
                Gn[k, :8] -= step[col[k]:col[k] + 8]
            rn = residual(Gn)
            if rn @ rn <= r @ r:
                break
            lam *= 10
            if lam > 1e6:
                return np.stack([Ti @ g.reshape(3, 3) @ T for g in G])
        small = np.abs(step).max() < 1e-13
        G, r, lam = Gn, rn, max(lam / 10, 1e-12)
        if small:
            break
    return np.stack([Ti @ g.reshape(3, 3) @ T for g in G])


# ---- geometry helpers and the shared scene ----

def corners(fw, fh):
    return np.array([[0, 0], [fw, 0], [fw, fh], [0, fh]], F64)


def apply(G, p):
    q = np.c_[p, np.ones(len(p))] @ np.asarray(G, F64).reshape(3, 3).T
    return q[:, :2] / q[:, 2:]


def corner_error(Gs, Gt, fw, fh):
    """largest corner distance of any frame between two sets of pixel -> mosaic maps"""
    c = corners(fw, fh)
    return max(float(np.linalg.norm(apply(a, c) - apply(b, c), axis=1).max()) for a, b in zip(Gs, Gt))


def footprint_scale(Gs, Gt, fw, fh):
    """per frame, the linear scale of its footprint in the mosaic against the truth: sqrt of the area ratio"""
    def area(g):
        c = apply(g, corners(fw, fh))
        return 0.5 * abs(np.dot(c[:, 0], np.roll(c[:, 1], 1)) - np.dot(c[:, 1], np.roll(c[:, 0], 1)))
    return np.array([np.sqrt(area(a) / area(b)) for a, b in zip(Gs, Gt)])


def chain_to_maps(chain):
    """chain rows M_k (mosaic -> pixel) to G_k = M_k^-1 scaled to [8] = 1"""
    out = []
    for m in np.asarray(chain, F64).reshape(-1, 3, 3):
        g = np.linalg.inv(m)
        out.append(g / g[2, 2])
    return np.stack(out)


def loop_gap(Gs, H_close, fw, fh):
    """the last frame's corners through the chain against through the closing link (last -> 0) and frame 0's map"""
    c = corners(fw, fh)
    return float(np.linalg.norm(apply(Gs[-1], c) - apply(Gs[0], apply(H_close, c)), axis=1).max())


FW, FH = 640, 480


def true_maps(n=12):
    """n frames on a closed path over a plane, slight rotation, scale and perspective; frame 0 is the mosaic's frame"""
    out = []
    for k in range(n):
        a = 2 * np.pi * k / n
        cx, cy = 260 * (np.cos(a) - 1), 200 * np.sin(a)
        th = 0.06 * np.sin(a + 0.4 * k) if k else 0.0
        s = 1 + 0.03 * np.sin(2 * a) if k else 1.0
        G = np.array([[s * np.cos(th), -s * np.sin(th), -cx], [s * np.sin(th), s * np.cos(th), cy], [0, 0, 1]], F64)
        if k:
            G = G @ np.array([[1, 0, 0], [0, 1, 0], [2e-5 * np.sin(a), -1.5e-5 * np.cos(a), 1]], F64)
        out.append(G / G[2, 2])
    return np.stack(out)


def link_points(Ga, Gb, rng, rows, noise, outliers, cap):
    """rows common points of frames a and b from a seeded plane, noisy in both frames, then `outliers` wrong rows; the
    refit-style tables (src_x, src_y, nA, dst_x, dst_y, matches, mask) with capacity cap, dst in shuffled order"""
    c = corners(FW, FH)
    lo = np.maximum(apply(Ga, c).min(0), apply(Gb, c).min(0))
    hi = np.minimum(apply(Ga, c).max(0), apply(Gb, c).max(0))
    p, q = np.zeros((0, 2)), np.zeros((0, 2))
    while len(p) < rows:
        w = lo + (hi - lo) * rng.random((4 * rows, 2))
        a, b = apply(np.linalg.inv(Ga), w), apply(np.linalg.inv(Gb), w)
        keep = ((a >= 0) & (a < [FW, FH]) & (b >= 0) & (b < [FW, FH])).all(1)
        p, q = np.r_[p, a[keep]], np.r_[q, b[keep]]
    p, q = p[:rows] + noise * rng.standard_normal((rows, 2)), q[:rows] + noise * rng.standard_normal((rows, 2))
    p = np.r_[np.abs(p), rng.random((outliers, 2)) * [FW, FH]]
    q = np.r_[q, rng.random((outliers, 2)) * [FW, FH]]
    m = rows + outliers
    assert m <= cap
    perm = rng.permutation(m)
    sx, sy = np.full(cap, -1, F32), np.zeros(cap, F32)
    dx, dy = np.zeros(cap, F32), np.zeros(cap, F32)
    mt = np.full(cap, -1, np.int32)
    sx[:m], sy[:m] = p[:, 0], p[:, 1]
    dx[perm], dy[perm] = q[:, 0].astype(F32), q[:, 1].astype(F32)
    mt[:m] = perm
    mask = np.zeros(cap, np.uint8)
    mask[:rows] = 1
    return sx, sy, m, dx, dy, mt, mask


def scene(n=12, rows=300, noise=0.3, outliers=20, cap=512, seed=5, skips=(1, 2)):
    """The loop: links (k, k + s) for s in skips and the closing (n - 1, 0). Returns (true maps, link_a, link_b, tables) with
    tables = the seven lists of link_points over the links."""
    rng = np.random.default_rng(seed)
    G = true_maps(n)
    la, lb = [], []
    for s in skips:
        for k in range(n - s):
            la.append(k)
            lb.append(k + s)
    la.append(n - 1)
    lb.append(0)
    cols = [[] for _ in range(7)]
    for a, b in zip(la, lb):
        for c, v in zip(cols, link_points(G[a], G[b], rng, rows, noise, outliers, cap)):
            c.append(v)
    return G, la, lb, cols


def inlier_points(tab, l):
    """the unmasked rows of link l as float64 (p, q) pixel arrays, as the library reads them (fp32 values)"""
    sx, sy, m, dx, dy, mt, mask = (c[l] for c in tab)
    i = np.nonzero((mask[:m] != 0) & (mt[:m] >= 0) & (sx[:m] >= 0))[0]
    return np.c_[sx[i], sy[i]].astype(F64), np.c_[dx[mt[i]], dy[mt[i]]].astype(F64)
