"""The two-band mosaic blend (include/nm_abi.h, "Two-band mosaic blend") restated in numpy float64, apart from the C++
functions. TEST INFRASTRUCTURE ONLY. Written from the header's text. The label is decided in exact comparisons on the fp32
weights, as the header says; everything after it is float64 with no prescribed order.

model       labels, blurred planes and the composed colour out_c (float64, before the byte store) of a set of tiles.
winner      the winner-take-all composite (what R = 0 must give exactly).
level_bound the allowance, in byte levels, for the fp32 entry against the model.
scene       random tiles and records for the tests (textures, not flat fields).
e2e_*       the loop-closure views end to end: geometry, float64 tiles, feather mean, Laplacian figures.

The tests hand `model` the taps that nm_mosaic_bands_taps returns, on purpose: the taps are an input of the arithmetic that
the bound is about, and taps() here checks them separately (to one ulp of libm's exp against numpy's).

THE BOUND. u = 2^-24. Labels and taps are the same numbers on both sides, so only the fp32 roundings differ.
  blur      one pass of tap_sum adds R + 1 non-negative terms: term i goes through one rounding of s(-i) + s(i), one of its
            fma and at most R more of the later fmas, so a pass is exact up to a relative (R + 2) u, two passes up to
            e_b = (2 R + 4) u (first order; all terms are >= 0, so relative bounds add).
  l = L/V   two blurred values and one division: relative e_l = 2 e_b + u. l_k is a weighted mean of C, so with
            A = max l_k over the frames valid at the pixel, |dl| <= e_l A.
  d = l_k - l_k*   |d| <= A; two l errors and one rounding: |dd| <= (2 e_l + u) A = e_d A.
  num       m terms fma(M_k, d_k, num), m = frames valid at the pixel: each product is off by M_k A (e_b + e_d), the m
            roundings act on partial sums of at most A sum M: |dnum| <= A sum M (e_b + e_d + m u).
  den       sum of m blurred values >= 0: relative e_b + (m - 1) u.
  q = num/den   |q| <= A:  |dq| <= A (e_b + e_d + m u) + A (e_b + m u) = A (2 e_b + e_d + 2 m u)
  out = C* + q  one rounding: u |out|.
            2 e_b + e_d = 6 e_b + 3 u, so   |d out| <= u ((12 R + 27 + 2 m) A + |out|),
  taken 1 % larger for the second-order terms. The stored byte is trunc(out * 255.9999f) with one more rounding of the
  product y, so in byte levels  B = 255.9999 |d out| + u |y|. A byte may differ from trunc(y_model) by one level only where
  y_model lies within B of an integer. Where a single frame has M > 0 the model's bracket is exactly 0, as the entry's.
"""
import numpy as np

F32 = np.float32
U32 = 2.0 ** -24
SCALE = float(F32(255.9999))
NONE = -1


def taps(R, sigma):
    """g[0..R] as the header writes them: double arithmetic, rounded to fp32"""
    t = np.array([np.exp(-float(i * i) / (2.0 * sigma * sigma)) if i else 1.0 for i in range(R + 1)], np.float64)
    S = 1.0
    for i in range(1, R + 1):
        S += 2.0 * t[i]
    return (t / S).astype(F32)


def records(recs):
    """int32 (n, 16) nm_mosaic_record rows (identity map) from (tx, ty, nw, nh, placed) tuples"""
    out = np.zeros((len(recs), 16), np.int32)
    out[:, :9] = np.tile(np.eye(3, dtype=F32).reshape(9).view(np.int32), (len(recs), 1))
    for k, r in enumerate(recs):
        out[k, 9:14] = r
    return out


def pack(tiles, tile_cap, fill=0.0):
    """(n, tile_cap, 4) float32 workspace of tiles (a list of (nh, nw, 4) arrays or None)"""
    out = np.full((len(tiles), tile_cap, 4), fill, F32)
    for k, t in enumerate(tiles):
        if t is not None:
            out[k, :t.shape[0] * t.shape[1]] = t.reshape(-1, 4)
    return out


def used(rec, tile_cap):
    tx, ty, nw, nh, placed = rec
    return bool(placed) and nw > 0 and nh > 0 and nw * nh <= tile_cap


def _clip(rec, cw, ch):
    """(canvas slices, local slices) of a rectangle's part on the canvas, or None"""
    tx, ty, nw, nh, _ = rec
    x0, y0, x1, y1 = max(tx, 0), max(ty, 0), min(tx + nw, cw), min(ty + nh, ch)
    if x1 <= x0 or y1 <= y0:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 - ty, y1 - ty), slice(x0 - tx, x1 - tx))


def blur(P, g):
    """separable blur of a (nh, nw) float64 plane with zeros outside it"""
    g = np.asarray(g, F32).astype(np.float64)
    R = g.size - 1
    for axis in (1, 0):
        pad = [(0, 0), (0, 0)]
        pad[axis] = (R, R)
        Q = np.pad(P, pad)
        n = P.shape[axis]
        out = np.zeros_like(P)
        for i in range(-R, R + 1):
            sl = [slice(None), slice(None)]
            sl[axis] = slice(R + i, R + i + n)
            out += g[abs(i)] * Q[tuple(sl)]
        P = out
    return P


def labels(tiles, recs, cw, ch, tile_cap, last_tie=False):
    """(label int (ch, cw), NONE where no frame is valid; covered bool). last_tie is a MUTANT: ties to the highest index."""
    label = np.full((ch, cw), NONE, np.int64)
    best = np.zeros((ch, cw), F32)
    covered = np.zeros((ch, cw), bool)
    for k, rec in enumerate(recs):
        c = _clip(rec, cw, ch) if used(rec, tile_cap) else None
        if c is None:
            continue
        cs, ls = c
        w = tiles[k][ls][..., 3]
        covered[cs] = True
        better = (w > 0) & ((label[cs] == NONE) | ((w >= best[cs]) if last_tie else (w > best[cs])))
        label[cs] = np.where(better, k, label[cs])
        best[cs] = np.where(better, w, best[cs])
    return label, covered


def model(tiles, recs, g, cw, ch, tile_cap, no_v=False, m_from_w=False, last_tie=False):
    """The float64 composite. tiles: list of (nh, nw, 4) float32 (C_B, C_G, C_R, w) or None; recs: (tx, ty, nw, nh, placed).
    Returns a dict: out (ch, cw, 3) float64 (nan where unlabelled), label, wstar float32, m (valid frames per pixel), A (max
    l_k per pixel), M_frames (frames with M > 0 per pixel). MUTANTS: no_v (l = L, not L / V), m_from_w (M = g * w instead of
    g * I), last_tie."""
    label, covered = labels(tiles, recs, cw, ch, tile_cap, last_tie)
    lk, Mk, vk = {}, {}, {}
    for k, rec in enumerate(recs):
        if not used(rec, tile_cap):
            continue
        t = tiles[k].astype(np.float64)
        v = tiles[k][..., 3] > 0
        I = np.zeros(v.shape, np.float64)
        c = _clip(rec, cw, ch)
        if c is not None:
            I[c[1]] = label[c[0]] == k
        L = np.stack([blur(np.where(v, t[..., q], 0.0), g) for q in range(3)], axis=-1)
        V = blur(v.astype(np.float64), g)
        Mk[k] = blur(np.where(v, t[..., 3], 0.0), g) if m_from_w else blur(I, g)
        with np.errstate(all="ignore"):
            lk[k] = np.where(v[..., None], L if no_v else L / V[..., None], 0.0)
        vk[k] = v
    lstar = np.zeros((ch, cw, 3))
    Cstar = np.zeros((ch, cw, 3))
    wstar = np.zeros((ch, cw), F32)
    for k in lk:
        c = _clip(recs[k], cw, ch)
        if c is None:
            continue
        cs, ls = c
        mine = label[cs] == k
        lstar[cs] = np.where(mine[..., None], lk[k][ls], lstar[cs])
        Cstar[cs] = np.where(mine[..., None], tiles[k][ls][..., :3].astype(np.float64), Cstar[cs])
        wstar[cs] = np.where(mine, tiles[k][ls][..., 3], wstar[cs])
    num, den = np.zeros((ch, cw, 3)), np.zeros((ch, cw))
    m, A, Mf = np.zeros((ch, cw), int), np.zeros((ch, cw)), np.zeros((ch, cw), int)
    for k in lk:
        c = _clip(recs[k], cw, ch)
        if c is None:
            continue
        cs, ls = c
        on = vk[k][ls] & (label[cs] != NONE)
        num[cs] += np.where(on[..., None], Mk[k][ls][..., None] * (lk[k][ls] - lstar[cs]), 0.0)
        den[cs] += np.where(on, Mk[k][ls], 0.0)
        m[cs] += on
        Mf[cs] += on & (Mk[k][ls] > 0)
        A[cs] = np.maximum(A[cs], np.where(on, lk[k][ls].max(axis=-1), 0.0))
    with np.errstate(all="ignore"):
        out = np.where((label != NONE)[..., None], Cstar + num / den[..., None], np.nan)
    return dict(out=out, label=label, covered=covered, wstar=wstar, m=m, A=A, M_frames=Mf, Cstar=Cstar)


def winner(tiles, recs, cw, ch, tile_cap):
    """(bytes (ch, cw, 3) of the winner's own fp32 sample through the store rule, wstar, label)"""
    label, _ = labels(tiles, recs, cw, ch, tile_cap)
    out = np.zeros((ch, cw, 3), np.uint8)
    wstar = np.zeros((ch, cw), F32)
    for k, rec in enumerate(recs):
        c = _clip(rec, cw, ch) if used(rec, tile_cap) else None
        if c is None:
            continue
        cs, ls = c
        mine = label[cs] == k
        out[cs] = np.where(mine[..., None], store_f32(tiles[k][ls][..., :3]), out[cs])
        wstar[cs] = np.where(mine, tiles[k][ls][..., 3], wstar[cs])
    return out, wstar, label


def store_f32(C):
    """nm_u8_sat(C * 255.9999f) of fp32 values, in fp32"""
    y = (np.asarray(C, F32) * F32(255.9999)).astype(F32)
    with np.errstate(invalid="ignore"):
        return np.where(y >= 0, np.minimum(np.floor(y), 255), 0).astype(np.uint8)


def store_f64(out):
    """(bytes, y) of float64 colours through the store rule"""
    y = np.asarray(out, np.float64) * SCALE
    with np.errstate(invalid="ignore"):
        return np.where(y >= 0, np.minimum(np.floor(y), 255), 0).astype(np.uint8), y


def level_bound(md, R):
    """B (ch, cw, 3) in byte levels, see THE BOUND; 0-extent only where a single frame has M > 0"""
    out = np.nan_to_num(md["out"])
    coef = np.where(md["M_frames"] <= 1, 0.0, 12.0 * R + 27.0 + 2.0 * md["m"]) * md["A"]
    d_out = 1.01 * U32 * (coef[..., None] + np.abs(out))
    return SCALE * d_out + U32 * np.abs(out) * SCALE


def compare(got, md, R):
    """Checks bytes `got` (ch, cw, 3) against the model on labelled pixels. Returns (worst level difference, mismatches that
    the bound does not excuse, share of labelled byte values within the bound of an integer)."""
    lab = md["label"] != NONE
    want, y = store_f64(md["out"])
    B = level_bound(md, R)
    y = np.clip(np.nan_to_num(y), 0.0, 255.5)
    near = np.abs(y - np.round(y)) <= B
    diff = np.abs(got.astype(int) - want.astype(int))
    diff = np.where(lab[..., None], diff, 0)
    bad = (diff > 1) | ((diff == 1) & ~near)
    share = float(near[lab].mean()) if lab.any() else 0.0
    return int(diff.max()), int(bad.sum()), share


def scene(n, fw, fh, cw, ch, seed, tile_cap=None, holes=True, spread=None):
    """n random frames of fw x fh (the first few of other sizes when n allows) scattered over a cw x ch canvas, some partly
    off it. Tiles: C uniform in [0, 1) where valid, a positive smooth weight with its own random scale, invalid holes (w = 0,
    C = 0). Returns (tiles list, recs list, tile_cap)."""
    rng = np.random.default_rng(seed)
    tile_cap = tile_cap or fw * fh
    tiles, recs = [], []
    for k in range(n):
        nw, nh = fw, fh
        tx = int(rng.integers(-fw // 3, cw - 2 * fw // 3)) if spread is None else int(rng.integers(0, spread))
        ty = int(rng.integers(-fh // 3, ch - 2 * fh // 3)) if spread is None else int(rng.integers(0, spread))
        recs.append((tx, ty, nw, nh, 1))
        tiles.append(texture(rng, nw, nh, holes))
    return tiles, recs, tile_cap


def texture(rng, nw, nh, holes=True):
    y, x = np.mgrid[0:nh, 0:nw]
    w = ((1.0 + np.minimum(np.minimum(x, nw - 1 - x), np.minimum(y, nh - 1 - y))) * rng.uniform(0.5, 2.0)).astype(F32)
    w = (w * rng.uniform(0.9, 1.1, (nh, nw))).astype(F32)
    t = np.zeros((nh, nw, 4), F32)
    t[..., :3] = rng.random((nh, nw, 3), dtype=F32)
    t[..., 3] = w
    if holes:
        dead = rng.random((nh, nw)) < 0.03
        t[dead] = 0
    return t


# ---- shared cases of the host and the GPU tests ----------------------------------------------------------------------------
CANVAS = {1: (100, 70), 2: (100, 70), 3: (110, 80), 17: (200, 140), 64: (330, 230)}


def pattern(cw, ch):
    """a patterned canvas and weight plane: what an entry must leave where it writes nothing"""
    y, x = np.mgrid[0:ch, 0:cw]
    canvas = np.stack([(x * 7 + y * 3) % 251, (x * 5 + y * 11) % 241, (x + y * 13) % 239, (x * 3 + y) % 233], axis=-1)
    return canvas.astype(np.uint8), ((x * 31 + y * 17) % 97 + 1000).astype(F32)


def sigma_of(R):
    return max(R, 1) / 2.0


_CASES = {}


def case(n, fw=67, fh=45):
    """(tiles, recs, tile_cap, cw, ch) of the n-frame case; built once, never changed by a test"""
    if (n, fw, fh) in _CASES:
        return _CASES[(n, fw, fh)]
    cw, ch = CANVAS[n]
    tiles, recs, cap = scene(n, fw, fh, cw, ch, seed=100 + n, spread=30 if n <= 3 else None)
    if n == 3:
        recs.append(recs[1][:4] + (0,))         # a fourth record, unplaced, over the second
        tiles.append(tiles[1])
    if n >= 17:                                 # one frame unplaced, one over the cap, one off the canvas, one tiny
        recs[1] = recs[1][:4] + (0,)
        recs[2] = (recs[2][0], recs[2][1], fw + 1, fh, 1)
        tiles[2] = None
        recs[5] = (cw + 3, 10, fw, fh, 1)
        recs[6], tiles[6] = (20, 30, 5, 3, 1), texture(np.random.default_rng(6), 5, 3, holes=False)
    _CASES[(n, fw, fh)] = (tiles, recs, cap, cw, ch)
    return _CASES[(n, fw, fh)]


def run_host(nm, tiles, recs, tile_cap, cw, ch, R, sigma=None, with_wts=True):
    """nm_mosaic_bands_host on a patterned canvas: (canvas, canvas_wts)"""
    canvas, cwts = pattern(cw, ch)
    nm.mosaic_bands_host(canvas, cwts if with_wts else None, pack(tiles, tile_cap, fill=np.nan), records(recs), R=R,
                         sigma=sigma)
    return canvas, cwts


# ---- end to end on the loop-closure views -----------------------------------------------------------------------------------
E2E_R, E2E_SIGMA = 8, 4.0
E2E_PERTURB_PX = 1.5            # corner displacement of every view's map but view 0's; the model shows the ordering at it
E2E_CAP = 520 * 400
E2E_EXPOSURE = dict(stride=4, lo=5, hi=250, min_pixels=64)
_VIEWS = {}


def e2e_views(seed):
    """the K loop-closure views rendered with the float64 sampler, channels scaled by factors in [0.8, 1.25]"""
    import loop_closure_ref as LC
    import warp_ref as WR
    if seed in _VIEWS:
        return _VIEWS[seed]
    tex = WR.Texture(LC.scene(seed))
    x, y = np.meshgrid(np.arange(LC.VW, dtype=np.float64), np.arange(LC.VH, dtype=np.float64))
    t = np.random.default_rng(3).uniform(0.8, 1.25, (LC.K, 3))
    out = []
    for A, tk in zip(LC.view_maps(), t):
        p = LC.apply(A, np.c_[x.reshape(-1), y.reshape(-1)])
        S = WR.sample(tex, p[:, 0], p[:, 1])[0]
        v = np.minimum(np.floor(S * WR.K_U8), 255).reshape(LC.VH, LC.VW, 4)
        v[..., :3] = np.clip(np.rint(v[..., :3] * tk), 0, 255)
        v[..., 3] = 255
        out.append(v.astype(np.uint8))
    _VIEWS[seed] = out
    return out


def _homography(src, dst):
    rows, rhs = [], []
    for (x, y), (u, v) in zip(src, dst):
        rows += [[x, y, 1, 0, 0, 0, -u * x, -u * y], [0, 0, 0, x, y, 1, -v * x, -v * y]]
        rhs += [u, v]
    return np.append(np.linalg.solve(np.array(rows, np.float64), np.array(rhs, np.float64)), 1.0).reshape(3, 3)


def e2e_geometry(px=E2E_PERTURB_PX, seed=1):
    """(link_a, link_b, H float32 (L, 9) true pair maps, chain float32 (K, 9)): the chain maps frame-0 pixels to view-k pixels,
    each view's map but view 0's followed by a homography that moves the view's four corners by px pixels in random directions"""
    import loop_closure_ref as LC
    rng = np.random.default_rng(seed)
    pairs = LC.high_pairs()
    Hs = np.stack([LC.pair_map(a, b).astype(F32).reshape(9) for a, b in pairs])
    A = LC.view_maps()
    corners = np.array([[0, 0], [LC.VW, 0], [LC.VW, LC.VH], [0, LC.VH]], np.float64)
    chain = []
    for k, a in enumerate(A):
        M = np.linalg.inv(a) @ A[0]
        if k:
            ang = rng.uniform(0, 2 * np.pi, 4)
            M = _homography(corners, corners + px * np.c_[np.cos(ang), np.sin(ang)]) @ M
        chain.append(M / M[2, 2])
    return [a for a, _ in pairs], [b for _, b in pairs], Hs, np.stack(chain).astype(F32).reshape(-1, 9)


def e2e_weights():
    import loop_closure_ref as LC
    y, x = np.mgrid[0:LC.VH, 0:LC.VW]
    return ((1 + np.minimum(np.minimum(x, LC.VW - 1 - x), np.minimum(y, LC.VH - 1 - y))) / (LC.VH / 2.0)).astype(F32)


def model_tiles(views, recs16, gains, wts):
    """float64 tiles of the definition (cast to float32 at the end): project, cut, mask of ones, weight, colour times gain"""
    import warp_ref as WR
    fh, fw = views[0].shape[:2]
    tmask, twts = WR.Texture(np.full((fh, fw), 255, np.uint8)), WR.Texture(np.asarray(wts, F32))
    out = []
    for k, v in enumerate(views):
        m = recs16[k, :9].view(F32).astype(np.float64)
        nw, nh = int(recs16[k, 11]), int(recs16[k, 12])
        x, y = np.meshgrid(np.arange(nw, dtype=np.float64), np.arange(nh, dtype=np.float64))
        xp, yp = WR.project(m, x.reshape(-1), y.reshape(-1))
        ok = ~((xp >= fw) | (yp >= fh)) & (WR.sample(tmask, xp, yp)[0][:, 0] > 0.5)
        w = WR.sample(twts, xp, yp)[0][:, 0]
        C = WR.sample(WR.Texture(v), xp, yp)[0][:, :3] * np.asarray(gains[k], F32).astype(np.float64)
        valid = ok & (w > 0)
        t = np.where(valid[:, None], np.c_[C, w], 0.0)
        out.append(t.reshape(nh, nw, 4).astype(F32))
    return out


def feather_f64(tiles, recs, cw, ch, tile_cap):
    """the weighted mean of every valid frame (what the running mean of the feather blend tends to, without its byte steps)"""
    num, den = np.zeros((ch, cw, 3)), np.zeros((ch, cw))
    for k, rec in enumerate(recs):
        c = _clip(rec, cw, ch) if used(rec, tile_cap) else None
        if c is None:
            continue
        t = tiles[k][c[1]].astype(np.float64)
        num[c[0]] += t[..., 3:] * t[..., :3]
        den[c[0]] += t[..., 3]
    with np.errstate(all="ignore"):
        return num / den[..., None]


def laplacian_ms(img, sel):
    """mean over the selected pixels and the channels of (4 p - up - down - left - right)^2, in byte levels squared"""
    p = np.asarray(img, np.float64) * 255.0
    lap = np.zeros_like(p)
    lap[1:-1, 1:-1] = 4 * p[1:-1, 1:-1] - p[:-2, 1:-1] - p[2:, 1:-1] - p[1:-1, :-2] - p[1:-1, 2:]
    return float((lap[sel] ** 2).mean())


def e2e_selection(md):
    """pixels with at least two valid frames whose four neighbours are labelled too"""
    lab = md["label"] != NONE
    inner = np.zeros_like(lab)
    inner[1:-1, 1:-1] = lab[1:-1, 1:-1] & lab[:-2, 1:-1] & lab[2:, 1:-1] & lab[1:-1, :-2] & lab[1:-1, 2:]
    return inner & (md["m"] >= 2)


def e2e_model(nm, seed, px=E2E_PERTURB_PX):
    """The whole path on the CPU: host twins for sums, gains and placement, the float64 model for tiles, bands and feather.
    Returns (dict of the three Laplacian figures, selection, views, geometry, records, gains)."""
    import loop_closure_ref as LC
    views = e2e_views(seed)
    la, lb, Hs, chain = e2e_geometry(px)
    S = nm.mosaic_exposure_sums_host(views, la, lb, Hs, stride=E2E_EXPOSURE["stride"], lo=E2E_EXPOSURE["lo"], hi=E2E_EXPOSURE["hi"])
    gains, _ = nm.mosaic_gains_host(LC.K, la, lb, S, min_pixels=E2E_EXPOSURE["min_pixels"])
    recs16, _ = nm.mosaic_place_host(chain, LC.VW, LC.VH, LC.SCENE_W, LC.SCENE_H, LC.ORIGIN_X, LC.ORIGIN_Y)
    tiles = model_tiles(views, recs16, gains, e2e_weights())
    recs = [tuple(int(v) for v in r[9:14]) for r in recs16]
    md = model(tiles, recs, nm.mosaic_bands_taps(E2E_R, E2E_SIGMA), LC.SCENE_W, LC.SCENE_H, E2E_CAP)
    sel = e2e_selection(md)
    fig = dict(bands=laplacian_ms(np.nan_to_num(md["out"]), sel), single=laplacian_ms(md["Cstar"], sel),
               feather=laplacian_ms(np.nan_to_num(feather_f64(tiles, recs, LC.SCENE_W, LC.SCENE_H, E2E_CAP)), sel))
    return fig, sel, views, (la, lb, Hs, chain), recs16, gains
