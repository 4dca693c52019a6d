"""The median mosaic composite (include/nm_abi.h, "Median mosaic composite") restated in numpy, apart from the C++ functions.
TEST INFRASTRUCTURE ONLY. Written from the header's text. Keys, validity, ranks and inliers are decided exactly: the key in
numpy float32 (three products and two sums, each rounded: the header's own operations), the rank by numpy.lexsort on
(index, key), the inlier test on one float32 subtraction. SELECT is therefore exact. MEAN is float64 with no prescribed order.

model        per canvas pixel: m, the median frame, inliers, support, counts, out (float64), weight.
mean_bound   the allowance for the fp32 entry's MEAN against the model, in byte levels and for the weight.
compare_mean bytes against the model under that allowance.
stack_case   n frames stacked on one rectangle with seeded validity (every depth m up to n occurs at some pixel).
e2e_*        the ten loop-closure views with a painted occluder each, end to end (figures: DESIGN.md section 7).

THE BOUND (MEAN). u = 2^-24. The inlier set is the same on both sides, s frames with weights w_k > 0, W = sum w_k,
A = max |C_k,c| over the inliers and the channels (s <= m, so "m fmas, m - 1 additions, one division" bounds it too).
  num   s fmas from 0: each rounds a partial sum of magnitude at most A W, so |d num| <= s u A W.
  den   s - 1 additions (the first, to 0, is exact) of positive terms: |d den| <= (s - 1) u W.
  q     num / den, one rounding: |d q| <= s u A + (s - 1) u |q| + u |q| <= 2 s u A, as |q| <= A.
  taken 1 % larger for the second-order terms. The stored byte is trunc(q * 255.9999f) with one more rounding of the product
  y, so in byte levels B = 255.9999 |d q| + u |y|: a byte may differ from trunc(y_model) by one level only where y_model lies
  within B of an integer. The weight written is den: |den - W| <= 1.01 (s - 1) u W.
"""
import numpy as np

import bands_ref as B

F32 = np.float32
U32 = 2.0 ** -24
SCALE = B.SCALE
FLT_MAX = float(np.finfo(F32).max)
SELECT, MEAN = 0, 1
DEPTHS = (1, 2, 3, 4, 5, 16, 17, 31, 32, 33, 63, 64)


def key(C):
    """y = (0.07f C_B + 0.72f C_G) + 0.21f C_R of float32 colours (..., 3), in float32"""
    C = np.asarray(C, F32)
    with np.errstate(all="ignore"):
        return (F32(0.07) * C[..., 0] + F32(0.72) * C[..., 1]) + F32(0.21) * C[..., 2]


def stacks(tiles, recs, cw, ch, tile_cap):
    """(samples float32 (n, ch, cw, 4), cover bool (n, ch, cw)) of the used frames' rectangles on the canvas"""
    n = len(recs)
    T, cover = np.zeros((n, ch, cw, 4), F32), np.zeros((n, ch, cw), bool)
    for k, rec in enumerate(recs):
        c = B._clip(rec, cw, ch) if B.used(rec, tile_cap) else None
        if c is not None:
            T[k][c[0]] = tiles[k][c[1]]
            cover[k][c[0]] = True
    return T, cover


def model(tiles, recs, cw, ch, tile_cap, mode=SELECT, w_min=0.0, tau=np.inf, upper=False, high_tie=False, strict=False):
    """The composite as a dict: m, valid (n, ch, cw), label (the median frame, -1 where m == 0), inlier (n, ch, cw), support,
    counts (n, 2), out (ch, cw, 3) float64 and weight float64 (nan where m == 0), A (max |C| over the inliers).
    MUTANTS: upper (the upper median), high_tie (equal keys to the higher index), strict (< tau in the inlier test)."""
    T, cover = stacks(tiles, recs, cw, ch, tile_cap)
    n = len(recs)
    y = key(T[..., :3])
    w = T[..., 3]
    with np.errstate(invalid="ignore"):
        valid = cover & (w > F32(w_min)) & (w <= F32(FLT_MAX)) & np.isfinite(y)
    m = valid.sum(0)
    index = np.broadcast_to(np.arange(n)[:, None, None], valid.shape)
    order = np.lexsort((-index if high_tie else index, np.where(valid, y, F32(0)), ~valid), axis=0)
    rank = np.maximum(m // 2 if upper else (m - 1) // 2, 0)
    label = np.take_along_axis(order, rank[None], 0)[0]
    y_med = np.take_along_axis(y, label[None], 0)[0]
    with np.errstate(all="ignore"):
        d = np.abs((y - y_med[None]).astype(F32))
        inl = valid & ((d < F32(tau)) if strict else (d <= F32(tau)))
    counts = np.stack([valid.sum((1, 2)), (valid & ~inl).sum((1, 2))], axis=1).astype(np.uint64)
    T64 = T.astype(np.float64)
    if mode == SELECT:
        t = np.take_along_axis(T64, label[None, ..., None], 0)[0]
        out, weight = t[..., :3], t[..., 3]
    else:
        wi = np.where(inl, T64[..., 3], 0.0)
        num = (wi[..., None] * np.where(inl[..., None], T64[..., :3], 0.0)).sum(0)
        weight = wi.sum(0)
        with np.errstate(all="ignore"):
            out = num / weight[..., None]
    none = m == 0
    out, weight = np.where(none[..., None], np.nan, out), np.where(none, np.nan, weight)
    A = np.where(inl[..., None], np.abs(T64[..., :3]), 0.0).max((0, 3))
    return dict(m=m, valid=valid, label=np.where(none, -1, label), inlier=inl, support=inl.sum(0), counts=counts, out=out,
                weight=weight, A=A, key=y)


def mean_bound(md):
    """(B in byte levels (ch, cw, 3), allowance of the weight (ch, cw)), see THE BOUND"""
    s = md["support"].astype(np.float64)
    dq = 1.01 * U32 * 2.0 * s * md["A"]
    y = np.abs(np.nan_to_num(md["out"])) * SCALE
    return SCALE * dq[..., None] + U32 * y, 1.01 * U32 * np.maximum(s - 1, 0) * np.nan_to_num(md["weight"])


def compare_mean(got, got_w, md):
    """Bytes `got` (ch, cw, 3) and weights against the MEAN model where m > 0. Returns (worst level difference, mismatches the
    bound does not excuse, share of byte values within the bound of an integer, weights outside their allowance)."""
    on = md["m"] > 0
    want, y = B.store_f64(md["out"])
    Bv, Bw = mean_bound(md)
    y = np.clip(np.nan_to_num(y), 0.0, 255.5)
    near = np.abs(y - np.round(y)) <= Bv
    diff = np.where(on[..., None], np.abs(got.astype(int) - want.astype(int)), 0)
    bad = (diff > 1) | ((diff == 1) & ~near)
    share = float(near[on].mean()) if on.any() else 0.0
    w_bad = on & ~(np.abs(got_w.astype(np.float64) - np.nan_to_num(md["weight"])) <= Bw)
    return int(diff.max()), int(bad.sum()), share, int(w_bad.sum())


def outputs(cw, ch, n):
    """patterned outputs: what an entry must leave where it writes nothing (canvas, weights, support, label, counts)"""
    canvas, cwts = B.pattern(cw, ch)
    return canvas, cwts, canvas[..., 0].copy(), canvas[..., 1].copy(), np.full((n, 2), 12345, np.uint64)


def run_host(nm, tiles, recs, tile_cap, cw, ch, mode, w_min=0.0, tau=np.inf, fill=np.nan):
    """nm_mosaic_median_host on patterned outputs: (canvas, weights, support, label, counts)"""
    out = outputs(cw, ch, len(recs))
    nm.mosaic_median_host(out[0], out[1], B.pack(tiles, tile_cap, fill=fill), B.records(recs), mode=mode, w_min=w_min, tau=tau,
                          support=out[2], label=out[3], counts=out[4])
    return out


def check_exact(got, md, cw, ch, mode):
    """every output of a run against the model: all of them for SELECT; support, label, counts and the untouched pixels for
    MEAN (its bytes and weights go through compare_mean)"""
    canvas, cwts, support, label, counts = got
    pat = outputs(cw, ch, 1)
    on, off = md["m"] > 0, md["m"] == 0
    assert np.array_equal(counts.reshape(-1, 2), md["counts"])
    assert np.array_equal(support[on], md["support"][on]) and np.array_equal(label[on], md["label"][on])
    for g, p in zip((canvas, cwts, support, label), pat):
        assert np.array_equal(g[off], p[off])
    assert (canvas[..., 3][on] == 255).all()
    if mode == SELECT:
        assert np.array_equal(canvas[..., :3][on], B.store_f32(md["out"].astype(F32))[on])
        assert np.array_equal(cwts[on].view(np.uint32), md["weight"][on].astype(F32).view(np.uint32))


_STACKS = {}
STACK_W, STACK_H, STACK_CANVAS = 70, 5, (80, 9)


def stack_case(n):
    """(tiles, recs, tile_cap, cw, ch): n frames on ONE 70 x 5 rectangle (six canvas tiles of the kernel) at (3, 2). The first
    8 columns are valid in every frame (m == n), the last column in none (m == 0), the rest with probability 0.85 per frame;
    invalid samples are w = 0, a NaN colour, an infinite colour or w = inf, in turn. Built once, never changed by a test."""
    if n in _STACKS:
        return _STACKS[n]
    rng = np.random.default_rng(1000 + n)
    tiles = []
    for k in range(n):
        t = B.texture(rng, STACK_W, STACK_H, holes=False)
        dead = rng.random((STACK_H, STACK_W)) >= 0.85
        dead[:, :8], dead[:, -1] = False, True
        kind = rng.integers(0, 4, dead.shape)
        t[dead & (kind == 0), 3] = 0
        t[dead & (kind == 1), 1] = np.nan
        t[dead & (kind == 2), 0] = np.inf
        t[dead & (kind == 3), 3] = np.inf
        tiles.append(t)
    _STACKS[n] = (tiles, [(3, 2, STACK_W, STACK_H, 1)] * n, STACK_W * STACK_H) + STACK_CANVAS
    return _STACKS[n]


def edge_scene():
    """rectangles 63, 64, 65 wide and 3, 4, 5 high, a 1 x 1 one, rectangles hanging off each canvas side and corner, two
    disjoint from the canvas, one unplaced, one over tile_cap, two larger frames under everything"""
    rng = np.random.default_rng(78)
    cw, ch = 300, 120
    recs = [(10, 8, 131, 97, 1), (120, 15, 131, 97, 1)]
    xs = 5
    for nw in (63, 64, 65):
        for j, nh in enumerate((3, 4, 5)):
            recs.append((xs, 20 + 25 * j, nw, nh, 1))
        xs += 70
    recs += [(230, 60, 1, 1, 1), (-20, 30, 67, 45, 1), (cw - 30, 40, 67, 45, 1), (90, -25, 67, 45, 1), (150, ch - 12, 67, 45, 1),
             (-10, -10, 67, 45, 1), (cw - 40, ch - 20, 67, 45, 1), (260, 5, 129, 33, 1), (cw, 10, 67, 45, 1), (20, -45, 67, 45, 1),
             (30, 30, 67, 45, 0), (40, 40, 131, 98, 1)]
    tiles = [B.texture(rng, r[2], r[3], holes=r[2] > 1) if r[2] * r[3] <= 131 * 97 else None for r in recs]
    return tiles, recs, 131 * 97, cw, ch


# ---- end to end on the loop-closure views, each with a painted occluder --------------------------------------------------------
E2E_BLOCK = 48                     # side of the solid block painted into each view
E2E_COLOUR = (255, 0, 255, 255)    # B, G, R, A: saturated magenta, absent from the scene's texture
E2E_TAUS = (0.02, 0.05, 0.1, 0.2)  # the candidates the default tau was chosen from (on the model's figures)
E2E_MIN_DEPTH = 3


def e2e_occluded(views):
    """(views with a block at a view-dependent position, the blocks' masks)"""
    import loop_closure_ref as LC
    out, masks = [], []
    for k, v in enumerate(views):
        x0 = 20 + (k * 37) % (LC.VW - E2E_BLOCK - 40)
        y0 = 15 + (k * 53) % (LC.VH - E2E_BLOCK - 30)
        o, mk = v.copy(), np.zeros(v.shape[:2], np.uint8)
        o[y0:y0 + E2E_BLOCK, x0:x0 + E2E_BLOCK] = E2E_COLOUR
        mk[y0:y0 + E2E_BLOCK, x0:x0 + E2E_BLOCK] = 255
        out.append(o)
        masks.append(mk)
    return out, masks


def mean_abs_levels(canvas_bytes, ref_bytes, sel):
    return float(np.abs(canvas_bytes[sel].astype(np.float64) - ref_bytes[sel].astype(np.float64)).mean())


_E2E = {}


def e2e_model(nm, seed, tau):
    """The whole path on the CPU, as bands_ref.e2e_model builds its own: host twins for sums, gains and placement (on the CLEAN
    views), the float64 sampler for the tiles, the models above for the composites. Returns (figures: mean absolute byte
    difference to the clean-frames feather canvas of feather-with-occluders / SELECT / MEAN over the selection, the selection
    (m >= 3 and an occluded sample valid), the occluded views, geometry, records, gains, the clean feather bytes)."""
    import loop_closure_ref as LC
    import warp_ref as WR
    if (seed, tau) in _E2E:
        return _E2E[(seed, tau)]
    views = B.e2e_views(seed)
    la, lb, Hs, chain = B.e2e_geometry()
    S = nm.mosaic_exposure_sums_host(views, la, lb, Hs, stride=B.E2E_EXPOSURE["stride"], lo=B.E2E_EXPOSURE["lo"],
                                     hi=B.E2E_EXPOSURE["hi"])
    gains, _ = nm.mosaic_gains_host(LC.K, la, lb, S, min_pixels=B.E2E_EXPOSURE["min_pixels"])
    recs16, _ = nm.mosaic_place_host(chain, LC.VW, LC.VH, LC.SCENE_W, LC.SCENE_H, LC.ORIGIN_X, LC.ORIGIN_Y)
    recs = [tuple(int(v) for v in r[9:14]) for r in recs16]
    cw, ch, cap = LC.SCENE_W, LC.SCENE_H, B.E2E_CAP
    occluded, masks = e2e_occluded(views)
    clean_tiles = B.model_tiles(views, recs16, gains, B.e2e_weights())
    tiles = B.model_tiles(occluded, recs16, gains, B.e2e_weights())
    # where a tile pixel saw the block: any of its bilinear taps, i.e. the sampled mask is not 0
    hit = []
    for k, mk in enumerate(masks):
        m9 = recs16[k, :9].view(F32).astype(np.float64)
        nw, nh = recs[k][2], recs[k][3]
        x, y = np.meshgrid(np.arange(nw, dtype=np.float64), np.arange(nh, dtype=np.float64))
        xp, yp = WR.project(m9, x.reshape(-1), y.reshape(-1))
        hit.append((WR.sample(WR.Texture(mk), xp, yp)[0][:, 0] > 0).reshape(nh, nw))
    clean = B.store_f64(np.nan_to_num(B.feather_f64(clean_tiles, recs, cw, ch, cap)))[0]
    feather = B.store_f64(np.nan_to_num(B.feather_f64(tiles, recs, cw, ch, cap)))[0]
    sel_md = model(tiles, recs, cw, ch, cap, SELECT)
    mean_md = model(tiles, recs, cw, ch, cap, MEAN, tau=tau)
    hit_stack = stacks([np.repeat(h[..., None].astype(F32), 4, axis=-1) for h in hit], recs, cw, ch, cap)[0][..., 0] > 0
    sel = (sel_md["m"] >= E2E_MIN_DEPTH) & (hit_stack & sel_md["valid"]).any(0)
    fig = dict(feather=mean_abs_levels(feather, clean, sel),
               select=mean_abs_levels(B.store_f64(np.nan_to_num(sel_md["out"]))[0], clean, sel),
               mean=mean_abs_levels(B.store_f64(np.nan_to_num(mean_md["out"]))[0], clean, sel))
    _E2E[(seed, tau)] = (fig, sel, occluded, (la, lb, Hs, chain), recs16, gains, clean)
    return _E2E[(seed, tau)]
