"""The frame-weights stage (include/nm_abi.h, "Frame masks and feather weights") restated in numpy, apart from the C++
functions. TEST INFRASTRUCTURE ONLY. Written from the header's definition, not from the separable recurrences of the
kernels: seeds by explicit 3 x 3 shifted sums, D as the minimum over all (2R + 1)^2 shifted seed planes, the border by
padding with seeds, weights in np.float32 (numpy's float32 sqrt, subtraction and division are each correctly rounded).

model      every output of one frame.
frames_for the planted frames of the host and GPU tests; run_host / run_model / same: the shared comparison.
e2e_*      the loop-closure views with a disc field of view and a saturated block, blended with the CPU oracle.
"""
import numpy as np

F32 = np.float32
U8N, TEX_F32 = 0, 2
KINDS = ("mask", "wts", "dist2")
LO, HI = 30, 240
SHAPES = [(1, 1), (7, 3), (63, 5), (64, 64), (65, 9), (129, 70), (200, 150)]
RADII = (1, 2, 8, 31)
MIN_COUNTS = (1, 4, 9)


def margins(R):
    return sorted({m for m in (0, 1, R - 1) if 0 <= m < R})


def seeds(frame, lo, hi, min_count, base=None):
    mx = frame[..., :3].max(axis=-1).astype(np.int64)
    bad = (mx < lo) | (mx > hi)
    fh, fw = bad.shape
    p = np.pad(bad, 1).astype(np.int64)
    count = sum(p[1 + dy:1 + dy + fh, 1 + dx:1 + dx + fw] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    s = bad & (count >= min_count)
    if base is not None:
        s = s | (np.asarray(base) == 0)
    return s


def dist2(seed, R, border):
    """min(R^2, squared distance to the nearest seed or, with border, lattice point outside the frame)"""
    fh, fw = seed.shape
    P = np.pad(seed, R, constant_values=bool(border))
    D = np.full((fh, fw), R * R, np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            d2 = dx * dx + dy * dy
            if d2 < R * R:                      # a farther shift cannot lower the clipped minimum
                np.minimum(D, d2, out=D, where=P[R + dy:R + dy + fh, R + dx:R + dx + fw])
    return D


def outputs_of(D, seed, R, margin, mask_format):
    valid = D > margin * margin
    with np.errstate(invalid="ignore"):
        w = ((np.sqrt(D.astype(F32)) - F32(margin)) / F32(R - margin)).astype(F32)
    mask = np.where(valid, 255, 0).astype(np.uint8) if mask_format == U8N else np.where(valid, 1, 0).astype(F32)
    return dict(mask=mask, wts=np.where(valid, w, F32(0)).astype(F32), dist2=D.astype(np.uint16),
                counts=np.array([seed.sum(), valid.sum()], np.uint64))


def model(frame, lo=0, hi=255, R=32, margin=0, min_count=1, border=True, base=None, mask_format=U8N):
    s = seeds(frame, lo, hi, min_count, base)
    return outputs_of(dist2(s, R, border), s, R, margin, mask_format)


def run_model(frames, **kw):
    outs = [model(f, **kw) for f in frames]
    return {q: np.stack([o[q] for o in outs]) for q in KINDS + ("counts",)}


def run_host(nm, frames, **kw):
    mask, wts, d2, counts = nm.frame_weights_host(frames, want=KINDS, counts=True, **kw)
    return dict(mask=mask, wts=wts, dist2=d2, counts=counts)


def bits(a):
    return a.view(np.uint32) if a.dtype == F32 else a


def same(got, want, kinds=KINDS + ("counts",)):
    for q in kinds:
        assert got[q].dtype == want[q].dtype and got[q].shape == want[q].shape, q
        assert np.array_equal(bits(got[q]), bits(want[q])), q


# ---- planted frames ---------------------------------------------------------------------------------------------------------
_FRAMES = {}


def frames_for(fw, fh, seed=0):
    """three byte frames of fw x fh: random mid-range pixels (never raw-bad at LO / HI) with (0) a dark surround outside an
    ellipse, single dark noise pixels inside it; (1) saturated highlights of 1 to 5 pixels and a dark corner; (2) both, and a
    disc of saturation. Built once per shape, never changed by a test."""
    if (fw, fh, seed) in _FRAMES:
        return _FRAMES[(fw, fh, seed)]
    rng = np.random.default_rng(1000 * fw + fh + seed)
    y, x = np.mgrid[0:fh, 0:fw]
    out = []
    for q in range(3):
        f = rng.integers(LO + 5, HI - 5, (fh, fw, 4), dtype=np.uint8)
        f[..., 3] = rng.integers(0, 256, (fh, fw), dtype=np.uint8)          # alpha must play no part
        cx, cy = (fw - 1) / 2.0, (fh - 1) / 2.0
        outside = ((x - cx) / (0.42 * fw + 1)) ** 2 + ((y - cy) / (0.42 * fh + 1)) ** 2 > 1
        if q in (0, 2):
            f[outside, :3] = rng.integers(0, LO, (int(outside.sum()), 3), dtype=np.uint8)
            for _ in range(max(1, fw * fh // 400)):
                f[rng.integers(0, fh), rng.integers(0, fw), :3] = 3
        if q in (1, 2):
            for _ in range(max(1, fw * fh // 300)):
                hy, hx = int(rng.integers(0, fh)), int(rng.integers(0, fw))
                for _ in range(int(rng.integers(1, 6))):
                    f[min(fh - 1, hy + int(rng.integers(0, 2))), min(fw - 1, hx + int(rng.integers(0, 3))), int(rng.integers(0, 3))] = 255
            f[:max(1, fh // 5), :max(1, fw // 6), :3] = 0
        if q == 2 and fw > 20 and fh > 20:
            f[(x - 0.6 * fw) ** 2 + (y - 0.4 * fh) ** 2 < (0.08 * min(fw, fh)) ** 2, :3] = 250
        out.append(f)
    _FRAMES[(fw, fh, seed)] = out
    return out


def base_for(fw, fh):
    """a shared plane with a zero band on the right edge, a zero pixel and non-zero values of several sizes elsewhere"""
    y, x = np.mgrid[0:fh, 0:fw]
    b = (1 + (x * 7 + y * 13) % 255).astype(np.uint8)
    if fw > 3:
        b[:, fw - max(1, fw // 10):] = 0
    if fw > 8 and fh > 2:
        b[fh // 2, fw // 3] = 0
    return b


def blank(fw, fh, value=128):
    f = np.full((fh, fw, 4), value, np.uint8)
    f[..., 3] = 255
    return f


def with_seeds(fw, fh, points):
    """a frame whose only raw-bad pixels at lo = LO are the given (x, y) points"""
    f = blank(fw, fh)
    for px, py in points:
        f[py, px, :3] = 0
    return f


# ---- end to end on the loop-closure views -----------------------------------------------------------------------------------
E2E = dict(lo=8, hi=250, R=32, margin=1, min_count=4, border=True)
_E2E = {}


def e2e_corrupt(views):
    """every pixel outside the inscribed disc black, one saturated 36 x 36 block per view at a view-dependent place in it"""
    fh, fw = views[0].shape[:2]
    y, x = np.mgrid[0:fh, 0:fw]
    outside = (x - (fw - 1) / 2.0) ** 2 + (y - (fh - 1) / 2.0) ** 2 > (fh / 2.0) ** 2
    out = []
    for k, v in enumerate(views):
        f = v.copy()
        f[outside, :3] = 0
        bx, by = fw // 2 - 110 + 23 * k, fh // 2 - 90 + 17 * ((3 * k) % 10)
        f[by:by + 36, bx:bx + 36, :3] = 255
        out.append(f)
    return out


def e2e_blend(oracle, views, masks, wts, recs16, cw, ch):
    """the feather blend of the views in order with the CPU oracle (what nm_transform_blend_batch computes bit for bit)"""
    canvas, cwts = np.zeros((ch, cw, 4), np.uint8), np.zeros((ch, cw), F32)
    for k, v in enumerate(views):
        tx, ty, nw, nh = (int(t) for t in recs16[k, 9:13])
        canvas, cwts = oracle.transform_blend(canvas, cwts, v, nw, nh, recs16[k, :9].view(F32), tx, ty, masks[k], wts[k])
    return canvas, cwts


def e2e_host(nm, oracle, seed=91):
    """The chain on the CPU: placement by the host twin, the stage's host twin on the corrupted views, three oracle blends.
    Returns a dict: corrupted views, records, the stage's planes, the three canvases, the selection (canvas pixels that some
    frame's generated valid region covers) and the two figures (mean absolute byte difference to the clean canvas there)."""
    import bands_ref as B
    import loop_closure_ref as LC
    if seed in _E2E:
        return _E2E[seed]
    views = B.e2e_views(seed)
    chain = B.e2e_geometry()[3]
    recs16, _ = nm.mosaic_place_host(chain, LC.VW, LC.VH, LC.SCENE_W, LC.SCENE_H, LC.ORIGIN_X, LC.ORIGIN_Y)
    cw, ch = LC.SCENE_W, LC.SCENE_H
    bad = e2e_corrupt(views)
    mask, wts = nm.frame_weights_host(bad, **E2E)
    ones, rect = np.full((LC.VH, LC.VW), 255, np.uint8), B.e2e_weights()
    clean = e2e_blend(oracle, views, [ones] * LC.K, [rect] * LC.K, recs16, cw, ch)
    plain = e2e_blend(oracle, bad, [ones] * LC.K, [rect] * LC.K, recs16, cw, ch)
    stage = e2e_blend(oracle, bad, mask, wts, recs16, cw, ch)
    sel = stage[1] > 0
    fig = dict(rectangle=mean_abs(plain[0], clean[0], sel), stage=mean_abs(stage[0], clean[0], sel))
    _E2E[seed] = dict(views=bad, recs16=recs16, mask=mask, wts=wts, clean=clean, plain=plain, stage=stage, sel=sel, fig=fig)
    return _E2E[seed]


def mean_abs(a, b, sel):
    return float(np.abs(a[..., :3].astype(np.int64) - b[..., :3].astype(np.int64))[sel].mean())
