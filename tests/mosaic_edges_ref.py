"""Edge inputs of the two-band blend and the median composite, shared by the CPU tests (host twin against the float64 models:
tests/test_mosaic_edges_host.py, test_mosaic_bands_host.py, test_mosaic_median_host.py) and the GPU tests (device against host
twin, bit for bit: tests/test_gpu_mosaic_bands_edges.py, test_gpu_mosaic_median_edges.py). TEST INFRASTRUCTURE ONLY. Every case
is built once, its arrays are made read-only, and no test changes it.

tile_counts      tiles that each grid-stride loop of the kernels walks, from the records.
multi_trip_case  many thin frames: every loop of the bands and median kernels makes two full trips and a remainder on 256 CUs.
warp_trip_case   real maps and source frames for the warp-tiles loop, the same way.
blur_edge_scene  rectangles at the blur's own tile edges (128 x 8 and 32 x 32), strips, a deep clip, records at the int limits.
bands_*          ties, weight limits, an all-invalid pixel, colours that saturate both ways.
median_*         equal keys (with distinct colours), signed zeros, subnormal and negative keys, keys of +-FLT_MAX, weight limits,
                 tau edges, frames 62 and 63 alone, a frame that is never valid.
"""
import numpy as np

import bands_ref as B
import median_ref as M

F32 = np.float32
INF = float("inf")
G_DESIGN = 8 * 256                   # workgroups per launch on 256 compute units
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
FLT_MAX = M.FLT_MAX
DENORM_MIN = float(np.nextafter(F32(0), F32(1)))
WALKS = dict(warp=(64, 4), row=(128, 8), col=(32, 32))      # per used frame's rectangle
UNION_WALKS = dict(canvas=(64, 4), median=(64, 2))          # over the bounding box of the clipped rectangles
_CACHE = {}


def _once(fn):
    def get(*args):
        key = (fn.__name__,) + args
        if key not in _CACHE:
            out = fn(*args)
            for t in out[0]:
                if t is not None:
                    t.setflags(write=False)
            _CACHE[key] = out
        return _CACHE[key]
    get.__doc__ = fn.__doc__
    return get


def _div(a, b):
    return -(-a // b)


def tile_counts(recs, tile_cap, cw, ch):
    """tiles walked by each grid-stride loop, by the kernels' own formulas: warp / row / col over every used frame's
    rectangle, canvas / median over the bounding box of the used rectangles' parts on the canvas"""
    recs = [tuple(int(v) for v in r) for r in recs]
    used = [r for r in recs if B.used(r, tile_cap)]
    out = {name: sum(_div(r[2], tw) * _div(r[3], th) for r in used) for name, (tw, th) in WALKS.items()}
    boxes = [c[0] for c in (B._clip(r, cw, ch) for r in used) if c is not None]
    uw = max(b[1].stop for b in boxes) - min(b[1].start for b in boxes) if boxes else 0
    uh = max(b[0].stop for b in boxes) - min(b[0].start for b in boxes) if boxes else 0
    for name, (tw, th) in UNION_WALKS.items():
        out[name] = _div(uw, tw) * _div(uh, th)
    return out


PALETTE = (0.3, 0.55, 0.8, 0.42)     # times 255.9999 none lies near an integer


# ---- A. two full trips and a remainder ----------------------------------------------------------------------------------
@_once
def multi_trip_case():
    """(tiles, recs, tile_cap, cw, ch). 64 records on a 1000 x 1200 canvas: thin frames of mixed sizes, most of them taller
    than the canvas, spread over its width; fourteen of them crowd into 60 columns in the middle (stacks deeper than 10),
    and those carry grey levels of a four-entry palette, so that equal keys are the rule there. Unused records: 0 and 20
    unplaced, 21 and 63 over tile_cap, 22 wholly off the canvas (it has tiles but no canvas pixel), so the running totals of
    the walks hold runs of equal ends, at the start, in the middle and at the end."""
    rng = np.random.default_rng(4097)
    cw, ch, cap = 1000, 1200, 33 * 1300
    shapes = [(33, 1300), (34, 1250), (33, 1291), (35, 1222), (33, 1300), (40, 1072), (34, 1261), (33, 1277), (65, 660),
              (17, 1300), (33, 1300), (36, 1190), (1, 1300), (33, 1289), (129, 331)]
    unused = {0: "unplaced", 20: "unplaced", 21: "over", 22: "off", 63: "over"}
    crowd = set(range(30, 44))
    tiles, recs = [], []
    spread = [k for k in range(64) if k not in unused and k not in crowd]
    xs = dict(zip(spread, np.linspace(-12, 972, len(spread)).astype(int)))
    for k in range(64):
        nw, nh = shapes[k % len(shapes)] if k not in crowd else shapes[k % 8]
        kind = unused.get(k)
        if kind == "over":
            recs.append((100 + k, 10, 33, 1301, 1))
            tiles.append(None)
            continue
        ty = int(rng.integers(-60, -40)) if nh > 1260 else int(rng.integers(-30, ch - nh + 30))
        tx = int(rng.integers(470, 497)) if k in crowd else int(xs.get(k, 500))
        if kind == "off":
            tx, ty = cw + 1, 0
        recs.append((tx, ty, nw, nh, 0 if kind == "unplaced" else 1))
        t = B.texture(rng, nw, nh)
        if k in crowd:
            grey = np.array(PALETTE, F32)[rng.integers(0, len(PALETTE), (nh, nw))]
            t[..., :3] = np.where(t[..., 3:] > 0, grey[..., None], 0)
        tiles.append(t)
    return tiles, recs, cap, cw, ch


def _warp_rec(tx, ty, nw, nh, placed, m):
    r = np.zeros(16, np.int32)
    r[:9] = np.asarray(m, F32).view(np.int32)
    r[9:14] = (tx, ty, nw, nh, placed)
    return r


_WARP = {}


def warp_trip_case():
    """dict(frames, mask, wts, recs (n, 16) int32, gains, cap, cw, ch, fw, fh, stats): 20 records with real maps (local
    canvas pixel -> pixel of a 131 x 97 frame: a tall rectangle squeezed into the frame's height, slightly rotated and with a
    little perspective), widths 1 .. 65 and heights about 1300, so that the 64 x 4 walk has many tiles from few pixels.
    Unused: 0 unplaced, 7 over tile_cap, 8 unplaced; 9 is wholly off the canvas (its tiles are still written)."""
    if _WARP:
        return _WARP
    rng = np.random.default_rng(2049)
    fw, fh, cw, ch = 131, 97, 150, 1320
    cap = 65 * 1300
    sizes = [(1, 1300), (63, 1203), (64, 1300), (65, 1101), (2, 1297), (33, 1300), (1, 1299), (65, 1301), (5, 600), (64, 1300),
             (5, 1300), (64, 1283), (3, 1111), (65, 1300), (63, 1299), (1, 1300), (64, 1187), (17, 1300), (65, 1250), (2, 1300)]
    recs = []
    for k, (nw, nh) in enumerate(sizes):
        a = rng.uniform(-0.01, 0.01)
        sx, sy = rng.uniform(0.8, 1.1), (fh - 9.0) / nh
        p = rng.uniform(-2e-6, 2e-6)
        dx = fw / 2.0 - sx * nw / 2.0 + rng.uniform(-6, 6)
        m = [sx * np.cos(a), -sy * np.sin(a) * 0.1, dx, sx * np.sin(a), sy * np.cos(a), 4.0 + rng.uniform(-1, 1), p, -p, 1.0]
        tx, ty = int(rng.integers(-3, cw - nw + 3)), int(rng.integers(-15, 25))
        placed = 0 if k in (0, 8) else 1
        if k == 9:
            tx = cw + 2
        recs.append(_warp_rec(tx, ty, nw, nh, placed, m))
    y, x = np.mgrid[0:fh, 0:fw]
    disc = ((x - fw / 2) ** 2 / (fw / 2) ** 2 + (y - fh / 2) ** 2 / (fh / 2) ** 2) < 0.95
    feather = (np.minimum(np.minimum(x, fw - 1 - x), np.minimum(y, fh - 1 - y)) / (fh / 2.0)).astype(F32)
    _WARP.update(frames=[rng.integers(0, 256, (fh, fw, 4), dtype=np.uint8) for _ in range(3)], mask=(disc * 255).astype(np.uint8),
                 wts=feather, recs=np.stack(recs), gains=rng.uniform(0.5, 2.0, (len(recs), 3)).astype(F32), cap=cap, cw=cw,
                 ch=ch, fw=fw, fh=fh, stats=[17, 3])
    return _WARP


# ---- B. the blur's tile edges ---------------------------------------------------------------------------------------------
BLUR_RADII = (2, 31, 32)
EXTREME = 5                          # the last records of blur_edge_scene: used frames at the int limits


@_once
def blur_edge_scene():
    """(tiles, recs, tile_cap, cw, ch). Two larger frames under everything; rectangles 127 / 128 / 129 x 7 / 8 / 9 (the row
    pass's 128 x 8 tile), squares of 31 / 32 / 33 and 63 / 64 / 65 (the column pass's 32 x 32 tile, one and two of them),
    strips 1 x 200 and 200 x 1, a single pixel, a 260 x 260 frame at (-200, -200) whose part on the canvas starts deep inside
    its second tile in both axes, and five used frames with tx or ty at INT_MAX, -INT_MAX and INT_MIN that touch no pixel."""
    rng = np.random.default_rng(128)
    cw, ch = 420, 300
    recs = [(20, 15, 230, 170, 1), (150, 90, 230, 170, 1)]
    for i, nw in enumerate((127, 128, 129)):
        for j, nh in enumerate((7, 8, 9)):
            recs.append((30 + 120 * i + 5 * j, 40 + 70 * j + 11 * i, nw, nh, 1))
    for i, s in enumerate((31, 32, 33, 63, 64, 65)):
        recs.append((45 + 58 * i, 95 + 17 * (i % 3), s, s, 1))
    recs += [(200, 50, 1, 200, 1), (110, 160, 200, 1, 1), (260, 130, 1, 1, 1), (-200, -200, 260, 260, 1)]
    recs += [(INT_MAX, 5, 3, 2, 1), (INT_MIN, 7, 2, 3, 1), (5, INT_MAX, 3, 2, 1), (9, INT_MIN, 4, 4, 1), (-INT_MAX, -INT_MAX, 2, 2, 1)]
    tiles = [B.texture(rng, r[2], r[3], holes=r[2] * r[3] > 300) for r in recs]
    for k in range(2, 20):                              # small frames weigh enough to win part of their rectangle
        tiles[k][..., 3] *= F32(12.0 if k < 17 else 90.0)
    tiles[19][..., 3] = F32(500.0)                      # the single pixel wins
    return tiles, recs, 260 * 260, cw, ch


# ---- C. bands: what only the host twin saw ----------------------------------------------------------------------------------
@_once
def bands_tie_case():
    """two frames on one rectangle, every weight 1.5 (the case of the host test's tie and last_tie checks)"""
    rng = np.random.default_rng(5)
    a, b = B.texture(rng, 40, 30, holes=False), B.texture(rng, 40, 30, holes=False)
    a[..., 3] = b[..., 3] = F32(1.5)
    return [a, b], [(2, 2, 40, 30, 1), (2, 2, 40, 30, 1)], 1200, 50, 40


TIE_BANDS = {"two": (0, 8), "three": (8, 16), "apart": (16, 24), "not_lowest": (24, 32), "free": (32, 70)}
TIE_WINNER = {"two": 1, "three": 1, "apart": 2, "not_lowest": 3}      # where every frame covers; see bands_ties_case


@_once
def bands_ties_case():
    """(tiles, recs, tile_cap, cw, ch). Six frames of 70 x 30; frames 1 .. 5 on one rectangle at (3, 2), frame 0 eight rows
    lower, so that the lowest covering frame changes inside the others. Weights by column band (TIE_BANDS), colours random:
      two         frames 1 and 2 at 1.5, the rest 1.0                         -> 1
      three       frames 1, 3 and 5 at 2.0, the rest 1.0                      -> 1
      apart       frames 2 and 4 at 2.5 with the lighter frame 3 between them -> 2
      not_lowest  frames 3 and 4 at 3.0 over the lighter frames 0, 1 and 2    -> 3 (the lowest covering frame is 0 or 1)
      free        random weights, no tie
    Frame 0 is the lightest everywhere, so TIE_WINNER holds on every row."""
    rng = np.random.default_rng(55)
    nw, nh = 70, 30
    heavy = {"two": ((1, 2), 1.5), "three": ((1, 3, 5), 2.0), "apart": ((2, 4), 2.5), "not_lowest": ((3, 4), 3.0)}
    tiles = []
    for k in range(6):
        t = B.texture(rng, nw, nh, holes=False)
        for name, (c0, c1) in TIE_BANDS.items():
            if name != "free":
                frames, w = heavy[name]
                t[:, c0:c1, 3] = F32(w if k in frames else (0.5 if k == 0 else 1.0))
        tiles.append(t)
    tiles[3][:, 16:24, 3] = F32(1.25)
    recs = [(3, 10, nw, nh, 1)] + [(3, 2, nw, nh, 1)] * 5
    return tiles, recs, nw * nh, 80, 45


SPECIAL = dict(neg_zero=(slice(4, 8), slice(4, 12)), denorm=(slice(4, 8), slice(16, 24)), flt_max=(slice(4, 8), slice(28, 36)),
               dead=(slice(14, 15), slice(20, 21)), dark=(slice(20, 26), slice(4, 16)), bright=(slice(20, 26), slice(24, 40)))


@_once
def bands_special_case():
    """(tiles, recs, tile_cap, cw, ch). Three frames of 50 x 30, frames 0 and 1 on one rectangle, frame 2 shifted by (9, 5).
    Local regions of frames 0 and 1 (SPECIAL, rows x columns):
      neg_zero  w = -0.0 in frame 0 (invalid: the pixel falls to frame 1)
      denorm    w = the smallest subnormal in frame 0 and 0 in frame 1 (valid: frame 0 wins wherever frame 2 is absent or 0)
      flt_max   w = FLT_MAX in frame 1
      dead      one pixel invalid in every frame, with valid pixels all round it
      dark      colours of 0 .. 0.004 in frame 0 under a heavier weight, against ordinary colours in frame 1; in the region's
                right half frame 1 is heavier still and every other pixel of it is black (valid, C = 0): next to the seam
                the low-band correction takes those below zero
      bright    gained colours of 1.5 .. 2.0 in frame 1 under a heavier weight
    The dark and bright regions are small, so that few bytes sit at the ends of the store's range."""
    rng = np.random.default_rng(56)
    nw, nh = 50, 30
    t = [B.texture(rng, nw, nh, holes=False) for _ in range(3)]
    t[0][SPECIAL["neg_zero"]] = (0, 0, 0, -0.0)
    t[0][SPECIAL["denorm"] + (3,)] = F32(DENORM_MIN)
    t[1][SPECIAL["denorm"]] = 0
    t[1][SPECIAL["flt_max"] + (3,)] = F32(FLT_MAX)
    t[0][SPECIAL["dead"]] = t[1][SPECIAL["dead"]] = 0
    t[2][14 - 5, 20 - 9] = 0
    shape = t[0][SPECIAL["dark"]].shape[:2]
    t[0][SPECIAL["dark"]] = np.concatenate([rng.uniform(0, 0.004, shape + (3,)), np.full(shape + (1,), 50.0)], -1).astype(F32)
    t[1][20:26, 10:16, 3] = F32(80.0)
    t[1][20:26:2, 10:16:2, :3] = 0
    shape = t[1][SPECIAL["bright"]].shape[:2]
    t[1][SPECIAL["bright"]] = np.concatenate([rng.uniform(1.5, 2.0, shape + (3,)), np.full(shape + (1,), 60.0)], -1).astype(F32)
    return t, [(4, 3, nw, nh, 1), (4, 3, nw, nh, 1), (13, 8, nw, nh, 1)], nw * nh, 70, 45


FLAT_SIGMA = (7, 1000.0)             # R, sigma: every tap within a few ulps of 1 / 15
SUBNORMAL_SIGMA = (32, 1.0)          # R, sigma: g[14] is subnormal in fp32, g[15 ..] are exactly 0


# ---- C. median --------------------------------------------------------------------------------------------------------------
def grey(level, w, nw=9, nh=4):
    t = np.empty((nh, nw, 4), F32)
    t[..., :3], t[..., 3] = F32(level), F32(w)
    return t


def colour_of_key(y0, rng):
    """a colour (B, G, R) in (0, 1) whose fp32 key is exactly y0: B and R drawn, G searched among the floats round the root"""
    y0 = F32(y0)
    for _ in range(100):
        b, r = F32(rng.uniform(0.05, 0.95)), F32(rng.uniform(0.05, 0.95))
        g0 = F32((float(y0) - 0.07 * float(b) - 0.21 * float(r)) / 0.72)
        if not 0.02 < g0 < 0.98:
            continue
        bs = (np.array([b]).view(np.int32) + np.arange(-8, 9, dtype=np.int32)).view(F32)
        gs = (np.array([g0]).view(np.int32) + np.arange(-64, 65, dtype=np.int32)).view(F32)
        C = np.stack(np.broadcast_arrays(bs[:, None], gs[None, :], r), axis=-1)
        hit = np.argwhere(M.key(C) == y0)
        if len(hit):
            i, j = hit[len(hit) // 2]
            return np.array([bs[i], gs[j], r], F32)
    raise AssertionError("no colour of key %r found" % (y0,))


def _stack(n, columns, nh=3, ordinary=0, seed=0):
    """n frames on ONE rectangle of len(columns) x (nh + ordinary) at (2, 1): columns[c] maps a frame index to its sample
    (B, G, R, w) in column c of the first nh rows; a frame absent from a column has w = 0 and colour 0 there. The `ordinary`
    rows below hold random colours and weights in frames 3, 17, 34, 48 and 62: they keep the share of bytes that sit on an
    integer (zeros, above all) under the comparison's cap."""
    rng = np.random.default_rng(seed)
    nw = len(columns)
    tiles = [np.zeros((nh + ordinary, nw, 4), F32) for _ in range(n)]
    for c, col in enumerate(columns):
        for k, s in col.items():
            tiles[k][:nh, c] = np.asarray(s, F32)
    for k in (3, 17, 34, 48, 62):
        if ordinary:
            tiles[k][nh:] = B.texture(rng, nw, ordinary, holes=False)
    return tiles, [(2, 1, nw, nh + ordinary, 1)] * n, nw * (nh + ordinary), nw + 5, nh + ordinary + 3


TIE_KEYS = (0.35, 0.5, 0.65)


@_once
def median_ties_case():
    """(tiles, recs, tile_cap, cw, ch): 64 frames, 96 columns (two canvas tiles of the kernel across). Every sample has its
    own colour and weight; keys come from the three values of TIE_KEYS, so that equal keys are everywhere.
      column 0      frames 0 and 1 tied (m = 2)
      column 1      keys (0.65, t, t, 0.65'): the tie holds ranks 0 and 1, the median rank is its second member
      column 2      keys (low, t, high, t, high'), m = 5: the tie holds ranks 1 and 2 and straddles the median rank
      column 3      all 64 frames with one key: the median frame is 31
      column 4      frames 62 and 63 alone, tied
      column 5      frames 40 .. 47, two keys, four frames each: the lower tie holds ranks 0 .. 3, the median is its last member
      columns 6 ..  2 .. 12 random frames each (half of them at or above 32), keys drawn from TIE_KEYS"""
    rng = np.random.default_rng(64)
    t = F32(0.5)
    s = lambda y, w=None: tuple(colour_of_key(y, rng)) + (rng.uniform(0.5, 2.0) if w is None else w,)
    cols = [{0: s(t), 1: s(t)},
            {0: s(0.65), 1: s(t), 2: s(t), 3: s(0.65)},
            {0: s(0.35), 1: s(t), 2: s(0.65), 3: s(t), 4: s(0.65)},
            {k: s(t) for k in range(64)},
            {62: s(t), 63: s(t)},
            {k: s(0.35 if k % 2 else 0.65) for k in range(40, 48)}]
    pool = list(range(64))
    while len(cols) < 96:
        m = int(rng.integers(2, 13))
        frames = rng.choice(pool[:32] if len(cols) % 2 else pool[32:], m, replace=False)
        cols.append({int(k): s(TIE_KEYS[int(rng.integers(0, 3))]) for k in frames})
    return _stack(64, cols)


@_once
def median_equal_greys(which):
    """the grey stacks of the host test: 0 four equal keys, 1 (-0, +0, -0), 2 (+0, -0, 0.7, -0, +0)"""
    recs, cap = [(1, 1, 9, 4, 1)] * 5, 36
    if which == 0:
        return [grey(0.5, 1.0 + k) for k in range(4)], recs[:4], cap, 12, 6
    if which == 1:
        return [grey(-0.0, 3.0), grey(0.0, 4.0), grey(-0.0, 5.0)], recs[:3], cap, 12, 6
    return [grey(0.0, 3.0), grey(-0.0, 4.0), grey(0.7, 5.0), grey(-0.0, 6.0), grey(0.0, 7.0)], recs, cap, 12, 6


EQUAL_GREYS_WANT = ((1, 2.0), (1, 4.0), (3, 6.0))            # (label, weight) of SELECT over the rectangle


LIMITS_W_MIN = 0.5


@_once
def median_limits_case():
    """six grey frames of 9 x 4 with one odd sample each in row 0 (the host test's): a NaN colour, +inf and -inf colours,
    w == w_min (invalid), w = inf (invalid), w = FLT_MAX (valid), w NaN, w = nextafter(w_min) (valid). w_min = LIMITS_W_MIN."""
    tiles = [grey(0.11 * (k + 1), 2.0) for k in range(6)]
    tiles[0][0, 0, 2] = np.nan
    tiles[1][0, 1, 0] = np.inf
    tiles[2][0, 2, 1] = -np.inf
    tiles[3][0, 3, 3] = F32(LIMITS_W_MIN)
    tiles[4][0, 4, 3] = np.inf
    tiles[4][0, 5, 3] = F32(FLT_MAX)
    tiles[5][0, 6, 3] = np.nan
    tiles[5][0, 7, 3] = np.nextafter(F32(LIMITS_W_MIN), F32(1))
    return tiles, [(0, 0, 9, 4, 1)] * 6, 36, 9, 4


TAU_LEVELS = (0.1, 0.3, 0.45, 0.7, 0.95)


@_once
def median_tau_case():
    """five grey frames of 9 x 4 at TAU_LEVELS (the host test's); tau_values() are the taus that belong to it"""
    return [grey(v, 1.0 + k) for k, v in enumerate(TAU_LEVELS)], [(2, 1, 9, 4, 1)] * 5, 36, 14, 6


def tau_values():
    """dict: zero, a subnormal, infinite, the fp32 difference of the keys of frames 3 and 2 itself, and the float below it"""
    ys = [M.key(t[0, 0, :3]) for t in median_tau_case()[0]]
    exact = float(np.abs(F32(ys[3] - ys[2])))
    return dict(zero=0.0, subnormal=DENORM_MIN * 3, inf=INF, exact=exact, below=float(np.nextafter(F32(exact), F32(0))))


@_once
def median_keys_case():
    """(tiles, recs, tile_cap, cw, ch): 64 frames, 8 columns of odd keys; colours differ from frame to frame.
      column 0  subnormal keys: colours of a few times 1e-41 (the products underflow into subnormals), m = 5
      column 1  negative keys and a positive one, m = 5
      column 2  keys +0, -0 and the subnormals of both signs next to them, m = 4
      column 3  colours of FLT_MAX and -FLT_MAX in frames 0 and 1: the key is +-FLT_MAX, the largest a finite colour can give
                (the coefficients add up to less than 1 + 2^-25, so the key of finite colours never overflows: only an
                infinite or NaN colour makes a key invalid, and median_limits_case has those); frames 2, 3, 4 ordinary
      column 4  a finite key of about 1e38 (valid; the bytes saturate) against ordinary ones, m = 3
      column 5  frames 62 and 63 alone, with different keys
      column 6  frames 5, 33 and 60: keys of 7, 9 and 29 subnormal steps, for a tau of three steps
      column 7  one frame alone: frame 47
    One row of these, and 150 ordinary rows under it (_stack). Frames 13 and 50 are valid nowhere."""
    rng = np.random.default_rng(65)
    w = lambda: float(rng.uniform(0.5, 2.0))
    tiny = lambda a, b, c: (a * 1e-41, b * 1e-41, c * 1e-41, w())
    cols = [{1: tiny(3, 5, 2), 8: tiny(9, 1, 4), 20: tiny(1, 2, 8), 35: tiny(7, 7, 1), 61: tiny(2, 9, 9)},
            {0: (-0.2, -0.5, -0.1, w()), 7: (-0.9, -0.1, -0.3, w()), 32: (0.1, -0.3, 0.2, w()), 44: (0.5, 0.4, 0.3, w()),
             63: (-0.6, -0.6, -0.6, w())},
            {2: (0.0, 0.0, 0.0, w()), 3: (-0.0, -0.0, -0.0, w()), 36: (0.0, 2 * DENORM_MIN, 0.0, w()), 37: (-0.0, -2 * DENORM_MIN, -0.0, w())},
            {0: (FLT_MAX, FLT_MAX, FLT_MAX, w()), 1: (-FLT_MAX, -FLT_MAX, -FLT_MAX, w()), 2: (0.2, 0.3, 0.4, w()), 3: (0.6, 0.5, 0.4, w()),
             4: (0.9, 0.8, 0.1, w())},
            {9: (1e38, 1e38, 1e38, w()), 10: (0.2, 0.3, 0.4, w()), 41: (0.3, 0.2, 0.6, w())},
            {62: (0.2, 0.7, 0.4, w()), 63: (0.8, 0.3, 0.1, w())},
            {5: (0.0, 10 * DENORM_MIN, 0.0, w()), 33: (0.0, 13 * DENORM_MIN, 0.0, w()), 60: (0.0, 40 * DENORM_MIN, 0.0, w())},
            {47: (0.25, 0.35, 0.45, w())}]
    return _stack(64, cols, nh=1, ordinary=150, seed=66)


def median_cases():
    """name -> (case, w_min, tau, modes): every C case of the median. The GPU test runs each in both modes against the host
    twin; the CPU test runs `modes` against the model. The grey stacks are SELECT only there, as in the host test they come
    from: the MEAN of equal greys of 0 or 0.5 sits on an integer byte at every pixel, which the comparison's cap on such bytes
    forbids; the ties and keys cases hold the same keys (equal, +0 against -0) between ordinary rows, in both modes."""
    both = (M.SELECT, M.MEAN)
    taus = tau_values()
    out = {"ties": (median_ties_case(), 0.0, 0.1, both), "ties_tau0": (median_ties_case(), 0.0, 0.0, both),
           "ties_inf": (median_ties_case(), 0.25, INF, both), "keys": (median_keys_case(), 0.0, 0.15, both),
           "keys_subnormal_tau": (median_keys_case(), 0.0, DENORM_MIN * 3, both),
           "keys_tau0": (median_keys_case(), 0.0, 0.0, both), "limits": (median_limits_case(), LIMITS_W_MIN, 0.25, both),
           "limits_inf": (median_limits_case(), LIMITS_W_MIN, INF, both)}
    for q in range(3):
        out["greys%d" % q] = (median_equal_greys(q), 0.0, INF, (M.SELECT,))
    for name, tau in taus.items():
        out["tau_" + name] = (median_tau_case(), 0.0, tau, both)
    out["blur_edges"] = (blur_edge_scene(), 0.0, 0.2, both)
    return out


def median_model(tiles, recs, cw, ch, cap, mode, w_min=0.0, tau=INF, slab=40, **mutant):
    """median_ref.model evaluated in column slabs of the canvas, each over the frames that meet it (the model is per pixel,
    so the slabs are exact): what a 64-frame case on a large canvas needs to fit in memory. Returns the entries that
    check_exact and compare_mean read: m, label, support, counts, out, weight, A."""
    n = len(recs)
    parts, counts = [], np.zeros((n, 2), np.uint64)
    for x0 in range(0, cw, slab):
        w = min(slab, cw - x0)
        keep = [k for k, r in enumerate(recs) if B.used(r, cap) and B._clip((r[0] - x0,) + tuple(r[1:]), w, ch) is not None]
        if not keep:
            nan3 = np.full((ch, w, 3), np.nan)
            parts.append(dict(m=np.zeros((ch, w), int), label=np.full((ch, w), -1), support=np.zeros((ch, w), int), out=nan3,
                              weight=nan3[..., 0], A=np.zeros((ch, w))))
            continue
        md = M.model([tiles[k] for k in keep], [(recs[k][0] - x0,) + tuple(recs[k][1:]) for k in keep], w, ch, cap, mode,
                     w_min=w_min, tau=tau, **mutant)
        md["label"] = np.where(md["label"] >= 0, np.array(keep)[np.maximum(md["label"], 0)], -1)
        counts[keep] += md["counts"]
        parts.append(md)
    out = {key: np.concatenate([p[key] for p in parts], axis=1) for key in ("m", "label", "support", "out", "weight", "A")}
    out["counts"] = counts
    return out


def median_written(tiles, recs, cw, ch, cap, w_min=0.0):
    """bool (ch, cw): the canvas pixels with at least one valid frame, i.e. the ones the median composite writes"""
    on = np.zeros((ch, cw), bool)
    for k, rec in enumerate(recs):
        c = B._clip(rec, cw, ch) if B.used(rec, cap) else None
        if c is None:
            continue
        t = tiles[k][c[1]]
        with np.errstate(invalid="ignore"):
            on[c[0]] |= (t[..., 3] > F32(w_min)) & (t[..., 3] <= F32(FLT_MAX)) & np.isfinite(M.key(t[..., :3]))
    return on
