"""The cases of tests/test_mosaic_exposure_edges_host.py and tests/test_gpu_mosaic_exposure_edges.py: the exposure stages
(measure, solve, gained blend) at the edges their own constants define. TEST INFRASTRUCTURE ONLY; it does not call the
library. Frames, masks and the numpy model come from tests/test_mosaic_exposure_host.py and tests/exposure_ref.py.

walk_cases     A  the measure kernel's tile walk: 255, 256, 257, 272, 512 and 1024 tiles of 64 x 32 lattice pixels for one
                  link, and batches of 17 and 256 links where ceil(4096 / L) sets the workgroups per link. Every case
                  carries the INTENDED (lw, lh, tiles_x, tiles, parts); the tests compare them with `lattice_of` (the entry
                  point's formulas) first, so a case that is not the edge it claims to be fails.
edge_cases     B  frames of 1 x 1 .. 2 x 2, lattices of 63 / 64 / 65 / 129 columns by 1 .. 5 / 31 / 32 / 33 rows at strides
                  1 and 3, empty lattices, all-0 and all-255 frames, whole-pixel translations, the last column on fw - 1.
SINGULAR, CORNERS, usability_cases, graph_cases
               C  the solve: inputs that end SINGULAR (kept as data), the corners of the sigma range, the usability
                  boundary, and graph shapes that stress the row assembly.

The maps of A are translations by a fraction of a pixel up and to the left, (-1, 0) in both axes: lattice column 0 and
lattice row 0 fall outside b, every other lattice pixel has its four taps inside b, so with bytes inside [lo, hi] every
64 x 32 tile of every shape holds counting pixels, the one-column and one-row tiles at the far edges included.
`model_sums` checks that per tile for the unmasked runs (the disc mask hides whole corner tiles by design).
"""
import numpy as np

import exposure_ref as X
import test_mosaic_exposure_host as HT

F32 = np.float32
TILE_W, TILE_H, MAX_PARTS, GRID_TARGET = 64, 32, 256, 4096       # csrc/nm_mosaic_exposure.hip
LO, HI = 5, 250
_CACHE = {}


def _once(key, build):
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def lattice_of(fw, fh, stride, L):
    """(lw, lh, tiles_x, tiles, parts) by the formulas of nm_mosaic_exposure_sums_dev"""
    lw, lh = fw // stride, fh // stride
    tiles_x = -(-lw // TILE_W)
    tiles = tiles_x * -(-lh // TILE_H)
    return lw, lh, tiles_x, tiles, min(-(-GRID_TARGET // L), MAX_PARTS, tiles)


def shift(tx, ty):
    return np.array([1, 0, tx, 0, 1, ty, 0, 0, 1], F32)


def frame(seed, fw, fh):
    """HT.frame with every colour byte inside [20, 235], shared between the cases of one shape"""
    return _once(("frame", seed, fw, fh), lambda: HT.frame(seed, fw, fh))


def mask_of(fw, fh):
    return _once(("mask", fw, fh), lambda: HT.disc_mask(fw, fh))


# ---- A: the tile walk ----
# L, (fw, fh, stride), the intended (lw, lh, tiles_x, tiles, parts), also under the disc mask
WALK = [
    (1, (16385, 3, 1), (16385, 3, 257, 257, 256), False),       # workgroup 0 alone takes a second tile, one column wide
    (1, (1087, 481, 1), (1087, 481, 17, 272, 256), True),       # 16 workgroups take two; t % 17 and t / 17 with remainders
    (1, (1024, 512, 1), (1024, 512, 16, 256, 256), False),      # workgroups == tiles: nothing wraps
    (1, (1087, 480, 1), (1087, 480, 17, 255, 255), True),       # parts clamped by the tiles
    (1, (2048, 512, 1), (2048, 512, 32, 512, 256), True),       # exactly two each
    (256, (1025, 5, 1), (1025, 5, 17, 17, 16), True),           # ceil(4096 / 256) = 16 < 17 tiles, every link slot
    (17, (1087, 481, 1), (1087, 481, 17, 272, 241), False),     # the uneven ceil(4096 / 17): 31 workgroups take two
    (1, (32767, 2, 1), (32767, 2, 512, 512, 256), False),       # the widest frame (under the disc no pixel of two rows counts)
    (1, (2, 32767, 1), (2, 32767, 1, 1024, 256), False),        # the tallest: four tiles each, tiles_x = 1
    (1, (2175, 963, 2), (1087, 481, 17, 272, 256), True),       # stride * u + stride / 2 under the walk
]
WALK_IDS = ["L%d-%dx%d-s%d" % ((w[0],) + w[1]) for w in WALK]
DISTINCT = 5            # a batch of 17 cycles through this many (a, b, H): the model runs once for each
SLOTS = dict(nonfinite=3, status0=5, status2=7)


def walk_cases():
    """dict(what, L, n, fw, fh, stride, lw, lh, tiles_x, tiles, parts, masked, frames, la, lb, H (L, 9), status or None).
    Batches: three distinct frames behind six table entries (pointers repeat), links in both directions, a non-finite H at
    slot 3, link_status 0 at slot 5 and 2 at slot 7."""
    def build():
        out = []
        for k, (L, (fw, fh, stride), (lw, lh, tiles_x, tiles, parts), masked) in enumerate(WALK):
            if L == 1:
                frames, la, lb, status = [frame(70, fw, fh), frame(71, fw, fh)], [0], [1], None
                H = shift(-0.3, -0.4)[None]
            else:
                base = [frame(70 + q, fw, fh) for q in range(3)]
                frames = [base[q % 3] for q in range(6)]
                pairs = [(0, 1), (2, 0), (1, 5), (4, 3), (3, 2)]        # as frames: (0,1) (2,0) (1,2) (1,0) (0,2)
                distinct = DISTINCT if fw * fh > 100000 else L
                la = [pairs[(l % distinct) % 5][0] for l in range(L)]
                lb = [pairs[(l % distinct) % 5][1] for l in range(L)]
                H = np.stack([shift(-0.1 - 0.003 * (l % distinct), -0.4 - 0.001 * (l % distinct)) for l in range(L)])
                H[SLOTS["nonfinite"], 4] = np.inf
                status = np.ones(L, np.int32)
                status[SLOTS["status0"]], status[SLOTS["status2"]] = 0, 2
            out.append(dict(what=WALK_IDS[k], L=L, n=len(frames), fw=fw, fh=fh, stride=stride, lw=lw, lh=lh, tiles_x=tiles_x,
                            tiles=tiles, parts=parts, masked=masked, frames=frames, la=la, lb=lb, H=H, status=status))
        return out
    return _once("walk", build)


def tile_counts(counted, tiles_x, tiles):
    """the counting pixels of each 64 x 32 tile, in the kernel's tile order t = row * tiles_x + column"""
    lh, lw = counted.shape
    pad = np.zeros((tiles // tiles_x * TILE_H, tiles_x * TILE_W), np.int64)
    pad[:lh, :lw] = counted
    return pad.reshape(tiles // tiles_x, TILE_H, tiles_x, TILE_W).sum(axis=(1, 3)).reshape(-1)


def live(c, l):
    return (c["status"] is None or c["status"][l] == 1) and bool(np.isfinite(c["H"][l]).all())


def model_sums(c, masked):
    """((L, 7) Python ints of the numpy model, the smallest per-tile count over the live links). A link's model is computed
    once per distinct (a, b, H)."""
    def build():
        mask = mask_of(c["fw"], c["fh"]) if masked else None
        seen, sums, least = {}, [], None
        for l in range(c["L"]):
            if not live(c, l):
                sums.append([0] * 7)
                continue
            A, B = c["frames"][c["la"][l]], c["frames"][c["lb"][l]]
            key = (id(A), id(B), c["H"][l].tobytes())
            if key not in seen:
                counted = []
                s = X.sums_int(A, B, c["H"][l], mask=mask, stride=c["stride"], lo=LO, hi=HI, counted=counted)
                per_tile = tile_counts(counted[0], c["tiles_x"], c["tiles"])
                assert int(per_tile.sum()) == s[0]
                seen[key] = (s, int(per_tile.min()))
            sums.append(seen[key][0])
            least = seen[key][1] if least is None else min(least, seen[key][1])
        return sums, least
    return _once(("model", c["what"], masked), build)


def cheap(c):
    """whether the GPU test evaluates the numpy model too (the host test does for every case)"""
    return c["L"] == 1 and c["lw"] * c["lh"] <= 100000


# ---- B: lattice and frame edges ----
def edge_cases():
    """dict(what, fw, fh, stride, A, B, H, lo, hi, want): want is None, or the N the case must give by construction"""
    def build():
        out = []

        def add(what, fw, fh, stride, H, A=None, B=None, lo=LO, hi=HI, want=None):
            k = len(out)
            out.append(dict(what="%s %d x %d stride %d" % (what, fw, fh, stride), fw=fw, fh=fh, stride=stride, H=np.asarray(H, F32),
                            A=frame(100 + k, fw, fh) if A is None else A, B=frame(300 + k, fw, fh) if B is None else B, lo=lo, hi=hi,
                            want=want))
        I, frac = shift(0, 0), np.array([1.002, 0.001, -0.3, -0.001, 0.998, -0.4, 1e-6, -1e-6, 1], F32)
        for fw, fh in ((1, 1), (2, 1), (1, 9), (9, 1), (2, 2)):
            add("tiny", fw, fh, 1, I, want=int((fw, fh) == (2, 2)))
        for lw in (63, 64, 65, 129):
            for lh in (1, 2, 3, 4, 5, 31, 32, 33):
                add("lattice %d x %d" % (lw, lh), lw, lh, 1, frac)
                add("lattice %d x %d" % (lw, lh), 3 * lw + (lw + lh) % 3, 3 * lh + lh % 3, 3, frac)
        for fw, fh, stride in ((131, 45, 64), (45, 131, 64), (3, 3, 4)):
            add("empty", fw, fh, stride, frac, want=0)
        for fw, fh in ((131, 45), (1025, 5)):
            zero, full = np.zeros((fh, fw, 4), np.uint8), np.full((fh, fw, 4), 255, np.uint8)
            add("all 0", fw, fh, 1, frac, zero, zero, 0, 255)
            add("all 255", fw, fh, 1, frac, full, full, 0, 255)
            add("all 255 hi 254", fw, fh, 1, frac, full, full, 0, 254, want=0)
        fw, fh = 67, 45
        for tx in (-1, 0, 1):
            for ty in (-1, 0, 1):           # column x counts when 0 <= x + tx <= fw - 2: fw - 1 columns, fw - 2 for tx = 1
                add("translation (%d, %d)" % (tx, ty), fw, fh, 1, shift(tx, ty), want=(fw - 1 - max(tx, 0)) * (fh - 1 - max(ty, 0)))
        # stride 3 on 3 lw + 2 columns: the last lattice column is x = fw - 4, and a shift of +3 lands it on fw - 1, whose
        # right-hand tap is outside b; fw - 2 would count
        add("last column on fw - 1", 3 * 22 + 2, 3 * 11, 3, shift(3, -0.5), want=21 * 11)
        add("last column on fw - 2", 3 * 22 + 2, 3 * 11, 3, shift(2, -0.5), want=22 * 11)
        return out
    return _once("edges", build)


def edge_model(c):
    return _once(("edge model", c["what"]), lambda: X.sums_int(c["A"], c["B"], c["H"], stride=c["stride"], lo=c["lo"], hi=c["hi"]))


# ---- C: the solve ----
P28 = 2 ** 28
# Inputs that end NM_EXPOSURE_END_SINGULAR: dict(n, la, lb, S, sn, sg, ends = (end in PER_CHANNEL mode, end in COMMON mode)).
# The first two are written by hand: equal means make the 2 x 2 matrix exactly singular once wg = N / sg^2 = 1e-9 is lost
# beside wn abar^2 = 4.9e16 (first): the chain of pivot 1 ends at -6.6; in the second channel B (means 100) solves and
# channel G (means 7) fails, and the COMMON system (means 69) passes its pivots. In the third the chain of pivot 1 ends at
# exactly 0.0, the one value at which `v > 0` and `v >= 0` differ. The other three were kept from a seeded search
# over n in 2 .. 4, L in 1 .. 5, sigma_n in 1e-6 .. 1e-1, sigma_g in 10 .. 1e6 with sums N m, m whole byte means: there the
# failing pivot is not the last row (a replica of the written chains in exact arithmetic names it).
SINGULAR = [
    dict(n=2, la=[0], lb=[1], S=[[1000, 7000, 7000, 7000, 7000, 7000, 7000]], sn=1e-6, sg=1e6, ends=(2, 2)),
    dict(n=2, la=[0], lb=[1], S=[[1000, 100000, 7000, 100000, 100000, 7000, 100000]], sn=1e-6, sg=1e6, ends=(2, 0)),
    dict(n=2, la=[1], lb=[0], S=[[64, 6400, 6400, 6400, 6400, 6400, 6400]], sn=1e-6, sg=1e6, ends=(2, 2)),
    # pivot 2 of 4 fails, in channel G after B solved (PER_CHANNEL) and in the one system (COMMON)
    dict(n=4, la=[2, 0, 3], lb=[1, 3, 0],
         S=[[8985, 0, 1868880, 1617300, 0, 1868880, 1617300], [78827, 7725046, 3941350, 15765400, 7725046, 3941350, 15765400],
            [85755, 4802280, 7717950, 8918520, 4973790, 9776070, 14921370]],
         sn=1.1517088253155347e-05, sg=37403.46310336091, ends=(2, 2)),
    # pivot 1 of 3 fails in channel B; frame 2 has no link and its row comes after the failure
    dict(n=3, la=[0], lb=[1], S=[[63883, 2108139, 15970750, 11754472, 9071386, 2619203, 15204154]],
         sn=2.752481954049149e-06, sg=318329.00067886856, ends=(2, 2)),
    # pivot 3 of 4 fails in channel B and pivot 2 in the COMMON system, both links reversed (a > b)
    dict(n=4, la=[3, 2], lb=[1, 0],
         S=[[65232, 2022192, 326160, 3848688, 2022192, 326160, 3848688], [32936, 2634880, 3721768, 1877352, 2634880, 3721768, 1877352]],
         sn=0.00017274823186956984, sg=214342.95579519047, ends=(2, 2)),
]
# The corners of the sigma range at the largest lattice, bytes 0 / 255: n = 3, links (0, 1) and (1, 2)
CORNER_SUMS = ([P28] + [255 * P28] * 6, [P28, 0, 0, 0] + [255 * P28] * 3)
CORNER_SIGMAS = [(sn, sg) for sn in (1e-6, 1e6) for sg in (1e-6, 1e6)]
CORNER_ENDS = {0: (0, 2, 0, 0), 1: (0, 0, 0, 0)}          # per CORNER_SUMS entry, in CORNER_SIGMAS order, both modes alike


def gain_bound_holds(sigma_n, sigma_g, n, L):
    """The condition under which exposure_ref.gain_bound is asserted against solve_f64: its conditioning term, relative,
    kappa 2^-53 (4 n (3 n + 1) + L + 4), stays below the float32 rounding 2^-24 that the bound is built around."""
    return X.kappa(sigma_n, sigma_g) * 2.0 ** -53 * (4 * n * (3 * n + 1) + L + 4) < 2.0 ** -24


SIGMA_PAIRS = [(1.0, 0.25), (1e-3, 2e-4), (100.0, 0.01)]       # non-default, inside gain_bound_holds for n = 64, L = 256


def usability_cases():
    """dict(what, n, la, lb, S, kw, usable (per link), gains_one (frames whose gain must be exactly 1))"""
    m = [90, 100, 110, 99, 90, 121]

    def s(N):
        return [N] + [N * v for v in m]
    out = []
    for mp, N, ok in ((64, 64, True), (64, 63, False), (1, 0, False), (1, 1, True), (1000, 1000, True), (1000, 999, False)):
        # link 0 is the one at the boundary; link 1 joins frames 1 and 2 and is always usable
        out.append(dict(what="N %d against min_pixels %d" % (N, mp), n=3, la=[0, 1], lb=[1, 2], S=[s(N), s(5000)],
                        kw=dict(min_pixels=mp), usable=[ok, True], gains_one=[] if ok else [0]))
    for st in (2, -1, 0):
        out.append(dict(what="link_status %d" % st, n=3, la=[0, 1], lb=[1, 2], S=[s(5000), s(5000)],
                        kw=dict(link_status=np.array([st, 1], np.int32)), usable=[False, True], gains_one=[0]))
    # frame 3's only links are unusable: one by its count, one by its status
    out.append(dict(what="a frame whose only links are unusable", n=5, la=[0, 3, 1, 3, 2], lb=[1, 0, 2, 4, 4],
                    S=[s(4000), s(10), s(3000), s(7000), s(2000)], kw=dict(link_status=np.array([1, 1, 1, 0, 1], np.int32)),
                    usable=[True, False, True, False, True], gains_one=[3]))
    return out


def graph_cases():
    """dict(what, n, la, lb, S): shapes of the link graph at n = 64 that stress the row assembly"""
    def build():
        rng = np.random.default_rng(64)
        t = rng.uniform(0.8, 1.25, (64, 3))

        def sums(la, lb, zero=False):
            S = []
            for a, b in zip(la, lb):
                N = int(rng.integers(500, 40000))
                mean = rng.uniform(60, 160, 3)
                S.append([N] + [0 if zero else int(round(N * mean[c] * t[a, c])) for c in range(3)] +
                         [0 if zero else int(round(N * mean[c] * t[b, c])) for c in range(3)])
            return S
        out = []

        def add(what, la, lb, **kw):
            out.append(dict(what=what, n=64, la=list(la), lb=list(lb), S=sums(la, lb, **kw)))
        add("256 copies of link (3, 9)", [3] * 256, [9] * 256)
        add("a star on frame 0", [0] * 63, range(1, 64))
        add("two live frames, 62 dead", [40], [17])
        add("256 links reversed", [1 + l % 63 for l in range(256)], [(l % 63) * (l // 63) // 4 for l in range(256)])
        add("Sa = Sb = 0", [l % 64 for l in range(256)], [(l + 1 + l // 64) % 64 for l in range(256)], zero=True)
        return out
    return _once("graphs", build)
