"""The cases of tests/test_link_edges_host.py and tests/test_gpu_link_edges.py: the link stages (verification, direct
refinement, vote scan) at the edges their own constants define. It does not call the library.

Every builder takes `T`, a namespace with the helpers frame, smooth, moved and disc of tests/test_link_refine_host.py, and
returns dicts; each dict carries the INTENDED lattice (lw, lh, tiles_x, tiles), which the tests compare with `lattice_of`
(the entry points' formulas) before anything else, so that a case that is not the edge it claims to be fails.

walk_cases      A  the tile walk: 255, 256, 257 (along a row and down a column), 256 at the widest and 512 at the tallest frame
                   the ABI admits, three pairs each; and 16385 x 3, the 257-tile row on which the refinement has pixels
interior_cases  B  lattices of 63 / 64 / 65 / 128 / 129 columns by 31 / 32 / 33 rows at stride 1; at stride 3 with and without
                   remainder columns and rows beside the last tile
extreme_cases   C  1 x 1 .. 2 x 2 (no sample possible), 3 x 3 and 65 x 3 (the smallest with samples), stride == fw, stride == fh,
                   a lattice empty in x only, and in y only
horizon_cases   D  maps whose denominator changes sign inside the frame, with den == 0 exactly at lattice pixels
gate_cases      E  the verification's gates at, below and above their thresholds
vote_cases      F  the vote scan for 17, 33 and 63 frames at caps of 65 and 257 rows
"""
import numpy as np

import link_propose_ref as P
import link_refine_ref as R
import link_verify_ref as V

F32 = np.float32
TILE_W, TILE_H, PARTS = 64, 32, 256          # csrc/nm_link_verify.hip, csrc/nm_link_refine_math.hpp
_CACHE = {}


def _once(key, build):
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def lattice_of(fw, fh, stride):
    """(lw, lh, tiles_x, tiles) by the formulas of nm_link_verify_batch_dev_f32 and nm_link_refine_batch_dev_f32"""
    lw, lh = fw // stride, fh // stride
    tiles_x = -(-lw // TILE_W)
    return lw, lh, tiles_x, tiles_x * -(-lh // TILE_H)


def translation(tx, ty):
    return np.array([1, 0, tx, 0, 1, ty, 0, 0, 1], F32)


def textured(T, seed, fw, fh):
    """A smooth pattern plus seeded noise (the frames of tests/test_gpu_link_refine.py), values inside [0, 255]"""
    return (0.5 * T.frame(seed, fw, fh) + 0.5 * T.smooth(fw, fh, 3.0 * seed, seed)).astype(F32)


def shifted(A, dx, dy):
    """T.moved for any whole shift: B(x + dx, y + dy) = 1.1 A(x, y) + 5 (rolled, so every pixel of B has a value)"""
    return np.clip(1.1 * np.roll(A, (dy, dx), (0, 1)) + 5, 0, 255).astype(F32)


# ---- A: the tile walk ----
# (fw, fh, stride), the intended (lw, lh, tiles_x, tiles), B's shift (dx, dy), the map's translation near it, and whether
# the refinement can have pixels. With fh = 2 only j = 0 passes j + 1 < fh, so the vertical translation lies in (-1, 0]:
# lattice row 1 samples between B's two rows, row 0 falls above B. The refinement needs (x, y - 1) and (x, y + 1) inside A
# as well, which no pixel of a frame of two rows has: there its N is 0 by definition and the walk shows in L alone.
WALK = [
    ((16320, 2, 1), (16320, 2, 255, 255), (2, 0), (2.3, -0.5), False),      # one below the limit
    ((16384, 2, 1), (16384, 2, 256, 256), (2, 0), (2.3, -0.5), False),      # workgroups == tiles, nothing wraps
    ((16385, 2, 1), (16385, 2, 257, 257), (2, 0), (2.3, -0.5), False),      # workgroup 0 owns two tiles, the last 1 column wide
    ((64, 8193, 1), (64, 8193, 1, 257), (2, 1), (2.3, 0.8), True),          # the same down a column, the last 1 row high
    ((32767, 4, 2), (16383, 2, 256, 256), (2, 0), (2.3, -0.5), True),       # the widest frame; the last tile 63 columns
    ((4, 32767, 2), (2, 16383, 1, 512), (0, 1), (-0.4, 0.8), True),         # the tallest; every workgroup owns two tiles
    ((16385, 3, 1), (16385, 3, 257, 257), (2, 0), (2.3, 0.0), True),        # 257 along a row with refinement pixels (row 1)
]
# the refinement's three pairs start this far (pixels, along x) from B's shift: END_CONVERGED after a few steps, END_STEP at
# once (the first step is above MAX_STEP), END_ITERATIONS (every step between 2^-7 and MAX_STEP)
OFFSETS, MAX_STEP = (0.3, 6.0, 4.0), 3.0


def walk_cases(T):
    def build():
        out = []
        for (fw, fh, stride), (lw, lh, tiles_x, tiles), (dx, dy), (tx, ty), counts in WALK:
            As = [textured(T, 3 + k, fw, fh) for k in range(3)]
            Bs = [T.moved(A) if (dx, dy) == (2, 1) else shifted(A, dx, dy) for A in As]
            H = np.stack([translation(tx, ty), translation(tx + 0.5, ty), translation(tx - 0.2, ty)])
            starts = np.stack([translation(dx + off, ty if fh < 8 else dy) for off in OFFSETS])
            # 16385 x 3 and 32767 x 4 have one row of refinement pixels, 4 x 32767 one column: X or Y is constant there, and
            # only the translation is determined
            out.append(dict(what="%d x %d stride %d" % (fw, fh, stride), fw=fw, fh=fh, stride=stride, lw=lw, lh=lh,
                            tiles_x=tiles_x, tiles=tiles, As=As, Bs=Bs, H=H, starts=starts, refine_counts=counts,
                            model=R.TRANSLATION if min(fw, fh) < 8 else R.HOMOGRAPHY))
        return out
    return _once("walk", build)


# ---- B: tile interior edges ----
def interior_cases(T):
    """Every shape without a mask; every second one under the disc as well (a mask hides the lattice's last column and row,
    so the unmasked run is the one that sees the guards)."""
    def build():
        shapes = [(lw, lh, 1, lw, lh) for lw in (63, 64, 65, 128, 129) for lh in (31, 32, 33)]
        shapes += [(3 * lw + r, 3 * lh + r, 3, lw, lh) for r in (0, 2) for lw in (64, 65) for lh in (32, 33)]
        out = []
        for k, (fw, fh, stride, lw, lh) in enumerate(shapes):
            A = textured(T, 20 + k, fw, fh)
            tiles_x = -(-lw // TILE_W)
            for masked in ((False, True) if k % 2 else (False,)):
                out.append(dict(what="%d x %d stride %d%s" % (fw, fh, stride, " masked" if masked else ""), fw=fw, fh=fh,
                                stride=stride, lw=lw, lh=lh, tiles_x=tiles_x, tiles=tiles_x * -(-lh // TILE_H), A=A, B=T.moved(A),
                                H=translation(2.3, 0.8), mask=T.disc(fw, fh) if masked else None))
        return out
    return _once("interior", build)


# ---- C: frame extremes ----
def extreme_cases(T):
    """kind: "none" (no pixel can have its taps inside B: N = 0, L > 0), "some" (N > 0), "empty" (no lattice: tiles = 0)"""
    def build():
        out = []

        def add(fw, fh, stride, kind, moved):
            A = textured(T, 40 + len(out), fw, fh)
            lw, lh, tiles_x, tiles = lattice_of(fw, fh, stride)
            out.append(dict(what="%d x %d stride %d" % (fw, fh, stride), fw=fw, fh=fh, stride=stride, lw=lw, lh=lh, tiles_x=tiles_x,
                            tiles=tiles, kind=kind, A=A, B=T.moved(A) if moved else A,
                            H=translation(2.3, 0.8) if moved else translation(0, 0)))
        for fw, fh in ((1, 1), (1, 7), (7, 1), (2, 2)):
            add(fw, fh, 1, "none", False)
        add(3, 3, 1, "some", False)
        add(65, 3, 1, "some", False)
        add(40, 90, 40, "some", True)                                   # stride == fw: lw = 1
        add(90, 40, 40, "some", True)                                   # stride == fh: lh = 1
        add(40, 90, 64, "empty", True)                                  # lw = 0, lh = 1
        add(90, 40, 64, "empty", True)                                  # lw = 1, lh = 0
        return out
    return _once("extreme", build)


# ---- D: the horizon through the frame ----
def horizon_cases(T):
    """96 x 40 at stride 1. zeros: lattice pixels with den == 0 exactly (all three denominators are exact in fp32)."""
    def build():
        fw, fh = 96, 40
        A, B = textured(T, 60, fw, fh), textured(T, 61, fw, fh)
        maps = (("den = 1 - x / 32", [1, 0, 0, 0, 1, 0, -1 / 32, 0, 1], 40),
                ("den = x / 32 - 1", [1, 0, 0, 0, 1, 0, 1 / 32, 0, -1], 40),
                ("den = 1 - x / 64 - y / 32", [1, 0, 0, 0, 1, 0, -1 / 64, -1 / 32, 1], 33))     # x = 64 - 2 y, y = 0 .. 32
        return [dict(what=what, fw=fw, fh=fh, stride=1, A=A, B=B, H=np.array(H, F32), zeros=zeros) for what, H, zeros in maps]
    return _once("horizon", build)


# ---- E: gates at, below and above ----
def gate_cases(T):
    """Calls of the verification: dict(what, As, Bs, H, kw, bit, want) with want[k] = whether `bit` is set in reason[k]."""
    def build():
        out = []
        A = textured(T, 70, 64, 48)
        I = translation(0, 0)
        out.append(dict(what="inliers at, below, above min_inliers", As=[A] * 3, Bs=[A] * 3, H=np.stack([I] * 3),
                        kw=dict(stride=3, min_inliers=12, inliers=[12, 11, 13], min_overlap=0.5, min_ncc=0.5), bit=V.FEW_INLIERS,
                        want=[False, True, False], only=True))
        A = textured(T, 71, 64, 32)
        four, below = 4.0, float(np.nextafter(F32(4), F32(0)))
        for scale, r in ((2.0, 4.0), (0.5, 0.25)):                      # r = 4 and 1 / 4 exactly: power-of-two sides
            H = np.array([scale, 0, 0, 0, scale, 0, 0, 0, 1], F32)
            for ratio, want in ((four, False), (below, True)):
                out.append(dict(what="area ratio %g against max_area_ratio %.9g" % (r, ratio), As=[A], Bs=[A], H=H[None],
                                kw=dict(stride=1, max_area_ratio=ratio), bit=V.BAD_GEOMETRY, want=[want], only=False))
        B, H = T.moved(A), translation(2.3, 0.8)
        L, N = V.sums_int(A, B, H, None, 1)[:2]
        assert L == 2048 and 0 < N < L and float(F32(N / 2048)) == N / 2048       # N / L is exact in float32
        at = float(F32(N / 2048))
        for mo, want in ((at, False), (float(np.nextafter(F32(at), F32(2))), True)):
            out.append(dict(what="overlap %d / 2048 against min_overlap %.9g" % (N, mo), As=[A], Bs=[B], H=H[None],
                            kw=dict(stride=1, min_overlap=mo, min_ncc=-1.0), bit=V.LOW_OVERLAP, want=[want], only=True))
        flat = np.full_like(A, 100)                                     # vb = 0: ncc = 0.0 by definition
        for mn, want in ((0.0, False), (float(np.nextafter(F32(0), F32(1))), True)):
            out.append(dict(what="ncc 0 against min_ncc %.9g" % mn, As=[A], Bs=[flat], H=I[None],
                            kw=dict(stride=1, min_overlap=0.5, min_ncc=mn), bit=V.LOW_NCC, want=[want], only=True))
        return out
    return _once("gates", build)


# ---- F: votes for mid-sized n ----
VOTE_SHAPES = ((17, 257), (33, 257), (33, 65), (63, 65))


def vote_cases():
    """dict(what, descs, counts, cap, amb): the counts cycle through P.COUNTS below cap, cap, cap + 5 (which the entry clips)."""
    def build():
        out = []
        for n, cap in VOTE_SHAPES:
            vals = [c for c in P.COUNTS if c < cap] + [cap, cap + 5]
            counts = [vals[k % len(vals)] for k in range(n)]
            assert {0, cap, cap + 5} <= set(counts)
            out.append(dict(what="n %d cap %d" % (n, cap), descs=P.world_frames(100 * n + cap, n, cap), counts=counts, cap=cap, amb=0.8))
        return out
    return _once("votes", build)


def model_votes(c):
    return _once("model votes " + c["what"], lambda: P.votes(c["descs"], c["counts"], c["cap"], c["amb"]))
