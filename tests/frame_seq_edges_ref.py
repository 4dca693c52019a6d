"""Inputs and conditions of the edge tests of the three frame-sequence stages: frame weights across the row pass's chunk
seams, frame quality at the size its sums were dimensioned for, the KLT sums at theirs, the tracker's launch split and the
pyramid shapes no other test runs. TEST INFRASTRUCTURE ONLY. Every input is built by design, none is drawn; the models are
those of frame_weights_ref, frame_quality_ref and klt_ref. tests/test_frame_seq_edges_host.py runs the host twins against
the models on these inputs and asserts the conditions; tests/test_gpu_frame_seq_edges.py runs the device against the host
twins."""
import numpy as np

import frame_quality_ref as FQ
import frame_weights_ref as FW
import klt_ref as K

F32 = np.float32

# ---- A. frame weights: the row pass cuts a row into chunks of 32 blocks of 64 pixels --------------------------------------
CHUNK = 32 * 64
SEAMS = (CHUNK, 2 * CHUNK, 3 * CHUNK)
WIDTHS = (2048, 2049, 2112, 4097, 7681)         # one chunk (control); 1 px, one block, and 2 chunks + 1 px; 3 chunks + 25 blocks
HEIGHTS = (3, 9, 17)                            # one strip; the strip seam between rows 7 and 8; two strips and a third's row
FW_SHAPES = [(w, h) for w in WIDTHS for h in HEIGHTS]
FW_RADII = (1, 8, 31, 64)
# what is planted at a seam s, as (dx, dy) offsets from (s, centre row): the single pixels in three sets that keep them
# single (with s - 1 alone the right chunk's g comes from the left chunk's seed, with s alone the left chunk's from the
# right's), and the 2 x 2 and 3 x 3 clusters centred on s - 1 and on s (a 2 x 2 cluster "centred on c" is columns c - 1, c)
KINDS = (
    [(-64, 0), (-2, 0), (1, 0), (64, 0)],
    [(-1, 0), (63, 0)],
    [(0, 0)],
    [(dx - 1, dy) for dx in (-1, 0) for dy in (0, 1)],
    [(dx, dy) for dx in (-1, 0) for dy in (0, 1)],
    [(dx - 1, dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1)],
    [(dx, dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1)],
)


def seams_of(fw):
    return [s for s in SEAMS if s < fw]


def plant(f, kind, s, row, shift=0):
    """the raw-bad pixels of KINDS[kind] round column s + shift and row `row`, clipped to the frame; dark and saturated
    pixels alternate"""
    fh, fw = f.shape[:2]
    for i, (dx, dy) in enumerate(KINDS[kind]):
        x, y = s + shift + dx, row + dy
        if 0 <= x < fw and 0 <= y < fh:
            f[y, x, :3] = 0 if (i + kind) & 1 else 255
            f[y, x, i % 3] = 3 if (i + kind) & 1 else 250       # max(B, G, R) decides, not one channel


def centre_rows(fh, late):
    """centre rows of the planted bands: row 1, and from nine rows on row 7 (the last of strip 0; `late`: row 8, the first
    of strip 1), and row 13 of 17"""
    return [1] if fh < 9 else [1, 8 if late else 7] + ([13] if fh > 14 else [])


def seam_frames(fw, fh):
    """Mid-gray frames of fw x fh (nothing raw-bad at FW.LO / FW.HI) with planted raw-bad pixels at every seam (and, in the
    one-chunk control, at the frame's right edge): frame v holds kind (v + band) % 7 at its band of rows, so that seven
    frames put every kind at every band; frames 7 .. 13 (from nine rows on) have the second band on row 8 instead of row 7. Then
    one frame of FW.frames_for. Built once per shape, never changed by a test."""
    key = (fw, fh)
    if key not in _SEAM_FRAMES:
        out = []
        for v in range(7 if fh < 9 else 14):
            f = FW.blank(fw, fh)
            f[..., 3] = (np.arange(fw) * 7 + v) % 256                              # alpha must play no part
            for s in (seams_of(fw) or [fw]):
                for band, row in enumerate(centre_rows(fh, v >= 7)):
                    plant(f, (v + band) % 7, s, row)
            out.append(f)
        out.append(FW.frames_for(fw, fh)[2])
        _SEAM_FRAMES[key] = out
    return _SEAM_FRAMES[key]


_SEAM_FRAMES = {}


def seam_bases(fw, fh):
    """[None, a base plane whose columns s - 1 and s are zero at every seam, one where column s - 1 is zero on rows 0 and 1
    of every four and column s on rows 1 and 2: there a row's only seed lies across the seam]"""
    y, x = np.mgrid[0:fh, 0:fw]
    full = (1 + (x * 7 + y * 13) % 255).astype(np.uint8)
    part = full.copy()
    for s in (seams_of(fw) or [fw]):
        full[:, s - 1] = 0
        part[(y[:, 0] % 4) < 2, s - 1] = 0
        if s < fw:
            full[:, s] = 0
            part[((y[:, 0] % 4) == 1) | ((y[:, 0] % 4) == 2), s] = 0
    return [None, full, part]


def fw_configs(shape_index, radii=FW_RADII):
    """the twelve (R, min_count) pairs; border, base (index into seam_bases), mask format and margin rotate over them and
    over the shapes, so that every value meets every radius and every min_count"""
    out, case = [], shape_index
    for R in radii:
        for min_count in FW.MIN_COUNTS:
            m = FW.margins(R)
            out.append(dict(lo=FW.LO, hi=FW.HI, R=R, min_count=min_count, border=bool(case & 1), base=(case // 2) % 3,
                            mask_format=(FW.U8N, FW.TEX_F32)[(case // 3) % 2], margin=m[case % len(m)]))
            case += 1
    return out


def with_base(kw, bases):
    return dict(kw, base=bases[kw["base"]])


def seam_dependence(frame, s, min_count, R=8):
    """(left, right): whether dist2 of the whole frame differs, on the chunk left (right) of seam s, from dist2 of that
    chunk's columns alone. Without border, so that only data from across the seam can make the difference."""
    fw = frame.shape[1]
    kw = dict(lo=FW.LO, hi=FW.HI, R=R, min_count=min_count, border=False)
    whole = FW.model(frame, **kw)["dist2"]
    lo, hi = s - CHUNK, min(s + CHUNK, fw)
    left = FW.model(np.ascontiguousarray(frame[:, lo:s]), **kw)["dist2"]
    right = FW.model(np.ascontiguousarray(frame[:, s:hi]), **kw)["dist2"]
    return not np.array_equal(whole[:, lo:s], left), not np.array_equal(whole[:, s:hi], right)


def assert_seam_dependence(fw, fh):
    """for every seam below the width and each side of it: the single pixel at s - 1 decides on the right and the one at s
    on the left at min_count 1; the 2 x 2 cluster on columns s - 1 and s at min_count 4 and the 3 x 3 cluster on columns
    s - 2 .. s at min_count 7 make a seed only with the raw-bad bits of both sides (a side alone holds at most 2 and 6)"""
    frames = seam_frames(fw, fh)
    for s in seams_of(fw):
        assert seam_dependence(frames[1], s, 1)[1] and seam_dependence(frames[2], s, 1)[0], (fw, fh, s, "singles")
        assert seam_dependence(frames[4], s, 4) == (True, True), (fw, fh, s, "2 x 2")
        assert seam_dependence(frames[5], s, 7) == (True, True), (fw, fh, s, "3 x 3")


def batch_frames():
    """64 frames of 2112 x 9, a different pattern each: kind k % 7 at a row and a column shift that change with k"""
    if not _BATCH:
        for k in range(64):
            f = FW.blank(2112, 9)
            plant(f, k % 7, CHUNK, 1 + (3 * k) % 7, k // 7 - 4)
            plant(f, (k + 3) % 7, 2112, (5 * k) % 9)
            _BATCH.append(f)
    return _BATCH


_BATCH = []

# ---- B. frame quality ---------------------------------------------------------------------------------------------------------
L2_MAX = 1020 * 1020                            # measure's L2 at a saturated checkerboard: L = +-4 * 255
G2_MAX = 2 * 255 * 255                          # measure's G2 when both central differences are +-255
WAVE_BOUND = 64 * 32 * L2_MAX                   # the static_assert of nm_frame_quality.hip: 2 130 739 200 = 0.992 * 2^31


def bgra(Y):
    """a BGRA frame whose three colours are all Y (so luma is Y), alpha varying"""
    Y = np.asarray(Y, np.uint8)
    f = np.repeat(Y[..., None], 4, axis=-1)
    f[..., 3] = (np.arange(Y.shape[1]) * 5 % 256).astype(np.uint8)[None, :]
    return np.ascontiguousarray(f)


def checker(fw, fh, block=1, phase=0):
    """0 / 255 squares of `block` pixels. block 1 maximises the squared Laplacian at every measured pixel, block 2 the
    squared gradient (Y(x + 1) - Y(x - 1) and Y(y + 1) - Y(y - 1) are both +-255 everywhere)"""
    y, x = np.mgrid[0:fh, 0:fw]
    return bgra(255 * (((x // block) + (y // block) + phase) & 1))


def stripes(fw, fh):
    """columns 0 0 255 255: the horizontal difference is +-255, the vertical one 0"""
    y, x = np.mgrid[0:fh, 0:fw]
    return bgra(255 * ((x // 2) & 1))


def quality_variants(fw=130, fh=70):
    """64 frames: the saturated checkerboard in both phases and block sizes, each with a flat mid-gray rectangle whose place
    and size change with k (every pixel stays measured, its Laplacian and gradient do not), some with a black or a white one"""
    out = []
    for k in range(64):
        f = checker(fw, fh, 1 + (k // 2) % 2, k & 1)
        f[k % 50:k % 50 + 5 + k % 11, (3 * k) % 60:(3 * k) % 60 + 8 + k, :3] = 128
        if k % 8 == 5:
            f[5:20, 2 * k - 10:2 * k + 3, :3] = 0
        if k % 8 == 7:
            f[fh - 12:, k:k + 40, :3] = 255
        out.append(f)
    return out


def cross_masks(fw, fh, fmt):
    """one mask that removes the middle row and the middle column, in the given format"""
    m = np.ones((fh, fw), bool)
    m[fh // 2, :] = m[:, fw // 2] = False
    return np.where(m, 255, 0).astype(np.uint8) if fmt == FQ.U8N else np.where(m, 1, 0).astype(F32)


def shift_chain(n):
    return np.stack([FQ.translation(-float(k)) for k in range(n)])


def big_stats(n=12):
    """hand-written statistics on 2 x 2 cells whose words 0 and 3 are of the size of 2^40: scores are exact small integers,
    and some differ only below fp32's precision of the sums"""
    s = np.zeros((n, 2, 2, 8), np.uint64)
    big = np.uint64(1 << 40)
    for k in range(n):
        for c in range(4):
            m = big + np.uint64(977 * k + 31 * c)
            s[k, c // 2, c % 2, 0] = m
            s[k, c // 2, c % 2, 1] = m * np.uint64(100)
            s[k, c // 2, c % 2, 3] = m * np.uint64(1000 + (7 * k + 3 * c) % 11) + np.uint64(k == 5)
            s[k, c // 2, c % 2, 7] = m
    return s


def tied_stats(n=12):
    """every cell of every frame holds 2^40 measured pixels and the sharpness 7: the walk's and the median's tie order"""
    s = np.zeros((n, 2, 2, 8), np.uint64)
    s[..., 0] = s[..., 7] = 1 << 40
    s[..., 1] = 100 << 40
    s[..., 3] = 7 << 40
    return s


PICK_KW = dict(d_min=2.0, d_max=4.0, rel=0.5, w=2, cell_min=64, min_pixels=1024)

def pick_inputs(nm):
    """name -> (stats, chain, keep, kw): the statistics of (a) to (d) and the two hand-written tables"""
    one = lambda f, grid=(1, 1): nm.frame_quality_host(f, lo=0, hi=255, grid=grid)
    abc = np.concatenate([one([checker(192, 160)]), one([checker(1920, 1080)]), one([checker(192, 160, 2)]),
                          one([stripes(192, 160)]), one([checker(192, 160, 1, 1)])])
    out = {"a, b and c on one cell": (abc, shift_chain(5), 5, dict(PICK_KW, d_min=1.0, d_max=2.0, rel=0.0))}
    for grid in ((1, 1), (8, 8)):
        out["d on %d x %d cells" % grid] = (one(quality_variants(), grid), shift_chain(64), 64, PICK_KW)
    out["words of 2^40"] = (big_stats(), shift_chain(12), 12, dict(PICK_KW, rel=0.998, w=3))
    out["all scores equal"] = (tied_stats(), shift_chain(12), 8, PICK_KW)
    return out


# ---- C. KLT -------------------------------------------------------------------------------------------------------------------
KW_, KH_ = 97, 61
UNIT2 = 4080 * 4080                             # the square of the largest difference of two levels


def blocks(w=KW_, h=KH_):
    """0 / 255 squares of two pixels (period 4 along both axes): at a whole-pixel point every tap has gx = +-4080 and
    gy = +-4080, so Gxx = Gyy = (2r + 1)^2 * 4080^2 (3.75e9 at radius 7), while gx gy alternates in sign from tap to tap
    and Gxy = +-4080^2: det > 0"""
    y, x = np.mgrid[0:h, 0:w]
    return (255 * (((x >> 1) + (y >> 1)) & 1)).astype(F32)


def klt_pairs():
    """name -> (A, B): B is A moved by whole pixels, and in the last the inverse of that"""
    A = blocks()
    return {"one right": (A, K.shifted(A, 1, 0)), "one down": (A, K.shifted(A, 0, 1)),
            "the inverse, one right": (A, (F32(255) - K.shifted(A, 1, 0)).astype(F32))}


def klt_points(r=7):
    """whole-pixel points of both parities well inside the frame, then the quarter-pixel grid points of klt_ref"""
    xs = [20, 21, 22, 23, 40, 41, 48, 49, 60, 61]
    ys = [20, 21, 23, 22, 30, 31, 30, 33, 28, 29]
    gx, gy = K.grid_points(KW_, KH_, 14, r)
    return np.r_[np.array(xs, F32), gx], np.r_[np.array(ys, F32), gy]


MISMATCH_TAPS = 120                             # no window brings -bx or -by above 120 * 4080^2 = 1 997 568 000 < 2^31


def mismatch_row_bound(taps=15):
    """The largest value of -sum e gx over one row of `taps` taps, in units of 4080^2, by enumeration. With T the template's
    samples along the row (two more than taps), gx(u) = T(u + 1) - T(u - 1) and e(u) = B(u) - T(u) in [-T(u), 4080 - T(u)]
    whatever B holds, the sum is linear in every e(u) and, with each e(u) at an end of its range, linear in every T(u)
    alone: its maximum is reached with every T(u) at 0 or 4080. All 2^(taps + 2) such rows are tried."""
    n = taps + 2
    t = ((np.arange(1 << n)[:, None] >> np.arange(n)) & 1).astype(np.int64)
    g, c = t[:, 2:] - t[:, :-2], t[:, 1:-1]
    return int(np.maximum(np.maximum(c * g, (1 - c) * -g), 0).sum(axis=1).max())


def split_pairs(n):
    """the pairs either side of the split at slot 32 and the last one"""
    return sorted({k for k in (31, 32, n - 1) if k < n})


def split_case(n, capA=24):
    """n pairs over three pyramids of 97 x 61: which pyramids, a start map and a status per pair, a size per pair"""
    grays = [K.textured(1, 105, 69)[3:64, 5:102].copy(), K.textured(1, 105, 69)[2:63, 3:100].copy(), K.textured(1, 97, 61)]
    ia, ib = [k % 3 for k in range(n)], [(k + 1 + k // 3) % 3 for k in range(n)]
    nAs = [(5 * k + 3) % (capA + 4) for k in range(n)]
    for k in split_pairs(n):
        nAs[k] = capA - (k % 3)                                    # the pairs the test looks at singly hold rows
    H = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], F32), (n, 1))
    H[:, 2], H[:, 5] = (np.arange(n) % 7 - 3) * 0.5, (np.arange(n) % 5 - 2) * 0.25
    status = (np.arange(n) % 6 != 4).astype(np.int32)
    xs, ys = K.grid_points(97, 61, capA, 3)
    return dict(grays=grays, ia=ia, ib=ib, nAs=nAs, H=H, status=status, xs=xs, ys=ys, capA=capA,
                kw=dict(levels=3, radius=3, iterations=6, fb_max=1.5, max_residual=20.0, capA=capA))


# shapes no device test ran: 16-byte loads at level 0 only (100), at levels 0 and 1 (104), six levels, planes smaller than
# a tile and than the filter, a plane of many tiles a row
PYRAMIDS = [(100, 52, 3), (104, 56, 3), (130, 70, 6), (5, 7, 2), (33, 2, 1), (2, 2, 1), (2050, 20, 3)]


def pyramid_gray(fw, fh, seed=0):
    g = K.textured(fw * 131 + fh + seed, fw, fh, 0.0, 255.0)
    g[fh // 2, fw // 3] = np.nan
    return g


def pyramid_masks(fw, fh):
    """name -> mask: the dense one of the host test; single unseen pixels in every corner and on every edge; and two with a
    single unseen pixel, whose reach the top level must clamp at one border and not at the other"""
    ones = np.ones((fh, fw), F32)
    edges, corner, side = ones.copy(), ones.copy(), ones.copy()
    for x, y in ((0, 0), (fw - 1, 0), (0, fh - 1), (fw - 1, fh - 1), (fw // 2, 0), (fw // 2, fh - 1), (0, fh // 2), (fw - 1, fh // 2)):
        edges[y, x] = 0.0
    corner[fh - 1, fw - 1] = 0.5
    side[fh // 2, 0] = 0.0
    return {"dense": (K.textured(7, fw, fh, 0.0, 1.0) > 0.25).astype(F32), "corners and edges": edges, "one corner": corner,
            "one edge": side}
