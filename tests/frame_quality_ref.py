"""A numpy restatement of the frame-quality definitions of include/nm_abi.h ("Frame quality and keyframe choice"), not of the
kernels: Y, the good mask and the measured mask from shifted arrays, the sums as uint64 integers, the cells from index
arrays; score, flags and walk as plain Python loops over fp64 and fp32 numpy scalars, with invert3x3 and project restated from
the ABI text; the gather as fancy indexing. Also the inputs and cases that tests/test_frame_quality_host.py and
tests/test_gpu_frame_quality.py share."""
import numpy as np

F32, F64 = np.float32, np.float64
U8N, TEX_F32 = 0, 2
STATUS, FEW, BAD, BLURRED, KEY, JUMP = 1, 2, 4, 8, 16, 32
SHAPES = [(1, 1), (2, 5), (3, 3), (63, 5), (64, 64), (65, 9), (129, 70), (200, 150)]
LO, HI = 20, 235


def grids_for(fw, fh):
    g = [(1, 1), (min(2, fw), min(3, fh)), (min(8, fw), min(8, fh))]
    return g + ([(3, 1)] if fw == 3 else [])


# ---- statistics ---------------------------------------------------------------------------------------------------------------
def luma(f):
    f = f.astype(np.int64)
    return (7 * f[..., 0] + 72 * f[..., 1] + 21 * f[..., 2] + 50) // 100


def eligible(mask, shape):
    if mask is None:
        return np.ones(shape, bool)
    return mask >= 128 if mask.dtype == np.uint8 else mask > F32(0.5)


def classes(f, mask, lo, hi):
    mx = f[..., :3].max(axis=-1).astype(np.int64)
    el = eligible(mask, mx.shape)
    dark, bright = el & (mx < lo), el & (mx > hi)
    return el, dark, bright, el & ~dark & ~bright


def measured_of(good):
    m = np.zeros_like(good)
    if good.shape[0] > 2 and good.shape[1] > 2:
        m[1:-1, 1:-1] = good[1:-1, 1:-1] & good[1:-1, :-2] & good[1:-1, 2:] & good[:-2, 1:-1] & good[2:, 1:-1]
    return m


def stats_model(frames, masks=None, lo=0, hi=255, grid=(4, 4)):
    gx, gy = grid
    n, (fh, fw) = len(frames), frames[0].shape[:2]
    out = np.zeros((n, gy, gx, 8), np.uint64)
    cell = ((np.arange(fh) * gy) // fh)[:, None] * gx + ((np.arange(fw) * gx) // fw)[None, :]
    for k, f in enumerate(frames):
        Y = luma(f)
        el, dark, bright, good = classes(f, None if masks is None else masks[k], lo, hi)
        meas = measured_of(good)
        P = np.pad(Y, 1)
        L = P[1:-1, :-2] + P[1:-1, 2:] + P[:-2, 1:-1] + P[2:, 1:-1] - 4 * Y
        G2 = (P[1:-1, 2:] - P[1:-1, :-2]) ** 2 + (P[2:, 1:-1] - P[:-2, 1:-1]) ** 2
        words = [meas, Y * meas, Y * Y * meas, L * L * meas, G2 * meas, dark, bright, el]
        for q, w in enumerate(words):
            acc = np.zeros(gx * gy, np.uint64)
            np.add.at(acc, cell.ravel(), w.astype(np.uint64).ravel())
            out[k, :, :, q] = acc.reshape(gy, gx)
    return out


def frames_for(fw, fh, seed=0, n=3):
    """frames with texture, a dark and a bright patch, pixels at exactly LO and HI, and one flat frame"""
    rng = np.random.default_rng(1000 * seed + 7 * fw + fh)
    out = []
    for k in range(n):
        f = rng.integers(LO + 1, HI, (fh, fw, 4), dtype=np.uint8)
        if k == 1:
            f[..., :3] = (f[..., :3].astype(np.int32) // 4 + 90).astype(np.uint8)          # low contrast
        f[rng.integers(0, fh), rng.integers(0, fw), :3] = (LO, LO - 1, 3)                   # max exactly LO: not dark
        f[rng.integers(0, fh), rng.integers(0, fw), :3] = (HI, 7, HI - 1)                   # max exactly HI: not bright
        f[rng.integers(0, fh), rng.integers(0, fw), :3] = (LO - 1, 0, 5)                    # dark
        f[rng.integers(0, fh), rng.integers(0, fw), :3] = (3, HI + 1, 9)                    # bright
        if fh > 8 and fw > 8:
            f[fh // 2:fh // 2 + 3, 1:4, :3] = 255
            f[1:3, fw - 4:fw - 1, :3] = 2
        out.append(f)
    return out


def masks_for(fw, fh, fmt, n=3, seed=0):
    rng = np.random.default_rng(77 + seed + fw * 3 + fh)
    out = []
    for k in range(n):
        if fmt == U8N:
            m = rng.choice(np.array([0, 127, 128, 255], np.uint8), (fh, fw), p=[0.1, 0.1, 0.3, 0.5])
        else:
            m = rng.choice(np.array([0.0, 0.5, np.nextafter(F32(0.5), F32(1)), 1.0], F32), (fh, fw), p=[0.1, 0.1, 0.3, 0.5])
        out.append(np.ascontiguousarray(m))
    return out


# ---- the choice ---------------------------------------------------------------------------------------------------------------
def fmaf(a, b, c):
    """fp32 fused multiply-add, exactly rounded: the product is exact in fp64, the sum's rounding error comes from TwoSum and
    decides the one case in which rounding twice differs (the fp64 sum lies on an fp32 tie)"""
    p, c = float(a) * float(b), float(c)
    s = p + c
    if not np.isfinite(s):
        return F32(s)
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = F32(s)
    if e != 0.0 and float(r) != s:
        other = np.nextafter(r, F32(np.inf) if s > float(r) else F32(-np.inf))
        if abs(s - float(r)) == abs(float(other) - s):
            hi_, lo_ = (other, r) if float(other) > float(r) else (r, other)
            r = hi_ if e > 0 else lo_
    return r


def invert3x3(t):
    t = [F32(v) for v in t]
    c0 = fmaf(t[4], t[8], -(t[7] * t[5]))
    c1 = fmaf(t[3], t[8], -(t[5] * t[6]))
    c2 = fmaf(t[3], t[7], -(t[4] * t[6]))
    det = fmaf(t[2], c2, fmaf(t[0], c0, -(t[1] * c1)))
    with np.errstate(all="ignore"):
        inv = F32(1) / det
        return [c0 * inv, fmaf(t[2], t[7], -(t[1] * t[8])) * inv, fmaf(t[1], t[5], -(t[2] * t[4])) * inv,
                fmaf(t[5], t[6], -(t[3] * t[8])) * inv, fmaf(t[0], t[8], -(t[2] * t[6])) * inv,
                fmaf(t[3], t[2], -(t[0] * t[5])) * inv, fmaf(t[3], t[7], -(t[6] * t[4])) * inv,
                fmaf(t[6], t[1], -(t[0] * t[7])) * inv, fmaf(t[0], t[4], -(t[3] * t[1])) * inv]


def project(m, x, y):
    """(x', y', denominator)"""
    m, x, y = [F32(v) for v in m], F32(x), F32(y)
    with np.errstate(all="ignore"):
        a = fmaf(m[0], x, m[1] * y) + m[2]
        b = fmaf(m[3], x, m[4] * y) + m[5]
        s = fmaf(m[6], x, m[7] * y) + m[8]
        return a / s, b / s, s


def motion(Ma, Mb, fw, fh):
    W = invert3x3(Ma)
    d = F32(0)
    with np.errstate(all="ignore"):
        for cx, cy in ((0, 0), (fw - 1, 0), (0, fh - 1), (fw - 1, fh - 1)):
            px, py, s1 = project(W, cx, cy)
            qx, qy, s2 = project(Mb, px, py)
            ex, ey = abs(qx - F32(cx)), abs(qy - F32(cy))
            if not (s1 > 0) or not (s2 > 0) or not np.isfinite(ex) or not np.isfinite(ey):
                return F32(np.inf)
            d = max(d, ex, ey)
    return d


def key_map(Ma, Mb):
    W, Mb = invert3x3(Ma), [F32(v) for v in Mb]
    with np.errstate(all="ignore"):
        p = [fmaf(Mb[3 * r + 2], W[6 + c], fmaf(Mb[3 * r + 1], W[3 + c], Mb[3 * r] * W[c])) for r in range(3) for c in range(3)]
        H = np.array([v / p[8] for v in p], F32)
    ok = p[8] != 0 and np.isfinite(np.array(p, F32)).all() and np.isfinite(H).all()
    return (H if ok else np.zeros(9, F32)), int(ok)


DEFAULTS = dict(cell_min=64, min_pixels=1024, max_bad=0.25, rel=0.6, w=2, d_min=32.0, d_max=128.0, carry=False)


def pick_model(stats, chain, fw, fh, keep, frame_status=None, **kw):
    p = dict(DEFAULTS, **kw)
    stats = np.asarray(stats).astype(np.uint64)
    n, cells = stats.shape[0], stats.shape[1] * stats.shape[2]
    chain = np.asarray(chain, F32).reshape(n, 9)
    S = stats.reshape(n, cells, 8)
    flags, scores = np.zeros(n, np.int32), np.zeros((n, 4), F64)
    for k in range(n):
        t = [int(S[k, :, q].astype(object).sum()) for q in range(8)]
        sharp = sorted((F64(int(S[k, c, 3])) / F64(int(S[k, c, 0])), c) for c in range(cells) if int(S[k, c, 0]) >= p["cell_min"])
        score = sharp[(len(sharp) - 1) // 2][0] if sharp else F64(0)
        f = 0
        row = chain[k]
        if (frame_status is not None and frame_status[k] != 1) or not np.isfinite(row).all() or not row.any():
            f |= STATUS
        if not sharp or t[0] < p["min_pixels"]:
            f |= FEW
        if not F64(t[5] + t[6]) <= F64(p["max_bad"]) * F64(t[7]):
            f |= BAD
        flags[k] = f
        scores[k, :3] = (score, F64(t[1]) / F64(t[0]) if t[0] else 0, F64(t[5] + t[6]) / F64(t[7]) if t[7] else 0)
    pre = flags.copy()
    for k in range(n):
        ref = max([scores[j, 0] for j in range(max(0, k - p["w"]), min(n - 1, k + p["w"]) + 1) if not pre[j] & 7] + [F64(0)])
        scores[k, 3] = ref
        if not pre[k] & 7 and scores[k, 0] < F64(p["rel"]) * ref:
            flags[k] |= BLURRED
    usable = [not flags[k] & 15 for k in range(n)]
    d_min, d_max = F32(p["d_min"]), F32(p["d_max"])
    keys, truncated, jump = [], 0, False
    last = 0 if p["carry"] else next((k for k in range(n) if usable[k]), -1)
    while last >= 0:
        if len(keys) == keep:
            truncated = 1
            break
        keys.append(last)
        flags[last] |= KEY | (JUMP if jump else 0)
        close, cand = -1, []
        for j in range(last + 1, n):
            if not usable[j]:
                continue
            d = motion(chain[last], chain[j], fw, fh)
            if d > d_max:
                close = j
                break
            if d >= d_min:
                cand.append(j)
        if cand:
            last, jump = max(cand, key=lambda j: (scores[j, 0], -j)), False
        else:
            last, jump = close, True
    out_keys = np.array(keys + [-1] * (keep - len(keys)), np.int32)
    H, Hs = np.zeros((keep - 1, 9), F32), np.zeros(keep - 1, np.int32)
    for i in range(len(keys) - 1):
        H[i], Hs[i] = key_map(chain[keys[i]], chain[keys[i + 1]])
    return dict(keys=out_keys, key_count=np.array([len(keys), truncated], np.int32), key_status=(out_keys >= 0).astype(np.int32),
                flags=flags, scores=scores, H_keys=H, H_status=Hs)


def same_pick(got, want):
    got = got._asdict() if hasattr(got, "_asdict") else got
    for name in ("keys", "key_count", "key_status", "flags", "H_status"):
        assert np.array_equal(np.asarray(got[name]), want[name]), (name, got[name], want[name])
    assert np.array_equal(np.asarray(got["scores"]).view(np.uint64), want["scores"].view(np.uint64)), "scores"
    assert np.array_equal(np.asarray(got["H_keys"]).view(np.uint32), want["H_keys"].view(np.uint32)), "H_keys"


def gather_model(keys, src, fill=0):
    src = np.stack(src)
    keys = np.asarray(keys)
    ok = (keys >= 0) & (keys < len(src))
    out = src[np.where(ok, keys, 0)]
    out.view(np.uint8).reshape(len(keys), -1)[~ok] = fill
    return out


# ---- the pick cases shared by the host and the device tests -------------------------------------------------------------------
def translation(tx, ty=0.0):
    return np.array([1, 0, tx, 0, 1, ty, 0, 0, 1], F32)


def flat_stats(scores, measured=5000, gx=1, gy=1, bad=0):
    """stats whose every cell holds `measured` pixels and the sharpness scores[k] exactly (scores are integers)"""
    n = len(scores)
    s = np.zeros((n, gy, gx, 8), np.uint64)
    s[..., 0] = measured
    s[..., 1] = measured * 100
    s[..., 3] = (np.asarray(scores, np.uint64) * np.uint64(measured))[:, None, None]
    s[..., 7] = measured + bad
    s[..., 5] = bad
    return s


def pick_cases():
    """name -> (stats, chain, fw, fh, keep, frame_status, kw)"""
    FW_, FH_ = 64, 48
    n = 12
    shift = np.stack([translation(-float(k)) for k in range(n)])                  # frame k looks 1 px further right per frame
    ident = np.stack([translation(0.0)] * n)
    c = {}
    flat = flat_stats([10] * n)
    c["identity chains"] = (flat, ident, FW_, FH_, 8, None, dict(d_min=1.0, d_max=4.0))
    for name, d_min, d_max in (("d_min hit", 3.0, 100.0), ("d_min one below", 2.0, 100.0), ("d_min one above", 4.0, 100.0),
                               ("d_max hit", 0.0, 3.0), ("d_max one below", 0.0, 2.0), ("d_max one above", 0.0, 4.0),
                               ("both hit", 3.0, 3.0)):
        c[name] = (flat_stats([10, 11, 12, 50, 14, 13, 60, 15, 16, 17, 70, 5]), shift, FW_, FH_, 8, None, dict(d_min=d_min, d_max=d_max, rel=0.0))
    c["a tie takes the lower index"] = (flat_stats([10, 30, 30, 30, 10, 30, 30, 9, 9, 9, 9, 9]), shift, FW_, FH_, 8, None,
                                        dict(d_min=1.0, d_max=3.0, rel=0.0))
    broken = shift.copy()
    broken[0] = 0
    c["carry on a broken row 0"] = (flat, broken, FW_, FH_, 8, None, dict(d_min=1.0, d_max=3.0, carry=True))
    c["a broken row without carry"] = (flat, broken, FW_, FH_, 8, None, dict(d_min=1.0, d_max=3.0))
    behind = shift.copy()
    behind[4, 6:] = 0                                                              # denominators 0 at frame 4
    c["a non-positive denominator"] = (flat, behind, FW_, FH_, 8, None, dict(d_min=2.0, d_max=9.0))
    neg = shift.copy()
    neg[5] = -neg[5]                                                               # denominators -1 at frame 5
    c["a negative denominator"] = (flat, neg, FW_, FH_, 8, None, dict(d_min=2.0, d_max=9.0))
    status = np.ones(n, np.int32)
    status[0] = 0
    c["carry with an unusable frame 0"] = (flat, shift, FW_, FH_, 8, status, dict(d_min=2.0, d_max=4.0, carry=True))
    c["no carry with an unusable frame 0"] = (flat, shift, FW_, FH_, 8, status, dict(d_min=2.0, d_max=4.0))
    c["keep reached with a follower"] = (flat, shift, FW_, FH_, 3, None, dict(d_min=2.0, d_max=4.0))
    c["keep reached without a follower"] = (flat_stats([10] * 7), shift[:7], FW_, FH_, 3, None, dict(d_min=3.0, d_max=4.0))
    c["keep of one"] = (flat, shift, FW_, FH_, 1, None, dict(d_min=3.0, d_max=4.0))
    # rel at the exact product: 0.5 * 64 = 32 exactly: 32 is not blurred, 31 is
    c["rel at the exact product"] = (flat_stats([64, 32, 31, 64, 32, 31, 64, 31, 32, 64, 31, 32]), shift, FW_, FH_, 12, None,
                                     dict(d_min=1.0, d_max=1.0, rel=0.5, w=1))
    c["w of zero"] = (flat_stats([64, 3, 31, 64, 2, 31, 64, 31, 1, 64, 31, 32]), shift, FW_, FH_, 12, None,
                      dict(d_min=1.0, d_max=1.0, rel=1.0, w=0))
    c["every cell below cell_min"] = (flat_stats([10] * n, measured=63, gx=2, gy=2), shift, FW_, FH_, 8, None,
                                      dict(d_min=1.0, d_max=3.0, min_pixels=0))
    c["too few pixels in all"] = (flat_stats([10] * n, measured=100, gx=2, gy=2), shift, FW_, FH_, 8, None,
                                  dict(d_min=1.0, d_max=3.0, min_pixels=401))
    c["just enough pixels in all"] = (flat_stats([10] * n, measured=100, gx=2, gy=2), shift, FW_, FH_, 8, None,
                                      dict(d_min=1.0, d_max=3.0, min_pixels=400))
    c["bad fraction at the bound"] = (flat_stats([10] * n, measured=3000, bad=1000), shift, FW_, FH_, 8, None,
                                      dict(d_min=1.0, d_max=3.0, max_bad=0.25))
    c["bad fraction above the bound"] = (flat_stats([10] * n, measured=2999, bad=1000), shift, FW_, FH_, 8, None,
                                         dict(d_min=1.0, d_max=3.0, max_bad=0.25))
    even = flat_stats([0] * n, gx=2, gy=2)
    rng = np.random.default_rng(5)
    even[..., 3] = rng.integers(1, 50, (n, 2, 2)).astype(np.uint64) * np.uint64(5000)
    even[3, 0, 0, 0] = 10                                                          # three qualifying cells in frame 3
    even[5, :, :, 3] = 7 * 5000                                                    # four equal cells
    c["the lower median on an even number of cells"] = (even, shift, FW_, FH_, 8, None, dict(d_min=1.0, d_max=2.0, rel=0.0))
    full = flat_stats([0] * 64, gx=8, gy=8)
    full[..., 3] = np.random.default_rng(6).integers(0, 1 << 40, (64, 8, 8)).astype(np.uint64)
    full[..., 0] = np.random.default_rng(7).integers(1, 9000, (64, 8, 8)).astype(np.uint64)
    long_shift = np.stack([np.array([1, 0.001, -1.5 * k, -0.001, 1, 0.25 * k, 1e-6, 0, 1], F32) for k in range(64)])
    c["64 frames on 8 x 8 cells"] = (full, long_shift, 640, 480, 64, None, dict(d_min=4.0, d_max=9.0, min_pixels=0))
    c["64 frames, a keep of 5"] = (full, long_shift, 640, 480, 5, None, dict(d_min=4.0, d_max=9.0, min_pixels=0, rel=0.3, w=8))
    nan = shift.copy()
    nan[3, 2] = np.nan
    nan[6, 0] = np.inf
    c["rows that are not finite"] = (flat, nan, FW_, FH_, 8, None, dict(d_min=2.0, d_max=3.0))
    return c


def median_check():
    """the lower median by hand: cells of sharpness 4, 9, 2, 7 -> sorted 2, 4, 7, 9 -> rank (4 - 1) // 2 = 1 -> 4"""
    s = flat_stats([0], gx=2, gy=2)
    s[0, :, :, 3] = np.array([[4, 9], [2, 7]], np.uint64) * np.uint64(5000)
    return s, 4.0


# ---- end to end: a pan over the loop-closure scene ------------------------------------------------------------------------
E2E_N, E2E_KEEP, E2E_PAN_X, E2E_PAN_Y = 48, 16, 19.3, 1.7
E2E_BLOCK = (60, 40, 260, 200)                                     # x, y, width, height of the painted block: 30 % of a view
E2E_PAINTED = 21
E2E_QUALITY = dict(lo=8, hi=250, grid=(4, 4))
E2E_PICK = dict(d_min=40.0, d_max=120.0)                           # everything else at its default
_e2e = {}


def e2e_maps():
    """A_k: view-k pixel -> scene pixel: the pan, a slow roll about the view's centre and a mild perspective term"""
    import loop_closure_ref as LC
    out = []
    for k in range(E2E_N):
        th = 0.0006 * k
        R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]], F64)
        P = np.array([[1, 0, 0], [0, 1, 0], [4e-7 * k, -2e-7 * k, 1]], F64)
        T = lambda x, y: np.array([[1, 0, x], [0, 1, y], [0, 0, 1]], F64)
        A = T(LC.ORIGIN_X + LC.VW / 2 + E2E_PAN_X * k, LC.ORIGIN_Y + LC.VH / 2 + E2E_PAN_Y * k) @ R @ P @ T(-LC.VW / 2, -LC.VH / 2)
        out.append(A / A[2, 2])
    return np.stack(out)


def render(scene, A, w, h):
    """bilinear samples of the scene at A (x, y), in float64, rounded to bytes"""
    y, x = np.mgrid[0:h, 0:w].astype(F64)
    s = A[2, 0] * x + A[2, 1] * y + A[2, 2]
    u, v = (A[0, 0] * x + A[0, 1] * y + A[0, 2]) / s, (A[1, 0] * x + A[1, 1] * y + A[1, 2]) / s
    i, j = np.floor(u).astype(int), np.floor(v).astype(int)
    assert i.min() >= 0 and j.min() >= 0 and i.max() + 1 < scene.shape[1] and j.max() + 1 < scene.shape[0]
    a, b = (u - i)[..., None], (v - j)[..., None]
    sc = scene.astype(F64)
    out = (1 - a) * (1 - b) * sc[j, i] + a * (1 - b) * sc[j, i + 1] + (1 - a) * b * sc[j + 1, i] + a * b * sc[j + 1, i + 1]
    return np.clip(np.floor(out + 0.5), 0, 255).astype(np.uint8)


def e2e():
    if _e2e:
        return _e2e
    import loop_closure_ref as LC
    scene, A = LC.scene(91), e2e_maps()
    views = []
    for k in range(E2E_N):
        v = render(scene, A[k], LC.VW, LC.VH)
        if k % 3 == 1:                                              # a 5-tap horizontal box
            p = np.pad(v.astype(np.int64), ((0, 0), (2, 2), (0, 0)), mode="edge")
            v = ((p[:, 0:-4] + p[:, 1:-3] + p[:, 2:-2] + p[:, 3:-1] + p[:, 4:] + 2) // 5).astype(np.uint8)
        if k == E2E_PAINTED:
            bx, by, bw, bh = E2E_BLOCK
            v[by:by + bh, bx:bx + bw, :3] = 255
        views.append(np.ascontiguousarray(v))
    chain = np.stack([(np.linalg.inv(A[k]) @ A[0]) / (np.linalg.inv(A[k]) @ A[0])[2, 2] for k in range(E2E_N)]).reshape(-1, 9).astype(F32)
    _e2e.update(views=views, A=A, chain=chain, blurred=[k for k in range(E2E_N) if k % 3 == 1],
                stats_model=stats_model(views, None, E2E_QUALITY["lo"], E2E_QUALITY["hi"], E2E_QUALITY["grid"]))
    return _e2e


def e2e_conditions(r, e):
    """the end-to-end conditions on a pick (a dict of numpy arrays)"""
    import loop_closure_ref as LC
    count = int(r["key_count"][0])
    keys = [int(k) for k in r["keys"][:count]]
    assert count >= 8 and keys == sorted(set(keys))
    assert not set(keys) & set(e["blurred"]), "a blurred view was chosen"
    assert E2E_PAINTED not in keys and r["flags"][E2E_PAINTED] & BAD and E2E_PAINTED % 3 != 1
    corners = np.array([[0, 0], [LC.VW - 1, 0], [0, LC.VH - 1], [LC.VW - 1, LC.VH - 1]], F64)
    for i in range(count - 1):
        a, b = keys[i], keys[i + 1]
        true = np.linalg.inv(e["A"][b]) @ e["A"][a]
        q = LC.apply(true, corners)
        d = np.abs(q - corners).max()
        assert E2E_PICK["d_min"] <= d <= E2E_PICK["d_max"], (a, b, d)
        assert r["H_status"][i] == 1 and np.abs(LC.apply(r["H_keys"][i].astype(F64), corners) - q).max() < 1e-3, (a, b)
    assert not (r["flags"][keys] & JUMP).any()
