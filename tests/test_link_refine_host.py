"""Direct link refinement on the host (nm_link_refine_host_f32) against tests/link_refine_ref.py: the restatement bit for
bit (sums in the written order, one iteration, whole calls), closed-form cases, one case per end reason, refused arguments,
and what the stage is worth on the synthetic mosaic views (the figures are recorded in DESIGN.md section 7, "Direct link
refinement")."""
import ctypes as C

import numpy as np
import pytest

import link_refine_ref as R

F32 = np.float32
FRAMES = [(64, 48), (67, 35), (131, 97)]
STRIDES = [1, 2, 3, 7, 64]           # 64 is larger than the two small frames' heights: L = 0 there
MODELS = [R.TRANSLATION, R.AFFINE, R.HOMOGRAPHY]
MAPS = {
    "identity": np.eye(3),
    "translation": [[1, 0, 3.3], [0, 1, -2.7], [0, 0, 1]],
    "homography": [[1.02, 0.03, 2.1], [-0.02, 0.98, 1.3], [1e-4, -2e-4, 1]],
    "outside": [[1, 0, 1000], [0, 1, 0], [0, 0, 1]],
}
START = np.array([[1, 0, 2.3], [0, 1, 0.8], [0, 0, 1]], F32)      # B below is A moved by (2, 1): about 0.4 px away


def frame(seed, fw, fh):
    """A smooth-ish frame with texture, values inside [0, 255] (the recipe of tests/test_link_verify_host.py)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:fh, 0:fw]
    f = 120 + 60 * np.sin(xx / 5.0 + seed) * np.cos(yy / 7.0) + 40 * rng.random((fh, fw))
    return np.clip(f, 0, 255).astype(F32)


def smooth(fw, fh, dx=0.0, dy=0.0):
    yy, xx = np.mgrid[0:fh, 0:fw]
    return (120 + 60 * np.sin((xx + dx) / 5.0 + 1.0) * np.cos((yy + dy) / 7.0)).astype(F32)


def moved(A):
    """A moved by (2, 1) pixels and brightened: B(x + 2, y + 1) = 1.1 A(x, y) + 5."""
    return np.clip(1.1 * np.roll(A, (1, 2), (0, 1)) + 5, 0, 255).astype(F32)


def disc(fw, fh):
    yy, xx = np.mgrid[0:fh, 0:fw]
    return ((xx - fw / 2) ** 2 + (yy - fh / 2) ** 2 < (0.45 * min(fw, fh)) ** 2).astype(F32)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(got, want):
    """(H_out, status, stats) of one pair, bit for bit (H as words, so a NaN compares)"""
    return (np.array_equal(np.asarray(got[0], F32).view(np.uint32), np.asarray(want[0], F32).view(np.uint32)) and
            int(got[1]) == int(want[1]) and np.array_equal(bits(got[2]), bits(want[2])))


def one(nm, A, B, H, **kw):
    """The host twin on one pair: (H_out[9], status, stats[9])."""
    H_out, st, stats = nm.link_refine_host([A], [B], np.asarray(H, F32).reshape(1, 9), **kw)
    return H_out[0], int(st[0]), stats[0]


def sums_of(nm, A, B, H, **kw):
    return nm.link_refine_host([A], [B], np.asarray(H, F32).reshape(1, 9), want_sums=True, **kw)[3][0]


def count(s):
    return s[54] / R.BIAS_SCALE ** 2


@pytest.mark.parametrize("size", FRAMES)
@pytest.mark.parametrize("masked", [False, True])
def test_host_twin_equals_restatement(nm, size, masked):
    """The 67 sums under four maps and one iteration of every model, bit for bit, at every stride."""
    fw, fh = size
    A, B = frame(1, fw, fh), frame(2, fw, fh)
    B2 = moved(A)
    mask = disc(fw, fh) if masked else None
    for stride in STRIDES:
        for name, H in MAPS.items():
            got = sums_of(nm, A, B, H, mask=mask, stride=stride)
            want = R.sums_ref(A, B, np.asarray(H, F32).reshape(9), mask, stride)
            assert np.array_equal(bits(got), bits(want)), (size, masked, stride, name)
            if name == "outside":
                assert count(got) == 0
        for model in MODELS:
            kw = dict(mask=mask, model=model, stride=stride, iterations=1, min_pixels=8)
            got, want = one(nm, A, B2, START, **kw), R.refine_ref(A, B2, START, **kw)
            assert same(got, want), (size, masked, stride, model, got[2], want[2])
            if stride == 64 and fh < 64:
                assert got[2][1] == 0 and got[1] == 0 and got[2][8] == R.END_FEW_PIXELS     # L = 0
                assert np.array_equal(got[0], START.reshape(9))


@pytest.mark.parametrize("model", MODELS)
def test_whole_calls_equal_restatement(nm, model):
    """Four iterations: the iterate carried in float64, its float32 rounding walked, the stop rule."""
    fw, fh = 131, 97
    A = smooth(fw, fh)
    for B, H in ((moved(A), START), (smooth(fw, fh, 1.5, -0.7), np.eye(3, dtype=F32))):
        kw = dict(model=model, stride=2, iterations=4)
        got, want = one(nm, A, B, H, **kw), R.refine_ref(A, B, H, **kw)
        assert same(got, want), (model, got[2], want[2])
        assert got[1] == 1 and got[2][6] >= 2


def test_identity_on_equal_frames(nm):
    """A = B under the identity: r = 0 everywhere, so J^T r = 0, the solution is 0 and W = I. M = Ti (W T) is the identity
    up to the rounding of h (1 / h) and cx - h (cx / h) in float64, so the step is below 1e-9 pixel, the pair converges in
    iteration 1 and H_out is the identity to the same rounding. gain = 1 and bias = 0 exactly (alpha = beta = 0)."""
    for (fw, fh), stride in (((67, 35), 3), ((64, 48), 1)):
        A = frame(3, fw, fh)
        for model in MODELS:
            H, st, stats = one(nm, A, A, np.eye(3), model=model, stride=stride)
            assert st == 1 and stats[8] == R.END_CONVERGED and stats[6] == 1 and stats[7] < 1e-9
            assert np.abs(H - np.eye(3).reshape(9)).max() < 1e-9
            assert stats[2] == 0 and stats[3] == 0 and stats[4] == 1 and stats[5] == 0
    # at stride 1 the border and the last column and row of taps drop out of N, nothing drops out of L
    s = sums_of(nm, frame(3, 64, 48), frame(3, 64, 48), np.eye(3), stride=1)
    assert s[R.S_L] == 64 * 48 and count(s) == 62 * 46


def test_gain_and_bias_of_an_affine_brightness_change(nm):
    """B = 1.2 A + 10 with A in [20, 120] (B stays inside [0, 255]) under the identity, where qb is B's own level. Levels:
    qa = 16 a + da, qb = 16 b + db with |da|, |db| <= 1/2 (b's own float32 rounding is below 2^-12 level), so
    r = qb - qa = 0.2 qa + 160 + e with |e| <= 0.5 + 1.2 * 0.5 + 2^-12 < 1.2: the residual is linear in the columns with
    alpha = 0.2 / GAIN_SCALE, beta = 160 / BIAS_SCALE and no motion, plus e. Least squares moves the solution by
    (J^T J)^-1 J^T e, at most |e|_2 / sigma_min(J) <= 1.2 sqrt(N / lambda_min(J^T J)) in every parameter; gain and bias
    scale that by GAIN_SCALE and BIAS_SCALE / 16. lambda_min is taken from the sums of the model's columns."""
    fw, fh = 67, 35
    A = (20 + 100 * np.random.default_rng(5).random((fh, fw))).astype(F32)
    B = (F32(1.2) * A + F32(10)).astype(F32)
    s = sums_of(nm, A, B, np.eye(3), stride=1)
    for model in MODELS:
        cols = R.COLUMNS[model]
        JtJ = np.array([[s[R.e_of(min(i, j), max(i, j))] for j in cols] for i in cols])
        d = 1.2 * np.sqrt(count(s) / np.linalg.eigvalsh(JtJ)[0])
        H, st, stats = one(nm, A, B, np.eye(3), model=model, stride=1)
        print("model %d: gain %.6f (bound %.2e) bias %.5f (bound %.2e)" % (model, stats[4], R.GAIN_SCALE * d, stats[5],
                                                                           R.BIAS_SCALE / 16 * d))
        assert abs(stats[4] - 1.2) <= R.GAIN_SCALE * d and abs(stats[5] - 10) <= R.BIAS_SCALE / 16 * d
        assert st == 1


def test_one_case_per_end_reason(nm):
    fw, fh = 64, 48
    A = smooth(fw, fh)
    B = moved(A)
    I = np.eye(3, dtype=F32).reshape(9)
    kw = dict(stride=1, min_pixels=64)
    # unusable: status_in = 0; a NaN in H. H_out is H_in bit for bit, stats are zero but for the reason.
    Hn = I.copy()
    Hn[4] = np.nan
    for H, status in ((I, [0]), (Hn, None)):
        H_out, st, stats = nm.link_refine_host([A], [B], H.reshape(1, 9), status=status, **kw)
        assert st[0] == 0 and stats[0][8] == R.END_UNUSABLE and not stats[0][:8].any()
        assert np.array_equal(H_out[0].view(np.uint32), H.view(np.uint32))
    # too few pixels
    H_out, st, stats = one(nm, A, B, START, stride=1, min_pixels=62 * 46 + 1)
    assert (st, stats[8], stats[6]) == (0, R.END_FEW_PIXELS, 0) and np.array_equal(H_out, START.reshape(9))
    assert 0 < stats[0] <= 62 * 46
    # singular: a flat frame has no gradient, the first pivot is 0
    flat = np.full_like(A, 100)
    for model in MODELS:
        H_out, st, stats = one(nm, flat, flat, I, model=model, **kw)
        assert (st, stats[8]) == (0, R.END_SINGULAR) and np.array_equal(H_out, I) and stats[0] == 62 * 46
    # a step larger than max_step is not applied
    H_out, st, stats = one(nm, A, B, START, max_step=0.05, **kw)
    assert (st, stats[8], stats[6]) == (0, R.END_STEP, 0) and stats[7] > 0.05 and np.array_equal(H_out, START.reshape(9))
    # converged
    H_out, st, stats = one(nm, A, B, START, iterations=8, **kw)
    assert (st, stats[8]) == (1, R.END_CONVERGED) and stats[7] < R.CONVERGED_STEP and 2 <= stats[6] <= 8
    assert R.corner_error(H_out, [[1, 0, 2], [0, 1, 1], [0, 0, 1]], fw, fh) < 0.05
    assert abs(stats[4] - 1.1) < 0.01 and abs(stats[5] - 5) < 1.0 and stats[3] < stats[2]
    # iterations exhausted
    H_out, st, stats = one(nm, A, B, START, iterations=1, **kw)
    assert (st, stats[8], stats[6]) == (1, R.END_ITERATIONS, 1) and not np.array_equal(H_out, START.reshape(9))


def test_nan_and_out_of_range_pixels(nm):
    """A bad pixel of A leaves L; it leaves N together with the four lattice pixels whose gradient reads it. A bad tap of B
    leaves N alone, for each of the four lattice pixels that read it."""
    fw, fh = 64, 48
    A = frame(9, fw, fh)
    I = np.eye(3)
    base = sums_of(nm, A, A, I, stride=1)
    for bad in (np.nan, -0.5, 255.5, np.inf):
        A2 = A.copy()
        A2[10, 20] = bad
        s = sums_of(nm, A2, A, I, stride=1)
        assert (s[R.S_L], count(s)) == (base[R.S_L] - 1, count(base) - 5), bad
        assert np.array_equal(bits(s), bits(R.sums_ref(A2, A, I, None, 1)))
        B2 = A.copy()
        B2[10, 20] = bad
        s = sums_of(nm, A, B2, I, stride=1)
        assert (s[R.S_L], count(s)) == (base[R.S_L], count(base) - 4), bad
        assert np.array_equal(bits(s), bits(R.sums_ref(A, B2, I, None, 1)))
    assert np.isfinite(s).all()


def test_refused_arguments_and_workspace(nm):
    A = frame(1, 64, 48)
    H = np.eye(3, dtype=F32).reshape(1, 9)
    bad = [dict(stride=0), dict(stride=65), dict(model=3), dict(model=-1), dict(iterations=0), dict(iterations=9),
           dict(min_pixels=0), dict(max_step=0.0), dict(max_step=-1.0), dict(max_step=np.nan), dict(max_step=np.inf)]
    for b in bad:
        with pytest.raises(nm.NmError):
            nm.link_refine_host([A], [A], H, **b)
    with pytest.raises(nm.NmError):
        nm.link_refine_host([], [], H)
    with pytest.raises(nm.NmError):
        nm.link_refine_host([A] * 65, [A] * 65, np.tile(H, (65, 1)))
    with pytest.raises(nm.NmError):
        nm.link_refine_host([A], [A[:, :32]], H)
    with pytest.raises(nm.NmError):
        nm.link_refine_host([A], [A], H[:, :8])
    with pytest.raises(nm.NmError):
        nm.link_refine_host([A], [A], H, status=[1, 1])
    # the C entries themselves (host and device: the device entry refuses before it touches anything, so host pointers do)
    L = nm.lib()
    tab = (C.c_void_p * 1)(A.ctypes.data)
    nul = (C.c_void_p * 1)(None)
    Ho, st, stats = np.zeros(9, F32), np.zeros(1, np.int32), np.zeros(9)
    p = lambda a: a.ctypes.data

    def call(n=1, ta=tab, tb=tab, fw=64, fh=48, Hp=p(H), model=2, stride=4, it=4, mp=64, ms=16.0, ho=p(Ho), so=p(st),
             xo=p(stats), ws=p(stats)):
        host = L.nm_link_refine_host_f32(n, ta, tb, fw, fh, None, Hp, None, model, stride, it, mp, ms, ho, so, xo)
        if host == 0 and ws is not None:
            return host, None                 # accepted: the device entry would launch, and these are host pointers
        dev = L.nm_link_refine_batch_dev_f32(n, ta, tb, fw, fh, None, Hp, None, model, stride, it, mp, ms, ho, so, xo, ws, None)
        return host, dev
    assert call() == (0, None)
    refused = [dict(n=0), dict(n=65), dict(fw=0), dict(fw=32768), dict(fh=0), dict(fh=32768), dict(stride=0), dict(stride=65),
               dict(fw=32767, fh=32767, stride=1), dict(model=-1), dict(model=3), dict(it=0), dict(it=9), dict(mp=0),
               dict(ms=0.0), dict(ms=float("nan")), dict(ms=float("inf")), dict(ta=None), dict(tb=nul), dict(Hp=None),
               dict(ho=None), dict(so=None), dict(xo=None)]
    for r in refused:
        host, dev = call(**r)
        assert host != 0 and dev != 0, r
    assert call(ws=None)[1] != 0
    assert L.nm_link_refine_sums_host_f32(1, tab, tab, 64, 48, None, p(H), 4, None) != 0
    assert L.nm_link_refine_sums_host_f32(1, tab, tab, 64, 48, None, p(H), 0, p(np.zeros(67))) != 0
    assert L.nm_link_refine_workspace_bytes(0) == 0 and L.nm_link_refine_workspace_bytes(65) == 0
    assert L.nm_link_refine_workspace_bytes(64) == 64 * L.nm_link_refine_workspace_bytes(1) > 0
    for name in ("nm_link_refine_workspace_bytes", "nm_link_refine_batch_dev_f32", "nm_link_refine_host_f32",
                 "nm_link_refine_sums_host_f32"):
        assert name in nm.ABI_SYMBOLS
    assert len(nm.LINK_REFINE_STATS) == 9 and nm.LINK_REFINE_MAX_BATCH == 64 and nm.LINK_REFINE_MAX_ITERATIONS == 8
    assert (nm.LINK_REFINE_TRANSLATION, nm.LINK_REFINE_AFFINE, nm.LINK_REFINE_HOMOGRAPHY) == (0, 1, 2)


# ---- what it is worth: the mosaic views of tests/test_link_verify_host.py, rebuilt here with the same recipe ----

VW, VH, SCENE_W, SCENE_H = 640, 480, 1240, 600


def view_maps():
    maps = []
    for k in range(8):
        deg = 0.0 if k == 0 else 1.5 * np.sin(k)
        c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
        maps.append(np.array([[c, -s, 40 + 70 * k], [s, c, 50 + 14 * (-1) ** k], [0, 0, 1]], np.float64))
    return maps


def scene_bgr(seed):
    import helpers
    g = np.clip(helpers.blurred_frame(seed, SCENE_W, SCENE_H, sigma=2.0) * 1.4, 0, 255).astype(np.uint8)
    return np.stack([g, np.roll(g, 3, 1), np.roll(g, 5, 0)], -1)


def gray_views(scene):
    yy, xx = np.mgrid[0:VH, 0:VW].astype(np.float64)
    out = []
    for A in view_maps():
        sx, sy = A[0, 0] * xx + A[0, 1] * yy + A[0, 2], A[1, 0] * xx + A[1, 1] * yy + A[1, 2]
        i, j = np.floor(sx).astype(int), np.floor(sy).astype(int)
        fx, fy = (sx - i)[..., None], (sy - j)[..., None]
        pad = np.zeros((SCENE_H + 2, SCENE_W + 2, 3))
        pad[1:-1, 1:-1] = scene
        tap = lambda dj, di: pad[np.clip(j + dj + 1, 0, SCENE_H + 1), np.clip(i + di + 1, 0, SCENE_W + 1)]
        v = (1 - fx) * (1 - fy) * tap(0, 0) + fx * (1 - fy) * tap(0, 1) + (1 - fx) * fy * tap(1, 0) + fx * fy * tap(1, 1)
        v = np.floor(np.clip(v / 255.0 * 255.9999, 0, 255))
        out.append((0.07 * v[..., 0] + 0.72 * v[..., 1] + 0.21 * v[..., 2]).astype(F32))
    return out


def true_maps():
    A = view_maps()
    out = []
    for k in range(7):
        Ht = np.linalg.inv(A[k + 1]) @ A[k]
        out.append(Ht / Ht[2, 2])
    return out


def perturbation():
    """A roll of 0.3 degrees about the frame's centre (2.1 px at the corners), a shift and a small projective term."""
    a = np.radians(0.3)
    c, s = np.cos(a), np.sin(a)
    centre = np.array([[1, 0, VW / 2], [0, 1, VH / 2], [0, 0, 1.0]])
    P = centre @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ np.linalg.inv(centre)
    P = np.array([[1, 0, 0.1], [0, 1, -0.05], [0, 0, 1.0]]) @ P
    P[2, 0] += 2e-7
    P[2, 1] -= 1.5e-7
    return P / P[2, 2]


SHIFT = np.array([[1, 0, 3.0], [0, 1, 0], [0, 0, 1.0]])
BAR = 0.05                    # px: the issue's bar for the corner error after 4 iterations
# corner distance between the bit-exact restatement's map and the unquantised model's, measured on the 7 links from the
# perturbed start: at most 1.485e-3 px; twice that is allowed between the host twin's corner error and the model's
# 
CORNER_ALLOWANCE = 2.97e-3


@pytest.fixture(scope="module")
def worth(oracle):
    views = gray_views(scene_bgr(90))
    brighter = [np.clip(1.1 * v + 5, 0, 255).astype(F32) for v in views]
    true = true_maps()
    start = []
    for k in range(7):
        H = true[k] @ perturbation()
        start.append((H / H[2, 2]).astype(F32))
    model = [R.model_f64(views[k], brighter[k + 1], start[k], stride=4, iterations=4) for k in range(7)]
    return dict(views=views, brighter=brighter, true=true, start=start, model=model)


def test_model_alone_brings_every_link_below_the_bar(worth):
    """The scene first: the unquantised float64 model, from a start about 2 px off at the corners."""
    e0 = [R.corner_error(worth["start"][k], worth["true"][k], VW, VH) for k in range(7)]
    e4 = [R.corner_error(worth["model"][k], worth["true"][k], VW, VH) for k in range(7)]
    print("start %.3f .. %.3f px, model after 4 iterations %.4f .. %.4f px" % (min(e0), max(e0), min(e4), max(e4)))
    assert 1.8 < min(e0) and max(e0) < 2.4
    assert max(e4) < BAR


def test_host_twin_close_to_the_model_on_every_link(nm, worth):
    v, b = worth["views"], worth["brighter"]
    H_out, st, stats = nm.link_refine_host(v[:7], b[1:], np.array(worth["start"]).reshape(7, 9), stride=4, iterations=4)
    worst_ref = worst_twin = 0.0
    for k in range(7):
        ref = R.refine_ref(v[k], b[k + 1], worth["start"][k], stride=4, iterations=4)
        assert same((H_out[k], st[k], stats[k]), ref), k
        e_model = R.corner_error(worth["model"][k], worth["true"][k], VW, VH)
        e_twin = R.corner_error(H_out[k], worth["true"][k], VW, VH)
        worst_ref = max(worst_ref, R.corner_error(ref[0], worth["model"][k], VW, VH))
        worst_twin = max(worst_twin, e_twin - e_model)
        print("link %d: model %.4f twin %.4f px, gain %.4f bias %.3f, rms %.3f -> %.3f, %d steps, end %d" % (
            k, e_model, e_twin, stats[k][4], stats[k][5], stats[k][2], stats[k][3], stats[k][6], stats[k][8]))
        assert e_twin <= e_model + CORNER_ALLOWANCE and e_twin < BAR
    print("corner distance restatement - model %.3e px, twin error over model error %.3e px" % (worst_ref, worst_twin))
    assert (st == 1).all()


@pytest.mark.parametrize("model", MODELS)
def test_every_model_recovers_a_pure_shift(nm, worth, model):
    """From the true map composed with a 3 px shift, links 0, 3 and 6: all three models end below the same bar."""
    v, b = worth["views"], worth["brighter"]
    ks = (0, 3, 6)
    start = np.array([(worth["true"][k] @ SHIFT).astype(F32) for k in ks]).reshape(3, 9)
    H_out, st, stats = nm.link_refine_host([v[k] for k in ks], [b[k + 1] for k in ks], start, model=model, stride=4,
                                           iterations=4)
    for n, k in enumerate(ks):
        e0, e4 = R.corner_error(start[n], worth["true"][k], VW, VH), R.corner_error(H_out[n], worth["true"][k], VW, VH)
        print("model %d link %d: %.3f -> %.4f px in %d steps" % (model, k, e0, e4, stats[n][6]))
        assert abs(e0 - 3) < 1e-3 and e4 < BAR and st[n] == 1
