"""nm_ransac_f32 and nm_ransac_batch_dev_f32 against the float64 reference of tests/ransac_ref.py AND against the CPU oracle.

Every GPU result is checked twice: by ransac_ref.check_call and the fit limits recorded in tests/test_ransac_float64.py (an
error that kernel and oracle share cannot hide behind their bit equality), and bit for bit against the oracle (nothing that
held before weakens). Covered: the geometry sweep at 1080p, 4K and 8K; point counts 1..100 003 and hypothesis counts
1..65 536 (above 8192 the grid-stride loop of ransac_inlier_kernel runs, with a skipped hypothesis up there); ties of the
best count placed across the strides of both selection schemes; the degenerate catalogue including calls where no
hypothesis is usable; align_points output with unmatched rows at wave boundaries.
Limits: ransac_ref.limits(model, W, H), the table in tests/test_ransac_float64.py. Wall time of this module on one MI355X,
measured once: 31 s for its 49 tests (most of it the host-side float64 brackets and the oracle), against 3 s for the two
existing RANSAC modules together.
"""
import numpy as np
import pytest

import ransac_ref as R
from test_gpu_ransac_batch import _rand_list, _run, _valid_rows
from test_ransac_batch_host import sample_np

pytestmark = pytest.mark.gpu

MODELS = [0, 1, 2]
GPU_FRAMES = [(1920, 1080), (3840, 2160), (7680, 4320)]


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    """Equal bit for bit, except that a NaN only has to meet a NaN: sign and payload of a NaN are not part of the contract
    (an invalid operation gives 0xFFC00000 on x86, where the oracle runs, and 0x7FC00000 on the GPU)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def _pts(sc):
    return sc["sx"], sc["sy"], sc["dx"], sc["dy"]


def _gpu(nm, dev, model, pts, rl, thr):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pos, Hb, Ha, inl = nm.ransac(model, *[t(a) for a in pts], t(rl), thr)
    torch.cuda.synchronize()
    return int(pos.item()), Hb.cpu().numpy(), Ha.cpu().numpy(), inl.cpu().numpy()


def _twice(oracle, model, pts, rl, thr, got, label, always=()):
    """float64 rules, then the oracle bit for bit."""
    R.check_call(model, pts, rl, thr, got, label, always=always)
    pos_r, Hb_r, Ha_r, inl_r = oracle.ransac(model, *pts, rl, thr)
    assert np.array_equal(got[3], inl_r), "%s: %d counts differ from the oracle" % (label, (got[3] != inl_r).sum())
    assert _same_bits(got[2], Ha_r), label + ": hypotheses differ from the oracle"
    assert got[0] == pos_r and _same_bits(got[1], Hb_r), label


def _identity_pair(pts):
    """A batch pair whose rows are already aligned: match i -> i."""
    return dict(nA=len(pts[0]), sx=pts[0], sy=pts[1], dx=pts[2], dy=pts[3], matches=np.arange(len(pts[0]), dtype=np.int32))


def _batch_twice(nm, oracle, dev, model, pairs, iterations, thr, seeds, capA, label, limits=None):
    out = _run(nm, dev, pairs, model, iterations, thr, seeds, capA)
    Hb, best, pos, status, Ha, inl = out
    for k, sc in enumerate(pairs):
        pts = tuple(sc[key][:min(sc["nA"], capA)] for key in ("sx", "sy", "dx", "dy"))
        V = _valid_rows(sc["sx"], sc["matches"], sc["nA"], capA)
        lab = "%s pair %d" % (label, k)
        if len(V) < (4 if model == 2 else 2):
            assert status[k] == 0 and best[k] == 0 and pos[k] == -1 and not Hb[k].any(), lab
            continue
        rl = _rand_list(V, seeds[k], model, iterations)
        assert status[k] == 1 and best[k] == inl[k][pos[k]], lab
        _twice(oracle, model, pts, rl, thr, (int(pos[k]), Hb[k], Ha[k], inl[k]), lab)
        if limits is not None:
            _assert_fit_limits(model, Ha[k], limits[k], rl, lab)
    return out


def _assert_fit_limits(model, Ha, sc, rl, label):
    lim_b, lim_f = R.limits(model, sc["W"], sc["H"])
    b, f = R.fit_errors(model, Ha, sc, rl)
    if len(b):
        assert np.isfinite(b).all() and b.max() <= lim_b, (label, b.max(), lim_b)
    if len(f):
        assert np.isfinite(f).all() and f.max() <= lim_f, (label, f.max(), lim_f)


# ------------------------------------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("W,Hh", GPU_FRAMES)
@pytest.mark.parametrize("model", MODELS)
def test_gpu_geometry_sweep(nm, oracle, cuda, model, W, Hh):
    scenes = []
    for motion, sc, rl in R.sweep(model, W, Hh):
        label = "model %d %dx%d %s" % (model, W, Hh, motion)
        got = _gpu(nm, cuda, model, _pts(sc), rl, R.SWEEP_THR)
        _assert_fit_limits(model, got[2], sc, rl, label)
        _twice(oracle, model, _pts(sc), rl, R.SWEEP_THR, got, label)
        scenes.append(sc)
    pairs = [_identity_pair(_pts(sc)) for sc in scenes]
    _batch_twice(nm, oracle, cuda, model, pairs, R.SWEEP_HYPOTHESES, R.SWEEP_THR, [11 * k + 5 for k in range(len(pairs))],
                 R.SWEEP_POINTS, "batched model %d %dx%d" % (model, W, Hh), limits=scenes)


@pytest.mark.parametrize("outliers", [0.0, 0.8])
@pytest.mark.parametrize("model", MODELS)
def test_gpu_recovers_the_true_map(nm, cuda, model, outliers):
    thr, W, Hh = 4.0, 3840, 2160
    motion = "perspective" if model == 2 else "rot90" if model == 1 else "negative"
    sc = R.scene(model, W, Hh, 1000, outliers, 0.0, 31 + model, motion)
    its = max(64, R.iterations_for(1.0 - outliers, R.SAMPLES[model]))
    assert its < R.MAX_ITERATIONS
    rl = R.sample_lists(1000, its, model, 8)
    R.assert_recovery(model, sc, rl, thr, _gpu(nm, cuda, model, _pts(sc), rl, thr))


# --------------------------------------------------------------------------------------------------------- shapes
POINT_COUNTS = [1, 2, 4, 63, 64, 65, 1023, 1024, 1025, 4097, 100003]
ITERATION_COUNTS = [1, 3, 255, 256, 257, 1023, 1024, 1025, 8192, 8193, 8196, 20001, 65536]


def _skip_high(rl):
    """A repeated-index hypothesis above 8192 (the -1 marker inside the grid-stride loop), where the list is that long."""
    marks = [t for t in (8200, 20000, 65535) if t < len(rl) and rl.shape[1] > 1]
    for t in marks:
        rl[t, :] = rl[t, 0]
    return marks


@pytest.mark.parametrize("model", MODELS)
def test_gpu_point_counts(nm, oracle, cuda, model):
    for n in POINT_COUNTS:
        sc = R.scene(model, 3840, 2160, n, 0.3 if n >= 63 else 0.0, 0.5, 50 + n, "mild", unmatched=(n // 2,) if n >= 63 else ())
        rl = R.sample_lists(n, 96, model, n)
        _twice(oracle, model, _pts(sc), rl, 3.0, _gpu(nm, cuda, model, _pts(sc), rl, 3.0), "model %d n=%d" % (model, n))


@pytest.mark.parametrize("model", MODELS)
def test_gpu_iteration_counts(nm, oracle, cuda, model):
    n = 257
    sc = R.scene(model, 1920, 1080, n, 0.4, 0.7, 60 + model, "perspective", unmatched=(64,))
    for its in ITERATION_COUNTS:
        rl = R.sample_lists(n, its, model, its)
        marks = _skip_high(rl)
        got = _gpu(nm, cuda, model, _pts(sc), rl, 4.0)
        _twice(oracle, model, _pts(sc), rl, 4.0, got, "model %d iterations=%d" % (model, its), always=marks)
        for t in marks:
            assert got[3][t] == 0 and not got[2][t].any()


@pytest.mark.parametrize("capA", [1024, 1025, 4096])
@pytest.mark.parametrize("model", MODELS)
def test_gpu_batch_iteration_counts(nm, oracle, cuda, model, capA):
    sc = R.scene(model, 1920, 1080, capA, 0.4, 0.7, 70 + model, "mild", unmatched=(63, 64, 65, capA - 1))
    pair = _identity_pair(_pts(sc))
    assert pair["nA"] == capA
    for its in ITERATION_COUNTS:
        _batch_twice(nm, oracle, cuda, model, [pair], its, 4.0, [its], capA, "model %d capA=%d iterations=%d" % (model, capA, its))


def test_gpu_batch_of_64_pairs_of_different_sizes(nm, oracle, cuda):
    rng = np.random.default_rng(5)
    capA, pairs = 3000, []
    sizes = [0, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, capA] + [int(v) for v in rng.integers(6, capA, nm.RANSAC_MAX_BATCH - 11)]
    for k, n in enumerate(sizes):
        sc = R.scene(2, 3840, 2160, capA, 0.4, 0.7, 900 + k, R.MOTIONS[k % len(R.MOTIONS)])
        p = _identity_pair(_pts(sc))
        p["nA"] = n                                           # rows beyond nA exist and must not be read
        pairs.append(p)
    assert len(pairs) == nm.RANSAC_MAX_BATCH
    out = _batch_twice(nm, oracle, cuda, 2, pairs, 300, 4.0, [3 * k + 1 for k in range(len(pairs))], capA, "64 pairs")
    assert out[3].tolist() == [0, 0] + [1] * 62


# ----------------------------------------------------------------------------------------------------------- ties
def _tie_scene(n, planted):
    """Integer coordinates, pure translations, thr 0.5: every row has a translation of its own except the `planted` rows,
    which share (7, -3). A hypothesis sampled from a planted row counts exactly `planted`, any other exactly 1."""
    rng = np.random.default_rng(n + planted)
    sx = rng.integers(0, 4000, n).astype(np.float32)
    sy = rng.integers(0, 2000, n).astype(np.float32)
    dx = sx + 10 + 2 * np.arange(n, dtype=np.float32)          # distinct translations, exact in float32
    dy = sy + 1
    rows = np.sort(rng.choice(n, planted, replace=False))
    dx[rows], dy[rows] = sx[rows] + 7, sy[rows] - 3
    return (sx, sy, dx, dy), rows


@pytest.mark.parametrize("its,winners", [(3000, (5, 5 + 1024)), (3000, (300, 300 + 256)), (3000, (1029, 2053, 2999)),
                                         (3000, (0, 2999)), (2055, (2050, 2054)), (8193 + 4096, (8192, 12288)),
                                         (1025, (1024,)), (1, (0,))])
def test_gpu_ties_take_the_first_maximum(nm, oracle, cuda, its, winners):
    n, planted = 2000, 40
    pts, rows = _tie_scene(n, planted)
    others = np.setdiff1d(np.arange(n), rows)
    rl = others[np.random.default_rng(its).integers(0, len(others), (its, 1))].astype(np.int32)
    for i, t in enumerate(winners):
        rl[t, 0] = rows[i % planted]                            # different planted rows: equal counts, different samples
    got = _gpu(nm, cuda, 0, pts, rl, 0.5)
    want = np.ones(its, np.int32)
    want[list(winners)] = planted
    assert np.array_equal(got[3], want)
    assert got[0] == min(winners), (got[0], winners)
    _twice(oracle, 0, pts, rl, 0.5, got, "ties %r" % (winners,))


def _search_seed(n_valid, its, pattern, limit=200000):
    """The first seed whose device-side sample list puts planted rows (valid-row ranks < pattern's `planted`) exactly where
    `pattern(winner indices)` wants them. The search is bounded and fails loudly."""
    t = np.arange(its)
    for seed in range(limit):
        j = sample_np(seed, t, np.zeros(its, np.int64), 1, np.full(its, n_valid))
        w = np.flatnonzero(j < pattern.planted)
        if len(w) and pattern(w):
            return seed, w
    raise AssertionError("no seed below %d gives the tie pattern %s" % (limit, pattern.__name__))


def _pattern(planted, name, fn):
    fn.planted, fn.__name__ = planted, name
    return fn


@pytest.mark.parametrize("name", ["t and t+256", "t and t+1024", "first and last", "last partial workgroup only"])
def test_gpu_batch_ties_take_the_first_maximum(nm, oracle, cuda, name):
    n = 2000
    if name == "t and t+256":
        its, planted = 1300, 40
        pat = _pattern(planted, name, lambda w: w[0] + 256 in w)
    elif name == "t and t+1024":
        its, planted = 1300, 40
        pat = _pattern(planted, name, lambda w: w[0] + 1024 in w)
    elif name == "first and last":
        its, planted = 1300, 200
        pat = _pattern(planted, name, lambda w: w[0] == 0 and w[-1] == 1299)
    else:
        its, planted = 1031, 2                                 # 4 full workgroups of 256 and one of 7
        pat = _pattern(planted, name, lambda w: w[0] >= 1024 and len(w) >= 2)
    pts, rows = _tie_scene(n, planted)
    # move the planted rows to the front, so that "valid-row rank < planted" means a planted row
    order = np.concatenate([rows, np.setdiff1d(np.arange(n), rows)])
    pts = tuple(a[order] for a in pts)
    seed, w = _search_seed(n, its, pat)
    out = _batch_twice(nm, oracle, cuda, 0, [_identity_pair(pts)], its, 0.5, [seed], n, "batched ties " + name)
    Hb, best, pos, status, Ha, inl = out
    want = np.ones(its, np.int32)
    want[w] = planted
    assert np.array_equal(inl[0], want)
    assert pos[0] == w[0] and best[0] == planted and status[0] == 1, (pos[0], w[:4], seed)


# ----------------------------------------------------------------------------------------------------- degenerate
@pytest.mark.parametrize("model", MODELS)
def test_gpu_degenerate_catalogue(nm, oracle, cuda, model):
    cases, dead = R.catalogue(model)
    clean = None
    for name, pts, rl, thr, base in cases:
        got = _gpu(nm, cuda, model, pts, rl, thr)
        _twice(oracle, model, pts, rl, thr, got, name)
        if name == "clean":
            clean = got[2].copy()
            assert np.isfinite(clean).all() and got[3].min() > 100
        assert np.array_equal(_u32(got[2][base]), _u32(clean)), name + ": a well-posed hypothesis changed"
    if len(dead):
        pts = cases[0][1]
        got = _gpu(nm, cuda, model, pts, dead, 4.0)
        _twice(oracle, model, pts, dead, 4.0, got, "all unusable")
        assert not got[3].any() and got[0] == 0 and not np.isfinite(got[1]).all()


def _workspace_hypotheses(nm, ws, n, capA, iterations):
    """The hypothesis block of the batch workspace (nm_ransac_batch.hip: 16-byte headers, float4 points, then n * iterations
    * 9 floats, each block rounded up to 256 bytes)."""
    al = lambda b: (b + 255) & ~255
    off = al(n * 16) + al(n * capA * 16)
    raw = ws.buf[off:off + n * iterations * 36].cpu().numpy()
    return raw.view(np.float32).reshape(n, iterations, 9)


@pytest.mark.parametrize("model", [1, 2])
def test_gpu_batch_degenerate_pairs(nm, oracle, cuda, model):
    import torch
    cases, _ = R.catalogue(model)
    base_pts = cases[0][1]
    rows = np.r_[200:212, 0:8]                                   # the coincident groups and eight ordinary rows
    dense = tuple(a[rows] for a in base_pts)
    same = tuple(np.full(40, a[208], np.float32) for a in base_pts)   # forty identical rows: no usable hypothesis at all
    point_lists = [dense, same] + [pts for name, pts, _, thr, _ in cases if "[" in name]
    pairs = [_identity_pair(p) for p in point_lists]
    capA, its = max(p["nA"] for p in pairs), 2048
    for p in pairs:                                               # pad every list to capA rows; nA keeps the true size
        for key in ("sx", "sy", "dx", "dy"):
            p[key] = np.concatenate([p[key], np.full(capA - len(p[key]), 9.0, np.float32)])
        p["matches"] = np.arange(capA, dtype=np.int32)
    seeds = list(range(100, 100 + len(pairs)))
    for thr in (4.0, 0.0, R.FLT_MAX, -1.0):
        out = _batch_twice(nm, oracle, cuda, model, pairs, its, thr, seeds, capA, "degenerate thr=%r" % thr)
        Hb, best, pos, status, Ha, inl = out
        assert status.tolist() == [1] * len(pairs)
        assert best[1] == 0 and pos[1] == 0 and not inl[1].any()          # the all-identical pair
        assert (~np.isfinite(Ha[1]).all(axis=1) | R.skipped(_rand_list(np.arange(40), seeds[1], model, its))).all()
        if thr == 4.0:
            assert (~np.isfinite(Ha[0]).all(axis=1)).any(), "the dense pair drew no coincident sample"
        if not thr > 0:
            assert not best.any() and not pos.any() and not inl.any()
    # the optional outputs equal the workspace's own copy, which H_best is read from
    T = lambda key: [torch.from_numpy(p[key]).to(cuda) for p in pairs]
    d_nA = [torch.tensor([p["nA"]], dtype=torch.int32, device=cuda) for p in pairs]
    ws = nm.RansacBatchWorkspace(len(pairs), capA, its, cuda)
    Hb, best, pos, status, Ha, inl = nm.ransac_batch_dev(model, T("sx"), T("sy"), d_nA, T("dx"), T("dy"), T("matches"),
                                                        iterations=its, threshold=4.0, seeds=seeds, capA=capA, workspace=ws,
                                                        want_all=True)
    torch.cuda.synchronize()
    kept = _workspace_hypotheses(nm, ws, len(pairs), capA, its)
    assert np.array_equal(_u32(kept), _u32(Ha.cpu().numpy()))          # same device, same NaNs: plain bit equality
    assert np.array_equal(_u32(kept[np.arange(len(pairs)), pos.cpu().numpy()]), _u32(Hb.cpu().numpy()))


# ---------------------------------------------------------------------------------------------------- align_points
def test_gpu_align_points_feeds_ransac(nm, oracle, cuda):
    import torch
    sc = R.scene(2, 3840, 2160, 300, 0.3, 0.7, 77, "perspective")
    perm = np.random.default_rng(3).permutation(300)
    dst_x, dst_y = np.empty(300, np.float32), np.empty(300, np.float32)
    dst_x[perm], dst_y[perm] = sc["dx"], sc["dy"]
    matches = perm.astype(np.int32)
    gone = [0, 63, 64, 65, 127, 128, 191, 192, 299]
    matches[gone] = -1
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    aligned = [a.cpu().numpy() for a in nm.align_points(t(sc["sx"]), t(sc["sy"]), t(dst_x), t(dst_y), t(matches))]
    want = oracle.align_points(sc["sx"], sc["sy"], dst_x, dst_y, matches)
    for a, b in zip(aligned, want):
        assert np.array_equal(_u32(a), _u32(b))
    assert all((a[gone] == -1).all() for a in aligned)
    for model in MODELS:
        rl = R.sample_lists(300, 600, model, 12)
        for i, g in enumerate(gone):                              # unmatched rows are not counted but may be sampled
            rl[5 + 7 * i, 0] = g
        rl[70, :] = np.array(gone)[:R.SAMPLES[model]]
        got = _gpu(nm, cuda, model, tuple(aligned), rl, 4.0)
        _twice(oracle, model, tuple(aligned), rl, 4.0, got, "aligned model %d" % model)
