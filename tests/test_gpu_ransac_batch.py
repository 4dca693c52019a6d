"""Batched RANSAC with device-side sampling (nm_ransac_batch_dev_f32) against the CPU oracle, bit for bit: synthetic scenes
of all three models (clipping, empty and too-small pairs, forced repeated samples), slot independence, real frames through
batched detect -> match -> RANSAC, and a HIP graph over match + RANSAC replayed on other frames."""
import numpy as np
import pytest

import helpers as H
from test_ransac_batch_host import sample_np

pytestmark = pytest.mark.gpu

MIN_POINTS = {0: 2, 1: 2, 2: 4}
SAMPLES = {0: 1, 1: 2, 2: 4}


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _valid_rows(sx, matches, nA, capA):
    n = max(0, min(nA, capA))
    return np.flatnonzero((matches[:n] >= 0) & (sx[:n] >= 0))


def _rand_list(V, seed, model, iterations):
    S = SAMPLES[model]
    t = np.repeat(np.arange(iterations), S)
    s = np.tile(np.arange(S), iterations)
    j = sample_np(seed, t, s, S, np.full(t.shape, len(V)))
    return V[j].reshape(iterations, S).astype(np.int32)


STALE_ROWS = 64                                            # rows beyond capA in every synthetic source array


def _pair(rng, nA, capA, m_target, model):
    """A frame pair with nA source rows, about m_target valid rows (exactly, when small), a known motion, outliers,
    unmatched rows and matched rows with a negative source x (not valid). The arrays hold capA + STALE_ROWS rows, and
    every row at or beyond min(nA, capA) carries a stale match with src_x >= 0 (what a matcher result keeps from a larger
    frame): valid-looking rows the call must never read, because the device row count d_nA (or capA) excludes them."""
    rows = capA + STALE_ROWS
    nB = max(nA, 8) + 40
    sx = rng.uniform(0, 1900, rows).astype(np.float32)
    sy = rng.uniform(0, 1070, rows).astype(np.float32)
    if model == 0:
        M = np.array([[1, 0, 20.5], [0, 1, -11.25], [0, 0, 1.0]])
    elif model == 1:
        c, s = 1.05 * np.cos(0.1), 1.05 * np.sin(0.1)
        M = np.array([[c, -s, 30.0], [s, c, 12.0], [0, 0, 1.0]])
    else:
        M = np.array([[1.02, 0.03, 12.0], [-0.02, 0.98, -7.0], [1e-5, -2e-5, 1.0]])
    matches = np.full(rows, -1, np.int32)
    nv = min(nA, capA)
    if nv > 0:
        take = rng.permutation(nv)[:min(m_target, nv)]
        matches[take] = rng.permutation(nB)[:len(take)]
        if m_target > 50:
            extra = rng.permutation(nv)[:max(1, nv // 40)]
            sx[extra[(matches[extra] >= 0)][:2]] = -3.0               # matched, but not a valid row
    dx = rng.uniform(0, 1900, nB).astype(np.float32)
    dy = rng.uniform(0, 1070, nB).astype(np.float32)
    good = np.flatnonzero(matches >= 0)
    good = good[rng.random(len(good)) < 0.7]
    p = M @ np.stack([sx[good], sy[good], np.ones(len(good))])
    dx[matches[good]] = (p[0] / p[2]).astype(np.float32)
    dy[matches[good]] = (p[1] / p[2]).astype(np.float32)
    matches[nv:] = rng.integers(0, nB, rows - nv)
    assert (sx[nv:] >= 0).all()
    return sx, sy, dx, dy, matches


def _scenes(model, capA=2500, seed=0):
    """16 pairs: nA > capA (clipped), nA = 0, one valid row short of the minimum, exactly the minimum, a tiny m (repeated
    samples), then ordinary pairs."""
    rng = np.random.default_rng(100 + model + seed)
    mn = MIN_POINTS[model]
    specs = [(capA + 700, 1800), (0, 0), (40, mn - 1), (60, mn), (30, mn + 1)]
    specs += [(int(rng.integers(50, capA)), int(rng.integers(20, 1500))) for _ in range(11)]
    out = []
    for nA, m in specs:
        sx, sy, dx, dy, mt = _pair(rng, nA, capA, m, model)
        out.append(dict(nA=nA, sx=sx, sy=sy, dx=dx, dy=dy, matches=mt))
    return out


def _run(nm, dev, scenes, model, iterations, thr, seeds, capA):
    import torch
    T = lambda key: [_t(s[key], dev) for s in scenes]
    d_nA = [torch.tensor([s["nA"]], dtype=torch.int32, device=dev) for s in scenes]
    out = nm.ransac_batch_dev(model, T("sx"), T("sy"), d_nA, T("dx"), T("dy"), T("matches"), iterations=iterations,
                              threshold=thr, seeds=seeds, capA=capA, want_all=True)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _check_pair(nm, oracle, dev, sc, k, out, model, iterations, thr, seed, capA, also_gpu_ransac=True):
    import torch
    Hb, best, pos, status, Ha, inl = out
    V = _valid_rows(sc["sx"], sc["matches"], sc["nA"], capA)
    if len(V) < MIN_POINTS[model]:
        assert status[k] == 0 and best[k] == 0 and pos[k] == -1 and not Hb[k].any(), k
        assert not Ha[k].any() and not inl[k].any(), k
        return None
    assert status[k] == 1, k
    nv = max(0, min(sc["nA"], capA))
    aligned = oracle.align_points(sc["sx"][:nv], sc["sy"][:nv], sc["dx"], sc["dy"], sc["matches"][:nv])
    rl = _rand_list(V, seed, model, iterations)
    pos_r, Hb_r, Ha_r, inl_r = oracle.ransac(model, *aligned, rl, thr)
    assert np.array_equal(inl[k], inl_r), "pair %d: counts differ at %d hypotheses" % (k, (inl[k] != inl_r).sum())
    assert np.array_equal(_u32(Ha[k]), _u32(Ha_r)), "pair %d: hypotheses differ" % k
    assert pos[k] == pos_r and best[k] == inl_r[pos_r] and np.array_equal(_u32(Hb[k]), _u32(Hb_r)), k
    if also_gpu_ransac:                                  # the per-pair entry on the same aligned rows and sample list
        p1, Hb1, Ha1, inl1 = nm.ransac(model, *[_t(a, dev) for a in aligned], _t(rl, dev), thr)
        torch.cuda.synchronize()
        assert int(p1.item()) == pos[k] and np.array_equal(inl1.cpu().numpy(), inl[k])
        assert np.array_equal(_u32(Ha1.cpu().numpy()), _u32(Ha[k])) and np.array_equal(_u32(Hb1.cpu().numpy()), _u32(Hb[k]))
    return rl


@pytest.mark.parametrize("model", [0, 1, 2])
def test_batch_equals_oracle_on_synthetic_scenes(nm, oracle, cuda, model):
    capA, iterations, thr = 2500, 1000, 3.0                 # 1000 hypotheses: not a multiple of the 256 per workgroup
    scenes = _scenes(model, capA)
    seeds = [7 * k + 3 for k in range(16)]
    out = _run(nm, cuda, scenes, model, iterations, thr, seeds, capA)
    assert [o.shape[0] for o in out] == [16] * 6 and out[4].shape == (16, iterations, 9) and out[5].shape == (16, iterations)
    statuses = []
    dups = 0
    for k, sc in enumerate(scenes):
        rl = _check_pair(nm, oracle, cuda, sc, k, out, model, iterations, thr, seeds[k], capA)
        statuses.append(int(out[3][k]))
        if rl is not None and model > 0:
            dups += int(sum(len(set(r)) < len(r) for r in rl.tolist()))
    assert statuses[:5] == [1, 0, 0, 1, 1] and all(statuses[5:])
    # the clipped pair used only rows < capA, the tiny pair repeated samples (skipped hypotheses: zero H, zero count)
    assert len(_valid_rows(scenes[0]["sx"], scenes[0]["matches"], scenes[0]["nA"], capA)) > 1000
    if model > 0:
        assert dups > 0
        skipped = ~out[4][4].any(axis=1)
        assert skipped.any() and not out[5][4][skipped].any()
    assert (out[1][5:] > 0).all()


def test_prep_compacts_through_a_second_chunk_that_ends_inside_a_wave(nm, oracle, cuda):
    """capA = nA = 1024 + 65 with every third row unmatched: the prep kernel's ordered compaction takes a second chunk of 1024
    rows whose second wave holds one row. Hypotheses and counts equal the oracle's on the valid rows in ascending order."""
    model, capA, iterations, thr = 1, 1024 + 65, 300, 3.0
    sx, sy, dx, dy, mt = _pair(np.random.default_rng(321), capA, capA, capA, model)
    mt[:capA:3] = -1
    sc = dict(nA=capA, sx=sx, sy=sy, dx=dx, dy=dy, matches=mt)
    V = _valid_rows(sx, mt, capA, capA)
    assert 700 < len(V) < 730 and V[-1] == capA - 1, "the last row, alone in its wave, is valid"
    out = _run(nm, cuda, [sc], model, iterations, thr, [11], capA)
    assert _check_pair(nm, oracle, cuda, sc, 0, out, model, iterations, thr, 11, capA) is not None


def test_pair_result_independent_of_slot(nm, oracle, cuda):
    import torch
    model, capA, iterations, thr = 2, 2500, 700, 3.0
    scenes = _scenes(model, capA, seed=5)
    pick = scenes[9]
    alone = _run(nm, cuda, [pick], model, iterations, thr, [77], capA)
    batch = scenes[:5] + [pick] + scenes[5:9] + scenes[10:]
    seeds = [1000 + k for k in range(16)]
    seeds[5] = 77
    full = _run(nm, cuda, batch, model, iterations, thr, seeds, capA)
    for a, b in zip(alone, full):
        assert np.array_equal(np.ascontiguousarray(a[0]).view(np.uint32), np.ascontiguousarray(b[5]).view(np.uint32))
    _check_pair(nm, oracle, cuda, pick, 0, alone, model, iterations, thr, 77, capA, also_gpu_ransac=False)
    # another seed draws another sample list (and other hypotheses)
    other = _run(nm, cuda, [pick], model, iterations, thr, [78], capA)
    V = _valid_rows(pick["sx"], pick["matches"], pick["nA"], capA)
    assert not np.array_equal(_rand_list(V, 77, model, iterations), _rand_list(V, 78, model, iterations))
    assert not np.array_equal(other[4], alone[4])
    # default seeds are range(n): pair 0 of a call without seeds = seed 0
    T = lambda key: [_t(pick[key], cuda)]
    d = nm.ransac_batch_dev(model, T("sx"), T("sy"), [torch.tensor([pick["nA"]], dtype=torch.int32, device=cuda)],
                            T("dx"), T("dy"), T("matches"), iterations=iterations, threshold=thr, capA=capA)
    zero = _run(nm, cuda, [pick], model, iterations, thr, [0], capA)
    torch.cuda.synchronize()
    assert int(d[2][0].item()) == zero[2][0] and np.array_equal(d[0].cpu().numpy(), zero[0])


HOMOGRAPHIES = [
    [[0.995, 0.02, 9.0], [-0.015, 1.005, -6.0], [1.5e-5, -1e-5, 1.0]],
    [[1.0, 0.0, 14.0], [0.0, 1.0, 5.0], [0.0, 0.0, 1.0]],
    [[0.99, -0.03, -8.0], [0.03, 0.99, 11.0], [0.0, 0.0, 1.0]],
    [[1.01, 0.01, 4.0], [0.0, 1.02, -9.0], [1e-5, 1e-5, 1.0]],
    [[1.0, 0.01, 6.0], [-0.01, 1.0, 7.0], [0.0, 0.0, 1.0]],
    [[1.0, 0.02, -5.0], [-0.02, 1.0, 3.0], [-1e-5, 0.0, 1.0]],
    [[1.005, 0.0, -12.0], [0.0, 0.995, -4.0], [0.0, 1e-5, 1.0]],
    [[0.997, 0.015, 2.0], [-0.01, 0.993, 10.0], [1e-5, -1.5e-5, 1.0]],
]


def test_real_frames_detect_match_ransac_batch(nm, oracle, cuda):
    import torch
    w, h, cap, iterations, thr = 640, 480, 8192, 4096, 2.0
    Hs = [np.array(m, np.float32) for m in HOMOGRAPHIES]
    grays = []
    for k, Hk in enumerate(Hs):
        g = np.clip(H.blurred_frame(90 + k, w, h, sigma=2.0) * 1.4, 0, 255).astype(np.uint8)
        view0 = np.stack([g, np.roll(g, 3, 1), np.roll(g, 5, 0), np.full_like(g, 255)], -1)
        v0 = _t(view0, cuda)
        v1, _, _ = nm.resample_perspective(v0, w, h, _t(Hk, cuda), inverse=True)
        grays += [nm.grayscale(v0), nm.grayscale(v1)]
    arenas = [nm.SiftArena(w, h, cap) for _ in range(16)]
    # stale matches everywhere (the matcher writes rows < nA only): rows at or beyond nA must not count. Arena x / y beyond
    # num_items are 0, i.e. valid-looking source coordinates.
    res = [(torch.arange(cap, dtype=torch.int32, device=cuda) % 256).contiguous() for _ in range(8)]
    A, B = arenas[0::2], arenas[1::2]
    nm.detect_describe_batch(arenas, grays)                  # one call over the 16 frames
    nm.sift_match_batch_dev([a.desc for a in A], [a.num_items for a in A], [b.desc for b in B],
                            [b.num_items for b in B], res, 0.8)
    Hb, best, pos, status, Ha, inl = nm.ransac_batch_dev(2, [a.x for a in A], [a.y for a in A], [a.num_items for a in A],
                                                         [b.x for b in B], [b.y for b in B], res, iterations=iterations,
                                                         threshold=thr, seeds=list(range(40, 48)), want_all=True)
    torch.cuda.synchronize()
    out = [o.cpu().numpy() for o in (Hb, best, pos, status, Ha, inl)]
    far = []
    for k in range(8):
        nA, nB = int(A[k].num_items.item()), int(B[k].num_items.item())
        mt = res[k].cpu().numpy()
        assert nA > 300 and nB > 300 and (mt[:nA] >= 0).sum() > 80 and (mt[nA:] >= 0).all(), k
        sc = dict(nA=nA, sx=A[k].x.cpu().numpy(), sy=A[k].y.cpu().numpy(), dx=B[k].x[:nB].cpu().numpy(),
                  dy=B[k].y[:nB].cpu().numpy(), matches=mt)
        _check_pair(nm, oracle, cuda, sc, k, out, 2, iterations, thr, 40 + k, cap, also_gpu_ransac=False)
        matched = int((mt[:nA] >= 0).sum())
        Hn = out[0][k].reshape(3, 3).astype(np.float64) / out[0][k][8]
        assert out[1][k] > 0.5 * matched, k
        if not (np.allclose(Hn, Hs[k], atol=0.6, rtol=0.05) and np.allclose(Hn[:2, :2], Hs[k][:2, :2], atol=5e-3, rtol=0)):
            far.append((k, np.round(Hn, 5).tolist()))
    assert not far, far                                     # the recovered motions, within test_gpu_pipeline's tolerances
    for a in arenas:
        a.close()


def test_match_ransac_graph_replays_on_other_frames(nm, cuda):
    """match + RANSAC captured into one HIP graph: the RANSAC call reads the keypoint counts and matches on the device and
    allocates nothing, so a replay over other frames' descriptors, coordinates and counts written into the captured
    buffers equals eager calls on those frames."""
    import torch
    w, h, cap, iterations, thr = 640, 480, 8192, 1500, 2.0
    base = [H.blurred_frame(s, w, h) for s in (0, 1, 2, 3)]
    frames = []
    for k, f in enumerate(base):
        frames += [f, np.roll(f, (2 + k, 3), axis=(0, 1)).copy()]
    arenas = [nm.SiftArena(w, h, cap) for _ in frames]
    nm.detect_describe_batch(arenas, [_t(f, cuda) for f in frames])
    torch.cuda.synchronize()
    sets = [arenas[0:4], arenas[4:8]]                        # two pairs per set: (A0, B0, A1, B1)
    counts = [[int(a.num_items.item()) for a in s] for s in sets]
    assert counts[0] != counts[1]
    # the captured buffers: own tensors, loaded with set 0
    buf = [dict(desc=a.desc.clone(), x=a.x.clone(), y=a.y.clone(), n=a.num_items.clone()) for a in sets[0]]
    res = [torch.full((cap,), -1, dtype=torch.int32, device=cuda) for _ in range(2)]
    mws = nm.MatchBatchDevWorkspace(2, cap, cap, cuda)
    rws = nm.RansacBatchWorkspace(2, cap, iterations, cuda)
    s = torch.cuda.Stream()

    def enqueue(bufs, results):
        A, B = bufs[0::2], bufs[1::2]
        nm.sift_match_batch_dev([a["desc"] for a in A], [a["n"] for a in A], [b["desc"] for b in B], [b["n"] for b in B],
                                results, 0.8, workspace=mws)
        return nm.ransac_batch_dev(2, [a["x"] for a in A], [a["y"] for a in A], [a["n"] for a in A], [b["x"] for b in B],
                                   [b["y"] for b in B], results, iterations=iterations, threshold=thr, seeds=[5, 6],
                                   capA=cap, workspace=rws, want_all=True)
    with torch.cuda.stream(s):
        enqueue(buf, res)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        captured = enqueue(buf, res)
    def stale(results, bufs):
        """-1 below the pair's nA, stale in-range matches from row nA on (what a larger frame's result leaves there)."""
        for r, a in zip(results, bufs[0::2]):
            n = int(a["n"].item())
            r.fill_(-1)
            r[n:] = torch.arange(cap - n, dtype=torch.int32, device=cuda) % 256
    for src in sets:
        for b, a in zip(buf, src):
            b["desc"].copy_(a.desc); b["x"].copy_(a.x); b["y"].copy_(a.y); b["n"].copy_(a.num_items)
        stale(res, buf)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = [o.cpu().numpy().copy() for o in captured]
        got_res = [r.cpu().numpy().copy() for r in res]
        eager_bufs = [dict(desc=a.desc, x=a.x, y=a.y, n=a.num_items) for a in src]
        eager_res = [torch.empty((cap,), dtype=torch.int32, device=cuda) for _ in range(2)]
        stale(eager_res, eager_bufs)
        clean_res = [torch.full((cap,), -1, dtype=torch.int32, device=cuda) for _ in range(2)]
        with torch.cuda.stream(s):
            want = enqueue(eager_bufs, eager_res)
            clean = enqueue(eager_bufs, clean_res)
        torch.cuda.synchronize()
        for a, b in zip(want, clean):                        # the stale rows beyond nA changed nothing
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        for gr, er in zip(got_res, eager_res):
            assert np.array_equal(gr, er.cpu().numpy())
        for a, b in zip(got, want):
            b = b.cpu().numpy()
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
        assert (got[3] == 1).all() and (got[1] > 50).all()
    for a in arenas:
        a.close()
