"""nm_ransac_refit_batch_dev_f32 on the MI355X: bit-identity with its host twin over models, rounds, batch sizes and mixed
pairs; slot independence; rounds = 0 against the batched RANSAC's own counts; sentinel-guarded outputs; the float64
one-round check of tests/test_ransac_refit_host.py on the device result; and the chain detect -> match -> RANSAC -> refit ->
plan -> blend captured into one HIP graph."""
import numpy as np
import pytest

import ransac_ref as R
import ransac_refit_ref as F

pytestmark = pytest.mark.gpu

THR = R.SWEEP_THR
CAP = 2048
OUT = ("H", "count", "status", "done", "mask", "rms")


def _u32(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _pair(model, seed, rows, motion="mild", frame=(1920, 1080), unmatched=(), perturb=1.0):
    """One pair's host arrays: source rows in A's order, destinations shuffled into B's order, matches mapping between them,
    and a deliberately rough input map (the true map with a translation error)."""
    rng = np.random.default_rng(1000 + seed)
    sx, sy, dx, dy = (np.zeros(CAP, np.float32) for _ in range(4))
    mt = np.full(CAP, -1, np.int32)
    H = R.motion_matrix(model, frame[0], frame[1], motion)
    if rows:
        sc = R.scene(model, frame[0], frame[1], rows, 0.35, 0.6, seed, motion, unmatched=unmatched)
        perm = rng.permutation(rows)
        sx[:rows], sy[:rows] = sc["sx"], sc["sy"]
        dx[perm], dy[perm] = sc["dx"], sc["dy"]
        mt[:rows] = perm
        mt[rng.choice(rows, rows // 10, replace=False)] = -1
        H = sc["M"].copy()
    H[0, 2] += perturb
    H[1, 2] -= 0.5 * perturb
    sx[rows:] = 5.0                                           # rows beyond nA hold plausible values that must not be read as rows
    return dict(sx=sx, sy=sy, dx=dx, dy=dy, mt=mt, nA=rows, H=(H / H[2, 2]).astype(np.float32).reshape(9))


def _host(nm, model, pairs, rounds, status=None, thr=THR):
    out = nm.ransac_refit_host(model, [p["sx"] for p in pairs], [p["sy"] for p in pairs], [p["nA"] for p in pairs],
                               [p["dx"] for p in pairs], [p["dy"] for p in pairs], [p["mt"] for p in pairs],
                               np.stack([p["H"] for p in pairs]), status=status, rounds=rounds, threshold=thr, capA=CAP,
                               want_mask=True, want_rms=True)
    return dict(zip(OUT, out))


def _upload(pairs, dev):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return [dict(sx=t(p["sx"]), sy=t(p["sy"]), dx=t(p["dx"]), dy=t(p["dy"]), mt=t(p["mt"]),
                 nA=t(np.array([p["nA"]], np.int32))) for p in pairs]


def _device(nm, model, pairs, rounds, dev, status=None, thr=THR, up=None):
    import torch
    up = _upload(pairs, dev) if up is None else up
    Hd = torch.from_numpy(np.stack([p["H"] for p in pairs])).to(dev)
    st = torch.from_numpy(np.asarray(status, np.int32)).to(dev) if status is not None else None
    out = nm.ransac_refit_batch_dev(model, [u["sx"] for u in up], [u["sy"] for u in up], [u["nA"] for u in up],
                                    [u["dx"] for u in up], [u["dy"] for u in up], [u["mt"] for u in up], Hd, status=st,
                                    rounds=rounds, threshold=thr, capA=CAP, want_mask=True, want_rms=True)
    torch.cuda.synchronize()
    return dict(zip(OUT, [o.cpu().numpy() for o in out]))


def _assert_same(a, b, what):
    for k in OUT:
        assert np.array_equal(_u32(a[k]), _u32(b[k])), (what, k)


def _mixed(model, n):
    sizes = [1500, 0, 700, 2048, 37, 1100, 3, 64, 65, 1999]
    motions = R.MOTIONS
    pairs = [_pair(model, 7 * k + model, sizes[k % len(sizes)], motions[k % len(motions)],
                   R.FRAMES[k % len(R.FRAMES)], unmatched=(1, 2) if sizes[k % len(sizes)] > 100 else ()) for k in range(n)]
    status = np.ones(n, np.int32)
    if n >= 3:
        status[2] = 0
    if n >= 16:
        status[9] = 5
        pairs[11]["H"][4] = np.nan
    return pairs, status


@pytest.mark.parametrize("n", [1, 3, 16, 64])
@pytest.mark.parametrize("model", [0, 1, 2])
def test_device_equals_host_twin(nm, cuda, model, n):
    pairs, status = _mixed(model, n)
    up = _upload(pairs, cuda)
    accepted = 0
    for rounds in range(5):
        want = _host(nm, model, pairs, rounds, status)
        got = _device(nm, model, pairs, rounds, cuda, status, up=up)
        _assert_same(got, want, "model %d n %d rounds %d" % (model, n, rounds))
        assert (got["count"] >= _host(nm, model, pairs, 0, status)["count"]).all() and (got["done"] <= rounds).all()
        assert np.array_equal(got["mask"].sum(axis=1), got["count"])
        assert np.array_equal(got["status"], (status == 1).astype(np.int32) * np.isfinite(np.stack([p["H"] for p in pairs])).all(axis=1))
        accepted += int(got["done"].sum())
    assert accepted > 0 or n == 1, "no pair ever accepted a round: the comparison covered nothing"
    # status_in = NULL means every pair is usable
    _assert_same(_device(nm, model, pairs, 2, cuda, None, up=up), _host(nm, model, pairs, 2, None), "status NULL")


@pytest.mark.parametrize("model", [0, 1, 2])
def test_slot_independence(nm, cuda, model):
    a, b = _pair(model, 5, 1800, "perspective"), _pair(model, 6, 900, "rot90", (3840, 2160))
    alone, other = _device(nm, model, [a], 3, cuda), _device(nm, model, [b], 3, cuda)
    assert alone["done"][0] > 0
    for n, slot in ((2, 1), (16, 7), (64, 63), (64, 0)):
        pairs = [b] * n
        pairs[slot] = a
        r = _device(nm, model, pairs, 3, cuda)
        for k in OUT:
            assert np.array_equal(_u32(r[k][slot]), _u32(alone[k][0])), (n, slot, k)
            assert np.array_equal(_u32(r[k][(slot + 1) % n]), _u32(other[k][0])), (n, slot, k)


@pytest.mark.parametrize("model", [0, 1, 2])
def test_rounds_0_reproduces_the_batched_ransac_count(nm, cuda, model):
    import torch
    pairs = [_pair(model, 40 + k, [1500, 800, 2048, 5, 0, 1200][k % 6], R.MOTIONS[k % 7]) for k in range(12)]
    up = _upload(pairs, cuda)
    args = ([u["sx"] for u in up], [u["sy"] for u in up], [u["nA"] for u in up], [u["dx"] for u in up], [u["dy"] for u in up],
            [u["mt"] for u in up])
    Hb, best, pos, status = nm.ransac_batch_dev(model, *args, iterations=512, threshold=THR, seeds=list(range(12)), capA=CAP)
    Ho, cnt, st, done = nm.ransac_refit_batch_dev(model, *args, Hb, status=status, rounds=0, threshold=THR, capA=CAP)
    torch.cuda.synchronize()
    assert torch.equal(cnt, best) and torch.equal(st, status) and not done.any()
    assert np.array_equal(_u32(Ho.cpu().numpy()), _u32(Hb.cpu().numpy()))
    assert int(status.sum()) >= 9 and int(best.max()) > 500
    Ho2, cnt2, st2, done2 = nm.ransac_refit_batch_dev(model, *args, Hb, status=status, rounds=2, threshold=THR, capA=CAP)
    torch.cuda.synchronize()
    assert (cnt2 >= best).all() and torch.equal(st2, status)


def test_outputs_are_written_inside_their_bounds(nm, cuda):
    """Every output lies inside one guarded buffer: n x 9, n and n x capA elements are written, nothing around them."""
    import ctypes as C
    import torch
    n, G = 5, 64
    pairs = [_pair(2, 70 + k, [1500, 0, 2048, 900, 33][k]) for k in range(n)]
    up = _upload(pairs, cuda)
    Hd = torch.from_numpy(np.stack([p["H"] for p in pairs])).to(cuda)
    st_in = torch.tensor([1, 1, 0, 1, 1], dtype=torch.int32, device=cuda)
    bufs = dict(H=torch.full((G + 9 * n + G,), -7.0, dtype=torch.float32, device=cuda),
                count=torch.full((G + n + G,), -7, dtype=torch.int32, device=cuda),
                status=torch.full((G + n + G,), -7, dtype=torch.int32, device=cuda),
                done=torch.full((G + n + G,), -7, dtype=torch.int32, device=cuda),
                mask=torch.full((G + n * CAP + G,), 0xA5, dtype=torch.uint8, device=cuda),
                rms=torch.full((G + n + G,), -7.0, dtype=torch.float32, device=cuda))
    inner = {k: b[G:-G] for k, b in bufs.items()}
    arr = lambda key: (C.c_void_p * n)(*[u[key].data_ptr() for u in up])
    rc = nm.lib().nm_ransac_refit_batch_dev_f32(2, n, arr("sx"), arr("sy"), arr("nA"), CAP, arr("dx"), arr("dy"), arr("mt"),
                                                Hd.data_ptr(), st_in.data_ptr(), THR, 3, inner["H"].data_ptr(),
                                                inner["count"].data_ptr(), inner["status"].data_ptr(), inner["done"].data_ptr(),
                                                inner["mask"].data_ptr(), inner["rms"].data_ptr(),
                                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    for k, b in bufs.items():
        guard = 0xA5 if k == "mask" else -7
        assert (b[:G] == guard).all() and (b[-G:] == guard).all(), k
    want = _host(nm, 2, pairs, 3, np.array([1, 1, 0, 1, 1], np.int32))
    assert np.array_equal(_u32(inner["H"].cpu().numpy().reshape(n, 9)), _u32(want["H"]))
    assert np.array_equal(inner["mask"].cpu().numpy().reshape(n, CAP), want["mask"])
    assert (inner["mask"] <= 1).all()
    for k in ("count", "status", "done", "rms"):
        assert np.array_equal(_u32(inner[k].cpu().numpy()), _u32(want[k])), k


@pytest.mark.parametrize("model,W,Hh", [(0, 1920, 1080), (1, 640, 480), (1, 7680, 4320), (2, 640, 480), (2, 1920, 1080),
                                        (2, 3840, 2160), (2, 7680, 4320)])
def test_one_round_against_float64_on_the_device(nm, oracle, cuda, model, W, Hh):
    """The check of test_ransac_refit_host.test_one_round_against_float64, on the device's maps: limit 4 x the largest corner
    displacement that rounding the float64 fit to float32 causes over the seven motions."""
    import torch
    pairs = []
    for motion, sc, rl in R.sweep(model, W, Hh):
        pos, Hb, Ha, inl = oracle.ransac(model, sc["sx"], sc["sy"], sc["dx"], sc["dy"], rl, THR)
        pad = lambda a, v: np.concatenate([a, np.full(CAP - len(a), v, a.dtype)])
        pairs.append(dict(sx=pad(sc["sx"], 0), sy=pad(sc["sy"], 0), dx=pad(sc["dx"], 0), dy=pad(sc["dy"], 0),
                          mt=pad(np.arange(R.SWEEP_POINTS, dtype=np.int32), -1), nA=R.SWEEP_POINTS,
                          H=np.asarray(Hb, np.float32).copy(), best=int(inl[int(pos)])))
    up = _upload(pairs, cuda)
    r0 = _device(nm, model, pairs, 0, cuda, up=up)
    r1 = _device(nm, model, pairs, 1, cuda, up=up)
    assert np.array_equal(r0["count"], [p["best"] for p in pairs])
    e_round, got = [], []
    for k, p in enumerate(pairs):
        S = r0["mask"][k, :R.SWEEP_POINTS].astype(bool)
        H64 = F.fit64(model, *(p[a][:R.SWEEP_POINTS][S] for a in ("sx", "sy", "dx", "dy")))
        e_round.append(F.rounding_error(H64, W, Hh))
        if r1["done"][k] == 1:
            got.append(F.corner_error(r1["H"][k], H64, W, Hh))
    limit = 4.0 * max(e_round)
    print("model %d %dx%d: e_round max %.3g  limit %.3g  device max %.3g over %d scenes" % (model, W, Hh, max(e_round), limit,
                                                                                          max(got), len(got)))
    assert len(got) >= (1 if model == 0 else 5) and max(got) <= limit, (got, limit)


def test_chain_with_refit_in_one_graph_replays_on_another_scene(nm, cuda):
    """detect -> match -> RANSAC -> refit -> plan -> blend on the eight synthetic views of test_gpu_mosaic, captured into one
    HIP graph on a single stream and replayed on a second scene: every output, the refit's included, equals the eager run."""
    import torch
    import test_gpu_mosaic as M

    class Chain(M._Chain):
        def enqueue(self, views):
            nm_ = self.nm
            A, B = self.arenas[:-1], self.arenas[1:]
            nm_.detect_describe_batch(self.arenas, [nm_.grayscale(v) for v in views])
            nm_.sift_match_batch_dev([a.desc for a in A], [a.num_items for a in A], [b.desc for b in B],
                                     [b.num_items for b in B], self.res, 0.8, workspace=self.mws)
            args = ([a.x for a in A], [a.y for a in A], [a.num_items for a in A], [b.x for b in B], [b.y for b in B], self.res)
            Hb, best, pos, status = nm_.ransac_batch_dev(2, *args, iterations=self.iterations, threshold=1.0,
                                                         seeds=list(range(7)), capA=M.CAP, workspace=self.rws)
            Hr, cnt, st, done, mask, rms = nm_.ransac_refit_batch_dev(2, *args, Hb, status=status, rounds=2, threshold=1.0,
                                                                      capA=M.CAP, want_mask=True, want_rms=True)
            records, chain, extent = nm_.mosaic_plan(Hr, st, M.VW, M.VH, M.SCENE_W, M.SCENE_H, self.ox, self.oy)
            self.canvas.zero_()
            self.cwts.zero_()
            nm_.transform_blend_batch(self.canvas, self.cwts, views, self.mask, self.wts, records)
            return Hb, best, status, Hr, cnt, st, done, mask, rms, records, chain, extent, self.canvas, self.cwts

    v1 = M._views(nm, cuda, M._scene(90))
    v2 = M._views(nm, cuda, M._scene(91))
    bufs = [v.clone() for v in v1]
    ch = Chain(nm, cuda)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ch.enqueue(bufs)                                  # warm-up outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        captured = ch.enqueue(bufs)
    for b, v in zip(bufs, v2):
        b.copy_(v)
    for r in ch.res:
        r.fill_(-1)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    got = [o.cpu().numpy().copy() for o in captured]
    with torch.cuda.stream(s):
        want = ch.enqueue([v.clone() for v in v2])
    torch.cuda.synchronize()
    want = [o.cpu().numpy().copy() for o in want]
    for a, b in zip(got, want):
        assert np.array_equal(_u32(a), _u32(b))
    Hb, best, status, Hr, cnt, st, done, mask, rms = got[:9]
    assert (status == 1).all() and (st == 1).all() and (cnt >= best).all() and (done <= 2).all() and done.sum() > 0
    assert np.array_equal(mask.sum(axis=1), cnt) and np.isfinite(Hr).all() and (rms < 1.0).all()
    assert got[12].max() > 0 and (got[9][:, 13] == 1).all()
    # for the record: how far the links are from the true pairwise maps before and after the refit
    maps = M._view_maps()
    err = lambda Hs: sum(F.corner_error(Hs[k], np.linalg.inv(maps[k + 1]) @ maps[k] / (np.linalg.inv(maps[k + 1]) @ maps[k])[2, 2],
                                        M.VW, M.VH) for k in range(7))
    print("corner error summed over 7 links: RANSAC %.3f px, refit %.3f px" % (err(Hb), err(Hr)))
    assert np.isfinite(err(Hr))
    ch.close()
