"""The device entry of the frame-weights stage: nm_frame_weights_batch_dev against its host twin bit for bit on masks (both
formats), weights, dist2 and counts (the host twin against the numpy model: tests/test_frame_weights_host.py), at every
shape of the host tests, with 64 frames, past the grid cap, at 1080p with R = 64, with every legal subset of the optional
outputs; one HIP graph of ingest, frame weights, warp tiles and median replayed on a second set of frames; the planes through
their consumers (the detector's mask, the feather blend); and the stage end to end on the loop-closure views with a disc
field of view (figures: DESIGN.md section 7, "Frame weights")."""
import ctypes as C
import itertools

import numpy as np
import pytest

import frame_weights_ref as FW

pytestmark = pytest.mark.gpu

F32 = np.float32
ALL = FW.KINDS + ("counts",)


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run_dev(nm, cuda, frames, **kw):
    base = kw.pop("base", None)
    mask, wts, d2, counts = nm.frame_weights_batch([f if hasattr(f, "is_cuda") else _t(f, cuda) for f in frames], want=FW.KINDS,
                                                   counts=True, base=None if base is None else _t(base, cuda), **kw)
    return dict(mask=mask.cpu().numpy(), wts=wts.cpu().numpy(), dist2=d2.cpu().numpy().view(np.uint16),
                counts=counts.cpu().numpy().view(np.uint64))


@pytest.mark.parametrize("fw,fh", FW.SHAPES)
def test_device_equals_the_host_twin(nm, cuda, fw, fh):
    """every radius, min_count, border and base of the host tests; margin and mask format alternate over the cases"""
    frames = FW.frames_for(fw, fh)
    d_frames = [_t(f, cuda) for f in frames]
    some_valid, case = False, 0
    for R in FW.RADII:
        for min_count in FW.MIN_COUNTS:
            for base in (None, FW.base_for(fw, fh)):
                for border in (True, False):
                    m = FW.margins(R)
                    kw = dict(lo=FW.LO, hi=FW.HI, R=R, margin=m[case % len(m)], min_count=min_count, border=border, base=base,
                              mask_format=(FW.U8N, FW.TEX_F32)[(case // 3) % 2])
                    case += 1
                    want = FW.run_host(nm, frames, **kw)
                    FW.same(run_dev(nm, cuda, d_frames, **kw), want)
                    some_valid |= bool((want["counts"][:, 1] > 0).all())
    assert some_valid


def test_sixty_four_small_frames(nm, cuda):
    frames = [FW.frames_for(33, 17, seed=s)[s % 3] for s in range(64)]
    for kw in (dict(R=8, margin=1, min_count=4), dict(R=31, margin=0, min_count=1, border=False, mask_format=FW.TEX_F32)):
        want = FW.run_host(nm, frames, lo=FW.LO, hi=FW.HI, **kw)
        FW.same(run_dev(nm, cuda, frames, lo=FW.LO, hi=FW.HI, **kw), want)
        assert (want["counts"][:, 1] > 0).all()


def test_more_units_than_the_grid_cap(nm, cuda):
    """64 frames of 300 x 200 are 1600 row-pass units and 640 column-pass units, below the default cap of 8 workgroups per
    compute unit; the cap is lowered to 48 through nm_frame_weights_set_grid_cap, so every workgroup walks many units of
    several frames (the counts are flushed at each change of frame), and the default cap is checked on the same input"""
    frames = [FW.frames_for(300, 200, seed=s % 4)[s % 3] for s in range(64)]
    kw = dict(lo=FW.LO, hi=FW.HI, R=8, margin=2, min_count=4, base=FW.base_for(300, 200))
    want = FW.run_host(nm, frames, **kw)
    d_frames = [_t(f, cuda) for f in frames]
    assert nm.frame_weights_set_grid_cap(48) == 0
    try:
        FW.same(run_dev(nm, cuda, d_frames, **kw), want)
    finally:
        assert nm.frame_weights_set_grid_cap(0) == 48
    FW.same(run_dev(nm, cuda, d_frames, **kw), want)
    assert (want["counts"] > 0).all()


def test_one_1080p_frame_at_radius_64(nm, cuda):
    rng = np.random.default_rng(8)
    fw, fh = 1920, 1080
    f = rng.integers(40, 220, (fh, fw, 4), dtype=np.uint8)
    y, x = np.mgrid[0:fh, 0:fw]
    f[(x - 960) ** 2 + (y - 540) ** 2 > 530 ** 2, :3] = 2                                  # the surround of a disc
    for _ in range(40):                                                                   # highlights and specks
        hy, hx, s = int(rng.integers(0, fh - 6)), int(rng.integers(0, fw - 6)), int(rng.integers(1, 6))
        f[hy:hy + s, hx:hx + s, :3] = 255
    for kw in (dict(R=64, margin=5, min_count=4), dict(R=64, margin=0, min_count=1, border=False)):
        want = FW.run_host(nm, [f], lo=FW.LO, hi=FW.HI, **kw)
        FW.same(run_dev(nm, cuda, [f], lo=FW.LO, hi=FW.HI, **kw), want)
        assert want["counts"][0, 1] > 500000 and want["dist2"].max() == 4096


# ---- optional outputs -------------------------------------------------------------------------------------------------------
def patterns(n, fw, fh, fmt):
    y, x = np.mgrid[0:fh, 0:fw]
    p = ((x * 7 + y * 3) % 251)[None] + np.arange(n)[:, None, None]
    return dict(mask=(p % 256).astype(np.uint8) if fmt == FW.U8N else (p + 1000).astype(F32), wts=(p + 2000).astype(F32),
                dist2=(p + 30000).astype(np.uint16), counts=np.full((n, 2), 1 << 40, np.uint64) + 7)


def raw_dev(nm, cuda, frames, give, fmt, **kw):
    """nm_frame_weights_batch_dev on patterned outputs with only the tables in `give` passed; returns every buffer"""
    import torch
    n, (fh, fw) = len(frames), frames[0].shape[:2]
    pat = patterns(n, fw, fh, fmt)
    d = dict(mask=_t(pat["mask"], cuda), wts=_t(pat["wts"], cuda), dist2=_t(pat["dist2"].view(np.int16), cuda),
             counts=_t(pat["counts"].view(np.int64), cuda))
    d_frames = [_t(f, cuda) for f in frames]
    ws = nm.FrameWeightsWorkspace(n, fw, fh, cuda)
    ws.buf.fill_(0xA5)
    table = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    arg = lambda q: table(list(d[q])) if q in give else None
    status = nm.lib().nm_frame_weights_batch_dev(n, table(d_frames), fw, fh, None, kw["lo"], kw["hi"], kw["min_count"], 1, kw["R"],
                                                 kw["margin"], arg("mask"), fmt, arg("wts"), arg("dist2"),
                                                 d["counts"].data_ptr() if "counts" in give else None, ws.buf.data_ptr(),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert status == 0
    torch.cuda.synchronize()
    return dict(mask=d["mask"].cpu().numpy(), wts=d["wts"].cpu().numpy(), dist2=d["dist2"].cpu().numpy().view(np.uint16),
                counts=d["counts"].cpu().numpy().view(np.uint64)), pat


SUBSETS = [s for r in range(1, 5) for s in itertools.combinations(ALL, r)]


@pytest.mark.parametrize("give", SUBSETS, ids=lambda s: "+".join(s))
def test_every_legal_subset_of_the_outputs(nm, cuda, give):
    frames = FW.frames_for(129, 70)
    kw = dict(lo=FW.LO, hi=FW.HI, R=8, margin=1, min_count=4)
    for fmt in (FW.U8N, FW.TEX_F32):
        want = FW.run_host(nm, frames, mask_format=fmt, **kw)
        got, pat = raw_dev(nm, cuda, frames, give, fmt, **kw)
        FW.same(got, {q: want[q] if q in give else pat[q] for q in ALL})


def test_counts_are_zeroed_by_every_call_and_the_workspace_is_scratch(nm, cuda):
    import torch
    frames = [_t(f, cuda) for f in FW.frames_for(129, 70)]
    kw = dict(lo=FW.LO, hi=FW.HI, R=8, margin=1, min_count=4)
    want = FW.run_host(nm, FW.frames_for(129, 70), **kw)
    ws = nm.FrameWeightsWorkspace(3, 129, 70, cuda)
    for fill in (0x00, 0xFF, 0x07):
        ws.buf.fill_(fill)
        mask, wts, d2, counts = nm.frame_weights_batch(frames, want=FW.KINDS, counts=True, workspace=ws, **kw)
        got = dict(mask=mask.cpu().numpy(), wts=wts.cpu().numpy(), dist2=d2.cpu().numpy().view(np.uint16),
                   counts=counts.cpu().numpy().view(np.uint64))
        FW.same(got, want)
    torch.cuda.synchronize()


# ---- one graph --------------------------------------------------------------------------------------------------------------
def test_ingest_weights_tiles_and_median_in_one_graph_replayed_on_a_second_set_of_frames(nm, cuda):
    import torch
    import median_ref as M
    from test_gpu_mosaic_bands import warp_records
    fw, fh, cw, ch = 67, 45, 140, 100
    recs = warp_records(fw, fh, cw, ch, fw + 6, fh + 6)
    recs[2, 9:14] = (30, 20, fw, fh, 1)
    recs[4, 9:11] = (60, 40)
    recs = recs[:5]
    n, cap = 5, (fw + 6) * (fh + 6)
    scenes = [(FW.frames_for(fw, fh, seed=s) + FW.frames_for(fw, fh, seed=s + 10))[:n] for s in (1, 2)]
    frames = [_t(f, cuda) for f in scenes[0]]
    d_recs = _t(recs, cuda)
    kw = dict(lo=FW.LO, hi=FW.HI, R=8, margin=1, min_count=4)
    pat = M.outputs(cw, ch, n)

    def chain(o, tiles=None, stats=None, workspace=None):
        gray = nm.ingest_batch(frames)
        mask, wts, fcounts = nm.frame_weights_batch(frames, counts=True, workspace=workspace, **kw)
        tiles, stats = nm.mosaic_blend_median(o[0], o[1], frames, list(mask), list(wts), d_recs, mode=M.SELECT, tau=0.1, tile_cap=cap,
                                              tiles=tiles, stats=stats, counts=o[2])
        return gray, mask, wts, fcounts

    def fresh():
        return [_t(pat[0], cuda), _t(pat[1], cuda), _t(pat[4].view(np.int64), cuda)]

    def read(o, res):
        return [t.cpu().numpy() for t in o] + [res[1].cpu().numpy(), res[2].cpu().numpy().view(np.uint32), res[3].cpu().numpy(),
                                               torch.stack(res[0]).cpu().numpy().view(np.uint32)]

    eager = []
    for sc in scenes:
        for f, src in zip(frames, sc):
            f.copy_(_t(src, cuda))
        o = fresh()
        got = read(o, chain(o))
        host = FW.run_host(nm, sc, **kw)
        assert np.array_equal(got[3], host["mask"]) and np.array_equal(got[4], host["wts"].view(np.uint32))
        assert np.array_equal(got[5].view(np.uint64), host["counts"]) and (host["counts"][:, 1] > 0).all()
        eager.append(got)
    assert not np.array_equal(eager[0][0], eager[1][0]) and not np.array_equal(eager[0][5], eager[1][5])
    o = fresh()
    tiles = torch.empty((n, cap, 4), dtype=torch.float32, device=cuda)
    stats = torch.empty(2, dtype=torch.int32, device=cuda)
    ws = nm.FrameWeightsWorkspace(n, fw, fh, cuda)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            res = chain(o, tiles, stats, ws)
    for sc, want in zip(scenes, eager):
        for f, src in zip(frames, sc):
            f.copy_(_t(src, cuda))
        for t, p in zip(o, fresh()):
            t.copy_(p)
        res[3].fill_(12345)                                  # the stage's counts must be re-zeroed by the replay
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(read(o, res), want):
            assert np.array_equal(a, b)


# ---- consumers --------------------------------------------------------------------------------------------------------------
def test_the_detector_takes_the_f32_mask_unchanged(nm, cuda):
    import torch
    fw, fh = 200, 150
    frame = FW.frames_for(fw, fh)[0]
    kw = dict(lo=FW.LO, hi=FW.HI, R=8, margin=3, min_count=4, mask_format=FW.TEX_F32)
    d_frame = _t(frame, cuda)
    d_mask = nm.frame_weights_batch([d_frame], want=("mask",), **kw)
    h_mask = nm.frame_weights_host([frame], want=("mask",), **kw)
    assert d_mask.dtype == torch.float32 and 0 < h_mask.sum() < fw * fh
    gray = nm.grayscale(d_frame)
    found = []
    for mask in (d_mask[0], _t(h_mask[0], cuda), None):
        arena = nm.SiftArena(fw, fh, 16384)
        arena.set_mask(mask)
        arena.detect_describe(gray)
        torch.cuda.synchronize()
        k = int(arena.num_items.cpu()[0])
        found.append((k, arena.x[:k].cpu().numpy().copy(), arena.y[:k].cpu().numpy().copy(), arena.desc[:k].cpu().numpy().copy()))
        arena.close()
    assert found[0][0] == found[1][0] and 0 < found[0][0] < found[2][0]
    for a, b in zip(found[0][1:], found[1][1:]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_end_to_end_on_the_device_equals_the_host_chain(nm, oracle, cuda):
    """The loop-closure views with a disc field of view and a saturated block each: the device's U8N masks and weights equal
    the host twin's, nm_transform_blend_batch takes them as they are and its canvas equals the CPU oracle's blend of the host
    twin's planes bit for bit, and on the device canvases the stage is closer to the clean-frames canvas than the rectangle
    feather with an all-ones mask (the figures are those of tests/test_frame_weights_host.py, the canvases being equal)."""
    import torch
    import bands_ref as B
    import loop_closure_ref as LC
    e = FW.e2e_host(nm, oracle)
    K, cw, ch = LC.K, LC.SCENE_W, LC.SCENE_H
    frames = [_t(v, cuda) for v in e["views"]]
    mask, wts, counts = nm.frame_weights_batch(frames, counts=True, **FW.E2E)
    assert np.array_equal(mask.cpu().numpy(), e["mask"]) and np.array_equal(wts.cpu().numpy().view(np.uint32), e["wts"].view(np.uint32))
    assert np.array_equal(counts.cpu().numpy()[:, 1], (e["mask"] == 255).reshape(K, -1).sum(axis=1)) and (counts.cpu().numpy()[:, 1] > 0).all()
    recs = _t(e["recs16"], cuda)

    def blend(views, masks, weights):
        c = torch.zeros((ch, cw, 4), dtype=torch.uint8, device=cuda)
        w = torch.zeros((ch, cw), dtype=torch.float32, device=cuda)
        nm.transform_blend_batch(c, w, views, masks, weights, recs)
        return c.cpu().numpy(), w.cpu().numpy()

    ones, rect = torch.full((LC.VH, LC.VW), 255, dtype=torch.uint8, device=cuda), _t(B.e2e_weights(), cuda)
    stage = blend(frames, list(mask), list(wts))
    plain = blend(frames, ones, rect)
    clean = blend([_t(v, cuda) for v in B.e2e_views(91)], ones, rect)
    for got, want in ((stage, e["stage"]), (plain, e["plain"]), (clean, e["clean"])):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    sel = stage[1] > 0
    d_stage, d_plain = FW.mean_abs(stage[0], clean[0], sel), FW.mean_abs(plain[0], clean[0], sel)
    print("device canvases, mean absolute byte difference to the clean feather canvas over %d pixels: stage %.3f, rectangle "
          "feather %.3f" % (sel.sum(), d_stage, d_plain))
    assert sel.sum() > 100000 and d_stage < d_plain
