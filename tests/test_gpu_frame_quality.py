"""The device entries of the frame-quality stage against their host twins, bit for bit (the host twins against the numpy model:
tests/test_frame_quality_host.py): nm_frame_quality_batch_dev at every shape of the host tests, with 64 frames, past the grid
cap, at 1080p and on frames narrower than a block; nm_keyframe_pick_dev on every case of the host tests;
nm_slots_gather_dev on both paths with sentinels round every slot; and ingest, frame weights, frame quality, pick, gather,
plan and blend as one HIP graph replayed on two sets of frames."""
import numpy as np
import pytest

import frame_quality_ref as FQ

pytestmark = pytest.mark.gpu

F32 = np.float32


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def dev_stats(nm, cuda, frames, masks=None, **kw):
    d_frames = [f if hasattr(f, "is_cuda") else _t(f, cuda) for f in frames]
    d_masks = None if masks is None else [m if hasattr(m, "is_cuda") else _t(m, cuda) for m in masks]
    return nm.frame_quality_batch(d_frames, masks=d_masks, **kw).cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("fw,fh", FQ.SHAPES)
def test_device_statistics_equal_the_host_twin(nm, cuda, fw, fh):
    frames = FQ.frames_for(fw, fh)
    d_frames = [_t(f, cuda) for f in frames]
    for grid in FQ.grids_for(fw, fh):
        for masks in (None, FQ.masks_for(fw, fh, FQ.U8N), FQ.masks_for(fw, fh, FQ.TEX_F32)):
            for lo, hi in ((FQ.LO, FQ.HI), (0, 255)):
                want = nm.frame_quality_host(frames, masks=masks, lo=lo, hi=hi, grid=grid)
                assert np.array_equal(dev_stats(nm, cuda, d_frames, masks, lo=lo, hi=hi, grid=grid), want), (grid, lo, hi)


def test_sixty_four_small_frames_one_frame_and_garbage_in_stats(nm, cuda):
    import torch
    frames = [FQ.frames_for(33, 17, seed=s)[s % 3] for s in range(64)]
    masks = [FQ.masks_for(33, 17, FQ.U8N, seed=s)[s % 3] for s in range(64)]
    want = nm.frame_quality_host(frames, masks=masks, lo=FQ.LO, hi=FQ.HI, grid=(4, 3))
    stats = torch.full((64, 3, 4, 8), 0x5EED5EED5EED, dtype=torch.int64, device=cuda)
    got = nm.frame_quality_batch([_t(f, cuda) for f in frames], masks=[_t(m, cuda) for m in masks], lo=FQ.LO, hi=FQ.HI, grid=(4, 3),
                                 stats=stats)
    assert got is stats and np.array_equal(got.cpu().numpy().view(np.uint64), want) and want[..., 0].any()
    for k in (0, 63):                                              # n = 1 against n = 64, and a repeated pointer
        f = _t(frames[k], cuda)
        one = dev_stats(nm, cuda, [f, f], [masks[k], masks[k]], lo=FQ.LO, hi=FQ.HI, grid=(4, 3))
        assert np.array_equal(one[0], want[k]) and np.array_equal(one[1], want[k])
        assert np.array_equal(dev_stats(nm, cuda, [f], [masks[k]], lo=FQ.LO, hi=FQ.HI, grid=(4, 3))[0], want[k])


def test_more_units_than_the_grid_cap(nm, cuda):
    """64 frames of 300 x 200 are 640 units; with the cap at 48 every workgroup walks 13 or 14 units of several frames (the
    LDS table is flushed at each change of frame); the default cap is checked on the same input"""
    frames = [FQ.frames_for(300, 200, seed=s % 4)[s % 3] for s in range(64)]
    masks = [FQ.masks_for(300, 200, FQ.TEX_F32, seed=s % 2)[s % 3] for s in range(64)]
    want = nm.frame_quality_host(frames, masks=masks, lo=FQ.LO, hi=FQ.HI, grid=(5, 7))
    d_frames, d_masks = [_t(f, cuda) for f in frames], [_t(m, cuda) for m in masks]
    assert nm.frame_quality_set_grid_cap(48) == 0
    try:
        assert np.array_equal(dev_stats(nm, cuda, d_frames, d_masks, lo=FQ.LO, hi=FQ.HI, grid=(5, 7)), want)
    finally:
        assert nm.frame_quality_set_grid_cap(0) == 48
    assert np.array_equal(dev_stats(nm, cuda, d_frames, d_masks, lo=FQ.LO, hi=FQ.HI, grid=(5, 7)), want)
    assert want[..., 0].all() and want[..., 5].any() and want[..., 6].any()


def test_one_1080p_frame_on_eight_by_eight_cells(nm, cuda):
    rng = np.random.default_rng(8)
    fw, fh = 1920, 1080
    f = rng.integers(40, 220, (fh, fw, 4), dtype=np.uint8)
    y, x = np.mgrid[0:fh, 0:fw]
    f[(x - 960) ** 2 + (y - 540) ** 2 > 530 ** 2, :3] = 2
    f[500:520, 900:1000, :3] = 255
    for masks in (None, [((x - 960) ** 2 + (y - 540) ** 2 < 500 ** 2).astype(np.uint8) * 255]):
        want = nm.frame_quality_host([f], masks=masks, lo=10, hi=250, grid=(8, 8))
        assert np.array_equal(dev_stats(nm, cuda, [f], masks, lo=10, hi=250, grid=(8, 8)), want)
        assert want[..., 0].sum() > 500000 and want[..., 6].sum() == 2000


@pytest.mark.parametrize("fw,fh,grid", [(9, 40, (8, 8)), (9, 9, (8, 8)), (70, 300, (8, 8)), (130, 129, (7, 5))])
def test_narrow_frames_whose_blocks_span_many_cells(nm, cuda, fw, fh, grid):
    frames = FQ.frames_for(fw, fh, seed=3)
    for masks in (None, FQ.masks_for(fw, fh, FQ.U8N)):
        want = nm.frame_quality_host(frames, masks=masks, lo=FQ.LO, hi=FQ.HI, grid=grid)
        assert np.array_equal(dev_stats(nm, cuda, frames, masks, lo=FQ.LO, hi=FQ.HI, grid=grid), want)


# ---- pick and gather ----------------------------------------------------------------------------------------------------------
CASES = FQ.pick_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_pick_equals_the_host_twin(nm, cuda, name):
    stats, chain, fw, fh, keep, status, kw = CASES[name]
    want = nm.keyframe_pick_host(stats, chain, fw, fh, keep, frame_status=status, **kw)
    got = nm.keyframe_pick(_t(stats.view(np.int64), cuda), _t(chain, cuda), fw, fh, keep,
                           frame_status=None if status is None else _t(status, cuda), **kw)
    FQ.same_pick({k: v.cpu().numpy() for k, v in got._asdict().items()}, want._asdict())


def test_device_pick_on_the_end_to_end_pan(nm, cuda):
    import loop_closure_ref as LC
    e = FQ.e2e()
    frames = [_t(v, cuda) for v in e["views"]]
    stats = nm.frame_quality_batch(frames, **FQ.E2E_QUALITY)
    assert np.array_equal(stats.cpu().numpy().view(np.uint64), e["stats_model"])
    got = nm.keyframe_pick(stats, _t(e["chain"], cuda), LC.VW, LC.VH, FQ.E2E_KEEP, **FQ.E2E_PICK)
    got = {k: v.cpu().numpy() for k, v in got._asdict().items()}
    FQ.same_pick(got, nm.keyframe_pick_host(e["stats_model"], e["chain"], LC.VW, LC.VH, FQ.E2E_KEEP, **FQ.E2E_PICK)._asdict())
    FQ.e2e_conditions(got, e)


@pytest.mark.parametrize("size", [1, 15, 16, 17, 4 * 33 * 17, 70000])
def test_device_gather(nm, cuda, size):
    rng = np.random.default_rng(size)
    n = 5
    keys = np.array([3, -1, n, 3, 0, 4, 1 << 30, -(1 << 31)], np.int32)
    for offset in (0, 1):
        pool = rng.integers(0, 256, (n, size + 64), dtype=np.uint8)
        d_pool = _t(pool, cuda)
        out = _t(np.full((len(keys), size + 64), 0xA5, np.uint8), cuda)
        got = nm.slots_gather(_t(keys, cuda), [d_pool[k, offset:offset + size] for k in range(n)],
                              dst=[out[i, 16 + offset:16 + offset + size] for i in range(len(keys))], fill=0x3C)
        want = FQ.gather_model(keys, [pool[k, offset:offset + size] for k in range(n)], 0x3C)
        assert np.array_equal(np.stack([g.cpu().numpy() for g in got]), want)
        o = out.cpu().numpy()
        assert (o[:, :16 + offset] == 0xA5).all() and (o[:, 16 + offset + size:] == 0xA5).all()
        assert (o[1, 16 + offset:16 + offset + size] == 0x3C).all()              # an absent slot holds the fill
    frames = FQ.frames_for(33, 17)
    got = nm.slots_gather(_t(np.array([2, 2, -1, 0], np.int32), cuda), [_t(f, cuda) for f in frames])
    assert np.array_equal(np.stack([g.cpu().numpy() for g in got]), FQ.gather_model([2, 2, -1, 0], frames, 0))
    counts = [_t(np.array([k + 10], np.int32), cuda) for k in range(3)]         # single count words
    got = nm.slots_gather(_t(np.array([1, 5], np.int32), cuda), counts, fill=0xFF)
    assert [int(g.cpu()[0]) for g in got] == [11, -1]


# ---- one graph ----------------------------------------------------------------------------------------------------------------
N, KEEP, GFW, GFH, GCW, GCH = 12, 6, 67, 45, 200, 80
G_WEIGHTS = dict(lo=12, hi=245, R=6, margin=1, min_count=2)
G_QUALITY = dict(lo=12, hi=245, grid=(2, 2))
G_PICK = dict(cell_min=16, min_pixels=100, d_min=8.0, d_max=20.0, rel=0.7, w=2)


def graph_scene(seed):
    """12 views of a smooth texture on a pan of 5 px per frame; some blurred, one with a saturated block"""
    import helpers
    rng = np.random.default_rng(seed)
    g = np.clip(helpers.blurred_frame(seed, 160, GFH + 8, sigma=1.2) * 1.4, 0, 255).astype(np.uint8)
    scene = np.stack([g, np.roll(g, 3, 1), np.roll(g, 5, 0), np.full_like(g, 255)], -1)
    views = []
    for k in range(N):
        v = scene[2 + k % 3:2 + k % 3 + GFH, 5 * k:5 * k + GFW].copy()
        if (k + seed) % 3 == 1:
            p = np.pad(v.astype(np.int64), ((0, 0), (2, 2), (0, 0)), mode="edge")
            v = ((p[:, 0:-4] + p[:, 1:-3] + p[:, 2:-2] + p[:, 3:-1] + p[:, 4:] + 2) // 5).astype(np.uint8)
        y0 = int(rng.integers(0, GFH - 6))
        v[y0:y0 + 4, 10:15, :3] = 255
        views.append(np.ascontiguousarray(v))
    chain = np.stack([np.array([1, 0, -5.0 * k, 0, 1, -float(k % 3), 0, 0, 1], F32) for k in range(N)])
    return views, chain


def test_ingest_weights_quality_pick_gather_plan_and_blend_in_one_graph(nm, cuda):
    import torch
    scenes = [graph_scene(s) for s in (1, 2)]
    frames = [_t(f, cuda) for f in scenes[0][0]]
    d_chain = _t(scenes[0][1], cuda)
    stats = torch.empty((N, 2, 2, 8), dtype=torch.int64, device=cuda)

    def chain(canvas, cwts):
        nm.ingest_batch(frames)
        mask, wts = nm.frame_weights_batch(frames, **G_WEIGHTS)
        nm.frame_quality_batch(frames, masks=list(mask), stats=stats, **G_QUALITY)
        pick = nm.keyframe_pick(stats, d_chain, GFW, GFH, KEEP, **G_PICK)
        kf, km, kw = (nm.slots_gather(pick.keys, list(t)) for t in (frames, mask, wts))
        recs, _, _ = nm.mosaic_plan(pick.H_keys, pick.H_status, GFW, GFH, GCW, GCH, 4, 6)
        nm.transform_blend_batch(canvas, cwts, kf, km, kw, recs)
        return pick, recs, kf

    def fresh():
        return torch.zeros((GCH, GCW, 4), dtype=torch.uint8, device=cuda), torch.zeros((GCH, GCW), dtype=torch.float32, device=cuda)

    eager = []
    for views, ch in scenes:
        for f, src in zip(frames, views):
            f.copy_(_t(src, cuda))
        d_chain.copy_(_t(ch, cuda))
        canvas, cwts = fresh()
        pick, recs, kf = chain(canvas, cwts)
        # the host chain: weights, statistics, pick, gather and plan on the host, then the device's blend of its planes
        h_mask, h_wts = nm.frame_weights_host(views, **G_WEIGHTS)
        h_stats = nm.frame_quality_host(views, masks=list(h_mask), **G_QUALITY)
        h_pick = nm.keyframe_pick_host(h_stats, ch, GFW, GFH, KEEP, **G_PICK)
        FQ.same_pick({k: v.cpu().numpy() for k, v in pick._asdict().items()}, h_pick._asdict())
        assert 3 <= h_pick.key_count[0] <= KEEP and np.array_equal(stats.cpu().numpy().view(np.uint64), h_stats)
        h_kf, h_km, h_kw = (nm.slots_gather_host(h_pick.keys, list(t)) for t in (views, h_mask, h_wts))
        h_recs = nm.mosaic_plan_host(h_pick.H_keys, h_pick.H_status, GFW, GFH, GCW, GCH, 4, 6)[0]
        assert np.array_equal(recs.cpu().numpy(), h_recs) and h_recs[:h_pick.key_count[0], 13].all()
        assert np.array_equal(torch.stack(kf).cpu().numpy(), np.stack(h_kf))
        h_canvas, h_cwts = fresh()
        nm.transform_blend_batch(h_canvas, h_cwts, [_t(a, cuda) for a in h_kf], [_t(a, cuda) for a in h_km],
                                 [_t(a, cuda) for a in h_kw], _t(h_recs, cuda))
        assert torch.equal(canvas, h_canvas) and torch.equal(cwts.view(torch.int32), h_cwts.view(torch.int32)) and (cwts > 0).sum() > 2000
        eager.append((canvas.cpu().numpy(), cwts.cpu().numpy(), pick.keys.cpu().numpy(), pick.key_count.cpu().numpy()))
    assert not np.array_equal(eager[0][2], eager[1][2]) and not np.array_equal(eager[0][0], eager[1][0])
    canvas, cwts = fresh()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            pick, recs, kf = chain(canvas, cwts)
    for (views, ch), want in zip(scenes, eager):
        for f, src in zip(frames, views):
            f.copy_(_t(src, cuda))
        d_chain.copy_(_t(ch, cuda))
        canvas.zero_(), cwts.zero_()
        stats.fill_(0x7777777777), pick.keys.fill_(9), pick.key_count.fill_(9)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = (canvas.cpu().numpy(), cwts.cpu().numpy(), pick.keys.cpu().numpy(), pick.key_count.cpu().numpy())
        for a, b in zip(got, want):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
