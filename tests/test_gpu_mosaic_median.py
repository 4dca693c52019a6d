"""The device entry of the median mosaic composite: nm_mosaic_median_dev against its host twin bit for bit on every output, in
both modes (the host twin against the numpy model: tests/test_mosaic_median_host.py), at every stack depth, on tile and canvas
edges, with each optional output absent; sentinel-guarded outputs, slot independence, counts re-zeroed, one HIP graph of warp
tiles + median, and the whole path end to end on the ten loop-closure views with a painted occluder each (figures: DESIGN.md
section 7, "Median composite")."""
import numpy as np
import pytest

import bands_ref as B
import median_ref as M

pytestmark = pytest.mark.gpu

F32 = np.float32
MODES = (M.SELECT, M.MEAN)
INF = float("inf")


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run_dev(nm, cuda, tiles, recs, cap, cw, ch, mode, w_min=0.0, tau=INF, give=(True, True, True, True)):
    """nm_mosaic_median_dev on patterned outputs (canvas, weights, support, label, counts); give: which of the four optional
    outputs are passed (the others come back as their patterns)"""
    out = M.outputs(cw, ch, len(recs))
    d = [_t(out[0], cuda), _t(out[1], cuda), _t(out[2], cuda), _t(out[3], cuda), _t(out[4].view(np.int64), cuda)]
    opt = [t if g else None for t, g in zip(d[1:], give)]
    nm.mosaic_median(d[0], opt[0], _t(B.pack(tiles, cap, fill=np.nan), cuda), _t(B.records(recs), cuda), mode=mode, w_min=w_min,
                     tau=tau, support=opt[1], label=opt[2], counts=opt[3])
    h = [t.cpu().numpy() for t in d]
    h[4] = h[4].view(np.uint64)
    return h


def same(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", M.DEPTHS)
def test_device_equals_the_host_twin_at_every_stack_depth(nm, cuda, n, mode):
    """m = n at 40 pixels of each case and every depth below it elsewhere; the list holds 64 slots, and n = 63, 64 fill it"""
    tiles, recs, cap, cw, ch = M.stack_case(n)
    tau = INF if mode == M.SELECT else 0.15
    want = M.run_host(nm, tiles, recs, cap, cw, ch, mode, tau=tau)
    same(run_dev(nm, cuda, tiles, recs, cap, cw, ch, mode, tau=tau), want)
    assert want[4][:, 0].min() >= 8 * M.STACK_H and (want[0] != M.outputs(cw, ch, 1)[0]).any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", (1, 2, 17, 64))
def test_device_equals_the_host_twin_on_scattered_frames(nm, cuda, n, mode):
    tiles, recs, cap, cw, ch = B.case(n)
    want = M.run_host(nm, tiles, recs, cap, cw, ch, mode, w_min=0.75, tau=0.1)
    same(run_dev(nm, cuda, tiles, recs, cap, cw, ch, mode, w_min=0.75, tau=0.1), want)
    assert len(recs) == n and want[4][:, 1].any() == (n > 1)


@pytest.mark.parametrize("mode", MODES)
def test_device_equals_the_host_twin_on_tile_and_canvas_edges(nm, cuda, mode):
    """rectangles 63 / 64 / 65 x 3 / 4 / 5, a 1 x 1 one, every canvas edge and corner, rectangles off the canvas"""
    tiles, recs, cap, cw, ch = M.edge_scene()
    want = M.run_host(nm, tiles, recs, cap, cw, ch, mode, tau=0.2)
    same(run_dev(nm, cuda, tiles, recs, cap, cw, ch, mode, tau=0.2), want)
    assert (want[4][:19, 0] > 0).all() and not want[4][19:, 0].any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cw,ch", [(1, 1), (65, 5)])
def test_small_canvases(nm, cuda, cw, ch, mode):
    rng = np.random.default_rng(cw)
    recs = [(-3, -2, 70, 9, 1), (0, 0, 65, 5, 1), (cw - 1, ch - 1, 1, 1, 1), (-69, -8, 70, 9, 1), (0, 0, 1, 1, 1)]
    tiles = [B.texture(rng, r[2], r[3], holes=False) for r in recs]
    want = M.run_host(nm, tiles, recs, 70 * 9, cw, ch, mode, tau=0.1)
    same(run_dev(nm, cuda, tiles, recs, 70 * 9, cw, ch, mode, tau=0.1), want)
    assert want[4][:, 0].tolist() == [cw * ch, cw * ch, 1, 1, 1]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("give", [(False, False, False, False), (True, False, False, False), (False, True, False, False),
                                  (False, False, True, False), (False, False, False, True)])
def test_optional_outputs_absent_and_each_alone(nm, cuda, mode, give):
    tiles, recs, cap, cw, ch = M.stack_case(17)
    want = M.run_host(nm, tiles, recs, cap, cw, ch, mode, tau=0.15)
    pat = M.outputs(cw, ch, len(recs))
    got = run_dev(nm, cuda, tiles, recs, cap, cw, ch, mode, tau=0.15, give=give)
    same(got, [want[0]] + [w if g else p for w, p, g in zip(want[1:], pat[1:], give)])


@pytest.mark.parametrize("mode", MODES)
def test_nothing_is_written_outside_the_outputs(nm, cuda, mode):
    import torch
    tiles, recs, cap, cw, ch = M.edge_scene()
    n = len(recs)
    want = M.run_host(nm, tiles, recs, cap, cw, ch, mode, tau=0.2)
    pat = M.outputs(cw, ch, n)
    guard = 4096
    bufs = []
    for a in (pat[0], pat[1], pat[2], pat[3], pat[4].view(np.int64)):
        raw = torch.full((a.nbytes + 2 * guard,), 0xA5, dtype=torch.uint8, device=cuda)
        raw[guard:guard + a.nbytes] = _t(a.reshape(-1).view(np.uint8), cuda)
        bufs.append(raw)
    view = lambda raw, a, dt: raw[guard:guard + a.nbytes].view(dt).view(a.shape)
    d = [view(bufs[0], pat[0], torch.uint8), view(bufs[1], pat[1], torch.float32), view(bufs[2], pat[2], torch.uint8),
         view(bufs[3], pat[3], torch.uint8), view(bufs[4], pat[4], torch.int64)]
    d_tiles = torch.full(((n + 2) * cap * 4,), np.nan, dtype=torch.float32, device=cuda)
    d_tiles[cap * 4:(n + 1) * cap * 4] = _t(B.pack(tiles, cap, fill=np.nan).reshape(-1), cuda)
    before = d_tiles.clone()
    nm.mosaic_median(d[0], d[1], d_tiles[cap * 4:(n + 1) * cap * 4].view(n, cap, 4), _t(B.records(recs), cuda), mode=mode, tau=0.2,
                     support=d[2], label=d[3], counts=d[4])
    got = [t.cpu().numpy() for t in d]
    got[4] = got[4].view(np.uint64)
    same(got, want)
    for raw in bufs:
        h = raw.cpu().numpy()
        assert (h[:guard] == 0xA5).all() and (h[-guard:] == 0xA5).all()
    assert torch.equal(before.view(torch.int32), d_tiles.view(torch.int32))     # the tiles are read only


def test_a_pixels_result_does_not_depend_on_the_slots_of_other_frames(nm, cuda):
    rng = np.random.default_rng(21)
    cw, ch, cap = 400, 200, 67 * 45
    group = [((10, 10, 67, 45, 1), B.texture(rng, 67, 45)), ((40, 25, 67, 45, 1), B.texture(rng, 67, 45)),
             ((25, 40, 67, 45, 1), B.texture(rng, 67, 45))]
    far = [((150 + 80 * (j % 3), 5 + 50 * (j // 3), 67, 45, 1), B.texture(rng, 67, 45)) for j in range(9)]
    region = (slice(0, 100), slice(0, 120))

    def run(slots, n, mode):
        recs, tiles = [(0, 0, 0, 0, 0)] * n, [None] * n
        others = iter(far)
        for k in range(n):
            src = group[slots.index(k)] if k in slots else next(others, None)
            if src is not None:
                recs[k], tiles[k] = src
        return run_dev(nm, cuda, tiles, recs, cap, cw, ch, mode, tau=0.1)

    for mode in MODES:
        base = run([0, 1, 2], 3, mode)
        for slots, n in (([0, 1, 2], 12), ([3, 7, 11], 12), ([5, 20, 63], 64), ([0, 62, 63], 64)):
            got = run(slots, n, mode)
            for q in range(3):                           # canvas, weights, support: the same; labels and counts: renamed
                assert np.array_equal(got[q][region], base[q][region]), (slots, q)
            remap = np.arange(256)
            remap[slots] = (0, 1, 2)
            on = base[2][region] != M.outputs(cw, ch, 1)[2][region]
            assert np.array_equal(remap[got[3][region]][on], base[3][region][on])
            assert np.array_equal(got[4][slots], base[4])
        assert (base[0][region] != B.pattern(cw, ch)[0][region]).any()


def test_counts_are_zeroed_by_every_call(nm, cuda):
    tiles, recs, cap, cw, ch = M.stack_case(16)
    d_tiles, d_recs = _t(B.pack(tiles, cap, fill=np.nan), cuda), _t(B.records(recs), cuda)
    out = M.outputs(cw, ch, len(recs))
    canvas, counts = _t(out[0], cuda), _t(out[4].view(np.int64), cuda)
    want = M.run_host(nm, tiles, recs, cap, cw, ch, M.MEAN, tau=0.15)[4]
    for _ in range(2):
        nm.mosaic_median(canvas, None, d_tiles, d_recs, mode=M.MEAN, tau=0.15, counts=counts)
        assert np.array_equal(counts.cpu().numpy().view(np.uint64), want)


def _place(nm, K, dchain, LC, cw, ch, records, extent):
    import ctypes as C
    import torch
    status = nm.lib().nm_mosaic_place_f32(K, dchain.data_ptr(), None, LC.VW, LC.VH, cw, ch, LC.ORIGIN_X, LC.ORIGIN_Y,
                                          records.data_ptr(), extent.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert status == 0


def test_warp_tiles_and_median_in_one_graph_replayed_on_a_second_set_of_frames(nm, cuda):
    import torch
    from test_gpu_mosaic_bands import warp_records
    rng = np.random.default_rng(31)
    fw, fh, cw, ch = 67, 45, 140, 100
    recs = warp_records(fw, fh, cw, ch, fw + 6, fh + 6)
    recs[2, 9:14] = (30, 20, fw, fh, 1)
    recs[4, 9:11] = (60, 40)
    recs = recs[:5]
    n, cap = 5, (fw + 6) * (fh + 6)
    y, x = np.mgrid[0:fh, 0:fw]
    wts = _t(((1 + np.minimum(np.minimum(x, fw - 1 - x), np.minimum(y, fh - 1 - y))) / 32.0).astype(F32), cuda)
    mask = _t(np.full((fh, fw), 255, np.uint8), cuda)
    scenes = [[rng.integers(0, 256, (fh, fw, 4), dtype=np.uint8) for _ in range(n)] for _ in range(2)]
    gains = _t(rng.uniform(0.8, 1.25, (n, 3)).astype(F32), cuda)
    d_recs = _t(recs, cuda)
    frames = [_t(f, cuda) for f in scenes[0]]
    pat = M.outputs(cw, ch, n)

    def fresh():
        return [_t(pat[0], cuda), _t(pat[1], cuda), _t(pat[2], cuda), _t(pat[3], cuda), _t(pat[4].view(np.int64), cuda)]

    for mode in MODES:
        eager = []
        for sc in scenes:
            for f, src in zip(frames, sc):
                f.copy_(_t(src, cuda))
            o = fresh()
            tiles, _ = nm.mosaic_blend_median(o[0], o[1], frames, mask, wts, d_recs, gains=gains, mode=mode, tau=0.1, tile_cap=cap,
                                              support=o[2], label=o[3], counts=o[4])
            got = [t.cpu().numpy() for t in o]
            host = M.outputs(cw, ch, n)                   # the device's own tiles through the host twin
            nm.mosaic_median_host(host[0], host[1], tiles.cpu().numpy(), recs, mode=mode, tau=0.1, support=host[2], label=host[3],
                                  counts=host[4])
            got[4] = got[4].view(np.uint64)
            same(got, host)
            eager.append(got)
        assert not np.array_equal(eager[0][0], eager[1][0])
        o = fresh()
        tiles = torch.empty((n, cap, 4), dtype=torch.float32, device=cuda)
        stats = torch.empty(2, dtype=torch.int32, device=cuda)
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                nm.mosaic_blend_median(o[0], o[1], frames, mask, wts, d_recs, gains=gains, mode=mode, tau=0.1, tile_cap=cap,
                                       tiles=tiles, stats=stats, support=o[2], label=o[3], counts=o[4])
        for sc, want in zip(scenes, eager):
            for f, src in zip(frames, sc):
                f.copy_(_t(src, cuda))
            for t, p in zip(o, fresh()):
                t.copy_(p)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            got = [t.cpu().numpy() for t in o]
            got[4] = got[4].view(np.uint64)
            same(got, want)
        assert stats.cpu().tolist() == [5, 0]


def test_place_tiles_median_on_the_loop_closure_views_with_occluders(nm, cuda):
    """The ten loop-closure views, a saturated block painted into each at a view-dependent position: place -> warp tiles ->
    median on the device, gains from the host twins on the clean views. The device equals the host twin on its own tiles,
    and the model's ordering holds on the device's canvases: over the pixels with m >= 3 at which an occluded sample is valid,
    SELECT and MEAN are both closer (mean absolute byte difference) to the clean-frames feather canvas than the feather blend
    of the occluded frames is."""
    import torch
    import loop_closure_ref as LC
    tau = nm.MEDIAN_TAU
    fig, sel, occluded, (la, lb, Hs, chain), recs16, gains_host, clean = M.e2e_model(nm, 91, tau)
    assert fig["select"] < fig["feather"] and fig["mean"] < fig["feather"]                 # the model shows the ordering
    K, cw, ch, cap = LC.K, LC.SCENE_W, LC.SCENE_H, B.E2E_CAP
    frames = [_t(v, cuda) for v in occluded]
    gains, dchain = _t(gains_host, cuda), _t(chain, cuda)
    wts = _t(B.e2e_weights(), cuda)
    ones = torch.ones((LC.VH, LC.VW), dtype=torch.float32, device=cuda)
    records = torch.empty((K, 16), dtype=torch.int32, device=cuda)
    extent = torch.empty(4, dtype=torch.float32, device=cuda)
    _place(nm, K, dchain, LC, cw, ch, records, extent)
    assert np.array_equal(records.cpu().numpy(), recs16)
    tiles, tstats = nm.mosaic_warp_tiles(frames, ones, wts, records, gains=gains, tile_cap=cap)
    assert tstats.cpu().tolist() == [K, 0]
    h_tiles = tiles.cpu().numpy()
    dev = {}
    for mode in MODES:
        o = [torch.zeros((ch, cw, 4), dtype=torch.uint8, device=cuda), torch.zeros((ch, cw), dtype=torch.float32, device=cuda),
             torch.zeros((ch, cw), dtype=torch.uint8, device=cuda), torch.zeros((ch, cw), dtype=torch.uint8, device=cuda),
             torch.zeros((K, 2), dtype=torch.int64, device=cuda)]
        nm.mosaic_median(o[0], o[1], tiles, records, mode=mode, tau=tau, support=o[2], label=o[3], counts=o[4])
        got = [t.cpu().numpy() for t in o]
        got[4] = got[4].view(np.uint64)
        host = [np.zeros_like(g) for g in got]
        nm.mosaic_median_host(host[0], host[1], h_tiles, recs16, mode=mode, tau=tau, support=host[2], label=host[3], counts=host[4])
        same(got, host)
        dev[mode] = got
    fcanvas, fwts = torch.zeros((ch, cw, 4), dtype=torch.uint8, device=cuda), torch.zeros((ch, cw), dtype=torch.float32, device=cuda)
    nm.transform_blend_batch_gain(fcanvas, fwts, frames, ones, wts, records, gains=gains)
    d_feather = M.mean_abs_levels(fcanvas.cpu().numpy()[..., :3], clean, sel)
    d_select = M.mean_abs_levels(dev[M.SELECT][0][..., :3], clean, sel)
    d_mean = M.mean_abs_levels(dev[M.MEAN][0][..., :3], clean, sel)
    print("mean absolute byte difference to the clean feather canvas over %d pixels, tau %.3f: device feather %.3f, SELECT %.3f, "
          "MEAN %.3f; model feather %.3f, SELECT %.3f, MEAN %.3f; outlier pixels per frame %s"
          % (sel.sum(), tau, d_feather, d_select, d_mean, fig["feather"], fig["select"], fig["mean"],
             dev[M.MEAN][4][:, 1].tolist()))
    assert d_select < d_feather and d_mean < d_feather
