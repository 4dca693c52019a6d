"""The device entries of the two-band mosaic blend: nm_mosaic_warp_tiles pinned against the bytes and weights that
nm_transform_blend_batch_gain writes for each record alone, nm_mosaic_bands_dev against its host twin bit for bit (the host
twin against the float64 model: tests/test_mosaic_bands_host.py), slot independence, and the whole path end to end on the
ten loop-closure views (figures: DESIGN.md section 7, "Two-band blend")."""
import numpy as np
import pytest

import bands_ref as B

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = -77.0


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def warp_records(fw, fh, cw, ch, cap_w, cap_h):
    """records with real maps (local canvas pixel -> frame pixel): two ordinary ones, one unplaced, one partly off the canvas
    at the top left, one wholly off it, one a pixel over tile_cap = cap_w * cap_h"""
    def rec(tx, ty, nw, nh, placed, a=0.03, s=1.02, dx=-3.0, dy=-2.0, p=1e-5):
        m = np.array([s * np.cos(a), -s * np.sin(a), dx, s * np.sin(a), s * np.cos(a), dy, p, -p, 1.0], F32)
        r = np.zeros(16, np.int32)
        r[:9] = m.view(np.int32)
        r[9:14] = (tx, ty, nw, nh, placed)
        return r
    return np.stack([rec(4, 3, cap_w, cap_h, 1), rec(20, 11, cap_w - 7, cap_h - 5, 1, a=-0.05, s=0.97, dx=2.5, dy=1.5),
                     rec(8, 8, cap_w, cap_h, 0), rec(-9, -6, cap_w - 1, cap_h, 1, a=0.0, s=1.0, dx=0.0, dy=0.0, p=0.0),
                     rec(cw + 5, 2, cap_w, cap_h, 1), rec(1, 1, cap_w * cap_h + 1, 1, 1)])


def check_warp_tiles(nm, cuda, frames, mask, wts, recs, d_gains, cap, cw, ch, want_stats):
    """nm_mosaic_warp_tiles on device frames, mask and weights with the (n, 16) records `recs`: every used record's tile
    against the canvas weights (exactly) and bytes that nm_transform_blend_batch_gain writes for that record alone, nothing
    written beyond a rectangle or into a skipped frame's slot or outside the slots. Returns the sentinel-guarded tiles."""
    import torch
    n = len(recs)
    d_recs = _t(recs, cuda)
    whole = torch.full((n + 2, cap, 4), SENTINEL, dtype=torch.float32, device=cuda)
    tiles, stats = nm.mosaic_warp_tiles(frames, mask, wts, d_recs, gains=d_gains, tile_cap=cap, tiles=whole[1:n + 1])
    h = whole.cpu().numpy()
    assert (h[0] == SENTINEL).all() and (h[-1] == SENTINEL).all()
    assert stats.cpu().tolist() == want_stats
    t = h[1:n + 1]
    for k in range(n):
        tx, ty, nw, nh, placed = (int(v) for v in recs[k, 9:14])
        if not placed or nw * nh > cap:
            assert (t[k] == SENTINEL).all(), k                              # a skipped frame's slot is never written
            continue
        assert (t[k, nw * nh:] == SENTINEL).all(), k                        # nothing beyond the rectangle
        tile = t[k, :nw * nh].reshape(nh, nw, 4)
        assert np.isfinite(tile).all() and (tile[..., 3] >= 0).all()
        assert (tile[tile[..., 3] == 0] == 0).all()                         # invalid: C = 0, w = 0
        canvas = torch.zeros((ch, cw, 4), dtype=torch.uint8, device=cuda)
        cwts = torch.zeros((ch, cw), dtype=torch.float32, device=cuda)
        nm.transform_blend_batch_gain(canvas, cwts, [frames[k]], mask, wts, d_recs[k:k + 1],
                                      None if d_gains is None else d_gains[k:k + 1].contiguous())
        c = B._clip((tx, ty, nw, nh, 1), cw, ch)
        if c is None:
            assert not cwts.any().item()
            continue
        cs, ls = c
        hw, hc = cwts.cpu().numpy(), canvas.cpu().numpy()
        assert np.array_equal(tile[ls][..., 3], hw[cs]), k                  # w is the blend's canvas weight, exactly
        on = hw[cs] > 0
        assert on.sum() > 500
        assert np.array_equal(B.store_f32(tile[ls][..., :3])[on], hc[cs][..., :3][on]), k
        outside = np.ones((ch, cw), bool)
        outside[cs] = False
        assert not hw[outside].any()
    return whole


@pytest.mark.parametrize("fw,fh", [(67, 45), (131, 97)])
@pytest.mark.parametrize("mask_u8,wts_u8", [(True, False), (False, True)])
@pytest.mark.parametrize("gain_kind", ["none", "unit", "random"])
def test_warp_tiles_equal_the_gained_blend_of_each_record_alone(nm, cuda, fw, fh, mask_u8, wts_u8, gain_kind):
    import torch
    rng = np.random.default_rng(fw + 2 * mask_u8 + wts_u8)
    cw, ch = fw + 40, fh + 30
    cap_w, cap_h = fw + 6, fh + 6
    cap = cap_w * cap_h
    recs = warp_records(fw, fh, cw, ch, cap_w, cap_h)
    n = len(recs)
    base = [_t(rng.integers(0, 256, (fh, fw, 4), dtype=np.uint8), cuda) for _ in range(2)]
    frames = [base[k % 2] for k in range(n)]                               # repeated pointers
    y, x = np.mgrid[0:fh, 0:fw]
    disc = ((x - fw / 2) ** 2 / (fw / 2) ** 2 + (y - fh / 2) ** 2 / (fh / 2) ** 2) < 0.95
    feather = (np.minimum(np.minimum(x, fw - 1 - x), np.minimum(y, fh - 1 - y)) / (fh / 2.0)).astype(F32)   # 0 on the border
    mask = _t((disc * 255).astype(np.uint8) if mask_u8 else disc.astype(F32), cuda)
    wts = _t(np.round(feather * 255).astype(np.uint8) if wts_u8 else feather, cuda)
    gains = {"none": None, "unit": np.ones((n, 3), F32), "random": rng.uniform(0.5, 2.0, (n, 3)).astype(F32)}[gain_kind]
    d_gains = None if gains is None else _t(gains, cuda)
    whole = check_warp_tiles(nm, cuda, frames, mask, wts, recs, d_gains, cap, cw, ch, [4, 2])
    d_recs = _t(recs, cuda)
    if gain_kind == "unit":                                                 # x * 1.0f == x: the ungained tiles
        whole2 = torch.full((n + 2, cap, 4), SENTINEL, dtype=torch.float32, device=cuda)
        nm.mosaic_warp_tiles(frames, mask, wts, d_recs, gains=None, tile_cap=cap, tiles=whole2[1:n + 1])
        assert torch.equal(whole.view(torch.int32), whole2.view(torch.int32))


def edge_scene():
    """rectangles 63, 64, 65 wide and 3, 4, 5 high, a 5 x 3 one (under R = 32 the halo is larger than the tile), rectangles
    clipped by each canvas edge and corner, two larger frames under them so that seams cross everything"""
    rng = np.random.default_rng(77)
    cw, ch = 300, 120
    recs = [(10, 8, 131, 97, 1), (120, 15, 131, 97, 1)]
    xs = 5
    for nw in (63, 64, 65):
        for j, nh in enumerate((3, 4, 5)):
            recs.append((xs, 20 + 25 * j, nw, nh, 1))
        xs += 70
    recs += [(230, 60, 5, 3, 1), (-20, 30, 67, 45, 1), (cw - 30, 40, 67, 45, 1), (90, -25, 67, 45, 1), (150, ch - 12, 67, 45, 1),
             (-10, -10, 67, 45, 1), (cw - 40, ch - 20, 67, 45, 1), (260, 5, 129, 33, 1)]
    tiles = [B.texture(rng, r[2], r[3]) for r in recs]
    return tiles, recs, 131 * 97, cw, ch


def run_dev(nm, cuda, tiles, recs, cap, cw, ch, R, with_wts=True):
    canvas, cwts = B.pattern(cw, ch)
    d_canvas, d_cwts = _t(canvas, cuda), _t(cwts, cuda)
    nm.mosaic_bands(d_canvas, d_cwts if with_wts else None, _t(B.pack(tiles, cap, fill=np.nan), cuda), _t(B.records(recs), cuda),
                    R=R)
    return d_canvas.cpu().numpy(), d_cwts.cpu().numpy()


@pytest.mark.parametrize("R", (0, 1, 7, 32))
@pytest.mark.parametrize("n", (1, 3, 17, 64))
def test_device_equals_the_host_twin_bit_for_bit(nm, cuda, n, R):
    tiles, recs, cap, cw, ch = B.case(n)
    want_c, want_w = B.run_host(nm, tiles, recs, cap, cw, ch, R)
    got_c, got_w = run_dev(nm, cuda, tiles, recs, cap, cw, ch, R)
    assert np.array_equal(got_c, want_c) and np.array_equal(got_w.view(np.int32), want_w.view(np.int32))
    pat_c, _ = B.pattern(cw, ch)
    assert (got_c != pat_c).any() and (got_c == pat_c).all(axis=-1).any()      # written, and unlabelled pixels kept


@pytest.mark.parametrize("R", (0, 1, 7, 32))
def test_device_equals_the_host_twin_on_tile_and_canvas_edges(nm, cuda, R):
    tiles, recs, cap, cw, ch = edge_scene()
    want_c, want_w = B.run_host(nm, tiles, recs, cap, cw, ch, R)
    got_c, got_w = run_dev(nm, cuda, tiles, recs, cap, cw, ch, R)
    assert np.array_equal(got_c, want_c) and np.array_equal(got_w.view(np.int32), want_w.view(np.int32))
    label, covered = B.labels(tiles, recs, cw, ch, cap)
    pat_c, pat_w = B.pattern(cw, ch)
    off = label == B.NONE
    assert off.any() and (off & covered).any()
    assert np.array_equal(got_c[off], pat_c[off]) and np.array_equal(got_w[off], pat_w[off])
    no_w, _ = run_dev(nm, cuda, tiles, recs, cap, cw, ch, R, with_wts=False)
    assert np.array_equal(no_w, want_c)


def test_larger_frames_against_the_host_twin_and_the_model(nm, cuda):
    tiles, recs, cap = B.scene(5, 131, 97, 260, 200, seed=9, spread=70)
    R = 16
    want_c, want_w = B.run_host(nm, tiles, recs, cap, 260, 200, R)
    got_c, got_w = run_dev(nm, cuda, tiles, recs, cap, 260, 200, R)
    assert np.array_equal(got_c, want_c) and np.array_equal(got_w.view(np.int32), want_w.view(np.int32))
    md = B.model(tiles, recs, nm.mosaic_bands_taps(R, 8.0), 260, 200, cap)
    worst, bad, share = B.compare(got_c[..., :3], md, R)
    assert bad == 0 and worst <= 1 and share < 0.01


def test_a_frames_contribution_does_not_depend_on_the_slots_of_others(nm, cuda):
    rng = np.random.default_rng(21)
    cw, ch, cap, R = 400, 200, 67 * 45, 7
    group = [((10, 10, 67, 45, 1), B.texture(rng, 67, 45)), ((40, 25, 67, 45, 1), B.texture(rng, 67, 45)),
             ((25, 40, 67, 45, 1), B.texture(rng, 67, 45))]
    far = [((150 + 80 * (j % 3), 5 + 50 * (j // 3), 67, 45, 1), B.texture(rng, 67, 45)) for j in range(9)]
    region = (slice(0, 100), slice(0, 120))

    def run(slots, n):
        recs, tiles = [(0, 0, 0, 0, 0)] * n, [None] * n
        others = iter(far)
        for k in range(n):
            src = group[slots.index(k)] if k in slots else next(others, None)
            if src is not None:
                recs[k], tiles[k] = src
        return run_dev(nm, cuda, tiles, recs, cap, cw, ch, R)

    base_c, base_w = run([0, 1, 2], 3)
    for slots, n in (([0, 1, 2], 12), ([3, 7, 11], 12), ([5, 20, 63], 64), ([0, 62, 63], 64)):
        c, w = run(slots, n)
        assert np.array_equal(c[region], base_c[region]) and np.array_equal(w[region], base_w[region]), slots
    assert (base_c[region] != B.pattern(cw, ch)[0][region]).any()


def test_warp_tiles_and_bands_in_one_call_and_in_a_graph(nm, cuda):
    """mosaic_blend_bands (five launches) eagerly and captured in one HIP graph that is replayed on a second set of frames:
    bit-equal canvases."""
    import torch
    rng = np.random.default_rng(31)
    fw, fh, cw, ch = 67, 45, 140, 100
    recs = warp_records(fw, fh, cw, ch, fw + 6, fh + 6)
    recs[2, 9:14] = (30, 20, fw, fh, 1)
    recs[4, 9:11] = (60, 40)
    recs = recs[:5]
    n, cap, R = 5, (fw + 6) * (fh + 6), 7
    y, x = np.mgrid[0:fh, 0:fw]
    wts = _t(((1 + np.minimum(np.minimum(x, fw - 1 - x), np.minimum(y, fh - 1 - y))) / 32.0).astype(F32), cuda)
    mask = _t(np.full((fh, fw), 255, np.uint8), cuda)
    scenes = [[rng.integers(0, 256, (fh, fw, 4), dtype=np.uint8) for _ in range(n)] for _ in range(2)]
    gains = _t(rng.uniform(0.8, 1.25, (n, 3)).astype(F32), cuda)
    d_recs = _t(recs, cuda)
    frames = [_t(f, cuda) for f in scenes[0]]
    eager = []
    for sc in scenes:
        for f, src in zip(frames, sc):
            f.copy_(_t(src, cuda))
        canvas, cwts = (_t(a, cuda) for a in B.pattern(cw, ch))
        nm.mosaic_blend_bands(canvas, cwts, frames, mask, wts, d_recs, gains=gains, R=R, tile_cap=cap)
        eager.append((canvas.cpu().numpy(), cwts.cpu().numpy()))
    assert not np.array_equal(eager[0][0], eager[1][0])
    canvas, cwts = (_t(a, cuda) for a in B.pattern(cw, ch))
    tiles = torch.empty((n, cap, 4), dtype=torch.float32, device=cuda)
    stats = torch.empty(2, dtype=torch.int32, device=cuda)
    ws = nm.MosaicBandsWorkspace(n, cap, cw, ch, cuda)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            nm.mosaic_blend_bands(canvas, cwts, frames, mask, wts, d_recs, gains=gains, R=R, tile_cap=cap, tiles=tiles,
                                  stats=stats, workspace=ws)
    for sc, want in zip(scenes, eager):
        for f, src in zip(frames, sc):
            f.copy_(_t(src, cuda))
        pc, pw = B.pattern(cw, ch)
        canvas.copy_(_t(pc, cuda))
        cwts.copy_(_t(pw, cuda))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(canvas.cpu().numpy(), want[0]) and np.array_equal(cwts.cpu().numpy(), want[1])
    assert stats.cpu().tolist() == [5, 0]


def test_measure_solve_place_tiles_bands_on_the_loop_closure_views(nm, cuda):
    """The ten loop-closure views with per-view channel factors in [0.8, 1.25] and maps perturbed by B.E2E_PERTURB_PX at the
    corners: measure -> solve -> place -> warp tiles -> bands, eagerly and as ONE HIP graph replayed on a second scene, bit
    for bit. The eager canvas and weights equal nm_mosaic_bands_host on the device's own tiles and records. The mean squared Laplacian over the pixels with at least two valid frames, bands against feather against the
    winning frame alone (the last from the float64 model on the CPU): the device's bands mosaic is closer to the single frame
    than the device's feather mosaic is."""
    import ctypes as C
    import torch
    import loop_closure_ref as LC
    fig, sel, views0, (la, lb, Hs, chain), recs16, gains_host = B.e2e_model(nm, 91)
    assert abs(fig["bands"] - fig["single"]) < abs(fig["feather"] - fig["single"])        # the model shows the ordering
    K, L, cw, ch, cap = LC.K, len(la), LC.SCENE_W, LC.SCENE_H, B.E2E_CAP
    scenes = [views0, B.e2e_views(92)]
    frames = [_t(v, cuda) for v in scenes[0]]
    dH, dchain = _t(Hs, cuda), _t(chain, cuda)
    wts = _t(B.e2e_weights(), cuda)
    ones = torch.ones((LC.VH, LC.VW), dtype=torch.float32, device=cuda)
    canvas = torch.zeros((ch, cw, 4), dtype=torch.uint8, device=cuda)
    cwts = torch.zeros((ch, cw), dtype=torch.float32, device=cuda)
    sums = torch.empty((L, 7), dtype=torch.int64, device=cuda)
    gains = torch.empty((K, 3), dtype=torch.float32, device=cuda)
    estats = torch.empty(9, dtype=torch.float64, device=cuda)
    records = torch.empty((K, 16), dtype=torch.int32, device=cuda)
    extent = torch.empty(4, dtype=torch.float32, device=cuda)
    tiles = torch.empty((K, cap, 4), dtype=torch.float32, device=cuda)
    tstats = torch.empty(2, dtype=torch.int32, device=cuda)
    ws = nm.MosaicBandsWorkspace(K, cap, cw, ch, cuda)

    def enqueue():                                           # no host read, no allocation: every output is given
        canvas.zero_()
        cwts.zero_()
        nm.mosaic_exposure(frames, la, lb, dH, sums=sums, gains=gains, stats=estats, **B.E2E_EXPOSURE)
        status = nm.lib().nm_mosaic_place_f32(K, dchain.data_ptr(), None, LC.VW, LC.VH, cw, ch, LC.ORIGIN_X, LC.ORIGIN_Y,
                                              records.data_ptr(), extent.data_ptr(),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert status == 0
        nm.mosaic_blend_bands(canvas, cwts, frames, ones, wts, records, gains=gains, R=B.E2E_R, sigma=B.E2E_SIGMA, tile_cap=cap,
                              tiles=tiles, stats=tstats, workspace=ws)

    def host():
        return [t.cpu().numpy().copy() for t in (sums, gains, records, tstats, canvas, cwts)]

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        enqueue()
    s.synchronize()
    eager = host()
    assert np.array_equal(eager[2], recs16) and np.array_equal(eager[1].view(np.uint32), gains_host.view(np.uint32))
    assert eager[3].tolist() == [K, 0]
    # the device's own tiles and records through the host twin: the same canvas and weights, bit for bit
    twin_c, twin_w = np.zeros((ch, cw, 4), np.uint8), np.zeros((ch, cw), F32)
    nm.mosaic_bands_host(twin_c, twin_w, tiles.cpu().numpy(), eager[2], R=B.E2E_R, sigma=B.E2E_SIGMA)
    assert np.array_equal(eager[4], twin_c) and np.array_equal(eager[5].view(np.int32), twin_w.view(np.int32))
    assert twin_c.any() and twin_w.any()
    # sharpness: bands and feather from the device, the winning frame alone from the model
    fcanvas, fwts = torch.zeros_like(canvas), torch.zeros_like(cwts)
    nm.transform_blend_batch_gain(fcanvas, fwts, frames, ones, wts, records, gains=gains)
    dev_bands = B.laplacian_ms(eager[4][..., :3] / B.SCALE, sel)
    dev_feather = B.laplacian_ms(fcanvas.cpu().numpy()[..., :3] / B.SCALE, sel)
    print("mean squared Laplacian over %d pixels (byte levels^2), perturbation %.1f px: device bands %.3f, device feather %.3f; "
          "model bands %.3f, model feather %.3f, winning frame alone %.3f"
          % (sel.sum(), B.E2E_PERTURB_PX, dev_bands, dev_feather, fig["bands"], fig["feather"], fig["single"]))
    assert abs(dev_bands - fig["single"]) < abs(dev_feather - fig["single"])
    # one graph, replayed on the second scene
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        enqueue()
    for f, v in zip(frames, scenes[1]):
        f.copy_(_t(v, cuda))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    replayed = host()
    with torch.cuda.stream(s):
        enqueue()
    s.synchronize()
    for a, b in zip(replayed, host()):
        assert np.array_equal(a, b)
    assert not np.array_equal(replayed[4], eager[4]) and np.array_equal(replayed[2], eager[2])
