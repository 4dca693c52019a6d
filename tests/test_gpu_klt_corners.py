"""The corner detector on the device (nm_klt_corners_batch_dev_f32) against its host twin, bit for bit, on the cases of
tests/klt_corners_ref.py (which tests/test_klt_corners_host.py holds against the Python model), and on what only the
device has: the response tile's seams (64 x 16 pixels), grid caps 1 and 3, planes aligned to 16 and to 4 bytes (a pyramid block
among them), a cap that cuts inside a tile, garbage in the outputs and the workspace, 64-slot tables with unused entries,
and pyramid -> corners -> select -> track -> RANSAC -> refit as one HIP graph replayed on new frames."""
import ctypes as C

import numpy as np
import pytest

import klt_corners_ref as R
import klt_ref as K

pytestmark = pytest.mark.gpu

F32 = np.float32
CASES = R.cases()
TX, TY = 64, 16                                                       # the response tile


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def shifted(a, dev, offset):
    """a on the device, `offset` elements into its allocation"""
    import torch
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + offset, dtype=_t(a[:0], "cpu").dtype, device=dev)
    view = buf[offset:offset + a.size].view(a.shape)
    view.copy_(_t(a, dev))
    return view


def same(got, want, what=""):
    """a device result dict against the host twin's, bit for bit up to each frame's count"""
    cnt, tot = got["count"].cpu().numpy(), got["total"].cpu().numpy()
    assert np.array_equal(cnt, want["count"]) and np.array_equal(tot, want["total"]), (what, cnt, want["count"], tot, want["total"])
    for k, n in enumerate(cnt):
        for key in ("x", "y", "score"):
            g = got[key][k][:n].cpu().numpy()
            assert np.array_equal(g.view(np.uint32), want[key][k][:n].view(np.uint32)), (what, k, key)
        if got["score_plane"] is not None:
            assert np.array_equal(got["score_plane"][k].cpu().numpy().view(np.uint32), want["score_plane"][k].view(np.uint32)), (what, k)


def host_and_device(nm, cuda, c, offset=0, want_plane=True, out=None, workspace=None):
    held_h = held_d = None
    if c["held"] is not None:
        held_h = ([h[0] for h in c["held"]], [h[1] for h in c["held"]], [h[2] for h in c["held"]])
        held_d = ([_t(h[0], cuda) for h in c["held"]], [_t(h[1], cuda) for h in c["held"]],
                  [_t(np.array([h[2]], np.int32), cuda) for h in c["held"]])
    kw = dict(radius=c["r"], nms=c["nms"], min_eig=c["min_eig"], cap=c["cap"], want_score_plane=want_plane)
    want = nm.klt_corners_host(c["grays"], mask=c["mask"], held=held_h, **kw)
    uniq = {id(g): shifted(g, cuda, offset) for g in c["grays"]}      # repeated frames repeat their pointer
    mask = None if c["mask"] is None else shifted(c["mask"], cuda, offset)
    got = nm.klt_corners_batch([uniq[id(g)] for g in c["grays"]], mask=mask, held=held_d, out=out, workspace=workspace, **kw)
    return got, want


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_device_equals_the_host_twin(nm, cuda, c):
    got, want = host_and_device(nm, cuda, c)
    same(got, want, c["name"])


@pytest.mark.parametrize("w", [TX - 1, TX, TX + 1, 2 * TX + 1])
@pytest.mark.parametrize("h", [3 * TY - 1, 3 * TY, 3 * TY + 1])
def test_tile_seams(nm, cuda, w, h):
    g = R.noise(w * 7 + h, w, h)
    hx, hy = np.array([w - 1, 10, w + 9, 3], F32), np.array([h - 1, h + 11, 20, -9], F32)
    for r, nms in ((7, 8), (3, 16), (1, 1)):
        c = R._case("seam", [g, g[::-1].copy()], r=r, nms=nms, cap=4096, held=[(hx, hy, 4), (hx, hy, 2)])
        got, want = host_and_device(nm, cuda, c)
        same(got, want, (w, h, r, nms))
        assert want["total"].sum() > 0


@pytest.mark.parametrize("offset,cap", [(4, 0), (1, 0), (0, 1), (4, 3), (3, 3)])
def test_alignment_and_grid_caps(nm, cuda, offset, cap):
    """planes 16 bytes aligned (offset 4 floats) take the 16-byte loads where the width is a multiple of 4 (64, 130 is not),
    planes 4 bytes aligned the scalar ones, the mask alike; with the cap at 1 or 3 workgroups every launch walks its units"""
    prev = nm.klt_corners_set_grid_cap(cap)
    try:
        for name in ("noise64x64_r7_nms8", "noise130x70_r3_nms16", "mask_holes", "three_frames", "held_nH20", "checker2_r7"):
            c = next(c for c in CASES if c["name"] == name)
            got, want = host_and_device(nm, cuda, c, offset)
            same(got, want, name)
        g, m = R.noise(9, 128, 40), R.holes(128, 40)
        c = R._case("wide_mask", [g], r=3, nms=4, mask=m, cap=4096)
        same(*host_and_device(nm, cuda, c, offset), "wide_mask")
    finally:
        nm.klt_corners_set_grid_cap(prev)


def test_a_pyramid_block_as_the_gray_plane(nm, cuda):
    fw, fh = 132, 50
    g = R.noise(12, fw, fh)
    mask = np.ones((fh, fw), F32)
    mask[20:24, 30:41] = 0
    pyrs, mp = nm.gray_pyramid_batch([_t(g, cuda)], levels=3, mask=_t(mask, cuda))
    got = nm.klt_corners_batch([nm.gray_pyramid_level(pyrs[0], fw, fh, 0)], radius=3, nms=4, min_eig=0.25, want_score_plane=True,
                               mask=nm.gray_pyramid_level(mp, fw, fh, 0))
    want = nm.klt_corners_host([g], radius=3, nms=4, min_eig=0.25, want_score_plane=True, mask=(mask > 0.5).astype(np.uint8))
    same(got, want)
    assert want["count"][0] > 4


def cut_inside_a_row(xs, ys):
    """a cap that keeps the first corners of a pixel row whose corners lie in more than one tile, and cuts its last"""
    for y in np.unique(ys):
        idx = np.nonzero(ys == y)[0]
        if len(set((xs[idx] // TX).tolist())) >= 2 and idx[-1] >= 1:
            return int(idx[-1])
    raise AssertionError("no pixel row with corners in two tiles")


def test_cap_cuts_inside_a_tile_and_garbage_is_overwritten(nm, cuda):
    """corners spread over several tiles of a 200 x 50 frame, the cap in the middle of a tile row; outputs longer than cap and
    the workspace filled with garbage before the call; a second call into the same tensors gives the same"""
    import torch
    g = R.noise(21, 200, 50)
    full = nm.klt_corners_host([g], radius=3, nms=2, min_eig=0.25, cap=4096)
    total = int(full["total"][0])
    cap = cut_inside_a_row(full["x"][0][:total], full["y"][0][:total])
    c = R._case("cut", [g, g[:, ::-1].copy()], r=3, nms=2, cap=cap)
    ws = nm.KltCornersWorkspace(2, 200, 50, cuda)
    ws.buf.fill_(0xA5)
    junk = lambda v: [torch.full((cap + 5,), v, dtype=torch.float32, device=cuda) for _ in range(2)]
    out = dict(x=junk(123.0), y=junk(float("nan")), score=junk(-5.0), count=torch.full((2,), 77, dtype=torch.int32, device=cuda),
               total=torch.full((2,), -9, dtype=torch.int32, device=cuda),
               score_plane=[torch.full((50, 200), float("nan"), dtype=torch.float32, device=cuda) for _ in range(2)])
    for _ in range(2):
        got, want = host_and_device(nm, cuda, c, out=out, workspace=ws)
        assert got is out
        same(got, want)
        assert int(want["count"][0]) == cap < total == int(want["total"][0])
        assert all((t[cap:].cpu().numpy() == v).all() for ts, v in ((got["x"], 123.0), (got["score"], -5.0)) for t in ts)
        ws.buf.fill_(0x3C)


@pytest.mark.parametrize("n", [1, 3])
def test_tables_of_64_slots_with_unused_trailing_entries(nm, cuda, n):
    """the C entry with 64-slot HOST tables whose entries beyond n hold a garbage address (or NULL, on the second round), in the
    optional tables too: they are never used"""
    import torch
    fw, fh, cap = 97, 61, 64
    L = nm.lib()
    grays = [R.noise(1, 97, 61), R.noise(7, 97, 61), R.checker(97, 61, 3)][:n]
    hx, hy = np.array([40, 41.5, 96], F32), np.array([30, 12.5, 60], F32)
    want = nm.klt_corners_host(grays, radius=3, nms=8, min_eig=0.25, cap=cap, held=([hx] * n, [hy] * n, [3, 1, 0][:n]),
                               want_score_plane=True)
    d_gray = [_t(g, cuda) for g in grays]
    d_hx, d_hy = _t(hx, cuda), _t(hy, cuda)
    d_n = [_t(np.array([v], np.int32), cuda) for v in [3, 1, 0][:n]]
    ws = torch.empty(nm.klt_corners_workspace_bytes(n, fw, fh), dtype=torch.uint8, device=cuda)
    for fill in (0xDEAD0000BEE0, None):
        table = lambda ts: (C.c_void_p * 64)(*([t.data_ptr() for t in ts] + [fill] * (64 - len(ts))))
        new = lambda: [torch.full((cap,), 99.0, dtype=torch.float32, device=cuda) for _ in range(n)]
        out = dict(x=new(), y=new(), score=new(), count=torch.full((n,), 5, dtype=torch.int32, device=cuda),
                   total=torch.full((n,), 5, dtype=torch.int32, device=cuda),
                   score_plane=[torch.empty((fh, fw), dtype=torch.float32, device=cuda) for _ in range(n)])
        assert L.nm_klt_corners_batch_dev_f32(n, table(d_gray), fw, fh, None, table([d_hx] * n), table([d_hy] * n), table(d_n), 3,
                                              3, 8, 0.25, cap, table(out["x"]), table(out["y"]), table(out["score"]),
                                              out["count"].data_ptr(), out["total"].data_ptr(), table(out["score_plane"]),
                                              ws.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        same(out, want)


# ---- one graph ----------------------------------------------------------------------------------------------------------------
def graph_frames(seed, n=3, fw=160, fh=120):
    """n + 1 views of a texture on a pan of (5, 2) px per frame"""
    g = R.noise(seed, fw + 5 * n + 4, fh + 2 * n + 4)
    return [np.ascontiguousarray(g[2 * k:2 * k + fh, 5 * k:5 * k + fw]) for k in range(n + 1)]


def test_pyramid_corners_select_track_ransac_and_refit_in_one_graph(nm, cuda):
    """the device chain, eager and as one captured graph replayed on two sets of frames, against the host twins of the
    pyramid, the corners, the selection and the tracker (equal bits); RANSAC and refit against their eager device run"""
    import torch
    n, fw, fh, levels, cap, keep = 3, 160, 120, 3, 1024, 48
    grays = [torch.empty((fh, fw), dtype=torch.float32, device=cuda) for _ in range(n + 1)]
    ckw = dict(radius=5, nms=4, min_eig=0.5, cap=cap)
    tkw = dict(levels=levels, radius=5, iterations=8, fb_max=1.0, min_eig=0.5)
    ws = nm.KltCornersWorkspace(n, fw, fh, cuda)
    sws = nm.SelectWorkspace(n, cap, 8, 6, cuda)
    keepers = {}

    def chain():
        pyr, _ = nm.gray_pyramid_batch(grays, levels=levels, pyrs=keepers.get("pyr"))
        c = nm.klt_corners_batch([nm.gray_pyramid_level(p, fw, fh, 0) for p in pyr[:n]], out=keepers.get("c"), workspace=ws, **ckw)
        d_cnt = [c["count"][k:k + 1] for k in range(n)]
        s = nm.sift_select_batch_dev(d_cnt, c["x"], c["y"], fw, fh, scores=c["score"], gx=8, gy=6, keep=keep, capacity=cap,
                                     out=keepers.get("s"), workspace=sws)
        d_n = [s["count"][k:k + 1] for k in range(n)]
        tr = nm.klt_track_batch_dev(pyr[:-1], pyr[1:], fw, fh, s["x"], s["y"], d_n, capA=keep, out=keepers.get("tr"), **tkw)
        tabs = (s["x"], s["y"], d_n, tr.dst_xs, tr.dst_ys, tr.matches)
        H, best, _, status = nm.ransac_batch_dev(0, *tabs, iterations=64, threshold=1.0, capA=keep)
        H2, count, st2, _ = nm.ransac_refit_batch_dev(0, *tabs, H, status, rounds=2, threshold=1.0, capA=keep)
        keepers.update(pyr=pyr, c=c, s=s, tr=tr)
        return c, s, tr, H2, count, st2

    def outputs(r):
        c, s, tr, H2, count, st2 = r
        m = s["count"].cpu().numpy()
        rows = [torch.stack(v).cpu().numpy()[:, :keep] for v in (s["x"], s["y"], tr.dst_xs, tr.dst_ys, tr.matches)]
        for a in rows[:2]:                                              # rows at and beyond a count are not written
            for k in range(n):
                a[k, m[k]:] = 0
        return rows + [v.cpu().numpy() for v in (c["count"], c["total"], s["count"], tr.count, H2, count, st2)]

    def host_chain(views):
        pyr, _ = nm.gray_pyramid_host(views, levels=levels)
        c = nm.klt_corners_host(views[:n], **ckw)
        s = nm.sift_select_host(list(c["count"]), list(c["x"]), list(c["y"]), fw, fh, scores=list(c["score"]), gx=8, gy=6, keep=keep,
                                capacity=cap)
        m = [int(v) for v in s["count"]]
        tr = nm.klt_track_host(pyr[:-1], pyr[1:], fw, fh, list(s["x"]), list(s["y"]), m, capA=keep, **tkw)
        return c, s, tr

    eager = []
    for seed in (11, 12):
        views = graph_frames(seed, n, fw, fh)
        for g, v in zip(grays, views):
            g.copy_(_t(v, cuda))
        got = outputs(chain())
        c, s, tr = host_chain(views)
        assert np.array_equal(got[5], c["count"]) and np.array_equal(got[6], c["total"]) and np.array_equal(got[7], s["count"])
        assert (s["count"] == keep).all() and (tr.count > keep // 2).all()
        for a, b in zip(got[:5], (s["x"][:, :keep], s["y"][:, :keep], tr.dst_xs, tr.dst_ys, tr.matches)):
            assert np.array_equal(a.view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
        assert np.array_equal(got[8].astype(np.uint64), tr.count) and (got[11] == 1).all()
        for Hk in got[9].astype(np.float64).reshape(n, 3, 3):           # the refitted maps are the pan
            q = Hk @ np.array([80.0, 60.0, 1.0])
            assert np.abs(q[:2] / q[2] - [75.0, 58.0]).max() < 0.1
        eager.append(got)
    assert not np.array_equal(eager[0][0], eager[1][0])
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            r = chain()
    for seed, want in ((11, eager[0]), (12, eager[1])):
        for g, v in zip(grays, graph_frames(seed, n, fw, fh)):
            g.copy_(_t(v, cuda))
        r[0]["count"].fill_(0x7777)
        r[2].count.fill_(0x7777777777)
        for t in r[2].matches + r[0]["x"]:
            t.fill_(9)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(outputs(r), want):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
