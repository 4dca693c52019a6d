"""Mosaic plan and batched blend on the GPU: transform_blend_batch against n per-frame transform_blend calls and the
oracle (bit for bit), the device plan against its host twin (bit for bit), the planned rectangle against a frame's actual
contribution, detect -> match -> RANSAC -> plan -> blend end to end on a synthetic scene, and that chain captured into one
HIP graph."""
import numpy as np
import pytest

import helpers as H
from test_mosaic_host import links_f32, make_links, rec_fields

pytestmark = pytest.mark.gpu

TEX_U8N, TEX_F32 = 0, 2


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _plane(rng, fw, fh, fmt, kind):
    if kind == "mask":
        p = (rng.uniform(0, 1, (fh, fw)) > 0.15)
        return p.astype(np.float32) if fmt == TEX_F32 else (p * rng.integers(100, 256, (fh, fw))).astype(np.uint8)
    yy, xx = np.mgrid[0:fh, 0:fw]
    w = np.minimum(np.minimum(xx, fw - 1 - xx), np.minimum(yy, fh - 1 - yy)) / 16.0 + rng.uniform(0, 0.05, (fh, fw))
    return w.astype(np.float32) if fmt == TEX_F32 else np.clip(w * 40, 0, 255).astype(np.uint8)


def _records(rng, n, cw, ch, fw, fh):
    """Random placements: overlapping, partly or wholly off the canvas, nw = 0, negative tx / ty; maps near similarity
    with mild perspective from the local grid into the frame."""
    rec = np.zeros((n, 16), np.int32)
    for k in range(n):
        deg, s = rng.uniform(-20, 20), rng.uniform(0.7, 1.3)
        c, sn = s * np.cos(np.radians(deg)), s * np.sin(np.radians(deg))
        m = np.array([[c, -sn, rng.uniform(-25, 15)], [sn, c, rng.uniform(-25, 15)],
                      [rng.uniform(-6e-4, 6e-4), rng.uniform(-6e-4, 6e-4), 1.0]], np.float32)
        tx, ty = int(rng.integers(-80, cw)), int(rng.integers(-60, ch))
        nw, nh = int(rng.integers(1, 2 * fw)), int(rng.integers(1, 2 * fh))
        rec[k, :9] = m.reshape(9).view(np.int32)
        rec[k, 9:14] = (tx, ty, nw, nh, 1)
    specials = [(0, 10, 0, 50), (cw + 5, 3, 40, 40), (-30, -20, 70, 60), (-200, -100, cw + 400, ch + 300),
                (10, ch - 2, 60, 80), (cw - 3, 0, 0, 0)]
    for j, (tx, ty, nw, nh) in enumerate(specials[:max(0, n - 1)]):
        rec[1 + j, 9:13] = (tx, ty, nw, nh)
    return rec


def _per_frame(nm, oracle, dev, canvas0, cwts0, frames, masks, wts, rec):
    """n per-frame nm.transform_blend calls on the GPU and the oracle's in-order transform_blend."""
    import torch
    c, w = _t(canvas0, dev), _t(cwts0, dev)
    rec_d = _t(rec, dev)
    oc, ow = canvas0.copy(), cwts0.copy()
    for k in range(len(frames)):
        m, tx, ty, nw, nh = rec_d[k, :9].view(torch.float32), *[int(v) for v in rec[k, 9:13]]
        nm.transform_blend(c, w, _t(frames[k], dev), nw, nh, m, tx, ty, _t(masks[k], dev), _t(wts[k], dev))
        oc, ow = oracle.transform_blend(oc, ow, frames[k], nw, nh, rec[k, :9].view(np.float32), tx, ty, masks[k], wts[k])
    torch.cuda.synchronize()
    return c.cpu().numpy(), w.cpu().numpy(), oc, ow


CASES = [  # (n, mask format, weight format, one shared mask / weight plane, canvas size)
    (1, TEX_U8N, TEX_F32, True, (333, 217)),
    (3, TEX_F32, TEX_F32, False, (200, 150)),
    (17, TEX_U8N, TEX_U8N, False, (333, 217)),
    (64, TEX_F32, TEX_U8N, True, (401, 263)),
    (64, TEX_U8N, TEX_F32, False, (129, 97)),
]


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: "n%d-m%d-w%d-%s-%dx%d" % (
    CASES[i][0], CASES[i][1], CASES[i][2], "shared" if CASES[i][3] else "distinct", *CASES[i][4]))
def test_batch_blend_equals_per_frame_blends_and_oracle(nm, oracle, cuda, case):
    import torch
    n, mfmt, wfmt, shared, (cw, ch) = CASES[case]
    rng = np.random.default_rng(700 + case)
    fw, fh = 96, 72
    frames = [rng.integers(0, 256, (fh, fw, 4), dtype=np.uint8) for _ in range(n)]
    if shared:
        masks, wts = [_plane(rng, fw, fh, mfmt, "mask")] * n, [_plane(rng, fw, fh, wfmt, "wts")] * n
    else:
        masks = [_plane(rng, fw, fh, mfmt, "mask") for _ in range(n)]
        wts = [_plane(rng, fw, fh, wfmt, "wts") for _ in range(n)]
    # patterned canvas, partly filled: weights 0 on the left part, non-zero elsewhere
    canvas0 = rng.integers(0, 256, (ch, cw, 4), dtype=np.uint8)
    cwts0 = np.where(np.arange(cw)[None, :] < cw // 3, 0.0, rng.uniform(0.1, 2.0, (ch, cw))).astype(np.float32)
    rec = _records(rng, n, cw, ch, fw, fh)
    got_c, got_w, oc, ow = _per_frame(nm, oracle, cuda, canvas0, cwts0, frames, masks, wts, rec)
    assert np.array_equal(got_c, oc) and np.array_equal(_u32(got_w), _u32(ow))
    c, w = _t(canvas0, cuda), _t(cwts0, cuda)
    fr = [_t(f, cuda) for f in frames]
    if shared:
        md, wd = _t(masks[0], cuda), _t(wts[0], cuda)
    else:
        md, wd = [_t(p, cuda) for p in masks], [_t(p, cuda) for p in wts]
    nm.transform_blend_batch(c, w, fr, md, wd, _t(rec, cuda))
    torch.cuda.synchronize()
    bc, bw = c.cpu().numpy(), w.cpu().numpy()
    assert np.array_equal(_u32(bw), _u32(got_w)), "weights differ at %d pixels" % (_u32(bw) != _u32(got_w)).sum()
    assert np.array_equal(bc, got_c), "canvas differs at %d pixels" % (bc != got_c).any(-1).sum()
    # outside every rectangle nothing moved, and the frames did change the canvas
    cover = np.zeros((ch, cw), bool)
    for k in range(n):
        tx, ty, nw, nh = (int(v) for v in rec[k, 9:13])
        if nw > 0 and nh > 0:
            cover[max(ty, 0):max(min(ty + nh, ch), 0), max(tx, 0):max(min(tx + nw, cw), 0)] = True
    assert np.array_equal(bc[~cover], canvas0[~cover]) and np.array_equal(_u32(bw[~cover]), _u32(cwts0[~cover]))
    assert (bw != cwts0).sum() > 50


def test_batch_blend_any_record_values_stay_in_bounds(nm, cuda):
    """Records from outside: values whose rectangles clip to nothing (or overflow 32-bit sums) leave the canvas alone;
    a normal record among them is applied as a per-frame call would."""
    import torch
    rng = np.random.default_rng(5)
    cw, ch, fw, fh = 150, 90, 40, 30
    I32 = np.iinfo(np.int32)
    frame = rng.integers(0, 256, (fh, fw, 4), dtype=np.uint8)
    mask, wts = np.ones((fh, fw), np.float32), np.ones((fh, fw), np.float32)
    canvas0 = rng.integers(0, 256, (ch, cw, 4), dtype=np.uint8)
    cwts0 = np.zeros((ch, cw), np.float32)
    eye = np.eye(3, dtype=np.float32).reshape(9).view(np.int32)
    bad = [(I32.max - 5, 0, 100, 10), (I32.min, 0, I32.max, 10), (0, I32.max, 10, I32.max), (0, 0, -5, 10),
           (0, 0, 10, I32.min), (I32.min, I32.min, I32.max, I32.max), (cw, 0, 10, 10), (0, ch, 10, 10)]
    rec = np.zeros((len(bad) + 1, 16), np.int32)
    for k, f in enumerate(bad):
        rec[k, :9] = eye
        rec[k, 9:13] = f
    rec[-1, :9] = eye
    rec[-1, 9:13] = (20, 10, fw, fh)
    c, w = _t(canvas0, cuda), _t(cwts0, cuda)
    fd = _t(frame, cuda)
    nm.transform_blend_batch(c, w, [fd] * len(rec), _t(mask, cuda), _t(wts, cuda), _t(rec, cuda))
    c2, w2 = _t(canvas0, cuda), _t(cwts0, cuda)
    nm.transform_blend(c2, w2, fd, fw, fh, _t(np.eye(3, dtype=np.float32), cuda), 20, 10, _t(mask, cuda), _t(wts, cuda))
    torch.cuda.synchronize()
    assert torch.equal(c, c2) and torch.equal(w.view(torch.int32), w2.view(torch.int32))
    assert (w.cpu().numpy() > 0).sum() > 0.5 * fw * fh


PLAN_GEOS = [(640, 480, 9000, 3000, 4000, 1200), (640, 480, 1500, 900, 700, 300), (320, 240, 32767, 32767, -900, 16000)]


def _plan_cases():
    cases = []
    for kind, n, seed in (("translation", 1, 1), ("similarity", 2, 2), ("perspective", 17, 3), ("perspective", 64, 4),
                          ("similarity", 64, 5)):
        cases.append((kind, links_f32(make_links(kind, n, seed)), None, None))
    base = links_f32(make_links("similarity", 10, 6))
    st = np.ones(9, np.int32)
    st[4] = 0
    cases.append(("status0", base, st, None))
    nan = base.copy()
    nan[2, 1] = np.nan
    cases.append(("nan", nan, None, None))
    z = base.copy()
    z[6, 6:] = 0
    cases.append(("p8zero", z, np.ones(9, np.int32), None))
    P = np.array([[1, 0, 0], [0, 1, 0], [0.01, 0, 1]], np.float64)
    lk = make_links("translation", 6, 7)
    lk[1], lk[2] = P, np.linalg.inv(P)
    cases.append(("behind", links_f32(lk), None, None))
    Mf = np.array([[0.99, 0.02, -35.5], [-0.02, 1.01, 12.25], [1e-6, -2e-6, 1.0]], np.float32)
    cases.append(("M_first", links_f32(make_links("perspective", 12, 8)), None, Mf))
    return cases


def test_device_plan_equals_host_twin(nm, cuda):
    import torch
    for name, Hs, st, Mf in _plan_cases():
        for geo in PLAN_GEOS:
            want = nm.mosaic_plan_host(Hs, st, *geo, M_first=Mf)
            got = nm.mosaic_plan(_t(Hs, cuda), _t(st, cuda) if st is not None else None, *geo,
                                 M_first=_t(Mf, cuda) if Mf is not None else None)
            torch.cuda.synchronize()
            got = [g.cpu().numpy() for g in got]
            assert np.array_equal(got[0], want[0]), (name, geo)
            assert np.array_equal(_u32(got[1]), _u32(want[1])), (name, geo)
            assert np.array_equal(_u32(got[2]), _u32(want[2])), (name, geo)
    # the records are a valid mat3x3 for transform_blend and the break cases did break
    r, c, e = nm.mosaic_plan_host(_plan_cases()[5][1], _plan_cases()[5][2], *PLAN_GEOS[0])
    assert rec_fields(r)[5].tolist() == [1] * 5 + [0] * 5


def test_planned_rectangle_covers_the_contribution(nm, cuda):
    """A full-canvas transform_blend of frame k with the map M_k T(-ox, -oy) changes no pixel outside records[k]."""
    import torch
    fw, fh, cw, ch, ox, oy = 320, 240, 900, 640, 260, 180
    rng = np.random.default_rng(3)
    links = make_links("perspective", 6, 11)
    links[2] = links[2] @ np.array([[np.cos(0.4), -np.sin(0.4), 60], [np.sin(0.4), np.cos(0.4), -30], [2e-4, -1e-4, 1]])
    Hs = links_f32(links)
    records, chain, _ = nm.mosaic_plan(_t(Hs, cuda), None, fw, fh, cw, ch, ox, oy)
    torch.cuda.synchronize()
    records, chain = records.cpu().numpy(), chain.cpu().numpy()
    m, tx, ty, nw, nh, placed, _ = rec_fields(records)
    frame = _t(rng.integers(0, 256, (fh, fw, 4), dtype=np.uint8), cuda)
    ones = _t(np.ones((fh, fw), np.float32), cuda)
    checked = 0
    for k in range(6):
        assert placed[k] == 1
        M = chain[k].reshape(3, 3).astype(np.float64)
        full = (M @ np.array([[1, 0, -ox], [0, 1, -oy], [0, 0, 1]], np.float64)).astype(np.float32)
        c = torch.zeros((ch, cw, 4), dtype=torch.uint8, device=cuda)
        w = torch.zeros((ch, cw), dtype=torch.float32, device=cuda)
        nm.transform_blend(c, w, frame, cw, ch, _t(full, cuda), 0, 0, ones, ones)
        torch.cuda.synchronize()
        hit = w.cpu().numpy() != 0
        inside = np.zeros_like(hit)
        inside[ty[k]:ty[k] + nh[k], tx[k]:tx[k] + nw[k]] = True
        assert not (hit & ~inside).any(), (k, np.argwhere(hit & ~inside)[:5])
        checked += int(hit.sum())
        # and the rectangle is tight: the frame reaches within 4 px of every clipped edge that is not the canvas border
        ys, xs = np.nonzero(hit)
        for edge, got, limit in ((tx[k], xs.min(), 0), (ty[k], ys.min(), 0)):
            if edge > limit:
                assert got - edge <= 4, (k, edge, got)
    assert checked > 6 * 0.5 * fw * fh


# ---- end to end: 8 views of one scene ----

VW, VH, CAP = 640, 480, 8192


def _view_maps():
    """A_k: view-k pixel -> scene pixel (a panning, slightly rolling camera). A_0 is a translation, so the mosaic's
    frame-0 coordinates are scene - (ox, oy)."""
    maps = []
    for k in range(8):
        deg = 0.0 if k == 0 else 1.5 * np.sin(k)
        c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
        A = np.array([[c, -s, 40 + 70 * k], [s, c, 50 + 14 * (-1) ** k], [0, 0, 1]], np.float64)
        maps.append(A)
    return maps


SCENE_W, SCENE_H = 1240, 600


def _scene(seed):
    g = np.clip(H.blurred_frame(seed, SCENE_W, SCENE_H, sigma=2.0) * 1.4, 0, 255).astype(np.uint8)
    return np.stack([g, np.roll(g, 3, 1), np.roll(g, 5, 0), np.full_like(g, 255)], -1)


def _views(nm, dev, scene):
    import torch
    out = []
    for A in _view_maps():
        v, _, _ = nm.resample_perspective(_t(scene, dev), VW, VH, _t(np.linalg.inv(A).astype(np.float32), dev), inverse=True)
        out.append(v)
    torch.cuda.synchronize()
    return out


def _feather():
    yy, xx = np.mgrid[0:VH, 0:VW]
    return (np.minimum(np.minimum(xx, VW - 1 - xx), np.minimum(yy, VH - 1 - yy)) / 64.0 + 0.01).astype(np.float32)


class _Chain:
    """detect -> match (7 pairs k -> k+1) -> RANSAC -> plan -> blend, all on the current stream with own workspaces."""

    def __init__(self, nm, dev, iterations=2048):
        import torch
        self.nm, self.dev, self.iterations = nm, dev, iterations
        self.arenas = [nm.SiftArena(VW, VH, CAP) for _ in range(8)]
        self.res = [torch.full((CAP,), -1, dtype=torch.int32, device=dev) for _ in range(7)]
        self.mws = nm.MatchBatchDevWorkspace(7, CAP, CAP, dev)
        self.rws = nm.RansacBatchWorkspace(7, CAP, iterations, dev)
        self.mask = torch.full((VH, VW), 255, dtype=torch.uint8, device=dev)
        self.wts = _t(_feather(), dev)
        self.canvas = torch.zeros((SCENE_H, SCENE_W, 4), dtype=torch.uint8, device=dev)
        self.cwts = torch.zeros((SCENE_H, SCENE_W), dtype=torch.float32, device=dev)
        A0 = _view_maps()[0]
        self.ox, self.oy = int(A0[0, 2]), int(A0[1, 2])

    def enqueue(self, views):
        nm = self.nm
        A, B = self.arenas[:-1], self.arenas[1:]
        nm.detect_describe_batch(self.arenas, [nm.grayscale(v) for v in views])
        nm.sift_match_batch_dev([a.desc for a in A], [a.num_items for a in A], [b.desc for b in B],
                                [b.num_items for b in B], self.res, 0.8, workspace=self.mws)
        Hb, best, pos, status = nm.ransac_batch_dev(2, [a.x for a in A], [a.y for a in A], [a.num_items for a in A],
                                                    [b.x for b in B], [b.y for b in B], self.res,
                                                    iterations=self.iterations, threshold=1.0, seeds=list(range(7)),
                                                    capA=CAP, workspace=self.rws)
        records, chain, extent = nm.mosaic_plan(Hb, status, VW, VH, SCENE_W, SCENE_H, self.ox, self.oy)
        self.canvas.zero_()
        self.cwts.zero_()
        nm.transform_blend_batch(self.canvas, self.cwts, views, self.mask, self.wts, records)
        return Hb, status, records, chain, extent, self.canvas, self.cwts

    def close(self):
        for a in self.arenas:
            a.close()


def test_end_to_end_detect_match_ransac_plan_blend(nm, oracle, cuda):
    import torch
    scene = _scene(90)
    views = _views(nm, cuda, scene)
    ch = _Chain(nm, cuda, iterations=4096)
    Hb, status, records, chain, extent, canvas, cwts = [o.cpu().numpy().copy() for o in ch.enqueue(views)]
    torch.cuda.synchronize()
    assert (status == 1).all()
    maps = _view_maps()
    far = []
    M64 = np.eye(3)
    for k in range(8):
        true = np.linalg.inv(maps[k]) @ maps[0]
        true /= true[2, 2]
        Mk = chain[k].reshape(3, 3).astype(np.float64)
        if k:
            # each RANSAC link within test_gpu_pipeline's tolerances of the true pairwise map
            Hk = Hb[k - 1].reshape(3, 3).astype(np.float64) / Hb[k - 1][8]
            Ht = np.linalg.inv(maps[k]) @ maps[k - 1]
            Ht /= Ht[2, 2]
            if not (np.allclose(Hk, Ht, atol=0.6, rtol=0.05) and np.allclose(Hk[:2, :2], Ht[:2, :2], atol=5e-3)):
                far.append(("link", k, float(np.abs(Hk - Ht).max())))
            M64 = Hk @ M64
            M64 /= M64[2, 2]
        # the plan's chain is the product of those links; against the truth, the links' errors add up (no bundle
        # adjustment): the pipeline's tolerances per link
        if not np.allclose(Mk, M64, rtol=1e-4, atol=1e-4 * np.abs(M64).max()):
            far.append(("product", k, float(np.abs(Mk - M64).max())))
        kk = max(k, 1)
        if not (np.allclose(Mk, true, atol=0.6 * kk, rtol=0.05) and np.allclose(Mk[:2, :2], true[:2, :2], atol=5e-3 * kk)):
            far.append(("chain", k, float(np.abs(Mk - true).max()), float(np.abs(Mk[:2, :2] - true[:2, :2]).max())))
    assert not far, far
    # the canvas equals the oracle's in-order transform_blend on the records read back
    oc = np.zeros((SCENE_H, SCENE_W, 4), np.uint8)
    ow = np.zeros((SCENE_H, SCENE_W), np.float32)
    count = np.zeros((SCENE_H, SCENE_W), np.int32)
    mask, wts = np.full((VH, VW), 255, np.uint8), _feather()
    for k in range(8):
        host_view = views[k].cpu().numpy()
        tx, ty, nw, nh = (int(v) for v in records[k, 9:13])
        before = ow.copy()
        oc, ow = oracle.transform_blend(oc, ow, host_view, nw, nh, records[k, :9].view(np.float32), tx, ty, mask, wts)
        count += (ow != before)
    assert np.array_equal(canvas, oc) and np.array_equal(_u32(cwts), _u32(ow))
    multi = count >= 2
    assert multi.sum() > 0.3 * SCENE_W * SCENE_H
    diff = np.abs(canvas[..., :3].astype(int) - scene[..., :3].astype(int))[multi]
    assert np.median(diff) <= 3, np.median(diff)
    assert extent[0] <= 0 and extent[2] >= 7 * 70 + VW - 10
    ch.close()


def test_detect_to_blend_graph_replays_on_another_scene(nm, cuda):
    """The whole chain, detection included, captured into one HIP graph: replayed on a second scene written into the
    captured frame buffers it equals eager calls on that scene bit for bit."""
    import torch
    v1 = _views(nm, cuda, _scene(90))
    v2 = _views(nm, cuda, _scene(91))
    bufs = [v.clone() for v in v1]
    ch = _Chain(nm, cuda)
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
    assert (got[1] == 1).all() and got[6].max() > 0 and (got[2][:, 13] == 1).all()
    ch.close()
