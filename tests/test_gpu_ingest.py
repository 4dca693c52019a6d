"""Batched frame ingest on the GPU: nm_resample_map_u8x4 against the oracle's per-channel sampling, nm_frame_ingest_batch_f32
against per-frame calls, the oracle and the per-frame channel chain (all bit for bit), identity mode, slot independence,
sentinel-guarded outputs, and raw distorted BGRA frames -> ingest -> detect -> match -> RANSAC -> plan -> blend captured
into one HIP graph."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_mosaic import SCENE_H, SCENE_W, VH, VW, _feather, _scene, _view_maps
from test_ingest_host import e2e_maps, e2e_oracle_gray_and_mask

pytestmark = pytest.mark.gpu


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _map(oracle, fw, fh, cols, rows, k1, rng, specials=True):
    """A radial map (oracle.undistort_map) from the output grid into the frame that leaves the frame on every side, with
    exact texel centres, NaN, +-inf and +-1e30 coordinates sprinkled in."""
    gx = np.linspace(-0.1 * fw, 1.1 * fw, cols, dtype=np.float64)
    gy = np.linspace(-0.1 * fh, 1.1 * fh, rows, dtype=np.float64)
    x, y = (a.astype(np.float32) for a in np.meshgrid(gx, gy))
    cam = np.array([0.9 * fw, 0.9 * fw, fw / 2, fh / 2], np.float32)
    u, v = oracle.undistort_map(x, y, cam, np.array([k1, 0, 0], np.float32))
    assert u.min() < -1 and u.max() > fw and v.min() < -1 and v.max() > fh
    if specials:
        n = u.size
        pick = rng.choice(n, n // 20, replace=False)
        u.flat[pick], v.flat[pick] = np.round(u.flat[pick]), np.round(v.flat[pick])
        for val in (np.nan, np.inf, -np.inf, 1e30, -1e30):
            for plane in (u, v):
                plane.flat[rng.choice(n, 7, replace=False)] = val
    return u, v


def _oracle_u8x4(oracle, frame, u, v):
    """The oracle's per-channel composition: each channel through resample_undistort (U8N), truncated to uint8."""
    return np.stack([oracle.resample_undistort(np.ascontiguousarray(frame[..., c]), u, v).astype(np.uint8)
                     for c in range(4)], -1)


GEOS = [(160, 120, 160, 120), (131, 97, 140, 90), (1920, 1080, 1920, 1080)]


@pytest.mark.parametrize("geo", GEOS, ids=lambda g: "%dx%d-to-%dx%d" % g)
@pytest.mark.parametrize("k1", [-0.15, 0.12])
def test_resample_map_u8x4_equals_oracle(nm, oracle, cuda, geo, k1):
    import torch
    fw, fh, cols, rows = geo
    rng = np.random.default_rng(fw + cols + int(100 * k1))
    frame = rng.integers(0, 256, (fh, fw, 4), dtype=np.uint8)
    u, v = _map(oracle, fw, fh, cols, rows, k1, rng)
    got = nm.resample_map_u8x4(_t(frame, cuda), _t(u, cuda), _t(v, cuda))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want = _oracle_u8x4(oracle, frame, u, v)
    assert np.array_equal(got, want), "differs at %d pixels" % (got != want).any(-1).sum()
    bad = ~np.isfinite(u) | ~np.isfinite(v) | (np.abs(u) > 1e20) | (np.abs(v) > 1e20)
    assert bad.sum() >= 50 and not got[bad].any()
    inside = (u > 0) & (u < fw - 1) & (v > 0) & (v < fh - 1)
    assert inside.sum() > 0.5 * cols * rows and got[inside].any()
    # on a perspective call's own map, the uchar4 result of both entries is the same
    M = np.array([[0.95, 0.08, -0.1 * fw], [-0.06, 1.05, 0.05 * fh], [1e-4, -2e-4, 1.0]], np.float32)
    res, xp, yp = nm.resample_perspective(_t(frame, cuda), cols, rows, _t(M, cuda), inverse=True)
    again = nm.resample_map_u8x4(_t(frame, cuda), xp, yp)
    torch.cuda.synchronize()
    assert torch.equal(res, again)


def _chain(nm, frame, u, v):
    """The parent commit's way to get the undistorted BGRA frame + gray: extract_channel -> cast_f32_u8 ->
    resample_undistort (U8N) -> put_channel for B, G, R, then grayscale (13 launches)."""
    import torch
    rows, cols = u.shape
    out = torch.zeros((rows, cols, 4), dtype=torch.uint8, device=frame.device)
    for c in range(3):
        plane = nm.cast_f32_u8(nm.extract_channel(frame, c))
        out = nm.put_channel(out, nm.resample_undistort(plane, u, v), c)
    return out, nm.grayscale(out)


BATCH_CASES = [(1, 131, 97, 140, 90), (3, 131, 97, 140, 90), (16, 131, 97, 140, 90), (64, 131, 97, 140, 90),
               (16, 1920, 1080, 1920, 1080)]


@pytest.mark.parametrize("case", BATCH_CASES, ids=lambda c: "n%d-%dx%d-to-%dx%d" % c)
def test_ingest_batch_equals_per_frame_oracle_and_chain(nm, oracle, cuda, case):
    import torch
    n, fw, fh, cols, rows = case
    rng = np.random.default_rng(n * 31 + fw)
    frames = [rng.integers(0, 256, (fh, fw, 4), dtype=np.uint8) for _ in range(n)]
    u, v = _map(oracle, fw, fh, cols, rows, -0.12 if n % 2 else 0.1, rng)
    fd = [_t(f, cuda) for f in frames]
    ud, vd = _t(u, cuda), _t(v, cuda)
    gray, und = nm.ingest_batch(fd, ud, vd, undistorted=True)
    gray_only = nm.ingest_batch(fd, ud, vd)
    torch.cuda.synchronize()
    assert len(gray) == len(und) == len(gray_only) == n
    for k in range(n):
        per = nm.resample_map_u8x4(fd[k], ud, vd)
        per_gray = nm.grayscale(per)
        ch_bgra, ch_gray = _chain(nm, fd[k], ud, vd)
        torch.cuda.synchronize()
        assert torch.equal(und[k], per), k
        assert torch.equal(gray[k].view(torch.int32), per_gray.view(torch.int32)), k
        assert torch.equal(gray_only[k].view(torch.int32), gray[k].view(torch.int32)), k
        assert torch.equal(und[k][..., :3], ch_bgra[..., :3]), k
        assert torch.equal(gray[k].view(torch.int32), ch_gray.view(torch.int32)), k
        want = _oracle_u8x4(oracle, frames[k], u, v)
        assert np.array_equal(und[k].cpu().numpy(), want), k
        assert np.array_equal(_u32(gray[k].cpu().numpy()), _u32(oracle.grayscale(want))), k


def test_identity_mode_repeats_and_slots(nm, cuda):
    import torch
    rng = np.random.default_rng(17)
    fw, fh = 203, 117
    frames = [_t(rng.integers(0, 256, (fh, fw, 4), dtype=np.uint8), cuda) for _ in range(64)]
    gray = nm.ingest_batch(frames)
    torch.cuda.synchronize()
    for k in range(64):
        assert torch.equal(gray[k].view(torch.int32), nm.grayscale(frames[k]).view(torch.int32)), k
    # repeated frame pointers, identity and mapped
    u, v = (a.to(cuda) for a in torch.meshgrid(torch.arange(150, dtype=torch.float32) * 1.3 - 7,
                                                 torch.arange(160, dtype=torch.float32) * 0.7 + 3, indexing="xy"))
    rep = [frames[5], frames[9], frames[5], frames[5], frames[9]]
    g_id = nm.ingest_batch(rep)
    g_map, u_map = nm.ingest_batch(rep, u, v, undistorted=True)
    one = nm.resample_map_u8x4(frames[5], u, v)
    torch.cuda.synchronize()
    for k in (0, 2, 3):
        assert torch.equal(g_id[k], g_id[0]) and torch.equal(u_map[k], one)
        assert torch.equal(g_map[k].view(torch.int32), nm.grayscale(one).view(torch.int32))
    assert torch.equal(g_id[4], nm.grayscale(frames[9]))
    # frame X alone at slot 0 equals frame X at slot 63 of a 64-frame call, mapped and identity
    X = frames[40]
    others = frames[:40] + frames[41:]
    for args in ((), (u, v)):
        alone = nm.ingest_batch([X], *args, undistorted=bool(args))
        full = nm.ingest_batch(others + [X], *args, undistorted=bool(args))
        torch.cuda.synchronize()
        if args:
            assert torch.equal(alone[1][0], full[1][63])
            alone, full = alone[0], full[0]
        assert torch.equal(alone[0].view(torch.int32), full[63].view(torch.int32))


@pytest.mark.parametrize("mode", ["gray_and_undistorted", "gray_only", "identity"])
def test_outputs_inside_guarded_buffers(nm, oracle, cuda, mode):
    """Every output plane sits between sentinel guard bands in one buffer: after the call the guards are unchanged and
    the planes equal the wrapper's results."""
    import torch
    rng = np.random.default_rng(3)
    n, fw, fh = 7, 97, 61
    cols, rows = (fw, fh) if mode == "identity" else (113, 58)
    P, G = cols * rows, 1000
    frames = [_t(rng.integers(0, 256, (fh, fw, 4), dtype=np.uint8), cuda) for _ in range(n)]
    if mode == "identity":
        ud = vd = None
    else:
        u, v = _map(oracle, fw, fh, cols, rows, 0.1, rng)
        ud, vd = _t(u, cuda), _t(v, cuda)
    gbuf = torch.full((G + n * (P + G),), -7, dtype=torch.int32, device=cuda)
    ubuf = torch.full((4 * (G + n * (P + G)),), 0xA5, dtype=torch.uint8, device=cuda)
    gptr = [gbuf.data_ptr() + 4 * (G + k * (P + G)) for k in range(n)]
    uptr = [ubuf.data_ptr() + 4 * (G + k * (P + G)) for k in range(n)]
    arr = lambda vals: (C.c_void_p * n)(*vals)
    want_undist = mode == "gray_and_undistorted"
    st = torch.cuda.current_stream().cuda_stream
    r = nm.lib().nm_frame_ingest_batch_f32(n, arr([f.data_ptr() for f in frames]), fw, fh,
                                           ud.data_ptr() if ud is not None else None,
                                           vd.data_ptr() if vd is not None else None, cols, rows, arr(gptr),
                                           arr(uptr) if want_undist else None, st)
    assert r == 0
    if mode == "identity":
        want = nm.ingest_batch(frames)
    else:
        want, want_u = nm.ingest_batch(frames, ud, vd, undistorted=True)
    torch.cuda.synchronize()
    g, ub = gbuf.cpu().numpy(), ubuf.cpu().numpy()
    for k in range(n + 1):
        s = k * (P + G)
        assert (g[s:s + G] == -7).all() and (ub[4 * s:4 * (s + G)] == 0xA5).all(), k
        if k < n:
            assert np.array_equal(g[s + G:s + G + P], want[k].view(torch.int32).cpu().numpy().reshape(-1)), k
            plane = ub[4 * (s + G):4 * (s + G + P)]
            if want_undist:
                assert np.array_equal(plane, want_u[k].cpu().numpy().reshape(-1)), k
            else:
                assert (plane == 0xA5).all(), k


# ---- end to end: raw distorted BGRA frames -> ingest -> detect -> match -> RANSAC -> plan -> blend, one graph ----

CAP = 8192
E2E_SEEDS = (3, 4)


class _IngestChain:
    """ingest (gray + undistorted) -> detect (masked arenas) -> match (7 pairs k -> k+1) -> RANSAC -> plan -> blend of
    the undistorted frames, all on the current stream with own workspaces."""

    def __init__(self, nm, dev, um, vm, mask, iterations=2048):
        import torch
        self.nm, self.dev, self.iterations = nm, dev, iterations
        self.um, self.vm = um, vm
        self.arenas = [nm.SiftArena(VW, VH, CAP) for _ in range(8)]
        for a in self.arenas:
            a.set_mask(mask)
        self.res = [torch.full((CAP,), -1, dtype=torch.int32, device=dev) for _ in range(7)]
        self.mws = nm.MatchBatchDevWorkspace(7, CAP, CAP, dev)
        self.rws = nm.RansacBatchWorkspace(7, CAP, iterations, dev)
        self.bmask = torch.full((VH, VW), 255, dtype=torch.uint8, device=dev)
        self.wts = _t(_feather(), dev)
        self.canvas = torch.zeros((SCENE_H, SCENE_W, 4), dtype=torch.uint8, device=dev)
        self.cwts = torch.zeros((SCENE_H, SCENE_W), dtype=torch.float32, device=dev)
        A0 = _view_maps()[0]
        self.ox, self.oy = int(A0[0, 2]), int(A0[1, 2])

    def enqueue(self, raw):
        nm = self.nm
        gray, und = nm.ingest_batch(raw, self.um, self.vm, undistorted=True)
        A, B = self.arenas[:-1], self.arenas[1:]
        nm.detect_describe_batch(self.arenas, gray)
        nm.sift_match_batch_dev([a.desc for a in A], [a.num_items for a in A], [b.desc for b in B],
                                [b.num_items for b in B], self.res, 0.8, workspace=self.mws)
        Hb, best, pos, status = nm.ransac_batch_dev(2, [a.x for a in A], [a.y for a in A], [a.num_items for a in A],
                                                    [b.x for b in B], [b.y for b in B], self.res,
                                                    iterations=self.iterations, threshold=1.0, seeds=list(range(7)),
                                                    capA=CAP, workspace=self.rws)
        records, chain, extent = nm.mosaic_plan(Hb, status, VW, VH, SCENE_W, SCENE_H, self.ox, self.oy)
        self.canvas.zero_()
        self.cwts.zero_()
        nm.transform_blend_batch(self.canvas, self.cwts, und, self.bmask, self.wts, records)
        counts = [a.num_items for a in self.arenas]
        return [Hb, status, records, chain, extent, self.canvas, self.cwts] + gray + und + counts

    def close(self):
        for a in self.arenas:
            a.close()


def _raw_views(nm, dev, seed, up, vp):
    """The 8 views of scene `seed` (as test_gpu_mosaic renders them), each distorted through the k1 = +0.12 map."""
    import torch
    out = []
    for A in _view_maps():
        v, _, _ = nm.resample_perspective(_t(_scene(seed), dev), VW, VH, _t(np.linalg.inv(A).astype(np.float32), dev),
                                          inverse=True)
        out.append(nm.resample_map_u8x4(v, up, vp))
    torch.cuda.synchronize()
    return out


def test_distorted_frames_to_blend_in_one_graph(nm, oracle, cuda):
    import torch
    (up, vp), (um, vm) = e2e_maps(oracle)
    upd, vpd, umd, vmd = (_t(a, cuda) for a in (up, vp, um, vm))
    ones = _t(np.ones((VH, VW), np.float32), cuda)
    mask = nm.resample_mask(ones, umd, vmd, 0.5).float()
    raw1 = _raw_views(nm, cuda, E2E_SEEDS[0], upd, vpd)
    raw2 = _raw_views(nm, cuda, E2E_SEEDS[1], upd, vpd)
    ch = _IngestChain(nm, cuda, umd, vmd, mask)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eager1 = [o.cpu().numpy().copy() for o in ch.enqueue([r.clone() for r in raw1])]
    torch.cuda.synchronize()
    assert (eager1[1] == 1).all(), eager1[1]
    assert (eager1[2][:, 13] == 1).all() and eager1[6].max() > 0
    # the ingest and two frames' detections against the oracle, from the same raw frames
    og, om = e2e_oracle_gray_and_mask(oracle, [raw1[k].cpu().numpy() for k in range(8)], um, vm)
    assert np.array_equal(mask.cpu().numpy(), om)
    for k in range(8):
        assert np.array_equal(_u32(eager1[7 + k]), _u32(og[k])), k
    for k in (0, 5):
        ref = oracle.sift_detect_describe(og[k], CAP, mask=om)
        a = ch.arenas[k]
        n = int(eager1[23 + k].reshape(-1)[0])
        assert n == ref["n"], (k, n, ref["n"])
        assert np.array_equal(a.kpts[:n].cpu().numpy(), ref["kpts"]) and np.array_equal(a.desc[:n].cpu().numpy(), ref["desc"])
    # capture with scene 1 in the captured buffers, replay on scene 2, compare with eager calls on scene 2
    bufs = [r.clone() for r in raw1]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        captured = ch.enqueue(bufs)
    for b, r in zip(bufs, raw2):
        b.copy_(r)
    for r in ch.res:
        r.fill_(-1)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    got = [o.cpu().numpy().copy() for o in captured]
    with torch.cuda.stream(s):
        want = [o.cpu().numpy().copy() for o in ch.enqueue([r.clone() for r in raw2])]
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(_u32(a) if a.dtype.itemsize == 4 else a, _u32(b) if b.dtype.itemsize == 4 else b), i
    assert (got[1] == 1).all() and (got[2][:, 13] == 1).all() and got[6].max() > 0
    ch.close()
