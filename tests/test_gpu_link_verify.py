"""Link verification on the device (nm_link_verify_batch_dev_f32): equal to the host twin bit for bit on every output,
independent of a pair's slot and of n, and capturable between the refit and the mosaic plan."""
import numpy as np
import pytest

import helpers
from test_link_verify_host import FRAMES, MAPS, disc, frame

pytestmark = pytest.mark.gpu

F32 = np.float32


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same(dev_out, host_out):
    st, why, stats = (o.cpu().numpy() for o in dev_out)
    return (np.array_equal(st, host_out[0]) and np.array_equal(why, host_out[1]) and
            np.array_equal(stats.view(np.uint64), host_out[2].view(np.uint64)))


def _both(nm, dev, As, Bs, H, **kw):
    """(device outputs, host twin outputs) of one call; frames are uploaded once each (repeated arrays share a tensor)"""
    up = {}
    for a in list(As) + list(Bs):
        if id(a) not in up:
            up[id(a)] = _t(a, dev)
    dkw = {k: (_t(np.asarray(v, F32 if k == "mask" else np.int32), dev) if k in ("mask", "status", "inliers") and v is not None
               else v) for k, v in kw.items()}
    got = nm.link_verify_batch_dev([up[id(a)] for a in As], [up[id(b)] for b in Bs], _t(np.asarray(H, F32), dev), **dkw)
    return got, nm.link_verify_host(As, Bs, H, **kw)


def _pairs(size, n):
    """n pairs over five frames of one size (frame k + 1 is B of pair k and A of pair k + 1), the maps in turn"""
    fw, fh = size
    frames = [frame(10 + k, fw, fh) for k in range(5)]
    maps = [np.asarray(m, F32).reshape(9) for m in MAPS.values()]
    return ([frames[k % 5] for k in range(n)], [frames[(k + 1) % 5] for k in range(n)],
            np.stack([maps[k % len(maps)] for k in range(n)]))


@pytest.mark.parametrize("size", FRAMES)
@pytest.mark.parametrize("n", [1, 2, 33, 64])
def test_device_equals_host_twin(nm, cuda, size, n):
    As, Bs, H = _pairs(size, n)
    for stride, mask in ((1, None), (2, disc(*size)), (3, None), (7, disc(*size)), (64, None)):
        got, want = _both(nm, cuda, As, Bs, H, stride=stride, mask=mask, inliers=list(range(8, 8 + n)))
        assert _same(got, want), (size, n, stride)
    assert want[2][:, 1].max() == 0 or min(size) >= 64


def test_pairs_of_one_call_fail_different_gates(nm, cuda):
    fw, fh = 64, 48
    A = frame(7, fw, fh)
    I = np.eye(3).reshape(9)
    nan = I.copy()
    nan[4] = np.nan
    refl = np.array([[-1, 0, fw - 1], [0, 1, 0], [0, 0, 1]], float).reshape(9)
    out = np.asarray(MAPS["outside"], float).reshape(9)
    As = [A] * 7
    Bs = [A, A, A, A, A[:, ::-1].copy(), A, np.full_like(A, 90)]
    H = np.stack([I, I, nan, I, refl, out, I]).astype(F32)
    kw = dict(status=[1, 0, 1, 1, 1, 1, 1], inliers=[50, 50, 50, 3, 50, 50, 50], stride=3, min_inliers=12)
    got, want = _both(nm, cuda, As, Bs, H, **kw)
    assert _same(got, want)
    assert want[1].tolist() == [0, 1, 1, 2, 4, 8 | 16, 16] and want[0].tolist() == [1, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("size,stride", [((1920, 1080), 2), ((1920, 1080), 1), ((4096, 2160), 4)])
def test_large_frames_equal_host_twin(nm, cuda, size, stride):
    """More lattice tiles than workgroups per pair, so workgroups walk several tiles."""
    fw, fh = size
    rng = np.random.default_rng(fw + stride)
    A = (255 * rng.random((fh, fw), dtype=F32)).astype(F32)
    B = (0.5 * np.roll(A, (3, -5), (0, 1)) + 0.5 * np.roll(A, (4, -4), (0, 1)) + 7).astype(F32)
    A[5, 7], B[100, 200], B[fh - 1, fw - 1] = np.nan, 300.0, -1.0
    H = np.array([[1.001, 0.002, -4.6], [-0.001, 0.999, 3.4], [1e-7, -2e-7, 1]], F32).reshape(1, 9)
    got, want = _both(nm, cuda, [A], [B], H, stride=stride, inliers=[40])
    assert _same(got, want), want
    assert want[2][0, 0] > 0.9 * (fw // stride) * (fh // stride)


def test_outputs_do_not_depend_on_slot_or_n(nm, cuda):
    fw, fh = 131, 97
    P = (frame(30, fw, fh), frame(31, fw, fh), np.asarray(MAPS["homography"], F32).reshape(9))
    alone, _ = _both(nm, cuda, [P[0]], [P[1]], P[2][None], stride=2)
    alone = [o.cpu().numpy() for o in alone]
    As, Bs, H = _pairs((fw, fh), 64)
    for slot in (0, 31, 32, 63):
        a, b, h = list(As), list(Bs), H.copy()
        a[slot], b[slot], h[slot] = P
        got, want = _both(nm, cuda, a, b, h, stride=2)
        assert _same(got, want)
        got = [o.cpu().numpy() for o in got]
        assert all(np.array_equal(g[slot:slot + 1].view(np.uint8), o.view(np.uint8)) for g, o in zip(got, alone)), slot


# ---- the chain: ingest -> detect -> match -> RANSAC -> refit -> verify -> plan, on the views of tests/test_gpu_mosaic.py ----

VW, VH, CAP, SCENE_W, SCENE_H = 640, 480, 8192, 1240, 600


def _view_maps():
    maps = []
    for k in range(8):
        deg = 0.0 if k == 0 else 1.5 * np.sin(k)
        c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
        maps.append(np.array([[c, -s, 40 + 70 * k], [s, c, 50 + 14 * (-1) ** k], [0, 0, 1]], np.float64))
    return maps


def _views(nm, dev, seed):
    import torch
    g = np.clip(helpers.blurred_frame(seed, SCENE_W, SCENE_H, sigma=2.0) * 1.4, 0, 255).astype(np.uint8)
    scene = np.stack([g, np.roll(g, 3, 1), np.roll(g, 5, 0), np.full_like(g, 255)], -1)
    out = [nm.resample_perspective(_t(scene, dev), VW, VH, _t(np.linalg.inv(A).astype(F32), dev), inverse=True)[0]
           for A in _view_maps()]
    torch.cuda.synchronize()
    return out


class _Chain:
    BAD = 3                               # the link whose map the flag overwrites with the identity (a wrong map)

    def __init__(self, nm, dev):
        import torch
        self.nm = nm
        self.arenas = [nm.SiftArena(VW, VH, CAP) for _ in range(8)]
        self.res = [torch.full((CAP,), -1, dtype=torch.int32, device=dev) for _ in range(7)]
        self.mws = nm.MatchBatchDevWorkspace(7, CAP, CAP, dev)
        self.rws = nm.RansacBatchWorkspace(7, CAP, 2048, dev)
        self.vws = nm.LinkVerifyWorkspace(7, dev)
        self.flag = torch.zeros(1, dtype=torch.bool, device=dev)
        self.wrong = _t(np.eye(3, dtype=F32).reshape(9), dev)

    def enqueue(self, views):
        import torch
        nm = self.nm
        A, B = self.arenas[:-1], self.arenas[1:]
        grays = nm.ingest_batch(views)
        nm.detect_describe_batch(self.arenas, grays)
        pts = ([a.x for a in A], [a.y for a in A], [a.num_items for a in A], [b.x for b in B], [b.y for b in B], self.res)
        nm.sift_match_batch_dev([a.desc for a in A], [a.num_items for a in A], [b.desc for b in B],
                                [b.num_items for b in B], self.res, 0.8, workspace=self.mws)
        Hb, _, _, status = nm.ransac_batch_dev(2, *pts, iterations=2048, threshold=1.0, seeds=list(range(7)), capA=CAP,
                                               workspace=self.rws)
        H, count, st, _ = nm.ransac_refit_batch_dev(2, *pts, Hb, status=status, rounds=2, threshold=1.0, capA=CAP)
        H[self.BAD].copy_(torch.where(self.flag, self.wrong, H[self.BAD]))
        ok, why, stats = nm.link_verify_batch_dev(grays[:-1], grays[1:], H, status=st, inliers=count, workspace=self.vws)
        records, chain, _ = nm.mosaic_plan(H, ok, VW, VH, SCENE_W, SCENE_H, 40, 64)
        return H, count, ok, why, stats, records, chain

    def close(self):
        for a in self.arenas:
            a.close()


def test_chain_with_verification_captures_and_breaks_at_a_wrong_link(nm, oracle, cuda):
    import torch
    v1, v2 = _views(nm, cuda, 90), _views(nm, cuda, 91)
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
    for flag in (False, True):
        ch.flag.fill_(flag)
        for r in ch.res:
            r.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = [o.cpu().numpy().copy() for o in captured]
        for r in ch.res:
            r.fill_(-1)
        with torch.cuda.stream(s):
            want = ch.enqueue([v.clone() for v in v2])
        torch.cuda.synchronize()
        want = [o.cpu().numpy().copy() for o in want]
        for a, b in zip(got, want):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        H, count, ok, why, stats, records, chain = got
        placed = records.view(np.int32).reshape(8, 16)[:, 13]
        if not flag:
            assert (ok == 1).all() and (why == 0).all() and (placed == 1).all(), (why, stats)
        else:
            assert ok.tolist() == [1, 1, 1, 0, 1, 1, 1] and why[ch.BAD] & nm.LINK_LOW_NCC, (why, stats)
            assert placed.tolist() == [1, 1, 1, 1, 0, 0, 0, 0]
    ch.close()
