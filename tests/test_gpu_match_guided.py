"""nm_sift_match_guided_batch_dev_f32 on the MI355X: bit-identity with its host twin over batch sizes and mixed pairs (the
match screens stay at their defaults: the guided call does not use them), slot independence, sentinel-guarded outputs, a
real 1080p pair against the restatement tests/guided_ref.py, and match -> RANSAC -> refit -> guided -> refit captured into
one HIP graph."""
import ctypes as C

import numpy as np
import pytest

import guided_ref as G
import ransac_refit_ref as F
from test_match_guided_host import random_pair

pytestmark = pytest.mark.gpu

CAPA, CAPB = 1100, 1200
R2 = 6.0
OUT = ("result", "count", "best")


def _u32(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _padded(p):
    """The pair's arrays at the call's capacities; the rows beyond the sizes hold plausible values that must not be read."""
    q = dict(p)
    for key, cap in (("A", CAPA), ("B", CAPB)):
        full = np.full((cap, 128), 1.0, np.float32)
        full[:len(p[key])] = p[key]
        q[key] = full
    for key, cap in (("ax", CAPA), ("ay", CAPA), ("bx", CAPB), ("by", CAPB)):
        full = np.full(cap, 5.0, np.float32)
        full[:len(p[key])] = p[key]
        q[key] = full
    return q


def _mixed(n):
    sizes = [(300, 280), (0, 200), (257, 1030), (1100, 1200), (37, 3), (700, 0), (64, 65), (1, 1), (513, 700), (1024, 1025)]
    pairs = []
    for k in range(n):
        ra, rb = sizes[k % len(sizes)]
        p = random_pair(500 + k, max(ra, 1), max(rb, 1), nA=ra, nB=rb, negative=(0,) if ra > 100 else ())
        pairs.append(_padded(p))
    if n >= 3:
        pairs[2]["status"] = 0
    if n >= 16:
        pairs[9]["status"] = 5
        pairs[11]["H"] = pairs[11]["H"].copy()
        pairs[11]["H"][4] = np.nan
        pairs[12]["nA"], pairs[12]["nB"] = 10 ** 6, -3
        pairs[13]["H"] = np.array([1, 0, 0, 0, 1, 0, -1.0 / 16, 0, 1], np.float32)
    return pairs


def _host(nm, pairs, radius2=R2, ambiguity=0.8, max_distance=np.inf, status=True):
    k = lambda key: [p[key] for p in pairs]
    out = nm.sift_match_guided_host(k("A"), k("ax"), k("ay"), k("nA"), k("B"), k("bx"), k("by"), k("nB"), np.stack(k("H")),
                                    status=np.array(k("status"), np.int32) if status else None, radius2=radius2,
                                    ambiguity=ambiguity, max_distance=max_distance, capA=CAPA, capB=CAPB, want_distance=True)
    return dict(zip(OUT, out))


def _upload(pairs, dev):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return [dict(A=t(p["A"]), ax=t(p["ax"]), ay=t(p["ay"]), B=t(p["B"]), bx=t(p["bx"]), by=t(p["by"]),
                 nA=t(np.array([p["nA"]], np.int32)), nB=t(np.array([p["nB"]], np.int32))) for p in pairs]


def _device(nm, pairs, dev, radius2=R2, ambiguity=0.8, max_distance=np.inf, status=True, up=None):
    import torch
    up = _upload(pairs, dev) if up is None else up
    k = lambda key: [u[key] for u in up]
    Hd = torch.from_numpy(np.stack([p["H"] for p in pairs])).to(dev)
    st = torch.from_numpy(np.array([p["status"] for p in pairs], np.int32)).to(dev) if status else None
    res, cnt, best = nm.sift_match_guided_batch_dev(k("A"), k("ax"), k("ay"), k("nA"), k("B"), k("bx"), k("by"), k("nB"), Hd,
                                                    status=st, radius2=radius2, ambiguity=ambiguity,
                                                    max_distance=max_distance, capA=CAPA, capB=CAPB, want_distance=True)
    torch.cuda.synchronize()
    return dict(result=np.stack([r.cpu().numpy() for r in res]), count=cnt.cpu().numpy(),
                best=np.stack([b.cpu().numpy() for b in best]))


def _assert_same(a, b, what):
    for k in OUT:
        assert np.array_equal(_u32(a[k]), _u32(b[k])), (what, k)


@pytest.mark.parametrize("n", [1, 3, 16, 64])
def test_device_equals_host_twin(nm, cuda, n):
    pairs = _mixed(n)
    up = _upload(pairs, cuda)
    matched = 0
    for kw in (dict(), dict(radius2=30.0, ambiguity=0.95), dict(radius2=1e12), dict(radius2=0.5, max_distance=40.0)):
        want = _host(nm, pairs, **kw)
        got = _device(nm, pairs, cuda, up=up, **kw)
        _assert_same(got, want, "n %d %r" % (n, kw))
        assert np.array_equal((got["result"] >= 0).sum(axis=1), got["count"])
        matched += int(got["count"].sum())
    assert matched > 0, "nothing matched: the comparison covered nothing"
    # status_in = NULL means every pair is usable
    _assert_same(_device(nm, pairs, cuda, up=up, status=False), _host(nm, pairs, status=False), "status NULL")


def test_the_match_screen_does_not_matter_and_is_left_as_found(nm, cuda):
    """The guided call uses none of the blind matcher's three MFMA screens: the same bits under each, and the process-wide
    setting is back at what it was (its default, unless the environment chose another)."""
    pairs = _mixed(3)
    up = _upload(pairs, cuda)
    want = _host(nm, pairs)
    found = nm.get_match_screen()
    try:
        for screen in nm.MATCH_SCREENS:
            nm.set_match_screen(screen)
            _assert_same(_device(nm, pairs, cuda, up=up), want, screen)
    finally:
        nm.set_match_screen(found)
    assert nm.get_match_screen() == found


def test_slot_independence(nm, cuda):
    a, b = _padded(random_pair(5, 1100, 1030, negative=(3,))), _padded(random_pair(6, 300, 1200))
    alone, other = _device(nm, [a], cuda), _device(nm, [b], cuda)
    assert alone["count"][0] > 50
    for n, slot in ((2, 1), (16, 7), (33, 32), (64, 63), (64, 0), (64, 31)):
        pairs = [b] * n
        pairs[slot] = a
        r = _device(nm, pairs, cuda)
        for k in OUT:
            assert np.array_equal(_u32(r[k][slot]), _u32(alone[k][0])), (n, slot, k)
            assert np.array_equal(_u32(r[k][(slot + 1) % n]), _u32(other[k][0])), (n, slot, k)


@pytest.mark.parametrize("n", [5, 37])
def test_outputs_are_written_inside_their_bounds(nm, cuda, n):
    """result and best_distance of every pair and the counts lie in guarded buffers: capA rows per pair and n counts are
    written, nothing around them."""
    import torch
    Gd = 64
    pairs = _mixed(n)
    up = _upload(pairs, cuda)
    Hd = torch.from_numpy(np.stack([p["H"] for p in pairs])).to(cuda)
    st = torch.from_numpy(np.array([p["status"] for p in pairs], np.int32)).to(cuda)
    res = [torch.full((Gd + CAPA + Gd,), -7, dtype=torch.int32, device=cuda) for _ in range(n)]
    best = [torch.full((Gd + CAPA + Gd,), -7.0, dtype=torch.float32, device=cuda) for _ in range(n)]
    count = torch.full((Gd + n + Gd,), -7, dtype=torch.int32, device=cuda)
    arr = lambda ptrs: (C.c_void_p * n)(*ptrs)
    tab = lambda key: arr([u[key].data_ptr() for u in up])
    rc = nm.lib().nm_sift_match_guided_batch_dev_f32(n, tab("A"), tab("ax"), tab("ay"), tab("nA"), CAPA, tab("B"), tab("bx"),
                                                     tab("by"), tab("nB"), CAPB, Hd.data_ptr(), st.data_ptr(), R2, 0.8,
                                                     float("inf"), arr([r[Gd:].data_ptr() for r in res]),
                                                     count[Gd:].data_ptr(), arr([b[Gd:].data_ptr() for b in best]),
                                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    for b in res + best + [count]:
        assert (b[:Gd] == -7).all() and (b[-Gd:] == -7).all()
    want = _host(nm, pairs)
    assert np.array_equal(np.stack([r[Gd:-Gd].cpu().numpy() for r in res]), want["result"])
    assert np.array_equal(_u32(np.stack([b[Gd:-Gd].cpu().numpy() for b in best])), _u32(want["best"]))
    assert np.array_equal(count[Gd:-Gd].cpu().numpy(), want["count"])


def test_real_1080p_pair_equals_the_restatement(nm, cuda):
    """A 1080p frame and its warp under a known map (as test_gpu_pipeline builds its pair): about 12k x 12k rows, one
    call, against tests/guided_ref.py and the host twin."""
    import torch

    import helpers as Hh
    w, h, cap = 1920, 1080, 16384
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    g = np.clip(Hh.blurred_frame(90, w, h, sigma=2.0) * 1.4, 0, 255).astype(np.uint8)
    view0 = np.stack([g, np.roll(g, 3, 1), np.roll(g, 5, 0), np.full_like(g, 255)], -1)
    true_H = np.array([[0.995, 0.02, 9.0], [-0.015, 1.005, -6.0], [1.5e-5, -1e-5, 1.0]], np.float32)
    view1, _, _ = nm.resample_perspective(t(view0), w, h, t(true_H), inverse=True)
    arenas = [nm.SiftArena(w, h, cap) for _ in range(2)]
    nm.detect_describe_batch(arenas, [nm.grayscale(t(view0)), nm.grayscale(view1)])
    a, b = arenas
    Hd = t(true_H.reshape(1, 9))
    res, cnt, best = nm.sift_match_guided_batch_dev([a.desc], [a.x], [a.y], [a.num_items], [b.desc], [b.x], [b.y],
                                                    [b.num_items], Hd, radius2=9.0, capA=cap, capB=cap, want_distance=True)
    blind = torch.full((cap,), -1, dtype=torch.int32, device=cuda)
    nm.sift_match_batch_dev([a.desc], [a.num_items], [b.desc], [b.num_items], [blind], 0.8, capA=cap, capB=cap)
    torch.cuda.synchronize()
    nA, nB = int(a.num_items.item()), int(b.num_items.item())
    host = lambda x: x.cpu().numpy()
    args = (host(a.desc), host(a.x), host(a.y), nA, host(b.desc), host(b.x), host(b.y), nB, true_H.reshape(9))
    want, wcount, wbest = G.guided(*args, 1, 9.0, 0.8, np.inf, capA=cap, capB=cap)
    got = host(res[0])
    print("1080p pair: %d x %d rows, blind ratio matches %d, guided %d" % (nA, nB, int((blind >= 0).sum()), wcount))
    assert nA > 8000 and nB > 8000
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert int(cnt.item()) == wcount > int((blind >= 0).sum()) and np.array_equal(_u32(host(best[0])), _u32(wbest))
    hres, hcnt, hbest = nm.sift_match_guided_host(*[[v] for v in args[:8]], args[8].reshape(1, 9), radius2=9.0, capA=cap,
                                                  capB=cap, want_distance=True)
    assert np.array_equal(hres[0], got) and hcnt[0] == wcount and np.array_equal(_u32(hbest[0]), _u32(wbest))
    rows = np.flatnonzero(got >= 0)
    assert F.is_inlier32(true_H, args[1][rows], args[2][rows], args[5][got[rows]], args[6][got[rows]], 9.0).all()
    for ar in arenas:
        ar.close()


def test_chain_with_guided_matching_in_one_graph_replays_on_another_scene(nm, cuda):
    """detect -> match -> RANSAC -> refit -> guided -> refit on the eight synthetic views of test_gpu_mosaic, captured into
    one HIP graph on a single stream and replayed on a second scene: every output equals the eager run bit for bit."""
    import torch
    import test_gpu_mosaic as M

    class Chain(M._Chain):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.gres = [torch.full((M.CAP,), -1, dtype=torch.int32, device=self.dev) for _ in range(7)]

        def enqueue(self, views):
            nm_ = self.nm
            A, B = self.arenas[:-1], self.arenas[1:]
            nm_.detect_describe_batch(self.arenas, [nm_.grayscale(v) for v in views])
            nm_.sift_match_batch_dev([a.desc for a in A], [a.num_items for a in A], [b.desc for b in B],
                                     [b.num_items for b in B], self.res, 0.8, workspace=self.mws)
            pts = ([a.x for a in A], [a.y for a in A], [a.num_items for a in A], [b.x for b in B], [b.y for b in B])
            Hb, best, pos, status = nm_.ransac_batch_dev(2, *pts, self.res, iterations=self.iterations, threshold=1.0,
                                                         seeds=list(range(7)), capA=M.CAP, workspace=self.rws)
            Hr, cnt, st, done = nm_.ransac_refit_batch_dev(2, *pts, self.res, Hb, status=status, rounds=2, threshold=1.0,
                                                           capA=M.CAP)
            gres, gcnt = nm_.sift_match_guided_batch_dev([a.desc for a in A], [a.x for a in A], [a.y for a in A],
                                                         [a.num_items for a in A], [b.desc for b in B], [b.x for b in B],
                                                         [b.y for b in B], [b.num_items for b in B], Hr, status=st,
                                                         radius2=9.0, capA=M.CAP, capB=M.CAP, results=self.gres)
            Hg, cnt2, st2, done2 = nm_.ransac_refit_batch_dev(2, *pts, gres, Hr, status=st, rounds=2, threshold=1.0,
                                                              capA=M.CAP)
            return (Hb, best, status, Hr, cnt, st, gcnt, Hg, cnt2, st2, done2) + tuple(gres)

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
    for r in ch.res + ch.gres:
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
    Hb, best, status, Hr, cnt, st, gcnt, Hg, cnt2, st2, done2 = got[:11]
    blind = np.array([(r.cpu().numpy() >= 0).sum() for r in ch.res])
    assert (status == 1).all() and (st == 1).all() and (st2 == 1).all() and np.isfinite(Hg).all()
    assert (gcnt > blind).all(), (gcnt, blind)             # more correspondences than the blind ratio test kept
    assert np.array_equal(gcnt, [(r >= 0).sum() for r in got[11:]])
    # for the record: how far the links are from the true pairwise maps (threshold 1.0, 2 048 hypotheses, 2 rounds)
    maps = M._view_maps()
    err = lambda Hs: sum(F.corner_error(Hs[k], np.linalg.inv(maps[k + 1]) @ maps[k] / (np.linalg.inv(maps[k + 1]) @ maps[k])[2, 2],
                                        M.VW, M.VH) for k in range(7))
    print("corner error summed over 7 links: RANSAC %.3f px, refit %.3f px, refit -> guided -> refit %.3f px; "
          "matches %s -> %s, inliers %s -> %s" % (err(Hb), err(Hr), err(Hg), blind.tolist(), gcnt.tolist(), cnt.tolist(),
                                                 cnt2.tolist()))
    assert np.isfinite(err(Hg))
    ch.close()
