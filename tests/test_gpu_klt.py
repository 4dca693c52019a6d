"""The device entries of the gray pyramid and the KLT tracker against their host twins, bit for bit (the host twins against the
Python model: tests/test_klt_host.py): every shared case of tests/klt_ref.py; 1, 3 and 64 pairs with repeated pointers and
oversize output tensors full of garbage; the C entries called with 64-slot tables whose entries beyond n are garbage; grid
caps 1 and 3, so that the persistent loops make several trips; 8, 16 and 32 lanes per point; blocks aligned to 16 bytes only
and to 4; and pyramid -> track -> RANSAC -> refit as one HIP graph replayed on new frames."""
import ctypes as C

import numpy as np
import pytest

import klt_ref as K

pytestmark = pytest.mark.gpu

F32 = np.float32
CASES = K.cases()


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def same_track(got, want, k=slice(None)):
    """a device KltTrack (lists of tensors) against the host's arrays, bit for bit"""
    import torch
    for name in ("dst_xs", "dst_ys", "matches", "reason", "residual", "fb_error"):
        g = torch.stack(getattr(got, name)).cpu().numpy()
        w = getattr(want, name)[k]
        assert np.array_equal(g.view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), name
    assert np.array_equal(got.count.cpu().numpy().astype(np.uint64), want.count[k])


def host_and_device(nm, cuda, c, offset=0):
    """one case on both sides; offset: floats by which every device block is shifted from its allocation"""
    import torch
    h, w = c["A"].shape
    kw = c["kw"]
    levels = kw.get("levels", 4)
    xs, ys = K.padded(c)
    st = c.get("status")
    pyr, mp = nm.gray_pyramid_host([c["A"], c["B"]], levels=levels, mask=c.get("mask"))
    want = nm.klt_track_host([pyr[0]], [pyr[1]], w, h, [xs], [ys], [c["nA"]], mask_pyr=mp, H=c.get("H"),
                             status=None if st is None else [st], capA=c["capA"], **kw)
    floats = nm.gray_pyramid_floats(w, h, levels)
    pool = torch.full((2, floats + 8), float("nan"), dtype=torch.float32, device=cuda)
    blocks = [pool[0, offset:offset + floats], pool[1, offset:offset + floats]]
    mask = None if c.get("mask") is None else _t(c["mask"], cuda)
    d_pyr, d_mp = nm.gray_pyramid_batch([_t(c["A"], cuda), _t(c["B"], cuda)], levels=levels, mask=mask, pyrs=blocks)
    for d, hst in zip(d_pyr, pyr):                                   # the floats between levels belong to nobody
        for l in range(levels):
            assert np.array_equal(nm.gray_pyramid_level(d, w, h, l).cpu().numpy().view(np.uint32),
                                  nm.gray_pyramid_level(hst, w, h, l).view(np.uint32)), l
    assert torch.isnan(pool[:, :offset]).all() and torch.isnan(pool[:, offset + floats:]).all()
    assert (d_mp is None) == (mp is None) and (mp is None or np.array_equal(d_mp.cpu().numpy(), mp))
    H = None if c.get("H") is None else _t(c["H"].reshape(1, 9), cuda)
    got = nm.klt_track_batch_dev([d_pyr[0]], [d_pyr[1]], w, h, [_t(xs, cuda)], [_t(ys, cuda)],
                                 [_t(np.array([c["nA"]], np.int32), cuda)], mask_pyr=d_mp, H=H,
                                 status=None if st is None else _t(np.array([st], np.int32), cuda), capA=c["capA"],
                                 want_reason=True, want_residual=True, want_fb_error=True, **kw)
    return got, want


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_device_equals_the_host_twin(nm, cuda, c):
    got, want = host_and_device(nm, cuda, c)
    same_track(got, want)


@pytest.mark.parametrize("offset,cap", [(4, 0), (1, 0), (0, 1), (4, 3)])
def test_alignment_and_grid_caps(nm, cuda, offset, cap):
    """blocks aligned to 16 bytes only (offset 4 floats from an allocation) take the 16-byte path at the levels whose width is a
    multiple of 4, blocks aligned to 4 bytes the scalar one; with the cap at 1 or 3 workgroups every launch walks its units"""
    prev = nm.klt_set_grid_cap(cap)
    try:
        for name in ("edges 64x64 r3 L4", "edges 97x61 r7 L3", "rows nA 130 capA 131", "mask cuts level 2 only"):
            c = next(c for c in CASES if c["name"] == name)
            got, want = host_and_device(nm, cuda, c, offset)
            same_track(got, want)
    finally:
        nm.klt_set_grid_cap(prev)


@pytest.mark.parametrize("n", [1, 3, 64])
def test_batches_repeated_pointers_and_garbage_in_the_outputs(nm, cuda, n):
    """n pairs over three frames' pyramids (pointers repeat, A and B swap), a size per pair, output tensors longer than capA
    and pre-filled with garbage (nothing beyond capA is written); the second call with optional outputs absent leaves the
    required ones equal. The Python wrapper passes tables of exactly n entries: the next test has the longer tables."""
    import torch
    fw, fh, levels, capA = 97, 61, 3, 40
    grays = [K.textured(1, 105, 69)[3:64, 5:102].copy(), K.textured(1, 105, 69)[2:63, 3:100].copy(), K.textured(1, 97, 61)]
    pyr, _ = nm.gray_pyramid_host(grays, levels=levels)
    d_pyr, _ = nm.gray_pyramid_batch([_t(g, cuda) for g in grays], levels=levels)
    xs, ys = K.grid_points(fw, fh, capA, 3)
    ia, ib = [k % 3 for k in range(n)], [(k + 1 + k // 3) % 3 for k in range(n)]
    nAs = [(7 * k + 1) % (capA + 6) for k in range(n)]
    H = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], F32), (n, 1))
    H[:, 2], H[:, 5] = np.arange(n) % 5 - 2, np.arange(n) % 3 - 1
    status = (np.arange(n) % 4 != 3).astype(np.int32)
    kw = dict(levels=levels, radius=3, iterations=6, fb_max=1.5, max_residual=20.0, capA=capA)
    want = nm.klt_track_host([pyr[i] for i in ia], [pyr[i] for i in ib], fw, fh, [xs] * n, [ys] * n, nAs, H=H, status=status, **kw)
    assert n == 1 or 0 < want.count.sum() < n * capA
    d_xs, d_ys = _t(xs, cuda), _t(ys, cuda)
    args = ([d_pyr[i] for i in ia], [d_pyr[i] for i in ib], fw, fh, [d_xs] * n, [d_ys] * n,
            [_t(np.array([v], np.int32), cuda) for v in nAs])
    junk = lambda dt, v: [torch.full((capA + 5,), v, dtype=dt, device=cuda) for _ in range(n)]
    out = nm.KltTrack(junk(torch.float32, 123.0), junk(torch.float32, float("nan")), junk(torch.int32, 77),
                      torch.full((n,), 0x5EED5EED5EED, dtype=torch.int64, device=cuda), junk(torch.uint8, 99),
                      junk(torch.float32, 5.0), junk(torch.float32, 6.0))
    got = nm.klt_track_batch_dev(*args, H=_t(H, cuda), status=_t(status, cuda), out=out, **kw)
    assert got is out
    cut = nm.KltTrack(*[[t[:capA] for t in f] if isinstance(f, list) else f for f in got])
    same_track(cut, want)
    assert all((t[capA:].cpu().numpy() == v).all() for f, v in ((got.dst_xs, 123.0), (got.matches, 77), (got.reason, 99)) for t in f)
    bare = nm.klt_track_batch_dev(*args, H=_t(H, cuda), status=_t(status, cuda), **kw)
    assert bare.reason is None and all(torch.equal(a, b[:capA]) for a, b in zip(bare.matches, got.matches))
    assert torch.equal(bare.count, got.count)


@pytest.mark.parametrize("n", [1, 3])
def test_tables_of_64_slots_with_unused_trailing_entries(nm, cuda, n):
    """nm_gray_pyramid_batch_f32 and nm_klt_track_batch_dev_f32 through the C interface with 64-slot HOST tables: the entries
    beyond n hold a garbage address (or NULL, on the second round), in the optional tables too, and are never used"""
    import torch
    fw, fh, levels, capA = 97, 61, 3, 24
    L = nm.lib()
    grays = [K.textured(1, 105, 69)[3:64, 5:102].copy(), K.textured(1, 105, 69)[2:63, 3:100].copy(), K.textured(4, 97, 61),
             K.textured(1, 105, 69)[4:65, 4:101].copy()]
    pyr, _ = nm.gray_pyramid_host(grays, levels=levels)
    xs, ys = K.grid_points(fw, fh, capA, 3)
    nAs = [capA, 9, 40][:n]
    kw = dict(levels=levels, radius=3, iterations=6, fb_max=1.5, max_residual=20.0)
    want = nm.klt_track_host(pyr[:n], pyr[1:n + 1], fw, fh, [xs] * n, [ys] * n, nAs, capA=capA, **kw)
    assert want.count.sum() > 0
    floats = nm.gray_pyramid_floats(fw, fh, levels)
    d_gray = [_t(g, cuda) for g in grays[:n + 1]]
    d_xs, d_ys = _t(xs, cuda), _t(ys, cuda)
    d_nA = [_t(np.array([v], np.int32), cuda) for v in nAs]
    for fill in (0xDEAD0000BEE0, None):
        table = lambda ts: (C.c_void_p * 64)(*([t.data_ptr() for t in ts] + [fill] * (64 - len(ts))))
        d_pyr = [torch.full((floats,), float("nan"), dtype=torch.float32, device=cuda) for _ in range(n + 1)]
        assert L.nm_gray_pyramid_batch_f32(n + 1, table(d_gray), fw, fh, levels, table(d_pyr), None, None,
                                           torch.cuda.current_stream().cuda_stream) == 0
        for d, hst in zip(d_pyr, pyr):
            for l in range(levels):
                assert np.array_equal(nm.gray_pyramid_level(d, fw, fh, l).cpu().numpy().view(np.uint32),
                                      nm.gray_pyramid_level(hst, fw, fh, l).view(np.uint32))
        new = lambda dt, v: [torch.full((capA,), v, dtype=dt, device=cuda) for _ in range(n)]
        out = nm.KltTrack(new(torch.float32, 123.0), new(torch.float32, 124.0), new(torch.int32, 77),
                          torch.full((n,), 99, dtype=torch.int64, device=cuda), new(torch.uint8, 99), new(torch.float32, 5.0),
                          new(torch.float32, 6.0))
        assert L.nm_klt_track_batch_dev_f32(n, table(d_pyr[:n]), table(d_pyr[1:]), fw, fh, levels, None, table([d_xs] * n),
                                            table([d_ys] * n), table(d_nA), capA, None, None, kw["radius"], kw["iterations"],
                                            2.0 ** -6, 16.0, 0.0, kw["max_residual"], kw["fb_max"], table(out.dst_xs),
                                            table(out.dst_ys), table(out.matches), out.count.data_ptr(), table(out.reason),
                                            table(out.residual), table(out.fb_error), torch.cuda.current_stream().cuda_stream) == 0
        same_track(out, want)


@pytest.mark.parametrize("lanes", [8, 32])
def test_results_do_not_depend_on_the_lanes_per_point(nm, cuda, lanes):
    prev = nm.klt_set_lanes(lanes)
    try:
        assert prev == 0
        for name in ("edges 64x64 r3 L4", "edges 97x61 r7 L3", "edges 97x61 r1 L3", "rows nA 130 capA 131", "H den <= 0 status 1",
                     "nan in B", "mask cuts level 2 only"):
            c = next(c for c in CASES if c["name"] == name)
            got, want = host_and_device(nm, cuda, c)
            same_track(got, want)
    finally:
        assert nm.klt_set_lanes(0) == lanes


@pytest.mark.parametrize("which", ["a", "b"])
def test_accuracy_inputs_equal_the_host_twin(nm, cuda, which):
    """the accuracy of tests/test_klt_host.py holds on the device by equality"""
    xs, ys = nm.klt_grid_points(K.AW, K.AH, K.ASTEP)
    A, B, _, H = K.accuracy_case(which)
    pyr, _ = nm.gray_pyramid_host([A, B], levels=K.ACC["levels"])
    want = nm.klt_track_host([pyr[0]], [pyr[1]], K.AW, K.AH, [xs], [ys], [len(xs)], H=H, **K.ACC)
    d_pyr, _ = nm.gray_pyramid_batch([_t(A, cuda), _t(B, cuda)], levels=K.ACC["levels"])
    got = nm.klt_track_batch_dev([d_pyr[0]], [d_pyr[1]], K.AW, K.AH, [_t(xs, cuda)], [_t(ys, cuda)],
                                 [_t(np.array([len(xs)], np.int32), cuda)], H=None if H is None else _t(H.reshape(1, 9), cuda),
                                 want_reason=True, want_residual=True, want_fb_error=True, **K.ACC)
    same_track(got, want)
    assert want.count[0] > 80


# ---- one graph ----------------------------------------------------------------------------------------------------------------
def graph_frames(seed, n=4, fw=160, fh=120):
    """n + 1 views of a smooth texture on a pan of (5, 2) px per frame"""
    g = K.textured(seed, fw + 5 * n + 4, fh + 2 * n + 4)
    return [np.ascontiguousarray(g[2 * k:2 * k + fh, 5 * k:5 * k + fw]) for k in range(n + 1)]


def test_pyramid_track_ransac_and_refit_in_one_graph(nm, cuda):
    import torch
    n, fw, fh, levels = 4, 160, 120, 3
    xs, ys = nm.klt_grid_points(fw, fh, 12)
    cap = len(xs)
    d_xs, d_ys, d_n = _t(xs, cuda), _t(ys, cuda), _t(np.array([cap], np.int32), cuda)
    grays = [torch.empty((fh, fw), dtype=torch.float32, device=cuda) for _ in range(n + 1)]
    kw = dict(levels=levels, radius=5, iterations=8, fb_max=1.0, capA=cap)

    def chain():
        pyr, _ = nm.gray_pyramid_batch(grays, levels=levels)
        tr = nm.klt_track_batch_dev(pyr[:-1], pyr[1:], fw, fh, [d_xs] * n, [d_ys] * n, [d_n] * n, **kw)
        tabs = ([d_xs] * n, [d_ys] * n, [d_n] * n, tr.dst_xs, tr.dst_ys, tr.matches)
        H, best, _, status = nm.ransac_batch_dev(0, *tabs, iterations=64, threshold=1.0, capA=cap)
        H2, count, st2, _ = nm.ransac_refit_batch_dev(0, *tabs, H, status, rounds=2, threshold=1.0, capA=cap)
        return pyr, tr, H2, count, st2

    def outputs(r):
        pyr, tr, H2, count, st2 = r
        return [torch.stack(v).cpu().numpy() for v in (tr.dst_xs, tr.dst_ys, tr.matches)] + \
               [v.cpu().numpy() for v in (tr.count, H2, count, st2)]

    eager = []
    for seed in (11, 12):
        views = graph_frames(seed, n, fw, fh)
        for g, v in zip(grays, views):
            g.copy_(_t(v, cuda))
        got = outputs(chain())
        pyr, _ = nm.gray_pyramid_host(views, levels=levels)
        want = nm.klt_track_host(pyr[:-1], pyr[1:], fw, fh, [xs] * n, [ys] * n, [cap] * n, **kw)
        assert np.array_equal(got[0].view(np.uint32), want.dst_xs.view(np.uint32)) and np.array_equal(got[2], want.matches)
        assert (want.count > cap // 2).all() and (got[6] == 1).all()
        for Hk in got[4].astype(np.float64).reshape(n, 3, 3):           # the refitted maps are the pan
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
        r[1].count.fill_(0x7777777777)
        for t in r[1].matches:
            t.fill_(9)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(outputs(r), want):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
