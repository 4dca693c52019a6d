"""The keypoint selection on the GPU (nm_sift_select_batch_dev) against its host twin, bit for bit: 1, 5 and 64 frames in one
call with ragged counts, a cell longer than any LDS tile, a nearly empty 64 x 64 grid, equal scores, keep = 1 and m - 1,
every subset of the payload, sentinel-filled outputs that rows beyond the count and refused calls must leave alone, slot
independence, real descriptors behind the frame driver, and the chain detect -> select -> finish -> u8 match -> mutual u8
captured into one HIP graph. The host twin itself is checked against an independent model in test_select_host.py.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAYLOAD = ("x", "y", "desc", "desc_u8", "kpts", "orients")
DTYPE = dict(x=np.float32, y=np.float32, desc=np.float32, desc_u8=np.uint8, kpts=np.float32, orients=np.float32, index=np.int32)
TAIL = dict(x=(), y=(), desc=(128,), desc_u8=(128,), kpts=(4,), orients=(2,), index=())
SENTINEL = 77


def make_frame(seed, cap, width, height, levels=None, one_cell=0):
    """Random rows: coordinates over (and a little beyond) the frame, scores random or quantised to `levels` values, the
    first `one_cell` rows inside pixel block [0, 8) x [0, 8)."""
    rng = np.random.default_rng(seed)
    f = dict(x=(rng.random(cap) * (width + 6) - 3).astype(np.float32), y=(rng.random(cap) * (height + 6) - 3).astype(np.float32))
    f["x"][:one_cell] = rng.random(one_cell).astype(np.float32) * 7
    f["y"][:one_cell] = rng.random(one_cell).astype(np.float32) * 7
    s = rng.random(cap).astype(np.float32) if levels is None else rng.integers(0, levels, cap).astype(np.float32)
    f["scores"] = s
    f["desc"] = rng.integers(0, 40, (cap, 128)).astype(np.float32) * np.float32(0.37)
    f["desc_u8"] = rng.integers(0, 256, (cap, 128)).astype(np.uint8)
    f["kpts"] = rng.random((cap, 4)).astype(np.float32)
    f["orients"] = rng.random((cap, 2)).astype(np.float32)
    return f


def run_both(nm, cuda, frames, counts, cap, width, height, gx, gy, keep, use=PAYLOAD, scores=True, index=True, n_check=None):
    """One device call on sentinel-filled outputs and one host-twin call; asserts equality of every output byte (rows beyond
    the count: the sentinel). Returns the host result."""
    import torch
    n = len(frames)
    col = lambda name: [f[name][:cap] for f in frames]
    kw = {("descs" if k == "desc" else "descs_u8" if k == "desc_u8" else k): col(k) for k in use if k not in ("x", "y")}
    sc = col("scores") if scores else None
    host = nm.sift_select_host(counts, col("x"), col("y"), width, height, scores=sc, gx=gx, gy=gy, keep=keep, capacity=cap,
                               fill=SENTINEL, **kw)
    dev = lambda arrs: None if arrs is None else [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrs]
    out = {k: ([torch.full((cap,) + TAIL[k], SENTINEL, dtype=getattr(torch, np.dtype(DTYPE[k]).name), device=cuda)
                for _ in range(n)] if k in use else None) for k in PAYLOAD}
    out["index"] = [torch.full((cap,), SENTINEL, dtype=torch.int32, device=cuda) for _ in range(n)] if index else None
    out["count"] = torch.full((n,), SENTINEL, dtype=torch.int32, device=cuda)
    d_counts = [torch.tensor([c], dtype=torch.int32, device=cuda) for c in counts]
    got = nm.sift_select_batch_dev(d_counts, dev(col("x")), dev(col("y")), width, height, scores=dev(sc), gx=gx, gy=gy, keep=keep,
                                   capacity=cap, out=out, **{k: dev(v) for k, v in kw.items()})
    torch.cuda.synchronize()
    assert got is out
    want_count = [min(keep, min(max(c, 0), cap)) for c in counts]
    assert got["count"].cpu().numpy().tolist() == want_count == host["count"].tolist()
    for k in list(PAYLOAD) + ["index"]:
        if got[k] is None:
            assert k not in use
            continue
        for j in range(n):
            g = got[k][j].cpu().numpy()
            assert np.array_equal(g.view(np.uint8), host[k][j].view(np.uint8)), (k, j, counts[j])
            assert (g[want_count[j]:] == SENTINEL).all(), (k, j, "rows beyond the count")
    return host


RAGGED = (0, 1, 63, 64, 65, 255, 256, 257, 1025, 1100, 1107, -1)


@pytest.mark.parametrize("by_scores", [True, False])
@pytest.mark.parametrize("n", [1, 5, 64])
def test_device_equals_host_twin_on_ragged_batches(nm, cuda, n, by_scores):
    cap = 1100
    frames = [make_frame(100 + k, cap, 301, 200, levels=8 if k % 3 == 1 else None) for k in range(n)]
    counts = [RAGGED[(k + 8 * (n == 1)) % len(RAGGED)] for k in range(n)]
    host = run_both(nm, cuda, frames, counts, cap, 301, 200, 7, 5, 300, scores=by_scores)
    if n == 5:
        assert sorted(host["count"].tolist()) == [0, 1, 63, 64, 65]


def test_a_cell_longer_than_a_tile_and_one_cell_grids(nm, cuda):
    cap = 4608
    f = make_frame(7, cap, 640, 480, one_cell=4097)
    f["x"][4097:] = 600.0                                            # the rest: the other cell of a 2 x 1 grid
    for gx, count, keep in ((2, 4500, 2000), (2, 4500, 4400), (1, cap + 7, 2048), (1, 4097, 4096)):
        run_both(nm, cuda, [f], [count], cap, 640, 480, gx, 1, keep, use=("x", "y", "desc_u8"))


def test_sparse_grid_equal_scores_and_extreme_keeps(nm, cuda):
    cap = 300
    sparse = make_frame(11, cap, 1920, 1080)
    for keep in (1, 10, 39, 40, 300):
        run_both(nm, cuda, [sparse], [40], cap, 1920, 1080, 64, 64, keep, use=("x", "y", "kpts"))
    equal = make_frame(12, cap, 320, 240)
    equal["scores"][:] = 2.5
    for keep, count in ((1, 300), (299, 300), (128, 257), (256, 257)):
        run_both(nm, cuda, [equal, sparse], [count, count - 1], cap, 320, 240, 5, 3, keep)
    odd = make_frame(13, cap, 320, 240)
    odd["scores"][::7] = np.nan
    odd["scores"][1::7] = -1.0
    odd["scores"][2::7] = np.inf
    odd["x"][::5] = np.nan
    odd["y"][3::5] = 1e30
    odd["x"][4::5] = -1e30
    run_both(nm, cuda, [odd], [300], cap, 320, 240, 16, 9, 100)


@pytest.mark.parametrize("n", [1, 3])
def test_gather_ranks_through_a_second_chunk_that_ends_inside_a_wave(nm, cuda, n):
    """256 + 65 rows, half of them kept: the gather's ordered rank over the flags takes a second chunk of 256 rows whose second
    wave holds one row, with the chunk base carried over from the first."""
    cap = 256 + 65
    frames = [make_frame(60 + k, cap, 301, 200) for k in range(n)]
    host = run_both(nm, cuda, frames, [cap] * n, cap, 301, 200, 7, 5, cap // 2)
    assert all(host["index"][k][:cap // 2].max() >= 256 + 64 - 40 for k in range(n)), "the selection ends in the first chunk"


def test_group_scan_over_more_than_1024_occupied_cells(nm, cuda):
    """One row in each of 1100 cells of a 64 x 64 grid (four cells per thread: 275 threads, five waves): every segment start
    of the group kernel's scan depends on the totals of the waves before it."""
    cap, side = 1100, 640
    f = make_frame(61, cap, side, side)
    cells = np.random.default_rng(62).permutation(cap)
    f["x"] = ((cells % 64) * 10 + 5).astype(np.float32)
    f["y"] = ((cells // 64) * 10 + 5).astype(np.float32)
    for keep in (600, cap):
        run_both(nm, cuda, [f], [cap], cap, side, side, 64, 64, keep, use=("x", "y", "kpts"))


def test_every_subset_of_the_payload(nm, cuda):
    cap = 200
    frames = [make_frame(20 + k, cap, 160, 120) for k in range(2)]
    optional = ("desc", "desc_u8", "kpts", "orients")
    for r in range(len(optional) + 1):
        for sub in itertools.combinations(optional, r):
            for index in (True, False):
                run_both(nm, cuda, frames, [200, 131], cap, 160, 120, 4, 4, 50, use=("x", "y") + sub, index=index)
    run_both(nm, cuda, frames, [200, 131], cap, 160, 120, 4, 4, 50, use=("x", "y", "desc"), scores=False)


def test_a_frame_is_the_same_alone_and_in_any_slot(nm, cuda):
    cap = 400
    frames = [make_frame(40 + k, cap, 301, 200, levels=4 if k % 2 else None) for k in range(64)]
    counts = [cap - 3 * k for k in range(64)]
    batch = run_both(nm, cuda, frames, counts, cap, 301, 200, 16, 9, 120, use=("x", "y", "kpts"))
    for k in (0, 17, 63):
        for slot in (0, 5):
            group = [frames[(k + 9) % 64]] * slot + [frames[k]]
            alone = run_both(nm, cuda, group, [7] * slot + [counts[k]], cap, 301, 200, 16, 9, 120, use=("x", "y", "kpts"))
            for key in ("x", "y", "kpts", "index"):
                assert np.array_equal(alone[key][slot].view(np.uint8), batch[key][k].view(np.uint8)), (k, slot, key)


def test_refusals_touch_nothing(nm, cuda):
    import torch
    lib = nm.lib()
    cap = 16
    t = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device=cuda)
    f32, u8, i32 = torch.float32, torch.uint8, torch.int32
    src = dict(num=t((1,), i32, cap), x=t((cap,), f32, 1.0), y=t((cap,), f32, 1.0), scores=t((cap,), f32, 1.0),
               desc=t((cap, 128), f32, 1.0), desc_u8=t((cap, 128), u8, 1), kpts=t((cap, 4), f32, 1.0), orients=t((cap, 2), f32, 1.0))
    dst = dict(out_x=t((cap,), f32, 7.0), out_y=t((cap,), f32, 7.0), out_desc=t((cap, 128), f32, 7.0),
               out_desc_u8=t((cap, 128), u8, 7), out_kpts=t((cap, 4), f32, 7.0), out_orients=t((cap, 2), f32, 7.0),
               out_index=t((cap,), i32, 7), out_items=t((1,), i32, 7))
    ws = nm.SelectWorkspace(2, cap, 4, 4, cuda)
    tab = lambda tensor, k=2: (C.c_void_p * 64)(*([tensor.data_ptr()] * k))
    st = torch.cuda.current_stream().cuda_stream
    order = ("num", "x", "y", "scores", "desc", "desc_u8", "kpts", "orients", "out_x", "out_y", "out_desc", "out_desc_u8",
             "out_kpts", "out_orients", "out_index", "out_items")

    def call(n=2, cap_=cap, w=64, h=48, gx=4, gy=4, keep=8, workspace=ws.buf.data_ptr(), **kw):
        a = {k: tab(src[k] if k in src else dst[k]) for k in order}
        a.update(kw)
        return lib.nm_sift_select_batch_dev(n, cap_, w, h, gx, gy, keep, *[a[k] for k in order], workspace, st)

    bad = [dict(n=0), dict(n=65), dict(cap_=0), dict(cap_=65537), dict(gx=0), dict(gx=65), dict(gy=0), dict(gy=65), dict(keep=0),
           dict(keep=cap + 1), dict(w=0), dict(h=0), dict(workspace=None), dict(num=None), dict(x=None), dict(y=None),
           dict(out_x=None), dict(out_y=None), dict(out_items=None), dict(scores=None, desc=None, out_desc=None),
           dict(out_desc=None), dict(desc=None), dict(out_desc_u8=None), dict(desc_u8=None), dict(out_kpts=None), dict(kpts=None),
           dict(out_orients=None), dict(orients=None), dict(out_x=tab(src["x"])), dict(out_desc=tab(src["desc"])),
           dict(out_kpts=tab(src["kpts"]))]
    bad += [{k: tab(src[k] if k in src else dst[k], 1)} for k in order]
    for kw in bad:
        assert call(**kw) != 0, kw
    torch.cuda.synchronize()
    for v in dst.values():
        assert (v == 7).all()
    assert nm.lib().nm_sift_select_workspace_bytes(2, 65537, 4, 4) == 0 and nm.lib().nm_sift_select_workspace_bytes(65, 16, 4, 4) == 0
    assert call(scores=None) == 0 and call() == 0
    torch.cuda.synchronize()
    assert dst["out_items"].item() == 8 and dst["out_index"][:8].tolist() == list(range(8)) and (dst["out_index"][8:] == 7).all()
    for kw in (dict(keep=cap + 1), dict(gx=65), dict(scores=None), dict(kpts=[src["kpts"].cpu()])):
        args = dict(scores=[src["scores"]], gx=4, gy=4, keep=8)
        args.update(kw)
        with pytest.raises(nm.NmError):
            nm.sift_select_batch_dev([src["num"]], [src["x"]], [src["y"]], 64, 48, **args)


def test_real_descriptors_behind_the_frame_driver(nm, cuda):
    """A 640 x 480 blob field through detect_describe_batch, then the selection with the default score on the arena's own
    tensors, against the host twin on host copies."""
    import torch
    import helpers as H
    cap, keep = 4608, 32                                             # the frame has some 90 keypoints
    arena = nm.SiftArena(640, 480, cap, device=cuda)
    nm.detect_describe_batch([arena], [torch.from_numpy(H.blob_field(3, 640, 480).astype(np.float32)).to(cuda)])
    got = nm.sift_select_batch_dev([arena.num_items], [arena.x], [arena.y], 640, 480, descs=[arena.desc], kpts=[arena.kpts],
                                   orients=[arena.orients], gx=4, gy=3, keep=keep)
    torch.cuda.synchronize()
    m = int(arena.num_items.item())
    print("blob field: %d keypoints, %d kept" % (m, int(got["count"][0])))
    assert m > keep
    cpu = lambda t: t.cpu().numpy()
    host = nm.sift_select_host([m], [cpu(arena.x)], [cpu(arena.y)], 640, 480, descs=[cpu(arena.desc)], kpts=[cpu(arena.kpts)],
                               orients=[cpu(arena.orients)], gx=4, gy=3, keep=keep)
    assert int(got["count"][0]) == host["count"][0] == keep
    for k in ("index", "x", "y", "desc", "kpts", "orients"):
        assert np.array_equal(cpu(got[k][0])[:keep].view(np.uint8), host[k][0][:keep].view(np.uint8)), k
    idx = host["index"][0][:keep]
    assert idx.max() >= keep, "the selection is the capacity cut"


def test_chain_detect_select_finish_match_u8_mutual_u8_in_one_graph(nm, cuda):
    """detect -> select -> finish (u8) -> u8 match -> mutual u8 on two views of one scene, on one stream, captured into one
    HIP graph and replayed on the views of a second scene: every output equals the eager run's bit for bit."""
    import torch
    import test_gpu_mosaic as G
    cap, keep = 4608, 1024
    arenas = [nm.SiftArena(G.VW, G.VH, cap) for _ in range(2)]
    u8 = [torch.zeros((cap, 128), dtype=torch.uint8, device=cuda) for _ in range(2)]
    res = [torch.full((cap,), -1, dtype=torch.int32, device=cuda)]
    mres = [torch.full((cap,), -1, dtype=torch.int32, device=cuda)]
    sws = nm.SelectWorkspace(2, cap, 16, 9, cuda)
    uws = nm.MatchU8Workspace(1, cap, cap, cuda)
    mws = nm.MatchMutualU8Workspace(1, cap, cap, cuda)
    held = {}

    def enqueue(views):
        a, b = arenas
        nm.detect_describe_batch(arenas, [nm.grayscale(v) for v in views])
        sel = nm.sift_select_batch_dev([a.num_items, b.num_items], [a.x, b.x], [a.y, b.y], G.VW, G.VH, descs=[a.desc, b.desc],
                                       keep=keep, capacity=cap, out=held.get("sel"), workspace=sws)
        held["sel"] = sel
        nA, nB = sel["count"][0:1], sel["count"][1:2]
        nm.desc_finish_batch_dev(sel["desc"], [nA, nB], out_u8=u8, capacity=cap)
        nm.sift_match_u8_batch_dev([u8[0]], [nA], [u8[1]], [nB], results=res, ambiguity=0.8, workspace=uws, capA=cap, capB=cap)
        _, mcnt = nm.sift_match_mutual_u8_batch_dev([u8[0]], [nA], [u8[1]], [nB], res, capA=cap, capB=cap, results=mres,
                                                    workspace=mws)
        return (sel["count"], sel["index"][0], sel["index"][1], sel["x"][0], sel["y"][1], sel["desc"][0], u8[0], u8[1], res[0],
                mres[0], mcnt)

    def reset():
        res[0].fill_(-1)
        mres[0].fill_(-1)

    v1 = G._views(nm, cuda, G._scene(90))[:2]
    v2 = G._views(nm, cuda, G._scene(91))[:2]
    bufs = [v.clone() for v in v1]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        first = [o.cpu().numpy().copy() for o in enqueue(bufs)]        # warm-up outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        captured = enqueue(bufs)
    for b, v in zip(bufs, v2):
        b.copy_(v)
    reset()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    got = [o.cpu().numpy().copy() for o in captured]
    reset()
    with torch.cuda.stream(s):
        want = [o.cpu().numpy().copy() for o in enqueue([v.clone() for v in v2])]
    torch.cuda.synchronize()
    for k, (x, y) in enumerate(zip(got, want)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), k
    print("graph: selected", got[0].tolist(), "matches", int((got[8] >= 0).sum()), "mutual", int(got[10][0]))
    assert (got[0] > 0).all() and (got[0] <= keep).all() and not np.array_equal(first[1], got[1]), "the replay saw the first scene"
    assert int(got[10][0]) == (got[9] >= 0).sum() > 0
