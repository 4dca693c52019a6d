"""nm_sift_match_guided_u8_batch_dev on the MI355X: bit-identity with its host twin over batch sizes and mixed pairs whose
sizes sit on the wave, workgroup, chunk and LDS-tile edges, the per-lane hit lists under pressure (the gate-hit patterns of
tests/guided_hits_ref.py on byte descriptors), the largest distance there is, agreement with the fp32 device entry on float
copies of the bytes, sentinel-guarded outputs, slot independence, the alignment rule, and the byte chain detect -> finish ->
u8 match -> mutual u8 -> RANSAC -> refit -> guided u8 -> refit captured into one HIP graph. Equality is exact everywhere:
array_equal on results and counts and on the uint32 views of the best distances."""
import ctypes as C

import numpy as np
import pytest

import guided_hits_ref as GH
from test_match_guided_u8_host import byte_pair, extreme_pair

pytestmark = pytest.mark.gpu

CAPA, CAPB = 300, 1100
R2 = 6.0
OUT = ("result", "count", "best")
NA = (257, 0, 1, 63, 64, 65, 255, 256)                  # the wave (64) and workgroup (256) edges
NB = (1025, 0, 1, 7, 8, 9, 1023, 1024)                  # the chunk (8) and LDS tile (1 024) edges


def _u32(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _padded(p, capA=CAPA, capB=CAPB):
    """The pair's arrays at the call's capacities; the rows beyond the sizes hold plausible values that must not be read."""
    q = dict(p)
    for key, cap in (("A", capA), ("B", capB)):
        full = np.full((cap, 128), 1, np.uint8)
        full[:len(p[key])] = p[key]
        q[key] = full
    for key, cap in (("ax", capA), ("ay", capA), ("bx", capB), ("by", capB)):
        full = np.full(cap, 5.0, np.float32)
        full[:len(p[key])] = p[key]
        q[key] = full
    return q


def _mixed(n):
    """Pair k has NA[k % 8] x NB[(k + k // 8) % 8] rows (all 64 combinations at n = 64), bytes 0 .. 3 or 0 .. 255 in turn;
    from the third pair on the unusable kinds of the host test are mixed in."""
    pairs = []
    for k in range(n):
        ra, rb = NA[k % 8], NB[(k + k // 8) % 8]
        p = byte_pair(900 + k, max(ra, 1), max(rb, 1), 3 if k % 2 else 255, nA=ra, nB=rb, negative=(0,) if ra > 100 else ())
        pairs.append(_padded(p))
    if n >= 3:
        pairs[2]["status"] = 0
    if n >= 33:
        pairs[8]["status"] = 5
        pairs[16]["H"][4] = np.nan
        pairs[24]["H"][2] = np.inf
        pairs[32]["nA"], pairs[32]["nB"] = 10 ** 6, 10 ** 6                 # clipped to the capacities: the padding is live
        pairs[7]["nA"], pairs[7]["nB"] = -4, -1
        pairs[14]["H"] = np.array([1, 0, 0, 0, 1, 0, -1.0 / 16, 0, 1], np.float32)     # z = 0 on the line ax = 16
        pairs[14]["ax"][:20] = 16.0
        pairs[22]["H"] = np.array([1, 0, 0, 0, 1, 0, 0, 0, 0], np.float32)             # z = 0 everywhere
    return pairs


def _host(nm, pairs, radius2=R2, ambiguity=0.8, max_distance=np.inf, status=True, capA=CAPA, capB=CAPB):
    k = lambda key: [p[key] for p in pairs]
    out = nm.sift_match_guided_u8_host(k("A"), k("ax"), k("ay"), k("nA"), k("B"), k("bx"), k("by"), k("nB"), np.stack(k("H")),
                                       status=np.array(k("status"), np.int32) if status else None, radius2=radius2,
                                       ambiguity=ambiguity, max_distance=max_distance, capA=capA, capB=capB,
                                       want_distance=True)
    return dict(zip(OUT, out))


def _upload(pairs, dev, floats=False):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = (lambda a: t(a.astype(np.float32))) if floats else t
    return [dict(A=d(p["A"]), ax=t(p["ax"]), ay=t(p["ay"]), B=d(p["B"]), bx=t(p["bx"]), by=t(p["by"]),
                 nA=t(np.array([p["nA"]], np.int32)), nB=t(np.array([p["nB"]], np.int32))) for p in pairs]


def _device(nm, pairs, dev, radius2=R2, ambiguity=0.8, max_distance=np.inf, status=True, up=None, capA=CAPA, capB=CAPB,
            fp32=False):
    """The u8 device entry (fp32: the fp32 device entry, `up` then holds float descriptors)."""
    import torch
    up = _upload(pairs, dev, fp32) if up is None else up
    k = lambda key: [u[key] for u in up]
    Hd = torch.from_numpy(np.stack([p["H"] for p in pairs])).to(dev)
    st = torch.from_numpy(np.array([p["status"] for p in pairs], np.int32)).to(dev) if status else None
    fn = nm.sift_match_guided_batch_dev if fp32 else nm.sift_match_guided_u8_batch_dev
    res, cnt, best = fn(k("A"), k("ax"), k("ay"), k("nA"), k("B"), k("bx"), k("by"), k("nB"), Hd, status=st, radius2=radius2,
                        ambiguity=ambiguity, max_distance=max_distance, capA=capA, capB=capB, want_distance=True)
    torch.cuda.synchronize()
    return dict(result=np.stack([r.cpu().numpy() for r in res]), count=cnt.cpu().numpy(),
                best=np.stack([b.cpu().numpy() for b in best]))


def _assert_same(a, b, what):
    for k in OUT:
        assert np.array_equal(_u32(a[k]), _u32(b[k])), (what, k)


RUNS = (dict(), dict(radius2=30.0, ambiguity=0.95), dict(radius2=0.5, max_distance=4e5), dict(radius2=1e12))


@pytest.mark.parametrize("n", [1, 3, 33, 64])
def test_device_equals_host_twin(nm, cuda, n):
    pairs = _mixed(n)
    up = _upload(pairs, cuda)
    matched = 0
    for kw in RUNS:
        want = _host(nm, pairs, **kw)
        got = _device(nm, pairs, cuda, up=up, **kw)
        _assert_same(got, want, "n %d %r" % (n, kw))
        assert np.array_equal((got["result"] >= 0).sum(axis=1), got["count"])
        matched += int(got["count"].sum())
    assert matched > 0, "nothing matched: the comparison covered nothing"
    # status_in = NULL means every pair is usable
    _assert_same(_device(nm, pairs, cuda, up=up, status=False), _host(nm, pairs, status=False), "status NULL")


@pytest.mark.parametrize("nB", [9, 37])
def test_a_gate_that_passes_everything_flushes_every_four_candidates(nm, cuda, nB):
    pairs = [_padded(byte_pair(70 + nB + top, 70, nB, top), 70, nB) for top in (3, 255)]
    for amb in (0.8, 0.95):
        kw = dict(radius2=1e30, ambiguity=amb, capA=70, capB=nB)
        want = _host(nm, pairs, **kw)
        _assert_same(_device(nm, pairs, cuda, **kw), want, "open gate nB %d" % nB)
        for k, p in enumerate(pairs):
            blind = nm.sift_match_u8_host([p["A"]], [70], [p["B"]], [nB], ambiguity=amb, prior=-1)
            assert np.array_equal(want["result"][k], blind[0])
    assert want["count"].sum() > 0


def _byte_case(c):
    """A case of guided_hits_ref on byte descriptors: its rows are small integers in [0, 255] held in float32."""
    q = dict(c)
    for key in ("A", "B"):
        assert c[key].min() >= 0 and c[key].max() <= 255 and np.array_equal(c[key], np.rint(c[key]))
        q[key] = c[key].astype(np.uint8)
    return q


@pytest.mark.parametrize("family", GH.FAMILIES)
def test_hit_patterns_on_byte_descriptors(nm, cuda, family):
    """The generators of tests/guided_hits_ref.py: lanes of one wave holding 0, 1, 2, 3, 4, 5, 7, 8 and 9 hits, hits in every
    position of a chunk with rounds inside the chunk, hits on both sides of the 1 024 tile boundary, ragged row counts.
    Against the host twin and against that module's integer restatement."""
    cases = GH.family_cases(family)
    if family == "hit_counts":
        assert {len(js) for c in cases for js in c["hits"].values()} >= {1, 4, 5, 9} and any(64 > len(c["hits"]) for c in cases)
    if family == "tile_edge":
        assert any(1023 in js and 1024 in js for c in cases for js in c["hits"].values())
    pairs = [_byte_case(c) for c in cases]
    up = _upload(pairs, cuda)
    hit_rows = 0
    for run in sorted({r for c in cases for r in c["runs"]}):
        sel = [k for k, c in enumerate(cases) if run in c["runs"]]
        kw = dict(radius2=run[0], ambiguity=run[1], max_distance=run[2], capA=GH.CAP_A, capB=GH.CAP_B)
        sub = [pairs[k] for k in sel]
        want = _host(nm, sub, **kw)
        got = _device(nm, sub, cuda, up=[up[k] for k in sel], **kw)
        _assert_same(got, want, (family, run))
        for s, k in enumerate(sel):
            res, cnt, best = GH.restate(cases[k], *run)
            assert np.array_equal(got["result"][s], res) and got["count"][s] == cnt, (cases[k]["what"], run)
            assert np.array_equal(_u32(got["best"][s]), _u32(best)), (cases[k]["what"], run)
            hit_rows += int(np.isfinite(best).sum())
    assert hit_rows > 0


def test_extremes_on_the_device(nm, cuda):
    p, want, wbest = extreme_pair()
    capA, capB = len(p["A"]), len(p["B"])
    got = _device(nm, [p], cuda, radius2=9.0, capA=capA, capB=capB)
    _assert_same(got, _host(nm, [p], radius2=9.0, capA=capA, capB=capB), "extremes")
    assert np.array_equal(got["result"][0], want) and np.array_equal(_u32(got["best"][0]), _u32(wbest))
    assert got["best"][0][0] == 8323200.0 and got["count"][0] == (want >= 0).sum()
    kw = dict(radius2=1e30, capA=capA, capB=capB)
    _assert_same(_device(nm, [p], cuda, **kw), _host(nm, [p], **kw), "extremes, open gate")


def test_agreement_with_the_fp32_device_entry_on_float_copies(nm, cuda):
    pairs = _mixed(64)[:16]
    up8, up32 = _upload(pairs, cuda), _upload(pairs, cuda, floats=True)
    matched = 0
    for kw in RUNS[:3]:
        got = _device(nm, pairs, cuda, up=up8, **kw)
        _assert_same(got, _device(nm, pairs, cuda, up=up32, fp32=True, **kw), "fp32 device entry %r" % (kw,))
        matched += int(got["count"].sum())
    assert matched > 0


@pytest.mark.parametrize("n", [5, 37])
def test_outputs_are_written_inside_their_bounds(nm, cuda, n):
    """result and best_distance of every pair and the counts lie in guarded buffers: capA rows per pair (capA above every
    nA: -1 / +inf from nA on) and n counts are written, nothing around them."""
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
    rc = nm.lib().nm_sift_match_guided_u8_batch_dev(n, tab("A"), tab("ax"), tab("ay"), tab("nA"), CAPA, tab("B"), tab("bx"),
                                                    tab("by"), tab("nB"), CAPB, Hd.data_ptr(), st.data_ptr(), R2, 0.8,
                                                    float("inf"), arr([r[Gd:].data_ptr() for r in res]),
                                                    count[Gd:].data_ptr(), arr([b[Gd:].data_ptr() for b in best]),
                                                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    for b in res + best + [count]:
        assert (b[:Gd] == -7).all() and (b[-Gd:] == -7).all()
    want = _host(nm, pairs)
    got_res = np.stack([r[Gd:-Gd].cpu().numpy() for r in res])
    got_best = np.stack([b[Gd:-Gd].cpu().numpy() for b in best])
    assert np.array_equal(got_res, want["result"]) and np.array_equal(_u32(got_best), _u32(want["best"]))
    assert np.array_equal(count[Gd:-Gd].cpu().numpy(), want["count"])
    for k, p in enumerate(pairs):
        nA = min(max(p["nA"], 0), CAPA)
        assert nA < CAPA or p["nA"] > CAPA
        assert (got_res[k][nA:] == -1).all() and np.isposinf(got_best[k][nA:]).all()


def test_slot_independence(nm, cuda):
    a, b = _padded(byte_pair(5, 290, 1030, 255, negative=(3,))), _padded(byte_pair(6, 200, 1100, 3))
    alone, other = _device(nm, [a], cuda), _device(nm, [b], cuda)
    assert alone["count"][0] > 20 and other["count"][0] > 20
    for n, slot in ((64, 0), (64, 31), (64, 32), (64, 63), (33, 32)):
        pairs = [b] * n
        pairs[slot] = a
        r = _device(nm, pairs, cuda)
        for k in OUT:
            assert np.array_equal(_u32(r[k][slot]), _u32(alone[k][0])), (n, slot, k)
            assert np.array_equal(_u32(r[k][(slot + 1) % n]), _u32(other[k][0])), (n, slot, k)


def test_a_descriptor_pointer_off_by_four_bytes_is_refused(nm, cuda):
    import torch
    p = _padded(byte_pair(7, 64, 64, 255), 64, 64)
    up = _upload([p, p], cuda)
    off = []
    for key in ("A", "B"):
        big = torch.zeros(64 * 128 + 16, dtype=torch.uint8, device=cuda)
        view = big[4:4 + 64 * 128].view(64, 128)
        view.copy_(up[0][key])
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        off.append(view)
    Hd = torch.from_numpy(np.stack([p["H"], p["H"]])).to(cuda)
    res = [torch.full((64,), -7, dtype=torch.int32, device=cuda) for _ in range(2)]
    best = [torch.full((64,), -7.0, dtype=torch.float32, device=cuda) for _ in range(2)]
    count = torch.full((2,), -7, dtype=torch.int32, device=cuda)
    arr = lambda ptrs: (C.c_void_p * 2)(*ptrs)
    tab = lambda key: arr([u[key].data_ptr() for u in up])

    def call(A, B):
        rc = nm.lib().nm_sift_match_guided_u8_batch_dev(2, A, tab("ax"), tab("ay"), tab("nA"), 64, B, tab("bx"), tab("by"),
                                                        tab("nB"), 64, Hd.data_ptr(), None, R2, 0.8, float("inf"),
                                                        arr([r.data_ptr() for r in res]), count.data_ptr(),
                                                        arr([b.data_ptr() for b in best]),
                                                        torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    invalid = 1                                                # hipErrorInvalidValue
    assert call(arr([up[0]["A"].data_ptr(), off[0].data_ptr()]), tab("B")) == invalid      # the second pair's A
    assert call(tab("A"), arr([off[1].data_ptr(), up[1]["B"].data_ptr()])) == invalid      # the first pair's B
    for t in res + best + [count]:
        assert (t == -7).all()
    with pytest.raises(nm.NmError, match="invalid"):
        nm.sift_match_guided_u8_batch_dev([off[0]], [up[0]["ax"]], [up[0]["ay"]], [up[0]["nA"]], [up[0]["B"]], [up[0]["bx"]],
                                          [up[0]["by"]], [up[0]["nB"]], Hd[:1], results=res[:1])
    torch.cuda.synchronize()
    assert (res[0] == -7).all()
    assert call(tab("A"), tab("B")) == 0 and int(count[0]) > 0 and (res[0] != -7).all()     # aligned: the same call runs


def test_byte_chain_with_guided_u8_in_one_graph_replays_on_another_scene(nm, cuda):
    """detect -> finish -> u8 match -> mutual u8 -> RANSAC -> refit -> guided u8 -> refit on the eight synthetic views of
    test_gpu_mosaic (7 links), captured into one HIP graph on a single stream and replayed on a second scene: every output
    equals the eager chain's on that scene bit for bit."""
    import torch
    import test_gpu_mosaic as M
    cap, iterations = M.CAP, 2048
    arenas = [nm.SiftArena(M.VW, M.VH, cap) for _ in range(8)]
    u8 = [torch.zeros((cap, 128), dtype=torch.uint8, device=cuda) for _ in range(8)]
    res, mres, gres = ([torch.full((cap,), -1, dtype=torch.int32, device=cuda) for _ in range(7)] for _ in range(3))
    uws = nm.MatchU8Workspace(7, cap, cap, cuda)
    mws = nm.MatchMutualU8Workspace(7, cap, cap, cuda)
    rws = nm.RansacBatchWorkspace(7, cap, iterations, cuda)

    def enqueue(views):
        A, B = arenas[:-1], arenas[1:]
        nm.detect_describe_batch(arenas, [nm.grayscale(v) for v in views])
        nm.desc_finish_batch_dev([a.desc for a in arenas], [a.num_items for a in arenas], out_u8=u8, capacity=cap)
        nA, nB = [a.num_items for a in A], [b.num_items for b in B]
        nm.sift_match_u8_batch_dev(u8[:-1], nA, u8[1:], nB, results=res, ambiguity=0.8, workspace=uws, capA=cap, capB=cap)
        _, mcnt = nm.sift_match_mutual_u8_batch_dev(u8[:-1], nA, u8[1:], nB, res, capA=cap, capB=cap, results=mres,
                                                    workspace=mws)
        pts = ([a.x for a in A], [a.y for a in A], nA, [b.x for b in B], [b.y for b in B])
        Hb, best, pos, status = nm.ransac_batch_dev(2, *pts, mres, iterations=iterations, threshold=1.0,
                                                    seeds=list(range(7)), capA=cap, workspace=rws)
        Hr, cnt, st, done = nm.ransac_refit_batch_dev(2, *pts, mres, Hb, status=status, rounds=2, threshold=1.0, capA=cap)
        _, gcnt, gbest = nm.sift_match_guided_u8_batch_dev(u8[:-1], pts[0], pts[1], nA, u8[1:], pts[3], pts[4], nB, Hr,
                                                           status=st, radius2=9.0, capA=cap, capB=cap, results=gres,
                                                           want_distance=True)
        Hg, cnt2, st2, done2 = nm.ransac_refit_batch_dev(2, *pts, gres, Hr, status=st, rounds=2, threshold=1.0, capA=cap)
        return (Hb, best, status, Hr, cnt, st, mcnt, gcnt, Hg, cnt2, st2, done2) + tuple(gres) + tuple(gbest) + tuple(mres) + \
            tuple(a.num_items for a in arenas)

    def reset():
        for r in res + mres + gres:
            r.fill_(-1)

    v1 = M._views(nm, cuda, M._scene(90))
    v2 = M._views(nm, cuda, M._scene(91))
    bufs = [v.clone() for v in v1]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        first = [o.cpu().numpy().copy() for o in enqueue(bufs)]          # warm-up outside capture
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
    bytes_a, bytes_b = u8[0].cpu().numpy(), u8[1].cpu().numpy()
    reset()
    with torch.cuda.stream(s):
        want = [o.cpu().numpy().copy() for o in enqueue([v.clone() for v in v2])]
    torch.cuda.synchronize()
    for x, y in zip(got, want):
        assert np.array_equal(_u32(x), _u32(y))
    assert any(not np.array_equal(x, y) for x, y in zip(first[-8:], got[-8:])), "the second scene has the first one's counts"
    Hb, best, status, Hr, cnt, st, mcnt, gcnt, Hg, cnt2, st2, done2 = got[:12]
    assert (status == 1).all() and (st == 1).all() and (st2 == 1).all() and np.isfinite(Hg).all()
    assert (gcnt > mcnt).all() and (mcnt > 100).all(), (gcnt, mcnt)      # more correspondences than the filtered blind list
    assert np.array_equal(gcnt, [(r >= 0).sum() for r in got[12:19]])
    # link 0 of the replay against the host twin on the bytes and the map the chain produced
    nA, nB = int(got[-8][0]), int(got[-7][0])
    a, b = arenas[0], arenas[1]
    hres, hcnt, hbest = nm.sift_match_guided_u8_host([bytes_a], [a.x.cpu().numpy()], [a.y.cpu().numpy()], [nA], [bytes_b],
                                                     [b.x.cpu().numpy()], [b.y.cpu().numpy()], [nB], Hr[:1], status=st[:1],
                                                     radius2=9.0, capA=cap, capB=cap, want_distance=True)
    assert np.array_equal(hres[0], got[12]) and hcnt[0] == gcnt[0] and np.array_equal(_u32(hbest[0]), _u32(got[19]))
    for ar in arenas:
        ar.close()
