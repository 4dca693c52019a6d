"""The mutual filter for u8 descriptors on the GPU (nm_sift_match_mutual_u8_batch_dev): array_equal on result, count and
forward_distance against its host twin AND against sift_match_mutual_batch_dev (the fp32 filter) on float copies of the same
bytes, over the cases of tests/mutual_u8_ref.py (sizes around the 32-row tile, the 64-claim wave, the 256-row workgroup and
the 8-way range split, claim counts 0 / 1 / 64 / 65 / all, tied rows across every merge, shared columns, 0 against 255,
clipped and empty sizes, ragged batches), slot independence, the two filters' shared claims stage on one two-workgroup batch
with guarded workspaces and the pinned workspace sizes, one 4096 x 4096 pair of finished real descriptors, and the
chain detect -> finish -> u8 match -> mutual u8 -> RANSAC captured into one HIP graph on a single stream and replayed on a
second view pair. No tolerance and no excluded rows anywhere.
"""
import numpy as np
import pytest

import mutual_u8_ref as M

pytestmark = pytest.mark.gpu

OUT = ("result", "count", "forward")


def _u32(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _upload(cases, dev, capA, capB):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return [dict(A=t(c["A"][:capA]), B=t(c["B"][:capB]), m=t(c["m"][:capA]), nA=t(np.array([c["nA"]], np.int32)),
                 nB=t(np.array([c["nB"]], np.int32))) for c in cases]


def _device(nm, cases, dev, capA, capB, floats=False):
    """One call of the u8 entry, or of the fp32 filter on float copies of the same bytes."""
    import torch
    up = _upload(cases, dev, capA, capB)
    k = lambda key: [u[key] for u in up]
    if floats:
        res, cnt, fwd = nm.sift_match_mutual_batch_dev([a.float() for a in k("A")], k("nA"), [b.float() for b in k("B")], k("nB"),
                                                       k("m"), capA=capA, capB=capB, want_distance=True)
    else:
        res, cnt, fwd = nm.sift_match_mutual_u8_batch_dev(k("A"), k("nA"), k("B"), k("nB"), k("m"), capA=capA, capB=capB,
                                                          want_distance=True)
    torch.cuda.synchronize()
    return dict(result=np.stack([r.cpu().numpy() for r in res]), count=cnt.cpu().numpy(),
                forward=np.stack([f.cpu().numpy() for f in fwd]))


def _host(nm, cases, capA, capB):
    k = lambda key: [c[key] for c in cases]
    return dict(zip(OUT, nm.sift_match_mutual_u8_host(k("A"), k("nA"), k("B"), k("nB"), k("m"), capA=capA, capB=capB,
                                                      want_distance=True)))


def _assert_all_equal(nm, dev, cases, capA, capB):
    got = _device(nm, cases, dev, capA, capB)
    host = _host(nm, cases, capA, capB)
    f32 = _device(nm, cases, dev, capA, capB, floats=True)
    for key in OUT:
        for i, c in enumerate(cases):
            assert np.array_equal(_u32(got[key][i]), _u32(host[key][i])), (c["what"], key, "host twin")
            assert np.array_equal(_u32(got[key][i]), _u32(f32[key][i])), (c["what"], key, "fp32 filter on float copies")
    assert np.array_equal((got["result"] >= 0).sum(axis=1), got["count"])
    return got


@pytest.mark.parametrize("family", ["size_cases", "claim_count_cases", "duplicate_cases", "shared_column_case", "extremes_case",
                                    "clip_cases"])
def test_cases_equal_host_twin_and_fp32_filter(nm, cuda, family):
    cases = getattr(M, family)()
    kept = 0
    for c in cases:
        got = _assert_all_equal(nm, cuda, [c], len(c["A"]), len(c["B"]))
        want = M.expected(c)
        assert np.array_equal(got["result"][0], want[0]) and got["count"][0] == want[1], c["what"]   # and the restatement itself
        assert np.array_equal(_u32(got["forward"][0]), _u32(want[2])), c["what"]
        kept += int(got["count"][0])
    assert kept == M.kept_removed(cases)[0]


@pytest.mark.parametrize("n", [1, 3, 16, 64])
def test_ragged_batches(nm, cuda, n):
    cases, capA, capB = M.ragged_batch(n)
    got = _assert_all_equal(nm, cuda, cases, capA, capB)
    empty = [i for i, c in enumerate(cases) if c["nA"] <= 0 or c["nB"] <= 0]
    assert len(empty) == 1 and (got["result"][empty[0]] == -1).all() and got["count"][empty[0]] == 0
    assert np.isposinf(got["forward"][empty[0]]).all()
    for i, c in enumerate(cases):
        assert (got["result"][i][min(max(c["nA"], 0), capA):] == -1).all(), "a row beyond nA is not -1"


def test_claims_rank_in_a_second_workgroup_that_ends_inside_a_wave(nm, cuda):
    """256 + 65 rows of A: the second workgroup of the claims stage ranks one full wave and one row of the next, behind the
    claims of the first workgroup; every row claiming, and the default mix. Both filters share the stage."""
    for c in (M.random_case(57, 256 + 65, 300, pad=0, claims=256 + 65), M.random_case(58, 256 + 65, 300, pad=0)):
        got = _assert_all_equal(nm, cuda, [c], len(c["A"]), len(c["B"]))
        assert 0 < got["count"][0] < M.claims_of(c)


def test_slot_independence(nm, cuda):
    """The same pair alone, twice, and at slot 11 of a batch of 16 other pairs: identical outputs."""
    a = M.random_case(55, 150, 140, pad=0)
    others, capA, capB = M.ragged_batch(16)
    alone = _device(nm, [a], cuda, capA, capB)
    again = _device(nm, [a], cuda, capA, capB)
    assert 0 < alone["count"][0] < M.claims_of(a)
    batch = list(others)
    batch[11] = a
    r = _device(nm, batch, cuda, capA, capB)
    for key in OUT:
        assert np.array_equal(_u32(alone[key][0]), _u32(again[key][0])), key
        assert np.array_equal(_u32(alone[key][0]), _u32(r[key][11])), key


# *_workspace_bytes by hand from the layouts: the fp32 filter 512 + n 3 ceil(capA / 64) 64 4, the u8 filter
# 256 + n (ceil(capA / 32) 32 + 4 ceil(capA / 64) 64) 4, the u8 matcher n (ceil(capA / 256) 256 + ceil(capB / 32) 32) 4
WORKSPACE_BYTES = {(1, 1, 1): (1280, 1408, 1152), (2, 257, 33): (8192, 12800, 4608), (64, 4096, 4096): (3146240, 5243136, 2097152)}


def test_shared_claims_stage_strides_and_claim_count(nm, cuda):
    """Both filters on the same bytes, n = 2, capA = 257 (two claims workgroups, the second with one row), nA = (257, 0),
    capB = 33, nB = (33, 1): pair 0 has claims on both sides of row 256, entries that are no claim, and rows 5 and 256 equal
    to column 7 and claiming it (a tie across the workgroups: row 5 keeps it); pair 1 takes the nA == 0 path. Each call
    equals its host twin and the other filter bit for bit, leaves m_k = (claims, 0) at the head of its workspace and a guard
    behind *_workspace_bytes untouched; the three *_workspace_bytes functions return the values worked out by hand."""
    import torch
    L = nm.lib()
    for (n, capA, capB), want in WORKSPACE_BYTES.items():
        got = (L.nm_sift_match_mutual_workspace_bytes(n, capA), L.nm_sift_match_mutual_u8_workspace_bytes(n, capA, capB),
               L.nm_sift_match_u8_workspace_bytes(n, capA, capB))
        assert got == want, (n, capA, capB)
    n, capA, capB, nA, nB = 2, 257, 33, (257, 0), (33, 1)
    rng = np.random.default_rng(257)
    A = [rng.integers(0, 256, (capA, 128), dtype=np.uint8) for _ in range(n)]
    B = [rng.integers(0, 256, (capB, 128), dtype=np.uint8) for _ in range(n)]
    A[0][5] = A[0][256] = B[0][7]
    m0 = rng.integers(0, capB, capA).astype(np.int32)
    m0[5] = m0[256] = 7
    m0[[0, 100, 255]] = (-1, capB, 1 << 20)                          # no claims: below 0, == nB, far outside
    m = [m0, np.zeros(capA, np.int32)]
    claims = int(((m0 >= 0) & (m0 < capB)).sum())
    assert 200 < claims == capA - 3

    dev = lambda arrays: [torch.from_numpy(a).to(cuda) for a in arrays]
    sizes = lambda ns: [torch.tensor([v], dtype=torch.int32, device=cuda) for v in ns]
    out = {}
    for name, cls, shape, call, host, conv in (
            ("u8", nm.MatchMutualU8Workspace, (n, capA, capB), nm.sift_match_mutual_u8_batch_dev, nm.sift_match_mutual_u8_host,
             lambda a: a),
            ("f32", nm.MatchMutualWorkspace, (n, capA), nm.sift_match_mutual_batch_dev, nm.sift_match_mutual_host,
             lambda a: a.astype(np.float32))):
        ws = cls(*shape, cuda)
        need = ws.buf.numel()
        assert need == WORKSPACE_BYTES[(n, capA, capB)][0 if name == "f32" else 1]
        guarded = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=cuda)
        ws.buf = guarded[:need]
        fA, fB = [conv(a) for a in A], [conv(b) for b in B]
        res, cnt, fwd = call(dev(fA), sizes(nA), dev(fB), sizes(nB), dev(m), capA=capA, capB=capB, workspace=ws,
                             want_distance=True)
        torch.cuda.synchronize()
        got = dict(result=np.stack([r.cpu().numpy() for r in res]), count=cnt.cpu().numpy(),
                   forward=np.stack([f.cpu().numpy() for f in fwd]))
        want = dict(zip(OUT, host(fA, nA, fB, nB, m, capA=capA, capB=capB, want_distance=True)))
        for key in OUT:
            assert np.array_equal(_u32(got[key]), _u32(want[key])), (name, key, "host twin")
        assert (guarded[need:] == 0xA5).all(), name + ": bytes behind the workspace were written"
        assert guarded[:8].view(torch.int32).tolist() == [claims, 0], name + ": m_k"
        out[name] = got
    for key in OUT:
        assert np.array_equal(_u32(out["u8"][key]), _u32(out["f32"][key])), (key, "the two filters")
    r = out["u8"]["result"]
    assert r[0][5] == 7 and r[0][256] == -1 and out["u8"]["forward"][0][256] == 0.0
    assert (r[1] == -1).all() and out["u8"]["count"][1] == 0 and np.isposinf(out["u8"]["forward"][1]).all()
    assert 0 < out["u8"]["count"][0] < claims


def test_finished_real_descriptors_4096(nm, cuda):
    """The lists sift_match_u8_batch_dev writes for one 4096 x 4096 pair of finished 1080p descriptors, filtered on the
    device, against the host twin."""
    import torch
    from test_gpu_match_u8 import _finished_1080p
    A, B = _finished_1080p(nm, cuda, (0, 1))
    tA, tB = torch.from_numpy(A).to(cuda), torch.from_numpy(B).to(cuda)
    n4096 = torch.tensor([4096], dtype=torch.int32, device=cuda)
    m = nm.sift_match_u8_batch_dev([tA], [n4096], [tB], [n4096], ambiguity=0.8)
    res, cnt, fwd = nm.sift_match_mutual_u8_batch_dev([tA], [n4096], [tB], [n4096], m, want_distance=True)
    torch.cuda.synchronize()
    mh = m[0].cpu().numpy()
    hres, hcnt, hfwd = nm.sift_match_mutual_u8_host([A], [4096], [B], [4096], [mh], want_distance=True)
    claims, kept = int((mh >= 0).sum()), int(cnt.item())
    print("4096 x 4096 finished descriptors: %d claims, %d kept" % (claims, kept))
    assert np.array_equal(res[0].cpu().numpy(), hres[0]) and kept == hcnt[0]
    assert np.array_equal(_u32(fwd[0].cpu().numpy()), _u32(hfwd[0]))
    assert 0 < kept < claims, "the filter kept everything or nothing"


def test_chain_detect_finish_match_u8_mutual_u8_ransac_in_one_graph(nm, cuda):
    """detect -> finish -> u8 match -> mutual u8 -> RANSAC on two views of one scene, on one stream, captured into one HIP
    graph and replayed on the views of a second scene with other keypoint counts: every output equals the eager run's bit
    for bit, and the recovered homography is within test_gpu_match_u8's tolerances of the true map."""
    import torch
    import test_gpu_mosaic as G
    cap, iterations = G.CAP, 2048
    arenas = [nm.SiftArena(G.VW, G.VH, cap) for _ in range(2)]
    u8 = [torch.zeros((cap, 128), dtype=torch.uint8, device=cuda) for _ in range(2)]
    res = [torch.full((cap,), -1, dtype=torch.int32, device=cuda)]
    mres = [torch.full((cap,), -1, dtype=torch.int32, device=cuda)]
    uws = nm.MatchU8Workspace(1, cap, cap, cuda)
    mws = nm.MatchMutualU8Workspace(1, cap, cap, cuda)
    rws = nm.RansacBatchWorkspace(1, cap, iterations, cuda)

    def enqueue(views):
        a, b = arenas
        nm.detect_describe_batch(arenas, [nm.grayscale(v) for v in views])
        nm.desc_finish_batch_dev([a.desc, b.desc], [a.num_items, b.num_items], out_u8=u8, capacity=cap)
        nm.sift_match_u8_batch_dev([u8[0]], [a.num_items], [u8[1]], [b.num_items], results=res, ambiguity=0.8, workspace=uws,
                                   capA=cap, capB=cap)
        _, mcnt = nm.sift_match_mutual_u8_batch_dev([u8[0]], [a.num_items], [u8[1]], [b.num_items], res, capA=cap, capB=cap,
                                                    results=mres, workspace=mws)
        Hb, best, pos, status = nm.ransac_batch_dev(2, [a.x], [a.y], [a.num_items], [b.x], [b.y], mres, iterations=iterations,
                                                    threshold=1.0, seeds=[3], capA=cap, workspace=rws)
        return Hb, best, pos, status, a.num_items, b.num_items, res[0], u8[0], u8[1], mres[0], mcnt

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
    res[0].fill_(-1)
    mres[0].fill_(-1)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    got = [o.cpu().numpy().copy() for o in captured]
    res[0].fill_(-1)
    mres[0].fill_(-1)
    with torch.cuda.stream(s):
        want = [o.cpu().numpy().copy() for o in enqueue([v.clone() for v in v2])]
    torch.cuda.synchronize()
    for x, y in zip(got, want):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    cnt = lambda o: (int(o[4].reshape(-1)[0]), int(o[5].reshape(-1)[0]))
    assert cnt(first) != cnt(got), "the second scene has the first one's counts"
    assert int(first[10][0]) != int(got[10][0]), "the second scene has the first one's mutual count"
    maps = G._view_maps()
    Ht = np.linalg.inv(maps[1]) @ maps[0]
    Ht /= Ht[2, 2]
    for out in (first, got):
        Hb, status, blind, kept, mcnt = out[0], out[3], out[6], out[9], out[10]
        assert int(status.reshape(-1)[0]) == 1 and 100 < int(mcnt[0]) == (kept >= 0).sum() <= (blind >= 0).sum()
        Hn = Hb.reshape(3, 3).astype(np.float64) / float(Hb.reshape(-1)[8])
        np.testing.assert_allclose(Hn, Ht, atol=0.6, rtol=0.05)
        np.testing.assert_allclose(Hn[:2, :2], Ht[:2, :2], atol=5e-3)
    # the replayed mutual matches equal the host twin on the bytes and the list the chain produced
    nA, nB = cnt(got)
    hres, hcnt = nm.sift_match_mutual_u8_host([got[7]], [nA], [got[8]], [nB], [got[6]])
    assert np.array_equal(hres[0], got[9]) and hcnt[0] == int(got[10][0])
    for a in arenas:
        a.close()
