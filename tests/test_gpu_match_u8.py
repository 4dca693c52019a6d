"""The u8 matcher on the GPU (nm_sift_match_u8_batch_dev): array_equal on the result lists against its host twin AND
against sift_match_batch_dev (the fp32 matcher) on float copies of the same bytes, over the cases of
tests/match_u8_ref.py (mixed sizes around the 32-candidate tile and the 64-query wave, ragged batches with an empty
pair, asymmetric bytes, 0 against 255, duplicates across every merge, min2 == 0, one candidate, ambiguity 0.8 and 1.0),
one 4096 x 4096 pair of finished real descriptors, and the chain detect -> finish -> u8 match -> RANSAC captured into one
HIP graph on a single stream and replayed on a second view pair.
"""
import numpy as np
import pytest

import match_u8_ref as M

pytestmark = pytest.mark.gpu


def _run(nm, dev, cases, capA, capB, amb):
    """One u8 call and the fp32 matcher on float copies (16 pairs a call), both on pre-filled results. Returns two lists."""
    import torch
    n = len(cases)
    up = lambda a, cap: torch.from_numpy(np.ascontiguousarray(a[:cap])).to(dev)
    A, B = [up(c["A"], capA) for c in cases], [up(c["B"], capB) for c in cases]
    nA = [torch.tensor([c["nA"]], dtype=torch.int32, device=dev) for c in cases]
    nB = [torch.tensor([c["nB"]], dtype=torch.int32, device=dev) for c in cases]
    pre = lambda: [torch.full((capA,), c["prior"], dtype=torch.int32, device=dev) for c in cases]
    got, ref = pre(), pre()
    nm.sift_match_u8_batch_dev(A, nA, B, nB, results=got, ambiguity=amb, capA=capA, capB=capB)
    Af, Bf = [a.float() for a in A], [b.float() for b in B]
    for c0 in range(0, n, nm.MATCH_MAX_BATCH):
        s = slice(c0, c0 + nm.MATCH_MAX_BATCH)
        nm.sift_match_batch_dev(Af[s], nA[s], Bf[s], nB[s], ref[s], amb, capA=capA, capB=capB)
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in got], [r.cpu().numpy() for r in ref]


def _assert_all_equal(nm, dev, cases, capA, capB, amb):
    got, ref = _run(nm, dev, cases, capA, capB, amb)
    k = lambda key: [c[key] for c in cases]
    host = nm.sift_match_u8_host(k("A"), k("nA"), k("B"), k("nB"), ambiguity=amb, capA=capA, capB=capB, prior=cases[0]["prior"])
    for i, c in enumerate(cases):
        d = np.flatnonzero(got[i] != host[i])
        assert not len(d), (c["what"], "host twin", d[:5], got[i][d[:5]], host[i][d[:5]])
        d = np.flatnonzero(got[i] != ref[i])
        assert not len(d), (c["what"], "fp32 matcher on float copies", d[:5], got[i][d[:5]], ref[i][d[:5]])
    return got


def test_cases_equal_host_twin_and_fp32_matcher(nm, cuda):
    matched = 0
    for c in M.all_cases():
        got = _assert_all_equal(nm, cuda, [c], len(c["A"]), len(c["B"]), c["amb"])
        assert np.array_equal(got[0], M.expected(c, len(c["A"]))), c["what"]      # and the restatement itself
        matched += int((got[0] >= 0).sum())
    assert matched > 150


@pytest.mark.parametrize("n", [1, 3, 16, 64])
def test_ragged_batches(nm, cuda, n):
    cases, capA, capB = M.ragged_batch(n)
    for amb in (0.8, 1.0):
        got = _assert_all_equal(nm, cuda, cases, capA, capB, amb)
    empty = [i for i, c in enumerate(cases) if c["nA"] <= 0 or c["nB"] <= 0]
    assert len(empty) == 1 and (got[empty[0]] == -7).all()
    for i, c in enumerate(cases):
        assert (got[i][min(max(c["nA"], 0), capA):] == -7).all(), "a row beyond nA was written"


@pytest.mark.parametrize("amb", [0.8, 1.0])
def test_shared_scan_cases_and_ratio_rule_on_device_k2_lists(nm, cuda, amb):
    """M.shared_scan_cases() (one candidate, two identical candidates, one row into the second tile, one row past a wave and
    past a workgroup, ties across the lane halves and the tile boundary), each alone and as a 3-pair batch with the empty
    pair: host twin, fp32 matcher, restatement, and the ratio rule applied to the device's own k = 2 lists."""
    import torch
    import knn_u8_ref as K
    cases, capA, capB = M.shared_scan_cases()
    one, same, empty, ties = cases
    for batch in [[one], [same], [ties], [same, empty, ties]]:
        got = _assert_all_equal(nm, cuda, batch, capA, capB, amb)
        up = lambda a: torch.from_numpy(a).to(cuda)
        size = lambda v: torch.tensor([v], dtype=torch.int32, device=cuda)
        idx, dist = nm.sift_match_knn_u8_batch_dev([up(c["A"]) for c in batch], [size(c["nA"]) for c in batch],
                                                   [up(c["B"]) for c in batch], [size(c["nB"]) for c in batch], 2,
                                                   capA=capA, capB=capB)
        torch.cuda.synchronize()
        for p, c in enumerate(batch):
            assert np.array_equal(got[p], M.expected_clipped(dict(c, amb=amb), capA, capB)), c["what"]
            lists = K.matcher_from_lists(c, idx[p].cpu().numpy(), dist[p].cpu().numpy(), amb, capA, capB)
            assert np.array_equal(got[p], lists), (c["what"], "ratio rule on the device k = 2 lists")
            assert (got[p][max(c["nA"], 0):] == -7).all(), "a row beyond nA was written"
    assert (got[0][:32] == -7).all() and (got[0][32:65] == -1).all()          # min2 == 0 kept, min2 == min1 rejected
    assert (got[1] == -7).all()                                               # the empty pair
    above = _assert_all_equal(nm, cuda, [ties], capA, capB, 1.5)[0]           # only an ambiguity above 1 shows a tie's index
    assert above[10] == 1 and above[11] == 0, "the lower index wins a tie"


def _finished_1080p(nm, dev, seeds, want_rows=4096):
    """uint8 descriptors of synthetic 1080p frames: detect, describe and finish on the device."""
    import torch
    from niftymatch_amd import synth
    W, Hh, cap = 1920, 1080, 16384
    taps, r = nm.create_kernel_for_sigma(synth.preblur_sigma(W, Hh))
    taps_d = torch.from_numpy(taps).to(dev)
    base = nm.convolve(synth.noise_frame_torch(seeds[0], W, Hh, dev), taps_d, r)
    other = nm.convolve(synth.noise_frame_torch(seeds[1], W, Hh, dev), taps_d, r)
    frames = [base, (0.75 * torch.roll(base, (5, 9), (0, 1)) + 0.25 * other).contiguous()]
    arenas = [nm.SiftArena(W, Hh, cap, device=dev) for _ in range(2)]
    nm.detect_describe_batch(arenas, frames)
    _, u8 = nm.desc_finish_batch_dev([a.desc for a in arenas], [a.num_items for a in arenas], out_u8=True)
    torch.cuda.synchronize()
    assert min(int(a.num_items.item()) for a in arenas) >= want_rows
    out = [u[:want_rows].cpu().numpy() for u in u8]
    for a in arenas:
        a.close()
    return out


def test_finished_real_descriptors_4096(nm, cuda):
    A, B = _finished_1080p(nm, cuda, (0, 1))
    c = dict(A=A, B=B, nA=4096, nB=4096, amb=0.8, prior=-1, what="4096 x 4096 finished descriptors")
    got = _assert_all_equal(nm, cuda, [c], 4096, 4096, 0.8)
    print("4096 x 4096 finished descriptors: %d matches" % (got[0] >= 0).sum())
    assert (got[0] >= 0).sum() > 200


def test_chain_detect_finish_match_u8_ransac_in_one_graph(nm, cuda):
    """detect -> finish -> u8 match -> RANSAC on two views of one scene, on one stream, captured into one HIP graph and
    replayed on the views of a second scene with other keypoint counts: every output equals the eager run's bit for bit, and
    the recovered homography is within test_gpu_pipeline's tolerance of the true map."""
    import torch
    import test_gpu_mosaic as G
    cap, iterations = G.CAP, 2048
    arenas = [nm.SiftArena(G.VW, G.VH, cap) for _ in range(2)]
    u8 = [torch.zeros((cap, 128), dtype=torch.uint8, device=cuda) for _ in range(2)]
    res = [torch.full((cap,), -1, dtype=torch.int32, device=cuda)]
    uws = nm.MatchU8Workspace(1, cap, cap, cuda)
    rws = nm.RansacBatchWorkspace(1, cap, iterations, cuda)

    def enqueue(views):
        a, b = arenas
        nm.detect_describe_batch(arenas, [nm.grayscale(v) for v in views])
        nm.desc_finish_batch_dev([a.desc, b.desc], [a.num_items, b.num_items], out_u8=u8, capacity=cap)
        nm.sift_match_u8_batch_dev([u8[0]], [a.num_items], [u8[1]], [b.num_items], results=res, ambiguity=0.8, workspace=uws,
                                   capA=cap, capB=cap)
        Hb, best, pos, status = nm.ransac_batch_dev(2, [a.x], [a.y], [a.num_items], [b.x], [b.y], res, iterations=iterations,
                                                    threshold=1.0, seeds=[3], capA=cap, workspace=rws)
        return Hb, best, pos, status, a.num_items, b.num_items, res[0], u8[0], u8[1]

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
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    got = [o.cpu().numpy().copy() for o in captured]
    res[0].fill_(-1)
    with torch.cuda.stream(s):
        want = [o.cpu().numpy().copy() for o in enqueue([v.clone() for v in v2])]
    torch.cuda.synchronize()
    for x, y in zip(got, want):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    cnt = lambda o: (int(o[4].reshape(-1)[0]), int(o[5].reshape(-1)[0]))
    assert cnt(first) != cnt(got), "the second scene has the first one's counts"
    maps = G._view_maps()
    Ht = np.linalg.inv(maps[1]) @ maps[0]
    Ht /= Ht[2, 2]
    for out in (first, got):
        Hb, status, matches = out[0], out[3], out[6]
        assert int(status.reshape(-1)[0]) == 1 and (matches >= 0).sum() > 100
        Hn = Hb.reshape(3, 3).astype(np.float64) / float(Hb.reshape(-1)[8])
        np.testing.assert_allclose(Hn, Ht, atol=0.6, rtol=0.05)
        np.testing.assert_allclose(Hn[:2, :2], Ht[:2, :2], atol=5e-3)
    # the eager u8 matches equal the host twin on the bytes the chain produced
    nA, nB = cnt(got)
    host = nm.sift_match_u8_host([got[7]], [nA], [got[8]], [nB], ambiguity=0.8, prior=-1)
    assert np.array_equal(host[0], got[6])
    for a in arenas:
        a.close()
