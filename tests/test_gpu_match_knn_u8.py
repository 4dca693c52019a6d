"""The u8 k-nearest-neighbour entry on the GPU (nm_sift_match_knn_u8_batch_dev): array_equal on index and distance lists
against its host twin AND the numpy restatement (tests/knn_u8_ref.py): sizes around the 32-candidate tile, the 64-query wave
and the 256-query workgroup at every k, sizes around k (empty slots), ties across the lane halves and a tile boundary, the
largest distance, ragged batches with an empty pair, agreement with the u8 matcher and with the u8 mutual filter's forward
distances, one 2048 x 2048 pair of finished real descriptors, and the two launches captured into one HIP graph.
"""
import numpy as np
import pytest

import knn_u8_ref as K
import match_u8_ref as M

pytestmark = pytest.mark.gpu


def _upload(dev, cases, capA, capB):
    import torch
    up = lambda a, cap: torch.from_numpy(np.ascontiguousarray(a[:cap])).to(dev)
    size = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)
    return ([up(c["A"], capA) for c in cases], [size(c["nA"]) for c in cases], [up(c["B"], capB) for c in cases],
            [size(c["nB"]) for c in cases])


def _device(nm, dev, cases, k, capA, capB, want_distance=True, tensors=None):
    """One device call on outputs pre-filled with K.PRIOR. Returns (index, distance) as lists of numpy arrays."""
    import torch
    A, nA, B, nB = tensors or _upload(dev, cases, capA, capB)
    pre = lambda v: [torch.full((capA, k), v, dtype=torch.int32, device=dev) for _ in cases]
    idx, dist = nm.sift_match_knn_u8_batch_dev(A, nA, B, nB, k, indices=pre(K.PRIOR[0]),
                                               distances=pre(K.PRIOR[1]) if want_distance else None,
                                               want_distance=want_distance, capA=capA, capB=capB)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in idx], [t.cpu().numpy() for t in dist] if want_distance else None


def _assert_all_equal(nm, dev, cases, k, capA, capB, tensors=None):
    idx, dist = _device(nm, dev, cases, k, capA, capB, tensors=tensors)
    col = lambda key: [c[key] for c in cases]
    hi, hd = nm.sift_match_knn_u8_host(col("A"), col("nA"), col("B"), col("nB"), k, capA=capA, capB=capB, prior=K.PRIOR)
    for p, c in enumerate(cases):
        for what, got, host in (("index", idx[p], hi[p]), ("distance", dist[p], hd[p])):
            bad = np.argwhere(got != host)
            assert not len(bad), (c["what"], k, what, "host twin", bad[:5], got[got != host][:5], host[got != host][:5])
        wi, wd = K.expected(c, k, capA, capB)
        assert np.array_equal(idx[p], wi) and np.array_equal(dist[p], wd), (c["what"], k, "restatement")
    return idx, dist


@pytest.mark.parametrize("k", range(1, 9))
def test_size_sweep(nm, cuda, k):
    for c in M.mixed_size_cases():
        _assert_all_equal(nm, cuda, [c], k, len(c["A"]), len(c["B"]))
    c = M.mixed_size_cases()[6]                                 # indices only: the same index lists
    only, none = _device(nm, cuda, [c], k, 127, 129, want_distance=False)
    assert none is None and np.array_equal(only[0], K.expected(c, k, 127)[0])


@pytest.mark.parametrize("k", [2, 4, 8])
def test_sizes_around_k(nm, cuda, k):
    for nB in (k - 1, k, k + 1):
        c = M.random_case(70 + nB, 33, nB)
        idx, dist = _assert_all_equal(nm, cuda, [c], k, 33, nB)
        m = min(k, nB)
        assert (idx[0][:, m:] == K.NO_INDEX).all() and (dist[0][:, m:] == K.NO_DISTANCE).all()
        assert ((idx[0][:, :m] >= 0) & (idx[0][:, :m] < nB)).all(), "a padded row's index was stored"
        assert (dist[0][:, :m] <= 128 * 255 * 255).all(), "a padded row's distance was stored"


def test_ties(nm, cuda):
    for c in K.tie_cases():
        idx, _ = _assert_all_equal(nm, cuda, [c], 8, 40, 70)
        first = 0 if "70" in c["what"] else 28
        assert (idx[0] == np.arange(first, first + 8)).all(), c["what"]
    dup = M.duplicate_cases()[0]
    pairs = [(3, 4), (8, 12), (20, 52), (60, 93), (31, 32)]
    for k in (2, 3):
        idx, dist = _assert_all_equal(nm, cuda, [dup], k, 12, 140)
        for t, p in enumerate(pairs):                          # query t ties on both copies, query 5 + t equals both
            assert tuple(idx[0][t, :2]) == p and tuple(idx[0][5 + t, :2]) == p and (dist[0][5 + t, :2] == 0).all()


def test_extremes(nm, cuda):
    for c in K.extreme_cases():
        _, dist = _assert_all_equal(nm, cuda, [c], 8, 40, 70)
    assert dist[0][:, 7].max() == 128 * 255 * 255 and dist[0].min() == 0


@pytest.mark.parametrize("n", [1, 3, 16, 64])
def test_ragged_batches(nm, cuda, n):
    cases, capA, capB = M.ragged_batch(n)
    tensors = _upload(cuda, cases, capA, capB)
    idx, dist = _assert_all_equal(nm, cuda, cases, 4, capA, capB, tensors=tensors)
    empty = [p for p, c in enumerate(cases) if c["nA"] <= 0 or c["nB"] <= 0]
    assert len(empty) == 1 and (idx[empty[0]] == K.PRIOR[0]).all() and (dist[empty[0]] == K.PRIOR[1]).all()
    for p, c in enumerate(cases):
        nA = min(max(c["nA"], 0), capA)
        assert (idx[p][nA:] == K.PRIOR[0]).all() and (dist[p][nA:] == K.PRIOR[1]).all(), "a row beyond nA was written"
    last = n - 1 if n - 1 not in empty else 0
    ai, ad = _device(nm, cuda, [cases[last]], 4, capA, capB, tensors=[t[last:last + 1] for t in tensors])
    assert np.array_equal(ai[0], idx[last]) and np.array_equal(ad[0], dist[last]), "a pair's lists depend on the batch"


@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_shared_scan_cases(nm, cuda, k):
    """M.shared_scan_cases() at a k of every list length the kernel is built for, each alone and as a 3-pair batch with the
    empty pair: host twin and restatement, untouched rows, and equal distances in index order."""
    cases, capA, capB = M.shared_scan_cases()
    one, same, empty, ties = cases
    for batch in [[one], [same], [ties], [same, empty, ties]]:
        idx, dist = _assert_all_equal(nm, cuda, batch, k, capA, capB)
        for p, c in enumerate(batch):
            assert (idx[p][c["nA"]:] == K.PRIOR[0]).all() and (dist[p][c["nA"]:] == K.PRIOR[1]).all(), c["what"]
    m = min(k, 2)
    assert (idx[0][:65, :m] == np.arange(m)).all() and (dist[0][:32, :m] == 0).all() and (idx[0][:65, m:] == K.NO_INDEX).all()
    if k >= 2:
        assert tuple(idx[2][10, :2]) == (1, 5) and tuple(idx[2][11, :2]) == (0, 32) and (dist[2][10:12, :2] == 9).all()


@pytest.mark.parametrize("amb", [0.8, 1.0])
def test_k2_lists_reproduce_the_matcher(nm, cuda, amb):
    import torch
    for c in M.all_cases():
        capA, capB = len(c["A"]), len(c["B"])
        tensors = _upload(cuda, [c], capA, capB)
        idx, dist = _device(nm, cuda, [c], 2, capA, capB, tensors=tensors)
        res = [torch.full((capA,), c["prior"], dtype=torch.int32, device=cuda)]
        nm.sift_match_u8_batch_dev(*tensors, results=res, ambiguity=amb, capA=capA, capB=capB)
        torch.cuda.synchronize()
        got = K.matcher_last_step(idx[0], dist[0], c["nB"], amb, np.full(capA, c["prior"], np.int32))
        assert np.array_equal(got, res[0].cpu().numpy()), (c["what"], amb)


def test_first_column_is_the_mutual_filters_forward_distance(nm, cuda):
    import torch
    c = M.random_case(77, 129, 127)
    tensors = _upload(cuda, [c], 129, 127)
    idx, dist = nm.sift_match_knn_u8_batch_dev(*tensors, 3, capA=129, capB=127)
    first = [idx[0][:, 0].contiguous()]
    _, _, fwd = nm.sift_match_mutual_u8_batch_dev(*tensors, first, capA=129, capB=127, want_distance=True)
    torch.cuda.synchronize()
    assert torch.equal(dist[0][:, 0].float(), fwd[0]) and bool(torch.isfinite(fwd[0]).all())


def test_finished_real_descriptors_2048(nm, cuda):
    from test_gpu_match_u8 import _finished_1080p
    A, B = _finished_1080p(nm, cuda, (0, 1), want_rows=2048)
    c = dict(A=A, B=B, nA=2048, nB=2048, what="2048 x 2048 finished descriptors")
    idx, dist = _assert_all_equal(nm, cuda, [c], 8, 2048, 2048)
    assert (np.diff(dist[0], axis=1) >= 0).all() and (idx[0] >= 0).all()


def test_two_launches_in_one_graph(nm, cuda):
    """The norms launch and the k-NN launch captured on one stream and replayed after the descriptor bytes and the device
    counts were overwritten with another case of the same capacities: the replay equals the host twin on the new case."""
    import torch
    capA, capB, k = 150, 140, 5
    c1, c2 = M.random_case(301, capA, capB), M.random_case(302, capA, capB)
    c1["nA"], c1["nB"], c2["nA"], c2["nB"] = 150, 140, 97, 33
    A, nA, B, nB = _upload(cuda, [c1], capA, capB)
    idx = [torch.full((capA, k), K.PRIOR[0], dtype=torch.int32, device=cuda)]
    dist = [torch.full((capA, k), K.PRIOR[1], dtype=torch.int32, device=cuda)]
    ws = nm.MatchKnnU8Workspace(1, capA, capB, cuda)
    run = lambda: nm.sift_match_knn_u8_batch_dev(A, nA, B, nB, k, indices=idx, distances=dist, workspace=ws, capA=capA, capB=capB)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        run()                                                  # warm-up outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run()
    for t, v in zip((A[0], B[0]), _upload(cuda, [c2], capA, capB)[0::2]):
        t.copy_(v[0])
    nA[0].fill_(c2["nA"])
    nB[0].fill_(c2["nB"])
    idx[0].fill_(K.PRIOR[0])
    dist[0].fill_(K.PRIOR[1])
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    hi, hd = nm.sift_match_knn_u8_host([c2["A"]], [97], [c2["B"]], [33], k, capA=capA, capB=capB, prior=K.PRIOR)
    assert np.array_equal(idx[0].cpu().numpy(), hi[0]) and np.array_equal(dist[0].cpu().numpy(), hd[0])
    assert np.array_equal(hi[0], K.expected(c2, k, capA, capB)[0])
