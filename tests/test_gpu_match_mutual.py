"""nm_sift_match_mutual_batch_dev_f32 on the MI355X: bit-identity with its host twin over batch sizes and ragged pairs, the
early-exit traps, slot independence, sentinel-guarded outputs and workspace, the chain behind the blind matcher against the
restatement tests/mutual_ref.py, detect -> match -> mutual -> RANSAC captured into one HIP graph, and one 1080p pair against
the swapped blind match.

The kernel's constants and the sizes below that cross them (csrc/nm_match_mutual.hip):
    64   claims per wave of the scan kernel:        claim counts 0, 1, 63, 64, 65
    256  claims per workgroup of the scan kernel,
         rows per workgroup of the claims kernel:    claim counts 255, 256, 257, 1100; row counts 255 .. 257, 513, 1024, 1100
    8    row ranges of a pair (SPLIT):               row counts 1 and 7 (ranges without rows), 8, 9, 37 (ragged last range)
"""
import ctypes as C

import numpy as np
import pytest

import mutual_ref as R
from test_match_mutual_host import NEVER, assert_one_to_one, trap_pair

pytestmark = pytest.mark.gpu

CAPA, CAPB = 1100, 1200
OUT = ("result", "count", "forward")
# rows of A, rows of B, claims
SIZES = [(300, 280, 65), (0, 200, 0), (257, 1030, 63), (1100, 1200, 257), (37, 3, 37), (700, 0, 0), (64, 65, 64), (1, 1, 1),
         (513, 700, 256), (1024, 1025, 255), (7, 40, 1), (9, 9, 0), (1100, 1100, 1100), (8, 500, 8), (256, 256, 256), (255, 90, 64)]


def _u32(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _pair(seed, ra, rb, claims, nA=None, nB=None):
    """Small-integer descriptors at the call's capacities (the rows beyond the sizes hold plausible values that must not be
    read). `claims` rows claim a column: a third of them sit on it (tau = 0, every rival drops out in the first chunk), a
    third sit on a column whose twin row comes earlier or later, the others claim an arbitrary column (tau as large as any
    rival's distance: long walks, exact ties). The other rows carry -1, -7, nB and nB + 3."""
    rng = np.random.default_rng(seed)
    A = rng.integers(0, 4, (CAPA, 128)).astype(np.float32)
    B = rng.integers(0, 4, (CAPB, 128)).astype(np.float32)
    m = np.array([(-1, -7, rb, rb + 3)[i % 4] for i in range(CAPA)], np.int32)
    rows = np.sort(rng.permutation(max(ra, 1))[:claims]) if ra and rb else np.zeros(0, np.int64)
    for t, i in enumerate(rows):
        j = int(rng.integers(0, rb))
        m[i] = j
        if t % 3 < 2:
            A[i] = B[j]
        if t % 3 == 1:
            A[int(rng.integers(0, ra))] = B[j]                # a twin somewhere: the lower index wins the tie
    return dict(A=A, B=B, m=m, nA=ra if nA is None else nA, nB=rb if nB is None else nB)


def _mixed(n):
    pairs = [_pair(900 + k, *SIZES[k % len(SIZES)]) for k in range(n)]
    if n >= 16:
        pairs[6]["nA"], pairs[6]["nB"] = 10 ** 6, 10 ** 6     # clipped to the capacities: the padding rows take part
        pairs[9]["nA"], pairs[9]["nB"] = -3, 50
        pairs[12]["A"][17, 5] = np.nan                        # NaN in a row that claims, and as a rival of every column
        pairs[12]["A"][500, 99] = np.inf
    return pairs


def _host(nm, pairs):
    k = lambda key: [p[key] for p in pairs]
    return dict(zip(OUT, nm.sift_match_mutual_host(k("A"), k("nA"), k("B"), k("nB"), k("m"), capA=CAPA, capB=CAPB,
                                                   want_distance=True)))


def _upload(pairs, dev):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return [dict(A=t(p["A"]), B=t(p["B"]), m=t(p["m"]), nA=t(np.array([p["nA"]], np.int32)),
                 nB=t(np.array([p["nB"]], np.int32))) for p in pairs]


def _device(nm, pairs, dev, up=None, capA=CAPA, capB=CAPB):
    import torch
    up = _upload(pairs, dev) if up is None else up
    k = lambda key: [u[key] for u in up]
    res, cnt, fwd = nm.sift_match_mutual_batch_dev(k("A"), k("nA"), k("B"), k("nB"), k("m"), capA=capA, capB=capB,
                                                   want_distance=True)
    torch.cuda.synchronize()
    return dict(result=np.stack([r.cpu().numpy() for r in res]), count=cnt.cpu().numpy(),
                forward=np.stack([f.cpu().numpy() for f in fwd]))


def _assert_same(a, b, what):
    for k in OUT:
        assert np.array_equal(_u32(a[k]), _u32(b[k])), (what, k)


@pytest.mark.parametrize("n", [1, 3, 16, 64])
def test_device_equals_host_twin(nm, cuda, n):
    pairs = _mixed(n)
    want = _host(nm, pairs)
    got = _device(nm, pairs, cuda)
    _assert_same(got, want, "n %d" % n)
    assert np.array_equal((got["result"] >= 0).sum(axis=1), got["count"])
    for k, p in enumerate(pairs):
        assert_one_to_one(got["result"][k], p, "pair %d" % k)
    claims = sum(int(((p["m"][:max(min(p["nA"], CAPA), 0)] >= 0) & (p["m"][:max(min(p["nA"], CAPA), 0)] < min(p["nB"], CAPB))).sum())
                 for p in pairs)
    kept = int(got["count"].sum())
    print("n %d: %d claims, %d kept" % (n, claims, kept))
    assert 0 < kept and (n == 1 or kept < claims), "the comparison covered nothing"


def test_claim_counts_around_the_wave_and_the_workgroup(nm, cuda):
    """One pair of 1100 x 1200 rows per claim count, all in one call."""
    counts = [0, 1, 63, 64, 65, 255, 256, 257, 1100]
    pairs = [_pair(40 + c, 1100, 1200, c) for c in counts]
    got, want = _device(nm, pairs, cuda), _host(nm, pairs)
    _assert_same(got, want, "claim counts")
    assert (got["count"] <= counts).all() and got["count"][0] == 0 and got["count"][-1] > 300


def test_early_exit_traps(nm, cuda):
    """The planted traps of the host test: in 40 rows (one wave, most row ranges 5 rows long) and spread over 1100 rows, so
    that a claim and its rival lie in different row ranges and workgroups."""
    for rows_a in (40, 1100):
        p, expect = trap_pair(rows_a)
        want = R.mutual(p["A"], p["nA"], p["B"], p["nB"], p["m"])
        got = _device(nm, [p], cuda, capA=rows_a, capB=12)
        assert np.array_equal(got["result"][0], want[0]), np.flatnonzero(got["result"][0] != want[0])
        assert got["count"][0] == want[1] and np.array_equal(_u32(got["forward"][0]), _u32(want[2]))
        kept = {i: bool(got["result"][0][i] >= 0) for i in expect}
        assert kept == expect, {i: (kept[i], expect[i]) for i in expect if kept[i] != expect[i]}


def test_slot_independence(nm, cuda):
    a, b = _pair(5, 1100, 1030, 700), _pair(6, 300, 1200, 100)
    alone, other = _device(nm, [a], cuda), _device(nm, [b], cuda)
    assert 50 < alone["count"][0] < 700
    for n, slot in ((1, 0), (38, 37), (64, 63), (64, 0)):
        pairs = [b] * n
        pairs[slot] = a
        r = _device(nm, pairs, cuda)
        for k in OUT:
            assert np.array_equal(_u32(r[k][slot]), _u32(alone[k][0])), (n, slot, k)
            if n > 1:
                assert np.array_equal(_u32(r[k][(slot + 1) % n]), _u32(other[k][0])), (n, slot, k)


@pytest.mark.parametrize("n", [5, 37])
def test_outputs_are_written_inside_their_bounds(nm, cuda, n):
    """result and forward_distance of every pair, the counts and the workspace lie in guarded buffers: capA rows per pair, n
    counts and nm_sift_match_mutual_workspace_bytes bytes are written at the most, nothing around them."""
    import torch
    Gd = 64
    pairs = _mixed(n)
    up = _upload(pairs, cuda)
    res = [torch.full((Gd + CAPA + Gd,), -7, dtype=torch.int32, device=cuda) for _ in range(n)]
    fwd = [torch.full((Gd + CAPA + Gd,), -7.0, dtype=torch.float32, device=cuda) for _ in range(n)]
    count = torch.full((Gd + n + Gd,), -7, dtype=torch.int32, device=cuda)
    need = nm.lib().nm_sift_match_mutual_workspace_bytes(n, CAPA)
    ws = torch.full((256 + need + 256,), 0xA5, dtype=torch.uint8, device=cuda)
    arr = lambda ptrs: (C.c_void_p * n)(*ptrs)
    tab = lambda key: arr([u[key].data_ptr() for u in up])
    rc = nm.lib().nm_sift_match_mutual_batch_dev_f32(n, tab("A"), tab("nA"), CAPA, tab("B"), tab("nB"), CAPB, tab("m"),
                                                     arr([r[Gd:].data_ptr() for r in res]), count[Gd:].data_ptr(),
                                                     arr([f[Gd:].data_ptr() for f in fwd]), ws[256:].data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    for b in res + fwd + [count]:
        assert (b[:Gd] == -7).all() and (b[-Gd:] == -7).all()
    assert (ws[:256] == 0xA5).all() and (ws[-256:] == 0xA5).all()
    want = _host(nm, pairs)
    assert np.array_equal(np.stack([r[Gd:-Gd].cpu().numpy() for r in res]), want["result"])
    assert np.array_equal(_u32(np.stack([f[Gd:-Gd].cpu().numpy() for f in fwd])), _u32(want["forward"]))
    assert np.array_equal(count[Gd:-Gd].cpu().numpy(), want["count"])
    for p, u in zip(pairs, up):                             # the inputs are read only
        assert np.array_equal(u["m"].cpu().numpy(), p["m"])


def test_chained_after_the_blind_matcher_equals_the_restatement(nm, cuda):
    """Two 640 x 480 views of one scene: detect -> sift_match_batch_dev -> mutual, sizes read on the device."""
    import torch
    import test_gpu_mosaic as M
    views = M._views(nm, cuda, M._scene(90))[:2]
    arenas = [nm.SiftArena(M.VW, M.VH, M.CAP) for _ in range(2)]
    nm.detect_describe_batch(arenas, [nm.grayscale(v) for v in views])
    a, b = arenas
    blind = torch.full((M.CAP,), -1, dtype=torch.int32, device=cuda)
    nm.sift_match_batch_dev([a.desc], [a.num_items], [b.desc], [b.num_items], [blind], 0.8)
    res, cnt, fwd = nm.sift_match_mutual_batch_dev([a.desc], [a.num_items], [b.desc], [b.num_items], [blind],
                                                   want_distance=True)
    torch.cuda.synchronize()
    host = lambda x: x.cpu().numpy()
    nA, nB = int(a.num_items.item()), int(b.num_items.item())
    want, wcount, wfwd = R.mutual(host(a.desc), nA, host(b.desc), nB, host(blind), capA=M.CAP, capB=M.CAP)
    got = host(res[0])
    print("640 x 480 views: %d x %d rows, blind ratio matches %d, mutual %d" % (nA, nB, int((blind >= 0).sum()), wcount))
    assert nA > 1500 and nB > 1500 and 500 < wcount <= int((blind >= 0).sum())
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert int(cnt.item()) == wcount and np.array_equal(_u32(host(fwd[0])), _u32(wfwd))
    assert_one_to_one(got, dict(nA=nA, m=host(blind)))
    for ar in arenas:
        ar.close()


def test_chain_with_the_mutual_filter_in_one_graph_replays_on_another_scene(nm, cuda):
    """detect -> match -> mutual -> RANSAC on the eight synthetic views of test_gpu_mosaic, captured into one HIP graph on a
    single stream and replayed on a second scene with other keypoint counts: every output equals the eager run bit for bit."""
    import torch
    import test_gpu_mosaic as M

    class Chain(M._Chain):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.mres = [torch.full((M.CAP,), -1, dtype=torch.int32, device=self.dev) for _ in range(7)]
            self.uws = self.nm.MatchMutualWorkspace(7, M.CAP, self.dev)

        def enqueue(self, views):
            nm_ = self.nm
            A, B = self.arenas[:-1], self.arenas[1:]
            nm_.detect_describe_batch(self.arenas, [nm_.grayscale(v) for v in views])
            nA, nB = [a.num_items for a in A], [b.num_items for b in B]
            nm_.sift_match_batch_dev([a.desc for a in A], nA, [b.desc for b in B], nB, self.res, 0.8, workspace=self.mws)
            mres, mcnt = nm_.sift_match_mutual_batch_dev([a.desc for a in A], nA, [b.desc for b in B], nB, self.res,
                                                         capA=M.CAP, capB=M.CAP, results=self.mres, workspace=self.uws)
            Hb, best, pos, status = nm_.ransac_batch_dev(2, [a.x for a in A], [a.y for a in A], nA, [b.x for b in B],
                                                         [b.y for b in B], mres, iterations=self.iterations, threshold=1.0,
                                                         seeds=list(range(7)), capA=M.CAP, workspace=self.rws)
            return (mcnt, Hb, best, pos, status) + tuple(a.num_items for a in self.arenas) + tuple(mres)

    v1 = M._views(nm, cuda, M._scene(90))
    v2 = M._views(nm, cuda, M._scene(91))
    bufs = [v.clone() for v in v1]
    ch = Chain(nm, cuda)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        first = [o.cpu().numpy().copy() for o in ch.enqueue(bufs)]     # warm-up outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        captured = ch.enqueue(bufs)
    for b, v in zip(bufs, v2):
        b.copy_(v)
    for r in ch.res + ch.mres:
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
    mcnt, status = got[0], got[4]
    assert any(int(x.reshape(-1)[0]) != int(y.reshape(-1)[0]) for x, y in zip(first[5:13], got[5:13])), "the second scene has the first one's keypoint counts"
    blind = np.array([(r.cpu().numpy() >= 0).sum() for r in ch.res])
    assert (status == 1).all() and (mcnt > 100).all() and (mcnt <= blind).all() and (mcnt < blind).any(), (mcnt, blind)
    assert np.array_equal(mcnt, [(r >= 0).sum() for r in got[13:]])
    ch.close()


def test_real_1080p_pair_equals_the_swapped_blind_match(nm, cuda):
    """A 1080p frame and its warp under a known map (as test_gpu_pipeline builds its pair), about 12k x 12k rows:
    kept(i) <=> rev[matches[i]] == i, rev being the blind match of B against A under a ratio test that never rejects. No
    claimed column may be left out of the comparison (rev is -1 where the blind scan leaves a row undecided, min2 <= 0)."""
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
    blind, rev = (torch.full((cap,), -1, dtype=torch.int32, device=cuda) for _ in range(2))
    nm.sift_match_batch_dev([a.desc], [a.num_items], [b.desc], [b.num_items], [blind], 0.8, capA=cap, capB=cap)
    nm.sift_match_batch_dev([b.desc], [b.num_items], [a.desc], [a.num_items], [rev], NEVER, capA=cap, capB=cap)
    res, cnt = nm.sift_match_mutual_batch_dev([a.desc], [a.num_items], [b.desc], [b.num_items], [blind], capA=cap, capB=cap)
    torch.cuda.synchronize()
    nA, nB = int(a.num_items.item()), int(b.num_items.item())
    m, rv, got = (x.cpu().numpy() for x in (blind, rev, res[0]))
    claimed = np.flatnonzero(m >= 0)
    assert nA > 8000 and nB > 8000 and len(claimed) > 2000
    assert (rv[m[claimed]] >= 0).all(), "the swapped match left a claimed column out"
    want = np.where((m >= 0) & (rv[np.maximum(m, 0)] == np.arange(cap)), m, -1)
    print("1080p pair: %d x %d rows, blind ratio matches %d, mutual %d" % (nA, nB, len(claimed), int((want >= 0).sum())))
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert int(cnt.item()) == (want >= 0).sum() > 1000
    assert_one_to_one(got, dict(nA=nA, m=m))
    for ar in arenas:
        ar.close()
