"""The link proposal on the GPU (nm_link_votes_dev_u8, nm_link_rank_dev): array_equal against the host twins over the cases
of tests/link_propose_ref.py -- every n in {1, 2, 3, 5} with every cap in {1, 31, 33, 255, 257, 300} and counts through
0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, cap and the clip; 64 frames of cap 40 (all 4032 ordered pairs, every slot, every
split of the candidate frames); stale workspace and outputs; permuted frames; the votes against sift_match_u8_batch_dev on
the same tables; duplicates, equal distances and a frame against its copy; the ranking on the CPU test's matrices; finish ->
votes -> rank captured into one HIP graph and replayed on other inputs; refusals that launch nothing.
"""
import ctypes as C

import numpy as np
import pytest

import link_propose_ref as R

pytestmark = pytest.mark.gpu

INVALID = 1                                     # hipErrorInvalidValue
_HOST = {}


def _host_votes(nm, c):
    """The host twin's votes of a case, computed once."""
    if c["what"] not in _HOST:
        _HOST[c["what"]] = nm.link_votes_host(c["descs"], c["counts"], ambiguity=c["amb"], cap=c["cap"])
    return _HOST[c["what"]]


def _upload(dev, c):
    import torch
    descs = [torch.from_numpy(d).to(dev) for d in c["descs"]]
    if "same" in c:
        descs[c["same"][1]] = descs[c["same"][0]]                     # two slots, one device table
    counts = [torch.tensor([v], dtype=torch.int32, device=dev) for v in c["counts"]]
    return descs, counts


def _dev_votes(nm, dev, c, **kw):
    import torch
    descs, counts = _upload(dev, c)
    v = nm.link_votes_dev(descs, counts, ambiguity=c["amb"], cap=c["cap"], **kw)
    torch.cuda.synchronize()
    return v.cpu().numpy()


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_votes_equal_host_twin_over_sizes(nm, cuda, n):
    import torch
    cases = [c for c in R.size_cases() if len(c["descs"]) == n]
    assert {c["cap"] for c in cases} == set(R.CAPS)
    total = 0
    for c in cases:
        n, cap = len(c["descs"]), c["cap"]
        ws = nm.LinkVotesWorkspace(n, cap, cuda)
        ws.buf.fill_(0x5a)                                            # stale norms, stale votes
        votes = torch.full((n, n), 0x5a5a5a5a, dtype=torch.int32, device=cuda)
        got = _dev_votes(nm, cuda, c, votes=votes, workspace=ws)
        host = _host_votes(nm, c)
        assert np.array_equal(got, host), (c["what"], got, host)
        total += int(got.sum())
    assert n == 1 or total > 0


def test_64_frames_every_split_of_the_candidate_frames(nm, cuda):
    c = R.ragged64()
    host = _host_votes(nm, c)
    assert (host[5] == 0).all() and (host[:, 5] == 0).all() and (np.diag(host) == 0).all() and host.sum() > 1000
    try:
        for z in (0, 1, 2, 3, 7, 64):                                 # the default, one part, uneven parts, one frame per part
            nm.link_votes_set_split(z)
            got = _dev_votes(nm, cuda, c)
            assert np.array_equal(got, host), (z, np.argwhere(got != host)[:5])
    finally:
        nm.link_votes_set_split(0)


def test_two_calls_through_one_workspace_and_permuted_frames(nm, cuda):
    import torch
    c1 = dict(what="reuse 1", descs=R.world_frames(21, 5, 300), counts=[300, 257, 64, 0, 33], cap=300, amb=0.8)
    c2 = dict(what="reuse 2", descs=R.world_frames(22, 5, 300), counts=[31, 300, 1, 256, 65], cap=300, amb=0.8)
    ws = nm.LinkVotesWorkspace(5, 300, cuda)
    ws.buf.fill_(0x5a)
    votes = torch.full((5, 5), 0x5a5a5a5a, dtype=torch.int32, device=cuda)
    for c in (c1, c2, c1):
        got = _dev_votes(nm, cuda, c, votes=votes, workspace=ws)
        assert np.array_equal(got, _host_votes(nm, c)), c["what"]
    perm = [3, 0, 4, 2, 1]
    p = dict(what="reuse 1 permuted", descs=[c1["descs"][k] for k in perm], counts=[c1["counts"][k] for k in perm], cap=300, amb=0.8)
    got = _dev_votes(nm, cuda, p, votes=votes, workspace=ws)
    assert np.array_equal(got, _host_votes(nm, c1)[np.ix_(perm, perm)])


def test_votes_equal_the_device_matcher_on_the_same_tables(nm, cuda):
    import torch
    c = dict(what="against the matcher", descs=R.world_frames(5, 5, 120), counts=[120, 77, 1, 64, 33], cap=120, amb=0.8)
    descs, counts = _upload(cuda, c)
    votes = nm.link_votes_dev(descs, counts, ambiguity=0.8, cap=120)
    pairs = [(a, b) for a in range(5) for b in range(5) if a != b]
    res = nm.sift_match_u8_batch_dev([descs[a] for a, _ in pairs], [counts[a] for a, _ in pairs], [descs[b] for _, b in pairs],
                                     [counts[b] for _, b in pairs], ambiguity=0.8, capA=120, capB=120)
    torch.cuda.synchronize()
    votes = votes.cpu().numpy()
    for (a, b), r in zip(pairs, res):
        assert votes[a, b] == int((r >= 0).sum().item()), (a, b)
    assert (np.diag(votes) == 0).all() and votes.sum() > 0


def test_special_frames(nm, cuda):
    for c in R.special_cases():
        got, host = _dev_votes(nm, cuda, c), _host_votes(nm, c)
        assert np.array_equal(got, host), (c["what"], got, host)
        if c["what"].startswith("a frame and its copy"):
            assert got[0, 1] == 96 and got[1, 0] == 96
        if c["what"].startswith("duplicated candidates"):
            assert got[0, 1] <= 48


def test_rank_equals_host_twin(nm, cuda):
    import torch
    for c in R.rank_cases():
        kw = {k: c[k] for k in ("min_votes", "min_gap", "per_frame", "max_links")}
        links = tuple(torch.full((c["max_links"],), 0x5a5a5a5a, dtype=torch.int32, device=cuda) for _ in range(3)) + \
            (torch.full((1,), 0x5a5a5a5a, dtype=torch.int32, device=cuda),)
        la, lb, ls, cnt = nm.link_rank_dev(torch.from_numpy(c["votes"]).to(cuda), links=links, **kw)
        torch.cuda.synchronize()
        ha, hb, hs, hcnt = nm.link_rank_host(c["votes"], **kw)
        assert int(cnt.item()) == hcnt, c["what"]
        for got, host in ((la, ha), (lb, hb), (ls, hs)):
            assert np.array_equal(got.cpu().numpy(), host), c["what"]


def _raw_frames(seed, n, cap):
    """Raw fp32 descriptors (non-negative, as the descriptor kernel leaves them) of frames that share a world."""
    rng = np.random.default_rng(seed)
    world = rng.gamma(1.0, 1.0, (2 * cap, 128))
    return [(world[rng.permutation(2 * cap)[:cap]] * rng.uniform(0.9, 1.1, (cap, 128))).astype(np.float32) for _ in range(n)]


def test_finish_votes_rank_in_one_graph_replays_on_other_inputs(nm, cuda):
    import torch
    n, cap = 6, 200
    raw1, raw2 = _raw_frames(1, n, cap), _raw_frames(2, n, cap)
    cnt1, cnt2 = [200, 130, 64, 200, 33, 97], [65, 200, 0, 150, 200, 31]
    raw = [torch.from_numpy(r).to(cuda) for r in raw1]
    counts = [torch.tensor([v], dtype=torch.int32, device=cuda) for v in cnt1]
    u8 = [torch.zeros((cap, 128), dtype=torch.uint8, device=cuda) for _ in range(n)]
    ws = nm.LinkVotesWorkspace(n, cap, cuda)
    votes = torch.empty((n, n), dtype=torch.int32, device=cuda)
    links = tuple(torch.empty(16, dtype=torch.int32, device=cuda) for _ in range(3)) + (torch.empty(1, dtype=torch.int32, device=cuda),)

    def run():
        nm.desc_finish_batch_dev(raw, counts, out_u8=u8, capacity=cap)
        nm.link_propose(u8, counts, ambiguity=0.8, min_votes=5, min_gap=2, per_frame=2, max_links=16, cap=cap, votes=votes,
                        links=links, workspace=ws)

    def expect(raws, cnts):
        _, h8 = nm.desc_finish_host(raws, cnts, want_f32=False, capacity=cap)
        hv = nm.link_votes_host(list(h8), cnts, ambiguity=0.8, cap=cap)
        return hv, nm.link_rank_host(hv, min_votes=5, min_gap=2, per_frame=2, max_links=16)

    def check(raws, cnts):
        hv, (ha, hb, hs, hcnt) = expect(raws, cnts)
        assert np.array_equal(votes.cpu().numpy(), hv)
        assert int(links[3].item()) == hcnt and hcnt > 0
        for got, host in zip(links[:3], (ha, hb, hs)):
            assert np.array_equal(got.cpu().numpy(), host)

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        run()                                                         # warm-up outside capture
    torch.cuda.synchronize()
    check(raw1, cnt1)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run()
    for t, r in zip(raw, raw2):
        t.copy_(torch.from_numpy(r))
    for t, v in zip(counts, cnt2):
        t.fill_(v)
    for t in u8:
        t.zero_()
    votes.fill_(-1)
    for t in links:
        t.fill_(-7)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    check(raw2, cnt2)


def test_refusals_launch_nothing(nm, cuda):
    import torch
    lib = nm.lib()
    n, cap = 2, 40
    c = dict(what="refusals", descs=R.world_frames(3, n, cap), counts=[cap, cap], cap=cap, amb=0.8)
    descs, counts = _upload(cuda, c)
    ws = nm.LinkVotesWorkspace(n, cap, cuda)
    votes = torch.full((n, n), -5, dtype=torch.int32, device=cuda)
    tab = lambda ptrs: (C.c_void_p * len(ptrs))(*ptrs)
    d, k = [t.data_ptr() for t in descs], [t.data_ptr() for t in counts]
    v, w, st = votes.data_ptr(), ws.buf.data_ptr(), torch.cuda.current_stream().cuda_stream
    assert w % 16 == 0 and all(p % 16 == 0 for p in d)
    bad = [(0, tab(d), tab(k), cap, v, w), (65, tab(d), tab(k), cap, v, w), (n, tab(d), tab(k), 0, v, w),
           (n, tab(d), tab(k), 1 << 22, v, w), (n, None, tab(k), cap, v, w), (n, tab(d), None, cap, v, w),
           (n, tab([d[0], None]), tab(k), cap, v, w), (n, tab(d), tab([None, k[1]]), cap, v, w), (n, tab(d), tab(k), cap, None, w),
           (n, tab(d), tab(k), cap, v, None), (n, tab([d[0], d[1] + 8]), tab(k), cap, v, w), (n, tab(d), tab(k), cap, v, w + 4)]
    for i, (nn, dd, kk, cp, vv, ww) in enumerate(bad):
        assert lib.nm_link_votes_dev_u8(nn, dd, kk, cp, 0.8, vv, ww, st) == INVALID, i
    torch.cuda.synchronize()
    assert (votes == -5).all()

    mat = torch.full((3, 3), 4, dtype=torch.int32, device=cuda)
    outs = [torch.full((4,), -5, dtype=torch.int32, device=cuda) for _ in range(3)] + [torch.full((1,), -5, dtype=torch.int32, device=cuda)]
    m, (a, b, s, dl) = mat.data_ptr(), [o.data_ptr() for o in outs]
    bad = [(0, m, 1, 1, 0, 4, a, b, s, dl), (65, m, 1, 1, 0, 4, a, b, s, dl), (3, None, 1, 1, 0, 4, a, b, s, dl),
           (3, m, 0, 1, 0, 4, a, b, s, dl), (3, m, 1, 0, 0, 4, a, b, s, dl), (3, m, 1, 1, -1, 4, a, b, s, dl),
           (3, m, 1, 1, 0, 0, a, b, s, dl), (3, m, 1, 1, 0, 257, a, b, s, dl), (3, m, 1, 1, 0, 4, None, b, s, dl),
           (3, m, 1, 1, 0, 4, a, None, s, dl), (3, m, 1, 1, 0, 4, a, b, None, dl), (3, m, 1, 1, 0, 4, a, b, s, None)]
    for i, args in enumerate(bad):
        assert lib.nm_link_rank_dev(*args, st) == INVALID, i
    torch.cuda.synchronize()
    assert all(bool((o == -5).all()) for o in outs)
    assert lib.nm_link_rank_dev(3, m, 1, 1, 0, 4, a, b, s, dl, st) == 0
    torch.cuda.synchronize()
    assert int(outs[3].item()) == 3
