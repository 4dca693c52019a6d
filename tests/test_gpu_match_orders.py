"""The brute-force matchers on the GPU on adversarial candidate ORDERS (tests/match_order_ref.py: strictly descending and
ascending distances, descending plateaus of identical rows, the two nearest rows in the partial last tile, sawtooths over
the lane halves and over the tiles): the u8 matcher, the u8 k-NN entry at every k in 1 .. 8, the u8 mutual filter in both
directions, the fp32 matcher under its three screens and the sharded entry. Everything is array_equal: against the host
twins, the numpy restatements (match_u8_ref, knn_u8_ref, mutual_u8_ref) and, for fp32, the oracle. No tolerance, no
excluded row. Which of these orders can see which slip of the scan is measured on the CPU, in test_match_orders_host.py.
"""
import numpy as np
import pytest

import knn_u8_ref as K
import match_order_ref as O
import match_u8_ref as M
import mutual_u8_ref as MU
import test_gpu_match_knn_u8 as TK
import test_gpu_match_mutual_u8 as TM
import test_gpu_match_u8 as TU

pytestmark = pytest.mark.gpu

AMBS = (0.8, 1.0, 1.5)
_CASES = {}


def cases_of(family):
    """A family's cases, built once and left unchanged."""
    if family not in _CASES:
        _CASES[family] = O.family_cases(family)
    return _CASES[family]


def _matcher(nm, dev, cases, amb):
    """The u8 matcher on one batch against its host twin, the fp32 matcher on float copies and the restatement."""
    got = TU._assert_all_equal(nm, dev, [dict(c, amb=amb) for c in cases], O.CAP_A, O.CAP_B, amb)
    for p, c in enumerate(cases):
        assert np.array_equal(got[p], M.expected_clipped(dict(c, amb=amb), O.CAP_A, O.CAP_B)), (c["what"], amb, "restatement")
        assert (got[p][max(c["nA"], 0):] == c["prior"]).all(), (c["what"], "a row at or beyond nA was written")
    return got


@pytest.mark.parametrize("amb", AMBS)
@pytest.mark.parametrize("family", O.FAMILIES)
def test_u8_matcher(nm, cuda, family, amb):
    cases = cases_of(family)
    got = _matcher(nm, cuda, cases, amb)
    if amb == 1.5:                                              # every ratio is at most 1: the nearest row itself
        for p, c in enumerate(cases):
            nearest = M.distances(c["A"][:c["nA"]], c["B"][:c["nB"]]).argmin(1)
            assert np.array_equal(got[p][:c["nA"]], nearest), c["what"]
    elif family != "plateaus_descending":                       # (a nearest run of two or more rows is min2 == min1: all -1)
        seen = np.concatenate([g[:c["nA"]] for g, c in zip(got, cases)])
        assert (seen >= 0).any() and (amb == 1.0 or (seen == -1).any()), "0.8 splits the queries, 1.0 accepts them"


@pytest.mark.parametrize("k", range(1, 9))
@pytest.mark.parametrize("family", O.FAMILIES)
def test_knn(nm, cuda, family, k):
    cases = cases_of(family)
    tensors = TK._upload(cuda, cases, O.CAP_A, O.CAP_B)
    idx, dist = TK._assert_all_equal(nm, cuda, cases, k, O.CAP_A, O.CAP_B, tensors=tensors)
    only, none = TK._device(nm, cuda, cases, k, O.CAP_A, O.CAP_B, want_distance=False, tensors=tensors)
    assert none is None
    for p, c in enumerate(cases):
        assert np.array_equal(only[p], idx[p]), (c["what"], k, "indices only")
        assert (idx[p][c["nA"]:] == K.PRIOR[0]).all() and (dist[p][c["nA"]:] == K.PRIOR[1]).all(), c["what"]
        if family == "descending":                              # outright: nB - 1, nB - 2, ..
            assert (idx[p][:c["nA"]] == c["nB"] - 1 - np.arange(k)).all(), (c["what"], k)
        if family == "plateaus_descending":                     # the nearest run, lowest index first
            r0, w = c["runs"][-1]
            m = min(k, w)
            assert (idx[p][:c["nA"], :m] == r0 + np.arange(m)).all() and (dist[p][:c["nA"], :m] == dist[p][:c["nA"], :1]).all()
            if c["nB"] == 44:                                   # then the lowest rows of the run before: one lane half of tile 1
                assert (idx[p][:c["nA"]] == np.array([40, 41, 42, 43, 32, 33, 34, 35])[:k]).all(), (c["what"], k)


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_knn_of_permuted_candidates(nm, cuda, k):
    """Metamorphic, no reference: shuffling the candidates maps the index lists through the permutation and leaves the
    distance lists as they are."""
    for c in (cases_of("descending")[2], M.random_case(47, 65, 129)):
        capA, capB = len(c["A"]), len(c["B"])
        idx, dist = TK._device(nm, cuda, [c], k, capA, capB)
        for seed in (1, 2):
            p, source = O.permuted(c, seed)
            pidx, pdist = TK._device(nm, cuda, [p], k, capA, capB)
            nA = c["nA"]
            assert np.array_equal(source[pidx[0][:nA]], idx[0][:nA]), (c["what"], k, seed, "index lists")
            assert np.array_equal(pdist[0], dist[0]), (c["what"], k, seed, "distance lists")


@pytest.mark.parametrize("amb", AMBS)
def test_k2_lists_against_the_matcher(nm, cuda, amb):
    """The list fold at L = 2 against the top-2 fold, on orders where both do their maximal work."""
    import torch
    cases = O.all_cases()
    tensors = TK._upload(cuda, cases, O.CAP_A, O.CAP_B)
    idx, dist = TK._device(nm, cuda, cases, 2, O.CAP_A, O.CAP_B, tensors=tensors)
    res = [torch.full((O.CAP_A,), c["prior"], dtype=torch.int32, device=cuda) for c in cases]
    nm.sift_match_u8_batch_dev(*tensors, results=res, ambiguity=amb, capA=O.CAP_A, capB=O.CAP_B)
    torch.cuda.synchronize()
    for p, c in enumerate(cases):
        lists = K.matcher_from_lists(c, idx[p], dist[p], amb, O.CAP_A, O.CAP_B)
        assert np.array_equal(lists, res[p].cpu().numpy()), (c["what"], amb)


@pytest.mark.parametrize("family", O.FAMILIES)
def test_u8_mutual_filter_in_both_directions(nm, cuda, family):
    for c in cases_of(family):
        for way, m in enumerate(O.mutual_cases(c)):
            capA, capB = len(m["A"]), len(m["B"])
            got = TM._assert_all_equal(nm, cuda, [m], capA, capB)             # host twin and the fp32 filter on float copies
            want, wcount, wfwd = MU.expected(m, capA, capB)
            assert np.array_equal(got["result"][0], want) and got["count"][0] == wcount, m["what"]
            assert np.array_equal(TM._u32(got["forward"][0]), TM._u32(wfwd)), m["what"]
            MU.kept_removed([m], capA, capB)
            if family == "descending" and way == 0:             # every query names the last row; the first nearest query stays
                assert (m["m"][:m["nA"]] == m["nB"] - 1).all() and wcount == 1
                survivor = int(M.distances(m["A"][:m["nA"]], m["B"][m["nB"] - 1:m["nB"]])[:, 0].argmin())
                assert np.flatnonzero(got["result"][0] >= 0).tolist() == [survivor]
                assert got["result"][0][survivor] == m["nB"] - 1


@pytest.fixture(params=["f16", "bf16x3", "f32"])
def screen(request, nm):
    """The three MFMA screens of the fp32 matcher. A copy of test_gpu_match.py's `screen` fixture, which is autouse and would
    run the u8 tests of this module three times if imported: keep the two in step (the screens, and the distance mode that
    rides along)."""
    before, dbefore = nm.get_match_screen(), nm.get_distance_mode()
    nm.set_match_screen(request.param)
    nm.set_distance_mode("exact" if request.param == "bf16x3" else "mfma")
    yield request.param
    nm.set_match_screen(before)
    nm.set_distance_mode(dbefore)


_ORACLE = {}


def _oracle(oracle, c, amb):
    """The oracle's answers for a case as float32, computed once per (case, ambiguity) and shared by the screens."""
    key = (c["what"], amb)
    if key not in _ORACLE:
        A, B = c["A"][:c["nA"]].astype(np.float32), c["B"][:c["nB"]].astype(np.float32)
        ref, _, _ = oracle.sift_matches(A, B, amb, want_distance=False, prior=np.full(c["nA"], -7, np.int32))
        _ORACLE[key] = (ref, oracle.sift_match_shard(A, B, 0))
    return _ORACLE[key]


def _fp32(nm, oracle, dev, c, amb):
    """sift_match on the whole buffers with the sizes passed (a row beyond them must not be read) and sift_match_shard."""
    import torch
    nA, nB = c["nA"], c["nB"]
    tA, tB = torch.from_numpy(c["A"].astype(np.float32)).to(dev), torch.from_numpy(c["B"].astype(np.float32)).to(dev)
    prior = torch.full((len(c["A"]),), -7, dtype=torch.int32, device=dev)
    got, _ = nm.sift_match(tA, tB, amb, prior=prior, nA=nA, nB=nB)
    m1, ix, m2 = nm.sift_match_shard(tA[:nA], tB[:nB], 0)
    torch.cuda.synchronize()
    ref, (r1, rx, r2) = _oracle(oracle, c, amb)
    got = got.cpu().numpy()
    assert np.array_equal(got[:nA], ref), (c["what"], amb, "sift_match")
    assert (got[nA:] == -7).all(), (c["what"], "a row at or beyond nA was written")
    assert np.array_equal(ix.cpu().numpy(), rx), (c["what"], "shard index")
    assert np.array_equal(m1.cpu().numpy(), r1) and np.array_equal(m2.cpu().numpy(), r2), (c["what"], "shard distances")
    return got[:nA]


@pytest.mark.parametrize("family", O.FAMILIES)
def test_fp32_matcher_and_shard(nm, oracle, cuda, screen, family):
    for c in cases_of(family):
        for amb in AMBS:
            got = _fp32(nm, oracle, cuda, c, amb)
            assert np.array_equal(got, M.expected(dict(c, amb=amb), c["nA"])), (c["what"], amb, "the u8 restatement")


def _large():
    if "large" not in _CASES:
        _CASES["large"] = [O.descending(300, 4000, 9, gap=4, capA=300, capB=4000),
                           O.last_tile(300, 4000, False, 9, capA=300, capB=4000),
                           O.last_tile(300, 4000, True, 9, capA=300, capB=4000)]
    return _CASES["large"]


def test_fp32_matcher_300_x_4000(nm, oracle, cuda, screen):
    """descending and last_tile at the 300 x 4000 of test_gpu_match_groups.py: many candidate tiles at one-workgroup cost."""
    for c in _large():
        for amb in (0.8, 1.5):
            got = _fp32(nm, oracle, cuda, c, amb)
            if amb == 1.5:
                assert (got == 3999).all(), c["what"]


def test_ragged_batch_of_mixed_families(nm, cuda):
    """16 pairs, the families mixed across the slots, one pair empty: the u8 matcher and k-NN at k = 8. Each pair equals its
    result alone."""
    batch = O.ragged_batch()
    tensors = TK._upload(cuda, batch, O.CAP_A, O.CAP_B)
    got = _matcher(nm, cuda, batch, 0.8)
    idx, dist = TK._assert_all_equal(nm, cuda, batch, 8, O.CAP_A, O.CAP_B, tensors=tensors)
    empty = [p for p, c in enumerate(batch) if c["nA"] <= 0 or c["nB"] <= 0]
    assert empty == [8] and (got[8] == -7).all() and (idx[8] == K.PRIOR[0]).all() and (dist[8] == K.PRIOR[1]).all()
    for p, c in enumerate(batch):
        alone = _matcher(nm, cuda, [c], 0.8)
        ai, ad = TK._device(nm, cuda, [c], 8, O.CAP_A, O.CAP_B, tensors=[t[p:p + 1] for t in tensors])
        assert np.array_equal(alone[0], got[p]), (c["what"], "the matcher's result depends on the batch")
        assert np.array_equal(ai[0], idx[p]) and np.array_equal(ad[0], dist[p]), (c["what"], "the lists depend on the batch")
