"""The host twins of the link proposal (nm_link_votes_host_u8, nm_link_rank_host) against the numpy restatement of
tests/link_propose_ref.py, equal entry for entry; the votes against the existing u8 matcher's host twin; every refusal with
the outputs untouched; and what the stage is worth: on a closed loop of 12 synthetic frames the proposal with min_gap = 3
returns exactly the three wrap-around pairs.
"""
import ctypes as C

import numpy as np
import pytest

import link_propose_ref as R

INVALID = 1                                     # hipErrorInvalidValue


def _host_votes(nm, c):
    return nm.link_votes_host(c["descs"], c["counts"], ambiguity=c["amb"], cap=c["cap"])


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_votes_equal_the_model_over_sizes_and_clipped_counts(nm, n):
    cases = [c for c in R.size_cases() if len(c["descs"]) == n]
    assert {c["cap"] for c in cases} == set(R.CAPS)
    seen = set()
    for c in cases:
        got, ref = _host_votes(nm, c), R.votes(c["descs"], c["counts"], c["cap"], c["amb"])
        assert np.array_equal(got, ref), (c["what"], got, ref)
        seen |= {(c["cap"], v) for v in c["counts"]}
    for cap in R.CAPS:                          # 0, 1, cap, a count above cap and a negative one, at every capacity
        assert {(cap, 0), (cap, cap), (cap, cap + 7), (cap, -3)} <= seen and ((cap, 1) in seen or cap == 1)
    if n >= 2:
        assert sum(int(R.votes(c["descs"], c["counts"], c["cap"], c["amb"]).sum()) for c in cases[-3:]) > 0


def test_votes_equal_the_model_on_special_frames(nm):
    by = {}
    for c in R.special_cases():
        got, ref = _host_votes(nm, c), R.votes(c["descs"], c["counts"], c["cap"], c["amb"])
        assert np.array_equal(got, ref), (c["what"], got, ref)
        by[c["what"]] = got
    # a frame of one row as candidate: min2 keeps its start value, every query row counts
    assert all(by["one-row candidate, amb %g" % a][0, 1] == 96 and by["one-row candidate, amb %g" % a][2, 1] == 70 for a in R.AMBS)
    # rows 0 .. 47 of frame 0 meet two identical candidates (min2 == 0) and do not count; the other way every row finds its twin once
    dup = by["duplicated candidates, amb 0.8"]
    assert dup[0, 1] <= 48 and dup[1, 0] == 96, dup
    # a frame against its copy: every row at distance 0 from its twin, min2 > 0
    assert all(by["a frame and its copy, amb %g" % a][0, 1] == 96 for a in R.AMBS)
    same = by["two slots, one table, amb 0.8"]
    assert same[0, 2] == 96 and same[2, 0] == 96 and same[0, 1] == same[2, 1] and same[1, 0] == same[1, 2]
    ties = [by["equal distances, amb %g" % a] for a in R.AMBS]
    assert ties[2].sum() > ties[0].sum()        # min1 == min2 fails even ambiguity 1.0, min1 < min2 passes it


def test_same_table_in_two_slots_is_one_pointer(nm):
    """The case above with the SAME array object in both slots, so the two host-table entries are one address."""
    c = [c for c in R.special_cases() if "same" in c][0]
    a, b = c["same"]
    descs = list(c["descs"])
    descs[b] = descs[a]
    got = nm.link_votes_host(descs, c["counts"], ambiguity=c["amb"], cap=c["cap"])
    assert np.array_equal(got, R.votes(descs, c["counts"], c["cap"], c["amb"]))


def test_votes_equal_the_existing_matcher_for_every_ordered_pair(nm):
    descs = R.world_frames(5, 5, 120)
    counts = [120, 77, 1, 64, 33]
    for amb in R.AMBS:
        got = nm.link_votes_host(descs, counts, ambiguity=amb, cap=120)
        for a in range(5):
            for b in range(5):
                if a == b:
                    assert got[a, b] == 0
                    continue
                res = nm.sift_match_u8_host([descs[a]], [counts[a]], [descs[b]], [counts[b]], ambiguity=amb, capA=120, capB=120)
                assert got[a, b] == int((res[0] >= 0).sum()), (amb, a, b)
        assert got.sum() > 0


def test_rank_equals_the_model(nm):
    for c in R.rank_cases():
        kw = {k: c[k] for k in ("min_votes", "min_gap", "per_frame", "max_links")}
        la, lb, ls, cnt = nm.link_rank_host(c["votes"], **kw)
        ra, rb, rs, rcnt = R.rank(c["votes"], **kw)
        assert cnt == rcnt and np.array_equal(la, ra) and np.array_equal(lb, rb) and np.array_equal(ls, rs), c["what"]
        assert (la[cnt:] == -1).all() and (lb[cnt:] == -1).all() and (ls[cnt:] == 0).all(), c["what"]


def test_rank_rules_by_hand(nm):
    """The same rules stated as expected lists, so that the model is not the only witness."""
    links = lambda r: list(zip(r[0][:r[3]].tolist(), r[1][:r[3]].tolist(), r[2][:r[3]].tolist()))
    eq = R.symmetric(4, {(a, b): 9 for a in range(4) for b in range(a + 1, 4)})
    assert links(nm.link_rank_host(eq, 1, 1, 0, 8)) == [(0, 1, 9), (0, 2, 9), (0, 3, 9), (1, 2, 9), (1, 3, 9), (2, 3, 9)]
    assert links(nm.link_rank_host(eq, 1, 2, 0, 8)) == [(0, 2, 9), (0, 3, 9), (1, 3, 9)]
    assert links(nm.link_rank_host(eq, 1, 4, 0, 8)) == []
    assert links(nm.link_rank_host(eq, 9, 1, 0, 2)) == [(0, 1, 9), (0, 2, 9)]
    assert links(nm.link_rank_host(eq, 10, 1, 0, 8)) == []
    asym = R.symmetric(4, {(0, 1): 5, (1, 2): 6, (2, 3): 7})
    asym[0, 3], asym[3, 0] = 90, 2
    assert links(nm.link_rank_host(asym, 1, 1, 0, 8)) == [(2, 3, 7), (1, 2, 6), (0, 1, 5), (0, 3, 2)]
    assert links(nm.link_rank_host(asym, 3, 1, 0, 8)) == [(2, 3, 7), (1, 2, 6), (0, 1, 5)]
    star = R.symmetric(6, {(0, 1): 50, (0, 2): 49, (0, 3): 48, (1, 2): 30, (2, 3): 29, (4, 5): 10, (3, 4): 9, (1, 5): 8})
    # per_frame 1: (0, 2), (0, 3) and (1, 2) are passed over, the walk goes on to (2, 3) and (4, 5)
    assert links(nm.link_rank_host(star, 1, 1, 1, 8)) == [(0, 1, 50), (2, 3, 29), (4, 5, 10)]
    assert links(nm.link_rank_host(star, 1, 1, 2, 8)) == [(0, 1, 50), (0, 2, 49), (1, 2, 30), (4, 5, 10), (3, 4, 9)]
    la, lb, ls, cnt = nm.link_rank_host(np.zeros((7, 7), np.int32), 1, 1, 0, 5)
    assert cnt == 0 and (la == -1).all() and (lb == -1).all() and (ls == 0).all()


def test_refusals_leave_the_outputs_untouched(nm):
    lib = nm.lib()
    cap, n = 8, 2
    descs = [np.zeros((cap, 128), np.uint8) for _ in range(n)]
    counts = [np.array([cap], np.int32) for _ in range(n)]
    tab = lambda arrays: (C.c_void_p * len(arrays))(*[a.ctypes.data if a is not None else None for a in arrays])
    votes = np.full((n, n), -5, np.int32)
    v = votes.ctypes.data
    bad = [(0, tab(descs), tab(counts), cap, v), (65, tab(descs), tab(counts), cap, v), (n, tab(descs), tab(counts), 0, v),
           (n, tab(descs), tab(counts), 1 << 22, v), (n, None, tab(counts), cap, v), (n, tab(descs), None, cap, v),
           (n, tab([descs[0], None]), tab(counts), cap, v), (n, tab(descs), tab([None, counts[1]]), cap, v),
           (n, tab(descs), tab(counts), cap, None)]
    for k, (nn, d, c, cp, out) in enumerate(bad):
        assert lib.nm_link_votes_host_u8(nn, d, c, cp, 0.8, out) == INVALID, k
    assert (votes == -5).all()
    assert lib.nm_link_votes_host_u8(n, tab(descs), tab(counts), cap, 0.8, v) == 0 and (votes == 0).all()
    assert [lib.nm_link_votes_workspace_bytes(*a) for a in ((0, 8), (65, 8), (2, 0), (2, 1 << 22))] == [0, 0, 0, 0]
    assert lib.nm_link_votes_workspace_bytes(3, 33) == 3 * 64 * 4

    mat = np.full((3, 3), 4, np.int32)
    outs = [np.full(4, -5, np.int32) for _ in range(3)] + [np.full(1, -5, np.int32)]
    m, (a, b, s, d) = mat.ctypes.data, [o.ctypes.data for o in outs]
    bad = [(0, m, 1, 1, 0, 4, a, b, s, d), (65, m, 1, 1, 0, 4, a, b, s, d), (3, None, 1, 1, 0, 4, a, b, s, d),
           (3, m, 0, 1, 0, 4, a, b, s, d), (3, m, 1, 0, 0, 4, a, b, s, d), (3, m, 1, 1, -1, 4, a, b, s, d),
           (3, m, 1, 1, 0, 0, a, b, s, d), (3, m, 1, 1, 0, 257, a, b, s, d), (3, m, 1, 1, 0, 4, None, b, s, d),
           (3, m, 1, 1, 0, 4, a, None, s, d), (3, m, 1, 1, 0, 4, a, b, None, d), (3, m, 1, 1, 0, 4, a, b, s, None)]
    for k, args in enumerate(bad):
        assert lib.nm_link_rank_host(*args) == INVALID, k
    assert all((o == -5).all() for o in outs)
    assert lib.nm_link_rank_host(3, m, 1, 1, 0, 4, a, b, s, d) == 0 and outs[3][0] == 3
    with pytest.raises(nm.NmError):
        nm.link_rank_host(mat, min_votes=0)
    with pytest.raises(nm.NmError):
        nm.link_votes_host(descs, [1], cap=cap)


def test_loop_closure_is_found(nm, capsys):
    """What the stage is worth. The inputs' condition is checked on the numpy model first: every overlapping pair scores at
    least min_votes, every other pair below it, with room to spare."""
    L = R.LOOP
    descs, shared = R.loop_frames()
    n, counts = L["frames"], [L["rows"]] * L["frames"]
    model = R.scores(R.votes(descs, counts, L["rows"], L["ambiguity"]))
    low = min(s for p, s in model.items() if p in shared)
    high = max(s for p, s in model.items() if p not in shared)
    with capsys.disabled():
        print("\nloop closure: smallest overlapping score %d, largest non-overlapping score %d, min_votes %d" % (low, high, L["min_votes"]))
    assert low >= 1.5 * L["min_votes"] and 4 * high <= L["min_votes"], (low, high)
    votes = nm.link_votes_host(descs, counts, ambiguity=L["ambiguity"], cap=L["rows"])
    la, lb, ls, cnt = nm.link_rank_host(votes, min_votes=L["min_votes"], min_gap=L["min_gap"])
    got = sorted(zip(la[:cnt].tolist(), lb[:cnt].tolist()))
    assert got == [(0, 10), (0, 11), (1, 11)], got
    assert all(b - a < L["min_gap"] or (a, b) in got for (a, b) in shared)
    # the one-step pair outranks the two-step pairs
    assert (int(la[0]), int(lb[0])) == (0, 11) and ls[0] > ls[1] >= ls[2] >= 1.5 * L["min_votes"]
