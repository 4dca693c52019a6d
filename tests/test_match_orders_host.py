"""The u8 host twins on adversarial candidate ORDERS (tests/match_order_ref.py), array_equal against the numpy restatements
(match_u8_ref, knn_u8_ref at every k in 1 .. 8, mutual_u8_ref in both directions), and a tile-structured numpy MODEL of the
device scan that measures which shared cases can see an order-dependent slip at all. No GPU.

The model (tile_model, for the tests only) is the scan of csrc/nm_match_u8.hip: per 32-row tile the rows go to two lane halves
by half = ((row % 32) // 4) % 2, each half inserts at most R of the tile's keys, smallest first and strict in d, into an
ascending list of L, and the halves are merged at the end by (d, j). With R = L it must equal knn_u8_ref.knn on every shared
case, old and new (test_model_equals_the_restatement). With R = L - 1 it is the kernel that stops its rounds one early
(equally: whose "next key above g1" loses one of several keys of a lane that enter at once). top2_model is the ratio
path's fold_top2; its mutant gives ld[1] the old ld[0] when a tile beats ld[0], without looking at the tile's second key.

A mutant is DETECTED by a family when some case of it has a first-L list (for the top-2 mutant: a matcher result at
ambiguity 0.8, 1.0 or 1.5) that differs from the truth. Measured (print_tables; cases detecting / cases):

    family                   R=L-1, L=2   L=4     L=8     top-2 mutant
    mixed_size_cases         13/18        5/18    1/18    5/18           (old)
    tie_cases                2/2          2/2     0/2     0/2            (old)
    duplicate_cases          0/3          0/3     0/3     0/3            (old)
    shared_scan_cases        2/3          1/3     0/3     2/3            (old)
    descending               1/4          1/4     0/4     1/4
    ascending                3/3          3/3     0/3     3/3
    plateaus_descending      5/5          2/5     1/5     2/5
    last_tile                2/4          0/4     0/4     2/4
    sawtooth, half           3/5          3/5     3/5     3/5
    sawtooth, tile_down/up   1/3          1/3     0/3     1/3

    most keys one lane half places for one query in one tile AFTER the first (test_new_orders_do_the_maximal_work):
    L = 8: old families 7, 7, 6, 1; descending, plateaus_descending and sawtooth-half 8. L = 2 and 4: both reach L.

What the table says, plainly. The old families are NOT blind to a scan that stops one round early, nor to the top-2 mutant:
filling the empty list from the FIRST tile is already L insertions, and with random bytes the L nearest of some query fall
into one lane half of one tile often enough at L = 2 and 4. At L = 8 exactly one old case sees the mutant, 33 x 31, which IS
a single tile; no old case with a second tile does, and no old case ever replaces a whole list of 8 from a later tile (7
at the most). That is the gap: L = 8 behind the first tile. The sawtooth's half form closes it at 44, 76 and 140 candidates
and `plateaus_descending` at 44: there the 8 nearest of every query are keys of one lane half of one later tile, so the
replaced list IS the output (list_from_one_later_tile; no old case and no strictly descending case has that), and the three
ordered families make every tile after the first do L placements at every L.

What `descending` cannot show, for a reason that is arithmetic, not measurement: its order is strict, so its L nearest are
L CONSECUTIVE rows, and consecutive rows change lane half every 4. A block of 8 is always 4 | 4, each half needs 4 <= 7
entries and the merge supplies the eighth: no first-8 output of a strictly descending case can show R = 7. The test asserts
exactly that (CANNOT_DETECT) and that every other (ordered family, L) detects. For the same reason `descending` sees L = 2,
L = 4 and the top-2 mutant only where its nearest rows share one lane half of the last tile: at 36 candidates (rows
32 .. 35). `plateaus_descending` is not bound by this, because ties come out in index order: behind the nearest run the
list goes on with the LOWEST rows of the run before it. Its 44-row case (runs of 32, 8, 4) has the 8 nearest at rows
40 .. 43, 32 .. 35, all keys of lane half 0 of tile 1 -- a whole list of 8 replaced by equal distances from a tile behind the
first -- and shows R = L - 1 at L = 2, 4 and 8 and the top-2 mutant; its 131-row case (nearest run: rows 129, 130) shows
L = 2 and the top-2 mutant. The top-2 mutant is caught by every new ordered family.
"""
import numpy as np
import pytest

import knn_u8_ref as K
import match_order_ref as O
import match_u8_ref as M
import mutual_u8_ref as MU

LIST_INF, NO_ROW, NO_SECOND = 0x7fffffff >> 4, 0x7fffffff, 1 << 24
AMBS = (0.8, 1.0, 1.5)
ORDERED = ("descending", "plateaus_descending", "sawtooth, half")
# strict order: the nearest 8 are consecutive rows, 4 | 4 over the lane halves, see the module docstring
CANNOT_DETECT = {("descending", 8)}


# ---- the model ----
def _half_columns(nB):
    """[(tile, half, columns ascending)] in the order the scan meets them."""
    rows = np.arange(nB)
    return [(t, h, rows[(rows // 32 == t) & (O.half(rows) == h)]) for t in range((nB + 31) // 32) for h in (0, 1)]


def tile_model(D, L, R, k, count=None):
    """(index, distance) (rows, k) int32 of the scan with lists of L and at most R insertions per lane half and tile. count:
    a dict that receives, per tile index, the largest number of keys one half placed for one query."""
    rows, nB = D.shape
    ld = np.full((2, rows, L), LIST_INF, np.int64)
    lj = np.full((2, rows, L), NO_ROW, np.int64)
    at = np.arange(rows)[:, None]
    for t, h, cols in _half_columns(nB):
        if not len(cols):
            continue
        order = np.argsort(D[:, cols], axis=1, kind="stable")       # a lane's keys (d << 4 | e): by d, then by row
        placed = np.zeros(rows, np.int64)
        for r in range(min(R, len(cols))):
            j = cols[order[:, r]]
            d = D[np.arange(rows), j]
            placed += d < ld[h][:, L - 1]
            both_d = np.concatenate([ld[h], d[:, None]], axis=1)    # strict in d: behind every equal entry, out if not below the tail
            both_j = np.concatenate([lj[h], j[:, None]], axis=1)
            keep = np.argsort(both_d, axis=1, kind="stable")[:, :L]
            ld[h], lj[h] = both_d[at, keep], both_j[at, keep]
        if count is not None:
            count[t] = max(count.get(t, 0), int(placed.max()))
    key = np.sort(np.concatenate([ld[0] << 32 | lj[0], ld[1] << 32 | lj[1]], axis=1), axis=1)[:, :k]     # merged by (d, j)
    m = min(k, nB)
    idx, dist = (key & 0xffffffff).astype(np.int64), key >> 32
    idx[:, m:], dist[:, m:] = K.NO_INDEX, K.NO_DISTANCE
    idx[idx == NO_ROW], dist[dist == LIST_INF] = K.NO_INDEX, K.NO_DISTANCE
    return idx.astype(np.int32), dist.astype(np.int32)


def top2_model(D, mutant=False):
    """(min1, index, min2) of fold_top2 per lane half and the merge by (d, j); min2 >= NO_SECOND where there is none."""
    rows, nB = D.shape
    ld = np.full((2, rows, 2), LIST_INF, np.int64)
    lj = np.full((2, rows), NO_ROW, np.int64)
    every = np.arange(rows)
    for t, h, cols in _half_columns(nB):
        if not len(cols):
            continue
        order = np.argsort(D[:, cols], axis=1, kind="stable")
        j1 = cols[order[:, 0]]
        d1 = D[every, j1]
        d2 = D[every, cols[order[:, 1]]] if len(cols) > 1 else np.full(rows, LIST_INF, np.int64)
        best = d1 < ld[h][:, 0]
        second = ~best & (d1 < ld[h][:, 1])
        new1 = np.where(best, ld[h][:, 0] if mutant else np.minimum(ld[h][:, 0], d2), np.where(second, d1, ld[h][:, 1]))
        ld[h][:, 1] = new1
        ld[h][:, 0] = np.where(best, d1, ld[h][:, 0])
        lj[h] = np.where(best, j1, lj[h])
    none = np.full(rows, NO_ROW, np.int64)
    key = np.sort(np.stack([ld[0][:, 0] << 32 | lj[0], ld[0][:, 1] << 32 | none, ld[1][:, 0] << 32 | lj[1],
                            ld[1][:, 1] << 32 | none], axis=1), axis=1)
    return key[:, 0] >> 32, key[:, 0] & 0xffffffff, key[:, 1] >> 32


def top2_results(case, mutant):
    """The matcher's result rows below nA from top2_model, per ambiguity of AMBS."""
    nA, nB = case["nA"], case["nB"]
    m1, ix, m2 = top2_model(M.distances(case["A"][:nA], case["B"][:nB]), mutant)
    idx, dist = np.stack([ix, ix], axis=1), np.stack([m1, np.where(m2 >= NO_SECOND, 0, m2)], axis=1)
    prior = np.full(nA, case["prior"], np.int32)
    step = lambda amb, no_second: K.matcher_last_step(idx, dist, 1 if no_second else 2, amb, prior)      # 1: min2 = its start value
    return [np.where(m2 >= NO_SECOND, step(amb, True), step(amb, False)) for amb in AMBS]


def _sized(case):
    """A case cut to its sizes (the model has no capacities)."""
    nA, nB = case["nA"], case["nB"]
    return dict(case, A=case["A"][:nA], B=case["B"][:nB])


def shared_families():
    """{name: cases} of every shared k-NN / matcher family with rows, the old ones first."""
    old = {"mixed_size_cases": M.mixed_size_cases(), "tie_cases": list(K.tie_cases()), "duplicate_cases": M.duplicate_cases(),
           "shared_scan_cases": M.shared_scan_cases()[0]}
    new = {f: O.family_cases(f) for f in O.FAMILIES if f != "sawtooth"}
    new["sawtooth, half"] = O.many_insertion_cases()
    new["sawtooth, tile_down/up"] = [c for c in O.family_cases("sawtooth") if c["form"] != "half"]
    fam = dict(old, **new)
    return {name: [_sized(c) for c in cases if c["nA"] > 0 and c["nB"] > 0] for name, cases in fam.items()}, tuple(old)


_FAMILIES = {}


def families():
    if not _FAMILIES:
        fam, old = shared_families()
        _FAMILIES.update(fam=fam, old=old, D={id(c): M.distances(c["A"], c["B"]) for cs in fam.values() for c in cs})
    return _FAMILIES["fam"], _FAMILIES["old"], _FAMILIES["D"]


def knn_mutant_detected(case, D, L):
    want = K.knn(D, L)
    got = tile_model(D, L, L - 1, L)
    return not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))


def top2_mutant_detected(case):
    return any(not np.array_equal(a, b) for a, b in zip(top2_results(case, True), top2_results(case, False)))


_TABLE = {}


def mutant_table():
    """{family: {2: (detecting, cases), 4: .., 8: .., "top2": ..}}"""
    if not _TABLE:
        fam, _, Ds = families()
        for name, cases in fam.items():
            row = {L: (sum(knn_mutant_detected(c, Ds[id(c)], L) for c in cases), len(cases)) for L in (2, 4, 8)}
            row["top2"] = (sum(top2_mutant_detected(c) for c in cases), len(cases))
            _TABLE[name] = row
    return _TABLE


def print_tables():
    fam, old, _ = families()
    print("%-24s %-12s %-7s %-7s %s" % ("family", "R=L-1, L=2", "L=4", "L=8", "top-2 mutant"))
    for name, row in mutant_table().items():
        cell = lambda key: "%d/%d" % row[key]
        print("%-24s %-12s %-7s %-7s %-14s %s" % (name, cell(2), cell(4), cell(8), cell("top2"), "(old)" if name in old else ""))


def rounds_after_first_tile(cases, Ds, L):
    """The most keys one lane half places for one query in one tile AFTER the first, over the cases."""
    most = 0
    for c in cases:
        count = {}
        tile_model(Ds[id(c)], L, L, L, count)
        most = max([most] + [v for t, v in count.items() if t > 0])
    return most


def list_from_one_later_tile(D, L):
    """True when the L nearest of EVERY query are keys of one lane half of one tile behind the first: that half's whole list
    is replaced by that tile, and every entry of it reaches the output (the other half can supply none)."""
    nearest = np.argsort(D, axis=1, kind="stable")[:, :L]
    return D.shape[1] >= L and bool(((nearest // 32 == nearest[:, :1] // 32) & (nearest[:, :1] >= 32) &
                                     (O.half(nearest) == O.half(nearest[:, :1]))).all())


# ---- the model is the restatement; what the mutants show ----
@pytest.mark.parametrize("L", [1, 2, 4, 8])
def test_model_equals_the_restatement(L):
    fam, _, Ds = families()
    for name, cases in fam.items():
        for c in cases:
            for k in sorted({L, L // 2 + 1}):
                want = K.knn(Ds[id(c)], k)
                got = tile_model(Ds[id(c)], L, L, k)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, c["what"], L, k)


def test_top2_model_equals_the_restatement():
    fam, _, _ = families()
    for name, cases in fam.items():
        for c in cases:
            for amb, got in zip(AMBS, top2_results(c, False)):
                assert np.array_equal(got, M.expected(dict(c, amb=amb), c["nA"])), (name, c["what"], amb)


def test_ordered_families_detect_the_mutants():
    """Nothing is asserted about the old families; their figures are printed, and kept in the module docstring."""
    print_tables()
    table = mutant_table()
    for name in ORDERED:
        for L in (2, 4, 8):
            assert (table[name][L][0] > 0) == ((name, L) not in CANNOT_DETECT), (name, L, table[name][L])
        assert table[name]["top2"][0] > 0, (name, "top-2 mutant")


def test_new_orders_do_the_maximal_work():
    """Placements per lane half, query and tile after the first: L in descending, plateaus_descending and sawtooth's half
    form (a whole list replaced by one tile), 0 in ascending, 1 in tile_down. The old families' figure is printed."""
    fam, old, Ds = families()
    for L in (2, 4, 8):
        print("L = %d: most placements in a tile after the first:" % L,
              ", ".join("%s %d" % (name, rounds_after_first_tile(cases, Ds, L)) for name, cases in fam.items()))
        for name in ORDERED:
            assert rounds_after_first_tile(fam[name], Ds, L) == L, (name, L)
        assert rounds_after_first_tile(fam["ascending"], Ds, L) == 0
        for c in fam["sawtooth, tile_down/up"]:
            assert rounds_after_first_tile([c], Ds, L) == (1 if c["form"] == "tile_down" else 0), (c["what"], L)
    # where the 8 placements land: a list of 8 that one later tile replaced AND that is the output
    through = {name: [c["what"] for c in cases if list_from_one_later_tile(Ds[id(c)], 8)] for name, cases in fam.items()}
    print("L = 8, the whole output from one lane half of one later tile:", {n: w for n, w in through.items() if w})
    assert not any(through[name] for name in old) and not through["descending"]
    assert len(through["plateaus_descending"]) == 1 and "x 44" in through["plateaus_descending"][0]
    assert len(through["sawtooth, half"]) == 3
    for name, cases in fam.items():                             # and it is exactly these that show R = 7 behind the first tile
        for c in cases:
            if c["nB"] > 32:
                assert knn_mutant_detected(c, Ds[id(c)], 8) == (c["what"] in through[name]), c["what"]


# ---- the host twins ----
def _col(cases, key):
    return [c[key] for c in cases]


@pytest.mark.parametrize("family", O.FAMILIES)
def test_matcher_twin_equals_restatement(nm, family):
    cases = O.family_cases(family)
    seen = set()
    for amb in AMBS:
        got = nm.sift_match_u8_host(_col(cases, "A"), _col(cases, "nA"), _col(cases, "B"), _col(cases, "nB"), ambiguity=amb,
                                    capA=O.CAP_A, capB=O.CAP_B, prior=-7)
        for p, c in enumerate(cases):
            want = M.expected_clipped(dict(c, amb=amb), O.CAP_A, O.CAP_B)
            assert np.array_equal(got[p], want), (c["what"], amb)
            assert (got[p][c["nA"]:] == -7).all()
            seen |= set(np.unique(got[p][:c["nA"]]).tolist())
    assert -1 in seen and max(seen) >= 0, "the family's results are all matches or all rejections"


@pytest.mark.parametrize("k", range(1, 9))
def test_knn_twin_equals_restatement(nm, k):
    cases = O.all_cases()
    idx, dist = nm.sift_match_knn_u8_host(_col(cases, "A"), _col(cases, "nA"), _col(cases, "B"), _col(cases, "nB"), k,
                                          capA=O.CAP_A, capB=O.CAP_B, prior=K.PRIOR)
    only, none = nm.sift_match_knn_u8_host(_col(cases, "A"), _col(cases, "nA"), _col(cases, "B"), _col(cases, "nB"), k,
                                           capA=O.CAP_A, capB=O.CAP_B, want_distance=False, prior=K.PRIOR)
    assert none is None
    for p, c in enumerate(cases):
        wi, wd = K.expected(c, k, O.CAP_A, O.CAP_B)
        assert np.array_equal(idx[p], wi) and np.array_equal(dist[p], wd) and np.array_equal(only[p], wi), (c["what"], k)
        if c["family"] == "descending":
            assert (idx[p][:c["nA"]] == c["nB"] - 1 - np.arange(k)).all(), c["what"]


def test_knn_twin_on_permuted_candidates(nm):
    for c in (O.family_cases("descending")[2], M.random_case(47, 65, 129)):
        p, source = O.permuted(c, 3)
        capA, capB = len(c["A"]), len(c["B"])
        a = nm.sift_match_knn_u8_host([c["A"]], [c["nA"]], [c["B"]], [c["nB"]], 8, capA=capA, capB=capB)
        b = nm.sift_match_knn_u8_host([p["A"]], [p["nA"]], [p["B"]], [p["nB"]], 8, capA=capA, capB=capB)
        nA = c["nA"]
        assert np.array_equal(source[b[0][0][:nA]], a[0][0][:nA]) and np.array_equal(b[1][0], a[1][0]), c["what"]


@pytest.mark.parametrize("family", O.FAMILIES)
def test_mutual_twin_equals_restatement_in_both_directions(nm, family):
    for c in O.family_cases(family):
        for way, m in enumerate(O.mutual_cases(c)):
            capA, capB = len(m["A"]), len(m["B"])
            res, cnt, fwd = nm.sift_match_mutual_u8_host([m["A"]], [m["nA"]], [m["B"]], [m["nB"]], [m["m"]], capA=capA,
                                                         capB=capB, want_distance=True)
            want, wcount, wfwd = MU.expected(m, capA, capB)
            assert np.array_equal(res[0], want) and cnt[0] == wcount, m["what"]
            assert np.array_equal(fwd[0].view(np.uint32), wfwd.view(np.uint32)), m["what"]
            MU.kept_removed([m], capA, capB)
            if family == "descending" and way == 0:             # every query names the last row; the first nearest query stays
                assert (m["m"][:m["nA"]] == m["nB"] - 1).all() and wcount == 1
                survivor = int(M.distances(m["A"][:m["nA"]], m["B"][m["nB"] - 1:m["nB"]])[:, 0].argmin())
                assert np.flatnonzero(res[0] >= 0).tolist() == [survivor] and res[0][survivor] == m["nB"] - 1
