"""Candidate ORDERS for the brute-force matchers: the cases tests/test_match_orders_host.py and tests/test_gpu_match_orders.py
share. Plain numpy on match_u8_ref._case and match_u8_ref.distances; no restatement of any entry lives here (the references
stay match_u8_ref.expected, knn_u8_ref.expected, mutual_u8_ref and, for fp32, the oracle).

Every other shared case of the matchers is random bytes in random order. A list, top-2 or threshold scan is sensitive to the
order in which candidates arrive, so here the order is the case. How an order is made to hold for every query at once:

  one base row of 128 bytes in [60, 195];
  a query is the base row with a perturbation e_i on bytes 0 .. 31 only (amplitude 0 .. 3; amplitude 0 makes identical
  queries, which the mutual filter must break by index);
  a candidate is the base row with steps of at most 55 on bytes 32 .. 127 only, chosen so that |candidate - base|^2 is
  EXACTLY a wanted integer v_j (a greedy sum of squares).

The two supports are disjoint, so D[i, j] = |e_i|^2 + v_j with no cross term: a gap between two candidates is the same
integer for every query, the perturbation moves it by exactly zero, and the order of the v_j is the order of every row of
D. Exact ties are identical rows (equal v_j give identical bytes). The nearest levels are 10 g, 13 g, then steps of g .. 2 g
(g = 16 unless said), so that min1 / min2 < 0.8 holds for the queries with |e_i|^2 < 2 g and fails for the others, and a
second distance taken from a few ranks further accepts queries the matcher must reject.

Every generator asserts with distances() that its case has the property it is named after, for EVERY query row. All cases
sit in buffers of CAP_A x CAP_B rows, larger than every size: the rows of A beyond nA are random bytes, the rows of B at nB
and nB + 1 are the base row and a row one step from it (nearer to every query than any candidate: reading one changes every
list), the rest random bytes.

Lane halves: the device scan gives the rows of a 32-row tile to two lane halves, half(row) = ((row % 32) // 4) % 2 (acc_row
in csrc/nm_match_u8_dev.hpp), each with a list of its own, merged at the end. A block of consecutive rows alternates halves
every 4 rows; the sawtooth's "half" form is built on that map.
"""
import math

import numpy as np

import match_u8_ref as M

CAP_A, CAP_B = 300, 264
QUERY_BYTES = 32                      # bytes 0 .. 31 carry the query perturbation, bytes 32 .. 127 the candidate steps
STEP_MAX = 55
GAP = 16
FAMILIES = ("descending", "ascending", "plateaus_descending", "last_tile", "sawtooth")
PLATEAU_WIDTHS = (4, 8, 16, 1, 33, 1, 1, 32, 33)      # one cycle is 129 rows; see plateaus_descending


def half(row):
    return ((np.asarray(row) % 32) // 4) % 2


def _base(rng):
    return rng.integers(60, 196, 128)


def rows_at(base, values, sign):
    """One row per value v: the base row moved on bytes 32 .. 127 so that |row - base|^2 == v exactly. Equal values give
    identical rows."""
    out = np.tile(np.asarray(base, np.int64), (len(values), 1))
    memo = {}
    for r, v in enumerate(values):
        v = int(v)
        if v not in memo:
            delta, rem = np.zeros(128 - QUERY_BYTES, np.int64), v
            for c in range(len(delta)):
                if rem == 0:
                    break
                delta[c] = min(STEP_MAX, math.isqrt(rem))
                rem -= int(delta[c]) ** 2
            assert rem == 0, ("a distance too large for 96 steps of 55", v)
            memo[v] = delta * sign
        out[r, QUERY_BYTES:] += memo[v]
    assert out.min() >= 0 and out.max() <= 255
    return out


def levels(rng, n, gap=GAP):
    """n strictly ascending distances: 10 gap, 13 gap, then steps of gap .. 2 gap."""
    steps = rng.integers(gap, 2 * gap + 1, max(n - 1, 0))
    steps[:1] = 3 * gap
    return 10 * gap + np.concatenate([[0], np.cumsum(steps)]).astype(np.int64)[:n]


def queries(rng, base, nA):
    amp = rng.integers(0, 4, nA)
    amp[3:nA:29] = 0                                            # identical queries: rows 3, 32, 61, ..
    A = np.tile(np.asarray(base, np.int64), (nA, 1))
    A[:, :QUERY_BYTES] += rng.integers(-1, 2, (nA, QUERY_BYTES)) * amp[:, None]
    return A


def _build(rng, base, values, nA, family, what, gap=GAP, capA=CAP_A, capB=CAP_B, B_rows=None):
    """The case of candidates at the distances `values` (or the rows B_rows) in buffers of capA x capB rows."""
    nB = len(values) if B_rows is None else len(B_rows)
    assert 0 < nA <= capA and 0 < nB <= capB
    sign = rng.choice((-1, 1), 128 - QUERY_BYTES)
    A = rng.integers(0, 256, (capA, 128))
    A[:nA] = queries(rng, base, nA)
    B = rng.integers(0, 256, (capB, 128))
    B[:nB] = rows_at(base, values, sign) if B_rows is None else B_rows
    if nB < capB:
        B[nB] = base
    if nB + 1 < capB:
        B[nB + 1] = base
        B[nB + 1, 127] += 1
    c = M._case(A, B, nA=nA, nB=nB, what="%s, %s, %d x %d" % (family, what, nA, nB))
    c["family"] = family
    D = M.distances(c["A"][:nA], c["B"][:nB])
    if nB < capB:                                               # the rows behind nB are nearer than every candidate
        assert (M.distances(c["A"][:nA], c["B"][nB:nB + 2]).max(1) < D.min(1)).all()
    return c, D


def _strict(D):
    """Pairwise distinct distances in every row (what permuted() needs, and more than it needs)."""
    s = np.sort(D, axis=1)
    return bool((np.diff(s, axis=1) > 0).all())


def descending(nA, nB, seed=0, gap=GAP, capA=CAP_A, capB=CAP_B):
    """D[i, j] strictly decreasing in j for every i: every tile beats everything before it, each lane replaces its whole
    list in every tile; the nearest row is nB - 1."""
    rng = np.random.default_rng(500 + seed)
    c, D = _build(rng, _base(rng), levels(rng, nB, gap)[::-1], nA, "descending", "strict", gap, capA, capB)
    assert (np.diff(D, axis=1) < 0).all() and (D.argmin(1) == nB - 1).all()
    return c


def ascending(nA, nB, seed=0):
    """D[i, j] strictly increasing in j: after the first tile no lane ever beats its list tail."""
    rng = np.random.default_rng(520 + seed)
    c, D = _build(rng, _base(rng), levels(rng, nB), nA, "ascending", "strict")
    assert (np.diff(D, axis=1) > 0).all() and (D.argmin(1) == 0).all()
    return c


ONE_HALF_WIDTHS = (32, 8, 4)                          # 44 rows: the nearest run 40 .. 43 and the head 32 .. 35 of the run before
                                                      # it are the 8 nearest, all keys of lane half 0 of tile 1


def plateau_runs(nB, widths=PLATEAU_WIDTHS):
    """[(first row, width)] of the runs: `widths` over and over from row 0, the last run cut at nB. PLATEAU_WIDTHS from row 0:
    4 (rows 0 .. 3: inside lane half 0), 8 (4 .. 11: both halves of a tile), 16, 1, 33 (29 .. 61: across 31 | 32), 1, 1,
    32 (64 .. 95: a whole tile), 33 (96 .. 128), then the same widths from row 129, where nothing is aligned."""
    runs, row = [], 0
    while row < nB:
        for w in widths:
            if row < nB:
                runs.append((row, min(w, nB - row)))
                row += w
    return runs


def plateaus_descending(nA, nB, seed=0, widths=PLATEAU_WIDTHS):
    """Runs of IDENTICAL candidate rows, each run nearer than the one before: a tile's keys tie, a whole list is replaced by
    equal distances, and those must come out in index order. The nearest run is the last one; its rows are the head of every
    k-NN list, lowest index first, and the list goes on with the LOWEST rows of the run before it: the k nearest need not be
    consecutive rows. With ONE_HALF_WIDTHS at 44 rows the 8 nearest are rows 40 .. 43, 32 .. 35: one tile, one lane half, a
    whole list of 8 replaced by two equal distances, and no entry of it can come from the other half."""
    rng = np.random.default_rng(540 + seed)
    runs = plateau_runs(nB, widths)
    lv = levels(rng, len(runs))[::-1]
    c, D = _build(rng, _base(rng), np.repeat(lv, [w for _, w in runs]), nA, "plateaus_descending", "%d runs" % len(runs))
    for t, (r0, w) in enumerate(runs):
        assert (D[:, r0:r0 + w] == D[:, r0:r0 + 1]).all() and (c["B"][r0:r0 + w] == c["B"][r0]).all()
        assert t == 0 or (D[:, r0] < D[:, runs[t - 1][0]]).all()
    if widths == ONE_HALF_WIDTHS:
        assert nB == 44
        nearest = np.argsort(D, axis=1, kind="stable")[:, :8]
        assert (nearest == [40, 41, 42, 43, 32, 33, 34, 35]).all() and (half(nearest) == 0).all() and (nearest // 32 == 1).all()
    elif nB >= 129:                                             # the placements the family is for
        inside = [(r, w) for r, w in runs if 1 < w <= 4 and len(set(half(np.arange(r, r + w)).tolist())) == 1]
        both = [(r, w) for r, w in runs if w <= 16 and r // 32 == (r + w - 1) // 32 and len(set(half(np.arange(r, r + w)).tolist())) == 2]
        tile = [(r, w) for r, w in runs if r % 32 == 0 and w == 32]
        across = [(r, w) for r, w in runs if r <= 31 < 32 < r + w]
        assert inside and both and tile and across and {w for _, w in runs} >= {1, 4, 8, 16, 32, 33}
        assert inside[0][0] % 8 < 3
    c["runs"] = runs
    return c


def last_tile(nA, nB, second_at_row_0=False, seed=0, capA=CAP_A, capB=CAP_B):
    """Random candidates, except that the nearest of every query is row nB - 1 and the second nearest row nB - 2 (or row 0):
    in every case of family_cases the partial last tile holds two rows or more, so that row nB - 1 and row nB - 2 both sit
    in it beside padded rows (34: rows 32, 33; 70: rows 64 .. 69)."""
    assert nB >= 3
    rng = np.random.default_rng(560 + seed + int(second_at_row_0))
    base = _base(rng)
    sign = rng.choice((-1, 1), 128 - QUERY_BYTES)
    B = rng.integers(0, 256, (nB, 128))
    second = 0 if second_at_row_0 else nB - 2
    near = rows_at(base, levels(rng, 2), sign)
    B[nB - 1], B[second] = near[0], near[1]
    c, D = _build(rng, base, None, nA, "last_tile", "second nearest at row %d" % second, capA=capA, capB=capB, B_rows=B)
    order = np.argsort(D, axis=1, kind="stable")
    assert (order[:, 0] == nB - 1).all() and (order[:, 1] == second).all() and (D[:, second] > D[:, nB - 1]).all()
    assert (np.sort(D, axis=1)[:, 2] > 4 * D[:, second]).all()          # everything else is far
    return c


def sawtooth(nA, nB, form, seed=0):
    """Three zigzags, all with pairwise distinct distances.
      "half"       a tooth every 8 rows: the rows of lane half 0 strictly descend over the whole case and are nearer than
                   every row of half 1, whose rows ascend. Half 0 replaces its whole list in every tile (L insertions per
                   tile, from one lane half only), half 1 never inserts after the first tile, and the k nearest of every
                   query all sit in ONE half: the merge of the halves cannot hide an entry that half lost.
      "tile_down"  ascending inside each tile, descending from tile to tile: the first row of a tile is nearer than
                   everything before it, its other rows farther than every tile's first row and farther than the tile
                   before: one insertion per tile, in every tile.
      "tile_up"    descending inside each tile, ascending from tile to tile: a tile's smallest key is its LAST row, and no
                   tile after the first places a key."""
    rng = np.random.default_rng(580 + seed + len(form))
    rows = np.arange(nB)
    v = np.zeros(nB, np.int64)
    if form == "half":
        h0 = np.flatnonzero(half(rows) == 0)
        h1 = np.flatnonzero(half(rows) == 1)
        lv = levels(rng, nB)
        v[h0] = lv[:len(h0)][::-1]
        v[h1] = lv[len(h0):]
    elif form == "tile_down":
        first = rows[rows % 32 == 0]
        rest = rows[rows % 32 != 0]
        lv = levels(rng, nB)
        v[first] = lv[:len(first)][::-1]
        v[rest] = lv[len(first):]
    elif form == "tile_up":
        lv = levels(rng, nB)
        for t in range(0, nB, 32):
            v[t:t + 32] = lv[t:t + 32][::-1]
    else:
        raise ValueError(form)
    c, D = _build(rng, _base(rng), v, nA, "sawtooth", form)
    c["form"] = form
    assert _strict(D)
    d = D[0]                                                    # one order for every query: check it on all, name it on row 0
    assert (np.argsort(D, axis=1) == np.argsort(d)[None, :]).all()
    if form == "half":
        h0, h1 = rows[half(rows) == 0], rows[half(rows) == 1]
        assert (np.diff(D[:, h0], axis=1) < 0).all() and (np.diff(D[:, h1], axis=1) > 0).all()
        assert (D[:, h0].max(1) < D[:, h1].min(1)).all()
        assert (half(np.argsort(D, axis=1)[:, :min(8, len(h0))]) == 0).all()
    elif form == "tile_down":
        first = rows % 32 == 0
        assert (np.diff(D[:, first], axis=1) < 0).all() and (D[:, first].max(1) < D[:, ~first].min(1)).all()
        for t in range(0, nB, 32):
            assert (np.diff(D[:, t:t + 32], axis=1) > 0).all() and (t == 0 or (D[:, t + 1:t + 32].min(1, initial=1 << 40) > D[:, t - 32:t].max(1)).all())
    else:
        for t in range(0, nB, 32):
            assert (np.diff(D[:, t:t + 32], axis=1) < 0).all() and (t == 0 or (D[:, t:t + 32].min(1) > D[:, t - 32:t].max(1)).all())
    return c


def family_cases(family):
    """The cases of one family, all in CAP_A x CAP_B buffers. nA is one row past a wave (65) or past a workgroup (257); nB is
    one row into the second, the fifth and the ninth tile (33, 129, 257), 70 where a partial last tile with several rows is
    wanted, and the sizes at which the nearest rows of a family share ONE lane half of the last tile, so that the merge of the
    halves cannot supply what that half lost: 36 for `descending` (rows 32 .. 35), 131 (its nearest run is rows 129, 130:
    r % 8 < 3) and 44 with ONE_HALF_WIDTHS for `plateaus_descending`, 44, 76 and 140 for the sawtooth's half form (12 rows in
    the last tile, 8 of them in half 0); 34 for `last_tile` (two rows in the partial tile)."""
    if family == "descending":
        return [descending(65, 33), descending(257, 36, 1), descending(65, 129, 2), descending(257, 257, 3)]
    if family == "ascending":
        return [ascending(257, 33), ascending(65, 129, 1), ascending(65, 257, 2)]
    if family == "plateaus_descending":
        return [plateaus_descending(65, 33), plateaus_descending(257, 44, 4, ONE_HALF_WIDTHS), plateaus_descending(257, 129, 1),
                plateaus_descending(65, 131, 3), plateaus_descending(65, 257, 2)]
    if family == "last_tile":
        cases = [last_tile(65, 70), last_tile(257, 70, True), last_tile(65, 34, False, 1), last_tile(65, 34, True, 1)]
        assert all(c["nB"] % 32 >= 2 for c in cases)
        return cases
    if family == "sawtooth":
        return [sawtooth(257, 33, "half"), sawtooth(65, 44, "half", 1), sawtooth(257, 76, "half", 3), sawtooth(65, 140, "half", 4),
                sawtooth(65, 257, "half", 2),
                sawtooth(65, 129, "tile_down"), sawtooth(257, 257, "tile_down", 1), sawtooth(65, 129, "tile_up")]
    raise ValueError(family)


def all_cases():
    return [c for f in FAMILIES for c in family_cases(f)]


def many_insertion_cases():
    """sawtooth in its many-insertions form."""
    return [c for c in family_cases("sawtooth") if c["form"] == "half"]


def permuted(case, seed):
    """The case with its nB candidates shuffled. Returns (case, source): row r of the new candidates is row source[r] of the
    old ones. Needs the 9 smallest distances of every query to be pairwise distinct (asserted): then the k <= 8 index lists
    of the two cases map onto each other through `source` and the distance lists are equal, whatever the matcher is."""
    nA, nB = case["nA"], case["nB"]
    s = np.sort(M.distances(case["A"][:nA], case["B"][:nB]), axis=1)[:, :9]
    assert (np.diff(s, axis=1) > 0).all(), "permuted() needs distinct nearest distances"
    source = np.random.default_rng(600 + seed).permutation(nB)
    assert (source != np.arange(nB)).sum() > nB // 2
    B = case["B"].copy()
    B[:nB] = case["B"][:nB][source]
    c = dict(case, B=B, what=case["what"] + ", permuted %d" % seed)
    return c, source


def mutual_cases(case):
    """The case as two inputs of the u8 mutual filter, dicts of mutual_u8_ref's kind: (forward, swapped). Forward: every
    query claims its nearest candidate (the u8 matcher's restatement at ambiguity 1.5; a row it leaves unwritten claims
    nothing), the entries beyond nA name real columns. Swapped: A and B change places, so the filter's own scan, which runs
    over the rows of A, meets the family's order."""
    out = []
    for A, nA, B, nB in ((case["A"], case["nA"], case["B"], case["nB"]), (case["B"], case["nB"], case["A"], case["nA"])):
        m = M.expected(dict(A=A, B=B, nA=nA, nB=nB, amb=1.5, prior=-7), len(A))
        m[nA:] = np.arange(len(A) - nA) % nB
        out.append(dict(A=A, B=B, m=m.astype(np.int32), nA=nA, nB=nB, what=case["what"] + (", swapped" if out else ", forward")))
    return out


def ragged_batch():
    """16 pairs in the CAP_A x CAP_B buffers, the families mixed across the slots, slot 8 empty (nB = 0)."""
    cases = all_cases()
    pick = [cases[i] for i in np.random.default_rng(610).permutation(len(cases))[:16]]
    assert {c["family"] for c in pick} == set(FAMILIES)
    pick[8] = dict(pick[8], nB=0, what=pick[8]["what"] + ", emptied")
    return pick
