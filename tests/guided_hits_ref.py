"""Gate-HIT PATTERNS for homography-guided matching: the cases tests/test_match_guided_hits_host.py and
tests/test_gpu_match_guided_hits.py share. Plain numpy; the references stay guided_ref.guided and the host twin. restate()
below is a third statement of the same result in integers, for the generators' own checks.

The device kernel (csrc/nm_match_guided.hip) does not follow a gate hit at once: a lane notes it in a list of LIST entries,
and the whole wave computes its noted distances when any lane's list is full, tested after every gate test of a chunk of
CHUNK, and once more after the last tile of TILE candidates. Random coordinates meet that machinery by chance, so here the
pattern of hits is the case, and every gate outcome is decided by construction:

  H is the identity or the integer translation SHIFT. Source row i sits at (100 (i % 32), 100 (i // 32)) unless a family
  moves it on purpose (always by a few integer pixels, onto or next to another row's point), a candidate sits on a point at
  a small integer offset, a candidate nobody owns is parked at PARK. All coordinates but PARK are integers below 2^12, so
  project() and gate() are exact in binary32: at radius2 = 6 offset (0, 0) gives 0 and hits, (2, 1) gives 5 and hits,
  (2, 2) gives 8 and misses; at radius2 = 5 offset (2, 1) misses, by the strict <.

  Distances as in tests/match_order_ref.py: a query is one base row moved by +-1 on e2_i of the elements 0 .. 31, a
  candidate the base row moved on elements 32 .. 127 to an exactly chosen squared distance v_j (match_order_ref.rows_at),
  all small integers held in float32. D[i, j] = e2_i + v_j is an exact integer below 2^24 and distance128's fma chain is
  exact.

Every case lies in buffers of CAP_A x CAP_B rows. Rows nA .. CAP_A - 1 are copies of live rows (coordinates and
descriptors: they would match), candidates nB .. CAP_B - 1 are copies of live QUERY rows on those rows' points: distance 0,
nearer than any real candidate. A read beyond either count changes a result, and _build asserts that it would.

Every generator asserts its own property before it returns (_build for what all share: the intended hit sets against a
float64 gate on the stored coordinates, D against e2 + v in int64, the tails; note_slots() for which list entry a hit
lands in and where the wave's distance rounds fall).
"""
from fractions import Fraction

import numpy as np

import match_order_ref as MO

CAP_A, CAP_B = 300, 1100
TB, WAVE, TILE, CHUNK, LIST = 256, 64, 1024, 8, 4       # csrc/nm_match_guided.hip
R2 = 6.0
INF = float("inf")
MIN2_INIT = 2139095040
PARK = (-5000, -5000)
EYE, SHIFT = (0, 0), (40, 24)
HIT = ((0, 0), (2, 1), (1, 2), (-2, 1), (1, -1), (-1, -2), (0, 2), (-2, 0), (1, 0), (0, 1))     # every |o|^2 <= 5
MISS = (2, 2)
# eight candidates around a point that hit it AND the point one pixel to its left (an invalid row's (-1, y))
BOTH = ((0, 0), (1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 0), (0, 2))
FAMILIES = ("chunk_burst", "hit_counts", "tile_edge", "scan_order", "ragged_rows", "shared_point")


def grid(rows):
    rows = np.asarray(rows)
    return np.stack([100 * (rows % 32), 100 * (rows // 32)], -1).astype(np.int64)


def _norm2(o):
    return int(o[0]) ** 2 + int(o[1]) ** 2


def note_slots(hits, L=LIST):
    """A count-only walk of the noting, one wave (64 consecutive rows) at a time: every hit goes to entry cnt of its lane's
    list, and when any lane of the wave holds L the wave's round runs and every count returns to 0. hits: {row: [j]}.
    Returns ({(row, j): (entry, number of the round that computes it)}, {wave: [j after which a round ran .., "end"]})."""
    where, rounds = {}, {}
    for w in sorted({r // WAVE for r in hits if hits[r]}):
        rows = [r for r in sorted(hits) if r // WAVE == w and hits[r]]
        cnt, n, ran = dict.fromkeys(rows, 0), 0, []
        for j in sorted({j for r in rows for j in hits[r]}):
            for r in rows:
                if j in hits[r]:
                    where[(r, j)] = (cnt[r], n)
                    cnt[r] += 1
            if any(c == L for c in cnt.values()):
                ran.append(j)
                n += 1
                cnt = dict.fromkeys(rows, 0)
        if any(cnt.values()):
            ran.append("end")
        rounds[w] = ran
    return where, rounds


# ---- the integer restatement ----
def gate64(c, radius2, rows=None, every_row=False):
    """(capA, capB) bool from the STORED coordinates in float64 (all integers: exact). Rows at or beyond nA, invalid rows
    (ax < 0, unless every_row) and candidates at or beyond nB pass nothing."""
    H = np.asarray(c["H"], np.float64)
    px, py = c["ax"].astype(np.float64) + H[2], c["ay"].astype(np.float64) + H[5]
    ex = c["bx"].astype(np.float64)[None, :] - px[:, None]
    ey = c["by"].astype(np.float64)[None, :] - py[:, None]
    G = ex * ex + ey * ey < radius2
    if not every_row:
        G &= (c["ax"] >= 0)[:, None]
    G[c["nA"]:] = False
    G[:, c["nB"]:] = False
    return G


def distances64(c):
    """(capA, capB) int64 squared distances of the stored descriptors (float64 products of small integers: exact)."""
    A, B = c["A"].astype(np.float64), c["B"].astype(np.float64)
    D = (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * (A @ B.T)
    assert (D == np.rint(D)).all() and D.min() >= 0 and D.max() < 1 << 24
    return D.astype(np.int64)


def scan_int(ds):
    """get_sift_matches over one row's gated distances in ascending candidate order, in Python integers:
    (local index, min1, min2); min2 is MIN2_INIT while the row has met one candidate only."""
    idx, min1, min2 = 0, int(ds[0]), MIN2_INIT
    for k in range(1, len(ds)):
        d = int(ds[k])
        if d < min1:
            min2, idx, min1 = min1, k, d
        elif d < min2:
            min2 = d
    return idx, min1, min2


def accepts(min1, min2, ambiguity, max_distance):
    """The decision on exact integers: min2 > 0, fl32(min1 / min2) < fl32(ambiguity), min1 < fl32(max_distance)."""
    if not min2 > 0:
        return False
    ratio = np.float32(min1) / np.float32(min2)
    return bool(ratio < np.float32(ambiguity) and np.float32(min1) < np.float32(max_distance))


def restate(c, radius2, ambiguity, max_distance, nA=None, nB=None):
    """(result (capA,) int32, count, best (capA,) float32) of one case at the given sizes (default: its own)."""
    c = dict(c, nA=c["nA"] if nA is None else nA, nB=c["nB"] if nB is None else nB)
    G, D = gate64(c, radius2), c["D"]
    result, best = np.full(CAP_A, -1, np.int32), np.full(CAP_A, np.inf, np.float32)
    if c["status"] != 1:
        return result, 0, best
    for i in np.flatnonzero(G.any(1)):
        js = np.flatnonzero(G[i])
        loc, min1, min2 = scan_int(D[i, js])
        best[i] = min1
        if accepts(min1, min2, ambiguity, max_distance):
            result[i] = js[loc]
    return result, int((result >= 0).sum()), best


# ---- the builder ----
def _build(family, what, seed, nA, nB, pts, cand, v, hits, runs, shift=EYE, e2=None, invalid_hits=None):
    """pts (nA, 2): the integer points of the live rows, x = -1 for an invalid row. cand (nB, 2): the integer places of the
    candidates (PARK for a parked one), both BEFORE the shift, which moves every candidate that is not parked. v (nB,): the
    exact squared distances from the base row. hits {row: [j ascending]}: what the family intends at R2. invalid_hits: what
    the invalid rows WOULD hit if their lanes projected them."""
    rng = np.random.default_rng(seed)
    pts, cand, v = np.asarray(pts, np.int64), np.asarray(cand, np.int64), np.asarray(v, np.int64)
    assert 0 < nA <= CAP_A and 0 < nB <= CAP_B and pts.shape == (nA, 2) and cand.shape == (nB, 2) and v.shape == (nB,)
    parked = (cand == PARK).all(1)
    assert np.abs(pts).max() < 1 << 12 and np.abs(cand[~parked]).max(initial=0) + max(shift) < 1 << 12
    e2 = rng.integers(0, 4, nA) if e2 is None else np.asarray(e2, np.int64)
    base = MO._base(rng)
    A = np.tile(np.asarray(base, np.int64), (CAP_A, 1))
    for i in range(nA):
        A[i, :e2[i]] += rng.choice((-1, 1), e2[i])
    B = np.tile(np.asarray(base, np.int64), (CAP_B, 1))
    B[:nB] = MO.rows_at(base, v, rng.choice((-1, 1), 128 - MO.QUERY_BYTES))
    ax, ay = np.zeros(CAP_A, np.int64), np.zeros(CAP_A, np.int64)
    ax[:nA], ay[:nA] = pts[:, 0], pts[:, 1]
    bx, by = np.zeros(CAP_B, np.int64), np.zeros(CAP_B, np.int64)
    bx[:nB] = np.where(parked, PARK[0], cand[:, 0] + shift[0])
    by[:nB] = np.where(parked, PARK[1], cand[:, 1] + shift[1])
    live = sorted(r for r in hits if len(hits[r]))               # the rows with hits first, then the other valid rows
    live += [r for r in np.flatnonzero(pts[:, 0] >= 0).tolist() if r not in hits or not len(hits[r])]
    for t in range(CAP_A - nA):                                 # rows beyond nA: copies of live rows
        r = live[t % len(live)]
        A[nA + t], ax[nA + t], ay[nA + t] = A[r], ax[r], ay[r]
    for t in range(CAP_B - nB):                                 # candidates beyond nB: live QUERY rows on their own points
        r = live[t % len(live)]
        B[nB + t], bx[nB + t], by[nB + t] = A[r], ax[r] + shift[0], ay[r] + shift[1]
    H = np.array([1, 0, shift[0], 0, 1, shift[1], 0, 0, 1], np.float32)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    c = dict(A=f(A), ax=f(ax), ay=f(ay), nA=nA, B=f(B), bx=f(bx), by=f(by), nB=nB, H=H, status=1, family=family, runs=tuple(runs),
             what="%s, %s, %d x %d%s" % (family, what, nA, nB, ", shifted" if shift != EYE else ""),
             hits={int(r): [int(j) for j in js] for r, js in hits.items() if len(js)}, v=v, e2=e2, shift=shift)
    for key in ("A", "B", "ax", "ay", "bx", "by"):
        assert np.array_equal(c[key], np.rint(c[key]))
    # the gate, from the stored coordinates: exactly the intended hits
    G = gate64(c, R2)
    got = {int(i): np.flatnonzero(G[i]).tolist() for i in np.flatnonzero(G.any(1))}
    assert got == c["hits"], (c["what"], "hit sets", {k: (got.get(k), c["hits"].get(k)) for k in set(got) ^ set(c["hits"])})
    would = gate64(c, R2, every_row=True) & ~G
    c["invalid_hits"] = {int(i): np.flatnonzero(would[i]).tolist() for i in np.flatnonzero(would.any(1))}
    assert c["invalid_hits"] == {int(r): list(js) for r, js in (invalid_hits or {}).items()}, (c["what"], c["invalid_hits"])
    # the distances
    c["D"] = distances64(c)
    assert (c["D"][:nA, :nB] == e2[:, None] + v[None, :]).all()
    # the tails: reading a row or a candidate beyond the counts changes a result
    first = c["runs"][0]
    own = restate(c, *first)
    wide_b, wide_a = restate(c, *first, nB=CAP_B), restate(c, *first, nA=CAP_A)
    on = live[:min(len(live), CAP_B - nB)]
    assert (wide_b[2][on] == 0).all() and (own[2][on] != 0).any(), (c["what"], "the candidates beyond nB change nothing")
    if nA < CAP_A:
        assert np.isfinite(wide_a[2][nA:]).any() and (own[0][nA:] == -1).all(), (c["what"], "the rows beyond nA would not match")
    c["where"], c["rounds"] = note_slots(c["hits"])
    return c


def _levels(rng, n):
    """n distinct distances of match_order_ref's levels (160, 208, then steps of 16 .. 32), shuffled."""
    return rng.permutation(MO.levels(rng, n))


def nearest_two(c, row):
    """(j of the nearest, j of the second nearest) of a row's hits by (distance, index)."""
    js = c["hits"][row]
    order = sorted(js, key=lambda j: (c["D"][row, j], j))
    return order[0], (order[1] if len(order) > 1 else None)


# ---- chunk_burst ----
BURST = ((-2, -1), (-2, 0), (-2, 1), (0, 0), (2, -1), (2, 0), (2, 1), (0, 2))       # the eight candidates around the burst row
HELPERS = ((0, 0), (1, 0), (0, 1), (2, 0), (0, 2), (3, 0), (0, 3), (1, 1), (1, 2), (2, 1))    # (hits at u <= 3, hits at u >= 4)


def _displacement(want):
    """An integer displacement d of a helper row from the burst row's point such that the helper hits `want[0]` of the
    BURST candidates 0 .. 3 and `want[1]` of the candidates 4 .. 7 (and which ones)."""
    for dx in range(-6, 7):
        for dy in range(-6, 7):
            seen = [u for u, o in enumerate(BURST) if _norm2((o[0] - dx, o[1] - dy)) < R2]
            if (sum(u <= 3 for u in seen), sum(u >= 4 for u in seen)) == tuple(want) and (dx, dy) != (0, 0):
                return (dx, dy), seen
    raise AssertionError("no displacement for %r" % (want,))


def _burst(pts, cand, hits, row, chunk, helpers, first_helper):
    """Row `row` owns the eight candidates of `chunk`; the rows from first_helper on sit next to it and share some."""
    P = grid(row)
    js = list(range(CHUNK * chunk, CHUNK * chunk + CHUNK))
    cand[js] = P + np.array(BURST)
    hits[row] = js
    for k, want in enumerate(helpers):
        d, seen = _displacement(want)
        pts[first_helper + k] = P + d
        hits[first_helper + k] = [js[u] for u in seen]


def chunk_burst(seed=0, shift=EYE):
    """Wave 0: lane 5 owns all of chunk 2 (candidates 16 .. 23), so the wave's rounds run at u = 3 and u = 7 INSIDE the
    chunk; lanes 6 .. 15 sit a few pixels from it and hit (0, 0), (1, 0), (0, 1), .. (2, 1) of the candidates at or before
    u = 3 / behind it: they are computed with partly filled lists and go on noting in the same chunk. Lane 20 holds one
    hit (candidate 25) from chunk 3 to the end. Wave 1 has no hit. Wave 2: lane 20 (row 148) owns all of chunk 4, with three
    helpers: its notes go to list[.][148], not to list[.][20], where row 20's pending entry lies."""
    rng = np.random.default_rng(700 + seed)
    nA, nB = 200, 48
    pts, cand, hits = grid(np.arange(nA)), np.tile(np.array(PARK), (nB, 1)), {}
    _burst(pts, cand, hits, 5, 2, HELPERS, 6)
    _burst(pts, cand, hits, 148, 4, ((1, 2), (3, 0), (0, 1)), 149)
    cand[25], hits[20] = grid(20) + HIT[1], [25]
    cand[26] = grid(20) + MISS                                  # nearer than everything, outside the gate
    cand[40], hits[21] = grid(21) + HIT[3], [40]                # pending in wave 0 while wave 2's rounds run
    v = np.sort(_levels(rng, nB))[::-1].copy()                  # descending in j: every step of a burst replaces min1
    v[26] = 1
    c = _build("chunk_burst", "bursts in chunks 2 and 4", 700 + seed, nA, nB, pts, cand, v, hits,
               [(R2, 0.8, INF), (R2, 1.5, INF)], shift)
    assert c["rounds"] == {0: [19, 23, "end"], 2: [35, 39]} and not any(64 <= r < 128 for r in c["hits"])
    for k, (before, after) in enumerate(HELPERS):
        mine = [c["where"][(6 + k, j)] for j in c["hits"].get(6 + k, [])]
        assert mine == [(e, 0) for e in range(before)] + [(e, 1) for e in range(after)], (k, mine)
    assert [c["where"][(5, j)] for j in c["hits"][5]] == [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (1, 1), (2, 1), (3, 1)]
    assert c["where"][(20, 25)] == (0, 2) and nearest_two(c, 5) == (23, 22) and nearest_two(c, 148) == (39, 38)
    return c


# ---- hit_counts ----
COUNTS = (0, 1, 2, 3, 4, 5, 7, 8, 9)


def hit_counts(near_at_entry_3, seed=0, shift=EYE):
    """Lane l of wave 0 owns COUNTS[(l + 3) % 9] consecutive candidates from 16 l + (3 l % 8) on: the end round only (1, 2, 3: an
    earlier round of another lane's may take them), one or two full rounds with nothing left (4, 8), full rounds with a
    remainder (5, 7, 9). No two lanes fill in the same chunk. For the lanes with 5 hits or more the two nearest are the hits
    3 and 4: entry 3 just before a round and entry 0 just after it; near_at_entry_3 says which of them is the nearest."""
    rng = np.random.default_rng(720 + seed + int(near_at_entry_3))
    nA, nB = 70, TILE
    pts, cand, hits = grid(np.arange(nA)), np.tile(np.array(PARK), (nB, 1)), {}
    v = rng.integers(1, 100, nB)                                # parked: nearer than every owned candidate
    for l in range(WAVE):
        n, s = COUNTS[(l + 3) % 9], 16 * l + (3 * l) % 8         # lanes 61, 62, 63: 1, 2, 3 hits, computed by the end round alone
        js = list(range(s, s + n))
        hits[l] = js
        for k, j in enumerate(js):
            cand[j] = grid(l) + HIT[(k + l) % len(HIT)]
        far = 1000 + 16 * rng.permutation(64)[:n]
        v[js] = far
        if n >= 5:
            near, second = 100 + l, (200 + 2 * l if l % 2 else 110 + l)        # ratio about 1/2, or above 0.8
            v[js[3]], v[js[4]] = (near, second) if near_at_entry_3 else (second, near)
    c = _build("hit_counts", "nearest at entry %d" % (3 if near_at_entry_3 else 0), 720 + seed, nA, nB, pts, cand, v, hits,
               [(R2, 0.8, INF), (R2, 1.5, INF)], shift)
    assert sorted({len(js) for js in c["hits"].values()} | {0}) == list(COUNTS)
    fills = [ch for js in c["hits"].values() for ch in {js[k] // CHUNK for k in range(LIST - 1, len(js), LIST)}]
    assert len(fills) == len(set(fills)), "two lanes fill in one chunk"
    for l, js in c["hits"].items():
        slots = [c["where"][(l, j)] for j in js]
        assert [e for e, _ in slots] == [k % LIST for k in range(len(js))], (l, slots)      # nobody else's round cuts a lane's run
        if len(js) >= 5:
            a, b = nearest_two(c, l)
            assert (a, b) == ((js[3], js[4]) if near_at_entry_3 else (js[4], js[3]))
            assert slots[3][0] == 3 and slots[4][0] == 0 and slots[4][1] == slots[3][1] + 1
    return c


# ---- tile_edge ----
TILE_EDGE_NB = (1024, 1025, 1031, 1032, 1033)


def tile_edge(nB, near_at, seed=0, shift=EYE):
    """Row 10 (wave 0) hits 700, 900, 1023 and 1024: three entries pending when tile 1 is loaded, and candidate 1024, the
    first of that tile, fills the list. Row 84 (wave 1) sits two pixels to the right and also hits 500: candidate 1023, the
    last of tile 0, fills its list and 1024 is entry 0 of the next round. near_at (1023 or 1024) is the nearest of both, the
    other the second nearest; at nB = 1024 there is no 1024 and 900 is the second. Row 158 (wave 2) owns candidates
    0 .. 15, the entries of tile 0 at the positions of tile 1's tail, and, from nB = 1031 on, nB - 1 (its nearest) and
    nB - 2: inside the rounded-up last chunk. At 1025 the nearest at nB - 1 is rows 10 and 84's, with near_at = 1024."""
    assert nB in TILE_EDGE_NB and near_at in (1023, 1024) and (nB > 1024 or near_at == 1023)
    rng = np.random.default_rng(740 + seed + nB + near_at)
    nA = 200
    pts, cand, hits = grid(np.arange(nA)), np.tile(np.array(PARK), (nB, 1)), {}
    P = grid(10)
    pts[84] = P + (2, 0)
    for j, o in ((500, (3, 0)), (700, (1, 1)), (900, (1, -1)), (1023, (1, 0)), (1024, (2, 1)), (1022, (-2, -2))):
        if j < nB:
            cand[j] = P + o
    hits[10] = [j for j in (700, 900, 1023, 1024) if j < nB]
    hits[84] = [j for j in (500, 700, 900, 1023, 1024) if j < nB]
    v = rng.integers(1, 100, nB)
    v[[500, 700, 900]] = (640, 480, 120 if nB == 1024 else 400)          # nearest 100, second 120: a match at 1.5 only, and
    v[1023] = 100 if near_at == 1023 else 120                           # at 0.8 too for a scan that loses the second
    if nB > 1024:
        v[1024] = 120 if near_at == 1023 else 100
    hits[158] = list(range(16))
    for j in range(16):
        cand[j] = grid(158) + HIT[j % len(HIT)]
    v[:16] = 1000 + 16 * rng.permutation(16)
    v[7] = 500                                                  # row 158's nearest of tile 0: the eighth hit of one chunk
    if nB >= 1031:
        hits[158] += [nB - 2, nB - 1]
        cand[nB - 2], cand[nB - 1] = grid(158) + HIT[1], grid(158) + HIT[0]
        v[nB - 2], v[nB - 1] = 120, 100
    c = _build("tile_edge", "nearest at %d" % near_at, 740 + seed, nA, nB, pts, cand, v, hits, [(R2, 0.8, INF), (R2, 1.5, INF)],
               shift)
    w = c["where"]
    assert [w[(10, j)][0] for j in hits[10]] == [0, 1, 2, 3][:len(hits[10])] and w[(84, 1023)] == (3, 0)
    assert c["rounds"][0] == ([1024] if nB > 1024 else ["end"]) and c["rounds"][1] == [1023] + (["end"] if nB > 1024 else [])
    other = (1024 if near_at == 1023 else 1023) if nB > 1024 else 900
    assert nearest_two(c, 10) == (near_at, other) == nearest_two(c, 84)
    if nB > 1024:
        assert w[(84, 1024)] == (0, 1)
    if nB >= 1031:
        assert nearest_two(c, 158) == (nB - 1, nB - 2)
    return c


# ---- scan_order ----
# (name, distances of the row's gated candidates in ascending j, (local index, min1, min2) of the scan; None: min2 stays at
# MIN2_INIT). Every one of these rows has e2 = 0, so D = v.
SCAN_ROWS = (
    ("descending", (400, 300, 200, 100), (3, 100, 200)),              # every step replaces min1
    ("ascending", (100, 200, 300, 400), (0, 100, 200)),
    ("all_equal", (200, 200, 200), (0, 200, 200)),                    # -1 at ambiguity 0.8 and 1.0, the FIRST at 1.5
    ("zero_duplicates", (0, 0, 50), (0, 0, 0)),                       # min2 == 0: -1 whatever the ambiguity
    ("single", (300,), (0, 300, None)),                               # min2 stays at 2139095040: a match
    ("far_then_two_equal", (400, 100, 100), (1, 100, 100)),           # the first of the two
    ("ratio_3_4", (300, 400), (0, 300, 400)),                         # exact in binary32: equal to 0.75 is not below it
    ("ratio_3_4_reversed", (400, 300), (1, 300, 400)),
    ("ratio_1_2", (200, 100, 400), (1, 100, 200)),
    ("max_distance", (100, 400, 900), (0, 100, 400)),                 # max_distance 100 is not a match, 101 is
    ("boundary", (300, 100), (1, 100, 300)),                          # the second sits at offset (2, 1): outside at radius2 5
)
SCAN_RUNS = ((R2, 0.8, INF), (R2, 0.5, INF), (R2, 0.75, INF), (R2, 1.0, INF), (R2, 1.5, INF), (R2, 0.8, 100.0), (R2, 0.8, 101.0),
             (5.0, 0.8, INF))
SCAN_OFFSETS = ((0, 0), (1, 0), (0, 1), (1, 1))


def scan_order(seed=0, shift=EYE):
    """Row s of wave 0 meets the distances of SCAN_ROWS[s] inside ONE round (its candidates are 16 s .. and nobody else of
    the wave hits in between); row 64 + s of wave 1 meets the same distances SPLIT over two rounds: between its first and
    its second hit lane 63 of that wave (row 127, the pacer) takes four hits and fills."""
    rng = np.random.default_rng(760 + seed)
    nA, nB = 128, 16 * len(SCAN_ROWS)
    pts, cand, hits = grid(np.arange(nA)), np.tile(np.array(PARK), (nB, 1)), {127: []}
    v = rng.integers(1, 100, nB)
    e2 = rng.integers(0, 4, nA)
    for s, (name, ds, _) in enumerate(SCAN_ROWS):
        n, j0 = len(ds), 16 * s
        offs = ((0, 0), (2, 1)) if name == "boundary" else SCAN_OFFSETS
        quiet = list(range(j0, j0 + n))
        split = [j0 + 4] + list(range(j0 + 9, j0 + 8 + n))
        pace = list(range(j0 + 5, j0 + 9))
        for row, js in ((s, quiet), (64 + s, split)):
            hits[row], e2[row] = js, 0
            for k, j in enumerate(js):
                cand[j], v[j] = grid(row) + offs[k], ds[k]
        hits[127] += pace
        cand[pace] = grid(127) + np.array(HIT[:4])
        v[pace] = 1000 + 16 * rng.permutation(64)[:4]
        cand[j0 + 15], v[j0 + 15] = grid(s) + MISS, 1
    c = _build("scan_order", "%d rows, once in one round and once split" % len(SCAN_ROWS), 760 + seed, nA, nB, pts, cand, v, hits,
               SCAN_RUNS, shift, e2=e2)
    c["expected"] = {}
    for s, (name, ds, (loc, min1, min2)) in enumerate(SCAN_ROWS):
        for row in (s, 64 + s):
            js = c["hits"][row]
            assert [c["D"][row, j] for j in js] == list(ds) and scan_int(ds) == (loc, min1, MIN2_INIT if min2 is None else min2)
            rounds = {c["where"][(row, j)][1] for j in js}
            assert len(rounds) == (1 if row < 64 or len(js) == 1 else 2), (name, row, rounds)
            for run in SCAN_RUNS:
                r2, amb, maxd = run
                l1, m1, m2 = (0, 300, None) if (name == "boundary" and r2 == 5.0) else (loc, min1, min2)
                m2 = MIN2_INIT if m2 is None else m2
                ok = m2 > 0 and Fraction(m1, max(m2, 1)) < Fraction(float(np.float32(amb))) and m1 < maxd
                c["expected"][(row, run)] = (js[l1] if ok else -1, m1)
    for run in SCAN_RUNS:                                       # the table above against the integer restatement
        res, _, best = restate(c, *run)
        for s in range(len(SCAN_ROWS)):
            for row in (s, 64 + s):
                assert (res[row], best[row]) == c["expected"][(row, run)], (SCAN_ROWS[s][0], row, run, res[row], best[row])
    name = lambda s: SCAN_ROWS[s][0]
    at = lambda s, run: c["expected"][(s, run)][0]
    for s in range(len(SCAN_ROWS)):                             # what the rows are there for, outright
        j0 = 16 * s
        if name(s) == "all_equal":
            assert at(s, (R2, 0.8, INF)) == at(s, (R2, 1.0, INF)) == -1 and at(s, (R2, 1.5, INF)) == j0
        if name(s) == "zero_duplicates":
            assert all(at(s, run) == -1 for run in SCAN_RUNS)
        if name(s) == "single":
            assert all(at(s, run) == j0 for run in SCAN_RUNS if run[2] == INF)
        if name(s) == "far_then_two_equal":
            assert at(s, (R2, 1.0, INF)) == -1 and at(s, (R2, 1.5, INF)) == j0 + 1
        if name(s).startswith("ratio_3_4"):
            assert at(s, (R2, 0.75, INF)) == -1 and at(s, (R2, 0.8, INF)) >= j0
        if name(s) == "ratio_1_2":
            assert at(s, (R2, 0.5, INF)) == -1 and at(s, (R2, 0.75, INF)) == j0 + 1
        if name(s) == "max_distance":
            assert at(s, (R2, 0.8, 100.0)) == -1 and at(s, (R2, 0.8, 101.0)) == j0
        if name(s) == "boundary":
            assert at(s, (R2, 0.8, INF)) == j0 + 1 and at(s, (5.0, 0.8, INF)) == j0
    return c


# ---- ragged_rows ----
RAGGED_NA = (1, 63, 64, 65, 257)


def ragged_rows(nA, invalid_burst=False, seed=0, shift=EYE):
    """The burst of chunk_burst on the LAST live row nA - 1 (chunk 1, candidates 8 .. 15, descending). The rows nA - 2 and
    nA - 3 are invalid (ax = -1) and sit on spots of their own where candidates 0 .. 3 and 16 .. 19 wait for them, nearer
    than everything: their lanes hold NaN and must note nothing. They are lanes of the burst row's own wave at nA = 63, 64
    and 257 (and at 65 with invalid_burst the burst's hits go to row 32, beside them in wave 0); at nA = 65 without it the
    burst lane is lane 0 of wave 1 and the invalid rows 62 and 63 are the last lanes of wave 0. With invalid_burst the row nA - 1 is itself invalid, at
    (-1, y), and the eight candidates lie around (0, y), the point of a live row that takes all eight."""
    assert nA in RAGGED_NA and not (invalid_burst and nA == 1)
    rng = np.random.default_rng(780 + seed + nA + int(invalid_burst))
    nB, rb = 24, nA - 1
    pts, cand, hits, would = grid(np.arange(nA)), np.tile(np.array(PARK), (nB, 1)), {}, {}
    burst = list(range(8, 16))
    if invalid_burst:
        r0 = max(r for r in range(rb) if r % 32 == 0)
        pts[rb] = grid(r0) + (-1, 0)
        cand[burst] = grid(r0) + np.array(BOTH)
        hits[r0], would[rb] = burst, burst
    else:
        cand[burst] = grid(rb) + np.array(HIT[:8])
        hits[rb] = burst
    for k, r in enumerate((rb - 1, rb - 2)):
        if r < 0:
            continue
        assert r not in hits
        spot = (-1, 100 * (r // 32) + 40 + 10 * k)
        pts[r] = spot
        js = [2 * k, 2 * k + 1, 16 + 2 * k, 17 + 2 * k]
        cand[js] = spot
        would[r] = js
    v = np.sort(_levels(rng, nB))[::-1].copy()
    for js in would.values():
        if js != burst:
            v[js] = 1
    c = _build("ragged_rows", "burst on row %d%s" % (rb, ", itself invalid" if invalid_burst else ""), 780 + seed, nA, nB, pts,
               cand, v, hits, [(R2, 0.8, INF), (R2, 1.5, INF)], shift, invalid_hits=would)
    owner = r0 if invalid_burst else rb
    assert c["rounds"] == {owner // WAVE: [11, 15]} and nearest_two(c, owner) == (15, 14)
    assert nA == 1 or len(c["invalid_hits"]) >= 2
    return c


# ---- shared_point ----
def shared_point(seed=0, shift=EYE):
    """Wave 0: all 64 rows on ONE point with ten candidates around it (the lanes fill in lockstep: rounds after candidates 3
    and 7 and at the end), each row with a perturbation of its own. Wave 1: chunk 2 (candidates 16 .. 23) lies on eight
    points far apart, and the rows 64 + 8 u + k sit on eight distinct places around candidate 16 + u: 64 distinct points, one
    hit each, all in one chunk."""
    rng = np.random.default_rng(800 + seed)
    nA, nB = 128, 32
    pts, cand, hits = grid(np.arange(nA)), np.tile(np.array(PARK), (nB, 1)), {}
    pts[:64] = grid(0)
    cand[:10] = grid(0) + np.array(HIT)
    for r in range(64):
        hits[r] = list(range(10))
    for u in range(CHUNK):
        cand[16 + u] = grid(65 + 8 * u)                         # (a column with x > 0: no row lands on x = -1)
        for k in range(8):
            pts[64 + 8 * u + k] = grid(65 + 8 * u) + BOTH[k]
            hits[64 + 8 * u + k] = [16 + u]
    v = _levels(rng, nB)
    v[10:16] = rng.integers(1, 100, 6)
    v[8], v[5] = 100, 120                                       # wave 0: the nearest is pending until the end round, the
                                                                # second nearest is the sixth hit of chunk 0
    c = _build("shared_point", "a wave on one point, a wave on 64", 800 + seed, nA, nB, pts, cand, v, hits,
               [(R2, 0.8, INF), (R2, 1.5, INF)], shift, e2=rng.integers(0, 33, nA))
    assert c["rounds"] == {0: [3, 7, "end"], 1: ["end"]} and len({tuple(p) for p in pts[64:].tolist()}) == 64
    return c


# ---- the families ----
_CASES = {}


def family_cases(family):
    """The cases of one family, built once and left unchanged. The geometry families come once more under SHIFT."""
    if family not in _CASES:
        if family == "chunk_burst":
            cs = [chunk_burst(), chunk_burst(1, SHIFT)]
        elif family == "hit_counts":
            cs = [hit_counts(True), hit_counts(False), hit_counts(True, 1, SHIFT)]
        elif family == "tile_edge":
            cs = [tile_edge(nB, near) for nB in TILE_EDGE_NB for near in (1023, 1024) if nB > 1024 or near == 1023]
            cs += [tile_edge(1025, 1024, 1, SHIFT), tile_edge(1033, 1023, 1, SHIFT)]
        elif family == "scan_order":
            cs = [scan_order(), scan_order(1, SHIFT)]
        elif family == "ragged_rows":
            cs = [ragged_rows(nA) for nA in RAGGED_NA] + [ragged_rows(nA, True) for nA in RAGGED_NA if nA > 1]
            cs += [ragged_rows(65, False, 1, SHIFT), ragged_rows(257, True, 1, SHIFT)]
        elif family == "shared_point":
            cs = [shared_point(), shared_point(1, SHIFT)]
        else:
            raise ValueError(family)
        _CASES[family] = cs
    return _CASES[family]


def all_cases():
    return [c for f in FAMILIES for c in family_cases(f)]


def permuted(case, seed):
    """The case with its candidates shuffled inside [0, nB). Returns (case, source, sure): candidate r of the new case is
    candidate source[r] of the old one; sure (capA,) bool marks the rows whose answer must map back, whatever the order of
    the scan: those whose nearest and second nearest gated distances are distinct and unique, and those with fewer than two
    gated candidates (at every radius the case runs). best must be bit-identical for EVERY row."""
    nB = case["nB"]
    source = np.random.default_rng(820 + seed).permutation(nB)
    assert (source != np.arange(nB)).sum() > nB // 2
    c = dict(case, what=case["what"] + ", permuted %d" % seed)
    for key in ("B", "bx", "by"):
        c[key] = case[key].copy()
        c[key][:nB] = case[key][:nB][source]
    c["D"] = distances64(c)
    sure = np.ones(CAP_A, bool)
    for r2 in sorted({run[0] for run in case["runs"]}):
        G = gate64(case, r2)
        for i in np.flatnonzero(G.sum(1) >= 2):
            d = np.sort(case["D"][i, G[i]])
            sure[i] &= d[0] < d[1] and (len(d) == 2 or d[1] < d[2])
    assert any(sure[r] for r in case["hits"]), "no row with a hit is sure of its answer"
    return c, source, sure


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def permuted_picks():
    """One case per family, for where every case is too many."""
    return [family_cases(f)[i] for f, i in (("chunk_burst", 0), ("hit_counts", 1), ("tile_edge", 3), ("scan_order", 0),
                                            ("ragged_rows", 6), ("shared_point", 0))]


def assert_maps_back(c, matcher):
    """matcher(case, run) -> (result, count, best): shuffling the candidates maps the matches through the permutation on
    the rows that are sure of their answer and leaves best as it is on every row. Returns the number of matches of sure rows
    that the permutations moved to another index."""
    moved = 0
    for seed in (1, 2):
        p, source, sure = permuted(c, seed)
        for run in c["runs"]:
            a, b = matcher(c, run), matcher(p, run)
            back = np.where(b[0] >= 0, source[np.maximum(b[0], 0)], -1)
            assert np.array_equal(back[sure], a[0][sure]), (p["what"], run, "matches")
            assert np.array_equal(bits(b[2]), bits(a[2])), (p["what"], run, "best")
            moved += int((b[0][sure] != a[0][sure]).sum())
    return moved


def ragged_batch():
    """16 pairs of mixed families: slot 5 emptied (nB = 0), slot 9 with status 0, a pair with nB = 1033 among them."""
    cases = all_cases()
    last = [c for c in family_cases("tile_edge") if c["nB"] == 1033 and "1024" in c["what"].split(",")[1] and c["shift"] == EYE]
    pick = [cases[i] for i in np.random.default_rng(830).permutation(len(cases))[:15]] + last[:1]
    assert len(pick) == 16
    assert {c["family"] for c in pick} == set(FAMILIES) and any(c["nB"] == 1033 for c in pick)
    pick[5] = dict(pick[5], nB=0, what=pick[5]["what"] + ", emptied")
    pick[9] = dict(pick[9], status=0, what=pick[9]["what"] + ", status 0")
    return pick
