"""Homography-guided matching on adversarial gate-HIT PATTERNS (tests/guided_hits_ref.py), on the CPU: the host twin against
the restatement guided_ref.guided and against the generators' integer restatement, and a numpy MODEL of the device kernel's
schedule that measures which cases can see a slip of that schedule at all. No GPU.

The model (schedule_model, for the tests only) is written from the comments of csrc/nm_match_guided.hip: one model wave per
64 rows, workgroups of 256 rows, the candidates' coordinates in tiles of TILE whose tail is NaN and whose length is rounded
up to a chunk, chunks of CHUNK gate tests that a wave enters only when one of its lanes has a hit in them, per-lane lists of L
noted candidates indexed by the row's place in the workgroup, a round of the whole wave ("flush") after any gate test that
leaves a lane's list full, walking the entries 0 .. L - 1, and one more round after the last tile. The waves of a workgroup
go chunk by chunk in turn, which only mutant (h) can see. With no mutant it must equal guided_ref.guided on every case, old
and new, at L = 4, and at L = 1 and 3 on all but the large old pairs (test_model_equals_the_restatement).

Mutants of the model, and what detects them (a case DETECTS a mutant when result, count or the bits of best differ from the
unmutated model in one of the runs the case names):
  a  the full-list test runs only at the end of a chunk, and hits beyond L are dropped
  b  no round after the last tile
  c  a round walks the entries in descending order
  d  the tile tail is not refilled: the coordinates of the previous tile stay, noted with indices >= nB
  e  the chunk count of the last tile is rounded down
  f  a lane computes its own full list only and ignores the other lanes' ballots: LEGAL, must change nothing
  g  rows with ax < 0 are projected and note hits
  h  the lists are indexed by lane, not by the place in the workgroup: the waves of a workgroup share them

Measured (print_table prints cases detecting / cases per family and mutant; the recorded table is in CHANGELOG.md, "Tests:
guided matching on adversarial gate-hit patterns"). The old families are _mixed(16) of test_gpu_match_guided.py (1100 x 1200
buffers) and the pairs of test_planted_duplicates_ties_and_degenerate_pairs, at radius2 6 / ambiguity 0.8 and 30 / 0.95, and
at radius2 1e12 (every lane hits every candidate) for the pairs in buffers of at most 300 rows.

What the table says, plainly. The old cases are NOT blind to most of this machinery: random coordinates crowded into
60 x 60 pixels give enough hits per chunk that (a), (b), (e), (g) and (h) already change a result in 5 to 10 old pairs of 16
or 17, and no gap is claimed for them; what the new families add there is that each mutant is seen by construction, in a named
row at a named candidate, also under a translation. Two mutants NO old case sees, and these are the gap that is closed:
  (c) the order of a round's entries shows only in WHICH of several equal nearest candidates is reported, and a tie at the
      minimum is a match only at an ambiguity above 1; no old run has one. scan_order's all_equal and far_then_two_equal
      rows at ambiguity 1.5 see it in both cases.
  (d) a stale tile tail is noted with indices >= nB, and in the old buffers the rows behind nB are far from every query
      (all ones) or the buffers end at nB, so the stale hits never become a minimum. Here they are copies of query rows,
      and tile_edge sees it at nB = 1025, 1031 and 1033.
  The test asserts both zeros, so the claim cannot go stale unseen.
(d) and (e) need a last tile with a tail and a partial chunk: at nB = 1024 and 1032 there is neither, nothing can be seen, and
the test asserts exactly that split (8 of 11). (g) needs an invalid row: every ragged_rows case but nA = 1. (h) is seen where
two waves of a workgroup hold entries at the same lane: chunk_burst (rows 20 and 148), scan_order (rows s and 64 + s) and
shared_point. scan_order never has more than L hits of a lane in one chunk, so it cannot see (a); ragged_rows' bursts end
with empty lists, so they cannot see (b). (f) changes nothing anywhere, as it must. Every empty cell of a new family is
asserted to be empty (DETECTS).
"""
import numpy as np
import pytest

import guided_hits_ref as R
import guided_ref as G
from test_match_guided_host import random_pair

TB, WAVE, TILE, CHUNK = R.TB, R.WAVE, R.TILE, R.CHUNK
MUTANTS = "abcdefgh"
OLD_RUNS = ((6.0, 0.8, np.inf), (30.0, 0.95, np.inf))
LOCKSTEP_RUN = (1e12, 0.8, np.inf)
OLD = ("mixed (old)", "planted (old)")
# family -> the mutants at least one of its cases must detect; every other (family, mutant) must detect nothing
DETECTS = {"chunk_burst": "abh", "hit_counts": "ab", "tile_edge": "abde", "scan_order": "bch", "ragged_rows": "ag",
           "shared_point": "abh"}


# ---- the model ----
def prepare(p, radius2, capA, capB):
    """What every variant of the model shares for one pair and radius: the gate of EVERY row of the buffers against every
    candidate of the buffers (validity and the counts are the schedule's business), and the distances."""
    A, B = np.asarray(p["A"], np.float32)[:capA], np.asarray(p["B"], np.float32)[:capB]
    ax, ay = np.asarray(p["ax"], np.float32)[:capA], np.asarray(p["ay"], np.float32)[:capA]
    bx, by = np.asarray(p["bx"], np.float32)[:capB], np.asarray(p["by"], np.float32)[:capB]
    H = np.asarray(p["H"], np.float32).reshape(9)
    usable = p["status"] == 1 and bool(np.isfinite(H).all())
    gate = G.gate_matrix(H, ax, ay, bx, by, radius2) if usable else None
    D = (A.astype(np.float64) ** 2).sum(1)[:, None] + (B.astype(np.float64) ** 2).sum(1)[None, :] - 2.0 * (A.astype(np.float64) @ B.astype(np.float64).T)
    assert (D == np.rint(D)).all() and D.max() < 1 << 24, "the model wants distances that are exact in float32"
    nA, nB = min(max(int(p["nA"]), 0), capA), min(max(int(p["nB"]), 0), capB)
    return dict(gate=gate, D=D.astype(np.float32), ax=ax, nA=nA, nB=nB, capA=capA, capB=capB, usable=usable)


def schedule_model(q, L=4, mutant=None):
    """The scan state (min1, min2, idx, seen) of every row of the buffers after the device schedule."""
    capA, capB, nA, nB, D = q["capA"], q["capB"], q["nA"], q["nB"], q["D"]
    min1 = np.full(capA, np.inf, np.float32)
    min2 = np.full(capA, G.MIN2_INIT, np.float32)
    idx, seen = np.full(capA, -1, np.int64), np.zeros(capA, bool)
    if not q["usable"] or nB == 0:
        return min1, min2, idx, seen
    for row0 in range(0, capA, TB):
        if row0 >= nA:
            continue
        rows = np.minimum(row0 + np.arange(TB), capA - 1)
        inside = row0 + np.arange(TB) < capA
        live = inside & (row0 + np.arange(TB) < nA)
        notes = live & ((q["ax"][rows] >= 0) | (mutant == "g"))            # the other lanes hold NaN and pass no gate
        lists, cnt = np.zeros((L, TB), np.int64), np.zeros(TB, np.int64)
        place = np.arange(TB) % WAVE if mutant == "h" else np.arange(TB)

        def flush(w, who):
            lanes = np.arange(w * WAVE, (w + 1) * WAVE)
            for c in (range(L - 1, -1, -1) if mutant == "c" else range(L)):
                t = lanes[who & (cnt[lanes] > c)]
                if not len(t):
                    continue
                r, j = rows[t], lists[c, place[t]]
                d = D[r, j]
                first = ~seen[r]
                lower = ~first & (d < min1[r])
                second = ~first & ~lower & (d < min2[r])
                min2[r] = np.where(lower, min1[r], np.where(second, d, min2[r]))
                idx[r] = np.where(first | lower, j, idx[r])
                min1[r] = np.where(first | lower, d, min1[r])
                seen[r] = True
            cnt[lanes[who]] = 0

        everyone = np.ones(WAVE, bool)
        for t0 in range(0, nB, TILE):
            left = nB - t0
            m = TILE if left >= TILE else (left // CHUNK * CHUNK if mutant == "e" else (left + CHUNK - 1) // CHUNK * CHUNK)
            j = t0 + np.arange(m)
            src = np.where(j < nB, j, -1)                                  # -1: NaN
            if mutant == "d" and t0 > 0:
                src = np.where(j < nB, j, j - TILE)                        # what the previous tile left there
            ok = (src >= 0) & (j < capB)                                   # (an index beyond the buffers cannot be followed)
            hit = np.zeros((TB, m), bool)
            hit[:, ok] = q["gate"][rows][:, src[ok]]
            hit &= notes[:, None]
            entered = hit.reshape(TB // WAVE, WAVE, m // CHUNK, CHUNK).any(axis=(1, 3))
            for qc in np.flatnonzero(entered.any(0)):
                for w in np.flatnonzero(entered[:, qc]):
                    lanes = np.arange(w * WAVE, (w + 1) * WAVE)
                    for u in range(CHUNK):
                        g = lanes[hit[lanes, qc * CHUNK + u]]
                        if not len(g):
                            continue                            # no count changed: no list became full
                        if mutant == "a":
                            g = g[cnt[g] < L]
                        lists[cnt[g], place[g]] = t0 + qc * CHUNK + u
                        cnt[g] += 1
                        full = cnt[lanes] == L
                        if mutant != "a" and full.any():
                            flush(w, full if mutant == "f" else everyone)
                    if mutant == "a" and (cnt[lanes] == L).any():
                        flush(w, everyone)
        if mutant != "b":
            for w in range(TB // WAVE):
                if (cnt[w * WAVE:(w + 1) * WAVE] > 0).any():
                    flush(w, everyone)
    return min1, min2, idx, seen


def decide(q, state, ambiguity, max_distance):
    """(result, count, best) of the buffers' rows from the scan state."""
    min1, min2, idx, seen = state
    valid = (np.arange(q["capA"]) < q["nA"]) & (q["ax"] >= 0) & q["usable"]
    with np.errstate(all="ignore"):
        ok = valid & seen & (min2 > 0) & (min1 / min2 < np.float32(ambiguity)) & (min1 < np.float32(max_distance))
    result = np.where(ok, idx, -1).astype(np.int32)
    return result, int((result >= 0).sum()), min1


def same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(R.bits(a[2]), R.bits(b[2]))


# ---- the families, old and new ----
def _old_mixed():
    import test_gpu_match_guided as T
    return [dict(p, capA=T.CAPA, capB=T.CAPB) for p in T._mixed(16)]


def _old_planted():
    """The pairs of test_match_guided_host.test_planted_duplicates_ties_and_degenerate_pairs, each at its own size."""
    z0 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 0], np.float32)
    zrow = np.array([1, 0, 0, 0, 1, 0, -1.0 / 16, 0, 1], np.float32)
    pairs = [random_pair(1, 300, 280), random_pair(2, 257, 1030, negative=(0, 5, 256)),
             random_pair(3, 64, 120), random_pair(4, 200, 200, status=0), random_pair(5, 200, 200, status=2),
             random_pair(6, 200, 150, nA=0), random_pair(7, 150, 200, nB=0), random_pair(8, 120, 130, nA=10 ** 6, nB=10 ** 6),
             random_pair(9, 120, 130, nA=-4, nB=-1), random_pair(10, 90, 77, nA=31, nB=50), random_pair(11, 100, 100, H=z0),
             random_pair(12, 100, 100, H=zrow)]
    pairs[11]["ax"][:20] = 16.0
    nanH = random_pair(13, 100, 100)
    nanH["H"][3] = np.nan
    pairs.append(nanH)
    pairs += [random_pair(20 + seed, ra, rb, negative=(1, 2)) for seed, (ra, rb) in enumerate([(300, 280), (257, 1030), (513, 700), (64, 9)])]
    return [dict(p, capA=len(p["ax"]), capB=len(p["bx"])) for p in pairs]


_FAMILIES = {}


def families():
    """{name: [(pair, runs)]}, the old families first; built once."""
    if not _FAMILIES:
        for name, pairs in zip(OLD, (_old_mixed(), _old_planted())):
            _FAMILIES[name] = [(p, OLD_RUNS + ((LOCKSTEP_RUN,) if p["capA"] <= 300 else ())) for p in pairs]
        for f in R.FAMILIES:
            _FAMILIES[f] = [(dict(c, capA=R.CAP_A, capB=R.CAP_B), c["runs"]) for c in R.family_cases(f)]
    return _FAMILIES


_PREPARED = {}


def prepared(p, radius2):
    key = (id(p), radius2)
    if key not in _PREPARED:
        _PREPARED[key] = (p, prepare(p, radius2, p["capA"], p["capB"]))    # (p keeps the id alive)
    return _PREPARED[key][1]


def outputs(p, runs, L, mutant):
    out = []
    for r2 in sorted({run[0] for run in runs}):
        q = prepared(p, r2)
        state = schedule_model(q, L, mutant)
        out += [decide(q, state, amb, maxd) for rr, amb, maxd in runs if rr == r2]
    return out


_TABLE = {}


def mutant_table():
    """{family: {mutant: [case detects it, ..]}}"""
    if not _TABLE:
        for name, cases in families().items():
            truth = [outputs(p, runs, 4, None) for p, runs in cases]
            _TABLE[name] = {m: [not all(same(a, b) for a, b in zip(outputs(p, runs, 4, m), t)) for (p, runs), t in zip(cases, truth)]
                            for m in MUTANTS}
    return _TABLE


def print_table():
    print("%-22s %s" % ("family", " ".join("%-6s" % m for m in MUTANTS)))
    for name, row in mutant_table().items():
        print("%-22s %s" % (name, " ".join("%-6s" % ("%d/%d" % (sum(row[m]), len(row[m]))) for m in MUTANTS)))


# ---- the host twin ----
def _host(nm, c, run):
    r2, amb, maxd = run
    res, cnt, best = nm.sift_match_guided_host([c["A"]], [c["ax"]], [c["ay"]], [c["nA"]], [c["B"]], [c["bx"]], [c["by"]], [c["nB"]],
                                               c["H"].reshape(1, 9), status=np.array([c["status"]], np.int32), radius2=r2,
                                               ambiguity=amb, max_distance=maxd, capA=R.CAP_A, capB=R.CAP_B, want_distance=True)
    return res[0], int(cnt[0]), best[0]


def _restatement(c, run):
    r2, amb, maxd = run
    return G.guided(c["A"], c["ax"], c["ay"], c["nA"], c["B"], c["bx"], c["by"], c["nB"], c["H"], c["status"], r2, amb, maxd,
                    capA=R.CAP_A, capB=R.CAP_B)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_host_twin_equals_both_restatements(nm, oracle, family):
    """Result, count and the bits of best, against guided_ref.guided (float32, the oracle's chain) and against the
    generator's integer restatement."""
    seen = set()
    for c in R.family_cases(family):
        for run in c["runs"]:
            got = _host(nm, c, run)
            assert got[1] == (got[0] >= 0).sum()
            assert same(got, _restatement(c, run)), (c["what"], run, "guided_ref")
            assert same(got, R.restate(c, *run)), (c["what"], run, "the integer restatement")
            assert (got[0][c["nA"]:] == -1).all() and np.isinf(got[2][c["nA"]:]).all()
            seen |= set(np.unique(got[0][:c["nA"]]).tolist())
            if family == "scan_order":
                for (row, r), (j, m1) in c["expected"].items():
                    if r == run:
                        assert (got[0][row], got[2][row]) == (j, m1), (c["what"], R.SCAN_ROWS[row % 64][0], row, run)
    assert -1 in seen and max(seen) >= 0, "the family's results are all matches or all rejections"


def test_host_twin_on_the_ragged_batch(nm, oracle):
    batch = R.ragged_batch()
    k = lambda key: [c[key] for c in batch]
    for run in ((R.R2, 0.8, np.inf), (R.R2, 1.5, np.inf)):
        res, cnt, best = nm.sift_match_guided_host(k("A"), k("ax"), k("ay"), k("nA"), k("B"), k("bx"), k("by"), k("nB"),
                                                   np.stack(k("H")), status=np.array(k("status"), np.int32), radius2=run[0],
                                                   ambiguity=run[1], capA=R.CAP_A, capB=R.CAP_B, want_distance=True)
        for p, c in enumerate(batch):
            assert same((res[p], int(cnt[p]), best[p]), _restatement(c, run)), (c["what"], run)
        assert cnt[5] == cnt[9] == 0 and cnt.sum() > 0
    # tile_edge's nearest two are 100 and 120: matches above a ratio of 0.83 only, so the 1033 pair is counted at 1.5
    assert any(c["nB"] == 1033 and cnt[p] >= 3 for p, c in enumerate(batch))


@pytest.mark.parametrize("family", R.FAMILIES)
def test_host_twin_on_permuted_candidates(nm, family):
    """EVERY case of the family, two permutations each."""
    moved = sum(R.assert_maps_back(c, lambda case, run: _host(nm, case, run)) for c in R.family_cases(family))
    assert moved > 0, "the permutations moved no match"


# ---- the model is the restatement; what the mutants show ----
@pytest.mark.parametrize("L", [4, 1, 3])
def test_model_equals_the_restatement(oracle, L):
    """Every case, old and new, in every run it names (L = 1 follows every hit at once; 3 is no divisor of CHUNK)."""
    for name, cases in families().items():
        for p, runs in cases:
            for run in runs:
                if L != 4 and (run == LOCKSTEP_RUN or p["capA"] > 300):
                    continue                                    # (the large old pairs once, at the kernel's L)
                q = prepared(p, run[0])
                got = decide(q, schedule_model(q, L), run[1], run[2])
                want = G.guided(p["A"], p["ax"], p["ay"], p["nA"], p["B"], p["bx"], p["by"], p["nB"], p["H"], p["status"], *run,
                                capA=p["capA"], capB=p["capB"])
                assert same(got, want), (name, p.get("what"), run, L)
                if "D" in p:
                    assert same(got, R.restate(p, *run)), (name, p["what"], run, L, "the integer restatement")


def test_the_new_families_reject_the_mutants_they_name():
    """The whole table is printed (CHANGELOG.md keeps it). Of the old families only the gap is asserted: no old case sees
    (c) or (d), and none is changed by the legal (f)."""
    print_table()
    table = mutant_table()
    for name in OLD:
        for m in "cdf":
            assert not any(table[name][m]), (name, m, "an old case sees this mutant now: the gap CHANGELOG.md names has moved")
    for family in R.FAMILIES:
        for m in MUTANTS:
            assert any(table[family][m]) == (m in DETECTS[family]), (family, m, table[family][m])
    assert not any(any(row["f"]) for row in table.values()), "a legal schedule changed a result"
    for m in "abcdegh":
        assert any(m in DETECTS[f] for f in R.FAMILIES)
    # where in a family: the cases the mutant names
    cases = {f: R.family_cases(f) for f in R.FAMILIES}
    for c, d, e in zip(cases["tile_edge"], table["tile_edge"]["d"], table["tile_edge"]["e"]):
        assert d == e == (c["nB"] % CHUNK != 0), (c["what"], "a tail to refill and a partial chunk exist off multiples of CHUNK")
    for c, g in zip(cases["ragged_rows"], table["ragged_rows"]["g"]):
        assert g == bool(c["invalid_hits"]), c["what"]
    assert all(table["chunk_burst"]["h"]) and all(table["scan_order"]["c"]) and all(table["ragged_rows"]["a"])
