"""An independent restatement of the u8 matcher (nm_sift_match_u8_*) and the cases its host and GPU tests share.

Written from the entry's stated semantics, not from csrc/nm_match_u8.hip: the distance matrix is exact integers (int64; the
products run through float64 BLAS, where every value is far below 2^53 and therefore exact), and the scan is the
reference's (kernels/match.cu:88-116) line by line on those values as float32, all rows at once. Everything is exact, so the
product must equal this with no tolerance and no excluded rows.
"""
import numpy as np

MIN2_INIT = np.float32(2139095040.0)
SIZES = (1, 2, 31, 32, 33, 127, 128, 129, 257)


def distances(A, B):
    a, b = np.asarray(A, np.uint8).astype(np.float64), np.asarray(B, np.uint8).astype(np.float64)
    d = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)
    D = d.astype(np.int64)
    assert (D == d).all() and (D >= 0).all() and D.max(initial=0) <= 128 * 255 * 255
    return D


def scan(D, ambiguity, prior):
    """set_matches of match.cu on the rows of D (as float32), starting from the pre-filled result `prior`."""
    D = D.astype(np.float32)
    rows, cols = D.shape
    res = np.array(prior, np.int32).copy()
    min1 = D[:, 0].copy()
    min2 = np.full(rows, MIN2_INIT, np.float32)
    idx = np.zeros(rows, np.int32)
    for j in range(1, cols):
        cur = D[:, j]
        lt1 = cur < min1
        lt2 = ~lt1 & (cur < min2)
        min2 = np.where(lt1, min1, np.where(lt2, cur, min2))
        idx = np.where(lt1, j, idx).astype(np.int32)
        min1 = np.where(lt1, cur, min1)
    live = min2 > 0
    with np.errstate(all="ignore"):
        ratio = (min1 / np.where(live, min2, np.float32(1))).astype(np.float32)
    res[live] = np.where(ratio[live] < np.float32(ambiguity), idx[live], -1)
    return res


def expected(case, capA):
    """What the entry leaves in a result row of capA entries pre-filled with case['prior']."""
    nA, nB = min(max(case["nA"], 0), capA), max(case["nB"], 0)
    res = np.full(capA, case["prior"], np.int32)
    if nA > 0 and nB > 0:
        res[:nA] = scan(distances(case["A"][:nA], case["B"][:nB]), case["amb"], res[:nA])
    return res


def _case(A, B, amb=0.8, nA=None, nB=None, prior=-7, what=""):
    return dict(A=np.ascontiguousarray(A, np.uint8), B=np.ascontiguousarray(B, np.uint8), amb=amb,
                nA=len(A) if nA is None else nA, nB=len(B) if nB is None else nB, prior=prior, what=what)


def random_case(seed, rows_a, rows_b, amb=0.8):
    """Asymmetric random bytes over the whole range; a third of the queries get a near copy among the candidates (a clear
    match), some of those a second near copy (an ambiguous one)."""
    rng = np.random.default_rng(seed)
    A = rng.integers(0, 256, (rows_a, 128))
    B = rng.integers(0, 256, (rows_b, 128))
    for i in range(0, rows_a, 3):
        j = int(rng.integers(0, rows_b))
        B[j] = np.clip(A[i] + rng.integers(-6, 7, 128), 0, 255)
        if i % 2 == 0 and rows_b > 2:
            B[int(rng.integers(0, rows_b))] = np.clip(A[i] + rng.integers(-7, 8, 128), 0, 255)
    return _case(A, B, amb, what="random %d x %d" % (rows_a, rows_b))


def mixed_size_cases():
    shapes = [(1, 1), (1, 2), (2, 1), (31, 33), (32, 32), (33, 31), (127, 129), (128, 128), (129, 127), (257, 2), (2, 257),
              (257, 257), (1, 257), (257, 1), (32, 129), (129, 32), (128, 33), (31, 128)]
    assert {s for p in shapes for s in p} == set(SIZES)
    return [random_case(40 + k, a, b) for k, (a, b) in enumerate(shapes)]


def extremes_case():
    """Rows of all 0 against all 255: the largest distance, both ends of the signed shift."""
    A = np.zeros((40, 128), np.uint8)
    A[1::2] = 255
    A[5, :7] = 9
    B = np.zeros((70, 128), np.uint8)
    B[::3] = 255
    B[4, 100:] = 254
    B[37, :50] = 1
    return [_case(A, B, amb, what="extremes, ambiguity %g" % amb) for amb in (0.8, 1.0, 1.5)]


def duplicate_cases():
    """Duplicate candidate rows 1, 4, 32 and 33 apart and across a tile boundary (rows 31 | 32). Query t sits at the same
    non-zero distance from both copies of pair t (an exact tie: only an ambiguity above 1 shows the index, and the lowest
    must win in every merge); query 5 + t EQUALS both copies (min2 == 0: the pre-filled entry is kept)."""
    rng = np.random.default_rng(11)
    B = rng.integers(0, 256, (140, 128))
    pairs = [(3, 4), (8, 12), (20, 52), (60, 93), (31, 32)]
    A = rng.integers(0, 256, (12, 128))
    for t, (j0, j1) in enumerate(pairs):
        B[j1] = B[j0]
        A[t] = B[j0]
        A[t, t] = B[j0, t] + (3 if B[j0, t] < 200 else -3)
        A[5 + t] = B[j0]
    out = [_case(A, B, amb, what="duplicates, ambiguity %g" % amb) for amb in (0.8, 1.0, 1.5)]
    want = expected(out[2], 12)
    assert want[:5].tolist() == [p[0] for p in pairs] and (want[5:10] == -7).all()
    assert (expected(out[1], 12)[:5] == -1).all()               # 1.0 on an exact tie: 1 < 1 is false
    return out


def single_candidate_cases():
    """nB = 1: min2 keeps its start value 2139095040.0f; a tiny ambiguity splits the rows by d / 2139095040 < ambiguity."""
    rng = np.random.default_rng(12)
    B = rng.integers(0, 256, (1, 128))
    A = np.clip(B + rng.integers(-1, 2, (33, 128)) * rng.integers(0, 90, (33, 1)), 0, 255)
    A[7] = B[0]                                                 # min1 = 0: 0 / 2139095040 < ambiguity, index 0
    out = [_case(A, B, amb, what="one candidate, ambiguity %g" % amb) for amb in (0.8, 1e-4)]
    want = expected(out[1], 33)
    assert 5 < (want == 0).sum() < 28 and ((want == 0) | (want == -1)).all() and (expected(out[0], 33) == 0).all()
    return out


def all_cases():
    return mixed_size_cases() + extremes_case() + duplicate_cases() + single_candidate_cases()


def ragged_batch(n, seed=0):
    """n pairs in buffers of one capacity with sizes of their own, one of them empty; the rows beyond a pair's sizes are
    random bytes (reading one of them changes a result)."""
    rng = np.random.default_rng(100 + n + seed)
    capA, capB = 150, 140
    cases = []
    for k in range(n):
        c = random_case(200 + 7 * n + k, capA, capB, amb=(0.8, 1.0)[k % 2])
        c["nA"], c["nB"] = int(rng.choice(SIZES[:-1] + (150, 1000))), int(rng.choice(SIZES[:-1] + (140, 1000)))
        if k == n // 2:
            c["nA" if n % 2 else "nB"] = (0, -3)[k % 2]         # the empty pair
        c["nA"], c["nB"] = min(c["nA"], 1000), min(c["nB"], 1000)
        c["what"] = "ragged %d/%d: %d x %d" % (k, n, c["nA"], c["nB"])
        cases.append(c)
    return cases, capA, capB


def shared_scan_cases():
    """The smallest shapes at which one list kernel behind both entries can differ from a top-2 kernel, in buffers of 300 x
    40 rows (random bytes beyond the sizes). Returns ([one candidate, two identical candidates, empty, ties], capA, capB):
      one candidate   65 x 1: no second candidate; row 7 equals the candidate (min1 = 0, index 0);
      identical       65 x 2, B[0] == B[1]: min2 == min1 everywhere (never below ambiguity <= 1); rows 0..31 equal them,
                      min2 == 0, the entry keeps its prior;
      empty           0 x 33;
      ties            257 x 33, one row into the second tile: B[5] == B[1] (the two lane halves of one tile), B[32] == B[0]
                      (across the tile boundary); query 10 is equally near rows 1 and 5, query 11 rows 0 and 32, nearer
                      than to any other row.
    nA = 65 is one row past a wave, 257 one past a workgroup."""
    rng = np.random.default_rng(13)
    capA, capB = 300, 40
    fresh = lambda: (rng.integers(0, 256, (capA, 128)), rng.integers(0, 256, (capB, 128)))
    A1, B1 = fresh()
    A1[7] = B1[0]
    A2, B2 = fresh()
    B2[1] = B2[0]
    A2[:32] = B2[0]
    A3, B3 = fresh()
    A4, B4 = fresh()
    B4[5], B4[32] = B4[1], B4[0]
    for q, j in ((10, 1), (11, 0)):
        A4[q] = B4[j]
        A4[q, q] += 3 if A4[q, q] < 200 else -3
    cases = [_case(A1, B1, nA=65, nB=1, what="65 x 1"), _case(A2, B2, nA=65, nB=2, what="65 x 2 identical candidates"),
             _case(A3, B3, nA=0, nB=33, what="empty, 0 x 33"), _case(A4, B4, nA=257, nB=33, what="257 x 33 with ties")]
    D = distances(A4[:257], B4[:33])
    assert D[10, 1] == D[10, 5] == 9 == D[11, 0] == D[11, 32] and (np.sort(D[10:12], axis=1)[:, 2] > 9).all()
    assert (distances(A2[:32], B2[:2]) == 0).all() and distances(A2[32:65], B2[:2]).min() > 0
    return cases, capA, capB


def expected_clipped(case, capA, capB):
    c = dict(case, nB=min(max(case["nB"], 0), capB))
    return expected(c, capA)
