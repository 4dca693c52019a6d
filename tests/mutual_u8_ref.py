"""An independent restatement of mutual-nearest-neighbour filtering over u8 descriptors (nm_sift_match_mutual_u8_*) and the
cases its host and GPU tests share.

Written from the entry's stated semantics in include/nm_abi.h, not from csrc/nm_match_mutual_u8.hip: the distances of every
claimed column to every row of A are an int64 matrix product on numpy arrays, the column's first minimum is numpy.argmin
(the first occurrence of the minimum), the forward distance is float32 of the integer. Everything is exact, so the product
must equal this with no tolerance and no excluded rows.

Every case family checks ON THIS RESTATEMENT ALONE that at least one claim is kept and at least one is removed (kept_removed),
so neither an all -1 output nor a pass-through of the match list can pass.

The sizes come from the entry's constants: 32 rows of A per matrix tile, 16 accumulator entries per lane holding the rows
(e & 3) + 8 (e >> 2) + 4 (lane >> 5) of a tile, 64 claims per wave, 256 rows / claims per workgroup, and 8 ranges of
ceil(ceil(nA / 32) / 8) tiles per pair.
"""
import numpy as np

INF = np.float32(np.inf)
SIZES = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257)
SPLIT_ROWS = 600                      # 19 tiles in ranges of 3: range boundaries at rows 96, 192, .., a ragged last range


def column_distances(A, B, cols):
    """(len(cols), len(A)) int64: d(i, j) for every row i of A and the listed columns j of B."""
    a, b = np.asarray(A, np.uint8).astype(np.int64), np.asarray(B, np.uint8)[cols].astype(np.int64)
    D = (b * b).sum(1)[:, None] + (a * a).sum(1)[None, :] - 2 * (b @ a.T)
    assert (D >= 0).all() and D.max(initial=0) <= 128 * 255 * 255
    return D


def mutual(A, nA, B, nB, matches, capA=None, capB=None):
    """One pair. Returns (result (capA,) int32, count, forward (capA,) float32)."""
    matches = np.asarray(matches, np.int32)
    capA = min(len(A), len(matches)) if capA is None else capA
    capB = len(B) if capB is None else capB
    nA, nB = min(max(int(nA), 0), capA), min(max(int(nB), 0), capB)
    result = np.full(capA, -1, np.int32)
    forward = np.full(capA, INF, np.float32)
    m = matches[:nA]
    rows = np.flatnonzero((m >= 0) & (m < nB))
    if len(rows) == 0:
        return result, 0, forward
    cols = np.unique(m[rows])
    D = column_distances(A[:nA], B, cols)
    first_min = D.argmin(axis=1)                                 # numpy: the first occurrence of the minimum
    c = np.searchsorted(cols, m[rows])
    forward[rows] = D[c, rows].astype(np.float32)
    keep = first_min[c] == rows
    result[rows[keep]] = m[rows[keep]]
    return result, int((result >= 0).sum()), forward


def expected(case, capA=None, capB=None):
    return mutual(case["A"], case["nA"], case["B"], case["nB"], case["m"], capA=capA, capB=capB)


def claims_of(case, capA=None, capB=None):
    capA = len(case["m"]) if capA is None else capA
    capB = len(case["B"]) if capB is None else capB
    nA, nB = min(max(case["nA"], 0), capA), min(max(case["nB"], 0), capB)
    m = case["m"][:nA]
    return int(((m >= 0) & (m < nB)).sum())


def kept_removed(cases, capA=None, capB=None):
    """(kept, removed) claims of a family according to the restatement; asserts that neither is zero."""
    kept = sum(expected(c, capA, capB)[1] for c in cases)
    removed = sum(claims_of(c, capA, capB) for c in cases) - kept
    assert kept >= 1 and removed >= 1, ([c["what"] for c in cases][:3], kept, removed)
    return kept, removed


def _case(A, B, m, nA=None, nB=None, what=""):
    A, B = np.ascontiguousarray(A, np.uint8), np.ascontiguousarray(B, np.uint8)
    m = np.ascontiguousarray(m, np.int32)
    assert len(m) == len(A)
    return dict(A=A, B=B, m=m, nA=len(A) if nA is None else nA, nB=len(B) if nB is None else nB, what=what)


def random_case(seed, nA, nB, pad=5, claims=None, what=None):
    """Asymmetric random bytes over the whole range in buffers of nA + pad and nB + pad rows. A third of A's rows get a near
    copy among the columns; every seventh row of A is the twin of the row before it (an exact tie on every column). The
    match list: a row claims its nearest column (`claims`: how many rows do, default about 60 %), every fourth claiming row
    is moved onto a column another row already claims, one row claims the last column, the other rows carry -1, -5, nB and
    nB + 7. The entries beyond nA hold numbers of real columns and must never be read as claims."""
    rng = np.random.default_rng(seed)
    A = rng.integers(0, 256, (nA + pad, 128))
    B = rng.integers(0, 256, (nB + pad, 128))
    for i in range(0, nA, 3):
        B[int(rng.integers(0, nB))] = np.clip(A[i] + rng.integers(-6, 7, 128), 0, 255)
    for i in range(6, nA, 7):
        A[i] = A[i - 1]
    A, B = A.astype(np.uint8), B.astype(np.uint8)
    m = np.array([(-1, -5, nB, nB + 7)[i % 4] for i in range(nA + pad)], np.int32)
    m[nA:] = np.arange(pad) % nB
    order = rng.permutation(nA)
    rows = np.sort(order[:int(0.6 * nA + 1) if claims is None else claims])
    if len(rows):
        a, b = A[rows].astype(np.int64), B[:nB].astype(np.int64)
        near = ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)).argmin(1)
        m[rows] = near
        for t in range(3, len(rows), 4):
            m[rows[t]] = m[rows[t - 3]]
        if claims is None:
            m[rows[-1]] = nB - 1
    return _case(A, B, m, nA, nB, what or "random %d x %d" % (nA, nB))


def size_cases():
    shapes = [(1, 1), (1, 33), (31, 257), (32, 32), (33, 31), (63, 65), (64, 64), (65, 63), (255, 1), (256, 256), (257, 255),
              (SPLIT_ROWS, 257), (289, 64)]
    assert {s for p in shapes for s in p} >= set(SIZES)
    cases = [random_case(70 + k, a, b) for k, (a, b) in enumerate(shapes)]
    kept_removed(cases)
    kept_removed(cases[-2:])                                   # and in the two that straddle a range boundary on their own
    return cases


def claim_count_cases():
    cases = [random_case(90 + c, 300, 280, claims=c, what="300 x 280, %d claims" % c) for c in (0, 1, 64, 65, 300)]
    assert [claims_of(c) for c in cases] == [0, 1, 64, 65, 300]
    kept_removed(cases)
    return cases


# tied pairs of rows of A, (lower, higher), one per merge of the scan over SPLIT_ROWS rows
TIED_ROWS = [(0, 1),        # inside one lane's 16 accumulator entries (e = 0, 1)
             (8, 16),       # inside one lane, e = 4 and 8
             (2, 6),        # across the two lane halves
             (31, 32),      # across tiles
             (63, 64),      # across waves of the claims kernel
             (255, 256),    # across workgroups of the claims kernel
             (95, 96),      # across split ranges (tiles 2 | 3)
             (100, 500)]    # far apart: ranges 1 and 5


def duplicate_cases():
    """A[lo] == A[hi] for every pair of TIED_ROWS, both one small step from column j = 3 t of B (so the pair is the column's
    nearest and an exact tie). Three match lists over the same rows: the lower twin claims alone (kept), the higher twin
    claims alone (removed: the first index wins), both claim (one-to-one: the lower one stays)."""
    rng = np.random.default_rng(21)
    A = rng.integers(0, 256, (SPLIT_ROWS, 128)).astype(np.uint8)
    B = rng.integers(0, 256, (40, 128)).astype(np.uint8)
    for t, (lo, hi) in enumerate(TIED_ROWS):
        A[lo] = B[3 * t]
        A[lo, t] = B[3 * t, t] + (3 if B[3 * t, t] < 200 else -3)
        A[hi] = A[lo]
    A[301] = B[39]
    out = []
    for who, what in ((0, "the lower twin claims"), (1, "the higher twin claims"), (2, "both twins claim")):
        m = np.full(SPLIT_ROWS, -1, np.int32)
        for t, (lo, hi) in enumerate(TIED_ROWS):
            if who in (0, 2):
                m[lo] = 3 * t
            if who in (1, 2):
                m[hi] = 3 * t
        m[300], m[301] = 0, 39                                   # a far row on a twin's column (removed), a lone claim (kept)
        out.append(_case(A, B, m, what="duplicates: " + what))
    los, his = [p[0] for p in TIED_ROWS], [p[1] for p in TIED_ROWS]
    r0, r1, r2 = (expected(c)[0] for c in out)
    assert (r0[los] >= 0).all() and (r1[his] == -1).all() and (r2[los] >= 0).all() and (r2[his] == -1).all()
    for c in out:
        kept_removed([c])
    return out


def shared_column_case():
    """Forty rows claim column 0 and thirty column 9; each column's nearest row is in the middle of its claimants."""
    rng = np.random.default_rng(22)
    A = rng.integers(0, 256, (130, 128)).astype(np.uint8)
    B = rng.integers(0, 256, (20, 128)).astype(np.uint8)
    A[57] = B[0]
    A[57, 0] ^= 1
    A[101] = B[9]
    m = np.full(130, -1, np.int32)
    m[30:70] = 0
    m[90:120] = 9
    c = _case(A, B, m, what="several rows claim one column")
    want = expected(c)[0]
    assert np.flatnonzero(want >= 0).tolist() == [57, 101]
    kept_removed([c])
    return [c]


def extremes_case():
    """Rows of all 0 against all 255: d = 128 * 255^2, both ends of the signed shift (byte ^ 0x80)."""
    A = np.zeros((70, 128), np.uint8)
    A[1::2] = 255
    A[5, :7] = 9
    B = np.zeros((40, 128), np.uint8)
    B[::3] = 255
    B[4, 100:] = 254
    m = np.full(70, -1, np.int32)
    m[0], m[1], m[2], m[3], m[5], m[8], m[9] = 0, 0, 1, 1, 1, 4, 39      # claims at d = 0, the largest d, ties of whole blocks
    c = _case(A, B, m, what="0 against 255")
    assert column_distances(A, B, [0]).max() == 128 * 255 * 255 and expected(c)[2][0] == np.float32(128 * 255 * 255)
    kept_removed([c])
    return [c]


def clip_cases():
    base = random_case(23, 120, 130, pad=0)
    cases = [dict(base, nA=10 ** 6, nB=10 ** 6, what="sizes above the capacities"), dict(base, nA=-4, what="nA negative"),
             dict(base, nB=-1, what="nB negative"), dict(base, nA=0, nB=0, what="both sizes zero"),
             dict(base, nA=31, nB=50, what="partial sizes")]
    for c in cases[1:4]:
        assert expected(c)[1] == 0 and (expected(c)[0] == -1).all() and np.isinf(expected(c)[2]).all()
    kept_removed(cases)
    return cases


def all_cases():
    return size_cases() + claim_count_cases() + duplicate_cases() + shared_column_case() + extremes_case() + clip_cases()


def ragged_batch(n):
    """n pairs in buffers of one capacity with sizes of their own (some above the capacity), one of them empty; the rows
    beyond a pair's sizes are random bytes and its match entries beyond nA name real columns."""
    rng = np.random.default_rng(300 + n)
    capA, capB = 150, 140
    cases = []
    for k in range(n):
        c = random_case(400 + 7 * n + k, capA, capB, pad=0)
        c["nA"], c["nB"] = int(rng.choice(SIZES[:7] + (150, 1000))), int(rng.choice(SIZES[:7] + (140, 1000)))
        if k == n // 2:
            c["nA" if n % 2 else "nB"] = (0, -3)[k % 2]         # the empty pair
        c["what"] = "ragged %d/%d: %d x %d" % (k, n, c["nA"], c["nB"])
        cases.append(c)
    if n > 1:
        kept_removed(cases, capA, capB)
    return cases, capA, capB
