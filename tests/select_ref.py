"""An independent numpy model of the keypoint selection (include/nm_abi.h, nm_sift_select_batch_dev). Nothing here is
shared with the product: the rule is restated as one sort by the precedence tuple.

The default score is accumulated in float32 in the finish's order: lane partial fmaf(b, b, a * a), then the xor butterfly
d = 32, 16, 8, 4, 2, 1. numpy has no float32 fma; fma32() emulates it through float64. a * a is rounded to float32 first (that
is what the product writes). b * b is formed in float64, where the product of two 24-bit significands (48 bits) is EXACT.
Adding the float32 addend in float64 is exact while the addend lies within about [2^-28, 2^4] of the product (the sum then
fits 53 bits), which covers these magnitudes: histogram elements of one row span far less. So that the emulation is right
outside that range too, the addition's rounding error is recovered (TwoSum) and, where it is not zero, folded into the last
bit of the float64 sum (round to odd): a value rounded to odd at 53 bits rounds to the correctly rounded 24-bit result,
because 53 >= 24 + 2. The tests check the outcome against the float64 sum of desc_finish_ref's step 1 to its 8 u bound, and
bit for bit against the host twin on real descriptors.
"""
import numpy as np

U = 2.0 ** -24


def fma32(b, c):
    """float32 fmaf(b, b, c) for float32 arrays b, c: exact product, TwoSum, round to odd, one rounding to float32."""
    p = b.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)                  # s + e = p + c exactly
    even = (s.view(np.int64) & 1) == 0
    nudge = np.isfinite(s) & (e != 0) & even
    s = np.where(nudge, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def default_scores(desc):
    """(rows, 128) float32 -> float32 squared norms in the finish's operation order."""
    v = np.asarray(desc, np.float32).reshape(-1, 128)
    a, b = v[:, 0::2], v[:, 1::2]
    with np.errstate(all="ignore"):
        p = fma32(b, (a * a).astype(np.float32))
        lanes = np.arange(64)
        for d in (32, 16, 8, 4, 2, 1):
            p = (p + p[:, lanes ^ d]).astype(np.float32)
    return p[:, 0].copy()


def pixel(v, size):
    v = np.asarray(v, np.float32)
    out = np.zeros(v.shape, np.int64)
    ok = v >= 0                                  # NaN fails
    big = ok & (v >= size)
    mid = ok & ~big
    out[big] = size - 1
    out[mid] = np.floor(v[mid].astype(np.float64)).astype(np.int64)
    return out


def cells(x, y, width, height, gx, gy):
    cw, ch = -(-width // gx), -(-height // gy)
    return (pixel(y, height) // ch) * gx + pixel(x, width) // cw


def ranking(scores):
    s = np.asarray(scores, np.float32)
    with np.errstate(all="ignore"):
        ok = np.isfinite(s) & (s > 0)
    return np.where(ok, s, np.float32(0)).astype(np.float32)


def select(count, capacity, x, y, scores, width, height, gx, gy, keep):
    """The source rows of the output, ascending, and the model's internals {u, cell, round} over the m rows."""
    m = min(max(int(count), 0), capacity)
    u = ranking(np.asarray(scores)[:m])
    cell = cells(np.asarray(x)[:m], np.asarray(y)[:m], width, height, gx, gy)
    rnd = np.zeros(m, np.int64)
    for c in np.unique(cell):
        rows = np.nonzero(cell == c)[0]
        order = sorted(rows, key=lambda i: (-float(u[i]), i))      # beats: higher score, then earlier row
        for r, i in enumerate(order):
            rnd[i] = r
    order = sorted(range(m), key=lambda i: (rnd[i], -float(u[i]), i))
    chosen = np.array(sorted(order[:min(keep, m)]), np.int64)
    return chosen, dict(u=u, cell=cell, round=rnd)


def check_properties(chosen, info, keep):
    """What follows from the rule, asserted on any claimed output."""
    u, cell, rnd = info["u"], info["cell"], info["round"]
    m = u.size
    assert chosen.size == min(keep, m) and (np.diff(chosen) > 0).all()
    picked = np.zeros(m, bool)
    picked[chosen] = True
    sizes, taken = {}, {}
    for c in np.unique(cell):
        rows = cell == c
        sizes[c], taken[c] = int(rows.sum()), int(picked[rows].sum())
        assert set(rnd[rows & picked]) == set(range(taken[c])), "a cell's selected rows are its best prefix"
    for c in sizes:
        for d in sizes:
            if taken[c] + 1 < taken[d]:
                assert taken[c] == sizes[c], "counts differ by more than one only when the smaller cell is exhausted"
    if keep >= len(sizes):
        assert all(t >= 1 for t in taken.values()), "every non-empty cell has a selected row"
