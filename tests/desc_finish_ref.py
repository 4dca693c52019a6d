"""A float64 restatement of the descriptor finish (include/nm_abi.h, nm_sift_desc_finish_batch_dev) and the checks the
finish tests run against it. Nothing here is shared with the product: numpy sums in float64, in numpy's own order.

The bound. u = 2^-24 is the unit roundoff of binary32. Every input element is >= 0, so no sum cancels and the relative
errors of the terms carry over to the sum. To first order, per operation count:
  s  = sum v^2   : a product (u) and an fma (u) in the lane partial, six butterfly additions (6 u)        ->  8 u
  d  = sqrt(s)   : half the argument's error plus its own rounding                                       ->  5 u
  v1 = v / d     : the divisor's error plus its own rounding                                             ->  6 u
  clip           : min(v1, 0.2f) moves no value by more than v1 itself was off                           ->  6 u
  s2 = sum v1^2  : twice the element error (12 u), product and fma (2 u), six additions (6 u)             -> 20 u
  v2 = v1 / sqrt(s2) : 6 u + (10 u + u) + u                                                              -> 18 u   (NM_DESC_L2)
  t  = sum v2    : 18 u, the lane's addition (u), six additions (6 u)                                    -> 25 u
  v3 = sqrt(v2 / t) : half of (18 u + 25 u + u), plus its own rounding                                   -> 23 u   (NM_DESC_ROOT)
REL = 24 u covers both modes with the second-order terms (24 u)^2 to spare. It holds where the intermediate values are
normal numbers; a result in the subnormal range carries up to 2^-150 per operation instead, eight operations at the
most: FLOOR = 2^-146 for L2, and, since |sqrt(a) - sqrt(b)| <= sqrt|a - b|, sqrt(2^-146) = 2^-73 for RootSIFT. Rows whose
SQUARES are subnormal without all being zero (elements around 1e-20) are outside the bound's domain: s itself is then
only known to 2^-150 absolute.

The zero rule is stated on the binary32 sum: the model sums in float64 and applies the rule when that sum, rounded to
binary32, is zero or not finite (a row of 1e-30 sums to 1.3e-58: zero in binary32).
"""
import numpy as np

U = 2.0 ** -24
REL = 24 * U
FLOOR = {0: 2.0 ** -146, 1: 2.0 ** -73}
CLIP = float(np.float32(0.2))
L2, ROOT = 0, 1


def model(rows, mode, clip=True, renorm=True):
    """float64 rows of the finish. clip / renorm switch steps off: the mutants the tests must reject."""
    v = np.asarray(rows, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        s = (v * v).sum(1)
        s32 = s.astype(np.float32)
        live = np.isfinite(s32) & (s32 > 0)
        out = np.zeros_like(v)
        w = v[live] / np.sqrt(s[live])[:, None]
        if clip:
            w = np.minimum(w, CLIP)
        if renorm:
            w = w / np.sqrt((w * w).sum(1))[:, None]
        if mode == ROOT:
            w = np.sqrt(w / w.sum(1)[:, None])
        out[live] = w
    return out, live


def codes(f, truncate=False):
    y = 512.0 * f
    return np.minimum(255, np.floor(y) if truncate else np.rint(y)).astype(np.int64)


def near_half(f, mode):
    """Elements whose 512 v lies within the bound of a half-integer: the only ones whose code may differ by 1."""
    y = 512.0 * f
    return np.abs(y - np.floor(y) - 0.5) <= 512.0 * (REL * f + FLOOR[mode])


def check(got_f32, got_u8, rows, mode, truncate=False, **mutant):
    """All the checks of one output set against the model (or a mutant of it). Returns the share of excepted codes."""
    f, live = model(rows, mode, **mutant)
    if got_f32 is not None:
        g = np.asarray(got_f32, np.float32).astype(np.float64)
        err = np.abs(g - f)
        lim = REL * f + FLOOR[mode]
        assert (err <= lim).all(), ("fp32 outside the bound", float((err / np.maximum(lim, 1e-300)).max()))
        norm = np.sqrt((g[live] * g[live]).sum(1))
        assert (np.abs(norm - 1.0) <= REL).all(), ("unit norm", float(np.abs(norm - 1.0).max()) if live.any() else 0.0)
        assert (np.asarray(got_f32)[~live].view(np.uint32) == 0).all(), "zero rule (fp32)"
    near = near_half(f, mode)
    if got_u8 is not None:
        want = codes(f, truncate)
        diff = np.abs(np.asarray(got_u8).astype(np.int64) - want)
        assert ((diff == 0) | (near & (diff <= 1))).all(), ("codes", int((diff != 0).sum()), int(((diff != 0) & ~near).sum()))
        assert (np.asarray(got_u8)[~live] == 0).all(), "zero rule (u8)"
    return float(near.mean())
