"""Shared test helpers: synthetic frames built with the oracle's Gaussian."""
import numpy as np

import oracle_lib as O
from niftymatch_amd import synth


def blurred_frame(seed, width, height, sigma=None):
    f = synth.noise_frame(seed, width, height)
    taps, r = O.create_kernel_for_sigma(synth.preblur_sigma(width, height) if sigma is None else sigma)
    return O.convolve(f, taps, r)[0]


def ulp_err(got, ref64):
    ref32 = ref64.astype(np.float32)
    u = np.spacing(np.abs(ref32)).astype(np.float64)
    return np.max(np.abs(got.astype(np.float64) - ref64) / u)


def assert_distance(nm, D, Dref, what="distance matrix"):
    """The materialised `distance` of compute_sift_matches against the oracle's chain (match.cu:36-42). Mode "exact": bit for
    bit. Mode "mfma" (default; fp32 matrix cores on centred rows): EVERY entry within 1e-4 relative -- the tolerance the north
    star states for distance values -- which makes an exact zero exactly zero and keeps NaN / inf where the chain has them."""
    D = D.detach().cpu().numpy() if hasattr(D, "detach") else np.asarray(D)
    Dref = np.asarray(Dref)
    assert D.shape == Dref.shape, (what, D.shape, Dref.shape)
    if nm.get_distance_mode() == "exact":
        same = D.view(np.uint32) == Dref.view(np.uint32)
        assert same.all(), "%s: %d of %d elements differ" % (what, (~same).sum(), same.size)
        return
    fin = np.isfinite(Dref)
    assert np.array_equal(np.isnan(D), np.isnan(Dref)), what + ": NaN pattern"
    assert np.array_equal(D[~fin & ~np.isnan(Dref)], Dref[~fin & ~np.isnan(Dref)]), what + ": infinities"
    a, b = D[fin].astype(np.float64), Dref[fin].astype(np.float64)
    bad = np.abs(a - b) > 1e-4 * np.abs(b)
    assert not bad.any(), "%s: %d of %d entries off by more than 1e-4 relative (worst %g)" % (
        what, bad.sum(), bad.size, float(np.max(np.abs(a - b)[bad] / np.maximum(np.abs(b[bad]), 1e-300))))


def blob_field(seed, width, height):
    """Signed isotropic Gaussian blobs on a grey background, ~w*h/6000 of them with sigma log-uniform in [1.5, min(w,h)/24],
    rounded to integers and clipped to [0, 255]: keypoints at every scale (the deep octaves that blurred noise barely reaches),
    quantised plateaus and, where blobs saturate, flats with exact ties."""
    rng = np.random.default_rng(seed)
    img = np.full((height, width), 128.0, np.float64)
    n = max(1, int(width * height / 6000))
    s_hi = max(1.6, min(width, height) / 24.0)
    sig = np.exp(rng.uniform(np.log(1.5), np.log(s_hi), n))
    amp = rng.uniform(40.0, 160.0, n) * rng.choice([-1.0, 1.0], n)
    cx, cy = rng.uniform(0, width, n), rng.uniform(0, height, n)
    for s, a, x0, y0 in zip(sig, amp, cx, cy):
        r = int(np.ceil(4 * s))
        xa, xb = max(0, int(x0) - r), min(width, int(x0) + r + 1)
        ya, yb = max(0, int(y0) - r), min(height, int(y0) + r + 1)
        if xa >= xb or ya >= yb:
            continue
        gx = np.exp(-((np.arange(xa, xb) - x0) ** 2) / (2 * s * s))
        gy = np.exp(-((np.arange(ya, yb) - y0) ** 2) / (2 * s * s))
        img[ya:yb, xa:xb] += a * np.outer(gy, gx)
    return np.clip(np.rint(img), 0, 255).astype(np.float32)


def step_field(seed, width, height):
    """0/255 rectangles XOR-ed onto a 0 background (~w*h/8000 of them, sides log-uniform from 3 px to a quarter of the frame):
    step edges, flats whose gradient is exactly zero and dense exact ties in the DoG planes."""
    rng = np.random.default_rng(seed)
    on = np.zeros((height, width), bool)
    n = max(1, int(width * height / 8000))
    s_hi = max(4.0, min(width, height) / 4.0)
    rw = np.exp(rng.uniform(np.log(3.0), np.log(s_hi), n)).astype(int)
    rh = np.exp(rng.uniform(np.log(3.0), np.log(s_hi), n)).astype(int)
    x0, y0 = rng.integers(0, width, n), rng.integers(0, height, n)
    for x, y, a, b in zip(x0, y0, rw, rh):
        on[y: y + b, x: x + a] ^= True
    return np.where(on, np.float32(255.0), np.float32(0.0))
