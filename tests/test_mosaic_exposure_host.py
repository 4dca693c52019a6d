"""The host twins of the mosaic exposure compensation (nm_mosaic_exposure_sums_host, nm_mosaic_gains_host) against the numpy
model of tests/exposure_ref.py: the sums exactly (integers), the gains within exposure_ref.gain_bound (derived there), the
refusals one by one, and mutants of the model that the same checks must reject. The cases are shared with the device test
(tests/test_gpu_mosaic_exposure.py), which asks the device for the host twins' bits."""
import ctypes as C

import numpy as np
import pytest

import exposure_ref as X
import loop_closure_ref as LC

F32 = np.float32
INVALID = 1                                   # hipErrorInvalidValue


def frame(seed, fw, fh, lo=20, hi=235):
    """a smooth BGRA frame with all colour bytes in [lo, hi], clipped to bytes (lo < 0 or hi > 255: a frame with clipped areas)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:fh, 0:fw]
    out = np.empty((fh, fw, 4), np.uint8)
    for c in range(3):
        f = rng.uniform(0.05, 0.25, 4)
        v = np.sin(f[0] * xx + f[1] * yy + c) + np.cos(f[2] * xx - f[3] * yy)
        out[..., c] = np.clip(lo + (hi - lo) * (v + 2) / 4 + rng.integers(-3, 4, (fh, fw)), max(lo, 0), min(hi, 255))
    out[..., 3] = 255
    return out


def maps(fw, fh):
    """name -> H (float32 9): inside, leaving B on every side, a non-positive denominator over part of the lattice, non-finite"""
    return dict(
        inside=np.array([1.01, 0.02, 2.3, -0.015, 0.99, 1.7, 1e-5, -2e-5, 1], F32),
        leaves=np.array([1.6, 0.05, -0.2 * fw, -0.04, 1.7, -0.25 * fh, 1e-5, 1e-5, 1], F32),
        denominator=np.array([1, 0, 0.4, 0, 1, 0.6, -2.0 / fw, 0, 1], F32),
        nonfinite=np.array([1, 0, 0, 0, np.nan, 0, 0, 0, 1], F32))


def disc_mask(fw, fh):
    yy, xx = np.mgrid[0:fh, 0:fw]
    return (((xx - 0.55 * fw) ** 2 / (0.52 * fw) ** 2 + (yy - 0.5 * fh) ** 2 / (0.49 * fh) ** 2) < 1).astype(F32)


SIZES = [(67, 45), (131, 97)]
STRIDES = [1, 3, 4, 64]


def sums_case(fw, fh):
    """frames and one link per map, a -> b and reversed"""
    frames = [frame(10 + k, fw, fh, lo=-60 if k == 2 else 20, hi=315 if k == 2 else 235) for k in range(3)]
    H = maps(fw, fh)
    names = list(H)
    link_a = [k % 3 for k in range(len(names))] + [1]
    link_b = [(k + 1) % 3 for k in range(len(names))] + [0]
    Hs = np.stack([H[k] for k in names] + [H["inside"]])
    return frames, link_a, link_b, Hs


@pytest.mark.parametrize("fw,fh", SIZES)
@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("masked", [False, True])
def test_host_sums_equal_the_integer_model(nm, fw, fh, stride, masked):
    frames, la, lb, Hs = sums_case(fw, fh)
    mask = disc_mask(fw, fh) if masked else None
    got = {}
    for lo, hi in ((5, 250), (0, 255)):
        got[lo] = nm.mosaic_exposure_sums_host(frames, la, lb, Hs, mask=mask, stride=stride, lo=lo, hi=hi)
        want = X.link_sums(frames, la, lb, Hs, mask=mask, stride=stride, lo=lo, hi=hi)
        assert got[lo].tolist() == want, (stride, lo, hi)
        assert got[lo][3].tolist() == [0] * 7               # the non-finite map
    if stride == 1 and not masked:
        full, tight = got[0], got[5]
        assert 0 < full[1, 0] < fw * fh and 0 < full[2, 0] < fw * fh       # the maps leave B / lose the denominator
        assert full[0, 0] >= 0.8 * fw * fh                                 # the inside map keeps most of the lattice
        assert (tight[[1, 2], 0] < full[[1, 2], 0]).all()                  # frame 2 holds clipped bytes


def test_status_gates_a_link(nm):
    frames, la, lb, Hs = sums_case(67, 45)
    status = np.array([1, 0, 2, 1, -1], np.int32)
    got = nm.mosaic_exposure_sums_host(frames, la, lb, Hs, link_status=status, stride=3)
    assert got.tolist() == X.link_sums(frames, la, lb, Hs, link_status=status, stride=3)
    assert not got[[1, 2, 4]].any() and got[0].all()


def test_one_tap_byte_of_one_channel_out_of_range_excludes_the_pixel(nm):
    fw, fh = 67, 45
    A, B = frame(1, fw, fh, 100, 150), frame(2, fw, fh, 100, 150)
    H = np.array([1, 0, 0.5, 0, 1, 0.5, 0, 0, 1], F32)       # four taps of weight 1/4 each
    clean = nm.mosaic_exposure_sums_host([A, B], [0], [1], H, stride=1, lo=5, hi=250)
    B2 = B.copy()
    B2[20, 30, 1] = 255                                      # one byte of G; it is a tap of the four pixels (29..30, 19..20)
    got = nm.mosaic_exposure_sums_host([A, B2], [0], [1], H, stride=1, lo=5, hi=250)
    assert got.tolist() == [X.sums_int(A, B2, H, stride=1, lo=5, hi=250)]
    assert int(clean[0, 0]) - int(got[0, 0]) == 4
    assert got.tolist() != [X.sums_int(A, B2, H, stride=1, lo=5, hi=250, a_only=True)]      # MUTANT: the test on A only
    B3 = B.copy()
    B3[20, 30, 3] = 0                                        # alpha is not looked at
    assert nm.mosaic_exposure_sums_host([A, B3], [0], [1], H, stride=1).tolist() == clean.tolist()
    A2 = A.copy()
    A2[10, 10, 2] = 3                                        # one byte of A's R below lo
    got = nm.mosaic_exposure_sums_host([A2, B], [0], [1], H, stride=1, lo=5, hi=250)
    assert int(clean[0, 0]) - int(got[0, 0]) == 1 and got.tolist() == [X.sums_int(A2, B, H, stride=1)]


# ---- the solve ----------------------------------------------------------------------------------------------------------
def synthetic_sums(n, L, seed, dead_frame=None, few=()):
    """links over n frames with known exposures t_k: sums as an overlap of N pixels of mean m would give them. Returns
    (link_a, link_b, sums (L, 7) uint64, t (n, 3)). Links repeat and come in both directions; frame dead_frame has no
    link; the links in `few` hold fewer than 64 pixels."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.8, 1.25, (n, 3))
    live = [k for k in range(n) if k != dead_frame]
    la, lb, S = [], [], []
    for l in range(L):
        if len(live) < 2:
            a, b = 0, 1
        elif l < len(live) - 1:
            a, b = live[l], live[l + 1]                      # a chain first, so that the live frames are connected
        else:
            a, b = rng.choice(live, 2, replace=False)
        if l % 3 == 1:
            a, b = b, a
        if l % 7 == 6 and l > 0:
            a, b = la[l - 1], lb[l - 1]                      # a repeated link
        N = 20 if l in few else int(rng.integers(500, 40000))
        m = rng.uniform(60, 160, 3)
        S.append([N] + [int(round(N * m[c] * t[a, c])) for c in range(3)] + [int(round(N * m[c] * t[b, c])) for c in range(3)])
        la.append(int(a))
        lb.append(int(b))
    return la, lb, np.array(S, np.uint64), t


SOLVE_CASES = [(2, 1, None), (2, 3, None), (5, 3, 4), (5, 65, None), (64, 65, 17), (64, 256, None), (5, 256, 2)]


def check_gains(nm, n, la, lb, S, mode, twin, **kw):
    g, stats = twin(n, la, lb, S, mode=mode, **kw)
    ref, raw, rs = X.solve_f64(n, la, lb, S.tolist(), mode=mode, **{k: v for k, v in kw.items() if k != "link_status"},
                               link_status=kw.get("link_status"))
    bound = X.gain_bound(ref, n, len(la), kw.get("sigma_n", 10.0), kw.get("sigma_g", 0.1))
    assert (np.abs(g.astype(np.float64) - ref) <= bound).all(), np.abs(g - ref).max()
    assert not np.isnan(g).any() and not np.isnan(stats).any()
    assert (stats[6], stats[7], stats[8]) == (rs["links"], rs["frames"], rs["end"])
    np.testing.assert_allclose(stats[:3], rs["cost_unit"], rtol=1e-9)
    np.testing.assert_allclose(stats[3:6], rs["cost"], rtol=1e-6, atol=1e-9 * max(rs["cost_unit"]))
    assert (stats[3:6] <= stats[:3]).all()
    return g, stats, ref, raw


@pytest.mark.parametrize("n,L,dead", SOLVE_CASES)
@pytest.mark.parametrize("mode", [X.PER_CHANNEL, X.COMMON])
def test_host_gains_against_numpy_solve(nm, n, L, dead, mode):
    la, lb, S, t = synthetic_sums(n, L, 100 * n + L, dead_frame=dead, few=(1,) if L > 2 else ())
    g, stats, ref, raw = check_gains(nm, n, la, lb, S, mode, nm.mosaic_gains_host)
    if dead is not None:
        assert (g[dead] == 1.0).all()                        # exactly
    if mode == X.COMMON:
        assert (g[:, 0] == g[:, 1]).all() and (g[:, 0] == g[:, 2]).all()
    elif L >= n:                                             # the gains pull the exposures together
        live = [k for k in range(n) if k != dead]
        assert (X.spread(g[live], t[live]) < X.spread(np.ones((len(live), 3)), t[live])).all()
    # MUTANTS of the model: the product must NOT agree with them
    for kw in (dict(swap=True), dict(prior=False)):
        bad = X.solve_f64(n, la, lb, S.tolist(), mode=mode, **kw)[0]
        assert (np.abs(g - bad) > X.gain_bound(bad, n, L)).any(), kw


def test_no_usable_link_ends_no_link_with_unit_gains(nm):
    la, lb, S, _ = synthetic_sums(5, 6, 3)
    for kw in (dict(link_status=np.zeros(6, np.int32)), dict(min_pixels=10 ** 6)):
        g, stats = nm.mosaic_gains_host(5, la, lb, S, **kw)
        assert (g == 1.0).all() and stats.tolist() == [0.0] * 6 + [0.0, 0.0, float(X.END_NO_LINK)]


def test_the_clamp_acts_on_both_sides(nm):
    la, lb = [0], [1]
    S = np.array([[1000, 200000, 200000, 200000, 50000, 50000, 50000]], np.uint64)       # a four times brighter than b
    kw = dict(sigma_g=10.0, sigma_n=1.0, g_min=0.9, g_max=1.1)
    g, stats, ref, raw = check_gains(nm, 2, la, lb, S, X.PER_CHANNEL, nm.mosaic_gains_host, **kw)
    assert (raw[0] < 0.9).all() and (raw[1] > 1.1).all()
    assert (g[0] == F32(0.9)).all() and (g[1] == F32(1.1)).all()


def test_high_overlap_pairs_of_the_loop_scene_are_all_usable():
    """The condition of the device's end-to-end test (tests/test_gpu_mosaic_exposure.py): with its lo, hi, min_pixels and
    factors the float64 model finds every high-overlap pair usable on the scaled views, so that test leaves out no link."""
    import test_gpu_mosaic_exposure as G
    views, t = G.scaled_views(G.host_views(91))
    pairs = LC.high_pairs()
    assert len(pairs) >= LC.K
    H = np.stack([LC.pair_map(a, b).astype(F32).reshape(9) for a, b in pairs])
    S = X.link_sums(views, [a for a, _ in pairs], [b for _, b in pairs], H, stride=G.STRIDE, lo=G.LO, hi=G.HI)
    assert min(s[0] for s in S) >= G.MIN_PIXELS, [s[0] for s in S]


# ---- refusals -------------------------------------------------------------------------------------------------------------
def _ints(v):
    return (C.c_int * len(v))(*v)


def test_sums_refusals(nm):
    lib = nm.lib()
    fw, fh = 16, 8
    A = np.full((fh, fw, 4), 100, np.uint8)
    H = np.eye(3, dtype=F32).reshape(9)
    out = np.full(7, 77, np.uint64)
    tab = lambda k: (C.c_void_p * max(k, 1))(*([A.ctypes.data] * k))

    def call(n=2, L=1, frames=None, la=(0,), lb=(1,), fw=fw, fh=fh, H=H.ctypes.data, stride=1, lo=5, hi=250, sums=out.ctypes.data):
        return lib.nm_mosaic_exposure_sums_host(n, L, tab(min(max(n, 0), 64)) if frames is None else frames or None,
                                                _ints(la) if la is not None else None, _ints(lb) if lb is not None else None,
                                                fw, fh, None, H, None, stride, lo, hi, sums)
    assert call() == 0 and out[0] == (fw - 1) * (fh - 1)           # the identity: the last column and row lack taps
    out[:] = 77
    hole = (C.c_void_p * 2)(A.ctypes.data, None)
    for kw in (dict(n=0), dict(n=65), dict(L=0), dict(L=257, la=(0,) * 257, lb=(1,) * 257), dict(fw=0), dict(fw=32768),
               dict(fh=0), dict(fh=32768), dict(stride=0), dict(stride=65), dict(lo=-1), dict(lo=200, hi=100), dict(hi=256),
               dict(frames=hole), dict(frames=0), dict(la=None), dict(lb=None), dict(H=None), dict(sums=None), dict(la=(2,)), dict(la=(-1,)),
               dict(lb=(2,)), dict(la=(1,)), dict(fw=32767, fh=32767)):     # the last: a lattice beyond 2^28
        assert call(**kw) == INVALID, kw
    assert (out == 77).all()


def test_gains_refusals(nm):
    lib = nm.lib()
    S = np.array([[100, 9000, 9000, 9000, 9900, 9900, 9900]], np.uint64)
    g, st = np.full((2, 3), 7, F32), np.full(9, 7.0)

    def call(n=2, L=1, la=(0,), lb=(1,), sums=S.ctypes.data, min_pixels=64, sn=10.0, sg=0.1, g_min=0.5, g_max=2.0, mode=0,
             gains=g.ctypes.data, stats=st.ctypes.data):
        return lib.nm_mosaic_gains_host(n, L, _ints(la) if la is not None else None, _ints(lb) if lb is not None else None, sums,
                                        None, min_pixels, sn, sg, g_min, g_max, mode, gains, stats)
    assert call() == 0 and st[8] == X.END_OK
    g[:], st[:] = 7, 7
    nan, inf = float("nan"), float("inf")
    for kw in (dict(n=0), dict(n=65), dict(L=0), dict(L=257, la=(0,) * 257, lb=(1,) * 257), dict(la=None), dict(lb=None),
               dict(sums=None), dict(gains=None), dict(stats=None), dict(la=(2,)), dict(lb=(-1,)), dict(la=(1,)),
               dict(min_pixels=0), dict(sn=0.0), dict(sn=nan), dict(sn=1e-7), dict(sn=1e7), dict(sg=0.0), dict(sg=nan),
               dict(sg=inf), dict(g_min=0.0), dict(g_min=-1.0), dict(g_min=1.5), dict(g_min=nan), dict(g_max=0.99),
               dict(g_max=inf), dict(g_max=nan), dict(mode=2), dict(mode=-1)):
        assert call(**kw) == INVALID, kw
    assert (g == 7).all() and (st == 7).all()


def test_wrappers_refuse_before_the_library(nm):
    A = np.full((8, 16, 4), 100, np.uint8)
    H = np.eye(3, dtype=F32)
    for kw in (dict(stride=0), dict(lo=9, hi=3), dict(hi=256)):
        with pytest.raises(nm.NmError):
            nm.mosaic_exposure_sums_host([A, A], [0], [1], H, **kw)
    with pytest.raises(nm.NmError):
        nm.mosaic_exposure_sums_host([A, A], [0], [0], H)
    S = np.zeros((1, 7), np.uint64)
    for kw in (dict(sigma_n=0.0), dict(g_min=2.0), dict(mode=3), dict(min_pixels=0)):
        with pytest.raises(nm.NmError):
            nm.mosaic_gains_host(2, [0], [1], S, **kw)
