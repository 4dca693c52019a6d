"""The two-band mosaic blend on the host: nm_mosaic_bands_host (the functions the device kernels are compiled from) against
the float64 model of tests/bands_ref.py within the bound derived there, its exact properties, the model's mutants, every
refusal, and the workspace size. No GPU: the input tiles are synthesised in numpy (random textures, so that few byte values
sit within the bound of an integer; the share is printed and capped at 1 %)."""
import ctypes as C

import numpy as np
import pytest

import bands_ref as B
import mosaic_edges_ref as E

F32 = np.float32
NS, RS = (1, 2, 3, 17, 64), (0, 1, 2, 7, 32)
INVALID = 1      # hipErrorInvalidValue
pattern, run_host, sigma_of, case = B.pattern, B.run_host, B.sigma_of, B.case


def check_untouched(canvas, cwts, md):
    want_c, want_w = pattern(canvas.shape[1], canvas.shape[0])
    off = md["label"] == B.NONE
    assert np.array_equal(canvas[off], want_c[off]) and np.array_equal(cwts[off], want_w[off])


def test_taps_are_the_written_gaussian(nm):
    for R in RS + (16,):
        for sigma in (0.3, sigma_of(R), 40.0):
            g = nm.mosaic_bands_taps(R, sigma)
            want = B.taps(R, sigma)
            assert g.shape == want.shape and (np.abs(g - want) <= np.spacing(want)).all()      # libm's exp against numpy's
            assert abs(float(g[0]) + 2.0 * float(g[1:].astype(np.float64).sum()) - 1.0) < (R + 2) * 2.0 ** -24
    assert nm.mosaic_bands_taps(0, float("nan"))[0] == 1.0


@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("n", NS)
def test_host_twin_against_the_float64_model(nm, n, R):
    tiles, recs, cap, cw, ch = case(n)
    canvas, cwts = run_host(nm, tiles, recs, cap, cw, ch, R)
    md = B.model(tiles, recs, nm.mosaic_bands_taps(R, sigma_of(R)), cw, ch, cap)
    lab = md["label"] != B.NONE
    assert lab.sum() > 1000 and (n < 2 or (md["M_frames"] > 1).any() or R == 0)
    worst, bad, share = B.compare(canvas[..., :3], md, R)
    print("n=%d R=%d: labelled %d, worst level difference %d, unexcused %d, share within the bound of an integer %.4f %%"
          % (n, R, lab.sum(), worst, bad, 100 * share))
    assert bad == 0 and worst <= 1
    assert share < 0.01
    assert (canvas[..., 3][lab] == 255).all()
    assert np.array_equal(cwts[lab], md["wstar"][lab])
    check_untouched(canvas, cwts, md)


def test_canvas_weights_are_optional(nm):
    tiles, recs, cap, cw, ch = case(3)
    a, _ = run_host(nm, tiles, recs, cap, cw, ch, 7)
    b, wts = run_host(nm, tiles, recs, cap, cw, ch, 7, with_wts=False)
    assert np.array_equal(a, b) and np.array_equal(wts, pattern(cw, ch)[1])


@pytest.mark.parametrize("R", (1, 7, 32))
def test_single_and_disjoint_frames_give_their_own_samples(nm, R):
    rng = np.random.default_rng(3)
    for recs in ([(5, 4, 67, 45, 1)], [(0, 0, 40, 30, 1), (40, 0, 40, 30, 1), (0, 30, 33, 20, 1), (50, 40, 30, 25, 1)]):
        tiles = [B.texture(rng, r[2], r[3]) for r in recs]
        cap = max(r[2] * r[3] for r in recs)
        canvas, cwts = run_host(nm, tiles, recs, cap, 90, 70, R)
        want, wstar, label = B.winner(tiles, recs, 90, 70, cap)
        lab = label != B.NONE
        assert lab.sum() >= 67 * 45 * 0.9
        assert np.array_equal(canvas[..., :3][lab], want[lab]) and np.array_equal(cwts[lab], wstar[lab])


@pytest.mark.parametrize("n", (3, 17))
def test_radius_zero_is_winner_take_all(nm, n):
    tiles, recs, cap, cw, ch = case(n)
    canvas, cwts = run_host(nm, tiles, recs, cap, cw, ch, 0, sigma=float("nan"))
    want, wstar, label = B.winner(tiles, recs, cw, ch, cap)
    lab = label != B.NONE
    assert np.array_equal(canvas[..., :3][lab], want[lab]) and np.array_equal(cwts[lab], wstar[lab])


@pytest.mark.parametrize("R", (2, 32))
def test_equal_colours_under_different_weights_give_the_colour(nm, R):
    rng = np.random.default_rng(11)
    # (a) the same rectangle and texture three times, three weight planes: every l_k is the same number
    base = B.texture(rng, 67, 45, holes=False)
    tiles = []
    for k in range(3):
        t = base.copy()
        t[..., 3] = rng.uniform(0.1, 3.0, t.shape[:2]).astype(F32)
        tiles.append(t)
    recs = [(3, 2, 67, 45, 1)] * 3
    canvas, _ = run_host(nm, tiles, recs, 67 * 45, 80, 60, R)
    assert np.array_equal(canvas[2:47, 3:70, :3], B.store_f32(base[..., :3]))
    # (b) different rectangles, one constant colour of powers of two: scaling by 2^-k commutes with every rounding
    col = np.array([0.5, 0.25, 0.125], F32)
    recs = [(0, 0, 67, 45, 1), (30, 10, 67, 45, 1), (10, 25, 50, 33, 1)]
    tiles = []
    for r in recs:
        t = B.texture(rng, r[2], r[3], holes=True)
        t[..., :3] = np.where(t[..., 3:] > 0, col, 0)
        tiles.append(t)
    canvas, _ = run_host(nm, tiles, recs, 67 * 45, 100, 60, R)
    label, _ = B.labels(tiles, recs, 100, 60, 67 * 45)
    assert (canvas[..., :3][label != B.NONE] == B.store_f32(col)).all()


@pytest.mark.parametrize("R", (1, 7))
def test_pixels_far_from_every_label_change_equal_the_winner(nm, R):
    tiles, recs, cap, cw, ch = case(17)
    canvas, _ = run_host(nm, tiles, recs, cap, cw, ch, R)
    want, _, label = B.winner(tiles, recs, cw, ch, cap)
    # independent of the model's M: a labelled pixel none of whose (2R+1)^2 neighbours on the canvas carries another label
    lab = label != B.NONE
    pad = np.pad(label, R, mode="edge")
    same = np.ones(label.shape, bool)
    for dy in range(2 * R + 1):
        for dx in range(2 * R + 1):
            nb = pad[dy:dy + ch, dx:dx + cw]
            same &= (nb == label) | (nb == B.NONE)
    far = lab & same
    assert far.sum() > 500 and (lab & ~same).sum() > 500
    assert np.array_equal(canvas[..., :3][far], want[far])
    assert not np.array_equal(canvas[..., :3][lab & ~same], want[lab & ~same])


def tie_case():
    """two frames on one rectangle, every weight equal: mosaic_edges_ref.bands_tie_case, which the GPU edge test runs too"""
    return E.bands_tie_case()[:3]


def test_tied_weights_label_the_lower_index(nm):
    tiles, recs, cap = tie_case()
    canvas, _ = run_host(nm, tiles, recs, cap, 50, 40, 0)
    assert np.array_equal(canvas[2:32, 2:42, :3], B.store_f32(tiles[0][..., :3]))
    canvas, _ = run_host(nm, tiles, recs, cap, 50, 40, 7)
    assert np.array_equal(canvas[2:32, 2:42, :3], B.store_f32(tiles[0][..., :3]))


@pytest.mark.parametrize("R", (1, 7, 32))
def test_straight_seam_profile(nm, R):
    nw, nh, s = 131, 97, 60                     # labels: frame 0 for x <= s, frame 1 beyond
    x = np.arange(nw, dtype=F32)[None, :].repeat(nh, 0)
    t0, t1 = np.zeros((nh, nw, 4), F32), np.zeros((nh, nw, 4), F32)
    t0[..., :3], t1[..., :3] = F32(0.2), F32(0.8)
    t0[..., 3], t1[..., 3] = 2 * (s + 1) - x, x + 1        # equal at x = s + 0.5
    tiles, recs = [t0, t1], [(0, 0, nw, nh, 1)] * 2
    canvas, _ = run_host(nm, tiles, recs, nw * nh, nw, nh, R)
    md = B.model(tiles, recs, nm.mosaic_bands_taps(R, sigma_of(R)), nw, nh, nw * nh)
    assert (md["label"][:, :s + 1] == 0).all() and (md["label"][:, s + 1:] == 1).all()
    assert B.compare(canvas[..., :3], md, R)[:2] in ((0, 0), (1, 0))
    lo, hi = B.store_f32(F32(0.2)), B.store_f32(F32(0.8))
    for row in (0, nh // 2, nh - 1):
        p = canvas[row, :, 1].astype(int)
        assert (np.diff(p) >= 0).all()
        assert (p[:s - R + 1] == lo).all() and (p[s + R + 1:] == hi).all()
        mixed = np.flatnonzero((p > lo) & (p < hi))
        # 2R mixed pixels, 2R + 1 steps from lo to hi. At R = 32 (sigma 16) the outermost taps move the value by less than
        # a byte level, so the bytes are held inside the span and the exact span is asserted on the model's profile, which
        # the bytes match within the bound (above)
        assert mixed.min() >= s - R + 1 and mixed.max() <= s + R and mixed.size > R
        if R <= 7:
            assert mixed.min() == s - R + 1 and mixed.max() == s + R and mixed.size == 2 * R
            assert (np.diff(p[s - R:s + R + 2]) > 0).all()
        q = md["out"][row, :, 1]
        assert (q[:s - R + 1] == float(F32(0.2))).all() and (q[s + R + 1:] == float(F32(0.8))).all()
        assert (np.diff(q[s - R:s + R + 2]) > 0).all()               # 2R + 1 strictly rising steps, none outside them


def test_the_model_shows_the_sharpness_ordering_on_the_loop_closure_views(nm):
    """The end-to-end figures on the CPU (host twins for sums, gains and placement, float64 model for tiles and composites):
    the mean squared Laplacian of the bands mosaic lies closer to the winning frame's than the feather mosaic's does, at
    the corner perturbation B.E2E_PERTURB_PX. tests/test_gpu_mosaic_bands.py asserts the same of the device's canvases."""
    fig = B.e2e_model(nm, 91)[0]
    print("mean squared Laplacian (byte levels^2) at %.1f px: bands %.3f, feather %.3f, winning frame alone %.3f"
          % (B.E2E_PERTURB_PX, fig["bands"], fig["feather"], fig["single"]))
    assert abs(fig["bands"] - fig["single"]) < abs(fig["feather"] - fig["single"])


@pytest.mark.parametrize("mutant", ("no_v", "m_from_w", "last_tie"))
def test_the_checks_reject_mutants_of_the_model(nm, mutant):
    R = 7
    if mutant == "last_tie":
        tiles, recs, cap = tie_case()
        cw, ch = 50, 40
    else:
        tiles, recs, cap, cw, ch = case(3)
    canvas, _ = run_host(nm, tiles, recs, cap, cw, ch, R)
    g = nm.mosaic_bands_taps(R, sigma_of(R))
    assert B.compare(canvas[..., :3], B.model(tiles, recs, g, cw, ch, cap), R)[1] == 0
    worst, bad, _ = B.compare(canvas[..., :3], B.model(tiles, recs, g, cw, ch, cap, **{mutant: True}), R)
    print(mutant, "worst", worst, "unexcused", bad)
    assert bad > 100


def _aligned(nbytes, guard=256, value=0xA5):
    raw = np.full(nbytes + 2 * guard + 16, value, np.uint8)
    off = (-(raw.ctypes.data + guard)) % 16 + guard
    return raw, off


def test_workspace_bytes_cover_what_is_touched(nm):
    lib = nm.lib()
    tiles, recs, cap, cw, ch = case(17)
    n = len(recs)
    need = lib.nm_mosaic_bands_workspace_bytes(n, cap, cw, ch)
    assert need == ((cw * ch + 255) // 256) * 256 + n * cap * 40
    packed, rec = B.pack(tiles, cap), B.records(recs)
    traw, toff = _aligned(packed.nbytes)
    traw[toff:toff + packed.nbytes] = packed.reshape(-1).view(np.uint8)
    results = []
    for value in (0xA5, 0x00):
        raw, off = _aligned(need, value=value)
        canvas, cwts = pattern(cw, ch)
        assert lib.nm_mosaic_bands_host(n, traw.ctypes.data + toff, cap, rec.ctypes.data, canvas.ctypes.data, cw, ch,
                                        cwts.ctypes.data, 7, 3.5, raw.ctypes.data + off) == 0
        assert (raw[:off] == value).all() and (raw[off + need:] == value).all()
        touched = np.flatnonzero(raw[off:off + need] != value)
        assert touched.size > cw * ch // 4 and touched.max() < need
        results.append((canvas, cwts))
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    assert (traw[:toff] == 0xA5).all() and (traw[toff + packed.nbytes:] == 0xA5).all()
    for bad in ((0, cap, cw, ch), (65, cap, cw, ch), (n, 0, cw, ch), (n, (1 << 30) + 1, cw, ch), (n, cap, 0, ch),
                (n, cap, 32768, ch), (n, cap, cw, 0), (n, cap, cw, 32768)):
        assert lib.nm_mosaic_bands_workspace_bytes(*bad) == 0


def test_every_refusal_of_the_bands_entry(nm):
    lib = nm.lib()
    tiles, recs, cap, cw, ch = case(3)
    n = len(recs)
    packed, rec = B.pack(tiles, cap), B.records(recs)
    traw, toff = _aligned(packed.nbytes)
    traw[toff:toff + packed.nbytes] = packed.reshape(-1).view(np.uint8)
    need = lib.nm_mosaic_bands_workspace_bytes(n, cap, cw, ch)
    raw, off = _aligned(need)
    canvas, cwts = pattern(cw, ch)
    good = dict(n=n, tiles=traw.ctypes.data + toff, cap=cap, rec=rec.ctypes.data, canvas=canvas.ctypes.data, cw=cw, ch=ch,
                wts=cwts.ctypes.data, R=7, sigma=3.5, ws=raw.ctypes.data + off)

    def call(**kw):
        a = dict(good, **kw)
        return lib.nm_mosaic_bands_host(a["n"], a["tiles"], a["cap"], a["rec"], a["canvas"], a["cw"], a["ch"], a["wts"],
                                        a["R"], a["sigma"], a["ws"])

    refused = [dict(n=0), dict(n=65), dict(cap=0), dict(cap=(1 << 30) + 1), dict(cw=0), dict(cw=32768), dict(ch=0),
               dict(ch=32768), dict(R=-1), dict(R=33), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")),
               dict(sigma=float("inf")), dict(tiles=None), dict(rec=None), dict(canvas=None), dict(ws=None),
               dict(ws=good["ws"] + 4), dict(tiles=good["tiles"] + 8)]
    for kw in refused:
        assert call(**kw) == INVALID, kw
        # the device entry refuses the same arguments before it touches anything (no GPU is needed to be refused)
        a = dict(good, **kw)
        assert lib.nm_mosaic_bands_dev(a["n"], a["tiles"], a["cap"], a["rec"], a["canvas"], a["cw"], a["ch"], a["wts"],
                                       a["R"], a["sigma"], a["ws"], None) == INVALID, kw
    want_c, want_w = pattern(cw, ch)
    assert np.array_equal(canvas, want_c) and np.array_equal(cwts, want_w) and (raw == 0xA5).all()
    assert call(R=0, sigma=float("nan")) == 0 and call(wts=None) == 0 and call() == 0
    g = (C.c_float * 40)()
    for R, sigma in ((-1, 1.0), (33, 1.0), (3, 0.0), (3, float("nan")), (3, float("inf"))):
        assert lib.nm_mosaic_bands_taps(R, sigma, g) == INVALID
    assert lib.nm_mosaic_bands_taps(3, 1.0, None) == INVALID


def test_every_refusal_of_the_warp_tiles_entry(nm):
    """Refused on the host before any device memory is touched: the pointers below are never dereferenced."""
    lib = nm.lib()
    n = 3
    dummy = 4096
    table = (C.c_void_p * n)(*([dummy] * n))
    holed = (C.c_void_p * n)(dummy, None, dummy)
    good = dict(n=n, frames=table, fw=67, fh=45, masks=table, mf=0, wts=table, wf=2, rec=dummy, gains=None, tiles=dummy, cap=4000,
                stats=dummy)

    def call(**kw):
        a = dict(good, **kw)
        return lib.nm_mosaic_warp_tiles(a["n"], a["frames"], a["fw"], a["fh"], a["masks"], a["mf"], a["wts"], a["wf"], a["rec"],
                                        a["gains"], a["tiles"], a["cap"], a["stats"], None)

    for kw in (dict(n=0), dict(n=65), dict(fw=0), dict(fw=32768), dict(fh=0), dict(fh=32768), dict(mf=1), dict(mf=7), dict(wf=1),
               dict(wf=-1), dict(cap=0), dict(cap=(1 << 30) + 1), dict(frames=None), dict(masks=None), dict(wts=None),
               dict(frames=holed), dict(masks=holed), dict(wts=holed), dict(rec=None), dict(tiles=None), dict(stats=None),
               dict(tiles=dummy + 4)):
        assert call(**kw) == INVALID, kw
