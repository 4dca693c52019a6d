"""The median mosaic composite on the host: nm_mosaic_median_host (the functions the device kernel is compiled from) against
the numpy model of tests/median_ref.py (SELECT exactly, MEAN within the bound derived there), at every stack depth, on the
edge cases of keys, weights and tau, on rectangles at and off the canvas edges, its exact properties, the model's mutants,
every refusal and the constants. No GPU: the tiles are synthesised in numpy."""
import re

import numpy as np
import pytest

import bands_ref as B
import median_ref as M
import mosaic_edges_ref as E

F32 = np.float32
INVALID = 1      # hipErrorInvalidValue
MODES = (M.SELECT, M.MEAN)
INF = float("inf")


def check_against_model(nm, tiles, recs, cap, cw, ch, mode, w_min=0.0, tau=INF, share_cap=0.01):
    got = M.run_host(nm, tiles, recs, cap, cw, ch, mode, w_min=w_min, tau=tau)
    md = M.model(tiles, recs, cw, ch, cap, mode, w_min=w_min, tau=tau)
    M.check_exact(got, md, cw, ch, mode)
    if mode == M.MEAN:
        worst, bad, share, w_bad = M.compare_mean(got[0][..., :3], got[1], md)
        print("worst level difference %d, unexcused %d, share within the bound of an integer %.4f %%, weights off %d"
              % (worst, bad, 100 * share, w_bad))
        assert bad == 0 and worst <= 1 and w_bad == 0
        assert share < share_cap                      # the model alone: the seeds keep it under the cap
    return got, md


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", M.DEPTHS)
def test_host_twin_against_the_model_at_every_stack_depth(nm, n, mode):
    tiles, recs, cap, cw, ch = M.stack_case(n)
    tau = INF if mode == M.SELECT else 0.15
    _, md = check_against_model(nm, tiles, recs, cap, cw, ch, mode, tau=tau)
    assert (md["m"] == n).sum() >= 8 * M.STACK_H and (md["m"] == 0).any()
    if n >= 16:
        assert len(np.unique(md["m"])) > 4 and (md["support"][md["m"] > 0] < md["m"][md["m"] > 0]).any() == (mode == M.MEAN)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", (1, 2, 3, 17))
def test_host_twin_against_the_model_on_scattered_frames(nm, n, mode):
    """the cases of the two-band tests: an unplaced record, a frame over tile_cap, one off the canvas, a tiny one"""
    tiles, recs, cap, cw, ch = B.case(n)
    _, md = check_against_model(nm, tiles, recs, cap, cw, ch, mode, w_min=0.75, tau=0.1)
    assert (md["m"] > 0).sum() > 1000 and (n < 3 or md["m"].max() >= 3)


@pytest.mark.parametrize("mode", MODES)
def test_rectangles_at_off_and_beyond_every_canvas_side(nm, mode):
    tiles, recs, cap, cw, ch = M.edge_scene()
    _, md = check_against_model(nm, tiles, recs, cap, cw, ch, mode, tau=0.2)
    assert len(recs) == 23
    for k in (19, 20, 21, 22):                          # beyond the right side, above the top, unplaced, over tile_cap
        assert md["counts"][k, 0] == 0
    assert (md["counts"][:19, 0] > 0).all() and md["valid"][11, 60, 230]


grey = E.grey


def test_equal_keys_and_signed_zeros_fall_to_the_index(nm):
    """the stacks of mosaic_edges_ref.median_equal_greys, which the GPU edge test runs too"""
    tiles, recs, cap, cw, ch = E.median_equal_greys(0)                  # four equal keys: rank 1 is frame 1
    got, md = check_against_model(nm, tiles, recs, cap, cw, ch, M.SELECT)
    assert len(tiles) == 4 and (got[3][1:5, 1:10] == 1).all() and (got[1][1:5, 1:10] == 2.0).all()
    tiles, recs, cap, cw, ch = E.median_equal_greys(1)                  # -0 == +0: rank 1 is frame 1, not a -0 frame
    got, md = check_against_model(nm, tiles, recs, cap, cw, ch, M.SELECT)
    assert len(tiles) == 3 and np.signbit(md["key"][0, 2, 2]) and not np.signbit(md["key"][1, 2, 2])
    assert np.signbit(md["key"][2, 2, 2]) and (got[3][1:5, 1:10] == 1).all() and (got[1][1:5, 1:10] == 4.0).all()
    tiles, recs, cap, cw, ch = E.median_equal_greys(2)
    got, md = check_against_model(nm, tiles, recs, cap, cw, ch, M.SELECT)
    assert len(tiles) == 5 and (md["key"][:, 2, 2] == np.array([0, 0, md["key"][2, 2, 2], 0, 0], F32)).all()
    assert (got[3][1:5, 1:10] == 3).all()                               # order 0, 1, 3, 4, 2: rank 2 is frame 3
    for q, (label, weight) in enumerate(E.EQUAL_GREYS_WANT):
        got = M.run_host(nm, *E.median_equal_greys(q), M.SELECT)
        assert (got[3][1:5, 1:10] == label).all() and (got[1][1:5, 1:10] == weight).all()


@pytest.mark.parametrize("mode", MODES)
def test_invalid_samples_nan_inf_and_the_weight_limits(nm, mode):
    tiles, recs, cap, cw, ch = E.median_limits_case()     # shared with the GPU edge test
    assert np.isnan(tiles[0][0, 0, 2]) and tiles[1][0, 1, 0] == np.inf and tiles[2][0, 2, 1] == -np.inf      # colours
    assert tiles[3][0, 3, 3] == F32(0.5) and tiles[4][0, 4, 3] == np.inf                # w == w_min exactly, w = inf: invalid
    assert tiles[4][0, 5, 3] == F32(M.FLT_MAX) and np.isnan(tiles[5][0, 6, 3])          # w = FLT_MAX: valid; w NaN
    assert tiles[5][0, 7, 3] == np.nextafter(F32(0.5), F32(1)) and (cw, ch) == (9, 4)   # the float after w_min: valid
    got, md = check_against_model(nm, tiles, recs, cap, 9, 4, mode, w_min=E.LIMITS_W_MIN,
                                  tau=INF if mode == M.SELECT else 0.25)
    assert md["m"][0].tolist() == [5, 5, 5, 5, 5, 6, 5, 6, 6]
    assert md["m"][1:].min() == 6
    for k, x in enumerate((0, 1, 2, 3, 4)):
        assert not md["valid"][k, 0, x]


def test_tau_zero_infinite_and_equal_to_a_key_difference(nm):
    tiles, recs, cap = E.median_tau_case()[:3]            # shared with the GPU edge test, as are the taus
    assert E.TAU_LEVELS == (0.1, 0.3, 0.45, 0.7, 0.95) and E.median_tau_case()[3:] == (14, 6) and E.LIMITS_W_MIN == 0.5
    ys = [M.key(t[0, 0, :3]) for t in tiles]
    for mode in MODES:
        got, md = check_against_model(nm, tiles, recs, cap, 14, 6, mode, tau=0.0)
        assert (got[2][1:5, 2:11] == 1).all() and md["counts"][:, 1].tolist() == [36, 36, 0, 36, 36]
        got, md = check_against_model(nm, tiles, recs, cap, 14, 6, mode, tau=INF)
        assert (got[2][1:5, 2:11] == 5).all() and not md["counts"][:, 1].any()
        exact = float(np.abs(F32(ys[3] - ys[2])))                      # the fp32 difference itself: <= keeps frame 3
        assert E.tau_values()["exact"] == exact and E.tau_values()["below"] == float(np.nextafter(F32(exact), F32(0)))
        got, md = check_against_model(nm, tiles, recs, cap, 14, 6, mode, tau=exact)
        assert (got[2][1:5, 2:11] == 3).all() and md["counts"][:, 1].tolist() == [36, 0, 0, 0, 36]
        below = float(np.nextafter(F32(exact), F32(0)))
        got, md = check_against_model(nm, tiles, recs, cap, 14, 6, mode, tau=below)
        assert (got[2][1:5, 2:11] == 2).all()


def test_optional_outputs_may_be_absent(nm):
    tiles, recs, cap, cw, ch = M.stack_case(5)
    full = M.run_host(nm, tiles, recs, cap, cw, ch, M.MEAN, tau=0.15)
    canvas, cwts = B.pattern(cw, ch)
    nm.mosaic_median_host(canvas, None, B.pack(tiles, cap), B.records(recs), mode=M.MEAN, tau=0.15)
    assert np.array_equal(canvas, full[0])


# ---- exact properties ------------------------------------------------------------------------------------------------------
def test_single_coverage_is_the_frames_own_sample_and_equals_winner_take_all(nm):
    rng = np.random.default_rng(3)
    for recs in ([(5, 4, 67, 45, 1)], [(0, 0, 40, 30, 1), (40, 0, 40, 30, 1), (0, 30, 33, 20, 1), (50, 40, 30, 25, 1)],
                 [(0, 0, 60, 40, 1), (30, 20, 60, 40, 1)]):
        tiles = [B.texture(rng, r[2], r[3]) for r in recs]
        cap = max(r[2] * r[3] for r in recs)
        for mode in MODES:
            got = M.run_host(nm, tiles, recs, cap, 90, 70, mode, tau=0.0)
            md = M.model(tiles, recs, 90, 70, cap, mode, tau=0.0)
            single = md["m"] == 1
            assert single.sum() >= 2000
            bands_c, bands_w = B.run_host(nm, tiles, recs, cap, 90, 70, 0)
            if mode == M.SELECT:                        # bit for bit nm_mosaic_bands_host at R = 0 on the same tiles
                assert np.array_equal(got[0][single], bands_c[single]) and np.array_equal(got[1][single], bands_w[single])
                if len(recs) == 1:
                    assert np.array_equal(got[0], bands_c) and np.array_equal(got[1], bands_w)


def test_select_writes_some_valid_frames_own_sample_everywhere(nm):
    tiles, recs, cap, cw, ch = B.case(17)
    canvas, cwts, support, label, _ = M.run_host(nm, tiles, recs, cap, cw, ch, M.SELECT)
    T, cover = M.stacks(tiles, recs, cw, ch, cap)
    on = M.model(tiles, recs, cw, ch, cap)["m"] > 0
    lab = np.where(on, label, 0).astype(np.int64)
    mine = np.take_along_axis(T, lab[None, ..., None], 0)[0]
    own = np.take_along_axis(cover, lab[None], 0)[0]
    assert own[on].all() and (mine[..., 3][on] > 0).all()
    assert np.array_equal(canvas[..., :3][on], B.store_f32(mine[..., :3])[on]) and np.array_equal(cwts[on], mine[..., 3][on])


@pytest.mark.parametrize("colour", [(1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)])
@pytest.mark.parametrize("m", (5, 6, 7))
def test_select_removes_an_occluder_present_in_fewer_than_half_of_the_frames(nm, m, colour):
    rng = np.random.default_rng(40 + m)
    base = B.texture(rng, 67, 45, holes=False)
    base[..., :3] = 0.3 + 0.5 * base[..., :3]            # keys strictly between the saturated colours'
    clean = []
    for k in range(m):
        t = base.copy()
        t[..., 3] = rng.uniform(0.5, 2.0, t.shape[:2]).astype(F32)
        clean.append(t)
    recs, cap = [(4, 3, 67, 45, 1)] * m, 67 * 45
    want = M.run_host(nm, clean, recs, cap, 80, 55, M.SELECT)[0]
    limit = (m + 1) // 2 - 1                             # ceil(m / 2) - 1
    occluded = [t.copy() for t in clean]
    order = rng.permutation(m)
    for q in range(1, m + 1):                            # block q: columns 8 q .., in q of the frames
        for k in order[:q]:
            occluded[k][5:30, 8 * q:8 * q + 6, :3] = colour
    got = M.run_host(nm, occluded, recs, cap, 80, 55, M.SELECT)[0]
    for q in range(1, m + 1):
        block = (slice(3 + 5, 3 + 30), slice(4 + 8 * q, 4 + 8 * q + 6))
        if q <= limit:
            assert np.array_equal(got[block], want[block]), q
        elif q > m // 2:                                 # more than half of the frames: the occluder is the median
            assert (got[block][..., :3] == B.store_f32(np.array(colour, F32))).all(), q
    outside = np.ones((55, 80), bool)
    outside[8:33, 12:4 + 8 * m + 6] = False
    assert np.array_equal(got[outside], want[outside])


def test_mean_with_infinite_tau_is_the_plain_weighted_mean(nm):
    tiles, recs, cap, cw, ch = B.case(17)
    got = M.run_host(nm, tiles, recs, cap, cw, ch, M.MEAN, tau=INF)
    md = M.model(tiles, recs, cw, ch, cap, M.MEAN, tau=INF)
    assert np.array_equal(md["support"], md["m"]) and not md["counts"][:, 1].any()
    plain = dict(md, out=np.where((md["m"] > 0)[..., None], B.feather_f64(tiles, recs, cw, ch, cap), np.nan))
    assert np.allclose(np.nan_to_num(plain["out"]), np.nan_to_num(md["out"]), rtol=1e-12, atol=0)
    worst, bad, share, w_bad = M.compare_mean(got[0][..., :3], got[1], plain)
    assert bad == 0 and worst <= 1 and w_bad == 0 and share < 0.01


# ---- mutants of the model, each rejected by a check above ------------------------------------------------------------------
@pytest.mark.parametrize("mutant", ("upper", "high_tie", "strict"))
def test_the_checks_reject_mutants_of_the_model(nm, mutant):
    if mutant == "upper":
        tiles, recs, cap, cw, ch = M.stack_case(4)
        mode, tau = M.SELECT, INF
    elif mutant == "high_tie":
        tiles, recs, cap, cw, ch = [grey(0.5, 1.0 + k) for k in range(4)], [(1, 1, 9, 4, 1)] * 4, 36, 12, 6
        mode, tau = M.SELECT, INF
    else:
        tiles = [grey(v, 1.0 + k) for k, v in enumerate((0.1, 0.3, 0.45, 0.7, 0.95))]
        recs, cap, cw, ch, mode = [(2, 1, 9, 4, 1)] * 5, 36, 14, 6, M.MEAN
        tau = float(np.abs(F32(M.key(tiles[3][0, 0, :3]) - M.key(tiles[2][0, 0, :3]))))
    got = M.run_host(nm, tiles, recs, cap, cw, ch, mode, tau=tau)
    M.check_exact(got, M.model(tiles, recs, cw, ch, cap, mode, tau=tau), cw, ch, mode)
    with pytest.raises(AssertionError):
        M.check_exact(got, M.model(tiles, recs, cw, ch, cap, mode, tau=tau, **{mutant: True}), cw, ch, mode)


# ---- the end-to-end figures on the CPU ---------------------------------------------------------------------------------------
def test_the_model_shows_both_robust_composites_closer_to_the_clean_mosaic(nm):
    """Ten loop-closure views, a saturated block painted into each: mean absolute byte difference to the clean-frames feather
    canvas over the pixels with m >= 3 at which an occluded sample is valid. tests/test_gpu_mosaic_median.py asserts the same
    ordering of the device's canvases. The figures are in DESIGN.md section 7, "Median composite"."""
    fig, sel = M.e2e_model(nm, 91, nm.MEDIAN_TAU)[:2]
    print("mean absolute byte difference to the clean feather canvas over %d pixels, tau %.3f: feather with occluders %.3f, "
          "SELECT %.3f, MEAN %.3f" % (sel.sum(), nm.MEDIAN_TAU, fig["feather"], fig["select"], fig["mean"]))
    assert sel.sum() > 5000
    assert fig["select"] < fig["feather"] and fig["mean"] < fig["feather"]


# ---- refusals and constants ----------------------------------------------------------------------------------------------------
def _aligned(nbytes):
    raw = np.zeros(nbytes + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw, off


def test_every_refusal_of_the_median_entries(nm):
    lib = nm.lib()
    tiles, recs, cap, cw, ch = M.stack_case(3)
    n = len(recs)
    packed, rec = B.pack(tiles, cap), B.records(recs)
    traw, toff = _aligned(packed.nbytes)
    traw[toff:toff + packed.nbytes] = packed.reshape(-1).view(np.uint8)
    canvas, cwts, support, label, counts = M.outputs(cw, ch, n)
    good = dict(n=n, tiles=traw.ctypes.data + toff, cap=cap, rec=rec.ctypes.data, canvas=canvas.ctypes.data, cw=cw, ch=ch,
                wts=cwts.ctypes.data, mode=0, w_min=0.0, tau=0.1, support=support.ctypes.data, label=label.ctypes.data,
                counts=counts.ctypes.data)

    def call(fn, *tail, **kw):
        a = dict(good, **kw)
        return fn(a["n"], a["tiles"], a["cap"], a["rec"], a["canvas"], a["cw"], a["ch"], a["wts"], a["mode"], a["w_min"], a["tau"],
                  a["support"], a["label"], a["counts"], *tail)

    nan = float("nan")
    refused = [dict(n=0), dict(n=65), dict(cap=0), dict(cap=(1 << 30) + 1), dict(cw=0), dict(cw=32768), dict(ch=0),
               dict(ch=32768), dict(mode=-1), dict(mode=2), dict(w_min=-1e-30), dict(w_min=INF), dict(w_min=nan),
               dict(tau=-1e-30), dict(tau=nan), dict(tau=-INF), dict(tiles=None), dict(rec=None), dict(canvas=None),
               dict(tiles=good["tiles"] + 8)]
    for kw in refused:
        assert call(lib.nm_mosaic_median_host, **kw) == INVALID, kw
        # the device entry refuses the same arguments before it touches anything (no GPU is needed to be refused)
        assert call(lib.nm_mosaic_median_dev, None, **kw) == INVALID, kw
    want = M.outputs(cw, ch, n)
    for a, b in zip((canvas, cwts, support, label, counts), want):
        assert np.array_equal(a, b)
    assert call(lib.nm_mosaic_median_host, tau=INF) == 0 and call(lib.nm_mosaic_median_host, tau=0.0, w_min=0.0) == 0
    assert call(lib.nm_mosaic_median_host, wts=None, support=None, label=None, counts=None, mode=1) == 0
    for kw in (dict(mode=2), dict(w_min=-1.0), dict(tau=nan), dict(tau=-1.0)):
        with pytest.raises(nm.NmError):
            nm.mosaic_median_host(canvas, cwts, packed, rec, **kw)


def test_header_constants_match_the_binding(nm):
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nm_abi.h")).read()
    value = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert value("NM_MEDIAN_SELECT") == nm.MEDIAN_SELECT == M.SELECT and value("NM_MEDIAN_MEAN") == nm.MEDIAN_MEAN == M.MEAN
    assert value("NM_MOSAIC_MAX_BATCH") == nm.MOSAIC_MAX_BATCH == max(M.DEPTHS)
    for name in ("nm_mosaic_median_dev", "nm_mosaic_median_host"):
        assert name in nm.ABI_SYMBOLS and hasattr(nm.lib(), name)
    assert 0.0 < nm.MEDIAN_TAU < 1.0
