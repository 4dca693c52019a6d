"""The edge inputs of tests/mosaic_edges_ref.py on the host: nm_mosaic_bands_host and nm_mosaic_median_host against the float64
models of bands_ref / median_ref, with their derived bounds unchanged. The GPU tests (test_gpu_mosaic_bands_edges.py,
test_gpu_mosaic_median_edges.py) compare the device with the host twins bit for bit on the same arrays, so this file keeps
their chain down to the models. No GPU. Each case is also checked to hold what its docstring promises (tile counts, ties at
the median, subnormal taps, both ends of the store's range), and the models' mutants turn the tie and tau cases red."""
import numpy as np
import pytest

import bands_ref as B
import median_ref as M
import mosaic_edges_ref as E

F32 = np.float32
MODES = (M.SELECT, M.MEAN)


def bands_against_model(nm, case, R, sigma=None, share_cap=0.01, **mutant):
    tiles, recs, cap, cw, ch = case
    sigma = B.sigma_of(R) if sigma is None else sigma
    canvas, cwts = B.run_host(nm, tiles, recs, cap, cw, ch, R, sigma=sigma)
    md = B.model(tiles, recs, nm.mosaic_bands_taps(R, sigma), cw, ch, cap, **mutant)
    worst, bad, share = B.compare(canvas[..., :3], md, R)
    print("R=%d sigma=%g: labelled %d, worst level difference %d, unexcused %d, share within the bound of an integer %.4f %%"
          % (R, sigma, (md["label"] != B.NONE).sum(), worst, bad, 100 * share))
    if mutant:
        return canvas, cwts, md, bad
    assert bad == 0 and worst <= 1
    assert share < share_cap
    lab = md["label"] != B.NONE
    assert (canvas[..., 3][lab] == 255).all() and np.array_equal(cwts[lab].view(np.uint32), md["wstar"][lab].view(np.uint32))
    pat_c, pat_w = B.pattern(cw, ch)
    assert np.array_equal(canvas[~lab], pat_c[~lab]) and np.array_equal(cwts[~lab], pat_w[~lab])
    return canvas, cwts, md, bad


def median_against_model(nm, case, mode, w_min, tau, **mutant):
    tiles, recs, cap, cw, ch = case
    got = M.run_host(nm, tiles, recs, cap, cw, ch, mode, w_min=w_min, tau=tau)
    md = E.median_model(tiles, recs, cw, ch, cap, mode, w_min=w_min, tau=tau, **mutant)
    M.check_exact(got, md, cw, ch, mode)
    if mode == M.MEAN:
        worst, bad, share, w_bad = M.compare_mean(got[0][..., :3], got[1], md)
        print("worst level difference %d, unexcused %d, share within the bound of an integer %.4f %%, weights off %d"
              % (worst, bad, 100 * share, w_bad))
        assert bad == 0 and worst <= 1 and w_bad == 0
        assert share < 0.01
    return got, md


# ---- A ----------------------------------------------------------------------------------------------------------------------
def test_the_multi_trip_cases_hold_two_trips_and_a_remainder_on_256_compute_units():
    tiles, recs, cap, cw, ch = E.multi_trip_case()
    counts = E.tile_counts(recs, cap, cw, ch)
    for loop in ("canvas", "row", "col", "median"):
        assert counts[loop] >= 2 * E.G_DESIGN + 1, (loop, counts)
    w = E.warp_trip_case()
    assert E.tile_counts([r[9:14] for r in w["recs"]], w["cap"], w["cw"], w["ch"])["warp"] >= 2 * E.G_DESIGN + 1
    assert len({(r[2], r[3]) for r in recs}) >= 10 and len({tuple(r[11:13]) for r in w["recs"]}) >= 10       # mixed sizes
    # between used frames: one unplaced, one over tile_cap, one wholly off the canvas
    for rs, cap_, cw_, ch_, (u, o, f) in ((recs, cap, cw, ch, (20, 21, 22)),
                                          ([tuple(int(v) for v in r[9:14]) for r in w["recs"]], w["cap"], w["cw"], w["ch"], (8, 7, 9))):
        lo, hi = min(u, o, f) - 1, max(u, o, f) + 1
        assert not rs[u][4] and rs[o][4] and rs[o][2] * rs[o][3] > cap_
        assert B.used(rs[f], cap_) and B._clip(rs[f], cw_, ch_) is None
        assert all(B.used(rs[k], cap_) and B._clip(rs[k], cw_, ch_) is not None for k in (lo, hi))
    assert E.tile_counts([(0, 0, 64, 4, 1), (70, 0, 65, 5, 1), (0, 0, 9, 9, 0), (0, 0, 40, 40, 1), (0, 0, 41, 40, 1)], 1600, 100,
                         50) == dict(warp=1 + 4 + 10, row=1 + 1 + 5, col=2 + 3 + 4, canvas=2 * 10, median=2 * 20)    # by hand


def test_bands_host_twin_against_the_model_on_the_multi_trip_case(nm):
    _, _, md, _ = bands_against_model(nm, E.multi_trip_case(), 3)
    assert (md["m"] > 10).sum() > 1000 and (md["M_frames"] > 1).sum() > 100000      # deep stacks and seams all over


@pytest.mark.parametrize("mode", MODES)
def test_median_host_twin_against_the_model_on_the_multi_trip_case(nm, mode):
    tiles, recs, cap, cw, ch = E.multi_trip_case()
    got, md = median_against_model(nm, E.multi_trip_case(), mode, 0.75, 0.1)
    assert md["m"].max() > 10 and (md["m"] > 10).sum() > 1000
    for k in (0, 20, 21, 22, 63):
        assert not md["counts"][k].any()
    assert (md["counts"][[k for k in range(64) if k not in (0, 20, 21, 22, 63)], 0] > 0).all() and md["counts"][32:, 1].any()
    # equal keys at the median itself, deeper than 10: the crowd's palette
    T, cover = M.stacks(tiles[30:44], recs[30:44], cw, ch, cap)
    y = M.key(T[..., :3])
    lab = np.clip(md["label"] - 30, 0, 13)
    y_med = np.take_along_axis(y, lab[None], 0)[0]
    shared = (cover & (T[..., 3] > F32(0.75)) & (y == y_med[None])).sum(0)
    assert ((shared >= 2) & (md["label"] >= 30) & (md["label"] < 44) & (md["m"] > 10)).sum() > 1000


# ---- B ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", E.BLUR_RADII + (0,))
def test_bands_host_twin_against_the_model_on_the_blur_tile_edges(nm, R):
    tiles, recs, cap, cw, ch = E.blur_edge_scene()
    canvas, cwts, md, _ = bands_against_model(nm, E.blur_edge_scene(), R)
    label = md["label"]
    n = len(recs)
    for k in range(n - E.EXTREME):                       # every rectangle shows somewhere, and a seam crosses most
        assert (label == k).any(), k
    for k in range(n - E.EXTREME, n):                    # the records at the int limits touch nothing
        assert B.used(recs[k], cap) and B._clip(recs[k], cw, ch) is None and not (label == k).any()
    assert sorted(r[2:4] for r in recs[2:11]) == sorted((w, h) for w in (127, 128, 129) for h in (7, 8, 9))
    assert [r[2:4] for r in recs[11:17]] == [(s, s) for s in (31, 32, 33, 63, 64, 65)]
    assert [r[2:4] for r in recs[17:20]] == [(1, 200), (200, 1), (1, 1)] and recs[20][:4] == (-200, -200, 260, 260)
    crossed = sum(1 for k in range(2, n - E.EXTREME) if (md["covered"] & (label != k))[B._clip(recs[k], cw, ch)[0]].any())
    assert crossed >= 15
    if R == 0:
        want, wstar, wl = B.winner(tiles, recs, cw, ch, cap)
        lab = wl != B.NONE
        assert np.array_equal(canvas[..., :3][lab], want[lab]) and np.array_equal(cwts[lab], wstar[lab])


# ---- C, bands ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", (0, 2, 7))
def test_bands_ties_fall_to_the_lowest_index_of_the_tie(nm, R):
    tiles, recs, cap, cw, ch = E.bands_ties_case()
    canvas, _, md, _ = bands_against_model(nm, E.bands_ties_case(), R)
    for name, want in E.TIE_WINNER.items():
        c0, c1 = E.TIE_BANDS[name]
        assert (md["label"][2:32, 3 + c0:3 + c1] == want).all(), name
        if R == 0:
            assert np.array_equal(canvas[2:32, 3 + c0:3 + c1, :3], B.store_f32(tiles[want][:, c0:c1, :3]))
    assert len(np.unique(md["label"][2:32, 35:73])) >= 2
    bad = bands_against_model(nm, E.bands_ties_case(), R, last_tie=True)[3]
    assert bad > 100                                     # the last_tie mutant of the model is rejected


@pytest.mark.parametrize("R", (0, 2, 7))
def test_bands_weight_limits_an_all_invalid_pixel_and_both_ends_of_the_store(nm, R):
    """Gained colours up to 2.0 and colours down to 0: bytes of 0 and of 255 count as `within the bound of an integer` only at
    the lower end (the model's product is clipped to [0, 255.5]), and the regions are small enough for the 1 % cap."""
    tiles, recs, cap, cw, ch = E.bands_special_case()
    canvas, cwts, md, _ = bands_against_model(nm, E.bands_special_case(), R)
    S, label = E.SPECIAL, md["label"]
    at = lambda name: (slice(S[name][0].start + 3, S[name][0].stop + 3), slice(S[name][1].start + 4, S[name][1].stop + 4))
    assert np.signbit(tiles[0][S["neg_zero"]][..., 3]).all() and not (label[at("neg_zero")] == 0).any()
    assert (label[at("neg_zero")] >= 1).all()
    den = label[at("denorm")]
    assert (den == 0).any() and not (den == 1).any() and (cwts[at("denorm")][den == 0] == F32(E.DENORM_MIN)).all()
    assert (label[at("flt_max")] == 1).all() and (cwts[at("flt_max")] == F32(E.FLT_MAX)).all()
    y0, x0 = at("dead")[0].start, at("dead")[1].start
    assert label[y0, x0] == B.NONE and md["covered"][y0, x0] and (label[y0 - 1:y0 + 2, x0 - 1:x0 + 2] != B.NONE).sum() == 8
    assert (label[at("dark")][:, :6] == 0).all() and (label[at("dark")][:, 6:] == 1).all() and (label[at("bright")] == 1).all()
    assert (canvas[at("bright")][..., :3] == 255).all() and (canvas[at("dark")][..., :3] == 0).any()
    assert R or (canvas[at("dark")][:, :6, :3] <= 1).all()
    if R:                                               # the low-band correction takes some dark outputs below zero
        assert (np.nan_to_num(md["out"])[at("dark")] < 0).any() and (np.nan_to_num(md["out"])[at("bright")] > 1).all()


def test_bands_with_flat_taps_and_with_subnormal_taps(nm):
    """Sigma away from R / 2. At R = 32, sigma = 1 the taps g[14] is subnormal in fp32 and g[15 ..] are exactly 0. The bound's
    relative-error argument does not cover a product that underflows, but each such product is off by at most 2^-149, far
    below u times any partial sum that holds the centre tap of a colour of at least 1e-30, which every colour here is; so
    the bound holds as it stands and the case is held to it, and to the exact properties as well: single coverage gives the
    frame's own sample (inside B.compare, whose bound is 0 there) and R = 0 is winner-take-all (above)."""
    R, sigma = E.SUBNORMAL_SIGMA
    g = nm.mosaic_bands_taps(R, sigma)
    tiny = float(np.finfo(F32).tiny)
    assert ((g > 0) & (g < tiny)).any() and (g[1:] == 0).any() and g[0] > 0.3
    assert ((g > 0) & (g < tiny)).sum() + (g == 0).sum() + (g >= tiny).sum() == R + 1
    bands_against_model(nm, B.case(17), R, sigma=sigma)
    bands_against_model(nm, E.bands_ties_case(), R, sigma=sigma)
    R, sigma = E.FLAT_SIGMA
    g = nm.mosaic_bands_taps(R, sigma)
    assert g[R] > 0.999 * g[0]
    bands_against_model(nm, B.case(17), R, sigma=sigma)
    bands_against_model(nm, E.bands_special_case(), R, sigma=sigma)


# ---- C, median --------------------------------------------------------------------------------------------------------------
CASES = sorted(E.median_cases())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CASES)
def test_median_host_twin_against_the_model_on_every_edge_case(nm, name, mode):
    case, w_min, tau, modes = E.median_cases()[name]
    if mode in modes:                                    # see median_cases: the grey stacks are SELECT only
        median_against_model(nm, case, mode, w_min, tau)


def test_the_median_tie_case_holds_what_it_promises(nm):
    tiles, recs, cap, cw, ch = E.median_ties_case()
    md = M.model(tiles, recs, cw, ch, cap, M.SELECT)
    row = lambda a: a[1, 2:2 + 96]
    assert row(md["m"])[:6].tolist() == [2, 4, 5, 64, 2, 8] and row(md["label"])[:6].tolist() == [0, 2, 3, 31, 62, 47]
    assert (md["counts"][:, 0] > 0).all()
    y_med = np.take_along_axis(md["key"], np.maximum(md["label"], 0)[None], 0)[0]
    shared = (md["valid"] & (md["key"] == y_med[None])).sum(0)
    assert (row(shared) >= 2).sum() > 60                 # a tie at the median in most columns
    colours = np.stack([t[0, :, :3] for t in tiles])     # distinct colours: a wrong median frame changes the bytes
    stored = B.store_f32(colours)
    for c in range(96):
        ks = np.flatnonzero(md["valid"][:, 1, 2 + c])
        assert len({tuple(stored[k, c]) for k in ks}) == len(ks), c
    out = M.model(tiles, recs, cw, ch, cap, M.MEAN, tau=0.1)
    assert out["counts"][32:, 1].any() and (row(out["support"]) < row(out["m"])).any()


def test_the_median_key_case_holds_what_it_promises(nm):
    tiles, recs, cap, cw, ch = E.median_keys_case()
    md = M.model(tiles, recs, cw, ch, cap, M.SELECT)
    tiny = F32(np.finfo(F32).tiny)
    key = md["key"][:, 1, 2:10]                        # the rectangle is at (2, 1): its first row
    valid = md["valid"][:, 1, 2:10]
    assert md["m"][1, 2:10].tolist() == [5, 5, 4, 5, 3, 2, 3, 1]
    assert (np.abs(key[:, 0][valid[:, 0]]) < tiny).all() and (key[:, 0][valid[:, 0]] > 0).all()
    assert (key[:, 1][valid[:, 1]] < 0).sum() == 4
    assert np.signbit(key[3, 2]) and key[3, 2] == 0 and not np.signbit(key[2, 2]) and key[36, 2] > 0 > key[37, 2]
    assert key[0, 3] == F32(E.FLT_MAX) and key[1, 3] == -F32(E.FLT_MAX) and valid[:2, 3].all()
    assert valid[62:, 5].all() and valid[:, 5].sum() == 2 and md["label"][1, 2 + 7] == 47
    assert not md["counts"][13].any() and not md["counts"][50].any()
    sub = M.model(tiles, recs, cw, ch, cap, M.MEAN, tau=E.DENORM_MIN * 3)
    assert sub["support"][1, 2 + 6] == 2 and sub["counts"][60, 1] >= 1        # 7 and 9 steps within three, 29 not


@pytest.mark.parametrize("mutant", ("high_tie", "strict"))
def test_the_model_mutants_turn_the_new_median_cases_red(nm, mutant):
    if mutant == "high_tie":
        names = ("ties", "greys0", "greys2")
    else:
        names = ("tau_exact", "tau_zero")
    for name in names:
        case, w_min, tau, _ = E.median_cases()[name]
        mode = M.SELECT if mutant == "high_tie" else M.MEAN
        median_against_model(nm, case, mode, w_min, tau)
        with pytest.raises(AssertionError):
            median_against_model(nm, case, mode, w_min, tau, **{mutant: True})
    if mutant == "high_tie":                             # and on the multi-trip case's crowd
        with pytest.raises(AssertionError):
            median_against_model(nm, E.multi_trip_case(), M.SELECT, 0.75, 0.1, high_tie=True)
