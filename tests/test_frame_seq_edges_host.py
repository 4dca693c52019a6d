"""The host twins of the frame-weights, frame-quality and KLT stages against their numpy models on the inputs of
tests/frame_seq_edges_ref.py, exactly, and the conditions that make those inputs worth running: that a result next to a chunk
seam depends on data from across it, that the sums reach the sizes their registers were dimensioned for, that the tracker
meets them without calling the window flat. The device against the host twins on the same inputs:
tests/test_gpu_frame_seq_edges.py.

Two sizes the kernels' comments name cannot be reached by any input, and the tests assert what can be instead:
  * a wave's 32-bit sum of the frame-quality walk is at most 64 * 32 * 1 040 400 = 2 130 739 200, the bound of the kernel's
    static_assert, which is 0.8 % BELOW 2^31; test_quality_saturated_checkerboard reaches it exactly;
  * the tracker's -bx and -by are at most 120 * 4080^2 = 1 997 568 000 at radius 7, 7 % below 2^31, whatever the two planes
    hold (test_no_window_brings_the_mismatch_sums_past_2_31 has the argument and the enumeration); the cases reach exactly
    that, and Gxx = Gyy = 225 * 4080^2 = 3 745 440 000, above 2^31."""
import numpy as np
import pytest

import frame_quality_ref as FQ
import frame_seq_edges_ref as E
import frame_weights_ref as FW
import klt_ref as K

F32 = np.float32


# ---- A. frame weights across chunk seams ------------------------------------------------------------------------------------
def model_subset(fw, fh, R):
    """the frames the model is run on: all of them at radius 1 and 8; at 31 and 64, where the model costs (2R + 1)^2 passes
    over the frame, the frame with the 2 x 2 cluster on the seam, the last planted frame and the frames_for frame"""
    n = len(E.seam_frames(fw, fh))
    return list(range(n)) if R <= 8 else [4, n - 2, n - 1]


@pytest.mark.parametrize("fw,fh", E.FW_SHAPES)
def test_weights_host_twin_equals_the_model_across_the_seams(nm, fw, fh):
    frames, bases = E.seam_frames(fw, fh), E.seam_bases(fw, fh)
    some_valid = some_seed = False
    for kw in E.fw_configs(E.FW_SHAPES.index((fw, fh))):
        if kw["R"] == 64 and fw * fh > 40000 and kw["min_count"] != (1, 4, 9)[E.FW_SHAPES.index((fw, fh)) % 3]:
            continue                                             # one min_count at radius 64 on the largest frames
        sub = [frames[i] for i in model_subset(fw, fh, kw["R"])]
        kw = E.with_base(kw, bases)
        got, want = FW.run_host(nm, sub, **kw), FW.run_model(sub, **kw)
        FW.same(got, want)
        some_valid |= bool((want["counts"][:, 1] > 0).all())
        some_seed |= bool((want["counts"][:, 0] > 0).all())
    assert some_valid and some_seed


@pytest.mark.parametrize("fw,fh", E.FW_SHAPES)
def test_weights_next_to_a_seam_depend_on_the_other_side(fw, fh):
    E.assert_seam_dependence(fw, fh)
    assert len(E.seams_of(fw)) == {2048: 0, 2049: 1, 2112: 1, 4097: 2, 7681: 3}[fw]
    assert (fw + 63) // 64 - 32 * len(E.seams_of(fw)) == {2048: 32, 2049: 1, 2112: 1, 4097: 1, 7681: 25}[fw]    # the last chunk's blocks


def test_weights_batch_of_sixty_four_patterns(nm):
    frames = E.batch_frames()
    assert len({f.tobytes() for f in frames}) == 64
    for kw in (dict(R=8, margin=1, min_count=4), dict(R=8, margin=0, min_count=1, border=False, mask_format=FW.TEX_F32)):
        got = FW.run_host(nm, frames, lo=FW.LO, hi=FW.HI, **kw)
        FW.same(got, FW.run_model(frames, lo=FW.LO, hi=FW.HI, **kw))
        assert (got["counts"][:, 1] > 0).all() and got["counts"][:, 0].any()
    assert any(E.seam_dependence(frames[k], E.CHUNK, 1)[1] for k in (29, 36)) and any(E.seam_dependence(frames[k], E.CHUNK, 1)[0] for k in (30, 37))


# ---- B. frame quality at its sum bounds -------------------------------------------------------------------------------------
def both_stats(nm, frames, masks=None, grid=(1, 1)):
    got = nm.frame_quality_host(frames, masks=masks, lo=0, hi=255, grid=grid)
    assert np.array_equal(got, FQ.stats_model(frames, masks, 0, 255, grid)), grid
    return got


@pytest.mark.parametrize("grid", [(1, 1), (2, 3), (8, 8)])
def test_quality_saturated_checkerboard(nm, grid):
    """(a) 192 x 160 is three blocks of 64 columns and five bands of 32 rows. The wave that takes columns 64 .. 127 and rows
    32 .. 63 touches neither the frame's border nor, with one cell, a cell border: all its 64 * 32 pixels are measured with
    L2 = 1 040 400, and its 32-bit sum is the static_assert's bound, 2 130 739 200."""
    f = E.checker(192, 160)
    s = both_stats(nm, [f], grid=grid)[0]
    assert (s[..., 3] == np.uint64(E.L2_MAX) * s[..., 0]).all() and s[..., 0].all() and s[..., 0].sum() == 190 * 158
    assert not s[..., 4].any() and not s[..., 5].any() and not s[..., 6].any() and s[..., 7].sum() == 192 * 160
    if grid == (1, 1):
        Y = FQ.luma(f)
        measured = FQ.measured_of(FQ.classes(f, None, 0, 255)[3])
        P = np.pad(Y, 1)
        L = P[1:-1, :-2] + P[1:-1, 2:] + P[:-2, 1:-1] + P[2:, 1:-1] - 4 * Y
        block = (slice(32, 64), slice(64, 128))
        assert measured[block].all() and int((L * L)[block].sum()) == E.WAVE_BOUND == 2130739200
        assert 0.99 * 2 ** 31 < E.WAVE_BOUND < 2 ** 31 and s[0, 0, 3] > 2 ** 32


def test_quality_one_cell_of_a_1080p_checkerboard(nm):
    """(b) every workgroup adds into one cell: 1918 * 1078 measured pixels of 1 040 400 are 2.15e12 > 2^40"""
    s = both_stats(nm, [E.checker(1920, 1080)])[0, 0, 0]
    assert s[0] == 1918 * 1078 and s[3] == np.uint64(E.L2_MAX) * s[0] and s[3] > 2 ** 40


def test_quality_the_largest_squared_gradient(nm):
    """(c) G2 = hd^2 + dv^2 with |hd|, |dv| <= 255 is at most 2 * 255^2 = 130 050. Of the saturated patterns the model is
    asked about, squares of ONE pixel have both differences 0, columns 0 0 255 255 reach 255^2, and squares of TWO pixels
    reach the bound at every measured pixel: Y(x + 1) and Y(x - 1) lie in neighbouring squares wherever x is."""
    fw, fh = 192, 160
    per_pixel = {}
    for name, f in (("squares of 1", E.checker(fw, fh)), ("stripes", E.stripes(fw, fh)), ("squares of 2", E.checker(fw, fh, 2))):
        m = FQ.stats_model([f], None, 0, 255, (1, 1))[0, 0, 0]
        assert m[4] % m[0] == 0
        per_pixel[name] = int(m[4] // m[0])
    assert per_pixel == {"squares of 1": 0, "stripes": 255 * 255, "squares of 2": E.G2_MAX} and E.G2_MAX == 130050
    for grid in ((1, 1), (8, 8)):
        s = both_stats(nm, [E.checker(fw, fh, 2), E.checker(fw, fh, 2, 1)], grid=grid)
        assert (s[..., 4] == np.uint64(E.G2_MAX) * s[..., 0]).all() and s[..., 0].all()


@pytest.mark.parametrize("masked", [None, FQ.U8N, FQ.TEX_F32])
def test_quality_sixty_four_variants(nm, masked):
    """(d) and (e): the host twin on the 64 variants at 130 x 70, without masks and with the cross masks of both formats"""
    frames = E.quality_variants()
    masks = None if masked is None else [E.cross_masks(130, 70, masked)] * 64
    for grid in ((1, 1), (8, 8)):
        s = both_stats(nm, frames, masks, grid)
        assert s[..., 0].reshape(64, -1).sum(axis=1).all() and len({a.tobytes() for a in s}) > 32
        if masked is not None:                                    # the cross removes a row and a column and their neighbours' measure
            assert (s[..., 7].reshape(64, -1).sum(axis=1) == 130 * 70 - 130 - 70 + 1).all()
            assert (s[0, ..., 0].sum() == 128 * 68 - 3 * 128 - 3 * 68 + 9)


def test_pick_on_the_large_statistics_equals_the_model(nm):
    """(f) sharp_of and the median on words above 2^32 and of the size of 2^40"""
    cases = E.pick_inputs(nm)
    assert cases["a, b and c on one cell"][0][..., 3].min() >= 0 and cases["a, b and c on one cell"][0][1, 0, 0, 3] > 2 ** 40
    assert cases["a, b and c on one cell"][0][0, 0, 0, 3] > 2 ** 32 and cases["words of 2^40"][0][..., 3].min() > 2 ** 49
    for name, (stats, chain, keep, kw) in cases.items():
        got = nm.keyframe_pick_host(stats, chain, 64, 48, keep, **kw)
        FQ.same_pick(got, FQ.pick_model(stats, chain, 64, 48, keep, **kw))
        assert got.key_count[0] >= 2, name
    tied = nm.keyframe_pick_host(*cases["all scores equal"][:2], 64, 48, 8, **E.PICK_KW)
    assert tied.keys.tolist() == [0, 2, 4, 6, 8, 10, -1, -1] and (tied.scores[:, 0] == 7.0).all()     # the lower index wins
    big = nm.keyframe_pick_host(*cases["words of 2^40"][:2], 64, 48, 12, **dict(E.PICK_KW, rel=0.998, w=3))
    assert big.flags.tolist().count(0) < 12 and (big.flags & FQ.BLURRED).any() and not (big.flags & FQ.BLURRED).all()


# ---- C. KLT -------------------------------------------------------------------------------------------------------------------
def klt_case(A, B, xs, ys, levels, radius):
    return dict(A=A, B=B, xs=xs, ys=ys, nA=len(xs), capA=len(xs) + 2, kw=dict(levels=levels, radius=radius, iterations=6, fb_max=1.5))


def test_no_window_brings_the_mismatch_sums_past_2_31():
    """a row of 15 taps gives at most 8 * 4080^2, so 15 rows give 120 * 4080^2 < 2^31 < 129.004 * 4080^2"""
    assert E.mismatch_row_bound(15) == 8 and 15 * 8 == E.MISMATCH_TAPS
    assert E.MISMATCH_TAPS * E.UNIT2 < 2 ** 31 < 225 * E.UNIT2


def test_klt_sums_reach_their_sizes_and_equal_the_model(nm):
    """Which pair gives what, at radius 7 and level 0, from nm_klt_sums_host: every pair has Gxx = Gyy = 225 * 4080^2 > 2^31 at
    its whole-pixel points; "one right" brings bx to -120 * 4080^2 (the largest any input can), "one down" does so for by,
    "the inverse, one right" brings bx to +120 * 4080^2; none of these points is lost as FLAT."""
    xs, ys = E.klt_points()
    extremes = {}
    for name, (A, B) in E.klt_pairs().items():
        pyr, _ = nm.gray_pyramid_host([A, B], levels=1)
        QA, QB = K.quantise(K.pyramid(A, 1)), K.quantise(K.pyramid(B, 1))
        rows = []
        for r in (7, 3):
            for x, y in zip(xs, ys):
                sums, flags = nm.klt_sums_host(pyr[0], pyr[1], E.KW_, E.KH_, 1, 0, r, x, y, 0.0, 0.0)
                tpl = K.template(QA[0], E.KW_, E.KH_, F32(x), F32(y), r)
                assert flags == 0 and tpl is not None and sums[:3] == tpl[3:6]
                assert sums[3:] == K.mismatch(QB[0], E.KW_, E.KH_, F32(x), F32(y), r, tpl)
                if r == 7:
                    rows.append(sums)
        rows = np.array(rows, dtype=object)
        track = nm.klt_track_host([pyr[0]], [pyr[1]], E.KW_, E.KH_, [xs], [ys], [len(xs)], levels=1, radius=7, iterations=6)
        big = [i for i in range(len(xs)) if rows[i, 0] > 2 ** 31 or rows[i, 2] > 2 ** 31]
        assert len(big) >= 10 and any(track.reason[0][i] != K.FLAT for i in big)
        assert max(rows[:, 0]) == max(rows[:, 2]) == 225 * E.UNIT2 and all(K.gate(*rows[i, :3], 7, 0.0) is not None for i in big)
        extremes[name] = (min(rows[:, 3]), max(rows[:, 3]), min(rows[:, 4]), max(rows[:, 4]))
    top = E.MISMATCH_TAPS * E.UNIT2
    assert extremes["one right"][0] == -top and extremes["one down"][2] == -top and extremes["the inverse, one right"][1] == top


@pytest.mark.parametrize("name", sorted(E.klt_pairs()))
def test_klt_tracks_on_the_block_pattern_equal_the_model(nm, name):
    A, B = E.klt_pairs()[name]
    xs, ys = E.klt_points()
    seen = set()
    for levels in (1, 3):
        for radius in (7, 3):
            c = klt_case(A, B, xs, ys, levels, radius)
            pyr, _ = nm.gray_pyramid_host([A, B], levels=levels)
            px, py = K.padded(c)
            got = nm.klt_track_host([pyr[0]], [pyr[1]], E.KW_, E.KH_, [px], [py], [c["nA"]], capA=c["capA"], **c["kw"])
            dst_x, dst_y, matches, count, reason, resid, fb = K.model_case(c)
            assert np.array_equal(got.reason[0], reason) and np.array_equal(got.matches[0], matches) and int(got.count[0]) == count
            for g, want in ((got.dst_xs[0], dst_x), (got.dst_ys[0], dst_y), (got.residual[0], resid), (got.fb_error[0], fb)):
                assert np.array_equal(g.view(np.uint32), want.view(np.uint32))
            seen |= set(reason[:c["nA"]].tolist())
    assert K.FLAT not in seen or len(seen) > 1


@pytest.mark.parametrize("n", [32, 33, 40])
def test_klt_split_pairs_equal_the_single_pair_results(nm, n):
    c = E.split_case(n)
    pyr, _ = nm.gray_pyramid_host(c["grays"], levels=3)
    run = lambda ks: nm.klt_track_host([pyr[c["ia"][k]] for k in ks], [pyr[c["ib"][k]] for k in ks], 97, 61, [c["xs"]] * len(ks),
                                       [c["ys"]] * len(ks), [c["nAs"][k] for k in ks], H=c["H"][ks], status=c["status"][ks], **c["kw"])
    full = run(list(range(n)))
    for k in E.split_pairs(n):
        one = run([k])
        for a, b in zip(one, full):
            assert np.array_equal(a[0], b[k])
        A, B = c["grays"][c["ia"][k]], c["grays"][c["ib"][k]]
        want = K.model_case(dict(A=A, B=B, xs=c["xs"], ys=c["ys"], nA=c["nAs"][k], capA=c["capA"], H=c["H"][k], status=int(c["status"][k]),
                                 kw={q: v for q, v in c["kw"].items() if q != "capA"}))
        assert np.array_equal(one.reason[0], want[4]) and int(one.count[0]) == want[3]
    assert all(full.count[k] > 0 for k in E.split_pairs(n)) and len(set(full.count.tolist())) > 3


@pytest.mark.parametrize("fw,fh,levels", E.PYRAMIDS + [(33, 17, 3)])
def test_pyramid_shapes_equal_the_model(nm, fw, fh, levels):
    g = E.pyramid_gray(fw, fh)
    for name, mask in E.pyramid_masks(fw, fh).items():
        pyr, mp = nm.gray_pyramid_host([g], levels=levels, mask=mask)
        assert np.array_equal(pyr[0].view(np.uint32), K.block(K.pyramid(g, levels), F32).view(np.uint32))
        assert np.array_equal(mp, K.block(K.mask_pyramid(mask, levels), np.uint8)), name
    if (fw, fh, levels) == (130, 70, 6):          # the top level tells the masks apart: its reach is clamped, not wrapped
        top = {name: nm.gray_pyramid_level(nm.gray_pyramid_host([g], levels=6, mask=m)[1], fw, fh, 5)
               for name, m in E.pyramid_masks(fw, fh).items()}
        assert top["one corner"].tolist() == [[1, 1, 1, 1, 1], [1, 1, 1, 0, 0], [1, 1, 1, 0, 0]]
        assert top["one edge"].tolist() == [[0, 0, 1, 1, 1]] * 3 and not top["corners and edges"].any()
