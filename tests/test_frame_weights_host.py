"""The host twin of the frame-weights stage (nm_frame_weights_host, compiled from the functions the kernels use) against the
numpy model of tests/frame_weights_ref.py, bit for bit on every output; the named edges of the definition; slot and history
independence; every refusal; and the stage end to end on the loop-closure views with a disc field of view (figures: DESIGN.md
section 7, "Frame weights"). The device against the host twin: tests/test_gpu_frame_weights.py."""
import ctypes as C

import numpy as np
import pytest

import frame_weights_ref as FW

F32 = np.float32
INVALID = 1                                     # hipErrorInvalidValue


def both(nm, frames, **kw):
    got, want = FW.run_host(nm, frames, **kw), FW.run_model(frames, **kw)
    FW.same(got, want)
    return got


@pytest.mark.parametrize("R", FW.RADII)
@pytest.mark.parametrize("fw,fh", FW.SHAPES)
def test_host_twin_equals_the_model(nm, fw, fh, R):
    """min_count, border, base, margin and both mask formats at every shape and radius; D is modelled once per seed set"""
    frames = FW.frames_for(fw, fh)
    some_valid = False
    for min_count in FW.MIN_COUNTS:
        for base in (None, FW.base_for(fw, fh)):
            seed = [FW.seeds(f, FW.LO, FW.HI, min_count, base) for f in frames]
            for border in (True, False):
                D = [FW.dist2(s, R, border) for s in seed]
                for margin in FW.margins(R):
                    for fmt in (FW.U8N, FW.TEX_F32):
                        outs = [FW.outputs_of(d, s, R, margin, fmt) for d, s in zip(D, seed)]
                        want = {q: np.stack([o[q] for o in outs]) for q in FW.KINDS + ("counts",)}
                        got = FW.run_host(nm, frames, lo=FW.LO, hi=FW.HI, R=R, margin=margin, min_count=min_count, border=border,
                                          base=base, mask_format=fmt)
                        FW.same(got, want)
                        some_valid |= bool((want["counts"][:, 1] > 0).all())
    assert some_valid                            # no comparison of empty valid sets only


def test_radius_64(nm):
    frames = FW.frames_for(150, 140)[:2]
    got = both(nm, frames, lo=FW.LO, hi=FW.HI, R=64, margin=3, min_count=4, border=True, base=FW.base_for(150, 140))
    assert (got["counts"][:, 1] > 0).all() and got["dist2"].max() > 32 * 32


@pytest.mark.parametrize("R", (3, 9, 17))
def test_single_seed_and_the_clip(nm, R):
    """R^2 - 1 = (R - 1)(R + 1) is a sum of two squares for these R, so probes at squared distance R^2 - 1, R^2 and R^2 + 1
    exist: the first keeps its distance, the other two read R^2"""
    n = 4 * R + 1
    c = 2 * R
    frame = FW.with_seeds(n, n, [(c, c)])
    got = both(nm, [frame], lo=FW.LO, R=R, border=False)
    y, x = np.mgrid[0:n, 0:n]
    d2 = (x - c) ** 2 + (y - c) ** 2
    assert np.array_equal(got["dist2"][0], np.minimum(d2, R * R))
    a, b = {3: (2, 2), 9: (8, 4), 17: (12, 12)}[R]
    D = got["dist2"][0]
    assert a * a + b * b == R * R - 1 and D[c + b, c + a] == R * R - 1 and D[c - a, c - b] == R * R - 1
    assert D[c, c + R] == D[c + R, c] == D[c, c - R] == D[c - R, c] == R * R               # exactly R away
    assert D[c + 1, c + R] == D[c + R, c - 1] == R * R                                    # R^2 + 1, clipped
    assert D[c, c + R - 1] == (R - 1) ** 2 and got["counts"].tolist() == [[1, n * n - 1]]
    assert got["wts"][0][c, c + R] == F32(1) and got["wts"][0][c, c] == 0


@pytest.mark.parametrize("border", (True, False))
def test_seeds_at_the_frame_corners(nm, border):
    fw, fh = 70, 9
    frame = FW.with_seeds(fw, fh, [(0, 0), (fw - 1, 0), (0, fh - 1), (fw - 1, fh - 1)])
    got = both(nm, [frame], lo=FW.LO, R=8, border=border)
    assert got["counts"][0, 0] == 4 and got["dist2"][0][4, 35] == (25 if border else 64)


@pytest.mark.parametrize("side", ("left", "right"))
@pytest.mark.parametrize("d", (63, 64, 65))
def test_a_seed_in_the_neighbouring_block_only(nm, side, d):
    """the probe sits in block 1 of a row of 200 pixels, the only seed d pixels away in block 0 or block 2"""
    probe = 74 if side == "left" else 70
    at = probe - d if side == "left" else probe + d
    assert at // 64 == (0 if side == "left" else 2) and probe // 64 == 1
    for fh in (1, 3):
        frame = FW.with_seeds(200, fh, [(at, fh // 2)])
        got = both(nm, [frame], lo=FW.LO, R=64, border=False)
        assert got["dist2"][0][fh // 2, probe] == min(d * d, 64 * 64)


@pytest.mark.parametrize("fw,fh", [(5, 40), (40, 5), (3, 3), (1, 50)])
def test_frames_narrower_or_lower_than_the_radius(nm, fw, fh):
    frame = FW.with_seeds(fw, fh, [(fw // 2, fh // 3)])
    for border in (True, False):
        got = both(nm, [frame, FW.blank(fw, fh)], lo=FW.LO, R=31, margin=0, border=border)
        assert (got["counts"][:, 1] > 0).all()


def test_an_all_seed_frame(nm):
    fw, fh = 67, 11
    for fmt in (FW.U8N, FW.TEX_F32):
        got = both(nm, [FW.blank(fw, fh, 0)], lo=FW.LO, R=8, mask_format=fmt)
        assert not got["mask"].any() and not got["wts"].any() and not got["dist2"].any()
        assert got["counts"].tolist() == [[fw * fh, 0]]


def test_a_seedless_frame_without_border(nm):
    fw, fh = 67, 11
    got = both(nm, [FW.blank(fw, fh)], lo=FW.LO, hi=FW.HI, R=8, margin=7, border=False)
    assert (got["dist2"] == 64).all() and (got["wts"].view(np.uint32) == F32(1).view(np.uint32)).all() and (got["mask"] == 255).all()
    assert got["counts"].tolist() == [[0, fw * fh]]


@pytest.mark.parametrize("min_count", (2, 4, 9))
def test_the_window_count_decides_at_min_count(nm, min_count):
    """the window count includes the pixel itself: with min_count - 1 raw-bad pixels in its window a raw-bad pixel is no
    seed, with min_count it is; in a frame corner the window holds four pixels"""
    window = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1)]
    for cx, cy in ((20, 4), (0, 0), (69, 8)):
        inside = [(cx + dx, cy + dy) for dx, dy in window if 0 <= cx + dx < 70 and 0 <= cy + dy < 9]
        if len(inside) < min_count:
            continue
        for count, is_seed in ((min_count - 1, False), (min_count, True)):
            got = both(nm, [FW.with_seeds(70, 9, inside[:count])], lo=FW.LO, R=8, min_count=min_count, border=False)
            assert (got["dist2"][0][cy, cx] == 0) == is_seed, (cx, cy, count)
            if not is_seed:
                assert got["counts"][0, 0] == 0


def test_lo_0_and_hi_255_switch_the_tests_off(nm):
    fw, fh = 40, 6
    frames = [FW.blank(fw, fh, 0), FW.blank(fw, fh, 255), FW.frames_for(65, 9)[2][:6, :40]]
    got = both(nm, frames, lo=0, hi=255, R=8, border=False)
    assert not got["counts"][:, 0].any() and (got["dist2"] == 64).all()
    dark = both(nm, frames, lo=1, hi=255, R=8, border=False)
    bright = both(nm, frames, lo=0, hi=254, R=8, border=False)
    assert dark["counts"][:, 0].tolist()[:2] == [fw * fh, 0] and bright["counts"][:, 0].tolist()[:2] == [0, fw * fh]


# ---- slots and history ------------------------------------------------------------------------------------------------------
KW = dict(lo=FW.LO, hi=FW.HI, R=8, margin=1, min_count=4, border=True)


def test_permuting_the_frames_permutes_the_outputs_and_repeats_agree(nm):
    frames = FW.frames_for(65, 9) + FW.frames_for(65, 9, seed=1)
    perm = [4, 0, 5, 2, 1, 3]
    a, b = FW.run_host(nm, frames, **KW), FW.run_host(nm, [frames[p] for p in perm], **KW)
    for q in FW.KINDS + ("counts",):
        assert np.array_equal(FW.bits(b[q]), FW.bits(a[q][perm])), q
    r = FW.run_host(nm, [frames[1], frames[2], frames[1]], **KW)
    for q in FW.KINDS + ("counts",):
        assert np.array_equal(FW.bits(r[q][0]), FW.bits(r[q][2])) and np.array_equal(FW.bits(r[q][0]), FW.bits(a[q][1])), q
    assert (a["counts"][:, 1] > 0).all()


def test_one_frame_and_sixty_four_agree(nm):
    frames = [FW.frames_for(33, 17, seed=s)[s % 3] for s in range(64)]
    all64 = FW.run_host(nm, frames, **KW)
    for k in (0, 31, 63):
        one = FW.run_host(nm, [frames[k]], **KW)
        for q in FW.KINDS + ("counts",):
            assert np.array_equal(FW.bits(one[q][0]), FW.bits(all64[q][k])), (q, k)


def raw_host(nm, frames, outs, n=None, fw=None, fh=None, base=None, lo=FW.LO, hi=FW.HI, min_count=1, border=1, R=8, margin=0,
             fmt=FW.U8N, give=("mask", "wts", "dist2", "counts"), null_frames=False, null_entry=None):
    """nm_frame_weights_host on caller-owned outputs; returns the status. outs: dict of (n, fh, fw) arrays and counts"""
    k = len(frames)
    table = lambda arrs: (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    tabs = {q: table(list(outs[q])) for q in FW.KINDS}
    ft = table(frames)
    if null_entry == "frames":
        ft[k - 1] = None
    elif null_entry:
        tabs[null_entry][k - 1] = None
    arg = lambda q: tabs[q] if q in give else None
    return nm.lib().nm_frame_weights_host(k if n is None else n, None if null_frames else ft,
                                          frames[0].shape[1] if fw is None else fw, frames[0].shape[0] if fh is None else fh,
                                          None if base is None else base.ctypes.data, lo, hi, min_count, border, R, margin,
                                          arg("mask"), fmt, arg("wts"), arg("dist2"),
                                          outs["counts"].ctypes.data if "counts" in give else None)


def garbage(n, fw, fh, fmt=FW.U8N, seed=5):
    rng = np.random.default_rng(seed)
    return dict(mask=rng.integers(0, 256, (n, fh, fw), dtype=np.uint8) if fmt == FW.U8N else rng.random((n, fh, fw), dtype=F32),
                wts=rng.random((n, fh, fw), dtype=F32), dist2=rng.integers(0, 65536, (n, fh, fw), dtype=np.uint16),
                counts=rng.integers(1, 1 << 62, (n, 2), dtype=np.uint64))


def test_outputs_full_of_garbage_end_the_same(nm):
    frames = FW.frames_for(65, 9)
    want = FW.run_host(nm, frames, **KW)
    for seed in (5, 6):
        outs = garbage(3, 65, 9, seed=seed)
        assert raw_host(nm, frames, outs, R=8, margin=1, min_count=4) == 0
        FW.same(outs, want)


REFUSALS = [dict(n=0), dict(n=65), dict(fw=0), dict(fh=0), dict(fw=32768), dict(fh=32768), dict(lo=-1), dict(lo=256),
            dict(hi=-1), dict(hi=256), dict(min_count=0), dict(min_count=10), dict(R=0), dict(R=65), dict(margin=-1),
            dict(margin=8), dict(R=1, margin=1), dict(fmt=1), dict(fmt=3), dict(give=()), dict(null_frames=True),
            dict(null_entry="frames"), dict(null_entry="mask"), dict(null_entry="wts"), dict(null_entry="dist2")]


@pytest.mark.parametrize("bad", REFUSALS, ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_refusals_leave_the_outputs_untouched(nm, bad):
    frames = FW.frames_for(65, 9)
    outs = garbage(3, 65, 9)
    keep = {q: a.copy() for q, a in outs.items()}
    assert raw_host(nm, frames, outs, **bad) == INVALID
    FW.same(outs, keep)
    # the device entry refuses the same arguments before any device access: host tables of made-up device pointers
    if "null_entry" in bad or "null_frames" in bad:
        return
    fake = (C.c_void_p * 64)(*[4096 * (k + 1) for k in range(64)])
    args = dict(n=3, fw=65, fh=9, lo=FW.LO, hi=FW.HI, min_count=1, R=8, margin=0, fmt=FW.U8N, give=("mask",))
    args.update(bad)
    given = lambda q: fake if q in args["give"] else None
    status = nm.lib().nm_frame_weights_batch_dev(args["n"], fake, args["fw"], args["fh"], None, args["lo"], args["hi"],
                                                 args["min_count"], 1, args["R"], args["margin"], given("mask"), args["fmt"],
                                                 given("wts"), given("dist2"), None, C.c_void_p(4096), None)
    assert status == INVALID


def test_device_entry_refuses_null_tables_and_a_null_workspace(nm):
    lib = nm.lib()
    fake = (C.c_void_p * 64)(*[4096 * (k + 1) for k in range(64)])
    holed = (C.c_void_p * 64)(*[4096 * (k + 1) if k != 2 else None for k in range(64)])
    call = lambda frames, masks, wts, d2, ws: lib.nm_frame_weights_batch_dev(3, frames, 65, 9, None, 0, 255, 1, 1, 8, 0, masks,
                                                                             FW.U8N, wts, d2, None, ws, None)
    ws = C.c_void_p(4096)
    assert call(None, fake, None, None, ws) == INVALID and call(holed, fake, None, None, ws) == INVALID
    assert call(fake, holed, None, None, ws) == INVALID and call(fake, None, holed, None, ws) == INVALID
    assert call(fake, None, None, holed, ws) == INVALID and call(fake, fake, None, None, None) == INVALID
    assert call(fake, None, None, None, ws) == INVALID
    assert lib.nm_frame_weights_workspace_bytes(3, 65, 9) >= 3 * 65 * 9
    assert [lib.nm_frame_weights_workspace_bytes(*s) for s in ((0, 65, 9), (65, 65, 9), (3, 0, 9), (3, 65, 32768))] == [0] * 4


def test_the_wrapper_rejects_what_the_entry_refuses(nm):
    frames = FW.frames_for(7, 3)
    for kw in (dict(R=0), dict(R=65), dict(margin=8, R=8), dict(lo=256), dict(hi=-1), dict(min_count=0), dict(mask_format=1),
               dict(want=()), dict(want=("mask", "mask")), dict(want=("weights",))):
        with pytest.raises(nm.NmError):
            nm.frame_weights_host(frames, **kw)
    assert nm.frame_weights_host(frames, want=(), counts=True).shape == (3, 2)


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_end_to_end_a_disc_field_of_view_on_the_loop_closure_views(nm, oracle):
    """Ten loop-closure views, black outside the inscribed disc, one saturated block each: the feather canvas with this
    stage's masks and weights is closer to the clean-frames feather canvas than the rectangle feather with an all-ones mask,
    over the canvas pixels that some frame's valid region covers. Measured with the host twins and the CPU oracle: mean
    absolute byte difference 4.842 with the stage, 26.387 with the rectangle feather, over 662 286 pixels."""
    e = FW.e2e_host(nm, oracle)
    assert (e["mask"].reshape(len(e["views"]), -1) == 255).any(axis=1).all() and e["sel"].sum() > 100000
    print("mean absolute byte difference to the clean feather canvas over %d pixels: stage %.3f, rectangle feather %.3f"
          % (e["sel"].sum(), e["fig"]["stage"], e["fig"]["rectangle"]))
    assert e["fig"]["stage"] < e["fig"]["rectangle"]
