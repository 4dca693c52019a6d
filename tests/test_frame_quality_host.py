"""The host twins of the frame-quality stage (nm_frame_quality_host, nm_keyframe_pick_host, nm_slots_gather_host) against the
numpy model of tests/frame_quality_ref.py, exactly; every refusal of the six entries (the device entries refuse before any
launch or device access, so they are called here with pointers that are never dereferenced); and the stage end to end on a
pan over the loop-closure scene with blurred views."""
import ctypes as C

import numpy as np
import pytest

import frame_quality_ref as FQ

F32 = np.float32


def host_stats(nm, frames, masks=None, lo=0, hi=255, grid=(4, 4)):
    return nm.frame_quality_host(frames, masks=masks, lo=lo, hi=hi, grid=grid)


@pytest.mark.parametrize("fw,fh", FQ.SHAPES)
def test_host_statistics_equal_the_model(nm, fw, fh):
    frames = FQ.frames_for(fw, fh)
    some = False
    for grid in FQ.grids_for(fw, fh):
        for masks in (None, FQ.masks_for(fw, fh, FQ.U8N), FQ.masks_for(fw, fh, FQ.TEX_F32)):
            for lo, hi in ((FQ.LO, FQ.HI), (0, 255)):
                want = FQ.stats_model(frames, masks, lo, hi, grid)
                got = host_stats(nm, frames, masks, lo, hi, grid)
                assert got.dtype == np.uint64 and np.array_equal(got, want), (grid, lo, hi)
                some |= bool(want[..., 0].any())
                if (lo, hi) == (0, 255):
                    assert not want[..., 5].any() and not want[..., 6].any()
    assert some or fw < 3 or fh < 3


def test_mask_thresholds_and_the_photometric_bounds():
    """byte 127 / 128, float 0.5 / nextafter(0.5), and max(B, G, R) at exactly lo and hi, on the model itself"""
    f = np.full((1, 4, 4), 100, np.uint8)
    assert FQ.eligible(np.array([[127, 128]], np.uint8), None).tolist() == [[False, True]]
    assert FQ.eligible(np.array([[0.5, np.nextafter(F32(0.5), F32(1))]], F32), None).tolist() == [[False, True]]
    f[0, :, :3] = [[FQ.LO, 0, 0], [FQ.LO - 1, 1, 1], [0, FQ.HI, 0], [0, 0, FQ.HI + 1]]
    el, dark, bright, good = FQ.classes(f, None, FQ.LO, FQ.HI)
    assert dark.tolist() == [[False, True, False, False]] and bright.tolist() == [[False, False, False, True]]
    assert good.tolist() == [[True, False, True, False]]


@pytest.mark.parametrize("where", ["interior", "corner", "cell edge"])
def test_one_bright_pixel_removes_itself_and_its_four_neighbours(nm, where):
    fw, fh, grid = 40, 24, (2, 2)
    rng = np.random.default_rng(3)
    f = rng.integers(30, 200, (fh, fw, 4), dtype=np.uint8)
    x, y = dict(interior=(9, 7), corner=(0, 0), **{"cell edge": (20, 12)})[where]
    g = f.copy()
    g[y, x, :3] = 255
    a, b = host_stats(nm, [f], None, 0, 250, grid)[0], host_stats(nm, [g], None, 0, 250, grid)[0]
    assert np.array_equal(b, FQ.stats_model([g], None, 0, 250, grid)[0])
    lost = [(x + dx, y + dy) for dx, dy in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1))
            if 1 <= x + dx < fw - 1 and 1 <= y + dy < fh - 1]
    want = a[..., 0].astype(np.int64).copy()
    for px, py in lost:
        want[py * 2 // fh, px * 2 // fw] -= 1
    assert np.array_equal(b[..., 0].astype(np.int64), want) and b[..., 6].sum() == 1 and a[..., 6].sum() == 0
    assert len(lost) == {"interior": 5, "corner": 0, "cell edge": 5}[where]
    if where == "cell edge":
        assert (a[..., 0] != b[..., 0]).sum() >= 3                  # the five pixels lie in several cells


def test_extreme_frames(nm):
    fw, fh = 70, 33
    y, x = np.mgrid[0:fh, 0:fw]
    dark = np.zeros((fh, fw, 4), np.uint8)
    bright = np.full((fh, fw, 4), 255, np.uint8)
    checker = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 4, -1)
    diag = np.repeat(((((x + y) % 4) < 2) * 255).astype(np.uint8)[..., None], 4, -1)
    for grid in ((1, 1), (3, 2)):
        got = host_stats(nm, [dark, bright, checker, diag], None, 1, 254, grid)
        assert np.array_equal(got, FQ.stats_model([dark, bright, checker, diag], None, 1, 254, grid))
        assert not got[:2, ..., :5].any() and got[0, ..., 5].sum() == fw * fh and got[1, ..., 6].sum() == fw * fh
        full = host_stats(nm, [checker, diag], None, 0, 255, grid)
        assert np.array_equal(full, FQ.stats_model([checker, diag], None, 0, 255, grid))
        inner = (fw - 2) * (fh - 2)
        assert full[..., 0].sum(axis=(1, 2)).tolist() == [inner, inner]
        assert full[0, ..., 3].sum() == inner * 1040400 and full[0, ..., 4].sum() == 0          # the Laplacian's maximum
        assert full[1, ..., 4].sum() == inner * 130050                                           # the gradient's maximum


def test_a_frames_words_depend_on_the_frame_alone(nm):
    base = FQ.frames_for(33, 17)
    order = [2, 0, 1, 0, 2, 2]
    masks = FQ.masks_for(33, 17, FQ.U8N)
    one = [host_stats(nm, [base[k]], [masks[k]], FQ.LO, FQ.HI, (4, 3))[0] for k in range(3)]
    got = host_stats(nm, [base[k] for k in order], [masks[k] for k in order], FQ.LO, FQ.HI, (4, 3))
    for slot, k in enumerate(order):
        assert np.array_equal(got[slot], one[k])
    many = nm.frame_quality_host([base[k % 3] for k in range(64)], masks=[masks[k % 3] for k in range(64)], lo=FQ.LO, hi=FQ.HI,
                                 grid=(4, 3), stats=np.full((64, 3, 4, 8), 0xDEADBEEFCAFE, np.uint64))
    for k in range(64):
        assert np.array_equal(many[k], one[k % 3])


# ---- the choice ---------------------------------------------------------------------------------------------------------------
CASES = FQ.pick_cases()


def host_pick(nm, case):
    stats, chain, fw, fh, keep, status, kw = case
    return nm.keyframe_pick_host(stats, chain, fw, fh, keep, frame_status=status, **kw)


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_pick_equals_the_model(nm, name):
    stats, chain, fw, fh, keep, status, kw = CASES[name]
    FQ.same_pick(host_pick(nm, CASES[name]), FQ.pick_model(stats, chain, fw, fh, keep, status, **kw))


def test_pick_cases_do_what_their_names_say(nm):
    r = {name: host_pick(nm, CASES[name]) for name in CASES}
    keys = lambda name: r[name].keys[:r[name].key_count[0]].tolist()
    assert keys("identity chains") == [0] and r["identity chains"].key_count.tolist() == [1, 0]
    # scores 10 11 12 50 14 13 60 15 16 17 70 5 on a pan of 1 px per frame
    assert keys("d_min hit") == [0, 10] and keys("d_min one below") == [0, 10] and keys("d_min one above") == [0, 10]
    assert keys("d_max hit") == [0, 3, 6, 9, 10, 11] and keys("d_max one above")[:3] == [0, 3, 6]
    assert keys("d_max one below") == [0, 2, 3, 4, 6, 8, 10, 11] and r["d_max one below"].key_count[1] == 0
    assert keys("both hit") == [0, 3, 6, 9] and not (r["both hit"].flags & FQ.JUMP).any()
    assert keys("a tie takes the lower index") == [0, 1, 2, 3, 5, 6, 7, 8] and r["a tie takes the lower index"].key_count[1] == 1
    b = r["carry on a broken row 0"]
    assert keys("carry on a broken row 0")[:2] == [0, 1] and b.flags[1] & FQ.JUMP and b.H_status[0] == 0 and not b.H_keys[0].any()
    assert b.flags[0] & FQ.STATUS and b.flags[0] & FQ.KEY and b.H_status[1] == 1
    assert keys("a broken row without carry")[0] == 1
    z = r["a non-positive denominator"]
    k = keys("a non-positive denominator")
    assert 4 in k and z.flags[4] & FQ.JUMP and z.H_status[k.index(4) - 1] == 0 and not z.H_keys[k.index(4) - 1].any()
    g = r["a negative denominator"]
    assert g.flags[5] & FQ.JUMP
    assert keys("carry with an unusable frame 0")[0] == 0 and keys("no carry with an unusable frame 0")[0] == 1
    assert r["keep reached with a follower"].key_count.tolist() == [3, 1]
    assert r["keep reached without a follower"].key_count.tolist() == [3, 0] and keys("keep reached without a follower") == [0, 3, 6]
    assert r["keep of one"].key_count.tolist() == [1, 1] and r["keep of one"].H_keys.shape == (0, 9)
    e = r["rel at the exact product"]
    assert [bool(f & FQ.BLURRED) for f in e.flags] == [s == 31 for s in (64, 32, 31, 64, 32, 31, 64, 31, 32, 64, 31, 32)]
    assert not (r["w of zero"].flags & FQ.BLURRED).any()
    assert (r["every cell below cell_min"].flags & FQ.FEW).all() and r["every cell below cell_min"].key_count[0] == 0
    assert (r["every cell below cell_min"].keys == -1).all() and not r["every cell below cell_min"].key_status.any()
    assert (r["too few pixels in all"].flags & FQ.FEW).all() and not (r["just enough pixels in all"].flags & FQ.FEW).any()
    assert not (r["bad fraction at the bound"].flags & FQ.BAD).any() and (r["bad fraction above the bound"].flags & FQ.BAD).all()
    assert r["64 frames on 8 x 8 cells"].key_count[0] > 8 and r["64 frames, a keep of 5"].key_count.tolist() == [5, 1]
    n = r["rows that are not finite"]
    assert n.flags[3] & FQ.STATUS and n.flags[6] & FQ.STATUS and 3 not in keys("rows that are not finite")
    s, want = FQ.median_check()
    got = nm.keyframe_pick_host(s, FQ.translation(0)[None], 64, 48, 1)
    assert got.scores[0, 0] == want
    one = nm.keyframe_pick_host(FQ.flat_stats([0]) + np.array([0, 0, 0, 12345, 0, 0, 0, 0], np.uint64), FQ.translation(0)[None], 64, 48, 1)
    assert one.scores[0, 0] == 12345 / 5000                         # gx = gy = 1: the mean squared Laplacian


# ---- the gather ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1, 15, 16, 17, 4 * 33 * 17])
def test_host_gather(nm, size):
    rng = np.random.default_rng(size)
    n = 5
    keys = np.array([3, -1, n, 3, 0, 4, 1 << 30, -(1 << 31)], np.int32)
    for offset in (0, 1):
        pool = rng.integers(0, 256, (n, size + 64), dtype=np.uint8)
        src = [pool[k, offset:offset + size] for k in range(n)]
        out = np.full((len(keys), size + 64), 0xA5, np.uint8)
        dst = [out[i, 16 + offset:16 + offset + size] for i in range(len(keys))]
        got = nm.slots_gather_host(keys, src, dst=dst, fill=0x3C)
        want = FQ.gather_model(keys, src, 0x3C)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
        assert (out[:, :16 + offset] == 0xA5).all() and (out[:, 16 + offset + size:] == 0xA5).all()
    frames = FQ.frames_for(33, 17)
    got = nm.slots_gather_host(np.array([2, 2, -1, 0], np.int32), frames)
    assert np.array_equal(np.stack(got), FQ.gather_model([2, 2, -1, 0], frames, 0))


# ---- refusals -----------------------------------------------------------------------------------------------------------------
PTR = 4096                                                          # a pointer that is never dereferenced


def table(n, null_at=None):
    return (C.c_void_p * max(n, 1))(*[None if k == null_at else PTR for k in range(max(n, 1))])


def quality_args(**kw):
    a = dict(n=2, frames=table(2), fw=8, fh=6, masks=None, fmt=FQ.U8N, lo=0, hi=255, gx=2, gy=2, stats=PTR)
    a.update(kw)
    return [a[k] for k in ("n", "frames", "fw", "fh", "masks", "fmt", "lo", "hi", "gx", "gy", "stats")]


QUALITY_REFUSALS = dict(
    n_zero=dict(n=0), n_65=dict(n=65, frames=table(65)), fw_zero=dict(fw=0), fw_big=dict(fw=32768), fh_zero=dict(fh=0),
    fh_big=dict(fh=32768), lo_neg=dict(lo=-1), lo_big=dict(lo=256), hi_neg=dict(hi=-1), hi_big=dict(hi=256), gx_zero=dict(gx=0),
    gx_9=dict(gx=9, fw=100), gx_above_fw=dict(gx=4, fw=3), gy_zero=dict(gy=0), gy_9=dict(gy=9, fh=100), gy_above_fh=dict(gy=7),
    bad_format=dict(masks=table(2), fmt=1), null_frames=dict(frames=None), null_stats=dict(stats=None),
    null_frame=dict(frames=table(2, 1)), null_mask=dict(masks=table(2, 0)))


def pick_args(**kw):
    a = dict(n=4, stats=PTR, gx=2, gy=2, chain=PTR, status=None, fw=64, fh=48, keep=3, cell_min=64, min_pixels=10, max_bad=0.25,
             rel=0.5, w=2, d_min=1.0, d_max=2.0, carry=0, keys=PTR, key_count=PTR)
    a.update(kw)
    return [a[k] for k in ("n", "stats", "gx", "gy", "chain", "status", "fw", "fh", "keep", "cell_min", "min_pixels", "max_bad", "rel",
                           "w", "d_min", "d_max", "carry", "keys", "key_count")] + [None] * 5


PICK_REFUSALS = dict(
    n_zero=dict(n=0), n_65=dict(n=65), gx_zero=dict(gx=0), gx_9=dict(gx=9), gy_zero=dict(gy=0), gy_9=dict(gy=9), fw_zero=dict(fw=0),
    fh_big=dict(fh=32768), keep_zero=dict(keep=0), keep_65=dict(keep=65), cell_min_zero=dict(cell_min=0), min_pixels_neg=dict(min_pixels=-1),
    max_bad_neg=dict(max_bad=-0.01), max_bad_big=dict(max_bad=1.01), max_bad_nan=dict(max_bad=float("nan")), rel_neg=dict(rel=-0.1),
    rel_big=dict(rel=1.5), rel_nan=dict(rel=float("nan")), w_neg=dict(w=-1), w_9=dict(w=9), d_order=dict(d_min=3.0, d_max=2.0),
    d_min_neg=dict(d_min=-1.0), d_min_nan=dict(d_min=float("nan")), d_max_inf=dict(d_max=float("inf")), d_max_nan=dict(d_max=float("nan")),
    null_stats=dict(stats=None), null_chain=dict(chain=None), null_keys=dict(keys=None), null_key_count=dict(key_count=None))


def gather_args(**kw):
    a = dict(n=3, src=table(3), keep=2, dst=table(2), keys=PTR, bytes=16, fill=0)
    a.update(kw)
    return [a[k] for k in ("n", "src", "keep", "dst", "keys", "bytes", "fill")]


GATHER_REFUSALS = dict(
    n_zero=dict(n=0), n_65=dict(n=65, src=table(65)), keep_zero=dict(keep=0), keep_65=dict(keep=65, dst=table(65)), bytes_zero=dict(bytes=0),
    bytes_neg=dict(bytes=-16), bytes_2g=dict(bytes=1 << 31), null_src=dict(src=None), null_dst=dict(dst=None), null_keys=dict(keys=None),
    null_src_entry=dict(src=table(3, 2)), null_dst_entry=dict(dst=table(2, 0)))


def test_the_c_entries_refuse_before_touching_anything(nm):
    """all six entries; PTR would fault if it were read or written, and the device entries would need a device"""
    lib = nm.lib()
    for make, refusals, names in ((quality_args, QUALITY_REFUSALS, ("nm_frame_quality_batch_dev", "nm_frame_quality_host")),
                                  (pick_args, PICK_REFUSALS, ("nm_keyframe_pick_dev", "nm_keyframe_pick_host")),
                                  (gather_args, GATHER_REFUSALS, ("nm_slots_gather_dev", "nm_slots_gather_host"))):
        for case, change in refusals.items():
            for name in names:
                args = make(**change) + ([None] if name.endswith("_dev") else [])
                assert getattr(lib, name)(*args) == 1, (name, case)          # hipErrorInvalidValue


def test_the_host_twins_leave_outputs_untouched_when_they_refuse(nm):
    lib = nm.lib()
    frames = FQ.frames_for(8, 6, n=2)
    stats = np.full((2, 2, 2, 8), 0xA5A5, np.uint64)
    ft = (C.c_void_p * 2)(*[f.ctypes.data for f in frames])
    for change in (dict(lo=256), dict(gy=7), dict(n=0), dict(masks=table(2, 1))):
        assert lib.nm_frame_quality_host(*quality_args(frames=ft, stats=stats.ctypes.data, **change)) == 1
        assert (stats == 0xA5A5).all()
    assert lib.nm_frame_quality_host(*quality_args(frames=ft, stats=stats.ctypes.data)) == 0 and not (stats == 0xA5A5).any()
    s, chain = FQ.flat_stats([1, 2, 3, 4], gx=2, gy=2), np.stack([FQ.translation(-k) for k in range(4)])
    keys, count = np.full(3, 77, np.int32), np.full(2, 77, np.int32)
    for change in (dict(d_min=3.0), dict(keep=65), dict(rel=2.0), dict(w=9)):
        args = pick_args(stats=s.ctypes.data, chain=chain.ctypes.data, keys=keys.ctypes.data, key_count=count.ctypes.data, **change)
        assert lib.nm_keyframe_pick_host(*args) == 1 and (keys == 77).all() and (count == 77).all()
    src, dst = np.arange(48, dtype=np.uint8).reshape(3, 16), np.full((2, 16), 0xA5, np.uint8)
    k = np.array([1, 2], np.int32)
    tab = lambda a: (C.c_void_p * len(a))(*[r.ctypes.data for r in a])
    for change in (dict(bytes=0), dict(n=0), dict(keep=65), dict(src=table(3, 1))):
        args = gather_args(**dict(dict(src=tab(src), dst=tab(dst), keys=k.ctypes.data), **change))
        assert lib.nm_slots_gather_host(*args) == 1 and (dst == 0xA5).all()


def test_the_wrappers_refuse_with_nmerror_before_any_library_call(nm, monkeypatch):
    frames = FQ.frames_for(8, 6, n=2)
    s, chain = FQ.flat_stats([1, 2, 3, 4], gx=2, gy=2), np.stack([FQ.translation(-k) for k in range(4)])
    keys = np.array([1, 0], np.int32)
    calls = [
        lambda: nm.frame_quality_host([]), lambda: nm.frame_quality_host(frames * 33), lambda: nm.frame_quality_host(frames, lo=-1),
        lambda: nm.frame_quality_host(frames, hi=256), lambda: nm.frame_quality_host(frames, lo=1.5), lambda: nm.frame_quality_host(frames, grid=(9, 1)),
        lambda: nm.frame_quality_host(frames, grid=(1, 7)), lambda: nm.frame_quality_host(frames, grid=(0, 1)),
        lambda: nm.frame_quality_host(frames, masks=[np.ones((6, 8), np.uint8)]),
        lambda: nm.frame_quality_host(frames, masks=np.ones((6, 9), np.uint8)),
        lambda: nm.frame_quality_host(frames, masks=np.ones((6, 8), np.int16)),
        lambda: nm.frame_quality_host(frames, masks=[np.ones((6, 8), np.uint8), np.ones((6, 8), F32)]),
        lambda: nm.frame_quality_host(frames, stats=np.zeros((2, 4, 4, 7), np.uint64)),
        lambda: nm.frame_quality_host([frames[0], frames[1][:, :7]]), lambda: nm.frame_quality_host([f[..., :3] for f in frames]),
        lambda: nm.keyframe_pick_host(s, chain, 64, 48, 0), lambda: nm.keyframe_pick_host(s, chain, 64, 48, 65),
        lambda: nm.keyframe_pick_host(s, chain[:3], 64, 48, 2), lambda: nm.keyframe_pick_host(s, chain, 0, 48, 2),
        lambda: nm.keyframe_pick_host(s, chain, 64, 32768, 2), lambda: nm.keyframe_pick_host(s, chain, 64, 48, 2, rel=1.1),
        lambda: nm.keyframe_pick_host(s, chain, 64, 48, 2, max_bad=-0.1), lambda: nm.keyframe_pick_host(s, chain, 64, 48, 2, w=9),
        lambda: nm.keyframe_pick_host(s, chain, 64, 48, 2, d_min=5, d_max=4), lambda: nm.keyframe_pick_host(s, chain, 64, 48, 2, d_max=float("inf")),
        lambda: nm.keyframe_pick_host(s, chain, 64, 48, 2, cell_min=0), lambda: nm.keyframe_pick_host(s, chain, 64, 48, 2, min_pixels=-1),
        lambda: nm.keyframe_pick_host(s[..., :7], chain, 64, 48, 2), lambda: nm.keyframe_pick_host(s.astype(np.float64), chain, 64, 48, 2),
        lambda: nm.keyframe_pick_host(s, chain, 64, 48, 2, frame_status=np.ones(3, np.int32)),
        lambda: nm.slots_gather_host(keys, []), lambda: nm.slots_gather_host(keys, frames * 33),
        lambda: nm.slots_gather_host(np.zeros(65, np.int32), frames), lambda: nm.slots_gather_host(keys, [frames[0], frames[1][:5]]),
        lambda: nm.slots_gather_host(keys, frames, dst=[np.zeros_like(frames[0])]), lambda: nm.slots_gather_host(keys, frames, fill=256),
        lambda: nm.slots_gather_host(keys, frames, dst=[np.zeros((6, 8, 4), np.int8)] * 2),
    ]
    assert nm.keyframe_pick_host(s, chain, 64, 48, 2).key_count[0] >= 1 and len(nm.slots_gather_host(keys, frames)) == 2
    monkeypatch.setattr(nm, "lib", lambda: (_ for _ in ()).throw(AssertionError("a refused input reached the library")))
    for i, call in enumerate(calls):
        with pytest.raises(nm.NmError):
            call()
    for name in ("nm_frame_quality_batch_dev", "nm_frame_quality_host", "nm_frame_quality_set_grid_cap", "nm_keyframe_pick_dev",
                 "nm_keyframe_pick_host", "nm_slots_gather_dev", "nm_slots_gather_host"):
        assert name in nm.ABI_SYMBOLS
    assert (nm.FRAME_QUALITY_MAX_BATCH, nm.FRAME_QUALITY_MAX_GRID) == (64, 8)
    assert (nm.KEYFRAME_STATUS, nm.KEYFRAME_FEW, nm.KEYFRAME_BAD, nm.KEYFRAME_BLURRED, nm.KEYFRAME_KEY, nm.KEYFRAME_JUMP) == \
        (FQ.STATUS, FQ.FEW, FQ.BAD, FQ.BLURRED, FQ.KEY, FQ.JUMP)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_end_to_end_the_choice_avoids_every_blurred_view(nm):
    """48 views of the loop-closure scene along a pan, every third blurred with a 5-tap horizontal box, one sharp view with a
    painted saturated block; the true maps as the chain. Model and host twin agree, and on both: no key is a blurred view,
    the painted view is flagged and not a key, consecutive keys are d_min .. d_max apart, at least 8 keys, and H_keys agrees
    with the true relative maps to 1e-3 px at the corners."""
    import loop_closure_ref as LC
    e = FQ.e2e()
    want = FQ.pick_model(e["stats_model"], e["chain"], LC.VW, LC.VH, FQ.E2E_KEEP, None, **FQ.E2E_PICK)
    stats = nm.frame_quality_host(e["views"], **FQ.E2E_QUALITY)
    assert np.array_equal(stats, e["stats_model"])
    got = nm.keyframe_pick_host(stats, e["chain"], LC.VW, LC.VH, FQ.E2E_KEEP, **FQ.E2E_PICK)
    FQ.same_pick(got, want)
    FQ.e2e_conditions(got._asdict(), e)
    frames = nm.slots_gather_host(got.keys, e["views"])
    for i, k in enumerate(got.keys):
        assert np.array_equal(frames[i], e["views"][k] if k >= 0 else np.zeros_like(e["views"][0]))
