"""The host twin of the keypoint selection (nm_sift_select_host) against the independent model of select_ref.py: the
selected rows and every gathered byte, the properties that follow from the rule, the default score against the float32
butterfly model and the float64 sum of desc_finish_ref's step 1, and every refusal with untouched outputs. No GPU.
"""
import ctypes as C

import numpy as np
import pytest

import desc_finish_ref
import select_ref as R

PAYLOAD = ("x", "y", "desc", "desc_u8", "kpts", "orients")
FILL = 77


def frame(seed, cap, width, height, levels=None):
    rng = np.random.default_rng(seed)
    f = dict(x=(rng.random(cap) * (width + 6) - 3).astype(np.float32), y=(rng.random(cap) * (height + 6) - 3).astype(np.float32))
    f["scores"] = rng.random(cap).astype(np.float32) if levels is None else rng.integers(0, levels, cap).astype(np.float32)
    f["desc"] = rng.integers(0, 40, (cap, 128)).astype(np.float32) * np.float32(0.37)
    f["desc_u8"] = rng.integers(0, 256, (cap, 128)).astype(np.uint8)
    f["kpts"] = rng.random((cap, 4)).astype(np.float32)
    f["orients"] = rng.random((cap, 2)).astype(np.float32)
    return f


def check(nm, f, count, cap, width, height, gx, gy, keep, by_desc=False):
    """Host twin against the model for one frame; returns (chosen rows, model internals)."""
    scores = R.default_scores(f["desc"][:cap]) if by_desc else f["scores"][:cap]
    chosen, info = R.select(count, cap, f["x"], f["y"], scores, width, height, gx, gy, keep)
    out = nm.sift_select_host([count], [f["x"][:cap]], [f["y"][:cap]], width, height, scores=None if by_desc else [scores],
                              descs=[f["desc"][:cap]], descs_u8=[f["desc_u8"][:cap]], kpts=[f["kpts"][:cap]],
                              orients=[f["orients"][:cap]], gx=gx, gy=gy, keep=keep, capacity=cap, fill=FILL)
    c = chosen.size
    assert out["count"][0] == c == min(keep, min(max(count, 0), cap))
    assert np.array_equal(out["index"][0][:c], chosen), (count, keep, gx, gy)
    assert (out["index"][0][c:] == FILL).all()
    for k in PAYLOAD:
        assert np.array_equal(out[k][0][:c].view(np.uint8), f[k][chosen].view(np.uint8)), k
        assert (out[k][0][c:] == FILL).all(), (k, "rows beyond the count")
    R.check_properties(chosen, info, keep)
    return chosen, info


@pytest.mark.parametrize("levels", [None, 8])
def test_random_and_tied_scores(nm, levels):
    cap = 700
    for seed, (w, h, gx, gy), keep in ((1, (301, 200, 16, 9), 150), (2, (10, 7, 4, 3), 64), (3, (1920, 1080, 16, 9), 699),
                                       (4, (64, 64, 64, 64), 300)):
        check(nm, frame(seed, cap, w, h, levels), cap, cap, w, h, gx, gy, keep)


def test_widths_not_divisible_by_the_grid(nm):
    """10 / 4: cw = 3, so column 3 holds pixel 9 alone; 301 / 16: cw = 19, the last column is 16 pixels wide."""
    assert R.cells(np.float32([0, 2.9, 3, 8.99, 9, 9.99, 10, 1e9]), np.zeros(8, np.float32), 10, 7, 4, 3).tolist() == [0, 0, 1, 2, 3, 3, 3, 3]
    assert R.cells(np.float32([284.9, 285, 300.5]), np.float32([0, 0, 199.5]), 301, 200, 16, 9).tolist() == [14, 15, 8 * 16 + 15]
    f = frame(5, 400, 10, 7)
    check(nm, f, 400, 400, 10, 7, 4, 3, 100)
    check(nm, frame(6, 400, 301, 200), 400, 400, 301, 200, 16, 9, 100)


def test_one_cell_is_top_n_and_one_by_one_grid_is_argsort(nm):
    f = frame(7, 500, 320, 240)
    f["x"][:] = 5.5
    f["y"][:] = 3.25
    chosen, info = check(nm, f, 500, 500, 320, 240, 16, 9, 77)
    assert (info["cell"] == 0).all()
    g = frame(8, 500, 320, 240, levels=8)
    for keep in (1, 100, 499):
        chosen, _ = check(nm, g, 500, 500, 320, 240, 1, 1, keep)
        top = np.argsort(-g["scores"].astype(np.float64), kind="stable")[:keep]      # stable: the earlier row wins a tie
        assert np.array_equal(chosen, np.sort(top))


def test_counts_identity_empty_single_clipped_and_negative(nm):
    cap = 120
    f = frame(9, cap + 10, 160, 120)
    for count, keep in ((cap, cap), (50, 50), (50, cap), (0, 10), (1, 1), (1, 10), (cap + 7, 30), (cap + 7, cap), (-1, 5), (-9, cap)):
        chosen, _ = check(nm, f, count, cap, 160, 120, 4, 4, keep)
        m = min(max(count, 0), cap)
        if keep >= m:
            assert np.array_equal(chosen, np.arange(m)), "keep >= m is the identity"


def test_unusable_scores_rank_last_and_odd_coordinates_land_in_edge_cells(nm):
    cap = 300
    f = frame(10, cap, 320, 240)
    f["scores"][::7] = np.nan
    f["scores"][1::7] = -1.0
    f["scores"][2::7] = np.inf
    f["scores"][3::7] = 0.0
    f["scores"][4::7] = -np.inf
    f["x"][::5] = np.nan
    f["y"][1::5] = np.nan
    f["x"][2::5] = -1e30
    f["y"][3::5] = 1e30
    f["x"][4::5] = 320.0
    for gx, gy, keep in ((16, 9, 100), (1, 1, 150), (2, 2, 299)):
        chosen, info = check(nm, f, cap, cap, 320, 240, gx, gy, keep)
    bad = info["u"] == 0
    assert bad.sum() == np.isin(np.arange(cap) % 7, (0, 1, 2, 3, 4)).sum()
    chosen, info = check(nm, f, cap, cap, 320, 240, 1, 1, int((~bad).sum()))
    assert not bad[chosen].any(), "an unusable score was taken before a usable one"
    assert R.cells(np.float32([np.nan, -5, 320, 1e30]), np.float32([np.nan, 1e30, -1, 3]), 320, 240, 16, 9).tolist() == [0, 8 * 16, 15, 15]


def test_default_score_on_real_descriptors_and_zero_rows(nm, oracle):
    import helpers as H
    refs = [oracle.sift_detect_describe(H.blob_field(seed, 320, 240).astype(np.float32), 4096) for seed in (3, 4, 5, 6)]
    ref = {k: np.concatenate([r[k] for r in refs]) for k in ("desc", "x", "y")}      # a frame has some 15 keypoints
    n = ref["desc"].shape[0]
    assert n >= 20
    desc = np.concatenate([ref["desc"], np.zeros((5, 128), np.float32), ref["desc"][:3]]).astype(np.float32)
    m = desc.shape[0]
    rng = np.random.default_rng(0)
    f = dict(x=np.concatenate([ref["x"], rng.random(8).astype(np.float32) * 320]).astype(np.float32),
             y=np.concatenate([ref["y"], rng.random(8).astype(np.float32) * 240]).astype(np.float32), desc=desc,
             desc_u8=rng.integers(0, 256, (m, 128)).astype(np.uint8), kpts=rng.random((m, 4)).astype(np.float32),
             orients=rng.random((m, 2)).astype(np.float32))
    # the float32 model of the score against the float64 sum of the finish model's step 1, to that model's 8 u
    s32 = R.default_scores(desc).astype(np.float64)
    v = desc.astype(np.float64)
    s64 = (v * v).sum(1)
    assert (np.abs(s32 - s64) <= 8 * desc_finish_ref.U * s64).all() and (s32[n:n + 5] == 0).all() and (s32[:n] > 0).all()
    for gx, gy, keep in ((4, 3, n // 2), (1, 1, n), (16, 9, m - 1), (1, 1, m)):
        chosen, info = check(nm, f, m, m, 320, 240, gx, gy, keep, by_desc=True)
    # the twin's own scores, observed through a 1 x 1 grid: bit-identical to the model's when fed back as scores
    by_desc = nm.sift_select_host([m], [f["x"]], [f["y"]], 320, 240, descs=[desc], gx=1, gy=1, keep=n)
    by_score = nm.sift_select_host([m], [f["x"]], [f["y"]], 320, 240, scores=[R.default_scores(desc)], descs=[desc], gx=1, gy=1, keep=n)
    assert np.array_equal(by_desc["index"], by_score["index"])
    assert not np.isin(np.arange(n, n + 5), by_desc["index"][0][:n]).any(), "a row of zeros was taken before a live row"


def test_batches_are_frame_by_frame(nm):
    cap = 200
    frames = [frame(20 + k, cap, 301, 200, levels=4 if k % 2 else None) for k in range(64)]
    counts = [cap - 3 * k for k in range(64)]
    col = lambda k: [f[k] for f in frames]
    out = nm.sift_select_host(counts, col("x"), col("y"), 301, 200, scores=col("scores"), kpts=col("kpts"), gx=7, gy=5, keep=60)
    for k in (0, 1, 31, 63):
        chosen, _ = R.select(counts[k], cap, frames[k]["x"], frames[k]["y"], frames[k]["scores"], 301, 200, 7, 5, 60)
        assert np.array_equal(out["index"][k][:chosen.size], chosen) and out["count"][k] == chosen.size
        assert np.array_equal(out["kpts"][k][:chosen.size], frames[k]["kpts"][chosen])


def test_refusals_touch_nothing(nm):
    lib = nm.lib()
    cap = 16
    full = lambda shape, dt, v: np.full(shape, v, dt)
    src = dict(num=full((1,), np.int32, cap), x=full((cap,), np.float32, 1), y=full((cap,), np.float32, 1),
               scores=full((cap,), np.float32, 1), desc=full((cap, 128), np.float32, 1), desc_u8=full((cap, 128), np.uint8, 1),
               kpts=full((cap, 4), np.float32, 1), orients=full((cap, 2), np.float32, 1))
    dst = dict(out_x=full((cap,), np.float32, 7), out_y=full((cap,), np.float32, 7), out_desc=full((cap, 128), np.float32, 7),
               out_desc_u8=full((cap, 128), np.uint8, 7), out_kpts=full((cap, 4), np.float32, 7),
               out_orients=full((cap, 2), np.float32, 7), out_index=full((cap,), np.int32, 7), out_items=full((1,), np.int32, 7))
    tab = lambda a, k=2: (C.c_void_p * 64)(*([a.ctypes.data] * k))
    order = ("num", "x", "y", "scores", "desc", "desc_u8", "kpts", "orients", "out_x", "out_y", "out_desc", "out_desc_u8",
             "out_kpts", "out_orients", "out_index", "out_items")

    def call(n=2, cap_=cap, w=64, h=48, gx=4, gy=4, keep=8, **kw):
        a = {k: tab(src[k] if k in src else dst[k]) for k in order}
        a.update(kw)
        return lib.nm_sift_select_host(n, cap_, w, h, gx, gy, keep, *[a[k] for k in order])

    bad = [dict(n=0), dict(n=65), dict(n=-1), dict(cap_=0), dict(cap_=65537), dict(gx=0), dict(gx=65), dict(gy=0), dict(gy=65),
           dict(keep=0), dict(keep=cap + 1), dict(w=0), dict(h=0), dict(h=-3), dict(num=None), dict(x=None), dict(y=None),
           dict(out_x=None), dict(out_y=None), dict(out_items=None), dict(scores=None, desc=None, out_desc=None),
           dict(out_desc=None), dict(desc=None), dict(out_desc_u8=None), dict(desc_u8=None), dict(out_kpts=None), dict(kpts=None),
           dict(out_orients=None), dict(orients=None), dict(out_x=tab(src["x"])), dict(out_y=tab(src["y"])),
           dict(out_desc=tab(src["desc"])), dict(out_desc_u8=tab(src["desc_u8"])), dict(out_kpts=tab(src["kpts"])),
           dict(out_orients=tab(src["orients"]))]
    bad += [{k: tab(src[k] if k in src else dst[k], 1)} for k in order]
    for kw in bad:
        assert call(**kw) == 1, kw                                   # hipErrorInvalidValue
    for v in dst.values():
        assert (v == 7).all()
    assert call(out_index=None) == 0 and (dst["out_index"] == 7).all() and dst["out_items"][0] == 8
    assert call(scores=None) == 0 and call(n=1, keep=cap, cap_=cap) == 0
    assert dst["out_index"].tolist() == list(range(cap)) and (dst["out_desc_u8"] == 1).all()
    ws = lib.nm_sift_select_workspace_bytes
    assert ws(1, 16, 4, 4) > 0 and ws(64, 65536, 64, 64) == 64 * ws(1, 65536, 1, 1)
    for args in ((0, 16, 4, 4), (65, 16, 4, 4), (1, 0, 4, 4), (1, 65537, 4, 4), (1, 16, 0, 4), (1, 16, 4, 65)):
        assert ws(*args) == 0, args
    for kw in (dict(keep=cap + 1), dict(gx=65), dict(gy=0), dict(scores=None), dict(kpts=[src["kpts"][:, :3]]), dict(capacity=cap + 1)):
        args = dict(scores=[src["scores"]], gx=4, gy=4, keep=8)
        args.update(kw)
        with pytest.raises(nm.NmError):
            nm.sift_select_host([cap], [src["x"]], [src["y"]], 64, 48, **args)


# nm_sift_select_workspace_bytes(n, capacity, gx, gy) as the release that introduced the selection returned it
WORKSPACE_BYTES = {(1, 1): 49376, (1, 7): 49488, (1, 1024): 68800, (1, 65536): 1294528,
                   (64, 1): 3160064, (64, 7): 3167232, (64, 1024): 4403200, (64, 65536): 82849792}


def test_workspace_bytes_are_the_recorded_values(nm):
    """The layout is stated once (key, skey, list, cstart, meta, pointer record, cell, flag; 16-byte stride); the byte count
    it yields stays what callers have allocated so far, for every grid."""
    ws = nm.lib().nm_sift_select_workspace_bytes
    for (n, cap), want in WORKSPACE_BYTES.items():
        for gx, gy in ((8, 8), (1, 1), (64, 64)):
            assert ws(n, cap, gx, gy) == want, (n, cap, gx, gy)
        assert want == n * ((cap * 19 + 4096 * 8 + (4096 + 8) * 4 + 8 * 4 + 128 + 15) // 16 * 16)
