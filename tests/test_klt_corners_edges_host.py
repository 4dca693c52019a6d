"""The host twin of the corner detector (nm_klt_corners_host_f32) against the Python model, exactly, on the inputs of
tests/klt_corners_edges_ref.py, and the assertion per input, made on the model alone, that it reaches what it is built for:
two to 32 scan trips of flag words with corners in every trip that can hold one, caps at the trip boundaries, Gxy beyond
2^31 of both signs at corners, exact ties of every kind on either side of both tile seams, the exact footprint of a pixel
without a level, and more than 256 held rows a launch. tests/test_gpu_klt_corners_edges.py holds the device against this
host twin on the same inputs."""
import numpy as np
import pytest

import klt_corners_edges_ref as E
import klt_corners_ref as R

F32 = np.float32


def host(nm, c, cap=None, want_plane=True):
    held = None
    if c["held"] is not None:
        held = ([h[0] for h in c["held"]], [h[1] for h in c["held"]], [h[2] for h in c["held"]])
    return nm.klt_corners_host(c["grays"], radius=c["r"], nms=c["nms"], min_eig=c["min_eig"], cap=c["cap"] if cap is None else cap,
                               mask=c["mask"], held=held, want_score_plane=want_plane, fill=-7)


def host_equals_model(nm, c):
    got, want = host(nm, c), R.model_case(c)
    for k, m in enumerate(want):
        assert m["total"] <= c["cap"]
        R.assert_equal(got, m, k, c["name"])
    return got, want


# ---- A ----
@pytest.mark.parametrize("name", list(E.TRIP_FRAMES))
def test_trip_frames(nm, name):
    E.assert_trip_frame(name)
    got = host(nm, E.trip_case(name))
    R.assert_equal(got, E.trip_model(name), 0, name)


@pytest.mark.parametrize("name", ["trips_64x2100", "trips_130x800"])
def test_caps_at_the_trip_boundaries(nm, name):
    caps, c1, c2, total = E.trip_caps(name)
    assert caps == sorted(set(caps)) and len(caps) == 8
    for cap in caps:
        got = host(nm, E.trip_case(name), cap=cap, want_plane=False)
        R.assert_equal(got, E.cut(E.trip_model(name), cap), 0, (name, cap))
        assert (got["x"][0][min(cap, total):] == -7).all()


def test_three_multi_trip_frames(nm):
    host_equals_model(nm, E.back_to_back_case())


def test_the_widest_frame_with_held_points(nm):
    host_equals_model(nm, E.wide_held_case())


# ---- B ----
@pytest.mark.parametrize("h", [70, 4 * 16 + 1, 4 * 16 + 15])
def test_gxy_beyond_32_bits_signed(nm, h):
    c = E.gxy_case(h)
    E.assert_gxy_case(c)
    host_equals_model(nm, c)


# ---- C ----
TIES = E.tie_cases()


@pytest.mark.parametrize("c,kinds,straddle", TIES, ids=[t[0]["name"] for t in TIES])
def test_exact_ties(nm, c, kinds, straddle):
    E.assert_tie_case(c, kinds, straddle)
    host_equals_model(nm, c)


# ---- D ----
@pytest.mark.parametrize("r", [1, 3, 7])
def test_the_footprint_of_a_pixel_without_a_level(nm, r):
    c, masked, groups = E.foot_cases(r)
    clean = R.score_plane(E.foot_clean(), r, 0.0)
    flipped = R.score_plane(E.foot_clean()[::-1].copy(), r, 0.0)
    got, want = host_equals_model(nm, c)
    reached = np.zeros(clean.shape, bool)
    for k, m in enumerate(want):
        foot, was = E.assert_footprint(m["plane"], clean, groups[k], r)
        reached |= foot & was
    for k, cm in enumerate(masked):
        got, want = host_equals_model(nm, cm)
        E.assert_footprint(want[0]["plane"], clean, groups[k], r)
        E.assert_footprint(want[1]["plane"], flipped, groups[k], r)
    # every column of the 88-bit word's split and both seams has a pixel that only a bad pixel's footprint unscores
    assert all(reached[:, x].any() for x in (52 - (r + 2), 52, 52 + r + 1, 63, 64, 116 - (r + 2), 116 + r + 1))


# ---- E ----
@pytest.mark.parametrize("w,h", [(128, 40), (130, 70)])
def test_a_mask_with_three_frames(nm, w, h):
    c = E.mask_case(w, h)
    got, want = host_equals_model(nm, c)
    free = R.model_case(dict(c, mask=None))
    assert all(not np.array_equal(a["plane"], b["plane"]) for a, b in zip(want, free))


def test_held_points_in_bulk(nm):
    c, want = E.bulk_held_case()
    ms = R.model_case(c)
    E.assert_bulk_held([m["x"] for m in ms], [m["y"] for m in ms], [m["count"] for m in ms], [m["total"] for m in ms], want)
    got, _ = host_equals_model(nm, c)
    E.assert_bulk_held(got["x"], got["y"], got["count"], got["total"], want)
