"""The corner detector on the device (nm_klt_corners_batch_dev_f32) against its host twin, bit for bit (coordinates, score
bits, counts, totals and score planes), on the inputs of tests/klt_corners_edges_ref.py, which tests/test_klt_corners_edges_host.py
holds against the Python model and whose purposes it asserts: the emit kernel's second to 32nd scan trip and caps at the
trip boundaries, Gxy beyond 2^31 of both signs, exact ties across both tile seams, the footprint of a pixel without a
level at the 88-bit word's split, and the call shapes that no other test makes on the device: a mask with several frames,
the workspace's own score planes, planes of mixed alignment, aligned planes with an unaligned mask, held rows for more
than one workgroup and a striding mark launch, one workgroup emitting several multi-trip frames."""
import numpy as np
import pytest

import klt_corners_edges_ref as E
import klt_corners_ref as R
from test_gpu_klt_corners import _t, host_and_device, same, shifted

pytestmark = pytest.mark.gpu

F32 = np.float32


class grid_cap:
    def __init__(self, nm, cap):
        self.nm, self.cap = nm, cap

    def __enter__(self):
        self.prev = self.nm.klt_corners_set_grid_cap(self.cap)

    def __exit__(self, *exc):
        self.nm.klt_corners_set_grid_cap(self.prev)


def host_of(nm, c, want_plane=True):
    held = None
    if c["held"] is not None:
        held = ([h[0] for h in c["held"]], [h[1] for h in c["held"]], [h[2] for h in c["held"]])
    return nm.klt_corners_host(c["grays"], mask=c["mask"], held=held, radius=c["r"], nms=c["nms"], min_eig=c["min_eig"], cap=c["cap"],
                               want_score_plane=want_plane)


def device_of(nm, cuda, c, offsets, mask_offset=0, want_plane=True, workspace=None):
    """the device call with plane k `offsets[k]` floats, and the mask `mask_offset` bytes, into a fresh allocation"""
    grays = [shifted(g, cuda, o) for g, o in zip(c["grays"], offsets)]
    assert all(g.data_ptr() % 16 == (4 * o) % 16 for g, o in zip(grays, offsets))
    mask = None if c["mask"] is None else shifted(c["mask"], cuda, mask_offset)
    assert mask is None or mask.data_ptr() % 4 == mask_offset % 4
    held = None
    if c["held"] is not None:
        held = ([_t(h[0], cuda) for h in c["held"]], [_t(h[1], cuda) for h in c["held"]],
                [_t(np.array([h[2]], np.int32), cuda) for h in c["held"]])
    return nm.klt_corners_batch(grays, mask=mask, held=held, radius=c["r"], nms=c["nms"], min_eig=c["min_eig"], cap=c["cap"],
                                want_score_plane=want_plane, workspace=workspace)


# ---- A. scan trips ----
@pytest.mark.parametrize("name", list(E.TRIP_FRAMES))
def test_scan_trips(nm, cuda, name):
    c = E.trip_case(name)
    got, want = host_and_device(nm, cuda, c)
    same(got, want, name)
    assert int(want["total"][0]) == E.trip_model(name)["total"]


def test_the_widest_frame_with_held_points(nm, cuda):
    c = E.wide_held_case()
    same(*host_and_device(nm, cuda, c), c["name"])


@pytest.mark.parametrize("name", ["trips_64x2100", "trips_130x800"])
def test_caps_at_the_trip_boundaries(nm, cuda, name):
    import torch
    caps, c1, c2, total = E.trip_caps(name)
    for cap in caps:
        c = E.trip_case(name, cap=cap)
        junk = lambda v: [torch.full((cap + 3,), v, dtype=torch.float32, device=cuda)]
        out = dict(x=junk(-3.0), y=junk(-3.0), score=junk(-3.0), count=torch.full((1,), 77, dtype=torch.int32, device=cuda),
                   total=torch.full((1,), 77, dtype=torch.int32, device=cuda), score_plane=None)
        got, want = host_and_device(nm, cuda, c, want_plane=False, out=out)
        same(got, want, (name, cap))
        assert int(want["count"][0]) == min(cap, total) and int(want["total"][0]) == total
        n = min(cap, total)
        assert all((got[key][0][n:] == -3.0).all().item() for key in ("x", "y", "score"))     # nothing at or beyond the cap


@pytest.mark.parametrize("cap", [1, 3])
def test_one_workgroup_emits_multi_trip_frames_back_to_back(nm, cuda, cap):
    c = E.back_to_back_case()
    with grid_cap(nm, cap):
        got, want = host_and_device(nm, cuda, c)
    same(got, want, cap)
    assert len(set(want["total"].tolist())) == 3


# ---- B. Gxy beyond 32 bits signed ----
@pytest.mark.parametrize("h", [70, 4 * 16 + 1, 4 * 16 + 15])
def test_gxy_beyond_32_bits_signed(nm, cuda, h):
    c = E.gxy_case(h)
    got, want = host_and_device(nm, cuda, c)
    same(got, want, h)
    assert (want["total"] >= 3).all()


# ---- C. exact ties ----
TIES = E.tie_cases()


@pytest.mark.parametrize("c", [t[0] for t in TIES], ids=[t[0]["name"] for t in TIES])
def test_exact_ties_across_the_tile_seams(nm, cuda, c):
    for cap in (0, 1):
        with grid_cap(nm, cap):
            got, want = host_and_device(nm, cuda, c)
        same(got, want, (c["name"], cap))


# ---- D. the window's footprint ----
@pytest.mark.parametrize("r", [1, 3, 7])
def test_the_footprint_of_a_pixel_without_a_level(nm, cuda, r):
    c, masked, groups = E.foot_cases(r)
    for offset in (4, 1):                                                # 16-byte loads and scalars
        same(*host_and_device(nm, cuda, c, offset), (r, offset))
    for k, cm in enumerate(masked):
        same(*host_and_device(nm, cuda, cm, 4 if k % 2 == 0 else 1), cm["name"])


# ---- E. call shapes ----
@pytest.mark.parametrize("w,h,offset", [(128, 40, 4), (128, 40, 1), (130, 70, 4)])
def test_a_mask_with_three_frames(nm, cuda, w, h, offset):
    c = E.mask_case(w, h)
    for cap in (0, 1):
        with grid_cap(nm, cap):
            same(*host_and_device(nm, cuda, c, offset), (w, h, offset, cap))


def test_the_workspaces_own_score_planes(nm, cuda):
    """want_score_plane=False with n = 3 at 97 x 61: the own planes start 5917 floats apart inside the workspace, which is
    filled with garbage before each of two calls; the corners and the own planes themselves equal the host twin's"""
    fw, fh = 97, 61
    c = E.case("own_planes", [R.noise(1, fw, fh), R.noise(7, fw, fh), R.checker(fw, fh, 3)], r=3, nms=4)
    want = host_of(nm, c)
    ws = nm.KltCornersWorkspace(3, fw, fh, cuda)
    for fill in (0xA5, 0x3C):
        ws.buf.fill_(fill)
        got = device_of(nm, cuda, c, (0, 0, 0), want_plane=False, workspace=ws)
        assert got["score_plane"] is None
        same(got, dict(want, score_plane=None), fill)
        first = (-ws.buf.data_ptr()) % 64                                 # the call aligns the workspace to 64 bytes
        own = ws.buf[first:first + 3 * fw * fh * 4].cpu().numpy().view(F32).reshape(3, fh, fw)
        assert np.array_equal(own.view(np.uint32), want["score_plane"].view(np.uint32))
    assert (want["total"] >= 3).sum() >= 2


def test_planes_of_mixed_alignment(nm, cuda):
    """two frames of 128 x 40, one 16 bytes and one 4 bytes aligned: the whole call takes the scalar loads, and gives what the
    all-scalar and the all-wide call give"""
    for mask in (None, R.holes(128, 40)):
        c = E.case("mixed", [R.noise(9, 128, 40), R.noise(10, 128, 40)], r=3, nms=4, mask=mask)
        want = host_of(nm, c)
        assert (want["total"] >= 3).all()
        for offsets in ((4, 1), (1, 4), (4, 3), (1, 1), (4, 4), (0, 8)):
            same(device_of(nm, cuda, c, offsets), want, offsets)


@pytest.mark.parametrize("mask_offset", [1, 2, 3, 4])
def test_aligned_planes_with_an_unaligned_mask(nm, cuda, mask_offset):
    c = E.mask_case(128, 40)
    want = host_of(nm, c)
    same(device_of(nm, cuda, c, (4, 0, 8), mask_offset), want, mask_offset)


@pytest.mark.parametrize("cap", [0, 1, 3])
def test_held_points_in_bulk(nm, cuda, cap):
    """3 x 643 held rows: eight workgroups' worth by default, a striding mark launch under grid caps 1 and 3"""
    c, left = E.bulk_held_case()
    assert 3 * len(c["held"][0][0]) > 256
    with grid_cap(nm, cap):
        got, want = host_and_device(nm, cuda, c)
    same(got, want, cap)
    E.assert_bulk_held([t.cpu().numpy() for t in got["x"]], [t.cpu().numpy() for t in got["y"]], got["count"].cpu().numpy(),
                       got["total"].cpu().numpy(), left)
