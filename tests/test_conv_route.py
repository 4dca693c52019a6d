"""Which kernel a Gaussian launch gets (niftymatch_amd/csrc/nm_conv_route.hpp) is one host function of integers, handed out by
nm_conv_route_of: no GPU needed. The table below is frozen by hand from the conditions of the launch path as it stood before the
routing was gathered into one place (launch_conv_r / _rv / _rvt, nm_launch_convolve, nm_launch_convolve_batch), so it holds on both
sides of that change. `a` = every pointer 16-byte aligned; radius 7 unless stated."""
import pytest

NONE, PACKED, PACKED_BUF, TILE, GENERIC, INVALID = range(6)
UNROLLED = (5, 7, 8, 10, 12, 13, 16)
OTHER = (0, 3, 6, 9, 11, 14, 15, 17)


def _route(nm, w, h, r=7, result=1, buffer=0, dog=0, grad=0, img=0, out=0):
    return nm.lib().nm_conv_route_of(w, h, r, result, buffer, dog, grad, img, out)


# (what, keyword arguments of _route without the radius, route): every row holds for each of the seven unrolled radii
ROWS = [
    ("1080p, a, result + buffer", dict(w=1920, h=1080, buffer=1), PACKED_BUF),
    ("1080p, aligned image, result or buffer off by 4 bytes", dict(w=1920, h=1080, buffer=1, out=4), TILE),
    ("1080p, a, buffer, no result", dict(w=1920, h=1080, result=0, buffer=1), TILE),
    ("1080p, a, no buffer, {result}", dict(w=1920, h=1080), PACKED),
    ("1080p, a, no buffer, {result, dog, grad}", dict(w=1920, h=1080, dog=1, grad=1), PACKED),
    ("1080p, a, no buffer, {grad}", dict(w=1920, h=1080, result=0, grad=1), PACKED),
    ("1921 x 1080, a", dict(w=1921, h=1080), TILE),
    ("1921 x 1080, a, buffer", dict(w=1921, h=1080, buffer=1), TILE),
    ("1080p, image off by 4 bytes", dict(w=1920, h=1080, img=4), TILE),
    ("1080p, image off by 4 bytes, buffer", dict(w=1920, h=1080, buffer=1, img=4), TILE),
    ("60 x 33, a, buffer", dict(w=60, h=33, buffer=1), PACKED_BUF),
    ("135 x 67", dict(w=135, h=67), TILE),
    ("135 x 67, buffer", dict(w=135, h=67, buffer=1), TILE),
    ("buffer with dog", dict(w=1920, h=1080, buffer=1, dog=1), INVALID),
    ("buffer with grad", dict(w=1920, h=1080, buffer=1, grad=1), INVALID),
    ("buffer with dog, odd width", dict(w=135, h=67, buffer=1, dog=1), INVALID),
    ("buffer with grad, odd width", dict(w=135, h=67, buffer=1, grad=1), INVALID),
    ("32768 x 32767, a, no buffer: the last plane below 4 GiB", dict(w=32768, h=32767), PACKED),
    ("32768 x 32768, a, no buffer: 4 GiB", dict(w=32768, h=32768), TILE),
    ("32768 x 32768, a, with buffer", dict(w=32768, h=32768, buffer=1), TILE),
]


@pytest.mark.parametrize("what,kw,route", ROWS, ids=[r[0] for r in ROWS])
def test_unrolled_radii_route_by_geometry_alignment_and_outputs(nm, what, kw, route):
    assert _route(nm, r=7, **kw) == route
    for r in UNROLLED:                                   # each of the seven radii routes like radius 7
        assert _route(nm, r=r, **kw) == route, (what, r)


def test_other_radii_need_a_buffer(nm):
    for r in OTHER:
        for w, h in ((1920, 1080), (135, 67)):
            assert _route(nm, w, h, r, buffer=1) == GENERIC
            assert _route(nm, w, h, r, buffer=1, dog=1, grad=1) == GENERIC      # the two-pass path takes the fused outputs
            assert _route(nm, w, h, r) == INVALID
            assert _route(nm, w, h, r, dog=1, grad=1) == INVALID


def test_negative_radius_is_rejected(nm):
    assert _route(nm, 1920, 1080, -1) == INVALID
    assert _route(nm, 1920, 1080, -1, buffer=1) == INVALID


def test_empty_image_is_a_no_op_before_the_radius_is_looked_at(nm):
    for w, h in ((0, 1080), (1920, 0), (0, 0), (-3, 5)):
        for r in UNROLLED + OTHER + (-1,):
            for buffer in (0, 1):
                assert _route(nm, w, h, r, buffer=buffer) == NONE
                assert _route(nm, w, h, r, buffer=buffer, dog=1) == NONE


def test_the_route_is_a_pure_function(nm):
    args = [kw for _, kw, _ in ROWS]
    first = [_route(nm, r=r, **kw) for kw in args for r in UNROLLED + OTHER + (-1,)]
    second = [_route(nm, r=r, **kw) for kw in args for r in UNROLLED + OTHER + (-1,)]
    assert first == second
    assert set(first) == {PACKED, PACKED_BUF, TILE, GENERIC, INVALID}


def test_only_the_low_four_address_bits_count(nm):
    for bits in range(1, 16):
        assert _route(nm, 1920, 1080, img=bits) == TILE
        assert _route(nm, 1920, 1080, buffer=1, out=bits) == TILE
    assert _route(nm, 1920, 1080, img=16) == PACKED and _route(nm, 1920, 1080, buffer=1, out=32) == PACKED_BUF
    assert _route(nm, 1920, 1080, out=4) == PACKED          # without a buffer the outputs' alignment was never looked at
