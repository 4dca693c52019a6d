"""nm_convolve_f32 on the routes next to the aligned one (niftymatch_amd/csrc/nm_conv_route.hpp): a result, a buffer or an image
that starts one float past a 16-byte boundary takes the tile kernel (conv_sep_kernel; tests/test_conv_route.py pins the route),
which stages and stores scalars. Both outputs are compared with the oracle bit for bit, on the smallest shapes that cross every
edge of a 64 x 32 tile, for every unrolled radius; each output lives inside a larger tensor of sentinels, and what lies in front
of and behind the written width x height floats must keep the sentinel."""
import functools

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

RADII = (5, 7, 8, 10, 12, 13, 16)
SHAPES = [(64, 32),        # exactly one tile
          (68, 35),        # a second tile column of 4 pixels and a second tile row of 3
          (4, 1),          # the smallest plane
          (200, 150)]      # a general case
# one-float offsets of (image, result, buffer)
CASES = {"result+1": (0, 1, 0), "buffer+1": (0, 0, 1), "result+1,buffer+1": (0, 1, 1), "image+1": (1, 0, 0)}
PAD = 64                   # floats in front of and behind a plane: 256 bytes, so PAD keeps the allocation's alignment
SENTINEL = np.float32(-12345.5)


def _taps(r):
    """2r+1 normalised binomial-like taps with full mantissas (the radius, not the sigma, selects the kernel)"""
    x = np.arange(-r, r + 1, dtype=np.float64)
    t = np.exp(-x * x / (2.0 * (r / 4.0 + 0.3) ** 2))
    return (t / t.sum()).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(oracle, w, h, r):
    img = H.synth.noise_frame(11, w, h)
    out, buf = oracle.convolve(img, _taps(r), r)
    for a in (img, out, buf):
        a.setflags(write=False)
    return img, out, buf


def _eq(got, ref, what):
    same = got.view(np.uint32) == ref.view(np.uint32)
    assert same.all(), "%s: %d of %d elements differ (max abs diff %g)" % (
        what, (~same).sum(), same.size, np.nanmax(np.abs(got.astype(np.float64) - ref.astype(np.float64))))


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("wh", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_convolve_off_the_aligned_route(nm, oracle, cuda, wh, case):
    import torch
    w, h = wh
    n = w * h
    oi, orr, ob = CASES[case]
    for r in RADII:
        img, ref, refbuf = _reference(oracle, w, h, r)
        taps = torch.tensor(_taps(r), device=cuda)
        d_img = torch.full((n + 2 * PAD,), float(SENTINEL), dtype=torch.float32, device=cuda)
        d_img[PAD + oi: PAD + oi + n] = torch.tensor(img.reshape(-1), device=cuda)      # a copy: the shared reference stays read-only
        d_res = torch.full((n + 2 * PAD,), float(SENTINEL), dtype=torch.float32, device=cuda)
        d_buf = torch.full((n + 2 * PAD,), float(SENTINEL), dtype=torch.float32, device=cuda)
        for t, off in ((d_img, oi), (d_res, orr), (d_buf, ob)):
            assert (t.data_ptr() + 4 * PAD) % 16 == 0 and (t.data_ptr() + 4 * (PAD + off)) % 16 == 4 * off
        rc = nm.lib().nm_convolve_f32(d_res.data_ptr() + 4 * (PAD + orr), d_img.data_ptr() + 4 * (PAD + oi),
                                      d_buf.data_ptr() + 4 * (PAD + ob), w, h, taps.data_ptr(), r,
                                      torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        what = "%dx%d r=%d %s" % (w, h, r, case)
        for name, t, off, want in (("result", d_res, orr, ref), ("buffer", d_buf, ob, refbuf)):
            got = t.cpu().numpy()
            _eq(got[PAD + off: PAD + off + n].reshape(h, w), want, "%s %s" % (name, what))
            assert (got[:PAD + off] == SENTINEL).all(), "%s %s: written in front of the plane" % (name, what)
            assert (got[PAD + off + n:] == SENTINEL).all(), "%s %s: written behind the plane" % (name, what)
        assert (d_img.cpu().numpy()[PAD + oi: PAD + oi + n] == img.reshape(-1)).all()
