"""The exposure stages on the device (nm_mosaic_exposure_sums_dev, nm_mosaic_gains_dev, nm_transform_blend_batch_gain) on the
cases of tests/exposure_edges_ref.py: sums equal to the host twin's as integers (and to the numpy model's where the lattice is
small; tests/test_mosaic_exposure_edges_host.py compares the twin with the model on every case and checks that every tile of
a walked shape holds counting pixels), gains and stats equal to the host twin's bit for bit. Every output is written between
two guard bands into memory pre-filled with a sentinel, so a sum that the memset misses, a launch behind the early return of
an empty lattice, or a gain that is not written shows.

Which case reaches which device-only line of mosaic_exposure_sums_kernel. `t += gridDim.x`: 16385 x 3 (workgroup 0 alone
takes a second tile), 1087 x 481 and 2175 x 963 at stride 2 (16 workgroups do), 2048 x 512 and 32767 x 2 (all, twice),
2 x 32767 (all, four times); 255 and 256 tiles are the sizes at which none may. `t % tiles_x`, `t / tiles_x`: 17 tile columns
under 256 workgroups (1087 x 481), one column (2 x 32767), one row (16385 x 3, 32767 x 2). The `parts` clamps: by the tiles
(1087 x 480: 255), by 256 (every L = 1 shape above 256 tiles), by ceil(4096 / L) (L = 256 on 1025 x 5: 16 workgroups for 17
tiles; L = 17: 241 for 272). `r += WAVES` and `v0 + r < lh`: lattices of 1 .. 5, 31, 32 and 33 rows. `u < lw`: 63, 65 and 129
columns, the one-column last tile of 16385 and 1025, the 63-column one of 32767. The `if (... && total)` skip: the all-0 frames
(N > 0, six sums 0), every link that is not usable, and every workgroup whose tiles the disc mask hides.
"""
import ctypes as C

import numpy as np
import pytest

import exposure_edges_ref as E
import exposure_ref as X
import test_gpu_mosaic_exposure as G

pytestmark = pytest.mark.gpu

F32 = np.float32
ONE = int(np.float32(1).view(np.uint32))
_t, _guarded, _guards_intact = G._t, G._guarded, G._guards_intact


def _dev_sums(nm, cuda, frames, la, lb, H, status=None, mask=None, stride=1, lo=E.LO, hi=E.HI, up=None):
    """the device's (L, 7) as uint64 numpy, written between intact guards over a sentinel"""
    import torch
    L = len(la)
    up = {} if up is None else up
    d = [up.setdefault(id(f), _t(f, cuda)) for f in frames]
    whole, out = _guarded(L * 7, torch.int64, cuda, -7)
    got = nm.mosaic_exposure_sums(d, la, lb, _t(np.asarray(H, F32).reshape(L, 9), cuda),
                                  link_status=None if status is None else _t(status, cuda),
                                  mask=None if mask is None else _t(mask, cuda), stride=stride, lo=lo, hi=hi, sums=out)
    got = got.cpu().numpy().view(np.uint64)
    assert _guards_intact(whole, L * 7, -7)
    return got


# ---- A ----
@pytest.mark.parametrize("k", range(len(E.WALK)), ids=E.WALK_IDS)
def test_tile_walk(nm, cuda, k):
    c = E.walk_cases()[k]
    assert E.lattice_of(c["fw"], c["fh"], c["stride"], c["L"]) == (c["lw"], c["lh"], c["tiles_x"], c["tiles"], c["parts"])
    up = {}
    for masked in ((False, True) if c["masked"] else (False,)):
        mask = E.mask_of(c["fw"], c["fh"]) if masked else None
        want = nm.mosaic_exposure_sums_host(c["frames"], c["la"], c["lb"], c["H"], link_status=c["status"], mask=mask,
                                            stride=c["stride"], lo=E.LO, hi=E.HI)
        got = _dev_sums(nm, cuda, c["frames"], c["la"], c["lb"], c["H"], c["status"], mask, c["stride"], up=up)
        assert np.array_equal(got, want), (c["what"], masked, np.argwhere(got != want)[:5])
        assert all(bool(want[l, 0]) == E.live(c, l) for l in range(c["L"]))
        if E.cheap(c):
            assert got.tolist() == E.model_sums(c, masked)[0], (c["what"], masked)


def test_a_walked_links_sums_do_not_depend_on_its_slot(nm, cuda):
    c = next(c for c in E.walk_cases() if c["L"] == 256)
    l0 = 11
    a, b, H = c["la"][l0], c["lb"][l0], c["H"][l0]
    alone = _dev_sums(nm, cuda, [c["frames"][a], c["frames"][b]], [0], [1], H)
    assert alone[0, 0] > 0 and alone.tolist() == [X.sums_int(c["frames"][a], c["frames"][b], H, stride=1)]
    up = {}
    for slot in (0, 100, 255):
        la, lb, Hs = list(c["la"]), list(c["lb"]), c["H"].copy()
        la[slot], lb[slot], Hs[slot] = a, b, H
        got = _dev_sums(nm, cuda, c["frames"], la, lb, Hs, c["status"], up=up)
        assert np.array_equal(got[slot], alone[0]), slot


# ---- B ----
def test_lattice_and_frame_edges(nm, cuda):
    for c in E.edge_cases():
        fr = [c["A"], c["B"]]
        want = nm.mosaic_exposure_sums_host(fr, [0], [1], c["H"], stride=c["stride"], lo=c["lo"], hi=c["hi"])
        got = _dev_sums(nm, cuda, fr, [0], [1], c["H"], stride=c["stride"], lo=c["lo"], hi=c["hi"])
        assert np.array_equal(got, want) and got.tolist() == [E.edge_model(c)], (c["what"], got, want)
        if c["want"] is not None:
            assert got[0, 0] == c["want"], c["what"]


# ---- C ----
def _gains(nm, cuda, c, **kw):
    """device gains and stats over sentinels == the host twin's, bit for bit; returns the twin's"""
    import torch
    n = c["n"]
    S = np.array(c["S"], np.uint64)
    want_g, want_s = nm.mosaic_gains_host(n, c["la"], c["lb"], S, **kw)
    wg, g = _guarded(3 * n, torch.float32, cuda, -3.0)
    ws, st = _guarded(9, torch.float64, cuda, -3.0)
    dkw = dict(kw, link_status=_t(kw["link_status"], cuda)) if "link_status" in kw else kw
    got_g, got_s = nm.mosaic_gains(n, c["la"], c["lb"], _t(S.view(np.int64), cuda), gains=g, stats=st, **dkw)
    got_g, got_s = got_g.cpu().numpy(), got_s.cpu().numpy()
    assert np.array_equal(got_g.view(np.uint32), want_g.view(np.uint32)), (c.get("what"), kw, got_g, want_g)
    assert np.array_equal(got_s.view(np.uint64), want_s.view(np.uint64)), (c.get("what"), kw, got_s, want_s)
    assert not np.isnan(got_g).any() and not np.isnan(got_s).any()
    assert _guards_intact(wg, 3 * n, -3.0) and _guards_intact(ws, 9, -3.0)
    return want_g, want_s


@pytest.mark.parametrize("k", range(len(E.SINGULAR)))
def test_singular_inputs(nm, cuda, k):
    c = E.SINGULAR[k]
    for mode in (X.PER_CHANNEL, X.COMMON):
        g, stats = _gains(nm, cuda, c, sigma_n=c["sn"], sigma_g=c["sg"], mode=mode)
        assert stats[8] == c["ends"][mode] and stats[6] == len(c["la"]), (mode, stats)
        if c["ends"][mode] == X.END_SINGULAR:
            assert (g.view(np.uint32) == ONE).all() and stats[3:6].tolist() == stats[:3].tolist()


def test_sigma_corners(nm, cuda):
    for which, sums in enumerate(E.CORNER_SUMS):
        c = dict(n=3, la=[0, 1], lb=[1, 2], S=[sums] * 2)
        for (sn, sg), end in zip(E.CORNER_SIGMAS, E.CORNER_ENDS[which]):
            for mode in (X.PER_CHANNEL, X.COMMON):
                g, stats = _gains(nm, cuda, c, sigma_n=sn, sigma_g=sg, mode=mode)
                assert np.isfinite(g).all() and np.isfinite(stats).all() and (g >= F32(0.25)).all() and (g <= F32(4)).all()
                assert (stats[6], stats[7], stats[8]) == (2, 3, end), (sn, sg, mode, stats)


def test_usability_boundary_and_other_sigmas(nm, cuda):
    import test_mosaic_exposure_host as HT
    for c in E.usability_cases():
        for mode in (X.PER_CHANNEL, X.COMMON):
            g, stats = _gains(nm, cuda, c, mode=mode, **c["kw"])
            assert (stats[6], stats[8]) == (sum(c["usable"]), X.END_OK) and stats[7] == c["n"] - len(c["gains_one"]), c["what"]
            assert (g[c["gains_one"]].view(np.uint32) == ONE).all()
    la, lb, S, _ = HT.synthetic_sums(64, 256, 6656, dead_frame=17, few=(1,))
    for sn, sg in E.SIGMA_PAIRS:
        assert E.gain_bound_holds(sn, sg, 64, 256)
        g, stats = _gains(nm, cuda, dict(n=64, la=la, lb=lb, S=S), sigma_n=sn, sigma_g=sg)
        ref = X.solve_f64(64, la, lb, S.tolist(), sigma_n=sn, sigma_g=sg)[0]
        assert (np.abs(g.astype(np.float64) - ref) <= X.gain_bound(ref, 64, 256, sn, sg)).all()


def test_graph_shapes_at_64_frames(nm, cuda):
    for c in E.graph_cases():
        for mode in (X.PER_CHANNEL, X.COMMON):
            g, stats = _gains(nm, cuda, c, mode=mode)
            assert stats[8] == X.END_OK and stats[6] == len(c["la"]), c["what"]
            ref = X.solve_f64(c["n"], c["la"], c["lb"], c["S"], mode=mode)[0]
            assert (np.abs(g.astype(np.float64) - ref) <= X.gain_bound(ref, c["n"], len(c["la"]))).all(), c["what"]


def test_one_frame_is_always_refused(nm, cuda):
    import torch
    lib = nm.lib()
    frame = torch.full((8, 16, 4), 100, dtype=torch.uint8, device=cuda)
    H = _t(np.eye(3, dtype=F32).reshape(1, 9).repeat(2, 0), cuda)
    S = _t(np.array([[100, 9000, 9000, 9000, 9900, 9900, 9900]] * 2, np.int64), cuda)
    ws, sums = _guarded(14, torch.int64, cuda, -7)
    wg, g = _guarded(3, torch.float32, cuda, -3.0)
    wt, st = _guarded(9, torch.float64, cuda, -3.0)
    ints = lambda v: (C.c_int * len(v))(*v)
    tab = (C.c_void_p * 1)(frame.data_ptr())
    for la, lb in (((0,), (0,)), ((0,), (1,)), ((1,), (0,)), ((0, 0), (0, 0)), ((-1,), (0,))):
        L = len(la)
        assert lib.nm_mosaic_exposure_sums_dev(1, L, tab, ints(la), ints(lb), 16, 8, None, H.data_ptr(), None, 1, 5, 250,
                                               sums.data_ptr(), nm._stream()) == 1
        assert lib.nm_mosaic_gains_dev(1, L, ints(la), ints(lb), S.data_ptr(), None, 64, 10.0, 0.1, 0.5, 2.0, 0, g.data_ptr(),
                                       st.data_ptr(), nm._stream()) == 1
    torch.cuda.synchronize()
    for whole, value in ((ws, -7), (wg, -3.0), (wt, -3.0)):
        assert (whole.cpu().numpy() == value).all()


# ---- D ----
def test_bad_gains_on_an_empty_canvas(nm, cuda):
    """On a canvas pixel of weight 0 the byte is nm_u8_sat(r g 255.9999f): a negative or NaN product stores 0; a gain of +inf
    stores 255 where the sample r is positive and 0 where it is exactly 0 (inf 0 is NaN). A finite gain of 3e38 tells the two
    apart the same way (the smallest positive sample is 2^-16 / 255 and no product overflows), so it is the reference for
    +inf; the frame carries a block of zero bytes so that exact zeros exist."""
    one = dict(G.small_blend_case(1, False))
    one["canvas"], one["cwts"] = np.zeros_like(one["canvas"]), np.zeros_like(one["cwts"])
    frame = one["frames"][0][0].copy()
    frame[30:80, 40:120, :3] = 0
    plain = G._blend(nm, cuda, one, frames=[frame])
    touched = plain[1] > 0
    rest = ~touched
    assert touched.sum() > 5000 and (plain[0][..., 3][touched] == 255).all()

    def run(row):
        cv, cw = G._blend(nm, cuda, one, np.array([row], F32), frames=[frame])
        assert np.array_equal(cw.view(np.uint32), plain[1].view(np.uint32)), row
        assert not cv[rest].any() and (cv[..., 3][touched] == 255).all(), row
        return cv[..., :3]
    nan, inf = float("nan"), float("inf")
    for row in ((-2.0, -0.5, -1e-30), (nan, nan, nan), (-inf, -inf, -inf)):
        assert not run(row)[touched].any(), row
    got, big = run((inf, inf, inf)), run((3e38, 3e38, 3e38))
    assert np.array_equal(got, big)
    bright = touched[..., None] & (plain[0][..., :3] > 0)
    assert bright.sum() > 5000 and (got[bright] == 255).all()
    zeros = touched[..., None] & (got == 0)
    assert zeros.sum() > 1000 and (plain[0][..., :3][zeros] == 0).all() and set(np.unique(got[touched])) == {0, 255}
    mixed = run((nan, 1.0, -2.0))
    assert np.array_equal(mixed[..., 1], plain[0][..., 1]) and not mixed[..., 0].any() and not mixed[..., 2].any()
    assert plain[0][..., 1][touched].any()
