"""The device kernels of the warp family through the float64 model (tests/warp_ref.py), with the cases, bounds and checks
of tests/test_warp_float64.py (see its docstring for every derivation): undistort_map, resample_undistort, resample_mask,
resample_perspective (both directions), resample_map_u8x4, ingest_batch (gray and undistorted, n in {1, 5, 64}),
transform_blend and transform_blend_batch (n in {1, 17, 64}); one canvas at the ABI limit of 32767 x 32767; and the
float -> unsigned char rule outside [0, 256) (nm_u8_sat: truncate toward zero, clamp to [0, 255], NaN -> 0; the
reference's own behaviour there cannot be observed without its hardware: parity unpinned)."""
import numpy as np
import pytest

import test_warp_float64 as W
import warp_ref as R

pytestmark = pytest.mark.gpu


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _records(frames, dev):
    import torch
    rec = np.zeros((len(frames), 16), np.int32)
    for k, (_, _, _, mat, tx, ty, nw, nh) in enumerate(frames):
        rec[k, :9] = np.asarray(mat, np.float32).reshape(9).view(np.int32)
        rec[k, 9:14] = (tx, ty, nw, nh, 1)
    return torch.from_numpy(rec).to(dev)


@pytest.mark.parametrize("case", W.PERSPECTIVE_CASES, ids=lambda c: "%dx%d-%s-%s-%s" % (c[0], c[1], c[2], c[3], "inv" if c[4] else "fwd"))
def test_gpu_perspective_against_model(nm, cuda, case):
    fw, fh, kind, mk, inverse, cols, rows = case
    frame, mat = W.perspective_inputs(case)
    d_frame = _t(frame, cuda)
    out, xp, yp = nm.resample_perspective(d_frame, cols, rows, _t(mat, cuda), inverse)
    name = "gpu perspective %dx%d %s %s %s" % (fw, fh, kind, mk, "inv" if inverse else "fwd")
    W._record(W.check_coords(name + " coords", xp.cpu().numpy(), yp.cpu().numpy(),
                             *W.perspective_coords(mat, inverse, cols, rows))).require()
    tex = R.Texture(frame)
    hx, hy = xp.cpu().numpy(), yp.cpu().numpy()
    W._record(W.check_u8_samples(name, out.cpu().numpy(), tex, hx, hy)).require()
    if fw < 7680:                                       # the caller's-map entry on the same coordinates
        got = nm.resample_map_u8x4(d_frame, xp, yp)
        W._record(W.check_u8_samples(name + " resample_map_u8x4", got.cpu().numpy(), tex, hx, hy)).require()


def _check_ingest(nm, cuda, name, frames, u, v, hu, hv, table):
    gray, und = nm.ingest_batch([_t(f, cuda) for f in frames], u, v, undistorted=True)
    for k, f in enumerate(frames):
        hund = und[k].cpu().numpy()
        W._record(W.check_u8_samples("%s ingest frame %d of %d" % (name, k, len(frames)), hund, R.Texture(f), hu, hv)).require()
        want = table[R.gray_index(hund)]
        assert np.array_equal(gray[k].cpu().numpy().view(np.uint32), want), "ingest gray != correctly rounded n/100 of its frame"


@pytest.mark.parametrize("case", W.RADIAL_CASES, ids=lambda c: "%dx%d" % (c[0], c[1]))
def test_gpu_radial_maps_against_model(nm, cuda, case):
    w, h, k = case
    x, y, cam, dist = W.radial_inputs(w, h, k)
    u, v = nm.undistort_map(_t(x, cuda), _t(y, cuda), _t(cam, cuda), _t(dist, cuda))
    hu, hv = u.cpu().numpy(), v.cpu().numpy()
    name = "gpu radial %dx%d" % (w, h)
    W._record(W.check_coords(name + " map", hu, hv, *R.undistort(x, y, cam, dist), *W.undistort_error(x, y, cam, dist))).require()
    assert hu.min() < -1 and hv.min() < -1 and hu.max() > w and hv.max() > h
    big = w >= 7680
    frame = W.content("smooth" if big else "noise", w, h, 41)
    got = nm.resample_map_u8x4(_t(frame, cuda), u, v)
    W._record(W.check_u8_samples(name + " u8x4 map", got.cpu().numpy(), R.Texture(frame), hu, hv)).require()
    tf = W.plane("noise" if big else "smooth", w, h, 42, np.float32)
    W._record(W.check_f32_samples(name + " f32", nm.resample_undistort(_t(tf, cuda), u, v).cpu().numpy(), R.Texture(tf),
                                  hu, hv)).require()
    table = R.gray_table()[0]
    if big:
        _check_ingest(nm, cuda, name, [frame], u, v, hu, hv, table)                      # n = 1 at 8K
        return
    tu = W.plane("step", w, h, 43, np.uint8)
    W._record(W.check_mask_samples(name + " mask", nm.resample_mask(_t(tu, cuda), u, v, 0.4).cpu().numpy(), R.Texture(tu),
                                   hu, hv, 0.4)).require()
    td = W.plane("disc", w, h, 44, np.float32)
    W._record(W.check_mask_samples(name + " mask disc", nm.resample_mask(_t(td, cuda), u, v, 0.5).cpu().numpy(),
                                   R.Texture(td), hu, hv, 0.5)).require()
    if w == 1920:
        _check_ingest(nm, cuda, name, [W.content(("noise", "smooth", "step")[i % 3], w, h, 60 + i) for i in range(5)],
                      u, v, hu, hv, table)                                                # n = 5 at 1080p


def test_gpu_ingest_64_frames_against_model(nm, cuda):
    w, h = 480, 270
    x, y, cam, dist = W.radial_inputs(w, h, (0.30, 0.08, -0.02))
    u, v = nm.undistort_map(_t(x, cuda), _t(y, cuda), _t(cam, cuda), _t(dist, cuda))
    frames = [W.content(("noise", "smooth", "step")[i % 3], w, h, 500 + i) for i in range(64)]
    _check_ingest(nm, cuda, "gpu radial 480x270", frames, u, v, u.cpu().numpy(), v.cpu().numpy(), R.gray_table()[0])


def _gpu_blend(nm, cuda, case, batched):
    canvas, cwts = _t(case["canvas"], cuda), _t(case["cwts"], cuda)
    fr = case["frames"]
    dev = {}

    def d(a):
        if id(a) not in dev:
            dev[id(a)] = _t(a, cuda)
        return dev[id(a)]
    if batched:
        nm.transform_blend_batch(canvas, cwts, [d(f[0]) for f in fr], [d(f[1]) for f in fr], [d(f[2]) for f in fr],
                                 _records(fr, cuda))
    else:
        for (frame, mask, wts, mat, tx, ty, nw, nh) in fr:
            nm.transform_blend(canvas, cwts, d(frame), nw, nh, _t(mat, cuda), tx, ty, d(mask), d(wts))
    return canvas, cwts


@pytest.mark.parametrize("name,entries", [("one_4k_f32", "both"), ("three_odd_u8", "both"), ("seventeen_1080p_f32", "both"),
                                          ("sixtyfour_small_u8", "batched")])
def test_gpu_blend_against_model(nm, cuda, name, entries):
    case = W.blend_case(name)
    st, covered = W.run_blend(case)
    initial = (case["canvas"], case["cwts"])
    results = []
    for batched in ((False, True) if entries == "both" else (True,)):
        canvas, cwts = _gpu_blend(nm, cuda, case, batched)
        hc, hw = canvas.cpu().numpy(), cwts.cpu().numpy()
        W._record(W.check_blend("gpu blend %s %s" % (name, "batched" if batched else "per frame"), hc, hw, st, covered,
                                initial)).require()
        results.append((hc, hw))
    assert (results[0][1] > 0).mean() > 0.3


def test_gpu_exact_subset_is_bit_exact(nm, cuda):
    tex, xs, ys, lx, ly = W.exact_subset_inputs()
    got = nm.resample_undistort(_t(tex, cuda), _t(xs, cuda), _t(ys, cuda)).cpu().numpy()
    np.testing.assert_array_equal(got.reshape(-1).view(np.uint32), W.exact_subset_expected(tex, lx, ly).view(np.uint32))


def test_gpu_gray_all_triples(nm, cuda):
    bgra = W.gray_triples()
    W.check_gray(nm.grayscale(_t(bgra, cuda)).cpu().numpy(), bgra)


def test_gpu_canvas_at_abi_limit(nm, cuda):
    """32767 x 32767: pixel indices pass 2^29 and 2^30, the uchar4 byte offset 2^31 and 2^32. Only the touched rectangles
    come to the host; the rest is verified on the device by counting."""
    import torch
    S = 32767
    fw, fh = 256, 192
    nw, nh = fw + 8, fh + 6
    rng = np.random.default_rng(21)
    mask = W.plane("disc", fw, fh, 1, np.float32)
    wts = W.plane("feather", fw, fh, 2, np.float32)
    place = [(-10, -7), (S - nw + 12, 0), (0, S - nh + 9), (S - nw, S - nh), (S - 100, S - 80)]
    frames = []
    for k, (tx, ty) in enumerate(place):
        a, s = rng.uniform(-0.03, 0.03), rng.uniform(0.97, 1.03)
        M = np.array([[s * np.cos(a), -s * np.sin(a), rng.uniform(-3, 1)], [s * np.sin(a), s * np.cos(a), rng.uniform(-3, 1)],
                      [1e-6, -1e-6, 1]], np.float32)
        frames.append((W.content(("noise", "smooth", "step")[k % 3], fw, fh, 700 + k), mask, wts, M, tx, ty, nw, nh))
    # the touched rectangles (x0, y0, x1, y1) and the frames inside each
    rects = [((0, 0, nw - 10, nh - 7), [0]), ((S - nw + 12, 0, S, nh), [1]), ((0, S - nh + 9, nw, S), [2]),
             ((S - nw, S - nh, S, S), [3, 4])]
    for batched in (False, True):
        try:
            canvas = torch.zeros((S, S, 4), dtype=torch.uint8, device=cuda)
            cwts = torch.zeros((S, S), dtype=torch.float32, device=cuda)
        except (RuntimeError, MemoryError) as e:        # torch.OutOfMemoryError is a RuntimeError
            pytest.skip("no memory for a 32767 x 32767 canvas: %s" % str(e)[:120])
        d = [(_t(f[0], cuda), _t(f[1], cuda), _t(f[2], cuda)) for f in frames]
        if batched:
            nm.transform_blend_batch(canvas, cwts, [a[0] for a in d], [a[1] for a in d], [a[2] for a in d],
                                     _records(frames, cuda))
        else:
            for f, a in zip(frames, d):
                nm.transform_blend(canvas, cwts, a[0], nw, nh, _t(f[3], cuda), f[4], f[5], a[1], a[2])
        torch.cuda.synchronize()
        n_pix = n_wts = 0
        for (x0, y0, x1, y1), ks in rects:
            hc = canvas[y0:y1, x0:x1].cpu().numpy()
            hw = cwts[y0:y1, x0:x1].cpu().numpy()
            sub = dict(canvas=np.zeros((y1 - y0, x1 - x0, 4), np.uint8), cwts=np.zeros((y1 - y0, x1 - x0), np.float32),
                       frames=[frames[k][:4] + (frames[k][4] - x0, frames[k][5] - y0, nw, nh) for k in ks])
            st, covered = W.run_blend(sub)
            s = W.check_blend("abi-limit canvas rect %d,%d %s" % (x0, y0, "batched" if batched else "per frame"), hc, hw, st,
                              covered, (sub["canvas"], sub["cwts"])).require()
            assert (hw > 0).mean() > 0.3, "the rectangle must be written"
            n_pix += int((hc.view(np.uint32) != 0).sum())
            n_wts += int((hw != 0).sum())
        assert int(torch.count_nonzero(canvas.view(torch.int32))) == n_pix, "a pixel outside the rectangles was written"
        assert int(torch.count_nonzero(cwts)) == n_wts, "a weight outside the rectangles was written"
        del canvas, cwts
        torch.cuda.empty_cache()


# ---- conversions outside [0, 256) ------------------------------------------------------------------------------------
SPECIALS = np.array([-1e10, -300.0, -1.5, -1.0, -0.5, -0.0, 0.0, 1e-40, -1e-40, 0.99, 17.5, 254.999, 255.0, 255.99, 255.99998,
                     256.0, 300.0, 65536.0, 1e10, np.inf, -np.inf, np.nan], np.float32)


def u8_rule(v):
    """truncate toward zero, clamp to [0, 255], NaN -> 0"""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v), 0.0, np.clip(np.trunc(v), 0.0, 255.0)).astype(np.uint8)


def _guarded(nbytes, cuda):
    import torch
    g = 4096
    buf = torch.full((nbytes + 2 * g,), 0xA5, dtype=torch.uint8, device=cuda)
    return buf, buf[g:g + nbytes], g


def test_gpu_put_channel_and_cast_follow_the_u8_rule(nm, oracle, cuda):
    import torch
    w, h = 64, 8
    plane = np.resize(SPECIALS, (h, w)).astype(np.float32)
    clean = np.full((h, w), 17.5, np.float32)
    bgra = np.random.default_rng(1).integers(0, 256, (h, w, 4), dtype=np.uint8)
    for ch in range(4):
        buf, view, g = _guarded(h * w * 4, cuda)
        view.copy_(_t(bgra, cuda).reshape(-1))
        d_plane = _t(plane, cuda)
        rc = nm.lib().nm_put_channel_f32(nm._dev(view, torch.uint8), nm._dev(d_plane, torch.float32), w, h, ch, nm._stream())
        torch.cuda.synchronize()
        assert rc == 0
        hb = buf.cpu().numpy()
        assert (hb[:g] == 0xA5).all() and (hb[-g:] == 0xA5).all(), "put_channel wrote outside the image"
        got = hb[g:-g].reshape(h, w, 4)
        want = bgra.copy()
        want[..., ch] = 255 if ch == 3 else u8_rule(plane)
        np.testing.assert_array_equal(got, want)                               # the rule, and the other channels untouched
        np.testing.assert_array_equal(got, oracle.put_channel(bgra, plane, ch))  # GPU and oracle agree
    for max_val in (0, 200):
        buf, view, g = _guarded(h * w, cuda)
        d_plane = _t(plane, cuda)
        rc = nm.lib().nm_cast_f32_u8(nm._dev(d_plane, torch.float32), w, h, nm._dev(view, torch.uint8), max_val, nm._stream())
        torch.cuda.synchronize()
        assert rc == 0
        hb = buf.cpu().numpy()
        assert (hb[:g] == 0xA5).all() and (hb[-g:] == 0xA5).all(), "cast_f32_u8 wrote outside the plane"
        got = hb[g:-g].reshape(h, w)
        want = u8_rule(plane)
        if max_val:
            with np.errstate(invalid="ignore"):
                want = np.where(plane >= max_val, max_val, want).astype(np.uint8)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got, oracle.cast_f32_u8(plane, max_val))
        np.testing.assert_array_equal(nm.cast_f32_u8(_t(clean, cuda), max_val).cpu().numpy(), np.full((h, w), 17, np.uint8))


def test_gpu_resample_of_out_of_domain_textures(nm, oracle, cuda):
    import torch
    w, h = 96, 64
    rng = np.random.default_rng(2)
    clean = rng.uniform(0, 1, (h, w)).astype(np.float32)
    tex = clean.copy()
    spots = [(8, 8, 2.0), (8, 24, 1e10), (8, 40, -1.0), (8, 56, -1e10), (24, 8, 300.0), (24, 24, 1.0000001)]
    for (j, i, val) in spots:
        tex[j, i] = val
    tex[48, 70], tex[48, 80], tex[56, 70] = np.inf, -np.inf, np.nan
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    x, y = np.ascontiguousarray(x + 0.25), np.ascontiguousarray(y + 0.125)
    affected = np.zeros((h, w), bool)
    for (j, i) in [s[:2] for s in spots] + [(48, 70), (48, 80), (56, 70)]:
        affected[max(j - 1, 0):j + 1, max(i - 1, 0):i + 1] = True       # the samples whose four taps include the texel
    got = nm.resample_undistort(_t(tex, cuda), _t(x, cuda), _t(y, cuda)).cpu().numpy()
    assert np.array_equal(got, oracle.resample_undistort(tex, x, y), equal_nan=True)
    base = nm.resample_undistort(_t(clean, cuda), _t(x, cuda), _t(y, cuda)).cpu().numpy()
    assert np.array_equal(got[~affected], base[~affected]), "an in-domain sample changed"
    buf, view, g = _guarded(h * w, cuda)
    d_tex, d_x, d_y = _t(tex, cuda), _t(x, cuda), _t(y, cuda)
    rc = nm.lib().nm_resample_mask_u8(nm._dev(view, torch.uint8), nm._dev(d_tex), w, h, nm.TEX_F32, w, h,
                                      nm._dev(d_x, torch.float32), nm._dev(d_y, torch.float32), 0.25, nm._stream())
    torch.cuda.synchronize()
    assert rc == 0
    hb = buf.cpu().numpy()
    assert (hb[:g] == 0xA5).all() and (hb[-g:] == 0xA5).all(), "resample_mask wrote outside the plane"
    gm = hb[g:-g].reshape(h, w)
    np.testing.assert_array_equal(gm, oracle.resample_mask(tex, x, y, 0.25))
    bm = nm.resample_mask(_t(clean, cuda), _t(x, cuda), _t(y, cuda), 0.25).cpu().numpy()
    np.testing.assert_array_equal(gm[~affected], bm[~affected])
    # the rule on the float the kernel itself reports: r = resample_undistort / 255.9999 up to rounding, so test it where
    # the scaled sample is far from an integer and from the threshold
    r = got.astype(np.float64) / 255.9999
    with np.errstate(invalid="ignore"):
        v = r * 255.999
        far = ~np.isfinite(v) | ((np.abs(v - np.round(v)) > 1e-3) & (np.abs(r - 0.25) > 1e-4))
        want = np.where(np.isnan(r) | (r <= 0.25), 0, u8_rule(v))
    np.testing.assert_array_equal(gm[far], want[far])
    assert gm[8, 8] == 255 and gm[8, 24] == 255 and gm[8, 40] == 0 and gm[8, 56] == 0 and gm[56, 70] == 0


def test_gpu_blend_with_out_of_domain_weights(nm, oracle, cuda):
    fw, fh, cw, ch = 96, 64, 128, 96
    rng = np.random.default_rng(3)
    f1, f2 = rng.integers(0, 256, (fh, fw, 4), dtype=np.uint8), rng.integers(0, 256, (fh, fw, 4), dtype=np.uint8)
    mask = np.ones((fh, fw), np.float32)
    w1 = np.full((fh, fw), 0.5, np.float32)
    w2 = np.full((fh, fw), 0.25, np.float32)
    w2[:, 16:32] = 0.0
    w2[:, 32:48] = -0.5                    # cwt + nwt == 0
    w2[:, 48:64] = -2.0                    # cwt + nwt < 0
    w2[:, 64:80] = np.nan
    eye = np.eye(3, dtype=np.float32)
    tx, ty = 16, 16
    fr = [(f1, mask, w1, eye, tx, ty, fw, fh), (f2, mask, w2, eye, tx, ty, fw, fh)]
    case = dict(canvas=np.zeros((ch, cw, 4), np.uint8), cwts=np.zeros((ch, cw), np.float32), frames=fr)
    oc, ow = case["canvas"], case["cwts"]
    for (frame, m, wt, mat, tx_, ty_, nw, nh) in fr:
        oc, ow = oracle.transform_blend(oc, ow, frame, nw, nh, mat, tx_, ty_, m, wt)
    for batched in (False, True):
        canvas, cwts = _gpu_blend(nm, cuda, case, batched)                    # raises unless the call returns 0
        hc, hw = canvas.cpu().numpy(), cwts.cpu().numpy()
        inside = np.zeros((ch, cw), bool)
        inside[ty:ty + fh, tx:tx + fw] = True
        assert (hc[~inside] == 0).all() and (hw[~inside] == 0).all(), "the blend wrote outside the frame's grid"
        np.testing.assert_array_equal(hc, oc)
        assert np.array_equal(hw, ow, equal_nan=True)
        # in-domain columns (weights 0.5 then 0.25): the weighted mean, within one level of the float64 value
        a, b = f1[:, :16, :3].astype(np.float64), f2[:, :16, :3] * (255.9999 / 255.0)
        d = (b * 0.25 + a * 0.5) / 0.75 - hc[ty:ty + fh, tx:tx + 16, :3]
        assert d.min() > -1e-3 and d.max() < 1 + 1e-3
        # weight 0 keeps the colour; a zero sum gives +-inf or NaN, by the rule 255 or 0; a NaN weight gives NaN -> 0; a
        # negative sum gives a finite quotient that follows the rule like any other (equal to the oracle, above)
        np.testing.assert_array_equal(hc[ty:ty + fh, tx + 16:tx + 32, :3], f1[:, 16:32, :3])
        z = hc[ty:ty + fh, tx + 32:tx + 48, :3]
        assert np.isin(z, (0, 255)).all()
        assert (hc[ty:ty + fh, tx + 64:tx + 80, :3] == 0).all()
        assert (hc[inside][:, 3] == 255).all()
