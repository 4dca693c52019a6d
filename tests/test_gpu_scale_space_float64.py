"""Every kernel family of the scale space, the extrema detection and the refinement against the binary64 model of
tests/scale_space_ref.py. Nothing here compares with the oracle: it only builds INPUT planes (blurred frames, DoG planes). Outputs
start as a sentinel and everything outside the written region must keep it. Prints the worst deviation / bound per family."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import helpers as H
import oracle_lib as O
import scale_space_ref as R
import test_scale_space_float64 as T

pytestmark = pytest.mark.gpu

SENT = 7.0
ROUTE_PACKED_BUF, ROUTE_TILE = 2, 3            # NM_CONV_ROUTE_* of include/nm_abi.h
FRAGILE_CAP = 0.05


def _build_constant(name):
    """A constexpr int of niftymatch_amd/csrc/nm_common.hpp, as the build compiles it."""
    import niftymatch_amd
    src = open(os.path.join(os.path.dirname(niftymatch_amd.__file__), "csrc", "nm_common.hpp")).read()
    m = re.search(r"\b%s\s*=\s*([^,;]+)[,;]" % name, src)
    assert m, name
    return int(eval(m.group(1), {"NM_DET_WAVE_W": int(re.search(r"\bNM_DET_WAVE_W\s*=\s*(\d+)", src).group(1))}))


WAVE_W, SEG_W = _build_constant("NM_DET_WAVE_W"), _build_constant("NM_DET_SEG_W")
DET_WIDTHS = (WAVE_W + 1, WAVE_W + 2, SEG_W + 1, SEG_W + 2)
DET_HEIGHTS = (6, 21, 28)                      # one past the 5-, 20- and 27-row unit groups


def _t(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _np(t):
    return t.detach().cpu().numpy()


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _full(shape, cuda, value=SENT):
    import torch
    return torch.full(shape, value, dtype=torch.float32, device=cuda)


def _sync():
    import torch
    torch.cuda.synchronize()


def _arena_view(ptr, count, cuda):
    import torch
    buf = torch.empty(count, dtype=torch.float32, device=cuda)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(buf.data_ptr(), ptr, count * 4, 3) == 0
    return _np(buf)


def _arena_put(ptr, tensor):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(ptr, tensor.data_ptr(), tensor.numel() * 4, 3) == 0


# ---- Gaussian convolution ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conv_model(w, h, sigma):
    img = H.synth.noise_frame(7, w, h)
    t64, e_t, r = R.taps64(sigma)
    return img, t64, e_t, r


@pytest.mark.parametrize("wh,route", [((320, 200), ROUTE_PACKED_BUF), ((201, 83), ROUTE_TILE), ((68, 35), ROUTE_TILE),
                                      ((3, 2), ROUTE_TILE)])
def test_convolve_both_outputs(nm, cuda, wh, route):
    w, h = wh
    p = R.sift_params64(1920, 1080)
    worst = [0.0, 0.0, 0.0]
    radii = []
    for s in [np.float32(x) for x in p["sigmas"]] + [np.float32(3.0), np.float32(4.0)]:
        img, t64, e_t, r = _conv_model(w, h, float(s))
        taps, r_nm = nm.create_kernel_for_sigma(float(s))
        assert r_nm == r
        worst[0] = max(worst[0], R.ratio(taps - t64, e_t))
        assert worst[0] <= 1.0
        radii.append(r)
        m = R.convolve64(img, taps, r)                       # the kernel receives the product's float32 taps
        if w % 4 == 0 and route == ROUTE_TILE:                 # a width the packed kernel would take: a misaligned plane takes the tile
            store = _t(np.concatenate([np.zeros(1, np.float32), img.ravel()]), cuda)
            timg = store[1:].view(h, w)
        else:
            timg = _t(img, cuda)
        ttaps = _t(taps, cuda)
        out, buf = _full((h + 2, w), cuda), _full((h + 2, w), cuda)
        assert nm.lib().nm_conv_route_of(w, h, r, 1, 1, 0, 0, timg.data_ptr() & 15, (out.data_ptr() | buf.data_ptr()) & 15) == route
        assert nm.lib().nm_convolve_f32(out.data_ptr(), timg.data_ptr(), buf.data_ptr(), w, h, ttaps.data_ptr(), r, None) == 0
        _sync()
        out, buf = _np(out), _np(buf)
        assert (out[h:] == SENT).all() and (buf[h:] == SENT).all()
        worst[1] = max(worst[1], R.ratio(buf[:h] - m["buf"], m["e_buf"]))
        worst[2] = max(worst[2], R.ratio(out[:h] - m["out"], m["e_out"]))
    assert radii == [5, 7, 8, 10, 13, 12, 16]
    T._report("gpu convolve %dx%d" % wh, taps=worst[0], row_pass=worst[1], result=worst[2])
    assert worst[1] <= 1.0 and worst[2] <= 1.0


# ---- decimation, subtraction, gradient ----------------------------------------------------------------------------------------------
def test_downsample_is_the_model_rounded(nm, cuda):
    a = H.blurred_frame(1, 270, 135)
    out = _full((67 + 2, 135), cuda)
    assert nm.lib().nm_downsample2_f32(out.data_ptr(), 135, 67, _t(a, cuda).data_ptr(), 270, 135, None) == 0
    _sync()
    out = _np(out)
    assert np.array_equal(out[:67], R.downsample64(a, 135, 67).astype(np.float32)) and (out[67:] == SENT).all()


def test_subtract_single_and_batch_are_the_model_rounded(nm, cuda):
    w, h = 201, 83
    planes = [H.blurred_frame(s, w, h) for s in range(6)]
    tp = [_t(x, cuda) for x in planes]
    one = _full((h + 2, w), cuda)
    assert nm.lib().nm_subtract_f32(tp[1].data_ptr(), tp[0].data_ptr(), one.data_ptr(), w, h, None) == 0
    out = [_full((h + 2, w), cuda) for _ in range(5)]
    assert nm.lib().nm_subtract_batch_f32(5, _ptrs(tp[1:]), _ptrs(tp[:5]), _ptrs(out), w, h, None) == 0
    _sync()
    want = [R.subtract64(planes[i + 1], planes[i]).astype(np.float32) for i in range(5)]
    for got, ref in zip([one] + out, [want[0]] + want):
        got = _np(got)
        assert np.array_equal(got[:h], ref) and (got[h:] == SENT).all()


def test_gradient_single_and_batch(nm, cuda):
    w, h = 201, 83
    planes = [H.blurred_frame(s, w, h) for s in (1, 2, 3)]
    tp = [_t(x, cuda) for x in planes]
    g = [_full((h + 2, w, 2), cuda) for _ in range(4)]
    assert nm.lib().nm_gradient_f32(tp[0].data_ptr(), g[0].data_ptr(), w, h, None) == 0
    assert nm.lib().nm_gradient_batch_f32(3, _ptrs(tp), _ptrs(g[1:]), w, h, None) == 0
    _sync()
    wm = wa = 0.0
    for got, src in zip(g, [planes[0]] + planes):
        got, m = _np(got), R.gradient64(src)
        assert (got[h:] == SENT).all()
        bad, rm, ra = R.gradient_outside(m, got[:h])
        assert bad == 0 and m["fragile"].mean() <= FRAGILE_CAP
        wm, wa = max(wm, rm), max(wa, ra)
    for name, src in T.gradient_inputs().items():            # ramp: (float)(2 pi); flats: exactly (0, 0); 3 x 2: ring only
        hh, ww = src.shape
        got = _full((hh + 1, ww, 2), cuda)
        assert nm.lib().nm_gradient_f32(_t(src, cuda).data_ptr(), got.data_ptr(), ww, hh, None) == 0
        _sync()
        got, m = _np(got), R.gradient64(src)
        assert (got[hh:] == SENT).all()
        bad, rm, ra = R.gradient_outside(m, got[:hh])
        assert bad == 0, name
        wm, wa = max(wm, rm), max(wa, ra)
        ring = np.ones(src.shape, bool)
        ring[1:-1, 1:-1] = False
        assert not got[:hh][ring].any(), name
        if name == "ramp":
            assert got[10, 10, 1] == np.float32(2 * np.pi)
        if name == "flat":
            assert not got[:hh].any()
    T._report("gpu gradient", magnitude=wm, angle=wa)


# ---- fused octave and scale-space batch against the chain ---------------------------------------------------------------------------
def _chain_ratios(m, levels, dogs, grad, first_level=1, last_level=5):
    fig = {}
    if levels is not None:
        fig["levels"] = max(R.ratio(levels[l] - m["levels"][l], m["e_levels"][l]) for l in range(first_level, last_level + 1))
    if dogs is not None:
        fig["dogs"] = max(R.ratio(dogs[d] - m["dogs"][d], m["e_dogs"][d]) for d in range(5))
    if grad is not None:
        rg = [R.gradient_outside(m["grads"][l], grad[l]) for l in range(3)]
        assert all(b == 0 for b, _, _ in rg), rg
        assert max(m["grads"][l]["fragile"].mean() for l in range(3)) <= FRAGILE_CAP
        fig["grad_mag"], fig["grad_ang"] = max(r[1] for r in rg), max(r[2] for r in rg)
    return fig


@functools.lru_cache(maxsize=None)
def _octave_model(w, h):
    lv0 = H.blurred_frame(3, w, h, sigma=2.0)
    return lv0, R.octave64(lv0, 1920, 1080)


@pytest.mark.parametrize("wh", [(320, 200), (201, 83)])
def test_octave_pyramid_against_the_chain(nm, cuda, wh):
    w, h = wh
    lv0, m = _octave_model(w, h)
    arena = nm.SiftArena(w, h, 1024)
    try:
        n = w * h
        _arena_put(arena.level_ptr(0), _t(lv0, cuda))
        arena.octave_pyramid(w, h)
        _sync()
        levels = [None] + [_arena_view(arena.level_ptr(l), n, cuda).reshape(h, w) for l in range(1, 6)]
        dogs = [_arena_view(arena.dog_ptr(d), n, cuda).reshape(h, w) for d in range(5)]
        grad = _arena_view(arena.grad_ptr(), 6 * n, cuda).reshape(3, h, w, 2)
    finally:
        arena.close()
    fig = _chain_ratios(m, levels, dogs, grad)
    T._report("gpu octave_pyramid %dx%d" % wh, **fig)
    assert max(fig.values()) <= 1.0, fig


@functools.lru_cache(maxsize=None)
def _frame0_model(seed):
    f = H.blurred_frame(seed, 320, 200)
    return f, R.frame_octave0_64(f)


@pytest.mark.parametrize("write_dog", [True, False])
@pytest.mark.parametrize("n", [1, 3])
def test_scale_space_batch_against_the_chain(nm, cuda, n, write_dog):
    w, h = 320, 200
    models = [_frame0_model(30 + i) for i in range(n)]
    arenas = [nm.SiftArena(w, h, 1024) for _ in range(n)]
    try:
        npx = w * h
        if not write_dog:
            for a in arenas:
                for d in range(5):
                    _arena_put(a.dog_ptr(d), _full((npx,), cuda))
        nm.scale_space_batch(arenas, [_t(f, cuda) for f, _ in models], write_dog=write_dog)
        _sync()
        worst = {}
        for a, (f, m) in zip(arenas, models):
            levels = [_arena_view(a.level_ptr(l), npx, cuda).reshape(h, w) for l in range(6)]
            dogs = [_arena_view(a.dog_ptr(d), npx, cuda).reshape(h, w) for d in range(5)]
            grad = _arena_view(a.grad_ptr(), 6 * npx, cuda).reshape(3, h, w, 2)
            if not write_dog:
                assert all((d == SENT).all() for d in dogs), "DoG planes written by a call that asked for none"
            # with DoG planes the launch sequence does not store level 5: it is only read through DoG 4, which is compared
            fig = _chain_ratios(m, levels, dogs if write_dog else None, grad, first_level=0, last_level=4 if write_dog else 5)
            for k, v in fig.items():
                worst[k] = max(worst.get(k, 0.0), v)
    finally:
        for a in arenas:
            a.close()
    T._report("gpu scale_space_batch n=%d dog=%d" % (n, write_dog), **worst)
    assert max(worst.values()) <= 1.0, worst


# ---- detection: every form on the same DoG planes -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _det_case(w, h):
    dogs = T.dense_planes(O, w, h, 11)
    sigma0 = np.float32(R.sift_params64(1920, 1080)["sigma_0"])
    masks = {}
    for xper in (1.0, 2.0):
        mw, mh = int(w * xper), int(h * xper)
        yy, xx = np.mgrid[0:mh, 0:mw]
        mask = (((xx // 7) + (yy // 5)) % 3 != 0).astype(np.float32)
        mask[:, -mw // 4:] = 0.5
        masks[xper] = mask
    models = {None: R.octave_detect64(dogs, 0.0, 10.0, 2.0, sigma0, 3)}
    for xper, mask in masks.items():
        models[xper] = R.octave_detect64(dogs, 0.0, 10.0, xper, sigma0, 3, mask)
    for ms in models.values():
        assert R.fragile_share(ms) <= FRAGILE_CAP
    assert sum(int((m["accepted"] & ~m["fragile"]).sum()) for m in models[None]) >= 3 * (w - 2) * (h - 2) // 30
    return dogs, float(sigma0), masks, models


def _dense_ok(model, got, h, what, sentinel=-1.0):
    got = _np(got)
    assert (got[h:] == SENT).all(), what + ": wrote past the region"
    bad, r, _ = R.dense_outside(model, got[:h], sentinel)
    assert bad == 0, "%s: %d pixels differ from the model" % (what, bad)
    return r


@pytest.mark.parametrize("h", DET_HEIGHTS)
@pytest.mark.parametrize("w", DET_WIDTHS)
def test_detection_forms(nm, cuda, w, h):
    import torch
    dogs, sigma0, masks, models = _det_case(w, h)
    tdog = [_t(d, cuda) for d in dogs]
    L = nm.lib()
    worst = 0.0

    def fresh(rows=2):
        d = [_full((h + rows, w, 4), cuda) for _ in range(3)]
        return d
    # single-level launchers: the caller pre-fills the region with -1, only accepted pixels are written
    for l in range(3):
        d = _full((h + 2, w, 4), cuda)
        d[:h] = -1.0
        assert L.nm_find_keypoints_f32(tdog[l + 1].data_ptr(), tdog[l].data_ptr(), tdog[l + 2].data_ptr(), w, h, 0.0, 10.0, 2.0,
                                       sigma0, 3, l, d.data_ptr(), None) == 0
        _sync()
        worst = max(worst, _dense_ok(models[None][l], d, h, "find_keypoints level %d" % l))
        for xper, mask in masks.items():
            tm = _t(mask, cuda)
            d = _full((h + 2, w, 4), cuda)
            d[:h] = -1.0
            assert L.nm_find_keypoints_masked_f32(tdog[l + 1].data_ptr(), tm.data_ptr(), mask.shape[1], mask.shape[0],
                                                  tdog[l].data_ptr(), tdog[l + 2].data_ptr(), w, h, 0.0, 10.0, xper, sigma0, 3, l,
                                                  d.data_ptr(), None) == 0
            _sync()
            worst = max(worst, _dense_ok(models[xper][l], d, h, "masked xper %g level %d" % (xper, l)))
    # three levels in one launch: every pixel of the region is written
    d = fresh()
    assert L.nm_find_keypoints3_f32(_ptrs(tdog), None, 0, 0, w, h, 0.0, 10.0, 2.0, sigma0, 3, _ptrs(d), None) == 0
    _sync()
    for l in range(3):
        worst = max(worst, _dense_ok(models[None][l], d[l], h, "find_keypoints3 level %d" % l))
    tm = _t(masks[2.0], cuda)
    d = fresh()
    assert L.nm_find_keypoints3_f32(_ptrs(tdog), tm.data_ptr(), 2 * w, 2 * h, w, h, 0.0, 10.0, 2.0, sigma0, 3, _ptrs(d), None) == 0
    _sync()
    for l in range(3):
        worst = max(worst, _dense_ok(models[2.0][l], d[l], h, "find_keypoints3 masked level %d" % l))
    # ... which also resets [w h, reset_end) to -1 and leaves the rest
    d = [_full((h + 40, w, 4), cuda) for _ in range(3)]
    ends = (C.c_size_t * 3)(w * h + 5, 0, (h + 33) * w + 1)
    assert L.nm_find_keypoints3_reset_f32(_ptrs(tdog), None, 0, 0, w, h, 0.0, 10.0, 2.0, sigma0, 3, _ptrs(d), ends, None) == 0
    _sync()
    for l in range(3):
        got = _np(d[l])
        bad, r, _ = R.dense_outside(models[None][l], got[:h])
        assert bad == 0, "reset form level %d" % l
        worst = max(worst, r)
        flat, end = got.reshape(-1, 4), max(int(ends[l]), w * h)
        assert (flat[w * h:end] == -1.0).all() and (flat[end:] == SENT).all(), l
    # compacted lists: raster order within a level, the levels back to back
    cap = w * h
    out = _full((cap + 8, 4), cuda)
    cnt = torch.full((4,), -5, dtype=torch.int32, device=cuda)
    ws = torch.empty(L.nm_find_keypoints3_compact_workspace_bytes(w, h) + 16, dtype=torch.uint8, device=cuda)
    assert L.nm_find_keypoints3_compact_f32(_ptrs(tdog), w, h, 0.0, 10.0, 2.0, sigma0, 3, cap, out.data_ptr(), cnt.data_ptr(),
                                            ws.data_ptr(), None) == 0
    _sync()
    cnt, out = _np(cnt), _np(out)
    assert cnt[3] == -5 and (cnt[:3] > 0).all()
    total = int(cnt[:3].sum())
    assert (out[total:] == SENT).all()
    bad, r, _ = R.list_outside(models[None], out[:total])
    assert bad == 0
    worst = max(worst, r)
    start = 0
    for l in range(3):                                          # raster order, asserted on the rows themselves
        rows = out[start:start + cnt[l]]
        start += cnt[l]
        assert (rows[:, 3] == l).all()
        m = models[None][l]
        keep = m["accepted"] & ~m["fragile"]
        if not m["fragile"].any():
            assert len(rows) == keep.sum()
            pix = m["ys"][keep] * w + m["xs"][keep]
            assert (np.diff(pix) > 0).all()
            assert (np.abs(rows[:, 0] / 2.0 - m["xs"][keep]) < 1).all() and (np.abs(rows[:, 1] / 2.0 - m["ys"][keep]) < 1).all()
    T._report("gpu detection %dx%d" % (w, h), keypoints=worst)


@functools.lru_cache(maxsize=None)
def _special_models(name):
    cur, dn, up = R.wide_exponent_dogs(1) if name == "wide" else R.saddle_dogs(2)
    sigma0 = np.float32(R.sift_params64(1920, 1080)["sigma_0"])
    m = R.detect64(cur, dn, up, 0.0, 10.0, 1.0, sigma0, 3, 1)
    assert R.fragile_share([m]) <= FRAGILE_CAP and (m["accepted"] & ~m["fragile"]).sum() >= 80
    return (cur, dn, up), float(sigma0), m


@pytest.mark.parametrize("name", ["wide", "saddle", "steps"])
def test_detection_on_wide_exponents_saddles_and_ties(nm, cuda, name):
    """Spikes whose neighbours are 2^30 times smaller (where the binary32 forms of refine_at and their binary64 originals could
    part; rejected candidates run through divisions by zero), negative in-plane determinants, exact ties and flats."""
    L = nm.lib()
    if name == "steps":
        dogs, peak, edge, xper, _ = T.detection_cases(O)["steps 96x64"]
        sigma0 = float(np.float32(R.sift_params64(1920, 1080)["sigma_0"]))
        models = R.octave_detect64(dogs, peak, edge, xper, np.float32(sigma0), 3)
        assert R.fragile_share(models) <= FRAGILE_CAP
        h, w = dogs[0].shape
        tdog = [_t(d, cuda) for d in dogs]
        d = [_full((h + 2, w, 4), cuda) for _ in range(3)]
        assert L.nm_find_keypoints3_f32(_ptrs(tdog), None, 0, 0, w, h, peak, edge, xper, sigma0, 3, _ptrs(d), None) == 0
        _sync()
        worst = max(_dense_ok(models[l], d[l], h, "steps level %d" % l) for l in range(3))
    else:
        (cur, dn, up), sigma0, m = _special_models(name)
        h, w = cur.shape
        d = _full((h + 2, w, 4), cuda)
        d[:h] = -1.0
        assert L.nm_find_keypoints_f32(_t(cur, cuda).data_ptr(), _t(dn, cuda).data_ptr(), _t(up, cuda).data_ptr(), w, h, 0.0, 10.0,
                                       1.0, sigma0, 3, 1, d.data_ptr(), None) == 0
        _sync()
        worst = _dense_ok(m, d, h, name)
    T._report("gpu detection %s" % name, keypoints=worst)


# ---- the frame driver (LevelPlanes path) and the octave tail ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _frame_model(w, h, seed):
    frame = H.blurred_frame(seed, w, h)
    models = T.frame_models(O, frame)
    assert R.fragile_share(models) <= FRAGILE_CAP
    assert sum(int((m["accepted"] & ~m["fragile"]).sum()) for m in models) >= (w * h) // 400
    return frame, models


def _check_arena(arena, models, what):
    n = int(arena.num_items.item())
    bad, r, nfr = R.list_outside(models, _np(arena.kpts[:n]))
    assert bad == 0, "%s: %d keypoints differ from the model's list of the whole frame" % (what, bad)
    return r


@pytest.mark.parametrize("tall_min", [1, -1])
@pytest.mark.parametrize("wh", [(320, 200), (250, 131)])
def test_frame_driver_keypoints(nm, cuda, wh, tall_min):
    w, h = wh
    prev = nm.set_detect_tall_min(tall_min)
    worst = 0.0
    try:
        for n in (1, 3):
            cases = [_frame_model(w, h, 60 + i) for i in range(n)]
            arenas = [nm.SiftArena(w, h, 16384) for _ in range(n)]
            try:
                if n == 1:
                    arenas[0].detect_describe(_t(cases[0][0], cuda))
                else:
                    nm.detect_describe_batch(arenas, [_t(f, cuda) for f, _ in cases])
                _sync()
                for i, (a, (f, models)) in enumerate(zip(arenas, cases)):
                    worst = max(worst, _check_arena(a, models, "%dx%d frame %d of %d" % (w, h, i, n)))
            finally:
                for a in arenas:
                    a.close()
    finally:
        nm.set_detect_tall_min(prev)
    T._report("gpu frame driver %dx%d tall_min=%d" % (w, h, tall_min), keypoints=worst)


@pytest.mark.parametrize("n", [1, 2])
def test_octave_tail_keypoints(nm, cuda, n):
    w, h = 640, 480
    cases = [_frame_model(w, h, 70 + i) for i in range(n)]
    arenas = [nm.SiftArena(w, h, 16384) for _ in range(n)]
    worst = 0.0
    try:
        if n == 1:
            arenas[0].detect_describe(_t(cases[0][0], cuda))
        else:
            nm.detect_describe_batch(arenas, [_t(f, cuda) for f, _ in cases])
        _sync()
        for i, (a, (f, models)) in enumerate(zip(arenas, cases)):
            oct3 = [m for m in models if m["xper"] == 8.0]
            assert oct3 and sum(int((m["accepted"] & ~m["fragile"]).sum()) for m in oct3) > 0, "octave 3 holds no keypoint"
            worst = max(worst, _check_arena(a, models, "640x480 frame %d of %d" % (i, n)))
            if not any(m["fragile"].any() for m in oct3):         # octave 3 is the end of the list: checked on its own as well
                kp = _np(a.kpts[:int(a.num_items.item())])
                n3 = sum(int(m["accepted"].sum()) for m in oct3)
                assert n3 <= len(kp) and R.list_outside(oct3, kp[len(kp) - n3:])[0] == 0
            assert a.tail_status() == 0
    finally:
        for a in arenas:
            a.close()
    T._report("gpu octave tail n=%d" % n, keypoints=worst)
