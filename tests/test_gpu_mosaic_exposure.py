"""The device entries of the mosaic exposure compensation: nm_mosaic_exposure_sums_dev and nm_mosaic_gains_dev against their
host twins bit for bit (the host twins against the numpy model: tests/test_mosaic_exposure_host.py), the gained blend
against nm_transform_blend_batch (bit for bit for no gains and unit gains) and against the float64 interval model
(tests/exposure_ref.run_blend), and the three stages end to end on the loop-closure views, eagerly and in one HIP graph.
There is no workspace: the outputs are the only device memory the stages write, and they are sentinel-guarded here.

End-to-end figures (printed by the test): see DESIGN.md section 7, "Exposure compensation"."""
import functools

import numpy as np
import pytest

import exposure_ref as X
import loop_closure_ref as LC
import test_mosaic_exposure_host as HT
import test_warp_float64 as W
import warp_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
STRIDE, LO, HI, MIN_PIXELS = 4, 5, 250, 64      # the end-to-end test's choices (the host test checks their condition)
GUARD = 64


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _guarded(n, dtype, dev, value):
    """a device tensor of n values between two guards of sentinels: (whole, view of the n)"""
    import torch
    whole = torch.full((n + 2 * GUARD,), value, dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + n]


def _guards_intact(whole, n, value):
    h = whole.cpu().numpy()
    return (h[:GUARD] == value).all() and (h[GUARD + n:] == value).all()


def link_batch(n, L, fw, fh, seed):
    """n frames (four distinct ones, so pointers repeat for n > 4), L links over them with every map of the host test in turn
    and a status that drops some"""
    rng = np.random.default_rng(seed)
    base = [HT.frame(40 + k, fw, fh, lo=-60 if k == 2 else 20, hi=315 if k == 2 else 235) for k in range(min(n, 4))]
    frames = [base[k % len(base)] for k in range(n)]
    H = list(HT.maps(fw, fh).values())
    la, lb = [], []
    for l in range(L):
        a, b = rng.choice(n, 2, replace=False)
        la.append(int(a))
        lb.append(int(b))
    Hs = np.stack([H[l % len(H)] for l in range(L)])
    status = np.where(np.arange(L) % 11 == 5, 0, 1).astype(np.int32)
    return frames, la, lb, Hs, status


def dev_frames(frames, dev):
    cache = {}
    return [cache.setdefault(id(f), _t(f, dev)) for f in frames]


@pytest.mark.parametrize("L,n,fw,fh,stride,masked", [(1, 2, 67, 45, 1, False), (63, 64, 67, 45, 3, True), (64, 64, 131, 97, 4, False),
                                                     (65, 2, 131, 97, 1, True), (256, 64, 67, 45, 1, False),
                                                     (5, 3, 131, 97, 64, True)])
def test_device_sums_equal_the_host_twin(nm, cuda, L, n, fw, fh, stride, masked):
    import torch
    frames, la, lb, Hs, status = link_batch(n, L, fw, fh, 7 * L + n)
    mask = HT.disc_mask(fw, fh) if masked else None
    want = nm.mosaic_exposure_sums_host(frames, la, lb, Hs, link_status=status, mask=mask, stride=stride, lo=LO, hi=HI)
    whole, out = _guarded(L * 7, torch.int64, cuda, -7)
    got = nm.mosaic_exposure_sums(dev_frames(frames, cuda), la, lb, _t(Hs, cuda), link_status=_t(status, cuda),
                                  mask=None if mask is None else _t(mask, cuda), stride=stride, lo=LO, hi=HI, sums=out)
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want)
    assert _guards_intact(whole, L * 7, -7)
    assert want[status == 1][:, 0].any() or stride == 64


@pytest.mark.parametrize("fw,fh", HT.SIZES)
def test_device_sums_on_the_host_test_cases(nm, cuda, fw, fh):
    frames, la, lb, Hs = HT.sums_case(fw, fh)
    d = dev_frames(frames, cuda)
    for stride in HT.STRIDES:
        for mask in (None, HT.disc_mask(fw, fh)):
            for lo, hi in ((5, 250), (0, 255)):
                want = nm.mosaic_exposure_sums_host(frames, la, lb, Hs, mask=mask, stride=stride, lo=lo, hi=hi)
                got = nm.mosaic_exposure_sums(d, la, lb, _t(Hs, cuda), mask=None if mask is None else _t(mask, cuda),
                                              stride=stride, lo=lo, hi=hi)
                assert np.array_equal(got.cpu().numpy().view(np.uint64), want), (stride, lo, hi)


def test_a_links_sums_do_not_depend_on_its_slot_or_its_neighbours(nm, cuda):
    fw, fh = 131, 97
    frames, la, lb, Hs, _ = link_batch(64, 256, fw, fh, 5)
    d = dev_frames(frames, cuda)
    a, b, H = la[0], lb[0], Hs[0]
    alone = nm.mosaic_exposure_sums([d[a], d[b]], [0], [1], _t(H[None], cuda), stride=1).cpu().numpy()
    assert alone[0, 0] > 0
    for slot in (0, 77, 255):
        la2, lb2, H2 = list(la), list(lb), Hs.copy()
        la2[slot], lb2[slot], H2[slot] = a, b, H
        got = nm.mosaic_exposure_sums(d, la2, lb2, _t(H2, cuda), stride=1).cpu().numpy()
        assert np.array_equal(got[slot], alone[0]), slot
    other = nm.mosaic_exposure_sums([d[b], d[a]], [1], [0], _t(H[None], cuda), stride=1).cpu().numpy()
    assert np.array_equal(other, alone)


@pytest.mark.parametrize("n,L,dead", HT.SOLVE_CASES)
def test_device_gains_equal_the_host_twin(nm, cuda, n, L, dead):
    import torch
    la, lb, S, _ = HT.synthetic_sums(n, L, 100 * n + L, dead_frame=dead, few=(1,) if L > 2 else ())
    dS = _t(S.view(np.int64), cuda)
    status = np.where(np.arange(L) % 5 == 3, 0, 1).astype(np.int32)
    for kw in (dict(), dict(mode=nm.EXPOSURE_COMMON), dict(link_status=status, g_min=0.95, g_max=1.05),
               dict(min_pixels=10 ** 6), dict(sigma_n=1.0, sigma_g=10.0, g_min=0.9, g_max=1.1)):
        want_g, want_s = nm.mosaic_gains_host(n, la, lb, S, **kw)
        wg, g = _guarded(3 * n, torch.float32, cuda, -3.0)
        ws, st = _guarded(9, torch.float64, cuda, -3.0)
        dkw = dict(kw, link_status=_t(status, cuda)) if "link_status" in kw else kw
        got_g, got_s = nm.mosaic_gains(n, la, lb, dS, gains=g, stats=st, **dkw)
        assert np.array_equal(got_g.cpu().numpy().view(np.uint32), want_g.view(np.uint32)), kw
        assert np.array_equal(got_s.cpu().numpy().view(np.uint64), want_s.view(np.uint64)), kw
        assert _guards_intact(wg, 3 * n, -3.0) and _guards_intact(ws, 9, -3.0)
        assert want_s[8] == (X.END_NO_LINK if "min_pixels" in kw else X.END_OK)


# ---- the gained blend ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_blend_case(n, u8):
    """n frames of 160 x 120 into a patterned, partly filled 420 x 300 canvas; rectangles inside, clipped on every side,
    empty (nw = 0) and wholly off the canvas among them"""
    rng = np.random.default_rng(11 + n)
    fw, fh, cw, ch = 160, 120, 420, 300
    dt = np.uint8 if u8 else np.float32
    canvas = np.zeros((ch, cw, 4), np.uint8)
    cwts = np.zeros((ch, cw), np.float32)
    yy, xx = np.mgrid[0:ch, 0:cw]
    filled = ((xx // 37 + yy // 29) % 3 == 0) & (xx < 0.6 * cw)
    pat = W.content("step", cw, ch, 5)
    pat[..., 3] = 255
    canvas[filled] = pat[filled]
    cwts[filled] = (0.25 + 0.5 * ((xx // 37) % 2))[filled]
    mask, wts = W.plane("disc", fw, fh, 1, dt), W.plane("feather", fw, fh, 2, dt)
    kinds = ("smooth", "noise", "step")
    frames = []
    for k in range(n):
        a = rng.uniform(-0.05, 0.05)
        s = rng.uniform(0.9, 1.05)
        M = np.array([[s * np.cos(a), -s * np.sin(a), rng.uniform(-3, 2)], [s * np.sin(a), s * np.cos(a), rng.uniform(-3, 2)],
                      [rng.uniform(-2e-5, 2e-5), rng.uniform(-2e-5, 2e-5), 1.0]], np.float32)
        nw, nh = fw + 12, fh + 8
        tx, ty = int(rng.integers(-40, cw - nw + 40)), int(rng.integers(-30, ch - nh + 30))
        if n > 1 and k % 8 == 1:
            tx = -60                                         # clipped on the left
        if n > 1 and k % 8 == 2:
            nw = 0                                           # empty
        if n > 1 and k % 8 == 5:
            tx, ty = cw + 10, -ch                            # off the canvas
        frames.append((W.content(kinds[k % 3], fw, fh, 300 + k), mask, wts, M, tx, ty, nw, nh))
    return dict(canvas=canvas, cwts=cwts, frames=frames)


def _records(frames, dev):
    import torch
    rec = np.zeros((len(frames), 16), np.int32)
    for k, (_, _, _, mat, tx, ty, nw, nh) in enumerate(frames):
        rec[k, :9] = np.asarray(mat, F32).reshape(9).view(np.int32)
        rec[k, 9:14] = (tx, ty, nw, nh, 1)
    return torch.from_numpy(rec).to(dev)


def _blend(nm, cuda, case, gains="ungained", frames=None):
    """(canvas, canvas_wts) as numpy; gains 'ungained': nm_transform_blend_batch, else the gained entry (None: NULL)"""
    canvas, cwts = _t(case["canvas"], cuda), _t(case["cwts"], cuda)
    fr = case["frames"]
    dev = {}
    d = lambda a: dev.setdefault(id(a), _t(a, cuda))
    fs = [d(f[0]) for f in fr] if frames is None else [d(f) for f in frames]
    args = (canvas, cwts, fs, [d(f[1]) for f in fr], [d(f[2]) for f in fr], _records(fr, cuda))
    if isinstance(gains, str):
        nm.transform_blend_batch(*args)
    else:
        nm.transform_blend_batch_gain(*args, gains=None if gains is None else _t(np.asarray(gains, F32), cuda))
    return canvas.cpu().numpy(), cwts.cpu().numpy()


@pytest.mark.parametrize("n", [1, 3, 17, 64])
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_no_gains_and_unit_gains_equal_the_ungained_blend(nm, cuda, n, u8):
    case = small_blend_case(n, u8)
    want = _blend(nm, cuda, case)
    assert (want[1] != case["cwts"]).mean() > 0.05
    for gains in (None, np.ones((n, 3), F32)):
        got = _blend(nm, cuda, case, gains)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


@pytest.mark.parametrize("n,u8", [(3, True), (17, False)])
def test_gained_blend_lies_inside_the_float64_models_interval(nm, cuda, n, u8):
    case = small_blend_case(n, u8)
    gains = np.random.default_rng(n).uniform(0.5, 2.0, (n, 3)).astype(F32)
    gains[0] = (0.5, 2.0, 1.0)
    canvas, cwts = _blend(nm, cuda, case, gains)
    st, covered = X.run_blend(case, gains)
    W._record(W.check_blend("gained blend n=%d" % n, canvas, cwts, st, covered, (case["canvas"], case["cwts"]))).require()
    plain = _blend(nm, cuda, case)
    assert np.array_equal(cwts.view(np.uint32), plain[1].view(np.uint32))
    assert (canvas[..., :3] != plain[0][..., :3]).mean() > 0.05
    # the check is sharp: the ungained canvas does not pass for the gained one
    assert W.check_blend("ungained as gained", plain[0], plain[1], st, covered, (case["canvas"], case["cwts"])).bad > 0


def test_gain_zero_and_a_saturating_gain(nm, cuda):
    case = dict(small_blend_case(3, False))
    zero = _blend(nm, cuda, case, np.zeros((3, 3), F32))
    black = [np.zeros_like(f[0]) for f in case["frames"]]
    want = _blend(nm, cuda, case, frames=black)
    assert np.array_equal(zero[0], want[0]) and np.array_equal(zero[1], want[1])     # what a black frame stores
    one = dict(small_blend_case(1, False))
    one["canvas"], one["cwts"] = np.zeros_like(one["canvas"]), np.zeros_like(one["cwts"])
    plain = _blend(nm, cuda, one)
    sat = _blend(nm, cuda, one, np.full((1, 3), 8.0, F32))
    touched = plain[1] > 0
    assert touched.sum() > 5000 and np.array_equal(sat[1], plain[1])       # the frame's disc: about 9 % of the canvas
    # on an empty canvas the byte is nm_u8_sat(r g 255.9999f): 255 wherever the ungained byte trunc(r 255.9999f) >= 32
    bright = touched[..., None] & (plain[0][..., :3] >= 32)
    assert bright.sum() > 5000 and (sat[0][..., :3][bright] == 255).all()
    dark = touched[..., None] & (plain[0][..., :3] == 0)
    assert (sat[0][..., :3][dark] <= 8).all()


# ---- end to end on the loop-closure views -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_views(seed):
    """the K views of the loop-closure scene, rendered on the host with the float64 sampler model"""
    tex = R.Texture(LC.scene(seed))
    x, y = np.meshgrid(np.arange(LC.VW, dtype=np.float64), np.arange(LC.VH, dtype=np.float64))
    out = []
    for A in LC.view_maps():
        p = LC.apply(A, np.c_[x.reshape(-1), y.reshape(-1)])
        S = R.sample(tex, p[:, 0], p[:, 1])[0]
        v = np.minimum(np.floor(S * R.K_U8), 255).astype(np.uint8).reshape(LC.VH, LC.VW, 4)
        v[..., 3] = 255
        out.append(v)
    return tuple(out)


def scaled_views(views, seed=3):
    """each view's channels scaled by known factors in [0.8, 1.25], rounded and clipped: (views, t (K, 3))"""
    t = np.random.default_rng(seed).uniform(0.8, 1.25, (len(views), 3))
    out = []
    for v, tk in zip(views, t):
        s = v.copy()
        s[..., :3] = np.clip(np.rint(v[..., :3] * tk), 0, 255)
        out.append(s)
    return out, t


def test_measure_solve_place_blend_on_the_loop_closure_views(nm, cuda):
    import torch
    K = LC.K
    pairs = LC.high_pairs()
    la, lb = [a for a, _ in pairs], [b for _, b in pairs]
    Hs = np.stack([LC.pair_map(a, b).astype(F32).reshape(9) for a, b in pairs])
    A = LC.view_maps()
    chain = np.stack([np.linalg.inv(np.linalg.inv(A[0]) @ a) for a in A])
    chain = (chain / chain[:, 2:, 2:]).astype(F32).reshape(K, 9)
    scenes = [scaled_views(host_views(seed)) for seed in (91, 93, 92)]
    frames = [_t(v, cuda) for v in scenes[0][0]]
    dH, dchain = _t(Hs, cuda), _t(chain, cuda)
    ones = torch.ones((LC.VH, LC.VW), dtype=torch.float32, device=cuda)
    canvas = torch.zeros((LC.SCENE_H, LC.SCENE_W, 4), dtype=torch.uint8, device=cuda)
    cwts = torch.zeros((LC.SCENE_H, LC.SCENE_W), dtype=torch.float32, device=cuda)
    sums = torch.empty((len(pairs), 7), dtype=torch.int64, device=cuda)
    gains = torch.empty((K, 3), dtype=torch.float32, device=cuda)
    stats = torch.empty(9, dtype=torch.float64, device=cuda)
    records, _ = nm.mosaic_place(dchain, LC.VW, LC.VH, LC.SCENE_W, LC.SCENE_H, LC.ORIGIN_X, LC.ORIGIN_Y)
    assert (records.cpu().numpy()[:, 13] == 1).all()

    def enqueue():                                           # measure -> solve -> gained blend, no host read
        canvas.zero_()
        cwts.zero_()
        nm.mosaic_exposure(frames, la, lb, dH, stride=STRIDE, lo=LO, hi=HI, min_pixels=MIN_PIXELS, sums=sums, gains=gains,
                           stats=stats)
        nm.transform_blend_batch_gain(canvas, cwts, frames, ones, ones, records, gains=gains)

    def host():
        return [t.cpu().numpy().copy() for t in (sums, gains, stats, canvas, cwts)]

    def check(views, t, got):
        S, g, st, cv, cw = got
        want_S = nm.mosaic_exposure_sums_host(views, la, lb, Hs, stride=STRIDE, lo=LO, hi=HI)
        assert np.array_equal(S.view(np.uint64), want_S)
        want_g, want_st = nm.mosaic_gains_host(K, la, lb, want_S, min_pixels=MIN_PIXELS)
        assert np.array_equal(g.view(np.uint32), want_g.view(np.uint32)) and np.array_equal(st, want_st)
        assert st[6] == len(pairs) and st[7] == K and st[8] == X.END_OK          # no link left out
        model_S = X.link_sums(views, la, lb, Hs, stride=STRIDE, lo=LO, hi=HI)
        ref = X.solve_f64(K, la, lb, model_S, min_pixels=MIN_PIXELS)[0]
        eps = float((X.gain_bound(ref, K, len(pairs)) / ref).max())
        before, model, after = X.spread(np.ones((K, 3)), t), X.spread(ref, t), X.spread(g, t)
        print("exposure spread per channel (B, G, R): uncorrected %s, float64 model %s, device %s"
              % (np.round(before, 4), np.round(model, 4), np.round(after, 4)))
        assert (after <= (1 + model) * (1 + eps) / (1 - eps) - 1).all(), (after, model)
        assert (after < before).all(), (after, before)
        assert (cw > 0).mean() > 0.5 and cv[..., :3].any()
        return cv, cw

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        enqueue()
    s.synchronize()
    eager = host()
    cv, cw = check(*scenes[0], eager)
    plain_c, plain_w = torch.zeros_like(canvas), torch.zeros_like(cwts)
    nm.transform_blend_batch(plain_c, plain_w, frames, ones, ones, records)
    assert np.array_equal(plain_w.cpu().numpy(), cw) and not np.array_equal(plain_c.cpu().numpy(), cv)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        enqueue()
    for views, t in scenes[1:]:                              # two replays, new frame contents each time
        for f, v in zip(frames, views):
            f.copy_(_t(v, cuda))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        replayed = host()
        check(views, t, replayed)
    with torch.cuda.stream(s):
        enqueue()
    s.synchronize()
    for a, b in zip(replayed, host()):
        assert np.array_equal(a, b)
    assert not np.array_equal(replayed[0], eager[0])
