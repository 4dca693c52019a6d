"""The binary64 model of tests/scale_space_ref.py against the CPU oracle, stage by stage (no GPU): every deviation within its
derived bound, identical candidate sets, at most 5 % fragile candidates per case (a condition on the inputs, asserted on the
model alone), a useful number of keypoints per case (floor from the model), and every mutant of the model rejected by the same
check that the model passes. Prints the worst deviation / bound per stage and the fragile shares (pytest -s)."""
import functools

import numpy as np
import pytest

import helpers as H
import scale_space_ref as R

FRAGILE_CAP = 0.05
CONV_SHAPES = ((320, 200), (201, 83), (68, 35), (3, 2))
DET_SHAPES = ((63, 6), (64, 21), (249, 28), (250, 21), (250, 28), (64, 6))


def _report(stage, **figures):
    print("  [scale_space_float64] %-28s %s" % (stage, "  ".join("%s=%.3g" % kv for kv in figures.items())))


@functools.lru_cache(maxsize=None)
def _octave(oracle, w, h, seed, kind="blurred"):
    """DoG planes of one real octave: level 0 is a frame blurred to the scale an octave starts at."""
    f = H.synth.noise_frame(seed, w, h) if kind == "blurred" else H.step_field(seed, w, h)
    lv0 = oracle.convolve(f, *oracle.create_kernel_for_sigma(2.0 if kind == "blurred" else 1.6))[0]
    return oracle.octave_pyramid(lv0, 1920, 1080)


@functools.lru_cache(maxsize=None)
def dense_planes(oracle, w, h, seed):
    """Five zero-mean planes of lightly blurred noise (differences of two independent frames): no scale space, but an extremum
    every 15 pixels or so, which is what the small detection shapes need to hold a useful number of candidates."""
    return [H.blurred_frame(seed + i, w, h, sigma=0.7) - H.blurred_frame(seed + 50 + i, w, h, sigma=0.7) for i in range(5)]


# ---- the checks: each returns (passes, figures) for the model or one mutant of it ------------------------------------------------
def check_params(oracle, mutant=None):
    worst = 0.0
    ok = True
    for w, h in ((1920, 1080), (640, 480), (320, 200), (37, 41), (4096, 2160)):
        p, m = oracle.sift_params(w, h), R.sift_params64(w, h, mutant)
        ok &= p.num_octaves == m["num_octaves"] and p.num_dog_levels == m["num_dog_levels"] and p.num_sigmas == len(m["sigmas"])
        ok &= (p.level_min, p.level_max, p.peak_threshold, p.edge_threshold) == (m["level_min"], m["level_max"], 0.0, 10.0)
        for k in ("sigma_k", "sigma_0", "sigma_d_0", "base_smooth"):
            worst = max(worst, R.ratio(getattr(p, k) - m[k], R.PARAM_REL[k] * m[k]))
        for i in range(5):
            worst = max(worst, R.ratio(p.sigmas[i] - m["sigmas"][i], R.PARAM_REL["sigmas"][i] * m["sigmas"][i]))
    return ok and worst <= 1.0, dict(params=worst)


def _sigmas(oracle):
    p = oracle.sift_params(1920, 1080)
    return [p.base_smooth] + list(p.sigmas)[:5] + [3.0, 4.0, 0.6]           # radii 7, 5, 7, 8, 10, 13, 12, 16, 3


def check_taps(oracle, mutant=None):
    worst, ok = 0.0, True
    for s in _sigmas(oracle):
        t, r = oracle.create_kernel_for_sigma(s)
        t64, e, r64 = R.taps64(s, mutant)
        if r != r64:
            ok = False
            continue
        worst = max(worst, R.ratio(t - t64, e))
    return ok and worst <= 1.0, dict(taps=worst)


def check_convolve(oracle, mutant=None):
    wb = wo = 0.0
    for w, h in CONV_SHAPES:
        img = H.synth.noise_frame(7, w, h)
        for s in _sigmas(oracle)[1:8]:
            t, r = oracle.create_kernel_for_sigma(s)
            out, buf = oracle.convolve(img, t, r)
            m = R.convolve64(img, t, r, mutant=mutant)
            wb, wo = max(wb, R.ratio(buf - m["buf"], m["e_buf"])), max(wo, R.ratio(out - m["out"], m["e_out"]))
    return wb <= 1.0 and wo <= 1.0, dict(row_pass=wb, result=wo)


def check_exact(oracle, mutant=None):
    a, b = H.blurred_frame(1, 270, 135), H.blurred_frame(2, 270, 135)
    ok = np.array_equal(oracle.downsample2(a, 135, 67), R.downsample64(a, 135, 67, mutant).astype(np.float32))
    c, d = a[:83, :201], b[:83, :201]
    ok &= np.array_equal(oracle.subtract(c, d), R.subtract64(c, d, mutant).astype(np.float32))
    return bool(ok), {}


def gradient_inputs():
    ramp = np.tile(np.arange(64, dtype=np.float32) * 2.0, (48, 1))           # dy = 0, dx > 0: theta = (float)(2 pi)
    return dict(blurred=H.blurred_frame(1, 201, 83), ramp=ramp, flat=np.full((40, 40), 3.0, np.float32),
                steps=H.step_field(5, 96, 64), tiny=np.zeros((3, 2), np.float32))


def check_gradient(oracle, mutant=None):
    wm = wa = 0.0
    ok = True
    for name, src in gradient_inputs().items():
        g, m = oracle.gradient(src), R.gradient64(src, mutant=mutant)
        bad, rm, ra = R.gradient_outside(m, g)
        ok &= bad == 0
        wm, wa = max(wm, rm), max(wa, ra)
        assert m["fragile"].mean() <= FRAGILE_CAP, name
        if mutant is None:
            ring = np.ones(src.shape, bool)
            ring[1:-1, 1:-1] = False
            assert not m["mag"][ring].any() and not m["ang"][ring].any()
    if mutant is None:
        m = R.gradient64(gradient_inputs()["ramp"])
        assert m["ang"][10, 10] == R.TWO_PI and np.float32(m["ang"][10, 10]) == np.float32(2 * np.pi)
        assert not R.gradient64(gradient_inputs()["flat"])["ang"].any()
    return ok, dict(magnitude=wm, angle=wa)


def check_chain(oracle, mutant=None):
    fig = {}
    ok = True
    for w, h in ((320, 200), (201, 83)):
        lv0 = H.blurred_frame(3, w, h, sigma=2.0)
        levels, dogs, grad = oracle.octave_pyramid(lv0, 1920, 1080)
        m = R.octave64(lv0, 1920, 1080, mutant)
        rl = max(R.ratio(levels[l] - m["levels"][l], m["e_levels"][l]) for l in range(1, 6))
        rd = max(R.ratio(dogs[d] - m["dogs"][d], m["e_dogs"][d]) for d in range(5))
        rg = [R.gradient_outside(m["grads"][l], grad[l]) for l in range(3)]
        ok &= rl <= 1.0 and rd <= 1.0 and all(b == 0 for b, _, _ in rg)
        assert max(m["grads"][l]["fragile"].mean() for l in range(3)) <= FRAGILE_CAP
        fig.update({"levels_%d" % w: rl, "dogs_%d" % w: rd, "grad_mag_%d" % w: max(r[1] for r in rg),
                    "grad_ang_%d" % w: max(r[2] for r in rg)})
    return ok, fig


def detection_cases(oracle):
    """name -> (dogs (5 planes), peak, edge, xper, mask). Shapes step one past a 62-column wave, a 248-column segment and the 5-,
    20- and 27-row unit groups of the detection kernels."""
    cases = {}
    for w, h in DET_SHAPES:
        cases["dense %dx%d" % (w, h)] = (dense_planes(oracle, w, h, 11), 0.0, 10.0, 2.0, None)
    cases["blurred 320x200"] = (_octave(oracle, 320, 200, 3)[1], 0.0, 10.0, 1.0, None)
    d = dense_planes(oracle, 250, 28, 11)               # a peak threshold in the middle of the candidates' values
    cases["peak 250x28"] = (d, float(np.float32(np.median(np.abs(d[2])))), 10.0, 1.0, None)
    # planes lifted far above zero: most minima are positive and must be gated out (c <= 0.8 peak = 0)
    cases["offset 64x21"] = ([p + np.float32(120.0) for p in dense_planes(oracle, 64, 21, 11)], 0.0, 10.0, 1.0, None)
    on = H.step_field(6, 960, 640)[::10, ::10] > 0        # flats of exact zeros outside the rectangles, integer ties inside
    cases["steps 96x64"] = ([(np.rint(p) * on).astype(np.float32) for p in dense_planes(oracle, 96, 64, 21)], 0.0, 10.0, 1.0, None)
    cur, dn, up = R.saddle_dogs(2)
    cases["saddle"] = ([dn, cur, up], 0.0, 10.0, 1.0, None)
    for xper in (1.0, 2.0):
        w, h = 160, 120
        mw, mh = int(w * xper), int(h * xper)
        yy, xx = np.mgrid[0:mh, 0:mw]
        mask = (((xx // 7) + (yy // 5)) % 3 != 0).astype(np.float32)          # many edges, at odd and even mask columns
        mask[:, -mw // 4:] = 0.5
        cases["masked xper %g" % xper] = (dense_planes(oracle, w, h, 9), 0.0, 10.0, xper, mask)
    cur, dn, up = R.wide_exponent_dogs(1)
    cases["wide exponent"] = ([dn, cur, up], 0.0, 10.0, 1.0, None)
    return cases


def _levels_of(dogs):
    return range(len(dogs) - 2)


def check_detection(oracle, mutant=None, names=None):
    sigma0 = oracle.sift_params(1920, 1080).sigma_0
    ok, worst, fig = True, 0.0, {}
    for name, (dogs, peak, edge, xper, mask) in detection_cases(oracle).items():
        if names is not None and name not in names:
            continue
        models = []
        for l in _levels_of(dogs):
            lvl = 1 if len(dogs) == 3 else l
            ref = oracle.find_keypoints(dogs[l + 1], dogs[l], dogs[l + 2], peak, edge, xper, sigma0, 3, lvl, mask=mask)
            m = R.detect64(dogs[l + 1], dogs[l], dogs[l + 2], peak, edge, xper, sigma0, 3, lvl, mask, mutant)
            bad, r, _ = R.dense_outside(m, ref)
            lbad, lr, _ = R.list_outside([m], oracle.compact_keypoints(ref))
            ok &= bad == 0 and lbad == 0
            worst = max(worst, r, lr)
            models.append(m)
        if mutant is None:
            share = R.fragile_share(models)
            n_acc = sum(int((m["accepted"] & ~m["fragile"]).sum()) for m in models)
            fig[name] = share
            assert share <= FRAGILE_CAP, (name, share)
            # floor from the model's own count on such content: dense planes hold an accepted extremum per ~15 interior pixels of
            # a searched plane (one per 30 is asked for; half of that behind the mask, which keeps half the plane, behind a peak
            # threshold or a sign gate that keeps half the candidates, and on the step planes, half of which are flat), a real octave at sigma 2 one per ~1000 (one per 2000 asked for); the spike planes 80
            h, w = np.asarray(dogs[0]).shape
            per = 2000 if name.endswith("320x200") else 60 if (mask is not None or peak > 0 or name[:5] in ("steps", "offse")) else 30
            floor = 80 if name in ("wide exponent", "saddle") else 3 * (w - 2) * (h - 2) // per
            assert n_acc >= max(floor, 3), (name, n_acc, floor)
    fig["keypoints"] = worst
    return ok, fig


def check_frame(oracle, mutant=None):
    """The whole frame: the model's octave-by-octave list on the oracle's DoG planes against the oracle's frame driver."""
    ok, worst, fig = True, 0.0, {}
    for w, h in ((320, 200), (250, 131)):
        frame = H.blurred_frame(0, w, h)
        models = frame_models(oracle, frame, mutant)
        ref = oracle.sift_detect_describe(frame, 16384)
        bad, r, nfr = R.list_outside(models, ref["kpts"])
        ok &= bad == 0
        worst = max(worst, r)
        if mutant is None:
            fig["fragile_%dx%d" % (w, h)] = R.fragile_share(models)
            assert R.fragile_share(models) <= FRAGILE_CAP
            assert sum(int((m["accepted"] & ~m["fragile"]).sum()) for m in models) >= (w * h) // 400
    fig["frame"] = worst
    return ok, fig


def frame_planes(oracle, frame):
    """The DoG planes of every octave of a frame, built by the oracle's stages (INPUT planes of the detection model)."""
    h, w = frame.shape
    p = oracle.sift_params(w, h)
    base = oracle.convolve(frame, *oracle.create_kernel_for_sigma(p.base_smooth))[0]
    out = []
    for o in range(p.num_octaves):
        ow, oh = w >> o, h >> o
        levels, dogs, _ = oracle.octave_pyramid(base, w, h, want_grad=False)
        out.append(dogs)
        if o + 1 < p.num_octaves:
            base = oracle.downsample2(levels[3], ow >> 1, oh >> 1)
    return out, p


def frame_models(oracle, frame, mutant=None, mask=None, peak=None, edge=None):
    planes, p = frame_planes(oracle, frame)
    octs = [R.octave_detect64(d, p.peak_threshold if peak is None else peak, p.edge_threshold if edge is None else edge,
                              float(2 ** o), p.sigma_0, 3, mask, mutant) for o, d in enumerate(planes)]
    return R.frame_list64(octs)


CHECKS = dict(params=check_params, taps=check_taps, convolve=check_convolve, exact=check_exact, gradient=check_gradient,
              chain=check_chain, detection=check_detection, frame=check_frame)

# which check sees which mutant (and, for the detection, on which cases it is looked for)
MUTANT_SEEN_BY = {
    "sigma_absolute": ("params", None), "radius_round": ("taps", None), "taps_unnormalised": ("taps", None),
    "border_replicate": ("convolve", None), "decimate_odd": ("exact", None), "dog_sign": ("exact", None),
    "grad_no_half": ("gradient", None), "angle_half_open": ("gradient", None),
    "extremum_ge": ("detection", ("steps 96x64",)), "no_sign_gate": ("detection", ("offset 64x21",)),
    "gate_at_peak": ("detection", ("peak 250x28",)), "edge_abs_det": ("detection", ("saddle",)),
    "offset_half": ("detection", ("blurred 320x200",)), "updn_fs": ("detection", ("blurred 320x200",)),
    "updn_fxs": ("detection", ("blurred 320x200",)), "updn_fys": ("detection", ("blurred 320x200",)),
    "sigma_no_div": ("detection", ("blurred 320x200",)), "sigma_no_xper": ("detection", ("masked xper 2",)),
    "v_no_half": ("detection", ("peak 250x28",)), "mask_no_half": ("detection", ("masked xper 2",)),
}


@pytest.mark.parametrize("stage", sorted(CHECKS))
def test_model_agrees_with_the_oracle_within_its_bounds(oracle, stage):
    ok, fig = CHECKS[stage](oracle)
    _report(stage, **fig)
    assert ok, (stage, fig)


def test_every_mutant_is_listed():
    assert set(MUTANT_SEEN_BY) == set(R.MUTANTS)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutant_is_rejected_by_the_check_the_model_passes(oracle, mutant):
    stage, names = MUTANT_SEEN_BY[mutant]
    ok, fig = CHECKS[stage](oracle, mutant, names) if names is not None else CHECKS[stage](oracle, mutant)
    assert not ok, "mutant %s passes the %s check: %s" % (mutant, stage, fig)


def test_chain_mutants_are_seen_by_the_chain_too(oracle):
    """The fused kernels expose no intermediates: the mutants of the scale-space constants must show in the chain check."""
    for mutant in ("sigma_absolute", "radius_round", "taps_unnormalised", "border_replicate", "dog_sign", "grad_no_half"):
        assert not check_chain(oracle, mutant)[0], mutant


def test_frame_mutants_are_seen_by_the_whole_frame_list(oracle):
    """The frame driver picks a candidate's planes by `lvl` and scales by the octave's xper: one wrong line there must show in the
    list of the whole frame."""
    for mutant in ("sigma_no_div", "sigma_no_xper", "updn_fs", "offset_half"):
        assert not check_frame(oracle, mutant)[0], mutant
    frame = H.blurred_frame(0, 320, 200)
    planes, p = frame_planes(oracle, frame)
    ref = oracle.sift_detect_describe(frame, 16384)["kpts"]
    # a level picked one too high (the planes of level l + 1 searched for level l) gives well-formed keypoints: not these
    octs = [[R.detect64(d[min(l + 2, 3)], d[min(l + 1, 2)], d[min(l + 3, 4)], 0.0, 10.0, float(2 ** o), p.sigma_0, 3, l)
             for l in range(3)] for o, d in enumerate(planes)]
    assert R.list_outside(R.frame_list64(octs), ref)[0] > 0
