"""The CPU oracle's RANSAC (oracle/nmo_ransac.h, the bit-exact twin of csrc/nm_ransac_math.hpp) against an independent float64
reference (tests/ransac_ref.py): fit accuracy, inlier counts, degenerate inputs and recovery of a known map. No GPU.

Fit errors are measured in float64 over ransac_ref.sweep(model, W, H): seven motions (mild, strong perspective, rotations of
90 and 180 degrees, scales 0.25 and 4, negative destinations), 1500 correspondences with 0.7 px noise and 40 % outliers,
400 samples each. Backward error: the largest distance between a hypothesis applied to its own sample and the sample's
destinations (ideal value 0: all three fits interpolate). Forward error: the largest distance between where the hypothesis
and the float64 fit send the four frame corners, divided by the sample's conditioning sigma[0] / sigma[-2]. Both are
asserted where the float64 side calls the sample usable (ransac_ref.WELL_POSED, RESOLVABLE, HORIZON give the reasons).

The limits are 8 x the maxima of an independent float32 implementation (the same DLT and closed forms in numpy float32
with LAPACK's SVD) over the same samples, in pixels:

    model        frame        LAPACK float32 maxima      limits (8 x)          this oracle, when recorded
                              backward    forward/k      backward   forward/k  backward   forward/k
    translation  640x480      6.82e-05    6.82e-05       5.46e-04   5.46e-04   6.82e-05   6.82e-05
    translation  1920x1080    2.46e-04    2.46e-04       1.97e-03   1.97e-03   2.46e-04   2.46e-04
    translation  3840x2160    2.73e-04    2.73e-04       2.18e-03   2.18e-03   2.73e-04   2.73e-04
    translation  7680x4320    5.46e-04    5.46e-04       4.37e-03   4.37e-03   5.46e-04   5.46e-04
    similarity   640x480      1.30e-03    9.60e-04       1.04e-02   7.68e-03   3.67e-03   2.36e-03
    similarity   1920x1080    3.05e-03    3.46e-03       2.44e-02   2.77e-02   6.97e-03   5.54e-03
    similarity   3840x2160    1.04e-02    1.20e-02       8.32e-02   9.60e-02   1.33e-02   1.06e-02
    similarity   7680x4320    1.09e-02    1.30e-02       8.72e-02   1.04e-01   1.69e-02   2.05e-02
    homography   640x480      4.65e-04    1.83e-03       3.72e-03   1.46e-02   9.48e-04   3.42e-03
    homography   1920x1080    1.32e-03    4.26e-03       1.06e-02   3.41e-02   3.36e-03   3.83e-03
    homography   3840x2160    2.82e-03    1.40e-02       2.26e-02   1.12e-01   7.98e-03   6.30e-03
    homography   7680x4320    5.79e-03    2.08e-02       4.63e-02   1.66e-01   1.24e-02   9.63e-03

(the last two columns are context, not limits: the Jacobi's worst case is 2.8 x LAPACK's). The similarity's figures exceed
the homography's because its scale-4 motion puts destinations near 30 000 px at 8K, where one float32 ulp is 2e-3 px.
"""
import numpy as np
import pytest

import ransac_ref as R

MODELS = [0, 1, 2]
NAMES = {0: "translation", 1: "similarity", 2: "homography"}


def _pts(sc):
    return sc["sx"], sc["sy"], sc["dx"], sc["dy"]


def test_reference_fits_known_maps():
    """fit64 on samples of the true maps returns them (to float32 input rounding), and tells degenerate samples apart."""
    for model in MODELS:
        for motion in R.MOTIONS:
            sc = R.scene(model, 1920, 1080, 400, 0.0, 0.0, 3, motion)
            rl = R.sample_lists(400, 50, model, 9)
            H64, sig = R.fit64(model, *R.gather(sc, rl))
            ok = ~R.skipped(rl) & (1 / R.conditioning(sig) >= 0.02)
            assert ok.sum() >= 8
            assert np.nanmax(R.corner_distance64(H64[ok], sc["M"], 1920, 1080)) < 0.05, (model, motion)
            assert np.nanmax(R.backward_error64(H64[ok], tuple(a[ok] for a in R.gather(sc, rl)))) < 1e-6
    x = np.array([[0.0, 100, 200, 300], [0, 100, 0, 100]])
    y = np.array([[0.0, 50, 100, 150], [0, 0, 100, 100]])
    d = np.array([[5.0, 70, 300, 20], [5, 70, 300, 20]])
    _, sig = R.fit64(2, x, y, d, d[:, ::-1])
    k = R.conditioning(sig)
    assert k[0] > 1e12 and k[1] < 1e3                       # four collinear sources against a square


@pytest.mark.parametrize("W,Hh", R.FRAMES)
@pytest.mark.parametrize("model", MODELS)
def test_oracle_fits_and_counts_against_float64(oracle, model, W, Hh):
    lim_b, lim_f = R.limits(model, W, Hh)
    worst = dict(lapack_b=0.0, lapack_f=0.0, oracle_b=0.0, oracle_f=0.0, share=0.0)
    checked = 0
    for motion, sc, rl in R.sweep(model, W, Hh):
        smp = R.gather(sc, rl)
        valid = int((sc["sx"] >= 0).sum())
        # the float64 side alone: its own fits, rounded to float32, leave at most 1 % of the pairs undecided
        H64, _ = R.fit64(model, *smp)
        fin = ~R.skipped(rl) & np.isfinite(H64).all(axis=(1, 2))
        lo, hi, _, _ = R.inlier_bracket64(H64[fin].astype(np.float32).reshape(-1, 9), *_pts(sc), R.SWEEP_THR)
        share = R.undecided_share(lo, hi, valid)
        assert share <= 0.01, (motion, share)
        worst["share"] = max(worst["share"], share)
        # the yardstick on this machine's LAPACK
        H32, _ = R.fit_lapack32(model, *smp)
        b, f = R.fit_errors(model, H32.reshape(-1, 9), sc, rl)
        assert np.isfinite(b).all() and np.isfinite(f).all(), motion
        worst["lapack_b"], worst["lapack_f"] = max(worst["lapack_b"], b.max()), max(worst["lapack_f"], f.max())
        # the oracle
        pos, Hb, Ha, inl = oracle.ransac(model, *_pts(sc), rl, R.SWEEP_THR)
        b, f = R.fit_errors(model, Ha, sc, rl)
        checked += len(b)
        assert np.isfinite(b).all() and np.isfinite(f).all(), motion
        worst["oracle_b"], worst["oracle_f"] = max(worst["oracle_b"], b.max()), max(worst["oracle_f"], f.max())
        print("%s %dx%d %-11s backward %.3g (limit %.3g)  forward/k %.3g (limit %.3g)  undecided %.2g" % (
            NAMES[model], W, Hh, motion, b.max(), lim_b, f.max(), lim_f, share))
        assert b.max() <= lim_b, (motion, b.max(), lim_b)
        assert f.max() <= lim_f, (motion, f.max(), lim_f)
        R.check_call(model, _pts(sc), rl, R.SWEEP_THR, (pos, Hb, Ha, inl), "%s %dx%d %s" % (NAMES[model], W, Hh, motion))
    print("%s %dx%d: %s over %d well-posed samples" % (NAMES[model], W, Hh, worst, checked))
    assert checked >= 1000
    # the yardstick itself has not moved: another LAPACK build stays within the margin of its recorded maxima
    assert worst["lapack_b"] <= lim_b and worst["lapack_f"] <= lim_f, worst


@pytest.mark.parametrize("model", MODELS)
def test_oracle_degenerate_catalogue(oracle, model):
    cases, dead = R.catalogue(model)
    clean = None
    for name, pts, rl, thr, base in cases:
        res = oracle.ransac(model, *pts, rl, thr)
        R.check_call(model, pts, rl, thr, res, name)
        pos, Hb, Ha, inl = res
        if name == "clean":
            clean = (Ha.copy(), inl.copy())
            assert np.isfinite(Ha).all() and inl.min() > 100         # the well-posed samples are what they claim to be
        assert np.array_equal(Ha[base].view(np.uint32), clean[0].view(np.uint32)), name + ": a well-posed hypothesis changed"
        if thr == 4.0 and "[" not in name:
            assert np.array_equal(inl[base], clean[1]), name
        if name == "repeated index":
            other = np.setdiff1d(np.arange(len(rl)), base)
            assert len(other) and not Ha[other].any() and not inl[other].any()
    if len(dead):
        pts = cases[0][1]
        pos, Hb, Ha, inl = oracle.ransac(model, *pts, dead, 4.0)
        R.check_call(model, pts, dead, 4.0, (pos, Hb, Ha, inl), "all unusable")
        assert not inl.any() and pos == 0 and not np.isfinite(Hb).all()
        assert (~np.isfinite(Ha).all(axis=1) | R.skipped(dead)).all()


@pytest.mark.parametrize("outliers", [0.0, 0.5, 0.8])
@pytest.mark.parametrize("W,Hh", [(1920, 1080), (7680, 4320)])
@pytest.mark.parametrize("model", MODELS)
def test_oracle_recovers_the_true_map(oracle, model, W, Hh, outliers):
    thr = 4.0
    motion = "perspective" if model == 2 else "rot90" if model == 1 else "negative"
    sc = R.scene(model, W, Hh, 1000, outliers, 0.0, 31 + model, motion)
    its = max(64, R.iterations_for(1.0 - outliers, R.SAMPLES[model]))
    assert its < R.MAX_ITERATIONS
    rl = R.sample_lists(1000, its, model, 8)
    R.assert_recovery(model, sc, rl, thr, oracle.ransac(model, *_pts(sc), rl, thr))
