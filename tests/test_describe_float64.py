"""The orientation and descriptor stages against the binary64 model of tests/describe_ref.py, with the CPU oracle in the
product's place (tests/test_gpu_describe_float64.py runs the same comparison on every kernel family). The model is written from the
reference's semantics and shares no code with the oracle or the kernels; the bounds are derived in its docstring, not measured.

Cases (the planes are gradients of a blurred-noise octave, built with the oracle; everything else is the model's):
  A  bulk: 300 random keypoints, borders included, every orientation radius 1..10, descriptor windows of 1, 2, 3 and 4+ diagonal
     chunks, windows clipped on both sides; 96 x 64 at xper 1 and 2, 61 x 45 (odd width) at xper 0.5
  B  clipping: keypoints in the corners and at the rims of a 200 x 20 plane (later diagonal chunks lie below the plane)
  C  rows that must not be processed
The teeth test shows that each one-line mutant of the model puts the oracle outside the bound on more than half of case A."""
import functools

import numpy as np
import pytest

import describe_ref as R
import helpers as H
import oracle_lib as O

NUM_DOGS = 3
GAUSS = 1.5
FRAGILE_CAP = 0.05
CASES_A = {"96x64-xper1": (96, 64, 1.0, 1), "96x64-xper2": (96, 64, 2.0, 2), "61x45-xper0.5": (61, 45, 0.5, 3)}
TEETH = "96x64-xper1"
C_SKIP_ORIENT = (3, 11, 12, 30, 47)                             # w = -1
C_SKIP_DESC = C_SKIP_ORIENT + (5, 20, 21) + (7, 25, 26, 40, 41)  # + level >= num_dogs, + pixel outside the plane


@functools.lru_cache(maxsize=None)
def plane(w, h):
    """Gradient planes (3, h, w, 2) of one blurred-noise octave. Read-only: shared by every test of both modules."""
    O.build()
    g = np.array(O.octave_pyramid(H.blurred_frame(3, w, h), 1920, 1080)[2], dtype=np.float32)
    g.setflags(write=False)
    return g


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def case_a(name):
    """(kp, ori, ow, oh, xper, model of the orientations, model of the descriptors); computed once, read-only."""
    w, h, xper, seed = CASES_A[name]
    g = plane(w, h)
    kp, ori = R.case_a_keypoints(g, w, h, xper, seed)
    kp.setflags(write=False), ori.setflags(write=False)
    return (kp, ori, w, h, xper, _freeze(R.orientations64(kp, g, w, h, GAUSS, xper)),
            _freeze(R.descriptors64(kp, ori, g, w, h, NUM_DOGS, xper)))


@functools.lru_cache(maxsize=None)
def case_b():
    w, h, xper = 200, 20, 1.0
    g = plane(w, h)
    kp, ori = R.case_b_keypoints(w, h, xper, 5)
    return (kp, ori, w, h, xper, _freeze(R.orientations64(kp, g, w, h, GAUSS, xper)),
            _freeze(R.descriptors64(kp, ori, g, w, h, NUM_DOGS, xper)))


@functools.lru_cache(maxsize=None)
def case_c():
    """(kp_orient, kp_desc, ori, ow, oh, xper, model of the orientations of kp_orient, model of the descriptors of kp_desc)."""
    w, h, xper = 96, 64, 2.0
    g = plane(w, h)
    kp_o, kp_d, ori = R.case_c_keypoints(g, w, h, xper, 7, NUM_DOGS)
    return (kp_o, kp_d, ori, w, h, xper, _freeze(R.orientations64(kp_o, g, w, h, GAUSS, xper)),
            _freeze(R.descriptors64(kp_d, ori, g, w, h, NUM_DOGS, xper)))


def fragile_share(model):
    return float(model["fragile"].sum()) / max(int(model["processed"].sum()), 1)


def assert_orientations(model, got, what, unset=-1.0):
    """Every processed, non-fragile keypoint of `got` within the model's bound; the figures are printed first."""
    c = R.compared(model)
    bad = R.orientations_outside(model, got, unset) & c
    s = (model["angles"] != -1.0) & c[:, None]
    dev = np.abs(np.asarray(got, np.float64) - model["angles"])[s] / model["bound"][s]
    print("%s: %d compared, %d fragile, worst deviation / bound %.3f" % (what, c.sum(), model["fragile"].sum(),
                                                                        dev.max() if dev.size else 0.0))
    assert c.sum() > 0 and not bad.any(), "%s: keypoints %s outside the bound" % (what, np.flatnonzero(bad)[:8])


def assert_descriptors(model, got, x, y, what):
    c = R.compared(model)
    bad = R.descriptors_outside(model, got) & c
    dev = np.abs(np.asarray(got, np.float64) - model["desc"])[c] / np.maximum(model["bound"][c], 1e-300)
    dev = np.where(model["bound"][c] > 0, dev, 0.0)
    print("%s: %d compared, %d fragile, worst deviation / bound %.3f" % (what, c.sum(), model["fragile"].sum(), dev.max()))
    assert c.sum() > 0 and not bad.any(), "%s: keypoints %s outside the bound" % (what, np.flatnonzero(bad)[:8])
    p = model["processed"]
    assert np.array_equal(np.asarray(x, np.float64)[p], model["x"][p]) and np.array_equal(np.asarray(y, np.float64)[p], model["y"][p])


def _oracle_outputs(kp, ori, w, h, xper):
    g = plane(w, h)
    return (O.detect_orientations(kp, g, w, h, GAUSS, xper),) + tuple(O.compute_sift_descriptors(kp, ori, g, w, h, NUM_DOGS, xper))


@pytest.mark.parametrize("name", list(CASES_A))
def test_case_a_reaches_what_it_is_for_and_stays_under_the_fragile_cap(name):
    kp, ori, w, h, xper, mo, md = case_a(name)
    assert mo["processed"].all() and md["processed"].all()
    assert set(mo["W"]) == set(range(1, 11))
    assert {1, 2, 3} <= set(md["chunks"]) and (md["chunks"] >= 4).any()
    assert md["clipped"].any() and (~md["clipped"]).any()
    assert (ori[:, 0] == -1).any() and (mo["angles"][:, 1] != -1).any() and (mo["angles"][:, 1] == -1).any()
    assert (md["nvotes"] > 0).any(1).all()
    print("fragile share: orientation %.4f, descriptor %.4f" % (fragile_share(mo), fragile_share(md)))
    assert fragile_share(mo) <= FRAGILE_CAP and fragile_share(md) <= FRAGILE_CAP
    assert md["coef"].max() <= R.C_D                        # the derived ceiling of the per-sample coefficient


@pytest.mark.parametrize("name", list(CASES_A))
def test_oracle_is_the_model_to_rounding_on_case_a(name):
    kp, ori, w, h, xper, mo, md = case_a(name)
    go, gd, gx, gy = _oracle_outputs(kp, ori, w, h, xper)
    assert_orientations(mo, go, "orientations " + name)
    assert_descriptors(md, gd, gx, gy, "descriptors " + name)


def test_case_b_windows_clipped_by_the_plane():
    kp, ori, w, h, xper, mo, md = case_b()
    assert mo["processed"].all() and md["processed"].all()
    assert fragile_share(mo) <= FRAGILE_CAP and fragile_share(md) <= FRAGILE_CAP
    assert md["clipped"].any()
    assert (md["chunks"] >= 3).any()                        # 16 (chunks - 1) > 20 rows: the later chunks lie below the plane
    go, gd, gx, gy = _oracle_outputs(kp, ori, w, h, xper)
    assert_orientations(mo, go, "orientations B")
    assert_descriptors(md, gd, gx, gy, "descriptors B")


def test_case_c_rows_that_must_not_be_processed():
    kp_o, kp_d, ori, w, h, xper, mo, md = case_c()
    assert np.array_equal(np.flatnonzero(~mo["processed"]), sorted(C_SKIP_ORIENT))
    assert np.array_equal(np.flatnonzero(~md["processed"]), sorted(C_SKIP_DESC))
    assert fragile_share(mo) <= FRAGILE_CAP and fragile_share(md) <= FRAGILE_CAP
    g = plane(w, h)
    go = O.detect_orientations(kp_o, g, w, h, GAUSS, xper)               # the binding pre-fills -1 / 0
    gd, gx, gy = O.compute_sift_descriptors(kp_d, ori, g, w, h, NUM_DOGS, xper)
    assert (go[~mo["processed"]] == -1).all()
    assert not gd[~md["processed"]].any() and not gx[~md["processed"]].any() and not gy[~md["processed"]].any()
    assert_orientations(mo, go, "orientations C")
    assert_descriptors(md, gd, gx, gy, "descriptors C")


def test_bounds_are_not_vacuous():
    """Median over descriptors of (largest element bound / largest element) and median angle bound on case A: a small multiple of
    u times the vote counts (module docstring of describe_ref)."""
    kp, ori, w, h, xper, mo, md = case_a(TEETH)
    rel = md["bound"].max(1) / np.abs(md["desc"]).max(1)
    votes = np.median(md["nvotes"].max(1))
    ang = mo["bound"][mo["angles"] != -1.0]
    print("median bound / max|d| %.3g (%.0f u), median of the largest vote count %d, median angle bound %.3g rad" % (
        np.median(rel), np.median(rel) / R.U, votes, np.median(ang)))
    assert 0 < np.median(rel) <= 2.0 * (votes + 8 * R.C_D) * R.U      # mass / value of an element is about 8: the mean trilinear factor
    assert 0 < np.median(ang) <= 2.0 ** -16


@pytest.mark.parametrize("mutant", R.ORIENT_MUTANTS + R.DESC_MUTANTS)
def test_teeth_every_mutant_of_the_model_is_caught(mutant):
    kp, ori, w, h, xper, _, _ = case_a(TEETH)
    g = plane(w, h)
    go, gd, gx, gy = _oracle_outputs(kp, ori, w, h, xper)
    if mutant in R.ORIENT_MUTANTS:
        m = R.orientations64(kp, g, w, h, GAUSS, xper, mutant=mutant)
        out = R.orientations_outside(m, go)
    else:
        m = R.descriptors64(kp, ori, g, w, h, NUM_DOGS, xper, mutant=mutant)
        out = R.descriptors_outside(m, gd)
    c = R.compared(m)
    share = float((out & c).sum()) / c.sum()
    print("%s: oracle outside the mutant's bound on %.3f of %d keypoints" % (mutant, share, c.sum()))
    assert share > 0.5
