"""The issue order of a detect/describe call is chosen per call (nm_frame_resolve, niftymatch_amd/csrc/nm_frame_plan.hpp): what
nm_sift_set_frame_skew selected; else the cross order (2) for calls of at least NM_FRAME_CROSS_MIN_FRAMES frames and order 0 below
that -- and always order 0 where the call takes the octave tail or a split description, which own the description stream.
nm_sift_frame_resolve is that decision as a host function, with the switches as arguments; every configuration it hands out must
have a plan, and the plan must pass the hazard checks of tests/test_frame_plan.py."""
import ctypes as C

import pytest

import test_frame_plan as FP

OCTAVES = 6                     # a 1080p frame
THRESHOLDS = (0, 3, 4, 16, 64, 65)   # 0: never


def resolve(nm, n, octaves=OCTAVES, tail_first=0, selected=-1, split=0, cross_min=0):
    cfg = (C.c_int * 5)()
    assert nm.lib().nm_sift_frame_resolve(octaves, tail_first, n, selected, split, cross_min, cfg) == 0
    return dict(octaves=cfg[0], first_tail=cfg[1], split=cfg[2], dogs=cfg[3], order=cfg[4])


def sizes(threshold):
    return sorted({1, 2, 3, 64} | ({threshold - 1, threshold} if threshold > 1 else set()))


def plan_is_sound(nm, cfg):
    ops = FP.plan(nm, **cfg)
    assert ops, "no plan for the resolved configuration %r" % (cfg,)
    assert FP.check(ops, cfg["octaves"], cfg["first_tail"], cfg["split"], cfg["dogs"]) == [], cfg
    return ops


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_default_order_without_the_tail(nm, threshold):
    for n in sizes(threshold):
        cfg = resolve(nm, n, cross_min=threshold)
        assert cfg["first_tail"] == OCTAVES and cfg["split"] == 0
        assert cfg["order"] == (2 if threshold and n >= threshold else 0), (threshold, n)
        ops = plan_is_sound(nm, cfg)
        # the cross order is the one that uses the description stream for levels 4-5
        assert any(op[0] == FP.LEV and op[1] == FP.DESC for op in ops) == (cfg["order"] == 2)


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_default_order_with_the_tail(nm, threshold):
    """Arenas with an octave-tail plan from octave 2: calls of one or two frames take it, in order 0 whatever the threshold."""
    for n in sizes(threshold):
        cfg = resolve(nm, n, tail_first=2, cross_min=threshold)
        if n <= 2:
            assert (cfg["first_tail"], cfg["split"], cfg["order"]) == (2, 2, 0), (threshold, n)
        else:
            assert (cfg["first_tail"], cfg["split"]) == (OCTAVES, 0)
            assert cfg["order"] == (2 if threshold and n >= threshold else 0), (threshold, n)
        plan_is_sound(nm, cfg)


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("tail_first", [0, 2])
def test_a_split_description_keeps_order_0(nm, threshold, tail_first):
    """NM_FRAME_SPLIT_DESCRIBE=2 puts the early description on the description stream: no cross order, and no octave tail."""
    for n in sizes(threshold):
        for selected in (-1, 2):
            cfg = resolve(nm, n, tail_first=tail_first, selected=selected, split=2, cross_min=threshold)
            assert (cfg["first_tail"], cfg["split"], cfg["order"]) == (OCTAVES, 2, 0), (threshold, n, selected)
            plan_is_sound(nm, cfg)


@pytest.mark.parametrize("threshold", THRESHOLDS)
def test_a_selected_order_overrides_the_threshold(nm, threshold):
    for n in sizes(threshold):
        for selected in (0, 1, 2):
            cfg = resolve(nm, n, selected=selected, cross_min=threshold)
            assert cfg["order"] == selected, (threshold, n, selected)
            plan_is_sound(nm, cfg)
            tail = resolve(nm, n, tail_first=2, selected=selected, cross_min=threshold)
            assert tail["order"] == (0 if n <= 2 else selected)
            plan_is_sound(nm, tail)


@pytest.mark.parametrize("octaves", [1, 2, 3, 5, 6, 8, 20])
def test_every_resolved_configuration_is_hazard_free(nm, octaves):
    seen = set()
    for tail_first in (0, 1, 2, 3):
        for split in (0, 1, 2, 3):
            for selected in (-1, 0, 1, 2):
                for threshold in (0, 3, 16):
                    for n in (1, 2, 3, 15, 16, 64):
                        cfg = resolve(nm, n, octaves, tail_first, selected, split, threshold)
                        key = tuple(sorted(cfg.items()))
                        if key not in seen:
                            seen.add(key)
                            plan_is_sound(nm, cfg)
    assert len(seen) >= 3


def test_the_process_threshold_is_what_the_default_follows(nm):
    """With the process's own switches (arguments < 0) the decision follows nm_sift_frame_cross_min_frames()."""
    threshold = nm.lib().nm_sift_frame_cross_min_frames()
    assert threshold >= 0
    for n in sizes(threshold):
        want = resolve(nm, n, cross_min=threshold, split=-1)
        assert resolve(nm, n, cross_min=-1, split=-1) == want, (threshold, n)


def test_out_of_range_arguments(nm):
    cfg = (C.c_int * 5)()
    for args in ((0, 0, 1), (21, 0, 1), (6, 0, 0), (6, -1, 1)):
        assert nm.lib().nm_sift_frame_resolve(args[0], args[1], args[2], -1, 0, 0, cfg) != 0, args
    assert nm.lib().nm_sift_frame_resolve(6, 0, 1, -1, 0, 0, None) != 0
