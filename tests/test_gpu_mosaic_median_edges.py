"""The median composite's kernel on the inputs of tests/mosaic_edges_ref.py: nm_mosaic_median_dev against its host twin bit for
bit on all five outputs (canvas, weights as integers, support, label, counts), in both modes. The host twin is held to the
numpy model on the same arrays in tests/test_mosaic_edges_host.py.
  A  the 64 x 2 walk makes two full trips and a remainder (asserted against 8 workgroups per compute unit of the device),
     with stacks deeper than 10 and equal keys at the median; counts accumulate over more than two grids of workgroups;
  C  equal keys with distinct colours (two-way, across the median rank, all 64 frames), +0 against -0, subnormal and
     negative keys, keys of +-FLT_MAX, the weight limits, tau of 0, a subnormal, a key difference and infinity, frames 62
     and 63 alone, frames that are valid nowhere, counted frames at and above 32; the blur-edge scene with its records at
     the int limits, which must count nothing."""
import numpy as np
import pytest

import median_ref as M
import mosaic_edges_ref as E
from test_gpu_mosaic_median import run_dev, same

pytestmark = pytest.mark.gpu

MODES = (M.SELECT, M.MEAN)


def check(nm, cuda, case, mode, w_min, tau):
    tiles, recs, cap, cw, ch = case
    want = M.run_host(nm, tiles, recs, cap, cw, ch, mode, w_min=w_min, tau=tau)
    got = run_dev(nm, cuda, tiles, recs, cap, cw, ch, mode, w_min=w_min, tau=tau)
    same(got, want)
    pat = M.outputs(cw, ch, len(recs))
    off = ~E.median_written(tiles, recs, cw, ch, cap, w_min)
    assert not off.all()
    for g, p in zip(got[:4], pat[:4]):                   # no valid frame: every output keeps its contents
        assert np.array_equal(g[off], p[off])
    assert (got[2][~off] >= 1).all() and (got[0][..., 3][~off] == 255).all()
    return got


@pytest.mark.parametrize("mode", MODES)
def test_the_median_walk_makes_two_trips_and_a_remainder(nm, cuda, mode):
    import torch
    case = E.multi_trip_case()
    tiles, recs, cap, cw, ch = case
    G = 8 * torch.cuda.get_device_properties(cuda).multi_processor_count
    assert E.tile_counts(recs, cap, cw, ch)["median"] >= 2 * G + 1
    got = check(nm, cuda, case, mode, 0.75, 0.1)
    counts = got[4].reshape(-1, 2)
    assert not counts[[0, 20, 21, 22, 63]].any() and (counts[[1, 19, 23, 62], 0] > 0).all() and counts[32:, 1].any()
    on = E.median_written(tiles, recs, cw, ch, cap, 0.75)
    assert got[2][on].max() > 10                         # more than ten inliers somewhere: the deep stacks were reached


CASES = sorted(E.median_cases())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CASES)
def test_device_equals_the_host_twin_on_every_edge_case(nm, cuda, name, mode):
    case, w_min, tau, _ = E.median_cases()[name]
    got = check(nm, cuda, case, mode, w_min, tau)
    counts = got[4].reshape(-1, 2)
    if name.startswith("ties"):
        assert got[3][1, 2:8].tolist() == [0, 2, 3, 31, 62, 47] and (counts[:, 0] > 0).all()
    if name.startswith("keys"):
        assert not counts[13].any() and not counts[50].any() and got[3][1, 2 + 5] in (62, 63) and got[3][1, 2 + 7] == 47
    if name == "keys_subnormal_tau":
        assert got[2][1, 2 + 6] == 2 and counts[60, 1] >= 1
    if name.startswith("greys"):
        label, weight = E.EQUAL_GREYS_WANT[int(name[-1])]
        if mode == M.SELECT:
            assert (got[3][1:5, 1:10] == label).all() and (got[1][1:5, 1:10] == weight).all()
    if name == "blur_edges":
        n = len(case[1])
        assert not counts[n - E.EXTREME:].any() and (counts[:n - E.EXTREME, 0] > 0).all()
    if name == "tau_inf" and mode == M.MEAN:
        assert (got[2][1:5, 2:11] == 5).all() and not counts[:, 1].any()
