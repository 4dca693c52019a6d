"""The scene model of the loop-closure tests (tests/loop_closure_ref.py), without a GPU: the overlaps are two-sided, the
polygon overlap agrees with a raster count of the same warp, and the true pairwise maps compose round the loop to the identity."""
import numpy as np

import loop_closure_ref as L


def test_overlaps_are_two_sided():
    ov = L.overlaps()
    pairs = [(a, b) for a in range(L.K) for b in range(a + 1, L.K)]
    for a, b in pairs:                      # both directions of a pair on one side, nothing between the sides
        lo, hi = min(ov[(a, b)], ov[(b, a)]), max(ov[(a, b)], ov[(b, a)])
        assert lo >= L.HIGH or hi <= L.LOW, (a, b, lo, hi)
    high, low = L.high_pairs(ov), L.low_pairs(ov)
    assert len(high) + len(low) == len(pairs)
    assert all((k, k + 1) in high for k in range(L.K - 1))          # the sequence itself is linked
    closures = [(a, b) for a, b in high if b - a >= 2]
    assert (0, L.K - 1) in closures and len(closures) >= 2, closures
    assert len(low) >= 10, low
    assert any(0 < L.pair_overlap(a, b, ov) for a, b in low)        # a low pair that does share a strip


def test_overlap_equals_a_raster_count_of_the_same_warp():
    """the centres of a 2-pixel grid over frame a, warped by the true map and counted inside frame b: within 1 % of the frame"""
    A = L.view_maps()
    ys, xs = np.mgrid[0:L.VH:2, 0:L.VW:2]
    p = np.c_[xs.reshape(-1) + 1.0, ys.reshape(-1) + 1.0]
    worst = 0.0
    for a in range(L.K):
        for b in range(L.K):
            if a == b:
                continue
            q = L.apply(L.pair_map(a, b, A), p)
            inside = (q[:, 0] >= 0) & (q[:, 0] < L.VW) & (q[:, 1] >= 0) & (q[:, 1] < L.VH)
            worst = max(worst, abs(inside.mean() - L.overlap(a, b, A)))
    assert worst <= 0.01, worst
    assert L.overlap(0, 4, A) == 0.0 and abs(L.overlap(3, 3, A) - 1.0) < 1e-12


def test_pairwise_maps_compose_round_the_loop_to_the_identity():
    A = L.view_maps()
    M = np.eye(3)
    for k in range(L.K):
        M = L.pair_map(k, (k + 1) % L.K, A) @ M
    assert np.allclose(M / M[2, 2], np.eye(3), rtol=0, atol=1e-9), M
    assert np.array_equal(A[0], [[1, 0, L.ORIGIN_X], [0, 1, L.ORIGIN_Y], [0, 0, 1]])
    c = np.array([[0, 0], [L.VW, 0], [L.VW, L.VH], [0, L.VH]], float)
    corners = np.concatenate([L.apply(a, c) for a in A])            # the scene holds every view, with room for the sampler
    assert corners.min() >= 8 and corners[:, 0].max() <= L.SCENE_W - 8 and corners[:, 1].max() <= L.SCENE_H - 8
