"""Host logic of the matcher's ONE-GROUP plans (no GPU needed): what a pair runs under when a batched call gives every pair an
XCD of its own (pairs_share_xcds in nm_match.hip: make_plan_on(nA, nB, CUs / XCDs, 1, ...)), through the test entries
nm_sift_match_plan_on / nm_sift_match_plan_segments_on. Every invariant tests/test_abi.py::test_match_plan_invariants asserts
of the whole-chip plans, plus X == 1 and G <= n_wg: the grouped kernels cut a workgroup off with `vg >= plan.G`, vg < n_wg."""
import ctypes as C

import pytest

# (workgroups, XCDs) of one XCD's share: MI355X (256 CUs / 8 XCDs), a 304-CU part (38 per XCD), a half-sized partition
GEOMETRIES = [(32, 1), (38, 1), (16, 1)]
SHAPES = [(1, 1), (255, 127), (256, 128), (257, 129), (1000, 50), (50, 1000), (4096, 130), (300, 4000), (2049, 1500),
          (4096, 5000), (12223, 12080), (16384, 16384), (300, 100000)]
# the shapes of test_match_plan_invariants, for the cross-check of the two pairs of entries
OLD_SHAPES = [(1, 1), (255, 127), (256, 128), (257, 129), (1000, 50), (50, 1000), (12223, 12080), (16384, 16384),
              (300, 100000), (100000, 300), (100000, 12500), (4097, 8193), (4096, 3000), (5000, 20000)]
MAX_SEG = 4096


def _plan_on(lib, nA, nB, n_wg, n_xcd):
    out = (C.c_int * 10)()
    assert lib.nm_sift_match_plan_on(nA, nB, n_wg, n_xcd, out) == 0
    return list(out)


def _segments_on(lib, nA, nB, n_wg, n_xcd, wg):
    buf = (C.c_int * (5 * MAX_SEG))()
    n = lib.nm_sift_match_plan_segments_on(nA, nB, n_wg, n_xcd, wg, buf, MAX_SEG)
    assert 0 <= n <= MAX_SEG
    return [tuple(buf[5 * k: 5 * k + 5]) for k in range(n)]


@pytest.mark.parametrize("n_wg,n_xcd", GEOMETRIES)
def test_one_group_plan_invariants(nm, n_wg, n_xcd):
    lib = nm.lib()
    for nA, nB in SHAPES:
        qb, T, G, S, X, Gx, Tc, Cn, q_base, q_rem = _plan_on(lib, nA, nB, n_wg, n_xcd)
        what = (nA, nB, n_wg)
        assert qb == -(-nA // 256) and T == -(-nB // 128), what
        assert X == 1, what                                   # one group: the grouped kernels pass xg = 0
        assert 1 <= G <= n_wg, what                           # ... and leave with vg >= G, vg = block / XCDs < n_wg
        assert G == X * Gx and 1 <= S <= 64 and Cn == -(-T // Tc) and X * q_base + q_rem == qb, what
        assert (Tc, Cn, q_base, q_rem) == (T, 1, qb, 0), what   # the plain query-block-major order
        seen, slots, ends, per_wg = {}, {}, {}, []
        for wg in range(G):
            units = 0
            for (b, t0, n, slot, last) in _segments_on(lib, nA, nB, n_wg, n_xcd, wg):
                assert 0 <= b < qb and 0 <= t0 and n >= 1 and t0 + n <= T and 0 <= slot < S, what
                for t in range(t0, t0 + n):
                    assert (b, t) not in seen, what           # every (query block, tile) once
                    seen[(b, t)] = wg
                assert slot not in slots.setdefault(b, set()), what
                slots[b].add(slot)
                if last:
                    assert b not in ends and t0 + n == T, what
                    ends[b] = slot
                units += n
            per_wg.append(units)
        assert len(seen) == qb * T, what
        n_slots = 0
        for b in range(qb):
            assert slots[b] == set(range(len(slots[b]))) and ends[b] == max(slots[b]), (what, b)
            n_slots = max(n_slots, len(slots[b]))
        assert n_slots <= S <= 64, what
        assert max(per_wg) - min(per_wg) <= 1, what           # loads differ by at most one unit
        # workgroups past G have nothing to do
        for wg in (G, n_wg, 8 * n_wg):
            assert _segments_on(lib, nA, nB, n_wg, n_xcd, wg) == [], what
        # partial lists (nA * S * 20 B) stay inside what the workspace bound reserves for them (nA * 64 * 20 B)
        assert lib.nm_sift_match_workspace_bytes(nA, nB) >= nA * S * 20 + 4 * (nA + nB) + 4 * nA, what


def test_plan_entries_are_the_on_entries_at_the_device_geometry(nm):
    """nm_sift_match_plan / _plan_segments are nm_sift_match_plan_on / _segments_on called with the device's CUs and XCDs (256 / 8
    where there is no device): same plan, same segments."""
    lib = nm.lib()
    # the device's geometry, as the library sees it: a shape large enough for the XCD-grouped order names it (G = CUs, X = XCDs)
    probe = (C.c_int * 10)()
    assert lib.nm_sift_match_plan(100000, 12500, probe) == 0 and probe[4] > 1
    n_cu, n_xcd = probe[2], probe[4]
    grouped = 0
    for nA, nB in OLD_SHAPES:
        old = (C.c_int * 10)()
        assert lib.nm_sift_match_plan(nA, nB, old) == 0
        grouped += old[4] > 1
        assert _plan_on(lib, nA, nB, n_cu, n_xcd) == list(old), (nA, nB)
        for wg in (0, 1, old[2] // 2, old[2] - 1, old[2]):
            buf = (C.c_int * (5 * 256))()
            n = lib.nm_sift_match_plan_segments(nA, nB, wg, buf, 256)
            want = [tuple(buf[5 * k: 5 * k + 5]) for k in range(n)]
            assert _segments_on(lib, nA, nB, n_cu, n_xcd, wg) == want, (nA, nB, wg)
    assert grouped >= 4


def test_plan_on_rejects_what_the_plain_entries_reject(nm):
    lib = nm.lib()
    out = (C.c_int * 10)()
    buf = (C.c_int * 5)()
    for nA, nB, n_wg, n_xcd in [(1 << 22, 10, 32, 1), (10, 1 << 22, 32, 1), (-1, 5, 32, 1), (5, 5, 0, 1), (5, 5, 32, 0)]:
        assert lib.nm_sift_match_plan_on(nA, nB, n_wg, n_xcd, out) != 0
        assert lib.nm_sift_match_plan_segments_on(nA, nB, n_wg, n_xcd, 0, buf, 1) == -1
    assert lib.nm_sift_match_plan_on(5, 5, 32, 1, None) != 0
    assert lib.nm_sift_match_plan_segments_on(5, 5, 32, 1, -1, buf, 1) == -1
