"""The host twins of the exposure stages (nm_mosaic_exposure_sums_host, nm_mosaic_gains_host) on the cases of
tests/exposure_edges_ref.py, against the numpy model of tests/exposure_ref.py: sums as exact integers, gains within
exposure_ref.gain_bound where its condition holds (exposure_edges_ref.gain_bound_holds), end reasons, counts and exact unit
gains everywhere. The device test (tests/test_gpu_mosaic_exposure_edges.py) asks the device for the twins' bits on the same
cases; this file also checks, per 64 x 32 tile and on the CPU, the condition that makes the device's tile walk visible in N.

Mutants of csrc/nm_mosaic_exposure_math.hpp and csrc/nm_chol_math.hpp tried against this file (none kept; CHANGELOG.md has the
table): `>= min_pixels` -> `>` fails test_usability_boundary; `in_range` with `< hi`, `acc` from 0 and `i + 1 <= fw` fail
test_lattice_and_frame_edges (`acc` from 0 every tile-walk case too). The pivot test `v > 0` -> `v >= 0` and dropping the
isfinite sweep of the solution each survive alone and fail together (SINGULAR[2], whose pivot chain ends at exactly 0.0, and
the first sigma corner): a zero pivot divides the right-hand side by zero, the solution is not finite and the sweep ends
SINGULAR with the same outputs, so each guards the other's only case.
"""
import ctypes as C

import numpy as np
import pytest

import exposure_edges_ref as E
import exposure_ref as X
import test_mosaic_exposure_host as HT

F32 = np.float32
INVALID = 1


def _claims_its_lattice(c):
    assert E.lattice_of(c["fw"], c["fh"], c["stride"], c["L"]) == (c["lw"], c["lh"], c["tiles_x"], c["tiles"], c["parts"]), c["what"]


# ---- A ----
@pytest.mark.parametrize("k", range(len(E.WALK)), ids=E.WALK_IDS)
def test_tile_walk_shapes_count_in_every_tile(nm, k):
    c = E.walk_cases()[k]
    _claims_its_lattice(c)
    assert c["parts"] < c["tiles"] or c["tiles"] in (255, 256)            # a second step, or a size at which none may happen
    for masked in ((False, True) if c["masked"] else (False,)):
        want, least = E.model_sums(c, masked)
        got = nm.mosaic_exposure_sums_host(c["frames"], c["la"], c["lb"], c["H"], link_status=c["status"],
                                           mask=E.mask_of(c["fw"], c["fh"]) if masked else None, stride=c["stride"], lo=E.LO, hi=E.HI)
        assert got.tolist() == want, (c["what"], masked)
        if not masked:
            assert least > 0, (c["what"], least)                          # a skipped or doubled tile changes N
            plain = want
        else:
            assert all(0 < m[0] < p[0] for m, p in zip(want, plain) if p[0]), c["what"]
    for l in range(c["L"]):
        assert bool(plain[l][0]) == E.live(c, l), (c["what"], l)
    if c["L"] > 1:
        assert not all(E.live(c, l) for l in E.SLOTS.values()) and len({tuple(s) for s in plain}) >= E.DISTINCT + 1


# ---- B ----
def test_lattice_and_frame_edges(nm):
    seen = set()
    for c in E.edge_cases():
        want = E.edge_model(c)
        got = nm.mosaic_exposure_sums_host([c["A"], c["B"]], [0], [1], c["H"], stride=c["stride"], lo=c["lo"], hi=c["hi"])
        assert got.tolist() == [want], c["what"]
        N = want[0]
        if c["want"] is not None:
            assert N == c["want"], (c["what"], N)
        if c["what"].startswith("lattice"):
            assert (N > 0) == (c["fh"] > 1), c["what"]
            seen.add((c["fw"] // c["stride"], c["fh"] // c["stride"], c["stride"]))
        if c["what"].startswith("all 0"):
            assert N > 0 and want[1:] == [0] * 6, c["what"]
        if c["what"].startswith("all 255 "):
            assert (N > 0 and want[1:] == [255 * N] * 6) if c["hi"] == 255 else want == [0] * 7, c["what"]
            assert not float(c["H"][2]).is_integer()                       # fractional taps
        if c["what"].startswith("empty"):
            assert E.lattice_of(c["fw"], c["fh"], c["stride"], 1)[3] == 0
    assert seen == {(lw, lh, s) for lw in (63, 64, 65, 129) for lh in (1, 2, 3, 4, 5, 31, 32, 33) for s in (1, 3)}
    empties = [(c["fw"] // c["stride"], c["fh"] // c["stride"]) for c in E.edge_cases() if c["what"].startswith("empty")]
    assert empties == [(2, 0), (0, 2), (0, 0)]


# ---- C ----
def _solve(nm, c, mode, **kw):
    return nm.mosaic_gains_host(c["n"], c["la"], c["lb"], np.array(c["S"], np.uint64), mode=mode, **kw)


def _counts(c, kw):
    L = len(c["la"])
    st, mp = kw.get("link_status"), kw.get("min_pixels", 64)
    usable = [(st is None or st[l] == 1) and c["S"][l][0] >= mp for l in range(L)]
    frames = {f for l in range(L) if usable[l] for f in (c["la"][l], c["lb"][l])}
    return usable, sum(usable), len(frames)


@pytest.mark.parametrize("k", range(len(E.SINGULAR)))
def test_singular_inputs_end_singular_with_unit_gains(nm, k):
    c = E.SINGULAR[k]
    assert X.END_SINGULAR in c["ends"]
    for mode in (X.PER_CHANNEL, X.COMMON):
        g, stats = _solve(nm, c, mode, sigma_n=c["sn"], sigma_g=c["sg"])
        assert not np.isnan(g).any() and not np.isnan(stats).any()
        _, links, frames = _counts(c, {})
        assert (stats[6], stats[7], stats[8]) == (links, frames, c["ends"][mode]), (mode, stats)
        if c["ends"][mode] == X.END_SINGULAR:
            assert (g.view(np.uint32) == F32(1).view(np.uint32)).all() and stats[3:6].tolist() == stats[:3].tolist()
    if k == 0:
        assert stats.tolist() == [0, 0, 0, 0, 0, 0, 1, 2, 2]


@pytest.mark.parametrize("which", range(len(E.CORNER_SUMS)))
def test_sigma_corners_give_finite_gains_inside_the_clamp(nm, which):
    c = dict(n=3, la=[0, 1], lb=[1, 2], S=[E.CORNER_SUMS[which]] * 2)
    for (sn, sg), end in zip(E.CORNER_SIGMAS, E.CORNER_ENDS[which]):
        for mode in (X.PER_CHANNEL, X.COMMON):
            g, stats = _solve(nm, c, mode, sigma_n=sn, sigma_g=sg)
            assert np.isfinite(g).all() and np.isfinite(stats).all(), (sn, sg, mode)
            assert (g >= F32(0.25)).all() and (g <= F32(4)).all()
            assert (stats[6], stats[7], stats[8]) == (2, 3, end), (sn, sg, mode, stats)


@pytest.mark.parametrize("sn,sg", E.SIGMA_PAIRS)
def test_gains_within_the_bound_at_other_sigmas(nm, sn, sg):
    """gain_bound against solve_f64 only where gain_bound_holds: kappa 2^-53 (4 n (3 n + 1) + L + 4) < 2^-24"""
    assert E.gain_bound_holds(sn, sg, 64, 256) and not E.gain_bound_holds(1e-6, 1e6, 2, 1)
    for n, L, dead in ((5, 65, None), (64, 256, 17)):
        la, lb, S, _ = HT.synthetic_sums(n, L, 100 * n + L, dead_frame=dead, few=(1,))
        for mode in (X.PER_CHANNEL, X.COMMON):
            g, stats, ref, raw = HT.check_gains(nm, n, la, lb, S, mode, nm.mosaic_gains_host, sigma_n=sn, sigma_g=sg)
            assert stats[8] == X.END_OK


def test_usability_boundary(nm):
    for c in E.usability_cases():
        S = np.array(c["S"], np.uint64)
        for mode in (X.PER_CHANNEL, X.COMMON):
            g, stats, ref, raw = HT.check_gains(nm, c["n"], c["la"], c["lb"], S, mode, nm.mosaic_gains_host, **c["kw"])
            usable, links, frames = _counts(c, c["kw"])
            assert usable == c["usable"] and (stats[6], stats[7], stats[8]) == (links, frames, X.END_OK), (c["what"], stats)
            one = np.zeros(c["n"], bool)
            one[c["gains_one"]] = True
            assert (g[one].view(np.uint32) == F32(1).view(np.uint32)).all() and (g[~one] != 1).all(), (c["what"], g)
            assert frames == c["n"] - len(c["gains_one"])


def test_graph_shapes_at_64_frames(nm):
    for c in E.graph_cases():
        S = np.array(c["S"], np.uint64)
        for mode in (X.PER_CHANNEL, X.COMMON):
            if c["what"] == "Sa = Sb = 0":                    # both costs are 0 in the model: check_gains' relative cost
                g, stats = nm.mosaic_gains_host(c["n"], c["la"], c["lb"], S, mode=mode)      # comparison has no scale here
                assert not np.isnan(g).any() and not np.isnan(stats).any() and stats[:3].tolist() == [0.0] * 3
            else:
                g, stats, ref, raw = HT.check_gains(nm, c["n"], c["la"], c["lb"], S, mode, nm.mosaic_gains_host)
            _, links, frames = _counts(c, {})
            assert (stats[6], stats[7], stats[8]) == (links, frames, X.END_OK) and links == len(c["la"]), c["what"]
            dead = np.ones(c["n"], bool)
            dead[c["la"] + c["lb"]] = False
            assert (g[dead] == 1).all() and int(dead.sum()) == c["n"] - frames
            if c["what"] == "Sa = Sb = 0":                    # the data term vanishes: the prior alone, g = 1 within the bound
                assert (np.abs(g.astype(np.float64) - 1) <= X.gain_bound(np.ones((64, 3)), 64, 256)).all()
            elif c["what"] == "two live frames, 62 dead":
                assert int(dead.sum()) == 62 and (g[~dead] != 1).all()
            elif c["what"] == "256 links reversed":
                assert all(a > b for a, b in zip(c["la"], c["lb"]))


def test_one_frame_is_always_refused(nm):
    """links_ok wants L >= 1 and a != b, both indices in [0, n): with n = 1 no link list passes"""
    lib = nm.lib()
    A = np.full((8, 16, 4), 100, np.uint8)
    H = np.eye(3, dtype=F32).reshape(9)
    sums = np.full(14, 77, np.uint64)
    S = np.array([[100, 9000, 9000, 9000, 9900, 9900, 9900]] * 2, np.uint64)
    g, st = np.full(3, 7, F32), np.full(9, 7.0)
    ints = lambda v: (C.c_int * len(v))(*v)
    tab = (C.c_void_p * 1)(A.ctypes.data)
    for la, lb in (((0,), (0,)), ((0,), (1,)), ((1,), (0,)), ((0, 0), (0, 0)), ((-1,), (0,))):
        L = len(la)
        assert lib.nm_mosaic_exposure_sums_host(1, L, tab, ints(la), ints(lb), 16, 8, None, H.ctypes.data, None, 1, 5, 250,
                                                sums.ctypes.data) == INVALID
        assert lib.nm_mosaic_gains_host(1, L, ints(la), ints(lb), S.ctypes.data, None, 64, 10.0, 0.1, 0.5, 2.0, 0, g.ctypes.data,
                                        st.ctypes.data) == INVALID
        with pytest.raises(nm.NmError):
            nm.mosaic_gains_host(1, list(la), list(lb), S[:L])
    assert (sums == 77).all() and (g == 7).all() and (st == 7).all()
