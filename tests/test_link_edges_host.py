"""The link stages' host twins (nm_link_verify_host_f32, nm_link_refine_host_f32, nm_link_votes_host_u8, nm_link_rank_host)
against the numpy restatements on the cases of tests/link_edges_ref.py: lattices of exactly 255, 256, 257 and 512 tiles, tile
interior edges, the smallest and the widest frames the ABI admits, lattices empty in one axis, the horizon through the frame,
the gates at their thresholds, the vote scan for 17 to 63 frames. Every comparison is exact: integers by value, float64 and
float32 by their words. Every case first asserts the lattice it claims (`lattice_of`) and whether samples count.

The restatements are quick enough for every shape (the slowest, link_refine_ref.sums_ref on 64 x 8193, takes 1.5 s); whole
refinement calls are restated on 16385 x 2 and 16385 x 3, not on 64 x 8193, where the eight walks of the three pairs would
take 12 s.
"""
import numpy as np
import pytest

import link_edges_ref as E
import link_propose_ref as P
import link_refine_ref as R
import link_verify_ref as V
import test_link_refine_host as T
from test_link_refine_host import bits, count, same

F32 = np.float32
PHOTO = V.LOW_OVERLAP | V.LOW_NCC


def claims_its_lattice(c):
    """R2: the intended lattice, recomputed from (fw, fh, stride) with the entry points' formulas."""
    assert E.lattice_of(c["fw"], c["fh"], c["stride"]) == (c["lw"], c["lh"], c["tiles_x"], c["tiles"]), c["what"]
    assert all(a.shape == (c["fh"], c["fw"]) for a in ([c["A"]] if "A" in c else c["As"])), c["what"]


def verify_twin(nm, As, Bs, H, **kw):
    """(status, reason, stats, sums) of the twin and the restatement's, compared: status, reason and the seven sums by value,
    the eight stats bit for bit. Returns the twin's."""
    kw = dict(dict(min_overlap=nm.LINK_MIN_OVERLAP, min_ncc=nm.LINK_MIN_NCC), **kw)      # the restatement's defaults differ
    got = nm.link_verify_host(As, Bs, np.asarray(H, F32).reshape(len(As), 9), want_sums=True, **kw)
    per_pair = {k: kw[k] for k in ("status", "inliers") if kw.get(k) is not None}
    rest = {k: v for k, v in kw.items() if k not in ("status", "inliers")}
    for k in range(len(As)):
        extra = dict(status_in=per_pair["status"][k]) if "status" in per_pair else {}
        if "inliers" in per_pair:
            extra["inliers"] = per_pair["inliers"][k]
        want = V.verify_int(As[k], Bs[k], np.asarray(H, F32).reshape(-1, 9)[k], **rest, **extra)
        assert (int(got[0][k]), int(got[1][k])) == want[:2], (k, got[1][k], want[1])
        assert np.array_equal(bits(got[2][k]), bits(want[2])), (k, got[2][k], want[2])
        if want[1] != V.UNUSABLE:             # the sums entry has no status: it walks every pair with a finite map
            assert [int(v) for v in got[3][k]] == want[3], (k, got[3][k], want[3])
    assert np.isfinite(got[2]).all()
    return got


def refine_twin(nm, A, B, H, **kw):
    """The twin's whole call on one pair against refine_ref, bit for bit (`same` of tests/test_link_refine_host.py)."""
    H_out, st, stats = nm.link_refine_host([A], [B], np.asarray(H, F32).reshape(1, 9), **kw)
    want = R.refine_ref(A, B, H, **kw)
    assert same((H_out[0], st[0], stats[0]), want), (stats[0], want[2])
    assert np.isfinite(stats[0]).all() and np.isfinite(H_out[0]).all()
    return H_out[0], int(st[0]), stats[0]


def refine_sums(nm, A, B, H, mask, stride):
    """The twin's 67 sums of one walk against sums_ref, bit for bit; L and N by value."""
    got = T.sums_of(nm, A, B, H, mask=mask, stride=stride)
    want = R.sums_ref(A, B, np.asarray(H, F32).reshape(9), mask, stride)
    assert np.array_equal(bits(got), bits(want))
    assert got[R.S_L] == want[R.S_L] and count(got) == count(want)
    return got


# ---- A ----
def _walk(k):
    return E.walk_cases(T)[k]


@pytest.mark.parametrize("k", range(len(E.WALK)), ids=["%dx%d" % w[0][:2] for w in E.WALK])
def test_tile_walk_verification(nm, k):
    """n = 1, and n = 3 over three frames and maps with the middle pair unusable."""
    c = _walk(k)
    claims_its_lattice(c)
    got = verify_twin(nm, c["As"][:1], c["Bs"][:1], c["H"][:1], stride=c["stride"])
    assert got[3][0][1] > 0 and got[3][0][0] == c["lw"] * c["lh"]              # N > 0; every lattice pixel is in L
    got = verify_twin(nm, c["As"], c["Bs"], c["H"], stride=c["stride"], status=[1, 0, 1])
    assert got[1][1] == V.UNUSABLE and got[2][0][0] > 0 and got[2][2][0] > 0


@pytest.mark.parametrize("k", range(len(E.WALK)), ids=["%dx%d" % w[0][:2] for w in E.WALK])
def test_tile_walk_refinement_sums(nm, k):
    c = _walk(k)
    claims_its_lattice(c)
    for p in range(3):
        s = refine_sums(nm, c["As"][p], c["Bs"][p], c["starts"][0], None, c["stride"])
        assert s[R.S_L] == c["lw"] * c["lh"]
        assert count(s) > 0 if c["refine_counts"] else count(s) == 0


@pytest.mark.parametrize("k", [k for k, w in enumerate(E.WALK) if w[1][3] == 257], ids=lambda k: "%dx%d" % E.WALK[k][0][:2])
def test_tile_walk_refinement_of_three_pairs(nm, k):
    """Three pairs, four iterations, at 257 tiles: one pair refuses its first step (END_STEP), one converges after a few, one
    runs all four, so the later walks wrap while they read each pair's state and skip the ended ones. On 16385 x 2 no pixel
    has both vertical neighbours inside A, so N = 0 there by definition and every pair ends with END_FEW_PIXELS after a walk
    that counts L alone; 16385 x 3 is the 257-tile row on which the three ends differ."""
    c = _walk(k)
    claims_its_lattice(c)
    assert c["tiles"] == 257
    kw = dict(model=c["model"], stride=c["stride"], iterations=4, max_step=E.MAX_STEP)
    H_out, st, stats = nm.link_refine_host(c["As"], c["Bs"], c["starts"], **kw)
    ends, applied = stats[:, 8].astype(int).tolist(), stats[:, 6].astype(int).tolist()
    if c["refine_counts"]:
        assert ends == [R.END_CONVERGED, R.END_STEP, R.END_ITERATIONS], stats
        assert 2 <= applied[0] <= 3 and applied[1] == 0 and applied[2] == 4 and (stats[:, 0] > 0).all(), stats
    else:
        assert ends == [R.END_FEW_PIXELS] * 3 and (stats[:, 0] == 0).all() and (stats[:, 1] == c["lw"] * c["lh"]).all()
    if c["fw"] * c["fh"] < 100000:
        for p in range(3):
            want = R.refine_ref(c["As"][p], c["Bs"][p], c["starts"][p], **kw)
            assert same((H_out[p], st[p], stats[p]), want), (p, stats[p], want[2])


# ---- B ----
def test_tile_interior_edges(nm):
    cases = E.interior_cases(T)
    assert {(c["lw"], c["lh"]) for c in cases if c["stride"] == 1} == {(w, h) for w in (63, 64, 65, 128, 129) for h in (31, 32, 33)}
    assert {(c["fw"], c["fh"]) for c in cases if c["stride"] == 3} == {(3 * w + r, 3 * h + r) for r in (0, 2) for w in (64, 65)
                                                                        for h in (32, 33)}
    assert sum(c["mask"] is not None for c in cases) == 11
    for c in cases:
        claims_its_lattice(c)
        got = verify_twin(nm, [c["A"]], [c["B"]], c["H"], stride=c["stride"], mask=c["mask"])
        L, N = int(got[3][0][0]), int(got[3][0][1])
        assert 0 < N <= L and (L == c["lw"] * c["lh"] or c["mask"] is not None), c["what"]
        s = refine_sums(nm, c["A"], c["B"], c["H"], c["mask"], c["stride"])
        assert count(s) > 0 and s[R.S_L] == L, c["what"]
        _, st, stats = refine_twin(nm, c["A"], c["B"], c["H"], mask=c["mask"], model=R.HOMOGRAPHY, stride=c["stride"], iterations=2)
        assert st == 1 and stats[6] >= 1 and stats[0] > 0, (c["what"], stats)


# ---- C ----
def test_frame_extremes(nm):
    for c in E.extreme_cases(T):
        claims_its_lattice(c)
        A, B, H, stride = c["A"], c["B"], c["H"], c["stride"]
        got = verify_twin(nm, [A], [B], H, stride=stride)
        L, N, why = int(got[3][0][0]), int(got[3][0][1]), int(got[1][0])
        iterations = 3 if c["kind"] == "empty" else 2
        _, st, stats = refine_twin(nm, A, B, H, stride=stride, iterations=iterations, min_pixels=1)
        s = refine_sums(nm, A, B, H, None, stride)
        if c["kind"] == "none":
            # a side of one pixel: i + 1 >= fw or j + 1 >= fh rejects every sample. 2 x 2: pixel (0, 0) alone has its four taps
            # inside B, so the verification's N is 1 (ncc is 0 below two samples); the refinement's N is 0, no pixel has its
            # four neighbours
            assert (L, N) == (c["lw"] * c["lh"], int((c["fw"], c["fh"]) == (2, 2))) and L > 0, (c["what"], L, N)
            assert why & PHOTO == PHOTO and not why & V.BAD_GEOMETRY and got[2][0][3] == 0, c["what"]
            assert (st, stats[8], stats[0], stats[1]) == (0, R.END_FEW_PIXELS, 0, L), (c["what"], stats)
        elif c["kind"] == "some":
            assert L == c["lw"] * c["lh"] and 0 < N and count(s) > 0 and stats[0] > 0, (c["what"], L, N, stats)
        else:
            assert c["tiles"] == 0 and (c["lw"] == 0) != (c["lh"] == 0), c["what"]
            assert not got[3][0].any() and why & PHOTO == PHOTO and not s.any(), c["what"]
            assert (st, stats[8], stats[0], stats[1]) == (0, R.END_FEW_PIXELS, 0, 0), (c["what"], stats)
    kinds = [c["kind"] for c in E.extreme_cases(T)]
    assert kinds.count("none") == 4 and kinds.count("some") == 4 and kinds.count("empty") == 2


# ---- D ----
def test_horizon_through_the_frame(nm):
    for c in E.horizon_cases(T):
        A, B, H = c["A"], c["B"], c["H"]
        x, y = V.lattice(c["fw"], c["fh"], 1)
        den = V.project32(H, x.astype(F32), y.astype(F32))[0]
        assert int((den == 0).sum()) == c["zeros"] and (den > 0).sum() > 100 and (den < 0).sum() > 100, c["what"]
        got = verify_twin(nm, [A], [B], H, stride=1, min_overlap=0.0, min_ncc=-1.0)
        L, N = int(got[3][0][0]), int(got[3][0][1])
        assert L == 96 * 40 and 0 < N < int((den > 0).sum()), (c["what"], N)
        assert int(got[1][0]) == V.BAD_GEOMETRY, c["what"]                # the photometric gates are open: this bit alone
        for model in T.MODELS:
            refine_twin(nm, A, B, H, model=model, stride=1, iterations=3)
        s = refine_sums(nm, A, B, H, None, 1)
        assert 0 < count(s) < N and np.isfinite(s).all(), c["what"]


# ---- E ----
def test_gates_at_below_and_above(nm):
    seen = set()
    for c in E.gate_cases(T):
        got = verify_twin(nm, c["As"], c["Bs"], c["H"], **c["kw"])
        for k, want in enumerate(c["want"]):
            assert bool(got[1][k] & c["bit"]) == want, (c["what"], k, got[1][k])
            if c["only"]:
                assert got[1][k] == (c["bit"] if want else 0) and got[0][k] == int(not want), (c["what"], k, got[1][k])
            seen.add((c["bit"], want))
    assert seen == {(b, w) for b in (V.FEW_INLIERS, V.BAD_GEOMETRY, V.LOW_OVERLAP, V.LOW_NCC) for w in (False, True)}


# ---- F ----
@pytest.mark.parametrize("k", range(len(E.VOTE_SHAPES)), ids=["n%d-cap%d" % s for s in E.VOTE_SHAPES])
def test_votes_for_mid_sized_n(nm, k):
    c = E.vote_cases()[k]
    n, cap = E.VOTE_SHAPES[k]
    assert len(c["descs"]) == n and c["cap"] == cap and -(-cap // 256) == (2 if cap > 256 else 1)
    got, ref = nm.link_votes_host(c["descs"], c["counts"], ambiguity=c["amb"], cap=cap), E.model_votes(c)
    assert np.array_equal(got, ref), (c["what"], np.argwhere(got != ref)[:5])
    empty = [a for a, v in enumerate(c["counts"]) if v == 0]
    assert empty and (got[empty] == 0).all() and (got[:, empty] == 0).all() and got.sum() > 0 and (np.diag(got) == 0).all()
    if (n, cap) == (33, 257):                                             # a real vote matrix through the ranking
        kw = dict(min_votes=16, min_gap=2, per_frame=2, max_links=P.MAX_LINKS)
        la, lb, ls, cnt = nm.link_rank_host(got, **kw)
        ra, rb, rs, rcnt = P.rank(ref, **kw)
        assert cnt == rcnt and cnt > 0 and np.array_equal(la, ra) and np.array_equal(lb, rb) and np.array_equal(ls, rs)
