"""nm_sift_match_guided_batch_dev_f32 on the MI355X on adversarial gate-HIT PATTERNS (tests/guided_hits_ref.py: a lane that
owns a whole chunk beside lanes with partly filled lists, every hit count around the list length, hits on the last candidate
of a tile and the first of the next with a list pending, the nearest candidate in the rounded-up last chunk, every order the
scan can meet, ragged row counts with invalid rows beside the burst, a wave in lockstep beside a wave of single hits).
Everything is array_equal against the host twin: result, count and the bits of best, one pair per call in 300 x 1100 buffers,
result, best_distance and count sentinel-filled before the call (the C entry, through ctypes). No tolerance, no excluded row.
The two batch tests also run on the families' integer descriptors cast to bytes, through nm_sift_match_guided_u8_batch_dev
against the u8 host twin: both entries are one kernel template and share the gate loop. Which of these patterns can see which slip of the
schedule is measured on the CPU, in test_match_guided_hits_host.py, where the host twin is held to guided_ref.guided.
"""
import ctypes as C

import numpy as np
import pytest

import guided_hits_ref as R

pytestmark = pytest.mark.gpu

OUT = ("result", "count", "best")
_HOST = {}


def _u32(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _upload(cases, dev):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return [dict(A=t(c["A"]), ax=t(c["ax"]), ay=t(c["ay"]), B=t(c["B"]), bx=t(c["bx"]), by=t(c["by"]),
                 nA=t(np.array([c["nA"]], np.int32)), nB=t(np.array([c["nB"]], np.int32))) for c in cases]


SENTINEL = -7


def _bytes(c):
    """The case on byte descriptors: its rows are small integers in [0, 255] held in float32."""
    q = dict(c)
    for key in ("A", "B"):
        assert c[key].min() >= 0 and c[key].max() <= 255 and np.array_equal(c[key], np.rint(c[key]))
        q[key] = c[key].astype(np.uint8)
    return q


ELEMS = pytest.mark.parametrize("u8", [False, True], ids=["fp32", "u8"])


def _device(nm, cases, dev, run, up=None, u8=False):
    """One call of the C entry (u8: of the u8 entry, `cases` / `up` then hold byte descriptors) on the pairs `cases`.
    result, best_distance and count are all made here and start filled
    with SENTINEL (no result is below -1, no distance below 0, no count below 0), and none may be left: a row or a count that
    the call does not write shows, whatever an earlier call left in the memory."""
    import torch
    r2, amb, maxd = run
    n = len(cases)
    up = _upload(cases, dev) if up is None else up
    Hd = torch.from_numpy(np.stack([c["H"] for c in cases])).to(dev)
    st = torch.from_numpy(np.array([c["status"] for c in cases], np.int32)).to(dev)
    res = [torch.full((R.CAP_A,), SENTINEL, dtype=torch.int32, device=dev) for _ in cases]
    best = [torch.full((R.CAP_A,), float(SENTINEL), dtype=torch.float32, device=dev) for _ in cases]
    count = torch.full((n,), SENTINEL, dtype=torch.int32, device=dev)
    arr = lambda ptrs: (C.c_void_p * n)(*ptrs)
    tab = lambda key: arr([u[key].data_ptr() for u in up])
    assert all(u["A"].dtype == u["B"].dtype == (torch.uint8 if u8 else torch.float32) for u in up)
    entry = nm.lib().nm_sift_match_guided_u8_batch_dev if u8 else nm.lib().nm_sift_match_guided_batch_dev_f32
    rc = entry(n, tab("A"), tab("ax"), tab("ay"), tab("nA"), R.CAP_A, tab("B"), tab("bx"),
               tab("by"), tab("nB"), R.CAP_B, Hd.data_ptr(), st.data_ptr(), r2, amb, maxd,
               arr([r.data_ptr() for r in res]), count.data_ptr(),
               arr([b.data_ptr() for b in best]), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    out = dict(result=np.stack([r.cpu().numpy() for r in res]), count=count.cpu().numpy(),
               best=np.stack([b.cpu().numpy() for b in best]))
    for k in OUT:
        assert not (out[k] == SENTINEL).any(), (k, "left unwritten", np.argwhere(out[k] == SENTINEL)[:8].tolist())
    return out


def _host(nm, cases, run, u8=False):
    """The host twin's answer (u8: the u8 host twin's, on byte descriptors), computed once per (cases, run, u8)."""
    key = (tuple(c["what"] for c in cases), run, u8)
    if key not in _HOST:
        r2, amb, maxd = run
        k = lambda name: [c[name] for c in cases]
        assert all(c["A"].dtype == c["B"].dtype == (np.uint8 if u8 else np.float32) for c in cases)
        twin = nm.sift_match_guided_u8_host if u8 else nm.sift_match_guided_host
        out = twin(k("A"), k("ax"), k("ay"), k("nA"), k("B"), k("bx"), k("by"), k("nB"), np.stack(k("H")),
                   status=np.array(k("status"), np.int32), radius2=r2, ambiguity=amb, max_distance=maxd,
                   capA=R.CAP_A, capB=R.CAP_B, want_distance=True)
        _HOST[key] = dict(zip(OUT, out))
    return _HOST[key]


def _assert_same(got, want, what):
    for k in OUT:
        assert np.array_equal(_u32(got[k]), _u32(want[k])), (what, k, np.argwhere(_u32(got[k]) != _u32(want[k]))[:8].tolist())
    assert np.array_equal((got["result"] >= 0).sum(axis=1), got["count"]), (what, "count")


@pytest.mark.parametrize("family", R.FAMILIES)
def test_device_equals_host_twin(nm, cuda, family):
    matched = 0
    for c in R.family_cases(family):
        up = _upload([c], cuda)
        for run in c["runs"]:
            got = _device(nm, [c], cuda, run, up=up)
            _assert_same(got, _host(nm, [c], run), (c["what"], run))
            assert (got["result"][0][c["nA"]:] == -1).all() and np.isinf(got["best"][0][c["nA"]:]).all(), c["what"]
            matched += int(got["count"][0])
            if family == "scan_order":                          # and outright, row by row
                for (row, r), (j, m1) in c["expected"].items():
                    if r == run:
                        assert (got["result"][0][row], got["best"][0][row]) == (j, m1), (c["what"], row, run)
    assert matched > 0, "nothing matched: the comparison covered nothing"


@ELEMS
def test_ragged_batch_of_mixed_families(nm, cuda, u8):
    """16 pairs in one call: the families mixed across the slots, one pair empty, one with status 0, one with nB = 1033.
    u8: the same pairs on byte descriptors through the u8 entry, against the u8 host twin."""
    batch = [_bytes(c) for c in R.ragged_batch()] if u8 else R.ragged_batch()
    up = _upload(batch, cuda)
    for run in ((R.R2, 0.8, np.inf), (R.R2, 1.5, np.inf)):
        got = _device(nm, batch, cuda, run, up=up, u8=u8)
        _assert_same(got, _host(nm, batch, run, u8), ("ragged batch", run, u8))
        assert got["count"][5] == got["count"][9] == 0 and (got["result"][[5, 9]] == -1).all() and np.isinf(got["best"][[5, 9]]).all()
    # tile_edge's nearest two are 100 and 120: matches above a ratio of 0.83 only, so the 1033 pair is counted at 1.5
    assert any(c["nB"] == 1033 and got["count"][p] >= 3 for p, c in enumerate(batch))


@ELEMS
def test_second_launch_and_last_slot_of_the_first(nm, cuda, u8):
    """33 pairs: chunk_burst in slot 32, the first slot of the second launch, tile_edge in slot 31; each equals its result
    alone in a one-pair call. u8: the same pairs on byte descriptors through the u8 entry, against the u8 host twin."""
    burst, edge, filler = R.family_cases("chunk_burst")[0], R.family_cases("tile_edge")[3], R.family_cases("shared_point")[0]
    if u8:
        burst, edge, filler = _bytes(burst), _bytes(edge), _bytes(filler)
    run = (R.R2, 1.5, np.inf)                                   # (tile_edge's nearest two, 100 and 120, match above 0.83 only)
    pairs = [filler] * 31 + [edge, burst]
    up = _upload([filler, edge, burst], cuda)
    got = _device(nm, pairs, cuda, run, up=[up[0]] * 31 + [up[1], up[2]], u8=u8)
    _assert_same(got, _host(nm, pairs, run, u8), ("33 pairs", u8))
    for slot, c in ((32, burst), (31, edge), (0, filler), (30, filler)):
        alone = _device(nm, [c], cuda, run, u8=u8)
        for k in OUT:
            assert np.array_equal(_u32(got[k][slot]), _u32(alone[k][0])), (slot, c["what"], k)
    assert got["count"][32] > 0 and got["count"][31] > 0


def test_permuted_candidates_map_back(nm, cuda):
    """Metamorphic: shuffling the candidates inside [0, nB) maps the matches through the permutation on every row that is
    sure of its answer, and leaves best bit-identical on every row."""
    def matcher(case, run):
        got = _device(nm, [case], cuda, run)
        return got["result"][0], int(got["count"][0]), got["best"][0]
    moved = sum(R.assert_maps_back(c, matcher) for c in R.permuted_picks())             # one case per family; all on the host
    assert moved > 0, "the permutations moved no match"
