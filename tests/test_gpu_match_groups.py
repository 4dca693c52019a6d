"""The matcher's grouped launches on ragged batches: a batched call whose number of non-empty pairs is a multiple of the XCD
count gives every pair ONE XCD (pairs_share_xcds, nm_match.hip): pair q on the workgroups of XCD q mod 8 under a one-group plan
for CUs / XCDs workgroups, the single-pass screens through match_top2_group_kernel (one launch per 8 pairs, the host-sized plans
packed into its arguments), the coarse pass through its pair_xcd branch. Here: 8- and 16-pair calls, host- and device-sized, on
tiny, one-tile and lopsided sets, with no-op pairs, NaN pairs, the phases, and one captured graph -- every result against the CPU
oracle's scan (oracle.sift_matches; kernels/match.cu:83-117), bit for bit, under all three screens."""
import os
import re

import numpy as np
import pytest

import helpers as H
from test_gpu_match import screen  # noqa: F401  (the autouse three-screen fixture of the matcher's tests)
from test_gpu_stages import _t

pytestmark = pytest.mark.gpu

CAP_A, CAP_B = 4096, 5000
PRIOR = -9
# the ragged set: a one-row pair, the three sizes around one query block x one tile, and lopsided pairs either way
R = [(1, 1), (255, 127), (256, 128), (257, 129), (2049, 1500), (300, 4000), (4096, 130), (700, 900)]
MORE = [(4096, 5000), (1, 1), (1000, 50), (50, 1000), (513, 1025), (33, 3000), (1300, 257), (3000, 2600)]
K_TIES, K_DUP = 4, 7                    # the sets that carry the near-tie construction / the duplicate candidates
N_TIES = 40

# Plain module-level caches: the descriptor sets (set k belongs to entry k of R + MORE; a pair of size (na, nb) is its first na /
# nb rows), their device copies, the oracle's answers (shared by the three screens) and the single-call row counts.
_SETS, _DEVICE, _REF, _SINGLE = {}, {}, {}, {}


def _sets():
    if not _SETS:
        As = [H.synth.descriptors(1500 + k, CAP_A) for k in range(16)]
        Bs = [H.synth.descriptors(1600 + k, CAP_B) for k in range(16)]
        # Uniform rows alone fail the ratio test everywhere (every result -1, whatever the screen found): every third candidate
        # is a noisy copy of a query row at or before its own index, so that any prefix (na, nb) of a set holds true matches
        # whose indices spread over all candidate tiles, and rows with two copies whose distances nearly tie
        rng = np.random.default_rng(2026)
        for k in range(16):
            j = np.arange(0, CAP_B, 3)
            i = (j * 2654435761 % (1 << 32)) % (np.minimum(j, CAP_A - 1) + 1)
            sigma = (10.0 ** rng.uniform(-3, -1.5, len(j))).astype(np.float32)
            Bs[k][j] = As[k][i] + sigma[:, None] * rng.standard_normal((len(j), 128)).astype(np.float32)
        Bs[K_DUP][7] = As[K_DUP][3]; Bs[K_DUP][800] = As[K_DUP][3]     # duplicate candidates: they tie on the lowest index
        for i in range(N_TIES):                                        # near-ties closer than any screen can resolve -> fallback
            for c in range(3):                                         # (the construction of test_match_batch_dev_sizes_sweep)
                v = As[K_TIES][i].copy()
                v[(7 * i + c) % 128] += np.float32(0.25)
                v[(11 * i + 5 * c) % 128] += np.float32(1e-6 * c)
                Bs[K_TIES][3 * i + c] = v
        # the non-finite variants of two sets: a NaN in candidate 0 (every row of the pair becomes -1), an inf in a query
        An, Bn = As[1].copy(), Bs[1].copy()
        Bn[0, 3] = np.nan
        Ai, Bi = As[5].copy(), Bs[5].copy()
        Ai[5, 7] = np.inf
        _SETS.update({k: (As[k], Bs[k]) for k in range(16)})
        _SETS["nan"] = (An, Bn)
        _SETS["inf"] = (Ai, Bi)
    return _SETS


def _dev_set(cuda, tag):
    if tag not in _DEVICE:
        A, B = _sets()[tag]
        _DEVICE[tag] = (_t(A, cuda), _t(B, cuda))
    return _DEVICE[tag]


def _ref(oracle, tag, na, nb):
    key = (tag, na, nb)
    if key not in _REF:
        A, B = _sets()[tag]
        r, _, _ = oracle.sift_matches(A[:na], B[:nb], 0.8, want_distance=False, prior=np.full(na, PRIOR, np.int32))
        r.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def _atoi(s):
    m = re.match(r"\s*[+-]?\d+", s)
    return int(m.group()) if m else 0


def _require_grouping(nm, screen):
    """The precondition of every test here, asserted: 8 pairs take the one-XCD-per-pair division under every screen, 16 pairs too
    (one coarse launch for all 16, one single-pass launch per 8). Skipped only where the division cannot apply."""
    for var in ("NM_COARSE_PAIR_XCD", "NM_TOP2_PAIR_XCD"):
        if var in os.environ and _atoi(os.environ[var]) == 0:
            pytest.skip("%s=0 switches the one-XCD-per-pair division off" % var)
    import ctypes as C
    probe = (C.c_int * 10)()
    assert nm.lib().nm_sift_match_plan(100000, 12500, probe) == 0
    if probe[4] != 8:
        pytest.skip("the device has %d XCD group(s), not 8" % probe[4])
    assert nm.get_match_screen() == screen
    assert nm.lib().nm_sift_match_pairs_per_launch(8) == 8
    assert nm.lib().nm_sift_match_pairs_per_launch(16) == (16 if screen == "f16" else 8)


class _Slice:
    """One pair's part of a batch workspace, shaped like a single-pair workspace (for the row counters)."""

    def __init__(self, buf):
        self.buf = buf


def _counts(nm, screen, view, na, nb):
    """(rows the bf16x3 pass screened again -- two-stage screen only, else 0 --, rows that took the exact fallback)"""
    return (nm.match_second_pass_count(view, na, nb) if screen == "f16" else 0, nm.match_fallback_count(view, na, nb))


def _single_counts(nm, cuda, screen, tag, na, nb):
    """The same counters after ONE nm.sift_match call on the pair (whole-chip plan, the ungrouped kernels)."""
    import torch
    key = (screen, tag, na, nb)
    if key not in _SINGLE:
        tA, tB = _dev_set(cuda, tag)
        ws = nm.MatchWorkspace(na, nb, cuda)
        nm.sift_match(tA, tB, 0.8, prior=torch.full((na,), PRIOR, dtype=torch.int32, device=cuda), workspace=ws, nA=na, nB=nb)
        _SINGLE[key] = _counts(nm, screen, ws, na, nb)
    return _SINGLE[key]


def _host_call(nm, cuda, screen, entries):
    """One nm_sift_match_batch_f32 call on entries (tag, na, nb). Returns every entry's result tensor (CAP_A rows, prior -9) and,
    for the non-empty entries, its (second pass, fallback) row counts."""
    import torch
    n = len(entries)
    tA = [_dev_set(cuda, tag)[0] for tag, _, _ in entries]
    tB = [_dev_set(cuda, tag)[1] for tag, _, _ in entries]
    results = [torch.full((CAP_A,), PRIOR, dtype=torch.int32, device=cuda) for _ in entries]
    ws = nm.MatchBatchWorkspace(n, CAP_A, CAP_B, cuda)
    nm.sift_match_batch(tA, tB, [e[1] for e in entries], [e[2] for e in entries], results, 0.8, workspace=ws)
    torch.cuda.synchronize()
    counts, off = [], 0
    for _, na, nb in entries:                      # the per-pair bounds laid end to end, in order (nm_abi.h)
        size = nm.lib().nm_sift_match_workspace_bytes(na, nb)
        counts.append(_counts(nm, screen, _Slice(ws.buf[off:off + size]), na, nb) if na > 0 and nb > 0 else None)
        off += size
    return results, counts


def _check(oracle, results, entries, what):
    """Every entry's result is the oracle's, rows past nA and the whole of a no-op pair's tensor keep the prior."""
    for k, (tag, na, nb) in enumerate(entries):
        got = results[k].cpu().numpy()
        na, nb = max(0, min(na, CAP_A)), max(0, min(nb, CAP_B))           # as the device-sized entry clips
        if na == 0 or nb == 0:
            assert (got == PRIOR).all(), (what, k, "a no-op pair's prior was touched")
            continue
        assert np.array_equal(got[:na], _ref(oracle, tag, na, nb)), (what, k, tag, na, nb)
        assert (got[na:] == PRIOR).all(), (what, k, tag, na, nb, "rows past nA were written")


def _dev_batch(nm, cuda, tags, sizes):
    """What a device-sized call needs besides the sizes' values: the sets, the two device int vectors, results, a workspace."""
    import torch
    n = len(tags)
    tA = [_dev_set(cuda, t)[0] for t in tags]
    tB = [_dev_set(cuda, t)[1] for t in tags]
    dA = _t(np.array([s[0] for s in sizes], np.int32), cuda)
    dB = _t(np.array([s[1] for s in sizes], np.int32), cuda)
    results = [torch.full((CAP_A,), PRIOR, dtype=torch.int32, device=cuda) for _ in tags]
    ws = nm.MatchBatchDevWorkspace(n, CAP_A, CAP_B, cuda)
    args = (tA, [dA[k:k + 1] for k in range(n)], tB, [dB[k:k + 1] for k in range(n)], results)
    return args, dA, dB, results, ws


def _set_sizes(cuda, dA, dB, results, sizes):
    dA.copy_(_t(np.array([s[0] for s in sizes], np.int32), cuda))
    dB.copy_(_t(np.array([s[1] for s in sizes], np.int32), cuda))
    for r in results:
        r.fill_(PRIOR)


def _entries(tags, sizes):
    return [(t, s[0], s[1]) for t, s in zip(tags, sizes)]


def _assert_screens_decide(nm, cuda, screen, entries, counts, what):
    """The grouped call's screens decide the rows themselves: per pair, the rows handed to the second pass and to the exact
    fallback stay within a margin of what ONE nm.sift_match call on the same data hands on. The two are not equal: a one-group
    plan has 32 workgroups where the single call has 256, so its segments are up to eight times longer, and a segment reports two
    candidates and the value of its third -- a row whose three closest candidates share a segment cannot be proven. Measured on
    MI355X, grouped against single call: at most 49 against 17 rows in the second pass and 22 against 1 in
    the fallback, both at 4096 x 5000 (0.8 % of the rows); equal for every pair below 2049 x 1500 except 300 x 4000 (9 against 8).
    Allowed: 1 % of the pair's rows, at least 2. A screen that lost candidates -- a wrong slot, a workgroup cut off -- and was
    rescued by the exact kernel would show here and nowhere else."""
    for (tag, na, nb), c in zip(entries, counts):
        if c is None:
            continue
        single = _single_counts(nm, cuda, screen, tag, na, nb)
        print("%s [%s] set %s %dx%d: grouped (second pass, fallback) = %s, single call = %s" % (what, screen, tag, na, nb, c, single))
        margin = max(2, na // 100)
        assert abs(c[0] - single[0]) <= margin and abs(c[1] - single[1]) <= margin, (what, tag, na, nb, c, single)


def test_host_sized_8_pairs_ragged_and_reversed(nm, oracle, cuda, screen):
    """8 host-sized pairs = R: the host makes eight one-group plans and packs them (bf16x3, f32) or nbmax_kernel makes them (f16).
    Reversed, every pair lands on another XCD and another slot of the pack: same results, same row counts."""
    import torch
    _require_grouping(nm, screen)
    entries = _entries(range(8), R)
    results, counts = _host_call(nm, cuda, screen, entries)
    _check(oracle, results, entries, "R")
    refs = [_ref(oracle, k, *R[k]) for k in range(8)]
    # the data bites: hundreds of true matches, spread over the candidate tiles of the lopsided pair
    assert sum(int((r >= 0).sum()) for r in refs) >= 500
    assert len({int(j) // 128 for j in refs[5][refs[5] >= 0]}) >= 16
    ref_dup = refs[K_DUP]
    assert ref_dup[3] == PRIOR, "two exact copies of a query: min2 = 0 leaves the prior"
    # the cases bite: the near-tie pair reaches the exact fallback under every screen, the coarse pass hands rows on
    assert counts[K_TIES][1] >= 1
    if screen == "f16":
        assert max(c[0] for c in counts) >= 1
    _assert_screens_decide(nm, cuda, screen, entries, counts, "host-sized R")
    rev = entries[::-1]
    results_r, counts_r = _host_call(nm, cuda, screen, rev)
    _check(oracle, results_r, rev, "R reversed")
    for k in range(8):
        assert torch.equal(results[k], results_r[7 - k]), k
        assert counts[k] == counts_r[7 - k], k


def test_host_sized_16_pairs(nm, oracle, cuda, screen):
    """R and eight more shapes (the largest pair the capacity allows, a second one-row pair) in one call: two grouped launches
    under the single-pass screens (pairs 0-7, 8-15), one coarse launch with two pairs per XCD under the two-stage screen, and the
    second pass on max(2 XCDs, CUs / 16) workgroups per pair for lists of very different lengths."""
    _require_grouping(nm, screen)
    entries = _entries(range(16), R + MORE)
    results, counts = _host_call(nm, cuda, screen, entries)
    _check(oracle, results, entries, "16 pairs")
    assert counts[K_TIES][1] >= 1
    if screen == "f16":
        listed = [c[0] for c in counts]
        assert max(listed) >= 1
        print("16 pairs [f16]: rows per pair in the second pass", listed)
    _assert_screens_decide(nm, cuda, screen, entries, counts, "host-sized 16 pairs")


def test_host_sized_calls_with_empty_pairs(nm, oracle, cuda, screen):
    """An empty host-sized pair is dropped BEFORE the pairs are counted: 9 entries of which one is (0, 50) are 8 pairs and take the
    division, 8 entries of which one is (50, 0) are 7 and do not. Same data either way: every non-empty pair's result reaches ITS
    tensor (the entries behind the empty one shift by one pair slot), the empty pair's prior stays."""
    _require_grouping(nm, screen)
    assert nm.lib().nm_sift_match_pairs_per_launch(7) == (7 if screen == "f16" else 1)
    nine = _entries(range(8), R)
    nine.insert(3, (8, 0, 50))
    results, counts = _host_call(nm, cuda, screen, nine)
    _check(oracle, results, nine, "9 entries, 8 pairs")
    assert counts[K_TIES + 1][1] >= 1
    _assert_screens_decide(nm, cuda, screen, nine, counts, "9 entries, 8 pairs")
    eight = _entries(range(8), R)
    eight[2] = (2, 50, 0)
    results, counts = _host_call(nm, cuda, screen, eight)
    _check(oracle, results, eight, "8 entries, 7 pairs")


@pytest.mark.parametrize("n", [8, 16])
def test_device_sized_ragged_sizes_and_noop_pairs(nm, oracle, cuda, screen, n):
    """Device-sized calls under one capacity: nbmax_kernel makes the one-group plans for the real sizes. The sizes of R; then the
    SAME call with other sizes written into the same device ints: a 0, a negative count, sizes above the capacity (clipped) --
    no-op pairs inside a grouped launch, whose XCD's workgroups must leave without touching anything."""
    import torch
    _require_grouping(nm, screen)
    tags = list(range(n))
    first = list(R) if n == 8 else R + [(0, 50), (-3, 10), (CAP_A + 77, CAP_B + 1), (1, 1), (50, 1000), (513, 1025), (4096, 0), (3000, 2600)]
    second = [(CAP_A + 77, CAP_B + 1), (5, 3), (-3, 10), (10, -1), (1000, 5000), (4096, 128), (0, 129), (77, 5000)]
    if n == 16:
        second = second[::-1] + [(256, 128), (1, 1), (2049, 1500), (300, 4000), (4096, 130), (257, 129), (255, 127), (700, 900)]
    args, dA, dB, results, ws = _dev_batch(nm, cuda, tags, first)
    nm.sift_match_batch_dev(*args, 0.8, workspace=ws, capA=CAP_A, capB=CAP_B)
    torch.cuda.synchronize()
    entries = _entries(tags, first)
    _check(oracle, results, entries, "device-sized, %d pairs" % n)
    counts = [tuple(ws.row_counts(k)) if s[0] > 0 and s[1] > 0 else None for k, s in enumerate(first)]
    counts = [c if c is None or screen == "f16" else (0, c[1]) for c in counts]
    assert counts[K_TIES][1] >= 1
    _assert_screens_decide(nm, cuda, screen, [(t, min(a, CAP_A), min(b, CAP_B)) for t, a, b in entries], counts,
                           "device-sized, %d pairs" % n)
    _set_sizes(cuda, dA, dB, results, second)
    nm.sift_match_batch_dev(*args, 0.8, workspace=ws, capA=CAP_A, capB=CAP_B)
    torch.cuda.synchronize()
    _check(oracle, results, _entries(tags, second), "device-sized, %d pairs, second sizes" % n)


def test_nonfinite_pairs_beside_clean_ones_on_one_launch(nm, oracle, cuda, screen):
    """A NaN in candidate 0 of one pair (every row of it becomes -1, through the exact fallback) and an inf in a query of another,
    inside an 8-pair call, host- and device-sized: those two follow the oracle, the six others give what they give without them."""
    import torch
    _require_grouping(nm, screen)
    tags = [0, "nan", 2, 3, 4, "inf", 6, 7]
    entries = _entries(tags, R)
    assert (_ref(oracle, "nan", *R[1]) == -1).all()
    results, _ = _host_call(nm, cuda, screen, entries)
    _check(oracle, results, entries, "host-sized, NaN and inf pairs")
    args, dA, dB, results, ws = _dev_batch(nm, cuda, tags, R)
    nm.sift_match_batch_dev(*args, 0.8, workspace=ws, capA=CAP_A, capB=CAP_B)
    torch.cuda.synchronize()
    _check(oracle, results, entries, "device-sized, NaN and inf pairs")


def test_phases_of_a_grouped_call_equal_the_whole_call(nm, oracle, cuda, screen):
    """PREP, SCREEN and FINISH of an 8-pair device-sized call issued as three calls: what the whole call gives."""
    import torch
    _require_grouping(nm, screen)
    tags = list(range(8))
    args, _, _, whole, ws = _dev_batch(nm, cuda, tags, R)
    nm.sift_match_batch_dev(*args, 0.8, workspace=ws, capA=CAP_A, capB=CAP_B)
    args2, _, _, parts, ws2 = _dev_batch(nm, cuda, tags, R)
    for ph in (nm.MATCH_PHASE_PREP, nm.MATCH_PHASE_SCREEN, nm.MATCH_PHASE_FINISH):
        nm.sift_match_batch_dev(*args2, 0.8, workspace=ws2, capA=CAP_A, capB=CAP_B, phases=ph)
    torch.cuda.synchronize()
    for k in range(8):
        assert torch.equal(whole[k], parts[k]), k
    _check(oracle, parts, _entries(tags, R), "three phases")


def test_grouped_call_captures_into_one_graph(nm, oracle, cuda, screen):
    """One 8-pair device-sized call captured on a single stream and replayed after the device sizes changed (a no-op pair and a
    clipped one among them): the grouped launches read sizes and plans on the device, nothing of them is baked into the graph."""
    import torch
    _require_grouping(nm, screen)
    tags = list(range(8))
    args, dA, dB, results, ws = _dev_batch(nm, cuda, tags, R)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                       # warm-up outside capture (module load, attributes)
        nm.sift_match_batch_dev(*args, 0.8, workspace=ws, capA=CAP_A, capB=CAP_B)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        nm.sift_match_batch_dev(*args, 0.8, workspace=ws, capA=CAP_A, capB=CAP_B)
    for sizes in (R, [(700, 900), (0, 127), (CAP_A + 1, 128), (1, 1), (257, 129), (300, 4000), (256, 5000), (2049, 1500)]):
        _set_sizes(cuda, dA, dB, results, sizes)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _check(oracle, results, _entries(tags, sizes), "graph replay")
