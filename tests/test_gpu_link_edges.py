"""The link stages on the device (nm_link_verify_batch_dev_f32, nm_link_refine_batch_dev_f32, nm_link_votes_dev_u8,
nm_link_rank_dev) on the cases of tests/link_edges_ref.py: equal to the host twin bit for bit on every output, and equal to
the numpy restatement where the quantity is an integer (status, reason, N, L, end reason, votes, links). Every call goes
through the C entry with its outputs and its workspace filled with the byte 0x5A beforehand, so an output that is not written
or a stale row of partials that is read shows.

Which case reaches which device-only line. The accumulate kernels' `t += gridDim.x` / `t += PARTS`: 16385 x 2, 16385 x 3
and 64 x 8193 (workgroup 0 alone walks a second tile), 4 x 32767 (every workgroup does); 255 and 256 tiles are the sizes at
which nothing may wrap. Their `u < lw`: lattices of 63, 65 and 129 columns, the one-column last tile of 16385, the 63-column
last tile of 32767 at stride 2, the two-column tiles of 4 x 32767; at stride 3 with remainder 2 the column behind the lattice
is inside the frame. The finalize's and the solve's `r < parts`: 255 rows (one fewer than the sentinel-filled 256), 0 rows
(an empty lattice), 1 row (every frame below one tile), and the rows of a pair with status_in = 0, which stay sentinels.
"""
import numpy as np
import pytest

import link_edges_ref as E
import link_propose_ref as P
import link_refine_ref as R
import link_verify_ref as V
import test_link_refine_host as T
from test_gpu_link_propose import _upload
from test_gpu_link_refine import _same as _same_refine
from test_gpu_link_verify import _same as _same_verify, _t

pytestmark = pytest.mark.gpu

F32 = np.float32
FILL = 0x5A
PHOTO = V.LOW_OVERLAP | V.LOW_NCC


def _claims_its_lattice(c):
    assert E.lattice_of(c["fw"], c["fh"], c["stride"]) == (c["lw"], c["lh"], c["tiles_x"], c["tiles"]), c["what"]


def _upload_frames(dev, As, Bs):
    up = {}
    for a in list(As) + list(Bs):
        if id(a) not in up:
            up[id(a)] = _t(a, dev)
    return [up[id(a)] for a in As], [up[id(b)] for b in Bs]


def _filled(torch, dev, shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=dev)
    t.view(torch.uint8).fill_(FILL)
    return t


def _opt(v, dtype, dev):
    return None if v is None else _t(np.asarray(v, dtype), dev)


def _verify(nm, dev, As, Bs, H, status=None, inliers=None, mask=None, stride=4, min_inliers=16, max_area_ratio=4.0,
            min_overlap=None, min_ncc=None):
    """(device outputs, host twin outputs) of one call of the C entry over sentinel-filled outputs and workspace"""
    import torch
    n = len(As)
    fh, fw = As[0].shape
    mo = nm.LINK_MIN_OVERLAP if min_overlap is None else min_overlap
    mn = nm.LINK_MIN_NCC if min_ncc is None else min_ncc
    H = np.asarray(H, F32).reshape(n, 9)
    dA, dB = _upload_frames(dev, As, Bs)
    dH, dmask, dst, dinl = _t(H, dev), _opt(mask, F32, dev), _opt(status, np.int32, dev), _opt(inliers, np.int32, dev)
    ws = nm.LinkVerifyWorkspace(n, dev)
    ws.buf.view(torch.uint8).fill_(FILL)
    st, why = _filled(torch, dev, n, torch.int32), _filled(torch, dev, n, torch.int32)
    stats = _filled(torch, dev, (n, 8), torch.float64)
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = nm.lib().nm_link_verify_batch_dev_f32(n, nm._pair_dev_table(dA, torch.float32), nm._pair_dev_table(dB, torch.float32), fw,
                                               fh, ptr(dmask), ptr(dH), ptr(dst), ptr(dinl), stride, min_inliers, max_area_ratio,
                                               mo, mn, ptr(st), ptr(why), ptr(stats), ptr(ws.buf), nm._stream())
    assert rc == 0
    torch.cuda.synchronize()
    host = nm.link_verify_host(As, Bs, H, status=status, inliers=inliers, mask=mask, stride=stride, min_inliers=min_inliers,
                               max_area_ratio=max_area_ratio, min_overlap=mo, min_ncc=mn)
    return (st, why, stats), host


def _refine(nm, dev, As, Bs, H, status=None, mask=None, model=R.HOMOGRAPHY, stride=4, iterations=4, min_pixels=64, max_step=16.0):
    import torch
    n = len(As)
    fh, fw = As[0].shape
    H = np.asarray(H, F32).reshape(n, 9)
    dA, dB = _upload_frames(dev, As, Bs)
    dH, dmask, dst = _t(H, dev), _opt(mask, F32, dev), _opt(status, np.int32, dev)
    ws = nm.LinkRefineWorkspace(n, dev)
    ws.buf.view(torch.uint8).fill_(FILL)
    H_out, st = _filled(torch, dev, (n, 9), torch.float32), _filled(torch, dev, n, torch.int32)
    stats = _filled(torch, dev, (n, 9), torch.float64)
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = nm.lib().nm_link_refine_batch_dev_f32(n, nm._pair_dev_table(dA, torch.float32), nm._pair_dev_table(dB, torch.float32), fw,
                                               fh, ptr(dmask), ptr(dH), ptr(dst), model, stride, iterations, min_pixels, max_step,
                                               ptr(H_out), ptr(st), ptr(stats), ptr(ws.buf), nm._stream())
    assert rc == 0
    torch.cuda.synchronize()
    host = nm.link_refine_host(As, Bs, H, status=status, mask=mask, model=model, stride=stride, iterations=iterations,
                               min_pixels=min_pixels, max_step=max_step)
    return (H_out, st, stats), host


def _verify_case(nm, dev, As, Bs, H, **kw):
    """device == twin bit for bit; status, reason, N and L == the restatement's. Returns the twin's outputs."""
    kw = dict(dict(min_overlap=nm.LINK_MIN_OVERLAP, min_ncc=nm.LINK_MIN_NCC), **kw)
    got, host = _verify(nm, dev, As, Bs, H, **kw)
    assert _same_verify(got, host), (got, host)
    st, why, stats = (o.cpu().numpy() for o in got)
    assert np.isfinite(stats).all()
    rest = {k: v for k, v in kw.items() if k not in ("status", "inliers")}
    for k in range(len(As)):
        extra = {}
        if kw.get("status") is not None:
            extra["status_in"] = kw["status"][k]
        if kw.get("inliers") is not None:
            extra["inliers"] = kw["inliers"][k]
        want = V.verify_int(As[k], Bs[k], np.asarray(H, F32).reshape(-1, 9)[k], **rest, **extra)
        assert (int(st[k]), int(why[k])) == want[:2] and (stats[k][0], stats[k][1]) == (want[3][1], want[3][0]), (k, why[k], want)
    return host


def _refine_case(nm, dev, As, Bs, H, restate=True, **kw):
    """device == twin bit for bit; with restate also status, N, L, applied steps and end reason == the restatement's"""
    got, host = _refine(nm, dev, As, Bs, H, **kw)
    assert _same_refine(got, host), (got, host)
    H_out, st, stats = (o.cpu().numpy() for o in got)
    assert np.isfinite(stats).all() and np.isfinite(H_out).all()
    if restate:
        rest = {k: v for k, v in kw.items() if k != "status"}
        for k in range(len(As)):
            want = R.refine_ref(As[k], Bs[k], np.asarray(H, F32).reshape(-1, 9)[k], **rest)
            assert int(st[k]) == want[1] and stats[k][[0, 1, 6, 8]].tolist() == want[2][[0, 1, 6, 8]].tolist(), (k, stats[k], want[2])
    return host


IDS = ["%dx%d" % w[0][:2] for w in E.WALK]


# ---- A ----
@pytest.mark.parametrize("k", range(len(E.WALK)), ids=IDS)
def test_tile_walk_verification(nm, cuda, k):
    c = E.walk_cases(T)[k]
    _claims_its_lattice(c)
    host = _verify_case(nm, cuda, c["As"][:1], c["Bs"][:1], c["H"][:1], stride=c["stride"])
    assert host[2][0][0] > 0 and host[2][0][1] == c["lw"] * c["lh"]
    host = _verify_case(nm, cuda, c["As"], c["Bs"], c["H"], stride=c["stride"], status=[1, 0, 1])
    assert host[1][1] == V.UNUSABLE and host[2][0][0] > 0 and host[2][2][0] > 0


@pytest.mark.parametrize("k", range(len(E.WALK)), ids=IDS)
def test_tile_walk_refinement(nm, cuda, k):
    """Three pairs, four iterations. At 257 tiles with refinement pixels (16385 x 3, 64 x 8193) the pairs end for three
    reasons at different iterations, so the later walks wrap while they read each pair's state and skip the ended ones; on
    the frames of two rows N is 0 by definition (no pixel has both vertical neighbours) and the walk shows in L."""
    c = E.walk_cases(T)[k]
    _claims_its_lattice(c)
    host = _refine_case(nm, cuda, c["As"], c["Bs"], c["starts"], restate=c["fw"] * c["fh"] < 100000, model=c["model"],
                        stride=c["stride"], iterations=4, max_step=E.MAX_STEP)
    stats = host[2]
    assert (stats[:, 1] == c["lw"] * c["lh"]).all()
    if not c["refine_counts"]:
        assert (stats[:, 0] == 0).all() and (stats[:, 8] == R.END_FEW_PIXELS).all()
    elif c["tiles"] == 257:
        assert stats[:, 8].tolist() == [R.END_CONVERGED, R.END_STEP, R.END_ITERATIONS] and (stats[:, 0] > 0).all(), stats
        assert 2 <= stats[0, 6] <= 3 and stats[1, 6] == 0 and stats[2, 6] == 4, stats
    else:
        assert stats[0, 0] > 0 and stats[0, 6] >= 1, stats
    # one pair alone, one iteration: the first walk of a single-pair grid
    _refine_case(nm, cuda, c["As"][:1], c["Bs"][:1], c["starts"][:1], restate=False, model=c["model"], stride=c["stride"],
                 iterations=1, max_step=E.MAX_STEP)


# ---- B ----
def test_tile_interior_edges(nm, cuda):
    for c in E.interior_cases(T):
        _claims_its_lattice(c)
        host = _verify_case(nm, cuda, [c["A"]], [c["B"]], c["H"], stride=c["stride"], mask=c["mask"])
        N, L = host[2][0][:2]
        assert 0 < N <= L and (L == c["lw"] * c["lh"] or c["mask"] is not None), c["what"]
        host = _refine_case(nm, cuda, [c["A"]], [c["B"]], c["H"], mask=c["mask"], model=R.HOMOGRAPHY, stride=c["stride"], iterations=2)
        assert host[1][0] == 1 and host[2][0][0] > 0 and host[2][0][1] == L, (c["what"], host[2])


# ---- C ----
def test_frame_extremes(nm, cuda):
    for c in E.extreme_cases(T):
        _claims_its_lattice(c)
        host = _verify_case(nm, cuda, [c["A"]], [c["B"]], c["H"], stride=c["stride"])
        (N, L), why = host[2][0][:2], int(host[1][0])
        rhost = _refine_case(nm, cuda, [c["A"]], [c["B"]], c["H"], stride=c["stride"], iterations=3 if c["kind"] == "empty" else 2,
                             min_pixels=1)
        st, stats = int(rhost[1][0]), rhost[2][0]
        if c["kind"] == "none":                          # 2 x 2: pixel (0, 0) alone has its taps inside B (the CPU test says why)
            assert (L, N) == (c["lw"] * c["lh"], int((c["fw"], c["fh"]) == (2, 2))) and L > 0 and why & PHOTO == PHOTO, c["what"]
            assert (st, stats[8], stats[0], stats[1]) == (0, R.END_FEW_PIXELS, 0, L), (c["what"], stats)
        elif c["kind"] == "some":
            assert L == c["lw"] * c["lh"] and N > 0 and stats[0] > 0, (c["what"], L, N, stats)
        else:
            assert c["tiles"] == 0 and (L, N) == (0, 0) and why & PHOTO == PHOTO and not host[2][0].any(), c["what"]
            assert (st, stats[8], stats[0], stats[1]) == (0, R.END_FEW_PIXELS, 0, 0), (c["what"], stats)


# ---- D ----
def test_horizon_through_the_frame(nm, cuda):
    for c in E.horizon_cases(T):
        x, y = V.lattice(c["fw"], c["fh"], 1)
        den = V.project32(c["H"], x.astype(F32), y.astype(F32))[0]
        assert int((den == 0).sum()) == c["zeros"] and (den > 0).any() and (den < 0).any(), c["what"]
        host = _verify_case(nm, cuda, [c["A"]], [c["B"]], c["H"], stride=1, min_overlap=0.0, min_ncc=-1.0)
        N, L = host[2][0][:2]
        assert L == 96 * 40 and 0 < N < L and int(host[1][0]) == V.BAD_GEOMETRY, (c["what"], N, host[1])
        for model in T.MODELS:
            _refine_case(nm, cuda, [c["A"]], [c["B"]], c["H"], model=model, stride=1, iterations=3)


# ---- E ----
def test_gates_at_below_and_above(nm, cuda):
    for c in E.gate_cases(T):
        host = _verify_case(nm, cuda, c["As"], c["Bs"], c["H"], **c["kw"])
        for k, want in enumerate(c["want"]):
            assert bool(host[1][k] & c["bit"]) == want, (c["what"], k, host[1][k])
            if c["only"]:
                assert host[1][k] == (c["bit"] if want else 0), (c["what"], k, host[1][k])


# ---- F ----
@pytest.mark.parametrize("k", range(len(E.VOTE_SHAPES)), ids=["n%d-cap%d" % s for s in E.VOTE_SHAPES])
def test_votes_for_mid_sized_n(nm, cuda, k):
    """The default split of the candidate frames, from csrc/nm_link_propose.hip: a workgroup scans QB = 256 queries, so the
    grid has blocks = ceil(cap / 256) n workgroups before the split, split_of gives z = ceil(FILL_BLOCKS / blocks) with
    FILL_BLOCKS = 512, per_z = ceil(n / z) frames per part and ceil(n / per_z) parts:
        n 17 cap 257: blocks 34, z 16, per_z 2, 9 parts, the last with 1 frame
        n 33 cap 257: blocks 66, z  8, per_z 5, 7 parts, the last with 3 frames
        n 33 cap  65: blocks 33, z 16, per_z 3, 11 parts, the last with 3 frames
        n 63 cap  65: blocks 63, z  9, per_z 7, 9 parts, the last with 7 frames
    At cap 257 a frame has two query workgroups; the second leaves at q0 >= nA for every count up to 256 and scans one query
    for 257 and the clipped 262. Each case runs under that split and under one part."""
    import torch
    c = E.vote_cases()[k]
    n, cap = E.VOTE_SHAPES[k]
    blocks = -(-cap // 256) * n
    z = -(-512 // blocks)
    per_z = -(-n // z)
    assert (z, per_z, n - per_z * (-(-n // per_z) - 1)) == {(17, 257): (16, 2, 1), (33, 257): (8, 5, 3), (33, 65): (16, 3, 3),
                                                           (63, 65): (9, 7, 7)}[(n, cap)]
    host, ref = nm.link_votes_host(c["descs"], c["counts"], ambiguity=c["amb"], cap=cap), E.model_votes(c)
    descs, counts = _upload(cuda, c)
    try:
        for split in (0, 1):
            nm.link_votes_set_split(split)
            ws = nm.LinkVotesWorkspace(n, cap, cuda)
            ws.buf.fill_(FILL)
            votes = torch.full((n, n), 0x5a5a5a5a, dtype=torch.int32, device=cuda)
            got = nm.link_votes_dev(descs, counts, ambiguity=c["amb"], cap=cap, votes=votes, workspace=ws)
            torch.cuda.synchronize()
            got = got.cpu().numpy()
            assert np.array_equal(got, host), (split, np.argwhere(got != host)[:5])
            assert np.array_equal(got, ref), (split, np.argwhere(got != ref)[:5])
    finally:
        nm.link_votes_set_split(0)
    assert got.sum() > 0
    if (n, cap) == (33, 257):                                             # a real vote matrix through the ranking
        kw = dict(min_votes=16, min_gap=2, per_frame=2, max_links=P.MAX_LINKS)
        links = tuple(torch.full((P.MAX_LINKS,), 0x5a5a5a5a, dtype=torch.int32, device=cuda) for _ in range(3)) + \
            (torch.full((1,), 0x5a5a5a5a, dtype=torch.int32, device=cuda),)
        la, lb, ls, cnt = nm.link_rank_dev(torch.from_numpy(got).to(cuda), links=links, **kw)
        torch.cuda.synchronize()
        ha, hb, hs, hcnt = nm.link_rank_host(got, **kw)
        ra, rb, rs, rcnt = P.rank(ref, **kw)
        assert int(cnt.item()) == hcnt == rcnt and hcnt > 0
        for dev_list, host_list, ref_list in ((la, ha, ra), (lb, hb, rb), (ls, hs, rs)):
            assert np.array_equal(dev_list.cpu().numpy(), host_list) and np.array_equal(host_list, ref_list)
