"""The global mosaic adjustment and the placement on a given chain on the device (nm_mosaic_adjust_dev_f32,
nm_mosaic_place_f32): equal to the host twins bit for bit on every output across the 64-links-per-launch and the 512-lane
edges, for every end reason, whatever the workspace and the outputs held, wherever a link sits in its launch group; and
capturable between the refit and the blend."""
import numpy as np
import pytest

import mosaic_adjust_ref as R
from test_mosaic_adjust_host import loop, pair_case  # noqa: F401  (loop: the host test's fixture)

pytestmark = pytest.mark.gpu

F32 = np.float32
FW, FH = R.FW, R.FH
GEO = (FW, FH, 2000, 1500, 700, 500)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def problem(n, L, cap, seed=0, rows=None):
    """n frames of the loop's maps, L links between frames at most three apart (either direction, repeats), cap rows each with
    noise and outliers; a drifted chain, a mask that drops the outliers, and a status table with a few zeros"""
    rng = np.random.default_rng(1000 * n + L + cap + seed)
    G = R.true_maps(max(n, 12))[:n] if n <= 12 else np.stack([R.true_maps(12)[k % 12] for k in range(n)])
    la, lb = [], []
    for l in range(L):
        a = int(rng.integers(0, n))
        b = (a + int(rng.integers(1, min(3, n - 1) + 1))) % n
        la.append(a if l % 3 else b)
        lb.append(b if l % 3 else a)
    rows = max(1, cap - 5) if rows is None else rows
    outl = min(3, cap - rows)
    cols = [[] for _ in range(7)]
    for a, b in zip(la, lb):
        for c, v in zip(cols, R.link_points(G[a], G[b], rng, rows - outl if rows > outl else rows, 0.3, outl if rows > outl else 0, cap)):
            c.append(v)
    chain = []
    for k in range(n):
        D = np.eye(3) + (0 if k == 0 else 1) * np.array([[2e-3, -1e-3, 1.5], [1e-3, -2e-3, -1.0], [2e-6, 1e-6, 0]]) * np.sin(1 + k)
        M = np.linalg.inv(G[k] @ D)
        chain.append((M / M[2, 2]).reshape(9))
    status = np.array([int(l % 7 != 5) for l in range(L)], np.int32)
    return dict(n=n, L=L, la=la, lb=lb, tab=cols[:6], mask=np.stack(cols[6]), chain=np.array(chain, F32), status=status)


def both(nm, dev, p, use_mask=True, use_status=True, workspace=None, **kw):
    up = [[_t(np.asarray(v), dev) if k != 2 else _t(np.array([v], np.int32), dev) for v in p["tab"][k]] for k in range(6)]
    mask = p["mask"] if use_mask else None
    status = p["status"] if use_status else None
    got = nm.mosaic_adjust(p["la"], p["lb"], *up, _t(p["chain"], dev), FW, FH, mask=None if mask is None else _t(mask, dev),
                           link_status=None if status is None else _t(status, dev), workspace=workspace, **kw)
    want = nm.mosaic_adjust_host(p["la"], p["lb"], *p["tab"], p["chain"], FW, FH, mask=mask, link_status=status, **kw)
    return [g.cpu().numpy() for g in got], want


def same(got, want):
    return all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


@pytest.mark.parametrize("n,L", [(2, 1), (3, 2), (9, 63), (9, 64), (9, 65), (64, 129), (64, 256)])
def test_device_equals_host_twin_across_the_launch_groups(nm, cuda, n, L):
    p = problem(n, L, 64)
    p["chain"][n // 2 if n > 3 else n - 1] = 0 if n > 3 else p["chain"][n - 1]      # a zero chain row where frames abound
    got, want = both(nm, cuda, p, iterations=3, max_step=200.0)
    assert same(got, want), (want[3], got[3])
    assert want[3][3] > 0 and want[3][1] <= want[3][0] and (n > 9 or want[3][5] >= 1), want[3]
    got, want = both(nm, cuda, p, use_mask=False, use_status=False, iterations=2, max_step=200.0, anchor=n - 1 if n <= 3 else 1)
    assert same(got, want), (want[3], got[3])


@pytest.mark.parametrize("cap", [1, 64, 513, 1100])
def test_device_equals_host_twin_across_the_lane_edge(nm, cuda, cap):
    p = problem(5, 7, cap)
    for use_mask in (True, False):
        got, want = both(nm, cuda, p, use_mask=use_mask, iterations=4, min_rows=4, max_step=200.0)
        assert same(got, want), (cap, want[3], got[3])
    assert (want[3][7] == R.END_NO_LINK) == (cap == 1)


REASONS = {"iterations": R.END_ITERATIONS, "converged": R.END_CONVERGED, "unusable": R.END_UNUSABLE,
           "no_link": R.END_NO_LINK, "singular": R.END_SINGULAR, "step": R.END_STEP, "rose_at_once": R.END_COST_ROSE,
           "rose_after_a_step": R.END_COST_ROSE}


@pytest.mark.parametrize("reason", list(REASONS))
def test_end_reason(nm, cuda, loop, reason):
    """one case per end reason: the device equals the host twin, and the twin ends for that reason"""
    kw, flags = dict(max_step=200.0), {}
    if reason == "singular":              # a detached component without damping (the host test's case)
        p = dict(n=4, L=2, la=[0, 2], lb=[1, 3], tab=[[c[0], c[2]] for c in loop["tab"]], mask=None, status=None,
                 chain=loop["chain"][:4])
        kw, flags = dict(damping=0.0), dict(use_mask=False, use_status=False)
    elif reason.startswith("rose"):       # the two-frame cases of the host test
        tab, chain = pair_case(3 if reason == "rose_at_once" else 18)
        p = dict(n=2, L=1, la=[0], lb=[1], tab=tab, chain=chain, mask=None, status=None)
        kw, flags = dict(iterations=8, max_step=1e6, damping=0.0), dict(use_mask=False, use_status=False)
    else:
        p = problem(6, 12, 64)
        kw.update(dict(iterations=dict(iterations=1), converged=dict(iterations=16), step=dict(max_step=1e-3),
                       no_link=dict(min_rows=65), unusable=dict(anchor=2))[reason])
        if reason == "unusable":
            p["chain"][2] = 0
    got, want = both(nm, cuda, p, **flags, **kw)
    assert same(got, want), (want[3], got[3])
    assert int(want[3][7]) == REASONS[reason], want[3]
    assert want[3][5] == dict(rose_at_once=0, rose_after_a_step=1).get(reason, want[3][5])


def _raw(nm, dev, p, up, ws, fill, la, lb, status, mask, **kw):
    """the C entry on outputs and a workspace filled beforehand, with guard bytes behind every output"""
    import torch
    n, L = p["n"], len(la)
    cap = p["mask"].shape[1]
    guard = 64
    outs = [torch.empty(n * 9 * 4 + guard, dtype=torch.uint8, device=dev), torch.empty(n * 4 + guard, dtype=torch.uint8, device=dev),
            torch.empty(L * 16 + guard, dtype=torch.uint8, device=dev), torch.empty(64 + guard, dtype=torch.uint8, device=dev)]
    for o in outs:
        o.fill_(0xA5)
    if isinstance(fill, float):
        ws.buf[:ws.buf.numel() // 8 * 8].view(torch.float64).fill_(fill)
    else:
        ws.buf.fill_(fill)
    import ctypes as C
    tables = nm._point_tables_dev(*up)
    chain = _t(p["chain"], dev)
    rc = nm.lib().nm_mosaic_adjust_dev_f32(n, L, (C.c_int * L)(*la), (C.c_int * L)(*lb), *tables[:3], cap, *tables[3:], mask.data_ptr(),
                                           status.data_ptr() if status is not None else None, chain.data_ptr(),
                                           0, FW, FH, kw["iterations"], 8, 1e-6, 200.0, *[o.data_ptr() for o in outs],
                                           ws.buf.data_ptr(), nm._stream())
    assert rc == 0
    torch.cuda.synchronize()
    res = [o.cpu().numpy() for o in outs]
    assert all((r[-guard:] == 0xA5).all() for r in res), "an output was written beyond its end"
    return [r[:-guard] for r in res]


def test_results_ignore_stale_contents_and_a_links_place_in_its_group(nm, cuda):
    import torch
    p = problem(7, 20, 64)
    up = [[_t(np.asarray(v), cuda) if k != 2 else _t(np.array([v], np.int32), cuda) for v in p["tab"][k]] for k in range(6)]
    want = nm.mosaic_adjust_host(p["la"], p["lb"], *p["tab"], p["chain"], FW, FH, mask=p["mask"], iterations=3, max_step=200.0)
    assert want[3][5] >= 2, want[3]
    dm = _t(p["mask"], cuda)
    ws = nm.MosaicAdjustWorkspace(7, 121, cuda)
    runs = [_raw(nm, cuda, p, up, ws, fill, p["la"], p["lb"], None, dm, iterations=3) for fill in (0x00, 0xFF, float("nan"))]
    for r in runs:
        assert all(np.array_equal(a, bits(w).ravel()) for a, w in zip(r, want))
    # The same links behind `shift` status-0 links: every link changes its slot in its launch (5), the links straddle the
    # 64-links-per-launch edge (50: links 50 .. 69), or sit in the second launch at other slots (101). The same link_rms,
    # maps and stats; and the links' sum rows, as the workspace holds them after a one-round call, are the same bits too.
    # Workspace layout (csrc/nm_mosaic_adjust_math.hpp): first L rows of ROW = MOSAIC_ADJUST_SUMS + 1 doubles, the sums
    # and then the row count (S_COUNT).
    row = nm.MOSAIC_ADJUST_SUMS + 1

    def sum_rows(la_, lb_, up_, st_, m_):
        _raw(nm, cuda, p, up_, ws, 0xFF, la_, lb_, st_, m_, iterations=1)
        L = len(la_)
        return ws.buf[:L * row * 8].view(torch.float64).reshape(L, row)[L - 20:].cpu().numpy().copy()

    alone = sum_rows(p["la"], p["lb"], up, None, dm)
    assert np.isfinite(alone).all() and (alone[:, row - 1] > 0).all()
    for shift in (5, 50, 101):
        la, lb = [0] * shift + p["la"], [1] * shift + p["lb"]
        ups = [[c[0]] * shift + c for c in up]
        status = _t(np.array([0] * shift + [1] * 20, np.int32), cuda)
        dms = torch.cat([dm[:1].repeat(shift, 1), dm])
        moved = _raw(nm, cuda, p, ups, ws, 0xFF, la, lb, status, dms, iterations=3)
        assert np.array_equal(moved[0], runs[0][0]) and np.array_equal(moved[3], runs[0][3]), shift
        assert np.array_equal(moved[2][16 * shift:], runs[0][2]) and not moved[2][:16 * shift].any(), shift
        assert np.array_equal(bits(sum_rows(la, lb, ups, status, dms)), bits(alone)), shift


def test_place_equals_host_twin_and_the_plan(nm, cuda):
    G, la, lb, tab = R.scene(rows=40, outliers=0, cap=64)
    n = len(G)
    H = np.stack([np.linalg.inv(G[k + 1]) @ G[k] for k in range(n - 1)])
    H = (H / H[:, 2:, 2:]).astype(F32).reshape(n - 1, 9)
    H[8] = np.array([1, 0, 0, 0, 1, 0, 0.01, 0, 1], F32)                  # frames 9 .. 11 chain through a map that puts their corners behind the camera
    for status in (None, np.array([1] * 5 + [0] + [1] * 5, np.int32)):
        records, chain, extent = nm.mosaic_plan(_t(H, cuda), None if status is None else _t(status, cuda), *GEO)
        got = nm.mosaic_place(chain, *GEO)
        host = nm.mosaic_place_host(chain.cpu().numpy(), *GEO)
        assert np.array_equal(bits(got[0].cpu().numpy()), bits(records.cpu().numpy()))
        assert np.array_equal(bits(got[1].cpu().numpy()), bits(extent.cpu().numpy()))
        assert np.array_equal(bits(got[0].cpu().numpy()), bits(host[0])) and np.array_equal(bits(got[1].cpu().numpy()), bits(host[1]))
        assert records[9, 13].item() == 0 and records[:, 13].sum().item() == (9 if status is None else 6)
    fs = np.ones(n, np.int32)
    fs[3] = 0
    got = nm.mosaic_place(chain, *GEO, frame_status=_t(fs, cuda))
    host = nm.mosaic_place_host(chain.cpu().numpy(), *GEO, frame_status=fs)
    assert np.array_equal(bits(got[0].cpu().numpy()), bits(host[0])) and not host[0][3].any()


def test_refit_plan_adjust_place_blend_capture_and_replay(nm, cuda):
    import torch
    n, cap, cw, ch = 6, 256, 1400, 1000

    def inputs(seed):
        G, la, lb, tab = R.scene(n=12, rows=200, noise=0.3, outliers=10, cap=cap, seed=seed)
        keep = [l for l, (a, b) in enumerate(zip(la, lb)) if a < n and b < n]
        order = [l for l in keep if lb[l] == la[l] + 1] + [l for l in keep if lb[l] != la[l] + 1]
        Ht = np.stack([np.linalg.inv(G[lb[l]]) @ G[la[l]] for l in order])
        return ([la[l] for l in order], [lb[l] for l in order], [[c[l] for l in order] for c in tab[:6]],
                (Ht / Ht[:, 2:, 2:]).astype(F32).reshape(len(order), 9))

    la, lb, tab1, H1 = inputs(5)
    _, _, tab2, H2 = inputs(6)
    L = len(la)
    assert [lb[l] - la[l] for l in range(n - 1)] == [1] * (n - 1)
    to_dev = lambda tab: [[_t(np.asarray(v), cuda) if k != 2 else _t(np.array([v], np.int32), cuda) for v in tab[k]] for k in range(6)]
    bufs, src2 = to_dev(tab1), to_dev(tab2)
    dH, dH2 = _t(H1, cuda), _t(H2, cuda)
    rng = np.random.default_rng(0)
    frames = [_t(rng.integers(0, 255, (FH, FW, 4), dtype=np.uint8), cuda) for _ in range(n)]
    ones = torch.ones((FH, FW), dtype=torch.float32, device=cuda)
    canvas = torch.zeros((ch, cw, 4), dtype=torch.uint8, device=cuda)
    wts = torch.zeros((ch, cw), dtype=torch.float32, device=cuda)
    ws = nm.MosaicAdjustWorkspace(n, L, cuda)

    def enqueue():
        H, count, st, _, mask = nm.ransac_refit_batch_dev(2, *bufs, dH, rounds=2, threshold=4.0, capA=cap, want_mask=True)
        records, chain, _ = nm.mosaic_plan(H[:n - 1], st[:n - 1], FW, FH, cw, ch, 500, 300)
        chain_out, fstat, rms, stats = nm.mosaic_adjust(la, lb, *bufs, chain, FW, FH, mask=mask, link_status=st, capA=cap,
                                                        workspace=ws)
        placed, extent = nm.mosaic_place(chain_out, FW, FH, cw, ch, 500, 300, frame_status=fstat)
        canvas.zero_()
        wts.zero_()
        nm.transform_blend_batch(canvas, wts, frames, ones, ones, placed)
        return H, mask, chain, chain_out, fstat, rms, stats, placed, extent, canvas, wts

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        enqueue()                                          # warm-up outside capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        captured = enqueue()
    for first, (tabs, Hs) in enumerate(((src2, dH2), (to_dev(tab1), _t(H1, cuda)))):
        for dst, src in zip(bufs, tabs):
            for d_, s_ in zip(dst, src):
                d_.copy_(s_)
        dH.copy_(Hs)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = [o.cpu().numpy().copy() for o in captured]
        with torch.cuda.stream(s):
            want = enqueue()
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert np.array_equal(bits(a), bits(b.cpu().numpy()))
        assert got[6][7] in (R.END_CONVERGED, R.END_ITERATIONS) and got[6][5] >= 1 and got[6][1] < got[6][0], got[6]
        assert got[4].all() and (got[7][:, 13] == 1).all() and got[9].any()
