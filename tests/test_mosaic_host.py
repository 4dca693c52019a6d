"""Host-side contract of the mosaic plan (nm_mosaic_plan_host_f32, the host twin of nm_mosaic_plan_f32): chains and
rectangles against an independent float64 numpy restatement, the chain-break rules, continuation across calls through
M_first, and refusal of every invalid argument before any device access (so these run without a GPU)."""
import ctypes as C

import numpy as np
import pytest

FW, FH = 640, 480


def rec_fields(records):
    """(m (n, 9) float32, tx, ty, nw, nh, placed, reserved (n, 2)) of an int32 (n, 16) record table."""
    r = np.ascontiguousarray(records)
    return (r[:, :9].view(np.float32), r[:, 9], r[:, 10], r[:, 11], r[:, 12], r[:, 13], r[:, 14:16])


def translation(dx, dy):
    return np.array([[1, 0, dx], [0, 1, dy], [0, 0, 1]], np.float64)


def similarity(deg, s, dx, dy):
    c, sn = s * np.cos(np.radians(deg)), s * np.sin(np.radians(deg))
    return np.array([[c, -sn, dx], [sn, c, dy], [0, 0, 1]], np.float64)


def make_links(kind, n, seed):
    """n-1 pairwise maps (frame k -> frame k+1) of a camera drifting along a path."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n - 1):
        dx, dy = rng.uniform(-40, -20), rng.uniform(-8, 8)
        if kind == "translation":
            Hk = translation(dx, dy)
        elif kind == "similarity":
            Hk = similarity(rng.uniform(-1.0, 1.0), rng.uniform(0.995, 1.005), dx, dy)
        else:
            Hk = similarity(rng.uniform(-0.7, 0.7), rng.uniform(0.997, 1.003), dx, dy)
            Hk[2, :2] = rng.uniform(-3e-6, 3e-6, 2)
        out.append(Hk)
    return out


def plan_f64(links, fw, fh, cw, ch, ox, oy, M_first=None):
    """Independent float64 restatement: chain, clipped rectangles (tx, ty, nw, nh) and the unclipped extent."""
    M = np.eye(3) if M_first is None else np.asarray(M_first, np.float64).reshape(3, 3)
    chain, rects, boxes = [M / 1.0], [], []
    for Hk in links:
        M = Hk @ M
        M = M / M[2, 2]
        chain.append(M)
    corners = np.array([[-1, -1, 1], [fw, -1, 1], [-1, fh, 1], [fw, fh, 1]], np.float64).T
    for M in chain:
        p = np.linalg.inv(M) @ corners
        x, y = p[0] / p[2], p[1] / p[2]
        box = np.array([np.floor(x.min()) - 1, np.floor(y.min()) - 1, np.ceil(x.max()) + 1, np.ceil(y.max()) + 1])
        x0, x1 = np.clip(box[[0, 2]] + ox, 0, cw)
        y0, y1 = np.clip(box[[1, 3]] + oy, 0, ch)
        rects.append((int(x0), int(y0), int(max(x1 - x0, 0)), int(max(y1 - y0, 0))))
        boxes.append(box)
    b = np.array(boxes)
    return np.array([c.reshape(9) for c in chain]), rects, np.array([b[:, 0].min(), b[:, 1].min(), b[:, 2].max(),
                                                                     b[:, 3].max()])


def links_f32(links):
    return np.array([h.reshape(9) for h in links], np.float32).reshape(-1, 9)


@pytest.mark.parametrize("kind", ["translation", "similarity", "perspective"])
@pytest.mark.parametrize("n", [1, 2, 17, 64])
def test_host_plan_equals_float64_restatement(nm, kind, n):
    links = make_links(kind, n, seed=n * 7 + len(kind))
    H32 = links_f32(links)
    # the float32 links are the input: restate from exactly those values
    links64 = [H32[k].astype(np.float64).reshape(3, 3) for k in range(n - 1)]
    for cw, ch, ox, oy in ((32767, 8000, 28000, 3000), (1500, 900, 700, 300)):
        records, chain, extent = nm.mosaic_plan_host(H32, None, FW, FH, cw, ch, ox, oy)
        m, tx, ty, nw, nh, placed, reserved = rec_fields(records)
        want_chain, want_rects, want_extent = plan_f64(links64, FW, FH, cw, ch, ox, oy)
        assert (placed == 1).all() and (reserved == 0).all()
        for k in range(n):
            g, w = chain[k].astype(np.float64), want_chain[k]
            scale = np.repeat([np.abs(w[:3]).max(), np.abs(w[3:6]).max(), np.abs(w[6:]).max()], 3)
            assert np.all(np.abs(g - w) <= 1e-5 * scale + 1e-9), (k, g, w)
            got_rect = (tx[k], ty[k], tx[k] + nw[k], ty[k] + nh[k])
            wr = want_rects[k]
            want_rect = (wr[0], wr[1], wr[0] + wr[2], wr[1] + wr[3])
            assert max(abs(int(a) - int(b)) for a, b in zip(got_rect, want_rect)) <= 1, (k, got_rect, want_rect)
        assert np.abs(extent.astype(np.float64) - want_extent).max() <= 1, (extent, want_extent)
        # the local map: column 2 = M_k T(tx - ox, ty - oy), columns 0 and 1 unchanged
        for k in range(n):
            M = chain[k].reshape(3, 3)
            assert np.array_equal(m[k].reshape(3, 3)[:, :2], M[:, :2])
            dx, dy = np.float32(tx[k] - ox), np.float32(ty[k] - oy)
            col = M[:, 0].astype(np.float64) * dx + M[:, 1].astype(np.float64) * dy + M[:, 2]
            assert np.allclose(m[k].reshape(3, 3)[:, 2], col, rtol=1e-6, atol=1e-4)
    if n == 1:
        assert np.array_equal(chain[0], np.eye(3, dtype=np.float32).reshape(9))


def test_first_frame_is_identity_placement(nm):
    records, chain, extent = nm.mosaic_plan_host(np.zeros((0, 9), np.float32), None, FW, FH, 2000, 1000, 100, 50)
    m, tx, ty, nw, nh, placed, _ = rec_fields(records)
    # corners -1 .. fw map to themselves: box (-2, -2, fw + 1, fh + 1), shifted by (100, 50)
    assert (tx[0], ty[0], nw[0], nh[0], placed[0]) == (98, 48, FW + 3, FH + 3, 1)
    assert np.array_equal(extent, np.array([-2, -2, FW + 1, FH + 1], np.float32))
    assert np.array_equal(m[0].reshape(3, 3), np.array([[1, 0, -2], [0, 1, -2], [0, 0, 1]], np.float32))


def _assert_broken_after(nm, H32, status, j, n):
    records, chain, extent = nm.mosaic_plan_host(H32, status, FW, FH, 8000, 4000, 3000, 1000)
    m, tx, ty, nw, nh, placed, reserved = rec_fields(records)
    assert (placed[:j + 1] == 1).all() and (nw[:j + 1] > 0).all()
    assert not records[j + 1:].any() and not chain[j + 1:].any()
    assert chain[:j + 1].any(axis=1).all()
    return records, chain, extent


@pytest.mark.parametrize("j", [0, 3, 8])
def test_chain_breaks(nm, j):
    n = 10
    H32 = links_f32(make_links("similarity", n, seed=5))
    status = np.ones(n - 1, np.int32)
    status[j] = 0
    _assert_broken_after(nm, H32, status, j, n)
    for bad in (np.nan, np.inf, -np.inf):
        Hb = H32.copy()
        Hb[j, 4] = bad
        _assert_broken_after(nm, Hb, None, j, n)
    Hz = H32.copy()                                     # p[8] = 0: the third row of H_j is zero
    Hz[j, 6:] = 0
    _assert_broken_after(nm, Hz, None, j, n)
    st2 = np.ones(n - 1, np.int32)                      # only status == 1 is valid
    st2[j] = 2
    _assert_broken_after(nm, H32, st2, j, n)


def test_extent_when_nothing_is_placed(nm):
    P = np.array([[1, 0, 0], [0, 1, 0], [0.01, 0, 1]], np.float32).reshape(1, 9)
    M_first = np.array([[1, 0, 0], [0, 1, 0], [0.01, 0, 1]], np.float32)   # frame 0 itself behind the camera
    records, chain, extent = nm.mosaic_plan_host(P[:0], None, FW, FH, 2000, 1000, 0, 0, M_first=M_first)
    assert not records.any() and np.array_equal(extent, np.zeros(4, np.float32))
    assert np.array_equal(chain[0], M_first.reshape(9))


def test_corner_behind_camera_unplaces_only_that_frame(nm):
    n = 6
    links = make_links("translation", n, seed=9)
    P = np.array([[1, 0, 0], [0, 1, 0], [0.01, 0, 1]], np.float64)
    # M_2 = P M_1: its inverse has a third row of (-0.01, 0, 1)-like shape, negative at x = fw; M_3 = P^-1 M_2 undoes it
    links[1] = P
    links[2] = np.linalg.inv(P)
    H32 = links_f32(links)
    records, chain, extent = nm.mosaic_plan_host(H32, None, FW, FH, 8000, 4000, 3000, 1000)
    m, tx, ty, nw, nh, placed, _ = rec_fields(records)
    assert placed.tolist() == [1, 1, 0, 1, 1, 1]
    assert not records[2].any()
    assert chain[2].any() and chain[3].any()          # the chain itself goes on
    assert np.allclose(chain[3].reshape(3, 3), chain[1].reshape(3, 3), atol=1e-4)


def test_frame_entirely_off_canvas_is_placed_empty(nm):
    links = [translation(-5000, 0)]
    records, chain, extent = nm.mosaic_plan_host(links_f32(links), None, FW, FH, 2000, 1000, 100, 100)
    m, tx, ty, nw, nh, placed, _ = rec_fields(records)
    assert placed.tolist() == [1, 1] and nw[1] == 0 and nh[1] > 0 and nw[0] > 0
    assert extent[2] > 5000                           # the extent is not clipped


def test_continuation_through_M_first_is_bit_identical(nm):
    n = 12
    H32 = links_f32(make_links("perspective", n, seed=21))
    st = np.ones(n - 1, np.int32)
    geo = (FW, FH, 9000, 3000, 4000, 1200)
    full = nm.mosaic_plan_host(H32, st, *geo)
    a = nm.mosaic_plan_host(H32[:6], st[:6], *geo)
    b = nm.mosaic_plan_host(H32[6:], st[6:], *geo, M_first=a[1][6])
    assert np.array_equal(full[0][:7], a[0]) and np.array_equal(full[1][:7].view(np.uint32), a[1].view(np.uint32))
    assert np.array_equal(full[0][6:], b[0]) and np.array_equal(full[1][6:].view(np.uint32), b[1].view(np.uint32))
    e = np.array([min(a[2][0], b[2][0]), min(a[2][1], b[2][1]), max(a[2][2], b[2][2]), max(a[2][3], b[2][3])])
    assert np.array_equal(full[2], e)


# ---- invalid arguments: refused before any device access ----

HIP_ERROR_INVALID_VALUE = 1
PLAN_CASES = [dict(n=0), dict(n=65), dict(n=-1), dict(fw=0), dict(fh=32768), dict(cw=0), dict(ch=40000), dict(fw=-3),
              dict(ox=1 << 20), dict(ox=-(1 << 20)), dict(oy=1 << 20), dict(oy=-(1 << 21)), dict(null="records"),
              dict(null="H")]
BLEND_CASES = [dict(n=0), dict(n=65), dict(cw=0), dict(ch=32768), dict(fw=0), dict(fh=-1), dict(mfmt=1), dict(wfmt=1),
               dict(mfmt=5), dict(null="canvas"), dict(null="canvas_wts"), dict(null="records"), dict(null="frames"),
               dict(null="masks"), dict(null="wts"), dict(null_elem="frames"), dict(null_elem="masks"),
               dict(null_elem="wts")]


def _plan_call(entry, n=3, fw=64, fh=48, cw=100, ch=100, ox=0, oy=0, null=None):
    fake = 0x1000
    args = dict(H=fake, records=fake)
    if null:
        args[null] = None
    if entry == "device":
        return _lib.nm_mosaic_plan_f32(n, args["H"], fake, fw, fh, cw, ch, ox, oy, fake, args["records"], fake, fake,
                                       None)
    H = (C.c_float * (9 * 64))()
    rec = (C.c_int * (16 * 64))()
    return _lib.nm_mosaic_plan_host_f32(n, H if args["H"] else None, None, fw, fh, cw, ch, ox, oy, None,
                                        rec if args["records"] else None, None, None)


def _blend_call(n=3, cw=100, ch=100, fw=64, fh=48, mfmt=0, wfmt=2, null=None, null_elem=None):
    fake = 0x1000
    nn = max(n, 1)
    arrays = {}
    for name in ("frames", "masks", "wts"):
        vals = [fake] * nn
        if null_elem == name:
            vals[-1] = None
        arrays[name] = (C.c_void_p * nn)(*vals)
    args = dict(canvas=fake, canvas_wts=fake, records=fake, **arrays)
    if null:
        args[null] = None
    return _lib.nm_transform_blend_batch(args["canvas"], cw, ch, args["canvas_wts"], n, args["frames"], fw, fh,
                                         args["masks"], mfmt, args["wts"], wfmt, args["records"], None)


_lib = None


def _child_main():
    """Runs every invalid case and prints the statuses as JSON. Refuses (exit 3, no call made) if a GPU is visible."""
    import json
    import sys
    import torch
    if torch.cuda.device_count() != 0:
        sys.exit(3)
    import niftymatch_amd as nm
    global _lib
    _lib = nm.lib()
    out = dict(plan_device=[_plan_call("device", **kw) for kw in PLAN_CASES],
               plan_host=[_plan_call("host", **kw) for kw in PLAN_CASES],
               blend=[_blend_call(**kw) for kw in BLEND_CASES])
    print(json.dumps(out))


@pytest.fixture(scope="module")
def invalid_statuses():
    """The invalid calls run in a fresh child process with every GPU hidden, so that even an entry whose checks had
    regressed could only fail to launch, never dereference the fake addresses on a real device."""
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    path = [here, os.path.dirname(here)] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else [])
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1",
               PYTHONPATH=os.pathsep.join(path))
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + flags + ["-c", "import test_mosaic_host as t; t._child_main()"], env=env,
                       cwd=here, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def _ids(cases):
    return lambda i: "-".join("%s=%s" % kv for kv in cases[i].items())


@pytest.mark.parametrize("entry", ["plan_device", "plan_host"])
@pytest.mark.parametrize("case", range(len(PLAN_CASES)), ids=_ids(PLAN_CASES))
def test_plan_invalid_arguments_refused(invalid_statuses, entry, case):
    assert invalid_statuses[entry][case] == HIP_ERROR_INVALID_VALUE, PLAN_CASES[case]


@pytest.mark.parametrize("case", range(len(BLEND_CASES)), ids=_ids(BLEND_CASES))
def test_blend_batch_invalid_arguments_refused(invalid_statuses, case):
    assert invalid_statuses["blend"][case] == HIP_ERROR_INVALID_VALUE, BLEND_CASES[case]


def test_plan_host_accepts_null_H_for_one_frame(nm):
    rec = (C.c_int * 16)()
    assert nm.lib().nm_mosaic_plan_host_f32(1, None, None, 64, 48, 100, 100, 0, 0, None, rec, None, None) == 0
    assert rec[13] == 1


def test_python_wrappers_validate_before_the_call(nm):
    import torch
    H = torch.zeros((3, 9))
    with pytest.raises(nm.NmError):                     # host tensors are refused, never computed on the CPU
        nm.mosaic_plan(H, None, 64, 48, 100, 100, 0, 0)
    with pytest.raises(nm.NmError):
        nm.mosaic_plan(torch.zeros((64, 9)), None, 64, 48, 100, 100, 0, 0)
    with pytest.raises(nm.NmError):
        nm.mosaic_plan(H, None, 0, 48, 100, 100, 0, 0)
    with pytest.raises(nm.NmError):
        nm.mosaic_plan(H, None, 64, 48, 100, 100, 1 << 20, 0)
    with pytest.raises(nm.NmError):
        nm.mosaic_plan(torch.zeros((3, 8)), None, 64, 48, 100, 100, 0, 0)
    with pytest.raises(nm.NmError):
        nm.mosaic_plan_host(np.zeros((64, 9), np.float32), None, 64, 48, 100, 100, 0, 0)
    with pytest.raises(nm.NmError):
        nm.mosaic_plan_host(np.zeros((3, 9), np.float32), np.ones(2, np.int32), 64, 48, 100, 100, 0, 0)
    with pytest.raises(nm.NmError):
        nm.mosaic_plan_host(np.zeros((3, 9), np.float32), None, 64, 48, 100, 32768, 0, 0)
    canvas, cwts = torch.zeros((50, 60, 4), dtype=torch.uint8), torch.zeros((50, 60))
    frame, plane = torch.zeros((10, 12, 4), dtype=torch.uint8), torch.zeros((10, 12))
    rec = torch.zeros((2, 16), dtype=torch.int32)
    with pytest.raises(nm.NmError):
        nm.transform_blend_batch(canvas, cwts, [], plane, plane, rec[:0])
    with pytest.raises(nm.NmError):
        nm.transform_blend_batch(canvas, cwts, [frame] * 65, plane, plane, torch.zeros((65, 16), dtype=torch.int32))
    with pytest.raises(nm.NmError):
        nm.transform_blend_batch(canvas, cwts, [frame, frame], [plane], plane, rec)
    with pytest.raises(nm.NmError):
        nm.transform_blend_batch(canvas, cwts, [frame, frame], plane, plane, rec[:1])
    with pytest.raises(nm.NmError):
        nm.transform_blend_batch(canvas, cwts, [frame, frame], [plane, plane.to(torch.uint8)], plane, rec)
    with pytest.raises(nm.NmError):
        nm.transform_blend_batch(canvas, cwts[:10], [frame, frame], plane, plane, rec)
    with pytest.raises(nm.NmError):
        nm.transform_blend_batch(canvas, cwts, [frame, frame], plane, plane, rec)   # host tensors
    assert nm.MOSAIC_MAX_BATCH == 64
