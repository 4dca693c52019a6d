"""Every kernel family of csrc/nm_describe.hip against the binary64 model of tests/describe_ref.py, on the cases of
tests/test_describe_float64.py (the oracle only builds the input planes there; nothing here compares with it).

Families: "api" (the one-list entries: orientations_kernel / descriptors_levels_kernel with one level), "levels" (the *_levels
launchers with host counts), "levels_dev" (device counts; descriptors into container slots) and the frame driver (frame_orient_kernel / frame_desc_kernel, its own test).
nm_detect_orientations writes found peaks only, so an unset slot keeps the caller's fill; the level launchers write -1 there.
Descriptor rows that are not processed are left as found by every family. Outputs start as a sentinel."""
import ctypes as C

import numpy as np
import pytest

import describe_ref as R
import helpers as H
import test_describe_float64 as T

pytestmark = pytest.mark.gpu

FILL = -7.0                     # what outputs hold before a launch
FAMILIES = ("api", "levels", "levels_dev")


def _t(a, cuda):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(cuda)            # a copy: the shared inputs are read-only


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _split(n):
    """Three consecutive, unequal parts of a list of n rows (the level lists of one octave); below 3 rows, one list and two empty."""
    if n < 3:
        return [(0, n), (n, n), (n, n)]
    a = max(1, n // 2)
    b = max(1, (n - a) // 3)
    return [(0, a), (a, a + b), (a + b, n)]


def run_orientations(nm, cuda, family, kp, g, w, h, xper):
    """-> (n, 2) float32 of the family's orientation launch; outputs pre-filled with FILL."""
    import torch
    n = len(kp)
    tg = _t(g, cuda)
    if family == "api":
        out = torch.full((n, 2), FILL, dtype=torch.float32, device=cuda)
        tkp = _t(kp, cuda)
        assert nm.lib().nm_detect_orientations(tkp.data_ptr(), tg.data_ptr(), n, w, h, T.GAUSS, xper, out.data_ptr(), None) == 0
        torch.cuda.synchronize()
        return out.cpu().numpy()
    parts = _split(n)
    tk = [_t(kp[a:b], cuda) for a, b in parts]
    out = [torch.full((b - a, 2), FILL, dtype=torch.float32, device=cuda) for a, b in parts]
    if family == "levels":
        cnt = (C.c_int * 3)(*[b - a for a, b in parts])
        assert nm.lib().nm_detect_orientations_levels(3, _ptrs(tk), cnt, tg.data_ptr(), w, h, T.GAUSS, xper, _ptrs(out), None) == 0
    else:
        d_counts = torch.tensor([b - a for a, b in parts], dtype=torch.int32, device=cuda)
        max_pts = max(b - a for a, b in parts)
        assert nm.lib().nm_detect_orientations_levels_dev(_ptrs(tk), d_counts.data_ptr(), max_pts, tg.data_ptr(), w, h, T.GAUSS,
                                                          xper, _ptrs(out), None, None) == 0
    torch.cuda.synchronize()
    return np.concatenate([o.cpu().numpy() for o in out])


def run_descriptors(nm, cuda, family, kp, ori, g, w, h, xper, max_pts=None, capacity=None):
    """-> desc (n, 128), x, y of the family's descriptor launch; outputs pre-filled with FILL."""
    import torch
    n = len(kp)
    tg = _t(g, cuda)

    def fill(*shape):
        return torch.full(shape, FILL, dtype=torch.float32, device=cuda)

    if family == "api":
        d, x, y = fill(n, 128), fill(n), fill(n)
        tkp, tori = _t(kp, cuda), _t(ori, cuda)
        assert nm.lib().nm_compute_sift_descriptors(tkp.data_ptr(), tori.data_ptr(), tg.data_ptr(), n, w, h,
                                                    T.NUM_DOGS, xper, d.data_ptr(), x.data_ptr(), y.data_ptr(), None) == 0
        torch.cuda.synchronize()
        return d.cpu().numpy(), x.cpu().numpy(), y.cpu().numpy()
    parts = _split(n)
    tk = [_t(kp[a:b], cuda) for a, b in parts]
    to = [_t(ori[a:b], cuda) for a, b in parts]
    if family == "levels":
        d, x, y = [fill(b - a, 128) for a, b in parts], [fill(b - a) for a, b in parts], [fill(b - a) for a, b in parts]
        cnt = (C.c_int * 3)(*[b - a for a, b in parts])
        assert nm.lib().nm_compute_sift_descriptors_levels(3, _ptrs(tk), _ptrs(to), cnt, tg.data_ptr(), w, h, T.NUM_DOGS, xper,
                                                           _ptrs(d), _ptrs(x), _ptrs(y), None) == 0
        torch.cuda.synchronize()
        return tuple(np.concatenate([t.cpu().numpy() for t in ts]) for ts in (d, x, y))
    longest = max(b - a for a, b in parts)
    max_pts = longest if max_pts is None else max_pts
    capacity = n + 16 if capacity is None else capacity
    assert max_pts >= longest and capacity >= n
    d, x, y = fill(capacity, 128), fill(capacity), fill(capacity)
    d_counts = torch.tensor([b - a for a, b in parts], dtype=torch.int32, device=cuda)
    d_items = torch.full((1,), -5, dtype=torch.int32, device=cuda)
    assert nm.lib().nm_compute_sift_descriptors_levels_dev(_ptrs(tk), _ptrs(to), d_counts.data_ptr(), max_pts, None, 0, capacity,
                                                           d_items.data_ptr(), None, tg.data_ptr(), w, h, T.NUM_DOGS, xper,
                                                           d.data_ptr(), x.data_ptr(), y.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert int(d_items.item()) == n
    assert bool((d[n:] == FILL).all()) and bool((x[n:] == FILL).all())
    return d[:n].cpu().numpy(), x[:n].cpu().numpy(), y[:n].cpu().numpy()


def _unset(family, n):
    return FILL if family == "api" else -1.0


def _rows(model, idx):
    """The model's per-keypoint arrays at rows idx (a tiled or cut list)."""
    return {k: (v[idx] if isinstance(v, np.ndarray) else {m: a[idx] for m, a in v.items()}) for k, v in model.items()}


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", list(T.CASES_A))
def test_case_a_bulk(nm, oracle, cuda, name, family):
    kp, ori, w, h, xper, mo, md = T.case_a(name)
    g = T.plane(w, h)
    go = run_orientations(nm, cuda, family, kp, g, w, h, xper)
    T.assert_orientations(mo, go, "orientations A %s %s" % (name, family), unset=_unset(family, len(kp)))
    gd, gx, gy = run_descriptors(nm, cuda, family, kp, ori, g, w, h, xper)
    T.assert_descriptors(md, gd, gx, gy, "descriptors A %s %s" % (name, family))


@pytest.mark.parametrize("family", FAMILIES)
def test_case_b_windows_clipped_by_the_plane(nm, oracle, cuda, family):
    kp, ori, w, h, xper, mo, md = T.case_b()
    g = T.plane(w, h)
    go = run_orientations(nm, cuda, family, kp, g, w, h, xper)
    T.assert_orientations(mo, go, "orientations B " + family, unset=_unset(family, len(kp)))
    gd, gx, gy = run_descriptors(nm, cuda, family, kp, ori, g, w, h, xper)
    T.assert_descriptors(md, gd, gx, gy, "descriptors B " + family)


@pytest.mark.parametrize("family", FAMILIES)
def test_case_c_rows_that_must_not_be_processed(nm, oracle, cuda, family):
    kp_o, kp_d, ori, w, h, xper, mo, md = T.case_c()
    g = T.plane(w, h)
    go = run_orientations(nm, cuda, family, kp_o, g, w, h, xper)
    skipped = ~mo["processed"]
    assert skipped.sum() == len(T.C_SKIP_ORIENT)
    assert (go[skipped] == _unset(family, len(kp_o))).all()       # api: left as found; level launchers: (-1, -1)
    T.assert_orientations(mo, go, "orientations C " + family, unset=_unset(family, len(kp_o)))
    gd, gx, gy = run_descriptors(nm, cuda, family, kp_d, ori, g, w, h, xper)
    skipped = ~md["processed"]
    assert skipped.sum() == len(T.C_SKIP_DESC)
    assert (gd[skipped] == FILL).all() and (gx[skipped] == FILL).all() and (gy[skipped] == FILL).all()
    T.assert_descriptors(md, gd, gx, gy, "descriptors C " + family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("length", [1, 4, 5, 257])
def test_case_d_short_lists(nm, oracle, cuda, length, family):
    kp, ori, w, h, xper, mo, md = T.case_a(T.TEETH)
    g = T.plane(w, h)
    idx = np.arange(length) + 20                                  # rows 20.. of case A: past the hand-placed ones
    go = run_orientations(nm, cuda, family, kp[idx], g, w, h, xper)
    T.assert_orientations(_rows(mo, idx), go, "orientations, %d rows, %s" % (length, family), unset=_unset(family, length))
    gd, gx, gy = run_descriptors(nm, cuda, family, kp[idx], ori[idx], g, w, h, xper)
    T.assert_descriptors(_rows(md, idx), gd, gx, gy, "descriptors, %d rows, %s" % (length, family))


def test_case_d_lists_past_the_grid_caps(nm, oracle, cuda):
    """One length past each grid cap, where the grid-stride loops run: 16 389 keypoints through orientations_kernel (4 per
    block, 4096 blocks), 4 101 through the one-list descriptor entry (4096 blocks), 4 101 with max_pts and capacity above it through both
    *_levels_dev kernels (1024 blocks of 4; 4096 blocks). Case A's list tiled: the model ran once per distinct row."""
    kp, ori, w, h, xper, mo, md = T.case_a(T.TEETH)
    g = T.plane(w, h)
    n = len(kp)
    idx = np.arange(16389) % n
    go = run_orientations(nm, cuda, "api", kp[idx], g, w, h, xper)
    T.assert_orientations(_rows(mo, idx), go, "orientations_kernel, 16389 rows", unset=FILL)
    idx = np.arange(4101) % n
    gd, gx, gy = run_descriptors(nm, cuda, "api", kp[idx], ori[idx], g, w, h, xper)
    T.assert_descriptors(_rows(md, idx), gd, gx, gy, "descriptors_kernel, 4101 rows")
    import torch
    parts = _split(4101)
    tk = [_t(kp[idx][a:b], cuda) for a, b in parts]
    out = [torch.full((b - a, 2), FILL, dtype=torch.float32, device=cuda) for a, b in parts]
    d_counts = torch.tensor([b - a for a, b in parts], dtype=torch.int32, device=cuda)
    tg = _t(g, cuda)
    assert nm.lib().nm_detect_orientations_levels_dev(_ptrs(tk), d_counts.data_ptr(), 4200, tg.data_ptr(), w, h, T.GAUSS,
                                                      xper, _ptrs(out), None, None) == 0      # max_pts 4200: 1024 blocks
    torch.cuda.synchronize()
    go = np.concatenate([o.cpu().numpy() for o in out])
    T.assert_orientations(_rows(mo, idx), go, "orientations_levels_kernel, device counts, 4101 rows")
    gd, gx, gy = run_descriptors(nm, cuda, "levels_dev", kp[idx], ori[idx], g, w, h, xper, max_pts=4200, capacity=4300)
    T.assert_descriptors(_rows(md, idx), gd, gx, gy, "descriptors_levels_kernel, device counts, 4101 rows")


def test_frame_driver_octave0(nm, oracle, cuda):
    """frame_orient_kernel / frame_desc_kernel: SiftArena.detect_describe on a 320 x 200 blurred frame; octave 0's keypoints (the
    prefix of kpts before the level column first drops) and gradient planes (read back from the arena) go to the model, whose
    descriptors take the arena's own first orientation as input."""
    import torch
    w, h, cap = 320, 200, 8192
    arena = nm.SiftArena(w, h, cap, device=cuda)
    try:
        frame = _t(H.blurred_frame(4, w, h), cuda)
        arena.detect_describe(frame)
        torch.cuda.synchronize()
        n = int(arena.num_items.item())
        kp = arena.kpts[:n].cpu().numpy()
        ori = arena.orients[:n].cpu().numpy()
        desc = arena.desc[:n].cpu().numpy()
        xs, ys = arena.x[:n].cpu().numpy(), arena.y[:n].cpu().numpy()
        buf = torch.empty(6 * w * h, dtype=torch.float32, device=cuda)
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip.hipMemcpy(buf.data_ptr(), arena.grad_ptr(), 6 * w * h * 4, 3) == 0
        g = buf.cpu().numpy().reshape(3, h, w, 2)
    finally:
        arena.close()
    drops = np.flatnonzero(np.diff(kp[:, 3]) < 0)
    assert len(drops) > 0
    n0 = int(drops[0]) + 1
    assert set(kp[:n0, 3]) == {0.0, 1.0, 2.0}, "the first drop of the level column is not the octave boundary"
    assert n0 > 100
    kp, ori, desc, xs, ys = kp[:n0], ori[:n0], desc[:n0], xs[:n0], ys[:n0]
    mo = R.orientations64(kp, g, w, h, 1.5, 1.0)                 # octave 0: xper = 1, gauss_factor 1.5
    md = R.descriptors64(kp, ori, g, w, h, T.NUM_DOGS, 1.0)
    assert mo["processed"].all() and md["processed"].all()
    assert T.fragile_share(mo) <= T.FRAGILE_CAP and T.fragile_share(md) <= T.FRAGILE_CAP
    T.assert_orientations(mo, ori, "frame driver orientations, octave 0")
    T.assert_descriptors(md, desc, xs, ys, "frame driver descriptors, octave 0")
