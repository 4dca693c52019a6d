"""The device entries of the frame-weights, frame-quality and KLT stages against their host twins, bit for bit, on the inputs of
tests/frame_seq_edges_ref.py (the host twins against the numpy models, and the conditions on the inputs:
tests/test_frame_seq_edges_host.py): frames of more than one row-pass chunk with raw-bad pixels planted round every chunk
seam; saturated patterns that bring a wave's 32-bit sums to their bound and one cell's word past 2^40; the keyframe choice on
such words; block patterns that bring the tracker's sums past 2^31 at 8, 16 and 32 lanes; batches either side of the
tracker's split at 32 pairs; and pyramids of six levels, of mixed 16-byte and scalar levels and of planes smaller than a tile."""
import numpy as np
import pytest

import frame_quality_ref as FQ
import frame_seq_edges_ref as E
import frame_weights_ref as FW
import klt_ref as K

pytestmark = pytest.mark.gpu

F32 = np.float32


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- A. frame weights across chunk seams ------------------------------------------------------------------------------------
def weights_dev(nm, frames, base=None, **kw):
    mask, wts, d2, counts = nm.frame_weights_batch(frames, want=FW.KINDS, counts=True, base=base, **kw)
    return dict(mask=mask.cpu().numpy(), wts=wts.cpu().numpy(), dist2=d2.cpu().numpy().view(np.uint16),
                counts=counts.cpu().numpy().view(np.uint64))


def weights_at_every_grid(nm, cuda, frames, configs, bases, caps=(0, 1, 3)):
    d_frames = [_t(f, cuda) for f in frames]
    d_bases = [None if b is None else _t(b, cuda) for b in bases]
    seeds = valid = False
    for kw in configs:
        want = FW.run_host(nm, frames, **E.with_base(kw, bases))
        seeds |= bool(want["counts"][:, 0].all())
        valid |= bool(want["counts"][:, 1].all())
        for cap in caps:
            assert nm.frame_weights_set_grid_cap(cap) == 0
            try:
                got = weights_dev(nm, d_frames, **E.with_base(kw, d_bases))
            finally:
                assert nm.frame_weights_set_grid_cap(0) == cap
            FW.same(got, want)
    assert seeds and valid


@pytest.mark.parametrize("fw,fh", E.FW_SHAPES)
def test_weights_across_the_chunk_seams(nm, cuda, fw, fh):
    """every planted frame of the shape and its frames_for frame, at the twelve (R, min_count) pairs with border, base, mask
    format and margin rotating, at the default grid and with one and three workgroups (a workgroup then walks neighbouring
    chunks and reuses its LDS arrays)"""
    assert (fw + 63) // 64 > 32 or fw == 2048
    weights_at_every_grid(nm, cuda, E.seam_frames(fw, fh), E.fw_configs(E.FW_SHAPES.index((fw, fh))), E.seam_bases(fw, fh))


def test_weights_sixty_four_patterns_of_two_chunks(nm, cuda):
    configs = [dict(lo=FW.LO, hi=FW.HI, R=8, margin=1, min_count=4, border=True, base=0, mask_format=FW.U8N),
               dict(lo=FW.LO, hi=FW.HI, R=31, margin=0, min_count=1, border=False, base=2, mask_format=FW.TEX_F32),
               dict(lo=FW.LO, hi=FW.HI, R=64, margin=5, min_count=9, border=True, base=1, mask_format=FW.U8N)]
    weights_at_every_grid(nm, cuda, E.batch_frames(), configs, E.seam_bases(2112, 9), caps=(0, 3))


# ---- B. frame quality at its sum bounds -------------------------------------------------------------------------------------
def quality_dev(nm, cuda, frames, masks=None, grid=(1, 1), cap=0):
    d_masks = None if masks is None else [_t(m, cuda) for m in masks]
    assert nm.frame_quality_set_grid_cap(cap) == 0
    try:
        return nm.frame_quality_batch([_t(f, cuda) for f in frames], masks=d_masks, lo=0, hi=255, grid=grid).cpu().numpy().view(np.uint64)
    finally:
        assert nm.frame_quality_set_grid_cap(0) == cap


@pytest.mark.parametrize("grid", [(1, 1), (2, 3), (8, 8)])
def test_quality_saturated_patterns(nm, cuda, grid):
    """(a) and (c): the one-pixel checkerboard (L2 = 1 040 400 at every measured pixel; with one cell the wave of columns
    64 .. 127 and rows 32 .. 63 sums 2 130 739 200 in 32 bits, the bound of the kernel's static_assert) and the two-pixel one
    (G2 = 130 050 at every measured pixel)"""
    frames = [E.checker(192, 160), E.checker(192, 160, 2), E.checker(192, 160, 1, 1), E.stripes(192, 160)]
    want = nm.frame_quality_host(frames, lo=0, hi=255, grid=grid)
    assert (want[0, ..., 3] == np.uint64(E.L2_MAX) * want[0, ..., 0]).all() and (want[1, ..., 4] == np.uint64(E.G2_MAX) * want[1, ..., 0]).all()
    assert want[..., 0].all() and (grid != (1, 1) or want[0, 0, 0, 3] > 14 * E.WAVE_BOUND)
    for cap in (0, 1):
        assert np.array_equal(quality_dev(nm, cuda, frames, grid=grid, cap=cap), want)
    assert np.array_equal(want, FQ.stats_model(frames, None, 0, 255, grid))


def test_quality_one_cell_of_a_1080p_checkerboard(nm, cuda):
    """(b) every workgroup adds into the one cell, whose squared-Laplacian word ends above 2^40"""
    f = E.checker(1920, 1080)
    want = nm.frame_quality_host([f], lo=0, hi=255, grid=(1, 1))
    assert want[0, 0, 0, 3] == np.uint64(E.L2_MAX) * want[0, 0, 0, 0] and want[0, 0, 0, 3] > 2 ** 40
    assert np.array_equal(quality_dev(nm, cuda, [f]), want)


@pytest.mark.parametrize("masked", [None, FQ.U8N, FQ.TEX_F32])
def test_quality_sixty_four_variants_through_one_workgroup(nm, cuda, masked):
    """(d) and (e): one workgroup walks all 64 frames and flushes its table 64 times"""
    frames = E.quality_variants()
    masks = None if masked is None else [E.cross_masks(130, 70, masked)] * 64
    for grid in ((1, 1), (8, 8)):
        want = nm.frame_quality_host(frames, masks=masks, lo=0, hi=255, grid=grid)
        assert want[..., 0].reshape(64, -1).sum(axis=1).all()
        for cap in (1, 0):
            assert np.array_equal(quality_dev(nm, cuda, frames, masks, grid, cap), want)


def test_pick_on_the_large_statistics(nm, cuda):
    """(f) the device's choice on the statistics of (a) to (d) and on the hand-written words of 2^40, against the host twin"""
    cases = E.pick_inputs(nm)
    assert cases["a, b and c on one cell"][0][1, 0, 0, 3] > 2 ** 40 and cases["words of 2^40"][0][..., 3].min() > 2 ** 49
    for name, (stats, chain, keep, kw) in cases.items():
        want = nm.keyframe_pick_host(stats, chain, 64, 48, keep, **kw)
        got = nm.keyframe_pick(_t(stats.view(np.int64), cuda), _t(chain, cuda), 64, 48, keep, **kw)
        FQ.same_pick({k: v.cpu().numpy() for k, v in got._asdict().items()}, want._asdict())
        assert want.key_count[0] >= 2, name


# ---- C. KLT -------------------------------------------------------------------------------------------------------------------
def same_track(got, want, k=slice(None)):
    import torch
    for name in ("dst_xs", "dst_ys", "matches", "reason", "residual", "fb_error"):
        g = torch.stack(getattr(got, name)).cpu().numpy()
        assert np.array_equal(g.view(np.uint8), np.ascontiguousarray(getattr(want, name)[k]).view(np.uint8)), name
    assert np.array_equal(got.count.cpu().numpy().astype(np.uint64), want.count[k])


@pytest.mark.parametrize("lanes", [8, 16, 32])
def test_klt_sums_past_2_31_at_every_group_size(nm, cuda, lanes):
    """the block pattern's pairs: Gxx = Gyy = 225 * 4080^2 > 2^31 at radius 7 and bx or by at -+120 * 4080^2, the largest any
    input gives (asserted from nm_klt_sums_host at the first points); radius 7 and 3, levels 1 and 3, fb_max on"""
    xs, ys = E.klt_points()
    n = len(xs)
    d_xs, d_ys, d_n = _t(xs, cuda), _t(ys, cuda), _t(np.array([n], np.int32), cuda)
    assert nm.klt_set_lanes(lanes) == 0
    try:
        for name, (A, B) in E.klt_pairs().items():
            for levels in (1, 3):
                pyr, _ = nm.gray_pyramid_host([A, B], levels=levels)
                sums = [nm.klt_sums_host(pyr[0], pyr[1], E.KW_, E.KH_, levels, 0, 7, x, y, 0.0, 0.0)[0] for x, y in zip(xs[:10], ys[:10])]
                assert all(s[0] == s[2] == 225 * E.UNIT2 > 2 ** 31 for s in sums)
                assert max(max(abs(s[3]), abs(s[4])) for s in sums) == E.MISMATCH_TAPS * E.UNIT2
                d_pyr, _ = nm.gray_pyramid_batch([_t(A, cuda), _t(B, cuda)], levels=levels)
                for radius in (7, 3):
                    kw = dict(levels=levels, radius=radius, iterations=6, fb_max=1.5)
                    want = nm.klt_track_host([pyr[0]], [pyr[1]], E.KW_, E.KH_, [xs], [ys], [n], **kw)
                    got = nm.klt_track_batch_dev([d_pyr[0]], [d_pyr[1]], E.KW_, E.KH_, [d_xs], [d_ys], [d_n], want_reason=True,
                                                 want_residual=True, want_fb_error=True, **kw)
                    same_track(got, want)
                    assert radius != 7 or (want.reason[0][:10] != K.FLAT).any()
    finally:
        assert nm.klt_set_lanes(0) == lanes


@pytest.mark.parametrize("n", [32, 33, 40])
def test_klt_batches_either_side_of_the_launch_split(nm, cuda, n):
    """n pairs over three pyramids with a start map, a status and a size per pair; at the default grid and with one
    workgroup. The pairs next to the split and the last one equal the host's single-pair results, count words included."""
    c = E.split_case(n)
    pyr, _ = nm.gray_pyramid_host(c["grays"], levels=3)
    d_pyr, _ = nm.gray_pyramid_batch([_t(g, cuda) for g in c["grays"]], levels=3)
    host = lambda ks: nm.klt_track_host([pyr[c["ia"][k]] for k in ks], [pyr[c["ib"][k]] for k in ks], 97, 61, [c["xs"]] * len(ks),
                                        [c["ys"]] * len(ks), [c["nAs"][k] for k in ks], H=c["H"][ks], status=c["status"][ks], **c["kw"])
    want = host(list(range(n)))
    d_xs, d_ys = _t(c["xs"], cuda), _t(c["ys"], cuda)
    args = ([d_pyr[i] for i in c["ia"]], [d_pyr[i] for i in c["ib"]], 97, 61, [d_xs] * n, [d_ys] * n,
            [_t(np.array([v], np.int32), cuda) for v in c["nAs"]])
    for cap in (0, 1):
        prev = nm.klt_set_grid_cap(cap)
        try:
            got = nm.klt_track_batch_dev(*args, H=_t(c["H"], cuda), status=_t(c["status"], cuda), want_reason=True,
                                         want_residual=True, want_fb_error=True, **c["kw"])
        finally:
            nm.klt_set_grid_cap(prev)
        same_track(got, want)
        count = got.count.cpu().numpy().astype(np.uint64)
        for k in E.split_pairs(n):
            one = host([k])
            assert count[k] == one.count[0] > 0 and np.array_equal(got.matches[k].cpu().numpy(), one.matches[0])
            assert np.array_equal(got.dst_xs[k].cpu().numpy().view(np.uint32), one.dst_xs[0].view(np.uint32))
            assert np.array_equal(got.reason[k].cpu().numpy(), one.reason[0])
    assert len(set(want.count.tolist())) > 3


def pyramids_dev(nm, cuda, grays, levels, mask, offset):
    """the device's pyramid blocks and mask bytes as numpy arrays, each block `offset` floats (bytes) into an allocation
    whose fill must survive round it"""
    import torch
    fh, fw = grays[0].shape
    floats = nm.gray_pyramid_floats(fw, fh, levels)
    pool = torch.full((len(grays), floats + 8), float("nan"), dtype=torch.float32, device=cuda)
    bytes_ = torch.full((floats + 32,), 0xA5, dtype=torch.uint8, device=cuda)
    d_pyr, d_mp = nm.gray_pyramid_batch([_t(g, cuda) for g in grays], levels=levels, mask=_t(mask, cuda),
                                        pyrs=[pool[k, offset:offset + floats] for k in range(len(grays))],
                                        mask_pyr=bytes_[16 + offset:16 + offset + floats])
    assert torch.isnan(pool[:, :offset]).all() and torch.isnan(pool[:, offset + floats:]).all()
    assert (bytes_[:16 + offset] == 0xA5).all() and (bytes_[16 + offset + floats:] == 0xA5).all()
    return [p.cpu().numpy() for p in d_pyr], d_mp.cpu().numpy()


def same_levels(nm, got, want, fw, fh, levels):
    for l in range(levels):                                         # the floats between levels belong to nobody
        assert np.array_equal(nm.gray_pyramid_level(got, fw, fh, l).view(np.uint32), nm.gray_pyramid_level(want, fw, fh, l).view(np.uint32)), l


@pytest.mark.parametrize("cap", [0, 1, 3])
@pytest.mark.parametrize("fw,fh,levels", E.PYRAMIDS)
def test_pyramid_shapes(nm, cuda, fw, fh, levels, cap):
    grays = [E.pyramid_gray(fw, fh), E.pyramid_gray(fw, fh, 1)[::-1].copy()]
    masks = E.pyramid_masks(fw, fh)
    prev = nm.klt_set_grid_cap(cap)
    try:
        for name, mask in masks.items():
            pyr, mp = nm.gray_pyramid_host(grays, levels=levels, mask=mask)
            for offset in (0, 1, 4):
                got, got_mp = pyramids_dev(nm, cuda, grays, levels, mask, offset)
                for g, w in zip(got, pyr):
                    same_levels(nm, g, w, fw, fh, levels)
                assert np.array_equal(got_mp, mp), (name, offset)
    finally:
        nm.klt_set_grid_cap(prev)
    if levels == 6:
        top = nm.gray_pyramid_level(nm.gray_pyramid_host(grays, levels=6, mask=masks["one corner"])[1], fw, fh, 5)
        assert top.any() and not top.all()


@pytest.mark.parametrize("cap", [0, 1, 3])
def test_pyramids_of_sixty_four_small_frames(nm, cuda, cap):
    fw, fh, levels = 33, 17, 3
    grays = [E.pyramid_gray(fw, fh, s) for s in range(64)]
    prev = nm.klt_set_grid_cap(cap)
    try:
        for name in ("dense", "corners and edges"):
            mask = E.pyramid_masks(fw, fh)[name]
            pyr, mp = nm.gray_pyramid_host(grays, levels=levels, mask=mask)
            got, got_mp = pyramids_dev(nm, cuda, grays, levels, mask, 4 if name == "dense" else 1)
            for g, w in zip(got, pyr):
                same_levels(nm, g, w, fw, fh, levels)
            assert np.array_equal(got_mp, mp) and len({p.tobytes() for p in pyr}) == 64
    finally:
        nm.klt_set_grid_cap(prev)
