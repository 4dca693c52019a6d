"""The two-band blend's kernels on the inputs of tests/mosaic_edges_ref.py: nm_mosaic_bands_dev against its host twin bit for bit
(canvas bytes, weights as integers, untouched pixels against the pattern), nm_mosaic_warp_tiles against the gained blend of
each record alone. The host twin is held to the float64 model on the same arrays in tests/test_mosaic_edges_host.py.
  A  every grid-stride loop (warp tiles, label and compose, row blur, column blur) makes two full trips and a remainder:
     the tile counts are computed from the records and asserted against 8 workgroups per compute unit of the device;
  B  rectangles at the blur's own tile edges, strips, a deep clip and records at the int limits, at R = 2, 31, 32;
  C  tied weights, weight limits, an all-invalid pixel, both ends of the store, flat and subnormal taps, any workspace
     contents, pointers aligned to 16 bytes only."""
import numpy as np
import pytest

import bands_ref as B
import mosaic_edges_ref as E

pytestmark = pytest.mark.gpu

F32 = np.float32


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def grid_of(cuda):
    import torch
    return 8 * torch.cuda.get_device_properties(cuda).multi_processor_count


def run_dev(nm, cuda, case, R, sigma=None, workspace=None, d_tiles=None):
    tiles, recs, cap, cw, ch = case
    canvas, cwts = B.pattern(cw, ch)
    d_canvas, d_cwts = _t(canvas, cuda), _t(cwts, cuda)
    if d_tiles is None:
        d_tiles = _t(B.pack(tiles, cap, fill=np.nan), cuda)
    nm.mosaic_bands(d_canvas, d_cwts, d_tiles, _t(B.records(recs), cuda), R=R, sigma=sigma, workspace=workspace)
    return d_canvas.cpu().numpy(), d_cwts.cpu().numpy()


def check(nm, cuda, case, R, sigma=None):
    """device == host twin on canvas and weights; where the host twin wrote nothing the pattern stands"""
    tiles, recs, cap, cw, ch = case
    want_c, want_w = B.run_host(nm, tiles, recs, cap, cw, ch, R, sigma=sigma)
    got_c, got_w = run_dev(nm, cuda, case, R, sigma=sigma)
    assert np.array_equal(got_c, want_c) and np.array_equal(got_w.view(np.int32), want_w.view(np.int32))
    label, _ = B.labels(tiles, recs, cw, ch, cap)
    pat_c, pat_w = B.pattern(cw, ch)
    off = label == B.NONE
    assert off.any() and not off.all()
    assert np.array_equal(got_c[off], pat_c[off]) and np.array_equal(got_w[off].view(np.int32), pat_w[off].view(np.int32))
    return got_c, got_w, label


# ---- A ----------------------------------------------------------------------------------------------------------------------
def test_label_blur_and_compose_walks_make_two_trips_and_a_remainder(nm, cuda):
    case = E.multi_trip_case()
    tiles, recs, cap, cw, ch = case
    G, counts = grid_of(cuda), E.tile_counts(recs, cap, cw, ch)
    for loop in ("canvas", "row", "col"):
        assert counts[loop] >= 2 * G + 1, (loop, counts[loop], G)
    check(nm, cuda, case, 3)


def test_warp_tiles_walk_makes_two_trips_and_a_remainder(nm, cuda):
    from test_gpu_mosaic_bands import check_warp_tiles
    w = E.warp_trip_case()
    n = len(w["recs"])
    assert E.tile_counts([r[9:14] for r in w["recs"]], w["cap"], w["cw"], w["ch"])["warp"] >= 2 * grid_of(cuda) + 1
    base = [_t(f, cuda) for f in w["frames"]]
    check_warp_tiles(nm, cuda, [base[k % len(base)] for k in range(n)], _t(w["mask"], cuda), _t(w["wts"], cuda), w["recs"],
                     _t(w["gains"], cuda), w["cap"], w["cw"], w["ch"], w["stats"])


# ---- B ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", E.BLUR_RADII)
def test_device_equals_the_host_twin_on_the_blur_tile_edges(nm, cuda, R):
    """At R = 32 the column pass's halo is exactly one tile, at 31 one row short of it. The five records at the int limits
    are used frames that touch no canvas pixel: the kernels clip in 64-bit and index a tile by local coordinates only, so
    no address is formed from their tx or ty; they must change nothing."""
    case = E.blur_edge_scene()
    tiles, recs, cap, cw, ch = case
    got_c, got_w, label = check(nm, cuda, case, R)
    n = len(recs)
    for k in range(n - E.EXTREME):
        assert (label == k).any(), k
    without = (tiles[:n - E.EXTREME], recs[:n - E.EXTREME], cap, cw, ch)
    c, w = run_dev(nm, cuda, without, R)
    assert np.array_equal(c, got_c) and np.array_equal(w.view(np.int32), got_w.view(np.int32))


# ---- C ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", (0, 2, 7))
def test_tied_weights_label_the_lowest_index_of_the_tie(nm, cuda, R):
    case = E.bands_ties_case()
    tiles = case[0]
    got_c, _, label = check(nm, cuda, case, R)
    for name, want in E.TIE_WINNER.items():
        c0, c1 = E.TIE_BANDS[name]
        assert (label[2:32, 3 + c0:3 + c1] == want).all(), name
        if R == 0:
            assert np.array_equal(got_c[2:32, 3 + c0:3 + c1, :3], B.store_f32(tiles[want][:, c0:c1, :3]))
    two = E.bands_tie_case()
    got_c, _, _ = check(nm, cuda, two, R)
    assert np.array_equal(got_c[2:32, 2:42, :3], B.store_f32(two[0][0][..., :3]))


@pytest.mark.parametrize("R", (0, 2, 7))
def test_weight_limits_an_all_invalid_pixel_and_both_ends_of_the_store(nm, cuda, R):
    case = E.bands_special_case()
    got_c, got_w, label = check(nm, cuda, case, R)
    S = E.SPECIAL
    at = lambda name: (slice(S[name][0].start + 3, S[name][0].stop + 3), slice(S[name][1].start + 4, S[name][1].stop + 4))
    den = label[at("denorm")] == 0
    assert den.any() and (got_w[at("denorm")][den] == F32(E.DENORM_MIN)).all()          # a subnormal weight is valid
    assert not (label[at("neg_zero")] == 0).any() and (got_w[at("flt_max")] == F32(E.FLT_MAX)).all()
    y0, x0 = at("dead")[0].start, at("dead")[1].start
    pat_c, _ = B.pattern(case[3], case[4])
    assert label[y0, x0] == B.NONE and np.array_equal(got_c[y0, x0], pat_c[y0, x0])
    assert (got_c[at("bright")][..., :3] == 255).all() and (got_c[at("dark")][..., :3] == 0).any()


@pytest.mark.parametrize("which", ("subnormal", "flat"))
def test_sigma_away_from_half_the_radius(nm, cuda, which):
    R, sigma = E.SUBNORMAL_SIGMA if which == "subnormal" else E.FLAT_SIGMA
    g = nm.mosaic_bands_taps(R, sigma)
    tiny = float(np.finfo(F32).tiny)
    if which == "subnormal":        # the bit-for-bit claim needs the device to keep fp32 subnormals, as the host does
        assert ((g > 0) & (g < tiny)).any() and (g[1:] == 0).any()
    else:
        assert g[R] > 0.999 * g[0]
    check(nm, cuda, B.case(17), R, sigma=sigma)
    check(nm, cuda, E.bands_ties_case(), R, sigma=sigma)
    check(nm, cuda, E.bands_special_case(), R, sigma=sigma)


def test_any_workspace_contents_and_pointers_aligned_to_16_bytes_only(nm, cuda):
    import torch
    case = B.case(17)
    tiles, recs, cap, cw, ch = case
    n, R = len(recs), 7
    fresh_c, fresh_w = run_dev(nm, cuda, case, R)
    want_c, want_w = B.run_host(nm, tiles, recs, cap, cw, ch, R)
    assert np.array_equal(fresh_c, want_c) and np.array_equal(fresh_w.view(np.int32), want_w.view(np.int32))
    ws = nm.MosaicBandsWorkspace(n, cap, cw, ch, cuda)

    def same(c, w, what):
        assert np.array_equal(c, fresh_c) and np.array_equal(w.view(np.int32), fresh_w.view(np.int32)), what

    ws.buf.fill_(0xFF)
    same(*run_dev(nm, cuda, case, R, workspace=ws), what="0xFF bytes")
    ws.buf.view(torch.float32).fill_(float("nan"))
    same(*run_dev(nm, cuda, case, R, workspace=ws), what="NaN")
    big = B.case(64)                                                        # a different, larger scene leaves its planes
    wide = nm.MosaicBandsWorkspace(len(big[1]), big[2], big[3], big[4], cuda)
    assert wide.buf.numel() > ws.buf.numel()
    run_dev(nm, cuda, big, 32, workspace=wide)
    same(*run_dev(nm, cuda, case, R, workspace=wide), what="left over from a larger scene")
    # 16-byte but not 32-byte aligned: the workspace and the tiles 16 bytes into a fresh allocation
    need = ws.buf.numel()
    raw_ws = torch.zeros(need + 32, dtype=torch.uint8, device=cuda)
    packed = B.pack(tiles, cap, fill=np.nan)
    raw_t = torch.zeros(packed.size + 8, dtype=torch.float32, device=cuda)
    assert raw_ws.data_ptr() % 32 == 0 and raw_t.data_ptr() % 32 == 0

    class Shifted:
        buf = raw_ws[16:16 + need]

    d_tiles = raw_t[4:4 + packed.size].view(n, cap, 4)
    d_tiles.copy_(_t(packed, cuda))
    assert Shifted.buf.data_ptr() % 32 == 16 and d_tiles.data_ptr() % 32 == 16
    same(*run_dev(nm, cuda, case, R, workspace=Shifted, d_tiles=d_tiles), what="16-byte alignment")
    assert not raw_ws[:16].any().item() and not raw_ws[16 + need:].any().item()
