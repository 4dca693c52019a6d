"""What the frame-sequence stages refuse, host side: one table over every host twin (link verify and refine, mosaic plan and
place, exposure sums and gains, bands, median, frame weights) and over ingest_batch / resample_map_u8x4 as far as they
refuse before they need a device. Frames are 8 x 6, the canvas 16 x 12, except where the case is a width. Every case names
what the parent of the frame-sequence refactor did with it: an exception class, or "accepted". A refused input raises
NmError before any library call, so an in-place output keeps its sentinel; an accepted one gives the result of the plain
call. NOW_NMERROR lists the cases whose answer the refactor changed; there is no tightening on the host side."""
import numpy as np
import pytest

FW, FH, CW, CH, CAP = 8, 6, 16, 12, 2 * 8 * 6
SENTINEL = 0xA5
NOW_NMERROR = {}                # case id -> what the parent did instead; empty: the host twins answered with NmError already


def frames(n=2, fw=FW, fh=FH, c=4, dtype=np.uint8):
    return [((np.arange(fh * fw * c) * 7 + 31 * k) % 251).reshape(fh, fw, c).astype(dtype) for k in range(n)]


def planes(n=2, fw=FW, fh=FH):
    return [f[..., 1].astype(np.float32) for f in frames(n, fw, fh)]


def eye(n):
    return np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (n, 1))


def records(n=2, dtype=np.int32, cols=16):
    r = np.zeros((n, cols), dtype)
    r[:, :9] = eye(n).view(np.int32)
    for k in range(n):
        r[k, 9:14] = (2 + 3 * k, 1 + 2 * k, FW, FH, 1)
    return r


def tiles(n=2, c=4):
    t = np.linspace(0.1, 0.9, n * CAP * c, dtype=np.float32).reshape(n, CAP, c)
    t[..., -1] = 1.0
    return t


def canvas(cw=CW, ch=CH):
    return np.full((ch, cw, 4), SENTINEL, np.uint8), np.full((ch, cw), float(SENTINEL), np.float32)


def plane_u8(cw=CW, ch=CH):
    return np.full((ch, cw), SENTINEL, np.uint8)


# ---- the entries: arguments of a plain call, the call, and the in-place outputs among the arguments ----
def link_args():
    return dict(grayAs=planes(), grayBs=planes()[::-1], H=eye(2), mask=np.ones((FH, FW), np.float32))


def exposure_args():
    return dict(frames=frames(), link_a=[0], link_b=[1], H=eye(1), mask=np.ones((FH, FW), np.float32))


def weights_args():
    return dict(frames=frames(), R=4, base=np.ones((FH, FW), np.uint8), counts=True)


def composite_args(n=2):
    cv, cwts = canvas()
    return dict(canvas=cv, canvas_wts=cwts, tiles=tiles(n), records=records(n))


def median_args(n=2):
    return dict(composite_args(n), support=plane_u8(), label=plane_u8(), counts=np.full((n, 2), SENTINEL, np.uint64))


def plan_args(n=2):
    return dict(H=eye(n - 1), status=None, fw=FW, fh=FH, cw=CW, ch=CH, ox=2, oy=1)


def place_args(n=2):
    return dict(chain=eye(n), fw=FW, fh=FH, cw=CW, ch=CH, ox=2, oy=1)


def gains_args(n=2):
    return dict(n=n, link_a=[0], link_b=[1], sums=np.array([[100, 9000, 9100, 9200, 9300, 9400, 9500]], np.uint64))


def ingest_args():
    import torch
    return dict(frames=[torch.from_numpy(f) for f in frames()], u=torch.zeros((FH, FW)), v=torch.zeros((FH, FW)))


def resample_args():
    import torch
    return dict(tex=torch.from_numpy(frames(1)[0]), x=torch.zeros((FH, FW)), y=torch.zeros((FH, FW)))


ENTRIES = {
    "link_verify_host": (link_args, ()), "link_refine_host": (link_args, ()),
    "mosaic_exposure_sums_host": (exposure_args, ()), "frame_weights_host": (weights_args, ()),
    "mosaic_bands_host": (composite_args, ("canvas", "canvas_wts")),
    "mosaic_median_host": (median_args, ("canvas", "canvas_wts", "support", "label", "counts")),
    "mosaic_plan_host": (plan_args, ()), "mosaic_place_host": (place_args, ()), "mosaic_gains_host": (gains_args, ()),
    "ingest_batch": (ingest_args, ()), "resample_map_u8x4": (resample_args, ()),
}


def set_planes(n=2, fw=FW, fh=FH):
    return lambda a: a.update(grayAs=planes(n, fw, fh), grayBs=planes(n, fw, fh), H=eye(n),
                              mask=None if (fw, fh) != (FW, FH) else a["mask"])


def set_frames(n=2, fw=FW, fh=FH, c=4, dtype=np.uint8, last=None, torch_=False):
    def change(a):
        fs = frames(n, fw, fh, c, dtype)
        if last is not None and fs:
            fs[-1] = frames(n, *last[:3], last[3] if len(last) > 3 else np.uint8)[-1]
        if torch_:
            import torch
            fs = [torch.from_numpy(f) for f in fs]
        a["frames"] = fs
        if (fw, fh) != (FW, FH):
            a.pop("mask", None), a.pop("base", None)
            if torch_:
                import torch
                a.update(u=torch.zeros((fh, fw)), v=torch.zeros((fh, fw)))
    return change


def set_composite(n):
    return lambda a: a.update(tiles=tiles(n), records=records(n), **({"counts": a["counts"][:0]} if "counts" in a and n == 0 else {}))


def wide_canvas(a):
    cv, cwts = canvas(32768, 1)
    a.update(canvas=cv, canvas_wts=cwts)
    for k in ("support", "label"):
        if k in a:
            a[k] = plane_u8(32768, 1)


# (entry, case, the change to a plain call's arguments, the parent's answer)
CASES = [(e, case, change, parent) for entries, case, change, parent in [
    (("link_verify_host", "link_refine_host"), "an empty list", set_planes(0), "NmError"),
    (("link_verify_host", "link_refine_host"), "65 pairs", set_planes(65), "NmError"),
    (("link_verify_host", "link_refine_host"), "one plane of another shape",
     lambda a: a["grayBs"].__setitem__(1, planes(1, FW + 1, FH)[0]), "NmError"),
    (("link_verify_host", "link_refine_host"), "a 3-channel plane",
     lambda a: a["grayAs"].__setitem__(0, frames(1, c=3)[0].astype(np.float32)), "NmError"),
    (("link_verify_host", "link_refine_host"), "a width of 32768", set_planes(2, 32768, 1), "NmError"),
    (("link_verify_host", "link_refine_host"), "a mask of another shape",
     lambda a: a.update(mask=np.ones((FH, FW + 1), np.float32)), "NmError"),
    (("link_verify_host", "link_refine_host"), "uint8 planes", lambda a: a.update(grayAs=[p.astype(np.uint8) for p in a["grayAs"]]),
     "accepted"),
    (("mosaic_exposure_sums_host", "frame_weights_host"), "an empty list", set_frames(0), "NmError"),
    (("mosaic_exposure_sums_host", "frame_weights_host"), "65 frames", set_frames(65), "NmError"),
    (("mosaic_exposure_sums_host", "frame_weights_host"), "one frame of another shape", set_frames(last=(FW + 1, FH, 4)), "NmError"),
    (("mosaic_exposure_sums_host", "frame_weights_host"), "a 3-channel frame", set_frames(last=(FW, FH, 3)), "NmError"),
    (("mosaic_exposure_sums_host", "frame_weights_host"), "3-channel frames", set_frames(c=3), "NmError"),
    (("mosaic_exposure_sums_host", "frame_weights_host"), "a float frame", set_frames(last=(FW, FH, 4, np.float32)), "accepted"),
    (("mosaic_exposure_sums_host", "frame_weights_host"), "a width of 32768", set_frames(2, 32768, 1), "NmError"),
    (("mosaic_exposure_sums_host",), "a mask of another shape", lambda a: a.update(mask=np.ones((FH + 1, FW), np.float32)), "NmError"),
    (("frame_weights_host",), "a mask of another shape", lambda a: a.update(base=np.ones((FH + 1, FW), np.uint8)), "NmError"),
    (("mosaic_bands_host", "mosaic_median_host"), "an empty list", set_composite(0), "NmError"),
    (("mosaic_bands_host", "mosaic_median_host"), "65 frames", set_composite(65), "NmError"),
    (("mosaic_bands_host", "mosaic_median_host"), "records of shape (n, 15)", lambda a: a.update(records=records(cols=15)), "NmError"),
    (("mosaic_bands_host", "mosaic_median_host"), "records of dtype int64",
     lambda a: a.update(records=a["records"].astype(np.int64)), "accepted"),
    (("mosaic_bands_host", "mosaic_median_host"), "a canvas_wts of another shape",
     lambda a: a.update(canvas_wts=canvas(CW + 1, CH)[1]), "NmError"),
    (("mosaic_bands_host", "mosaic_median_host"), "a float canvas", lambda a: a.update(canvas=a["canvas"].astype(np.float32)), "NmError"),
    (("mosaic_bands_host", "mosaic_median_host"), "tiles of shape (n, cap, 3)", lambda a: a.update(tiles=tiles(c=3)), "NmError"),
    (("mosaic_bands_host", "mosaic_median_host"), "a width of 32768", wide_canvas, "NmError"),
    (("mosaic_median_host",), "a support of another shape", lambda a: a.update(support=plane_u8(CW, CH + 1)), "NmError"),
    (("mosaic_plan_host",), "65 frames", lambda a: a.update(H=eye(64)), "NmError"),
    (("mosaic_place_host",), "an empty list", lambda a: a.update(chain=eye(0)), "NmError"),
    (("mosaic_place_host",), "65 frames", lambda a: a.update(chain=eye(65)), "NmError"),
    (("mosaic_plan_host", "mosaic_place_host"), "a width of 32768", lambda a: a.update(fw=32768), "NmError"),
    (("mosaic_gains_host",), "an empty list", lambda a: a.update(n=0), "NmError"),
    (("mosaic_gains_host",), "65 frames", lambda a: a.update(n=65), "NmError"),
    (("ingest_batch",), "an empty list", set_frames(0, torch_=True), "NmError"),
    (("ingest_batch",), "65 frames", set_frames(65, torch_=True), "NmError"),
    (("ingest_batch",), "one frame of another shape", set_frames(last=(FW + 1, FH, 4), torch_=True), "NmError"),
    (("ingest_batch",), "a 3-channel frame", set_frames(last=(FW, FH, 3), torch_=True), "NmError"),
    (("ingest_batch",), "a float frame", set_frames(last=(FW, FH, 4, np.float32), torch_=True), "NmError"),
    (("ingest_batch",), "a width of 32768", set_frames(2, 32768, 1, torch_=True), "NmError"),
    (("ingest_batch",), "one tensor on the CPU", lambda a: None, "NmError"),
    (("resample_map_u8x4",), "a 3-channel frame", lambda a: a.update(tex=a["tex"][..., :3].contiguous()), "NmError"),
    (("resample_map_u8x4",), "a float frame", lambda a: a.update(tex=a["tex"].float()), "NmError"),
    (("resample_map_u8x4",), "a width of 32768", lambda a: a.update(tex=a["tex"].new_zeros((1, 32768, 4))), "NmError"),
    (("resample_map_u8x4",), "one tensor on the CPU", lambda a: None, "NmError"),
] for e in entries]


def flat(result):
    return [np.asarray(r) for r in (result if isinstance(result, tuple) else (result,)) if r is not None]


@pytest.mark.parametrize("entry,case,change,parent", CASES, ids=["%s: %s" % c[:2] for c in CASES])
def test_refusal(nm, entry, case, change, parent):
    make, outputs = ENTRIES[entry]
    args = make()
    change(args)
    kept = {k: args[k].copy() for k in outputs}
    if parent == "accepted":
        plain = make()
        got, want = getattr(nm, entry)(**args), getattr(nm, entry)(**plain)
        for g, w in zip(flat(got) + [args[k] for k in outputs], flat(want) + [plain[k] for k in outputs]):
            assert np.array_equal(g, w)
        return
    assert parent == "NmError" or "%s: %s" % (entry, case) in NOW_NMERROR
    with pytest.raises(nm.NmError):
        getattr(nm, entry)(**args)
    for k in outputs:
        assert np.array_equal(args[k], kept[k]), k


def test_every_listed_case_is_in_the_table():
    ids = {"%s: %s" % c[:2] for c in CASES}
    assert set(NOW_NMERROR) <= ids and len(ids) == len(CASES)
