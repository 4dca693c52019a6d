"""What the frame-sequence stages refuse, device side: the table of test_frame_seq_refusals_host.py over every device entry
(link verify and refine, mosaic plan and place, the batched blend with and without gains, exposure sums and gains, warp
tiles, bands, median, ingest, resample_map_u8x4, frame weights). Frames are 8 x 6, the canvas 16 x 12, except where the case
is a width. Every refused input raises NmError before any launch: the in-place outputs keep their sentinel. TIGHTENED lists
the inputs the parent of the frame-sequence refactor accepted and the refactor refuses, each on a written contract."""
import numpy as np
import pytest

import test_frame_seq_refusals_host as T

pytestmark = pytest.mark.gpu
FW, FH, CW, CH, CAP = T.FW, T.FH, T.CW, T.CH, T.CAP
# case id -> the contract: nm_common.hpp, "frame, canvas and output extents of every stage lie in [1, NM_SIZE_LIMIT]"
TIGHTENED = {"transform_blend_batch: a width of 32768": "accepted: the blend checked no upper limit on fw and fh",
             "transform_blend_batch_gain: a width of 32768": "accepted: the blend checked no upper limit on fw and fh"}


def dev(v, cuda):
    import torch
    if isinstance(v, np.ndarray):
        return torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to(cuda)
    return [dev(x, cuda) for x in v] if isinstance(v, list) and v and isinstance(v[0], np.ndarray) else v


def masks(n=2, fw=FW, fh=FH, dtype=np.float32):
    return [np.ones((fh, fw), dtype) for _ in range(n)]


def blend_args(n=2):
    cv, cwts = T.canvas()
    return dict(canvas=cv, canvas_wts=cwts, frames=T.frames(n), masks=masks(n), wts=masks(n), records=T.records(n))


def warp_args(n=2):
    return dict(frames=T.frames(n), masks=masks(n), wts=masks(n), records=T.records(n), tile_cap=CAP,
                tiles=np.full((n, CAP, 4), float(T.SENTINEL), np.float32), stats=np.full(2, T.SENTINEL, np.int32))


def exposure_args():
    return dict(T.exposure_args(), sums=np.full((1, 7), T.SENTINEL, np.int64))


def weights_args():
    return dict(frames=T.frames(), R=4, base=np.ones((FH, FW), np.uint8), counts=True)


def ingest_args():
    return dict(frames=T.frames(), u=np.zeros((FH, FW), np.float32), v=np.zeros((FH, FW), np.float32))


def resample_args():
    return dict(tex=T.frames(1)[0], x=np.zeros((FH, FW), np.float32), y=np.zeros((FH, FW), np.float32))


def gains_args():
    a = T.gains_args()
    return dict(a, sums=a["sums"].view(np.int64))


def median_args(n=2):
    return dict(T.median_args(n), counts=np.full((n, 2), T.SENTINEL, np.int64))


ENTRIES = {
    "link_verify_batch_dev": (T.link_args, ()), "link_refine_batch_dev": (T.link_args, ()),
    "mosaic_plan": (T.plan_args, ()), "mosaic_place": (T.place_args, ()),
    "transform_blend_batch": (blend_args, ("canvas", "canvas_wts")),
    "transform_blend_batch_gain": (blend_args, ("canvas", "canvas_wts")),
    "mosaic_exposure_sums": (exposure_args, ("sums",)), "mosaic_gains": (gains_args, ()),
    "mosaic_warp_tiles": (warp_args, ("tiles", "stats")),
    "mosaic_bands": (T.composite_args, ("canvas", "canvas_wts")),
    "mosaic_median": (median_args, ("canvas", "canvas_wts", "support", "label", "counts")),
    "ingest_batch": (ingest_args, ()), "resample_map_u8x4": (resample_args, ()), "frame_weights_batch": (weights_args, ()),
}
LINK = ("link_verify_batch_dev", "link_refine_batch_dev")
FRAMES = ("transform_blend_batch", "transform_blend_batch_gain", "mosaic_warp_tiles", "mosaic_exposure_sums", "ingest_batch",
          "frame_weights_batch")
MASKED = FRAMES[:3]
COMPOSITE = ("mosaic_bands", "mosaic_median")
RECORDS = MASKED + COMPOSITE


def set_frames(n=2, fw=FW, fh=FH, last=None):
    """the host table's change, and masks, weights, records and tiles that follow the new n and extents"""
    def change(a):
        T.set_frames(n, fw, fh, last=last)(a)
        if "masks" in a:
            a.update(masks=masks(n, fw, fh), wts=masks(n, fw, fh), records=T.records(n))
        if "tiles" in a:
            a.update(tiles=np.full((n, CAP, 4), float(T.SENTINEL), np.float32))
        if "u" in a:
            a.update(u=np.zeros((fh, fw), np.float32), v=np.zeros((fh, fw), np.float32))
    return change


def cpu(key):
    """leave argument `key` (its last element, for a list) on the CPU"""
    def change(a):
        a["_cpu"] = key
    return change


CASES = [(e, case, change) for entries, case, change in [
    (LINK, "an empty list", T.set_planes(0)),
    (LINK, "65 pairs", T.set_planes(65)),
    (LINK, "one plane of another shape", lambda a: a["grayBs"].__setitem__(1, T.planes(1, FW + 1, FH)[0])),
    (LINK, "a 3-channel plane", lambda a: a["grayAs"].__setitem__(0, T.frames(1, c=3)[0].astype(np.float32))),
    (LINK, "a width of 32768", T.set_planes(2, 32768, 1)),
    (LINK, "a mask of another shape", lambda a: a.update(mask=np.ones((FH, FW + 1), np.float32))),
    (LINK, "one tensor on the CPU", cpu("grayBs")),
    (FRAMES, "an empty list", set_frames(0)),
    (FRAMES, "65 frames", set_frames(65)),
    (FRAMES, "one frame of another shape", set_frames(last=(FW + 1, FH, 4))),
    (FRAMES, "a 3-channel frame", set_frames(last=(FW, FH, 3))),
    (FRAMES, "a float frame", set_frames(last=(FW, FH, 4, np.float32))),
    (FRAMES, "a width of 32768", set_frames(2, 32768, 1)),
    (FRAMES, "one tensor on the CPU", cpu("frames")),
    (MASKED, "a mask list one short", lambda a: a.update(masks=a["masks"][:-1])),
    (MASKED, "mixed mask formats", lambda a: a.update(masks=[a["masks"][0], a["masks"][1].astype(np.uint8)])),
    (MASKED, "mixed weight formats", lambda a: a.update(wts=[a["wts"][0].astype(np.uint8), a["wts"][1]])),
    (MASKED, "a mask of another shape", lambda a: a.update(masks=[a["masks"][0], np.ones((FH, FW + 1), np.float32)])),
    (("mosaic_exposure_sums",), "a mask of another shape", lambda a: a.update(mask=np.ones((FH + 1, FW), np.float32))),
    (("frame_weights_batch",), "a mask of another shape", lambda a: a.update(base=np.ones((FH + 1, FW), np.uint8))),
    (RECORDS, "records of shape (n, 15)", lambda a: a.update(records=T.records(cols=15))),
    (RECORDS, "records of dtype int64", lambda a: a.update(records=a["records"].astype(np.int64))),
    (RECORDS, "records on the CPU", cpu("records")),
    (MASKED[:2] + COMPOSITE, "a canvas_wts of another shape", lambda a: a.update(canvas_wts=T.canvas(CW + 1, CH)[1])),
    (COMPOSITE, "an empty list", T.set_composite(0)),
    (COMPOSITE, "65 frames", T.set_composite(65)),
    (COMPOSITE, "tiles of shape (n, cap, 3)", lambda a: a.update(tiles=T.tiles(c=3))),
    (COMPOSITE, "a float canvas", lambda a: a.update(canvas=a["canvas"].astype(np.float32))),
    (COMPOSITE, "a width of 32768", T.wide_canvas),
    (COMPOSITE, "one tensor on the CPU", cpu("tiles")),
    (("mosaic_median",), "a support of another shape", lambda a: a.update(support=T.plane_u8(CW, CH + 1))),
    (("mosaic_plan",), "65 frames", lambda a: a.update(H=T.eye(64))),
    (("mosaic_plan",), "one tensor on the CPU", cpu("H")),
    (("mosaic_place",), "an empty list", lambda a: a.update(chain=T.eye(0))),
    (("mosaic_place",), "65 frames", lambda a: a.update(chain=T.eye(65))),
    (("mosaic_place",), "one tensor on the CPU", cpu("chain")),
    (("mosaic_plan", "mosaic_place"), "a width of 32768", lambda a: a.update(fw=32768)),
    (("mosaic_gains",), "an empty list", lambda a: a.update(n=0)),
    (("mosaic_gains",), "65 frames", lambda a: a.update(n=65)),
    (("mosaic_gains",), "one tensor on the CPU", cpu("sums")),
    (("resample_map_u8x4",), "a 3-channel frame", lambda a: a.update(tex=np.ascontiguousarray(a["tex"][..., :3]))),
    (("resample_map_u8x4",), "a float frame", lambda a: a.update(tex=a["tex"].astype(np.float32))),
    (("resample_map_u8x4",), "a width of 32768", lambda a: a.update(tex=np.zeros((1, 32768, 4), np.uint8))),
    (("resample_map_u8x4",), "one tensor on the CPU", cpu("tex")),
] for e in entries]
IDS = ["%s: %s" % c[:2] for c in CASES]


@pytest.mark.parametrize("entry,case,change", CASES, ids=IDS)
def test_refusal(nm, cuda, entry, case, change):
    import torch
    make, outputs = ENTRIES[entry]
    args = make()
    change(args)
    on_cpu = args.pop("_cpu", None)
    host = {k: v for k, v in args.items()}
    args = {k: dev(v, cuda) for k, v in args.items()}
    if on_cpu is not None:
        if isinstance(args[on_cpu], list):
            args[on_cpu][-1] = args[on_cpu][-1].cpu()
        else:
            args[on_cpu] = args[on_cpu].cpu()
    torch.cuda.synchronize()
    with pytest.raises(nm.NmError):
        getattr(nm, entry)(**args)
    torch.cuda.synchronize()
    for k in outputs:
        want = host[k].view(np.int64) if host[k].dtype == np.uint64 else host[k]
        assert np.array_equal(args[k].cpu().numpy(), want), k


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_the_plain_call_is_accepted(nm, cuda, entry):
    """the arguments every case starts from are a call the entry takes"""
    import torch
    make, _ = ENTRIES[entry]
    getattr(nm, entry)(**{k: dev(v, cuda) for k, v in make().items()})
    torch.cuda.synchronize()


def test_every_tightening_is_a_case_of_the_table():
    assert set(TIGHTENED) <= set(IDS) and len(set(IDS)) == len(IDS)
