"""Batched mosaic blend (nm_transform_blend_batch) against per-frame nm_transform_blend calls, and the plan launch
(nm_mosaic_plan_f32), on the GPU.

    python tools/kmosaic_batch.py [--frames 16 64] [--rounds 20] [--trace]

A 1080p sequence of n frames along a path (about 90 % overlap between consecutive frames: 150 x 40 px steps with a slight
rotation) is planned on the device; the canvas is sized from the plan's extent and the plan is run again for it. One
shared U8N mask and one shared F32 feather weight plane, as a video client has. The records are read to the host for the
per-frame side before timing. One round = n back-to-back nm_transform_blend calls into one canvas, then one batched call
into another, each bracketed by device events on one stream; rounds alternate the two after warm-up. Both canvases keep
accumulating, so both sides take the weighted-blend branch at every covered pixel. Results are checked equal before
timing. The plan launch is timed on its own. Prints one JSON line per n. --trace runs a few calls of each (for
`rocprofv3 --kernel-trace --stats`).
"""
import argparse
import ctypes as C
import math

import numpy as np

import karms
import torch

import niftymatch_amd as nm

FW, FH = 1920, 1080


def links(n):
    out = []
    for k in range(n - 1):
        a = math.radians(0.2 * math.sin(k))
        out.append([math.cos(a), -math.sin(a), -150.0, math.sin(a), math.cos(a), -40.0, 0.0, 0.0, 1.0])
    return np.array(out, np.float32).reshape(-1, 9)


def feather():
    yy, xx = np.mgrid[0:FH, 0:FW]
    return (np.minimum(np.minimum(xx, FW - 1 - xx), np.minimum(yy, FH - 1 - yy)) / 64.0 + 0.01).astype(np.float32)


def measure(n, rounds, warmup, trace, dev, frames_all, mask, wts):
    stream = torch.cuda.Stream()
    frames = frames_all[:n]
    Hd = torch.from_numpy(links(n)).to(dev)
    _, _, extent = nm.mosaic_plan(Hd, None, FW, FH, 32767, 32767, 16000, 16000)
    e = extent.cpu().numpy()
    ox, oy = int(-math.floor(e[0])), int(-math.floor(e[1]))
    cw, ch = int(math.ceil(e[2])) + ox, int(math.ceil(e[3])) + oy
    records, chain, _ = nm.mosaic_plan(Hd, None, FW, FH, cw, ch, ox, oy)
    torch.cuda.synchronize()
    rec = records.cpu().numpy()
    assert (rec[:, 13] == 1).all() and (rec[:, 11] > 0).all()
    canv = {s: torch.zeros((ch, cw, 4), dtype=torch.uint8, device=dev) for s in ("per_frame", "batched")}
    cwts = {s: torch.zeros((ch, cw), dtype=torch.float32, device=dev) for s in ("per_frame", "batched")}
    L = nm.lib()
    st = C.c_void_p(stream.cuda_stream)
    fptr = (C.c_void_p * n)(*[f.data_ptr() for f in frames])
    mptr = (C.c_void_p * n)(*([mask.data_ptr()] * n))
    wptr = (C.c_void_p * n)(*([wts.data_ptr()] * n))

    def per_frame():
        c, w = canv["per_frame"], cwts["per_frame"]
        for k in range(n):
            tx, ty, nw, nh = (int(v) for v in rec[k, 9:13])
            r = L.nm_transform_blend(c.data_ptr(), cw, ch, frames[k].data_ptr(), FW, FH, nw, nh,
                                     records.data_ptr() + 64 * k, tx, ty, mask.data_ptr(), 0, w.data_ptr(),
                                     wts.data_ptr(), 2, st)
            assert r == 0, r

    def batched():
        r = L.nm_transform_blend_batch(canv["batched"].data_ptr(), cw, ch, cwts["batched"].data_ptr(), n, fptr, FW, FH,
                                       mptr, 0, wptr, 2, records.data_ptr(), st)
        assert r == 0, r

    def plan():
        r = L.nm_mosaic_plan_f32(n, Hd.data_ptr(), None, FW, FH, cw, ch, ox, oy, None, records.data_ptr(),
                                 chain.data_ptr(), extent.data_ptr(), st)
        assert r == 0, r

    runs = {"per_frame": per_frame, "batched": batched, "plan": plan}
    if trace:
        with torch.cuda.stream(stream):
            for _ in range(3):
                for fn in runs.values():
                    fn()
        torch.cuda.synchronize()
        return {"tool": "kmosaic_batch", "frames": n, "trace_calls": 3, "canvas": [cw, ch]}
    with torch.cuda.stream(stream):
        per_frame()
        batched()
    torch.cuda.synchronize()
    assert torch.equal(canv["per_frame"], canv["batched"])
    assert torch.equal(cwts["per_frame"].view(torch.int32), cwts["batched"].view(torch.int32))
    sp = karms.spread(karms.time_eager(runs, stream, rounds, warmup))
    # bytes: per-frame calls read 8 B and write 8 B (uchar4 + weight) per covered pixel per covering frame; the batched
    # call does so once per pixel covered by any frame. Texels: each frame's planes (uchar4 + 1 B mask + 4 B weight).
    cover = np.zeros((ch, cw), np.uint8)
    for k in range(n):
        tx, ty, nw, nh = (int(v) for v in rec[k, 9:13])
        cover[ty:ty + nh, tx:tx + nw] += 1
    rect_px = int(cover.sum(dtype=np.int64))
    union_px = int((cover > 0).sum())
    med = sp["median_us"]
    return {"tool": "kmosaic_batch", "frames": n, "frame": [FW, FH], "canvas": [cw, ch], "rounds": rounds, **sp,
            "speedup": med["per_frame"] / med["batched"], "launches_per_call": {"per_frame": n, "batched": 1, "plan": 1},
            "rect_pixels": rect_px, "union_pixels": union_px,
            "canvas_bytes_per_call": {"per_frame": 16 * rect_px, "batched": 16 * union_px},
            "texel_plane_bytes_per_call": n * FW * FH * (4 + 1 + 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[16, 64])
    karms.timing_args(ap, rounds=20, warmup=3, trace=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kmosaic_batch.py measures on a GPU"
    assert all(1 <= n <= nm.MOSAIC_MAX_BATCH for n in a.frames)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    frames = [torch.randint(0, 256, (FH, FW, 4), dtype=torch.uint8, device=dev, generator=g) for _ in range(max(a.frames))]
    mask = torch.full((FH, FW), 255, dtype=torch.uint8, device=dev)
    wts = torch.from_numpy(feather()).to(dev)
    for n in a.frames:
        karms.emit(measure(n, a.rounds, a.warmup, a.trace, dev, frames, mask, wts))


if __name__ == "__main__":
    main()
