"""Median mosaic composite on the GPU: nm_mosaic_median_dev in both modes (with and without the optional outputs) against the
feather blend (nm_transform_blend_batch_gain) and the two-band call at R = 0 (nm_mosaic_bands_dev) on the same records and,
for the latter, the same tiles. Needs an MI355X.

    python tools/kmedian.py [--rounds 12] [--tau 0.05] [--trace]

The 64-frame 1080p sequence of kmosaic_batch.py and kbands.py (150 x 40 px steps with a slight rotation), random gains in
[0.8, 1.25]; the tiles are warped once, before the timing. One round = every arm once, each bracketed by device events on one
stream; rounds repeat after warm-up, so the arms alternate in one process.
Byte model (K = canvas pixels with a valid frame, c = mean valid frames per such pixel):
  SELECT   16 c K read (every covering sample once) + 16 K (the median frame's sample again), 4 K written
  MEAN     16 c K read + 16 s K (the inliers' samples again, s = mean support), 4 K written
  both     + 4 K with canvas_wts, + 2 K with the support and label planes
Prints one JSON line. --trace runs a few calls of each instead (for a kernel trace, with the program after `--`).
"""
import argparse
import ctypes as C
import math

import numpy as np

import karms
import torch

import kmosaic_batch as KB
import niftymatch_amd as nm

FW, FH, N = KB.FW, KB.FH, 64
HBM_PEAK_GBPS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tau", type=float, default=nm.MEDIAN_TAU)
    karms.timing_args(ap, rounds=12, warmup=2, trace=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kmedian.py measures on a GPU"
    assert a.rounds >= 10 or a.trace, "at least 10 rounds"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    frames = [torch.randint(16, 240, (FH, FW, 4), dtype=torch.uint8, device=dev, generator=g) for _ in range(N)]
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    lib = nm.lib()
    rounds, warmup = (3, 0) if a.trace else (a.rounds, a.warmup)
    n = N
    mask = torch.full((FH, FW), 255, dtype=torch.uint8, device=dev)
    wts = torch.from_numpy(KB.feather()).to(dev)
    Hd = torch.from_numpy(KB.links(n)).to(dev)
    _, _, extent = nm.mosaic_plan(Hd, None, FW, FH, 32767, 32767, 16000, 16000)
    e = extent.cpu().numpy()
    ox, oy = int(-math.floor(e[0])), int(-math.floor(e[1]))
    cw, ch = int(math.ceil(e[2])) + ox, int(math.ceil(e[3])) + oy
    records, _, _ = nm.mosaic_plan(Hd, None, FW, FH, cw, ch, ox, oy)
    torch.cuda.synchronize()
    rec = records.cpu().numpy()
    area = rec[:, 11].astype(np.int64) * rec[:, 12]
    cap, P = int(area.max()), int(area.sum())
    fptr = (C.c_void_p * n)(*[f.data_ptr() for f in frames])
    mptr, wptr = (C.c_void_p * n)(*([mask.data_ptr()] * n)), (C.c_void_p * n)(*([wts.data_ptr()] * n))
    gains = torch.from_numpy(np.random.default_rng(0).uniform(0.8, 1.25, (n, 3)).astype(np.float32)).to(dev)
    arms = ("feather", "bands", "select", "mean")
    canv = {s: torch.zeros((ch, cw, 4), dtype=torch.uint8, device=dev) for s in arms}
    cwts = {s: torch.zeros((ch, cw), dtype=torch.float32, device=dev) for s in arms}
    support = torch.zeros((ch, cw), dtype=torch.uint8, device=dev)
    label = torch.zeros((ch, cw), dtype=torch.uint8, device=dev)
    counts = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    tiles = torch.zeros((n, cap, 4), dtype=torch.float32, device=dev)
    stats = torch.zeros(2, dtype=torch.int32, device=dev)
    ws = nm.MosaicBandsWorkspace(n, cap, cw, ch, dev)
    with torch.cuda.stream(stream):
        r = lib.nm_mosaic_warp_tiles(n, fptr, FW, FH, mptr, 0, wptr, 2, records.data_ptr(), gains.data_ptr(), tiles.data_ptr(), cap,
                                     stats.data_ptr(), st)
        assert r == 0, r
    torch.cuda.synchronize()

    def feather():
        r = lib.nm_transform_blend_batch_gain(canv["feather"].data_ptr(), cw, ch, cwts["feather"].data_ptr(), n, fptr, FW, FH,
                                              mptr, 0, wptr, 2, records.data_ptr(), gains.data_ptr(), st)
        assert r == 0, r

    def bands():
        r = lib.nm_mosaic_bands_dev(n, tiles.data_ptr(), cap, records.data_ptr(), canv["bands"].data_ptr(), cw, ch,
                                    cwts["bands"].data_ptr(), 0, 1.0, ws.buf.data_ptr(), st)
        assert r == 0, r

    def median(arm, mode, full):
        r = lib.nm_mosaic_median_dev(n, tiles.data_ptr(), cap, records.data_ptr(), canv[arm].data_ptr(), cw, ch,
                                     cwts[arm].data_ptr() if full else None, mode, 0.0, a.tau,
                                     support.data_ptr() if full else None, label.data_ptr() if full else None,
                                     counts.data_ptr() if full else None, st)
        assert r == 0, r

    runs = {"feather_blend": feather, "bands_R0": bands,
            "median_select": lambda: median("select", nm.MEDIAN_SELECT, False),
            "median_mean": lambda: median("mean", nm.MEDIAN_MEAN, False),
            "median_select_all_outputs": lambda: median("select", nm.MEDIAN_SELECT, True),
            "median_mean_all_outputs": lambda: median("mean", nm.MEDIAN_MEAN, True)}
    sp = karms.spread(karms.time_eager(runs, stream, rounds, warmup))
    t = {k: {"median_us": sp["median_us"][k], "min_us": sp["min_max_us"][k][0], "max_us": sp["min_max_us"][k][1]} for k in runs}
    torch.cuda.synchronize()
    K = int((support > 0).sum().item())
    c = float(counts[:, 0].sum().item()) / max(K, 1)
    s = float(support.sum(dtype=torch.int64).item()) / max(K, 1)          # of the last full call: MEAN
    model = {"median_select": int(16 * c * K + 16 * K + 4 * K), "median_mean": int(16 * c * K + 16 * s * K + 4 * K)}
    model["median_select_all_outputs"] = model["median_select"] + 6 * K
    model["median_mean_all_outputs"] = model["median_mean"] + 6 * K
    out = {"tool": "kmedian", "frames": n, "frame": [FW, FH], "canvas": [cw, ch], "tile_cap": cap, "tile_pixels": P,
           "valid_pixels": K, "mean_valid_frames": c, "mean_support": s, "tau": a.tau, "rounds": rounds, "times": t,
           "model_bytes": model, "outliers_per_frame_max": int(counts[:, 1].max().item())}
    for name, nbytes in model.items():
        us = t[name]["median_us"]
        out[name] = {"model_GBps": nbytes / us * 1e-3, "hbm_fraction": nbytes / us * 1e-3 / HBM_PEAK_GBPS,
                     "over_feather": us / t["feather_blend"]["median_us"], "over_bands_R0": us / t["bands_R0"]["median_us"]}
    karms.emit(out)


if __name__ == "__main__":
    main()
