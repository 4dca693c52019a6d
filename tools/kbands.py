"""Two-band mosaic blend on the GPU: the warp-tiles launch (nm_mosaic_warp_tiles) and the bands call (nm_mosaic_bands_dev) at
R = 4, 16 and 32 against the feather blend (nm_transform_blend_batch_gain) on the same records. Needs an MI355X.

    python tools/kbands.py [--radii 4 16 32] [--rounds 12] [--trace]

The 64-frame 1080p sequence of kmosaic_batch.py (150 x 40 px steps with a slight rotation, about six covering frames per
canvas pixel), random gains in [0.8, 1.25]. One round = the feather blend, the warp-tiles launch and the bands call at every
radius, each bracketed by device events on one stream; rounds repeat after warm-up, so the variants alternate in one process.
Byte model (P = sum of nw * nh over the used frames, K = covered canvas pixels, c = mean covering frames):
  warp tiles   16 P written (the frames' taps come from L2 / HBM as in the feather blend)
  label        4 c K read (w of each covering tile pixel), K written
  row pass     (16 + 1) P read (tile and label byte), 20 P written     -- halo re-reads not counted
  column pass  20 P read, 20 P written
  compose      K + (16 + 20) K + (4 + 20) c K read, 8 K written
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
    ap.add_argument("--radii", type=int, nargs="+", default=[4, 16, 32])
    karms.timing_args(ap, rounds=12, warmup=2, trace=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kbands.py measures on a GPU"
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
    canv = {s: torch.zeros((ch, cw, 4), dtype=torch.uint8, device=dev) for s in ("feather", "bands")}
    cwts = {s: torch.zeros((ch, cw), dtype=torch.float32, device=dev) for s in ("feather", "bands")}
    tiles = torch.zeros((n, cap, 4), dtype=torch.float32, device=dev)
    stats = torch.zeros(2, dtype=torch.int32, device=dev)
    ws = nm.MosaicBandsWorkspace(n, cap, cw, ch, dev)

    def feather():
        r = lib.nm_transform_blend_batch_gain(canv["feather"].data_ptr(), cw, ch, cwts["feather"].data_ptr(), n, fptr, FW, FH,
                                              mptr, 0, wptr, 2, records.data_ptr(), gains.data_ptr(), st)
        assert r == 0, r

    def warp():
        r = lib.nm_mosaic_warp_tiles(n, fptr, FW, FH, mptr, 0, wptr, 2, records.data_ptr(), gains.data_ptr(), tiles.data_ptr(),
                                     cap, stats.data_ptr(), st)
        assert r == 0, r

    def bands(R):
        r = lib.nm_mosaic_bands_dev(n, tiles.data_ptr(), cap, records.data_ptr(), canv["bands"].data_ptr(), cw, ch,
                                    cwts["bands"].data_ptr(), R, R / 2.0, ws.buf.data_ptr(), st)
        assert r == 0, r

    runs = {"feather_blend": feather, "warp_tiles": warp}
    runs.update({"bands_R%d" % R: (lambda R=R: bands(R)) for R in a.radii})
    sp = karms.spread(karms.time_eager(runs, stream, rounds, warmup))
    t = {k: {"median_us": sp["median_us"][k], "min_us": sp["min_max_us"][k][0], "max_us": sp["min_max_us"][k][1]} for k in runs}
    torch.cuda.synchronize()
    K = int((cwts["bands"] > 0).sum().item())
    # mosaic_plan clips every rectangle to the canvas, so every tile pixel is a canvas pixel: valid tile pixels per covered pixel
    c = float((tiles[..., 3] > 0).sum().item()) / max(K, 1)
    model = {"warp_tiles": 16 * P, "bands": int(4 * c * K + K + 37 * P + 40 * P + 37 * K + 24 * c * K + 8 * K)}
    out = {"tool": "kbands", "frames": n, "frame": [FW, FH], "canvas": [cw, ch], "tile_cap": cap, "tile_pixels": P,
           "covered_pixels": K, "mean_cover": c, "stats": stats.cpu().tolist(), "rounds": rounds, "times": t,
           "model_bytes": model, "workspace_bytes": int(ws.buf.numel()), "tiles_bytes": int(tiles.numel() * 4),
           "warp_tiles_GBps": model["warp_tiles"] / t["warp_tiles"]["median_us"] * 1e-3,
           "warp_tiles_hbm_fraction": model["warp_tiles"] / t["warp_tiles"]["median_us"] * 1e-3 / HBM_PEAK_GBPS}
    for R in a.radii:
        us = t["bands_R%d" % R]["median_us"]
        out["bands_R%d" % R] = {"model_GBps": model["bands"] / us * 1e-3, "hbm_fraction": model["bands"] / us * 1e-3 / HBM_PEAK_GBPS,
                                "warp_plus_bands_over_feather": (us + t["warp_tiles"]["median_us"]) / t["feather_blend"]["median_us"]}
    karms.emit(out)


if __name__ == "__main__":
    main()
