"""Mosaic exposure compensation on the GPU: the measure launch (nm_mosaic_exposure_sums_dev), the solve launch
(nm_mosaic_gains_dev), and the gained blend (nm_transform_blend_batch_gain) against nm_transform_blend_batch. Needs an MI355X.

    python tools/kexposure.py [--links 64 256] [--strides 1 2 4] [--rounds 12] [--trace]

64 frames of 1080p with bytes in [16, 240) (every lattice pixel that lands inside its partner counts, the full work). Link l
of L joins frame k = l mod 64 to frame k + d, d = 1 + l div 64, under the map of the kmosaic_batch.py sequence taken d times
(150 x 40 px steps with a slight rotation: about 90 % overlap at d = 1). The blend pair runs on the kmosaic_batch.py
sequence itself: the same records, masks and weights for both entries, two canvases that keep accumulating. One round =
every measure variant, the solve, the ungained and the gained blend, each bracketed by device events on one stream; rounds
repeat after warm-up, so the variants alternate in one process. Model bytes of a measure call: 20 per counted pixel (one
uchar4 of frame a, four uchar4 taps of frame b). Prints one JSON line per L and one for the blend. --trace runs a few calls
of each instead (for a kernel trace, with the program after `--`).
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


def link_maps(L):
    la, lb, H = [], [], []
    for l in range(L):
        k, d = l % N, 1 + l // N
        a = math.radians(0.2 * math.sin(k))
        la.append(k)
        lb.append((k + d) % N)
        H.append([math.cos(a), -math.sin(a), -150.0 * d, math.sin(a), math.cos(a), -40.0 * d, 0.0, 0.0, 1.0])
    return la, lb, np.array(H, np.float32)


def timed(runs, rounds, warmup, stream):
    """This tool's record of the eager method: median, min and max per arm."""
    sp = karms.spread(karms.time_eager(runs, stream, rounds, warmup))
    return {k: {"median_us": sp["median_us"][k], "min_us": sp["min_max_us"][k][0], "max_us": sp["min_max_us"][k][1]} for k in runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--strides", type=int, nargs="+", default=[1, 2, 4])
    karms.timing_args(ap, rounds=12, warmup=2, trace=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kexposure.py measures on a GPU"
    assert a.rounds >= 10 or a.trace, "at least 10 rounds"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    frames = [torch.randint(16, 240, (FH, FW, 4), dtype=torch.uint8, device=dev, generator=g) for _ in range(N)]
    stream = torch.cuda.Stream()
    st = C.c_void_p(stream.cuda_stream)
    lib = nm.lib()
    fptr = (C.c_void_p * N)(*[f.data_ptr() for f in frames])
    rounds, warmup = (3, 0) if a.trace else (a.rounds, a.warmup)

    for L in a.links:
        la, lb, H = link_maps(L)
        ia, ib = (C.c_int * L)(*la), (C.c_int * L)(*lb)
        dH = torch.from_numpy(H).to(dev)
        sums = torch.zeros((L, 7), dtype=torch.int64, device=dev)
        gains = torch.zeros((N, 3), dtype=torch.float32, device=dev)
        stats = torch.zeros(9, dtype=torch.float64, device=dev)

        def measure(stride):
            r = lib.nm_mosaic_exposure_sums_dev(N, L, fptr, ia, ib, FW, FH, None, dH.data_ptr(), None, stride, 5, 250,
                                                sums.data_ptr(), st)
            assert r == 0, r

        def solve():
            r = lib.nm_mosaic_gains_dev(N, L, ia, ib, sums.data_ptr(), None, 64, 10.0, 0.1, 0.25, 4.0, 0, gains.data_ptr(),
                                        stats.data_ptr(), st)
            assert r == 0, r

        counted = {}
        for s in a.strides:
            with torch.cuda.stream(stream):
                measure(s)
            torch.cuda.synchronize()
            counted[s] = int(sums[:, 0].sum().item())
        runs = {"measure_stride_%d" % s: (lambda s=s: measure(s)) for s in a.strides}
        runs["solve"] = solve
        t = timed(runs, rounds, warmup, stream)
        torch.cuda.synchronize()
        out = {"tool": "kexposure", "frames": N, "links": L, "frame": [FW, FH], "rounds": rounds, "times": t,
               "end": int(stats[8].item()), "usable_links": int(stats[6].item())}
        for s in a.strides:
            lattice = L * (FW // s) * (FH // s)
            out["stride_%d" % s] = {"lattice_pixels": lattice, "counted_pixels": counted[s], "model_bytes": 20 * counted[s],
                                    "model_GBps": 20 * counted[s] / t["measure_stride_%d" % s]["median_us"] * 1e-3}
        karms.emit(out)

    # the blend pair on the kmosaic_batch sequence
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
    canv = {s: torch.zeros((ch, cw, 4), dtype=torch.uint8, device=dev) for s in ("plain", "gained")}
    cwts = {s: torch.zeros((ch, cw), dtype=torch.float32, device=dev) for s in ("plain", "gained")}
    mptr, wptr = (C.c_void_p * n)(*([mask.data_ptr()] * n)), (C.c_void_p * n)(*([wts.data_ptr()] * n))
    gains = torch.from_numpy(np.random.default_rng(0).uniform(0.8, 1.25, (n, 3)).astype(np.float32)).to(dev)

    def plain():
        r = lib.nm_transform_blend_batch(canv["plain"].data_ptr(), cw, ch, cwts["plain"].data_ptr(), n, fptr, FW, FH, mptr, 0,
                                         wptr, 2, records.data_ptr(), st)
        assert r == 0, r

    def gained():
        r = lib.nm_transform_blend_batch_gain(canv["gained"].data_ptr(), cw, ch, cwts["gained"].data_ptr(), n, fptr, FW, FH,
                                              mptr, 0, wptr, 2, records.data_ptr(), gains.data_ptr(), st)
        assert r == 0, r

    t = timed({"blend": plain, "blend_gain": gained}, rounds, warmup, stream)
    torch.cuda.synchronize()
    assert torch.equal(cwts["plain"].view(torch.int32), cwts["gained"].view(torch.int32))
    karms.emit({"tool": "kexposure", "blend_frames": n, "canvas": [cw, ch], "rounds": rounds, "times": t,
                "gained_over_plain": t["blend_gain"]["median_us"] / t["blend"]["median_us"]})


if __name__ == "__main__":
    main()
