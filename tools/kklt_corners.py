"""Corner detection (nm_klt_corners_batch_dev_f32) on the GPU, timed as graph replays beside the two yardsticks of the KLT
section on the same frames: the gray pyramid call and the identity-mode ingest launch.

    python tools/kklt_corners.py [--frames 64] [--radii 3 7] [--nms 8] [--rounds 5] [--seconds 1.0] [--trace] [--out FILE]

`--frames` 1920x1080 gray frames on a pan of (6, 2) px per frame over a smooth texture (tools/kklt.py's frames). Arms, each
captured into a HIP graph once and replayed, alternated round by round in one process on one stream:
  pyramid          the pyramid call on the frames, levels = 4 (reads 4 B and writes 5.33 B per pixel)
  ingest           the identity-mode ingest launch on as many BGRA frames (reads 4 B, writes 4 B per pixel)
  corners_rR       the corners call at radius R, nms as given, min_eig 1, cap 4096, into the workspace's score planes
  corners_rR_held  the same with 2048 held points per frame (the fourth launch)
Frame 0 of every corners arm is checked against the host twin before timing. Each arm is timed with device events after a
warm-up; a round replays an arm enough times for --seconds / --rounds of work. Prints one JSON line and appends it to --out
(default profiles/kklt_corners_mi355x.jsonl): the median and min / max per arm over the rounds, and the corners found.
--trace: run every corners arm three times eagerly and exit, for a kernel trace by an outside profiler."""
import argparse
import os

import numpy as np

import karms
import torch

import kklt
import niftymatch_amd as nm

FW, FH, LEVELS = kklt.FW, kklt.FH, kklt.LEVELS
HELD = 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--radii", type=int, nargs="+", default=[3, 7])
    ap.add_argument("--nms", type=int, default=8)
    karms.timing_args(ap, rounds=5, warmup=2, seconds=1.0, trace=True,
                      out=os.path.join(karms.ROOT, "profiles", "kklt_corners_mi355x.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kklt_corners.py measures on a GPU"
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream()
    n = a.frames
    grays = kklt.make_frames(n, dev)[:n]
    bgra = [torch.stack([g, g, g, torch.full_like(g, 255)], -1).to(torch.uint8) for g in grays]
    pyrs, _ = nm.gray_pyramid_batch(grays, levels=LEVELS)
    ws = nm.KltCornersWorkspace(n, FW, FH, dev)
    hx, hy = nm.klt_grid_points(FW, FH, 32)
    hx, hy = hx[:HELD] + np.float32(0.25), hy[:HELD] + np.float32(0.5)
    held = ([torch.from_numpy(hx).to(dev)] * n, [torch.from_numpy(hy).to(dev)] * n,
            [torch.tensor([HELD], dtype=torch.int32, device=dev)] * n)
    outs, arms = {}, {}
    arms["pyramid"] = lambda: nm.gray_pyramid_batch(grays, levels=LEVELS, pyrs=pyrs)
    arms["ingest"] = lambda: nm.ingest_batch(bgra)

    def corners(r, with_held, name):
        outs[name] = nm.klt_corners_batch(grays, radius=r, nms=a.nms, min_eig=1.0, cap=4096, held=held if with_held else None,
                                          out=outs.get(name), workspace=ws)
        return outs[name]

    for r in a.radii:
        for with_held in (False, True):
            name = "corners_r%d%s" % (r, "_held" if with_held else "")
            arms[name] = lambda r=r, with_held=with_held, name=name: corners(r, with_held, name)
    found = {}
    with torch.cuda.stream(stream):
        torch.cuda.synchronize()
        if a.trace:
            for _ in range(3):
                for name, fn in arms.items():
                    if name.startswith("corners"):
                        fn()
            stream.synchronize()
            return
        g0 = grays[0].cpu().numpy()
        for name, fn in arms.items():
            fn()
            stream.synchronize()
            if not name.startswith("corners"):
                continue
            o = outs[name]
            r = int(name.split("_r")[1].split("_")[0])
            h = nm.klt_corners_host([g0], radius=r, nms=a.nms, min_eig=1.0, cap=4096,
                                    held=([hx], [hy], [HELD]) if name.endswith("_held") else None)
            m = int(h["count"][0])
            assert int(o["count"][0]) == m and int(o["total"][0]) == int(h["total"][0]), name
            for key in ("x", "y", "score"):
                assert np.array_equal(o[key][0][:m].cpu().numpy().view(np.uint32), h[key][0][:m].view(np.uint32)), (name, key)
            found[name] = float(o["total"].sum()) / n
    graphs, kept = karms.capture(arms, stream)
    reps, times = karms.time_replays(graphs, stream, a.rounds, a.seconds, a.warmup)
    karms.emit({"tool": "kklt_corners", "frames": n, "frame": [FW, FH], "levels": LEVELS, "nms": a.nms, "held": HELD,
                "rounds": a.rounds, "reps_per_round": reps, **karms.spread(times), "corners_per_frame": found}, a.out)


if __name__ == "__main__":
    main()
