"""Frame masks and feather weights (nm_frame_weights_batch_dev) on the GPU, timed as graph replays.

    python tools/kframe_weights.py [--frames 64] [--radii 8 32 64] [--rounds 5] [--seconds 1.0] [--trace]

n 1920x1080 BGRA frames with a disc field of view (black outside a circle of radius 530 about the centre), mid-range noise
inside it and a few saturated highlights per frame at frame-dependent places. Arms, each captured into a HIP graph once and
replayed, alternated round by round in one process on one stream:
  all_R   the call at radius R with masks (U8N), weights, dist2 and counts
  mw_R    the call at radius R with masks and weights only
  ingest  the identity-mode ingest launch on the same frames (reads 4 B and writes 4 B per pixel): the bandwidth yardstick
lo = 30, hi = 240, margin = 2, min_count = 4, border on. The all_R outputs of one frame are checked against the host twin
before timing. Each arm is timed with device events after a warm-up; a round replays an arm enough times for
--seconds / --rounds of work. Prints one JSON line: the median and min / max per arm over the rounds, the bytes each pass
must move at least (row pass: 4 B read and 1 B of g written per pixel; column pass: 1 B of g read and the outputs written
per pixel; every byte counted once, the column pass's halo rows not at all), and the call's total over its time as a
fraction of --copy-tbps (default 4.86 TB/s, the device-to-device copy rate tools/hbm_probe.py reported on the box of
the recorded run; run the probe on yours). The two passes are one C call, so their separate
times come from a kernel trace only: --trace runs 3 eager calls of each arm, untimed (for `rocprofv3 --kernel-trace --stats`;
the kernels are frame_weights_row_kernel, frame_weights_col_kernel and frame_weights_zero_kernel).
"""
import argparse

import numpy as np

import karms
import torch

import niftymatch_amd as nm

FW, FH = 1920, 1080
PARAMS = dict(lo=30, hi=240, margin=2, min_count=4, border=True)


def make_frames(n, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(FH, device=dev), torch.arange(FW, device=dev), indexing="ij")
    outside = (xx - FW // 2) ** 2 + (yy - FH // 2) ** 2 > 530 ** 2
    rng = np.random.default_rng(0)
    frames = []
    for _ in range(n):
        f = torch.randint(40, 220, (FH, FW, 4), dtype=torch.uint8, device=dev, generator=g)
        f[outside] = 0
        for _ in range(6):
            hx, hy, s = int(rng.integers(500, 1400)), int(rng.integers(200, 860)), int(rng.integers(3, 40))
            f[hy:hy + s, hx:hx + s, :3] = 255
        frames.append(f)
    return frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--radii", type=int, nargs="+", default=[8, 32, 64])
    ap.add_argument("--copy-tbps", type=float, default=4.86, help="what tools/hbm_probe.py reports as the d2d copy rate")
    karms.timing_args(ap, rounds=5, warmup=2, seconds=1.0, trace=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kframe_weights.py measures on a GPU"
    assert 1 <= a.frames <= nm.FRAME_WEIGHTS_MAX_BATCH and all(3 <= R <= nm.FRAME_WEIGHTS_MAX_RADIUS for R in a.radii)
    dev = torch.device("cuda:0")
    n, P = a.frames, FW * FH
    frames = make_frames(n, dev)
    ws = nm.FrameWeightsWorkspace(n, FW, FH, dev)
    stream = torch.cuda.Stream()
    arms = {}
    for R in a.radii:
        arms["all_%d" % R] = lambda R=R: nm.frame_weights_batch(frames, R=R, want=("mask", "wts", "dist2"), counts=True,
                                                               workspace=ws, **PARAMS)
        arms["mw_%d" % R] = lambda R=R: nm.frame_weights_batch(frames, R=R, workspace=ws, **PARAMS)
    arms["ingest"] = lambda: nm.ingest_batch(frames)
    with torch.cuda.stream(stream):
        for R in a.radii:                                # check one frame against the host twin (and load the kernels)
            mask, wts, d2, counts = arms["all_%d" % R]()
            host = nm.frame_weights_host([frames[0].cpu().numpy()], R=R, want=("mask", "wts", "dist2"), counts=True, **PARAMS)
            stream.synchronize()
            assert np.array_equal(mask[0].cpu().numpy(), host[0][0]) and np.array_equal(d2[0].cpu().numpy().view(np.uint16), host[2][0])
            assert np.array_equal(wts[0].cpu().numpy().view(np.uint32), host[1][0].view(np.uint32))
            assert np.array_equal(counts[0].cpu().numpy().view(np.uint64), host[3][0])
        if a.trace:
            for _ in range(3):
                for fn in arms.values():
                    fn()
            torch.cuda.synchronize()
            karms.emit({"tool": "kframe_weights", "frames": n, "trace_calls": 3})
            return
    graphs, kept = karms.capture(arms, stream)
    reps, times = karms.time_replays(graphs, stream, a.rounds, a.seconds, a.warmup)
    sp = karms.spread(times)
    med = sp["median_us"]
    pitch = (FW + 63) // 64 * 64
    row_bytes = n * (4 * P + pitch * FH)
    col_bytes = {"all": n * (pitch * FH + P * (1 + 4 + 2)), "mw": n * (pitch * FH + P * (1 + 4))}
    model = {k: (2 * n * 4 * P if k == "ingest" else row_bytes + col_bytes[k.split("_")[0]]) for k in graphs}
    bw = {k: model[k] / (med[k] * 1e-6) / 1e12 for k in graphs}
    karms.emit({"tool": "kframe_weights", "frames": n, "frame": [FW, FH], "params": PARAMS, "rounds": a.rounds,
                "reps_per_round": reps, **sp, "row_pass_bytes": row_bytes, "col_pass_bytes": col_bytes, "model_bytes": model,
                "model_TBps": bw, "fraction_of_copy_rate": {k: b / a.copy_tbps for k, b in bw.items()}, "copy_TBps": a.copy_tbps})


if __name__ == "__main__":
    main()
