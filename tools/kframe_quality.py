"""Frame quality statistics, keyframe pick and gather (nm_frame_quality_batch_dev, nm_keyframe_pick_dev, nm_slots_gather_dev)
on the GPU, timed as graph replays.

    python tools/kframe_quality.py [--frames 64] [--grids 1 4 8] [--rounds 5] [--seconds 1.0] [--trace]

n 1920x1080 BGRA frames with the disc field of view of tools/kframe_weights.py (its make_frames). Arms, each captured into
a HIP graph once and replayed, alternated round by round in one process on one stream:
  q_G        the statistics call on a G x G grid, no masks (reads 4 B per pixel)
  q_G_u8     the same with U8N masks (5 B per pixel)
  q_G_f32    the same with F32 masks (8 B per pixel)
  pick       the keyframe pick on the masked 4 x 4 statistics and a pan of 12 px per frame, keep = 16
  gather     one gather of the BGRA frames by the pick's keys (16 slots of 8.3 MB, read and written)
  ingest     the identity-mode ingest launch on the same frames (reads 4 B and writes 4 B per pixel): the bandwidth yardstick
lo = 30, hi = 240. The statistics of two frames are checked against the host twin before timing, the pick and the gather
against theirs. Each arm is timed with device events after a warm-up; a round replays an arm enough times for
--seconds / --rounds of work. Prints one JSON line: the median and min / max per arm over the rounds, the bytes each arm
must move at least and that over its time as a fraction of --copy-tbps (default 4.86 TB/s, the device-to-device copy
rate tools/hbm_probe.py reported on the box of the recorded run; run the probe on yours). --trace runs 3 eager calls of each
arm, untimed (for `rocprofv3 --kernel-trace --stats`, in a run of its own; the kernels are frame_quality_kernel,
keyframe_pick_kernel, slots_gather_kernel and the shared zero kernel).
"""
import argparse

import numpy as np

import karms
import torch

import niftymatch_amd as nm
from kframe_weights import FH, FW, make_frames

PARAMS = dict(lo=30, hi=240)
PICK = dict(keep=16, d_min=40.0, d_max=120.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--grids", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--copy-tbps", type=float, default=4.86, help="what tools/hbm_probe.py reports as the d2d copy rate")
    karms.timing_args(ap, rounds=5, warmup=2, seconds=1.0, trace=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kframe_quality.py measures on a GPU"
    assert 1 <= a.frames <= nm.FRAME_QUALITY_MAX_BATCH and all(1 <= g <= nm.FRAME_QUALITY_MAX_GRID for g in a.grids)
    dev = torch.device("cuda:0")
    n, P = a.frames, FW * FH
    frames = make_frames(n, dev)
    m_u8 = nm.frame_weights_batch(frames, lo=30, hi=240, R=8, margin=2, min_count=4, want=("mask",))
    m_f32 = m_u8.to(torch.float32) / 255.0
    masks = {"": None, "_u8": list(m_u8), "_f32": list(m_f32)}
    stats = {(g, s): torch.empty((n, g, g, 8), dtype=torch.int64, device=dev) for g in set(a.grids) | {4} for s in masks}
    chain = torch.tensor([[1, 0, -12.0 * k, 0, 1, 0, 0, 0, 1] for k in range(n)], dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream()
    arms = {}
    for g in a.grids:
        for s, m in masks.items():
            arms["q_%d%s" % (g, s)] = lambda g=g, s=s, m=m: nm.frame_quality_batch(frames, masks=m, grid=(g, g), stats=stats[(g, s)],
                                                                                     **PARAMS)
    nm.frame_quality_batch(frames, masks=masks["_u8"], grid=(4, 4), stats=stats[(4, "_u8")], **PARAMS)
    pick0 = nm.keyframe_pick(stats[(4, "_u8")], chain, FW, FH, **PICK)
    gathered = list(torch.empty((PICK["keep"], FH, FW, 4), dtype=torch.uint8, device=dev))
    arms["pick"] = lambda: nm.keyframe_pick(stats[(4, "_u8")], chain, FW, FH, **PICK)
    arms["gather"] = lambda: nm.slots_gather(pick0.keys, frames, dst=gathered)
    arms["ingest"] = lambda: nm.ingest_batch(frames)
    with torch.cuda.stream(stream):
        torch.cuda.synchronize()
        for g in a.grids:                                # check two frames against the host twin (and load the kernels)
            for s, m in masks.items():
                got = arms["q_%d%s" % (g, s)]()
                stream.synchronize()
                host = nm.frame_quality_host([frames[k].cpu().numpy() for k in (0, n - 1)],
                                             masks=None if m is None else [m[k].cpu().numpy() for k in (0, n - 1)], grid=(g, g), **PARAMS)
                assert np.array_equal(got[[0, n - 1]].cpu().numpy().view(np.uint64), host)
        h_pick = nm.keyframe_pick_host(stats[(4, "_u8")].cpu().numpy(), chain.cpu().numpy(), FW, FH, **PICK)
        assert all(np.array_equal(x.cpu().numpy().view(np.uint8), y.view(np.uint8)) for x, y in zip(pick0, h_pick))
        arms["gather"]()
        stream.synchronize()
        keys = h_pick.keys
        assert all(torch.equal(gathered[i], frames[k]) if k >= 0 else not gathered[i].any() for i, k in enumerate(keys))
        if a.trace:
            for _ in range(3):
                for fn in arms.values():
                    fn()
            torch.cuda.synchronize()
            karms.emit({"tool": "kframe_quality", "frames": n, "trace_calls": 3})
            return
    graphs, kept = karms.capture(arms, stream)
    reps, times = karms.time_replays(graphs, stream, a.rounds, a.seconds, a.warmup)
    sp = karms.spread(times)
    med = sp["median_us"]
    per_pixel = lambda k: 8 if k.endswith("_f32") else (5 if k.endswith("_u8") else 4)
    filled = int((h_pick.keys >= 0).sum())
    model = {k: (2 * n * 4 * P if k == "ingest" else 4 * P * (filled + PICK["keep"]) if k == "gather" else
                 n * 16 * 8 * 8 if k == "pick" else n * per_pixel(k) * P) for k in graphs}
    bw = {k: model[k] / (med[k] * 1e-6) / 1e12 for k in graphs}
    karms.emit({"tool": "kframe_quality", "frames": n, "frame": [FW, FH], "params": PARAMS, "pick": PICK,
                "keys": h_pick.keys.tolist(), "rounds": a.rounds, "reps_per_round": reps, **sp, "model_bytes": model,
                "model_TBps": bw, "fraction_of_copy_rate": {k: b / a.copy_tbps for k, b in bw.items()},
                "copy_TBps": a.copy_tbps})


if __name__ == "__main__":
    main()
