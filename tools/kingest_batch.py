"""Batched frame ingest (nm_frame_ingest_batch_f32) against per-frame launches, on the GPU.

    python tools/kingest_batch.py [--frames 16 64] [--rounds 5] [--seconds 1.0] [--trace]

n random 1920x1080 BGRA frames and one undistortion map from nm_undistort_map_f32 (k1 = -0.12, centred camera). Three
ways to get each frame's undistorted BGRA frame and gray plane, alternated round by round in one process on one stream:
  A  the per-frame channel chain: extract_channel -> cast_f32_u8 -> resample_undistort (U8N) -> put_channel for B, G, R,
     then grayscale (13 launches per frame; the same B, G, R and gray bits as C)
  B  per frame resample_map_u8x4 + grayscale (2 launches per frame)
  C  one ingest call (1 launch)
plus C_gray (one gray-only ingest call) and the identity mode against n grayscale calls (I against G). Outputs are
checked equal before timing. Each arm is timed with device events after a warm-up; a round repeats an arm's call enough
times for --seconds / --rounds of work, and the per-call time of each round is recorded. Prints one JSON line per n with
the median and the min / max over rounds, and the achieved bandwidth against the byte model
8 P + n (4 fw fh + 4 P [+ 4 P undistorted]) per call (P = output pixels) as a fraction of 6.29 TB/s (the copy rate of
this device, tools/hbm_probe.py). --trace runs 3 calls of each arm, untimed (for `rocprofv3 --kernel-trace --stats`).
"""
import argparse
import ctypes as C

import karms
import torch

import niftymatch_amd as nm

FW, FH = 1920, 1080
COPY_TBPS = 6.29


def measure(n, rounds, seconds, warmup, trace, dev, frames_all, u, v):
    stream = torch.cuda.Stream()
    frames = frames_all[:n]
    P = FW * FH
    L = nm.lib()
    st = C.c_void_p(stream.cuda_stream)
    outs = {s: [torch.zeros((FH, FW, 4), dtype=torch.uint8, device=dev) for _ in range(n)] for s in "ABC"}
    grays = {s: [torch.empty((FH, FW), dtype=torch.float32, device=dev) for _ in range(n)] for s in ("A", "B", "C", "C_gray",
                                                                                                     "I", "G")}
    tmp_f = torch.empty((FH, FW), dtype=torch.float32, device=dev)
    tmp_u8 = torch.empty((FH, FW), dtype=torch.uint8, device=dev)
    tmp_r = torch.empty((FH, FW), dtype=torch.float32, device=dev)
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    fptr = arr(frames)
    ptrs = {s: arr(g) for s, g in grays.items()}
    uptr = arr(outs["C"])

    def chk(r):
        assert r == 0, r

    def arm_A():
        for k in range(n):
            for c in range(3):
                chk(L.nm_extract_channel_f32(frames[k].data_ptr(), tmp_f.data_ptr(), FW, FH, c, st))
                chk(L.nm_cast_f32_u8(tmp_f.data_ptr(), FW, FH, tmp_u8.data_ptr(), 0, st))
                chk(L.nm_resample_undistort_f32(tmp_u8.data_ptr(), FW, FH, nm.TEX_U8N, u.data_ptr(), v.data_ptr(), FW, FH,
                                                tmp_r.data_ptr(), st))
                chk(L.nm_put_channel_f32(outs["A"][k].data_ptr(), tmp_r.data_ptr(), FW, FH, c, st))
            chk(L.nm_grayscale_f32(outs["A"][k].data_ptr(), grays["A"][k].data_ptr(), FW, FH, st))

    def arm_B():
        for k in range(n):
            chk(L.nm_resample_map_u8x4(outs["B"][k].data_ptr(), frames[k].data_ptr(), FW, FH, u.data_ptr(), v.data_ptr(),
                                       FW, FH, st))
            chk(L.nm_grayscale_f32(outs["B"][k].data_ptr(), grays["B"][k].data_ptr(), FW, FH, st))

    def arm_C():
        chk(L.nm_frame_ingest_batch_f32(n, fptr, FW, FH, u.data_ptr(), v.data_ptr(), FW, FH, ptrs["C"], uptr, st))

    def arm_C_gray():
        chk(L.nm_frame_ingest_batch_f32(n, fptr, FW, FH, u.data_ptr(), v.data_ptr(), FW, FH, ptrs["C_gray"], None, st))

    def arm_I():
        chk(L.nm_frame_ingest_batch_f32(n, fptr, FW, FH, None, None, FW, FH, ptrs["I"], None, st))

    def arm_G():
        for k in range(n):
            chk(L.nm_grayscale_f32(frames[k].data_ptr(), grays["G"][k].data_ptr(), FW, FH, st))

    arms = {"A": arm_A, "B": arm_B, "C": arm_C, "C_gray": arm_C_gray, "I": arm_I, "G": arm_G}
    if trace:
        with torch.cuda.stream(stream):
            for _ in range(3):
                for fn in arms.values():
                    fn()
        torch.cuda.synchronize()
        return {"tool": "kingest_batch", "frames": n, "trace_calls": 3}
    with torch.cuda.stream(stream):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    i32 = lambda t: t.view(torch.int32)
    for k in range(n):
        assert torch.equal(outs["B"][k], outs["C"][k]) and torch.equal(outs["A"][k][..., :3], outs["C"][k][..., :3])
        for s in ("A", "B", "C_gray"):
            assert torch.equal(i32(grays[s][k]), i32(grays["C"][k])), (s, k)
        assert torch.equal(i32(grays["I"][k]), i32(grays["G"][k])), k
    reps, times = karms.time_replays(arms, stream, rounds, seconds, warmup)
    sp = karms.spread(times)
    med = sp["median_us"]
    bytes_map = 8 * P
    model = {"A": None, "B": None, "C": bytes_map + n * (4 * P + 4 * P + 4 * P), "C_gray": bytes_map + n * (4 * P + 4 * P),
             "I": n * (4 * P + 4 * P), "G": n * (4 * P + 4 * P)}
    model["A"] = model["B"] = model["C"]
    bw = {k: model[k] / (med[k] * 1e-6) / 1e12 for k in arms}
    return {"tool": "kingest_batch", "frames": n, "frame": [FW, FH], "rounds": rounds, "reps_per_round": reps, **sp,
            "launches_per_call": {"A": 13 * n, "B": 2 * n, "C": 1, "C_gray": 1, "I": 1, "G": n},
            "speedup_C_over_A": med["A"] / med["C"], "speedup_C_over_B": med["B"] / med["C"],
            "speedup_I_over_G": med["G"] / med["I"],
            "C_faster_than_A_beyond_spread": max(times["C"]) < min(times["A"]),
            "model_bytes": model, "model_TBps": bw, "fraction_of_copy_rate": {k: b / COPY_TBPS for k, b in bw.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[16, 64])
    karms.timing_args(ap, rounds=5, warmup=2, seconds=1.0, trace=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kingest_batch.py measures on a GPU"
    assert all(1 <= n <= nm.INGEST_MAX_BATCH for n in a.frames)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    frames = [torch.randint(0, 256, (FH, FW, 4), dtype=torch.uint8, device=dev, generator=g) for _ in range(max(a.frames))]
    yy, xx = torch.meshgrid(torch.arange(FH, dtype=torch.float32, device=dev),
                            torch.arange(FW, dtype=torch.float32, device=dev), indexing="ij")
    cam = torch.tensor([0.8 * FW, 0.8 * FW, FW / 2, FH / 2], dtype=torch.float32, device=dev)
    dist = torch.tensor([-0.12, 0.0, 0.0], dtype=torch.float32, device=dev)
    u, v = nm.undistort_map(xx.contiguous(), yy.contiguous(), cam, dist)
    torch.cuda.synchronize()
    for n in a.frames:
        karms.emit(measure(n, a.rounds, a.seconds, a.warmup, a.trace, dev, frames, u, v))


if __name__ == "__main__":
    main()
